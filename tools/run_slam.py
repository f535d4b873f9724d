#!/usr/bin/env python
"""The SLAM system on a recorded sequence, as the reference's `slam.py --config X.yaml [--eval] [--dynamic]` (slam.py:250-276): the config
(with its inherit_from chain, slam/config.py) names a TUM / Bonn, CoFusion or EuRoC-layout stereo sequence on disk (slam/recorded.py; a stereo
sequence gets its depth from the on-device matcher, slam/stereo.py, and a `stereo` block reports its device ms per frame). Prints the JSON document
of tools/run_slam_demo.py plus an `ingest` block: host decode ms per frame, the time the loop waited for a frame, and how many frames
came from the read-ahead thread vs were decoded on demand. With --dynamic --raft-weights PATH (the reference's pretrained/raft-things.pth) the
dynamic mapping's optical-flow term runs on RAFT's flows (slam/optical_flow.py), and a `flow` block reports the pairs estimated and the
device ms per pair; --gma-weights PATH (a GMA checkpoint, gma-things.pth and its kind) runs the term on GMA's flows instead (RAFT with global
motion aggregation, the reference's second estimator), and the `flow` block's `estimator` says which. With --yolo-weights PATH (the reference's pretrained/yolov9e-seg.pt) every frame is segmented as the reference's loaders do
(slam/segmentation.py), static and dynamic runs alike, and a `segmentation` block reports the frames segmented and the device ms per frame.
With --flow-masks (needs --dynamic and one of --raft-weights / --gma-weights) every frame's motion mask also loses what its flow to a
partner frame and its depth cannot explain as one camera motion, whatever its class (slam/motion_segmentation.py), and a
`motion_segmentation` block reports the frames segmented, the device ms per frame of the fit and of the cleaning, the mean moving share
and the mean cutoff; the flow pair this adds per frame is the dominant cost and is counted in the `flow` block.
With --lpips-weights ALEXNET.pth LIN.pth (a torchvision AlexNet state_dict and the LPIPS v0.1 linear layers) the rendering evaluation
reports `mean_lpips` as well (slam/perceptual.py), and an `lpips` block reports the pairs scored and the device ms per pair.
`Dataset.sensor_type: monocular` runs on the images alone (a sequence whose Calibration has no depth_scale is read without depth files; the
ATE is scale-aligned); it cannot be combined with --dynamic.
A `Training.loop_closure` block in the YAML (`enabled: true` and any key of slam/stages.py LOOP_CLOSURE_DEFAULTS) ties every new keyframe
to old keyframes of the same place and corrects poses and map (slam/loop_closure.py; static RGB-D and stereo runs only, refused with --dynamic
and for monocular input), and a `loop_closure` block reports the keyframes queried, the edges accepted and the corrections applied.
With --video PATH --calibration fx fy cx cy [k1 k2 p1 p2 k3] the input is a plain video with no ground truth: a Motion-JPEG AVI file, or a
folder of .jpg files with --size W H (`Dataset.type: video`, slam/recorded.py VideoDataset; the pictures are decoded on the device,
include/video_io.h gsr_jpeg_decode). Without --config a minimal monocular configuration is built in memory; a --config whose Dataset.type is
`video` works as for any other type. Such a run reports `ate_rmse: null`, writes `trajectory.txt` (TUM format, camera to world) into its
save directory, and its `ingest` block has the device decode time per frame.
With --save-map [DIR] the finished map is saved after the evaluations (slam/map_io.py) for tools/play_map.py."""
import argparse
import json
import os
import sys
import warnings
from datetime import datetime

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam.config import apply_cli_overrides, load_config  # noqa: E402
from slam.recorded import load_dataset  # noqa: E402
from slam.system import SLAM, default_config, merge_config  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default=None, help="YAML configuration (required unless --video is given)")
    ap.add_argument("--video", default=None, metavar="PATH", help="a Motion-JPEG AVI file or a folder of .jpg files: run on it without ground truth")
    ap.add_argument("--calibration", type=float, nargs="+", default=None, metavar="V", help="fx fy cx cy [k1 k2 p1 p2 k3] of --video")
    ap.add_argument("--size", type=int, nargs=2, default=None, metavar=("W", "H"), help="picture size of a --video folder (an AVI file states its own)")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--dynamic", action="store_true", default=False)
    ap.add_argument("--dataset-path", default=None, help="overrides Dataset.dataset_path")
    ap.add_argument("--frames", type=int, default=None, help="use the first N frames (after Calibration start / end)")
    ap.add_argument("--save-dir", default=None, help="where results go (default: slam.py's Results.save_dir/<scene>/<name>_<time>)")
    ap.add_argument("--prefetch", type=int, default=4, help="frames decoded ahead of the loop")
    est = ap.add_mutually_exclusive_group()
    est.add_argument("--raft-weights", default=None, help="RAFT-basic checkpoint (raft-things.pth): the flow term of --dynamic runs")
    est.add_argument("--gma-weights", default=None, help="GMA checkpoint (gma-things.pth): the flow term of --dynamic runs, on GMA's flows")
    ap.add_argument("--yolo-weights", default=None, help="YOLO-seg checkpoint (yolov9e-seg.pt): motion masks of people and the "
                                                         "loader's object classes")
    ap.add_argument("--flow-masks", action="store_true", default=False,
                    help="segment moving regions of any class from flow and depth (needs --dynamic and --raft-weights or --gma-weights)")
    ap.add_argument("--lpips-weights", nargs=2, default=None, metavar=("ALEXNET", "LIN"),
                    help="torchvision AlexNet state_dict and LPIPS v0.1 linear layers: mean_lpips in the rendering evaluation")
    ap.add_argument("--save-map", nargs="?", const="", default=None, metavar="DIR",
                    help="after the evaluations, save the map for tools/play_map.py (default DIR: <save dir>/map)")
    args = ap.parse_args(argv)
    if args.config is None and args.video is None:
        ap.error("one of --config and --video is required")
    if args.video is not None and args.config is None:
        if args.calibration is None or len(args.calibration) not in (4, 9):
            ap.error("--video needs --calibration fx fy cx cy [k1 k2 p1 p2 k3]")
        if args.dynamic:
            ap.error("--video is monocular input and cannot run with --dynamic: the dynamic model is seeded from sensor depth")
    elif args.calibration is not None or args.size is not None:
        ap.error("--calibration and --size belong to --video without --config (a configuration file carries its own Calibration)")
    if args.flow_masks and not (args.dynamic and (args.raft_weights or args.gma_weights)):
        ap.error("--flow-masks needs --dynamic and one of --raft-weights / --gma-weights: the masks are segmented from the estimated flow")
    if args.raft_weights and not args.dynamic:
        warnings.warn("--raft-weights only serves the flow term of --dynamic runs; ignored")
        args.raft_weights = None
    if args.gma_weights and not args.dynamic:
        warnings.warn("--gma-weights only serves the flow term of --dynamic runs; ignored")
        args.gma_weights = None
    if args.yolo_weights and not os.path.isfile(args.yolo_weights):
        ap.error(f"--yolo-weights {args.yolo_weights}: no such file")
    for path in args.lpips_weights or ():
        if not os.path.isfile(path):
            ap.error(f"--lpips-weights {path}: no such file")
    return args


def video_config(path, calibration, size=None):
    """A minimal monocular configuration for a plain video: default_config() with Dataset.type 'video' and the given calibration. The size
    comes from the AVI header, or from `size` for a folder."""
    from slam.jpeg_decode import open_source
    info = open_source(path).info
    if "width" in info:
        width, height = info["width"], info["height"]
    elif size is not None:
        width, height = size
    else:
        raise SystemExit(f"--video {path}: a folder of JPEG files needs --size W H")
    names = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
    c = dict(zip(names, [float(v) for v in calibration] + [0.0] * (9 - len(calibration))), width=int(width), height=int(height))
    c["distorted"] = any(c[k] != 0.0 for k in names[4:])
    return merge_config(default_config(), {"Dataset": {"type": "video", "sensor_type": "monocular", "dataset_path": path, "Calibration": c}})


def main(argv=None):
    args = parse_args(argv)

    if args.config is None:
        config = apply_cli_overrides(video_config(args.video, args.calibration, args.size), eval=args.eval, dynamic=False)
    else:
        config = apply_cli_overrides(load_config(args.config), eval=args.eval, dynamic=args.dynamic)
    if args.video and args.config:
        config["Dataset"]["dataset_path"] = args.video
    if args.dataset_path:
        config["Dataset"]["dataset_path"] = args.dataset_path
    if config["Dataset"].get("sensor_type") == "monocular" and config["model_params"]["dynamic_model"]:
        raise SystemExit("Dataset.sensor_type 'monocular' cannot run with model_params.dynamic_model (--dynamic): the dynamic model is seeded "
                         "from sensor depth")
    save_dir = args.save_dir
    if save_dir is None and config["Results"]["save_results"]:          # slam.py:278-285
        path = config["Dataset"]["dataset_path"].rstrip("/").split("/")
        stamp = datetime.now().strftime("%Y-%m-%d-%H-%M-%S")
        save_dir = os.path.join(config["Results"]["save_dir"], "_".join(path[-3:-1]), path[-1] + "_" + stamp)
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "config.json"), "w") as f:
            json.dump(config, f, indent=1, default=str)
    torch.manual_seed(0)
    flow = None
    if args.raft_weights:
        from slam.optical_flow import RaftFlow
        flow = RaftFlow.from_checkpoint(args.raft_weights, "cuda:0")
    elif args.gma_weights:
        from slam.optical_flow import GmaFlow
        flow = GmaFlow.from_checkpoint(args.gma_weights, "cuda:0")
    segmenter = None
    if args.yolo_weights:
        from slam.segmentation import YoloSeg
        segmenter = YoloSeg.from_checkpoint(args.yolo_weights, "cuda:0")
    lpips = None
    if args.lpips_weights and not config["Results"].get("eval_rendering", True):
        warnings.warn("--lpips-weights only serves the rendering evaluation (Results.eval_rendering, or --eval); ignored")
    elif args.lpips_weights:
        from slam.perceptual import Lpips
        lpips = Lpips.from_checkpoints(*args.lpips_weights, device="cuda:0")
    extra = {}
    if args.flow_masks:
        from slam.motion_segmentation import FlowMotionSegmenter
        extra["motion_segmenter"] = FlowMotionSegmenter(gap=int(config["Training"].get("kf_interval", 5)))
    ds = load_dataset(config, "cuda:0", prefetch=args.prefetch, max_frames=args.frames, flow=flow, segmenter=segmenter, **extra)
    slam = SLAM(config, ds, save_dir=save_dir, lpips=lpips)
    res = slam.run()
    if args.save_map is not None:
        res = dict(res, saved_map=slam.save_map(args.save_map or None))
    res["graph_stats"] = slam.frontend.graph_stats
    res["mapping_graph_stats"] = {"static": dict(getattr(slam.backend, "graph_stats", {}) or {}),
                                  "dynamic": dict(getattr(slam.backend, "dynamic_graph_stats", {}) or {}),
                                  "initialize_map": dict(getattr(slam.backend, "init_graph_stats", {}) or {}),
                                  "initialize_network": dict(getattr(slam.backend, "network_init_graph_stats", {}) or {})}
    res["resolution"] = [ds.width, ds.height]
    res["ingest"] = ds.ingest_stats
    if hasattr(ds, "stereo_stats"):
        res["stereo"] = ds.stereo_stats
    if flow is not None:
        res["flow"] = dict(ds.flow_stats, estimator="gma" if args.gma_weights else "raft")
    if segmenter is not None:
        res["segmentation"] = ds.segmentation_stats
    if args.flow_masks:
        res["motion_segmentation"] = ds.motion_segmentation_stats
    if lpips is not None:
        res["lpips"] = lpips.stats
    ds.close()
    name = os.path.splitext(os.path.basename(args.config or args.video.rstrip("/")))[0] + ("_dynamic" if args.dynamic else "")
    print(json.dumps({name: res}, indent=1, default=str))


if __name__ == "__main__":
    main()
