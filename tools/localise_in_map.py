#!/usr/bin/env python
"""Localise the frames of a sequence in a saved map (slam/map_io.py) without a start pose (slam/relocalise.py MapLocaliser.follow):
  localise_in_map.py --map DIR --synthetic [--frames N] [--first I] [--size WxH] [--trajectory FILE]
  localise_in_map.py --map DIR --config YAML [--dataset-path DIR] [--frames N] [--first I] [--trajectory FILE]
The first frame is found from nothing among the map's keyframes, every later one is tracked from the previous pose, judged against the map
and found again when the verdict refuses it. --synthetic reads the synthetic demo's dataset (tools/run_slam_demo.py), --config a recorded
sequence as tools/run_slam.py does; the YAML's Training.relocalisation block is read whether or not it is enabled. Prints one JSON line:
the frames, their status (localised | tracked | relocalised | lost), the counts of each and the ATE where the dataset has ground truth;
--trajectory writes the world-to-camera poses as `frame r00 .. r22 tx ty tz` lines. Static maps only; the map is not modified."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map", required=True, help="directory written by SLAM.save_map / run_slam.py --save-map")
    source = ap.add_mutually_exclusive_group(required=True)
    source.add_argument("--synthetic", action="store_true", help="the synthetic demo's sequence")
    source.add_argument("--config", default=None, help="YAML of a recorded sequence (tools/run_slam.py)")
    ap.add_argument("--dataset-path", default=None, help="overrides Dataset.dataset_path")
    ap.add_argument("--frames", type=int, default=40, help="frames to localise")
    ap.add_argument("--first", type=int, default=0, help="the first of them")
    ap.add_argument("--size", default=None, help="WxH of the synthetic frames (default: the map's)")
    ap.add_argument("--trajectory", default=None, help="write the poses to this file")
    ap.add_argument("--feature-solver", choices=("points", "pnp"), default="points", help="with --feature-seed: the pose from both frames' depths "
                    "(points) or from the map's depth and the frame's pixels alone (pnp), which needs no depth of the frame")
    ap.add_argument("--feature-seed", action="store_true", help="start each candidate's alignment at the pose of matched features "
                    "(Training.feature_seed); the synthetic frames then carry the blocks texture, as the map must")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    import torch
    from slam.map_io import load_map
    from slam.relocalise import MapLocaliser
    from slam.system import default_config, merge_config
    loaded = load_map(args.map, args.device)
    torch.manual_seed(0)
    if args.synthetic:
        from slam.dataset import SyntheticRGBDDataset
        W, H = (int(v) for v in args.size.lower().split("x")) if args.size else (int(loaded.meta["width"]), int(loaded.meta["height"]))
        ds = SyntheticRGBDDataset(num_frames=args.first + args.frames, width=W, height=H, seed=0, spacing=None if args.feature_seed else (0.025 if W > 320 else 0.03), device=args.device,
                                  texture="blocks" if args.feature_seed else "smooth")
        config = merge_config(default_config(), {"Training": {"tracking_itr_num": 60}})
    else:
        from slam.config import apply_cli_overrides, load_config
        from slam.recorded import load_dataset
        config = apply_cli_overrides(load_config(args.config))
        if args.dataset_path:
            config["Dataset"]["dataset_path"] = args.dataset_path
        ds = load_dataset(config, args.device, max_frames=args.first + args.frames)
    if args.feature_seed:
        config = merge_config(config, {"Training": {"feature_seed": {"enabled": True, "solver": args.feature_solver}}})
    frames = list(range(args.first, min(len(ds), args.first + args.frames)))
    out = MapLocaliser(loaded, config).follow(ds, frames)
    if args.trajectory:
        with open(args.trajectory, "w", encoding="utf-8") as f:
            for i, pose in zip(out["frames"], out["poses"].tolist()):
                f.write(" ".join([str(i)] + [repr(v) for row in pose[:3] for v in row[:3]] + [repr(row[3]) for row in pose[:3]]) + "\n")
    status = out["status"]
    print(json.dumps({"map": args.map, "frames": out["frames"], "status": status, "counts": {s: status.count(s) for s in sorted(set(status))},
                      "ate_rmse": out["ate_rmse"], "keyframes": len(loaded.kf_indices), "gaussians": int(loaded.gaussians.get_xyz.shape[0]),
                      "trajectory": args.trajectory, **{k: out[k] for k in ("feature_seeds_tried", "feature_seeds_accepted") if k in out}}))


if __name__ == "__main__":
    main()
