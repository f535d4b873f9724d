#!/usr/bin/env python
"""BASELINE config #4 in its asset-free form: the whole SLAM system (slam/system.py) on the synthetic RGB-D sequence (slam/dataset.py),
static and dynamic, eager tracking and hipGraph tracking; prints ATE / PSNR / fps as one JSON document. With --monocular the static
sequence runs with its depth withheld (Dataset.sensor_type 'monocular': every frame's depth is None; the ATE is scale-aligned); with
--mono-sweep as well, new keyframes are seeded from a plane sweep over the window (Training.mono_sweep, slam/sweep.py) and the result has a
`sweep` block. With --pose-prior every frame's tracking starts from the dense frame-to-frame alignment (Training.pose_prior,
slam/odometry.py) and the result has an `odometry` block; --tracking-itr N sets Training.tracking_itr_num (default 60): a prior is worth
most where the tracker is given few iterations. --pose-prior-terms (implies --pose-prior) turns on Training.pose_prior_terms with its defaults:
the alignment's affine brightness and depth term; --pose-prior-against keyframe aligns against the last keyframe, not the previous frame.
--loop-closure turns on Training.loop_closure with its defaults on the static scenarios (a dynamic model is refused) and the result has a
`loop_closure` block; the demo's arc never returns to a place, so it shows the cost of the stage, not a correction. --feature-seed (with
--loop-closure) turns on Training.feature_seed and gives the room the blocks texture, which has corners to find; --feature-solver pnp
makes it the pose from 2D-3D matches, the one a --monocular run can use (with a Training.relocalisation block: loop closure is refused
for monocular input)."""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam.dataset import SyntheticRGBDDataset  # noqa: E402
from slam.system import SLAM, default_config, merge_config  # noqa: E402

# --only <substring>: run the matching scenarios only; --profile: cProfile each run and print the 25 most expensive functions to stderr;
# --save-map DIR: after a scenario's evaluations, save its map to DIR/<scenario> (slam/map_io.py) for tools/play_map.py
save_map = sys.argv[sys.argv.index("--save-map") + 1] if "--save-map" in sys.argv else None
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
profile = "--profile" in sys.argv
monocular = "--monocular" in sys.argv
mono_sweep = "--mono-sweep" in sys.argv
pose_prior = "--pose-prior" in sys.argv
pose_prior_terms = "--pose-prior-terms" in sys.argv      # implies --pose-prior; --pose-prior-against keyframe aligns against keyframes
pose_prior = pose_prior or pose_prior_terms
pose_prior_against = sys.argv[sys.argv.index("--pose-prior-against") + 1] if "--pose-prior-against" in sys.argv else "previous"
loop_closure = "--loop-closure" in sys.argv
feature_seed = "--feature-seed" in sys.argv               # needs --loop-closure (or a Training.relocalisation block); the blocks texture
feature_solver = sys.argv[sys.argv.index("--feature-solver") + 1] if "--feature-solver" in sys.argv else "points"      # points | pnp
tracking_itr = int(sys.argv[sys.argv.index("--tracking-itr") + 1]) if "--tracking-itr" in sys.argv else 60
out = {}
scenarios = (("static_640x480_eager", False, False, 40, (640, 480)), ("static_640x480_graph", False, True, 40, (640, 480)),
             ("dynamic_320x240_eager", True, False, 36, (320, 240)), ("dynamic_320x240_graph", True, True, 36, (320, 240)),
             ("dynamic_640x480_graph", True, True, 36, (640, 480)))
if monocular:
    scenarios = (("monocular_sweep_320x240_graph" if mono_sweep else "monocular_320x240_graph", False, True, 40, (320, 240)),)
for name, dyn, graph, frames, wh in scenarios:
    if only not in name or (loop_closure and dyn):
        continue
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=frames, width=wh[0], height=wh[1], seed=0, dynamic=dyn, dystart=6 if dyn else None, spacing=None if feature_seed else (0.025 if wh[0] > 320 else 0.03),
                              sensor_depth=not monocular, texture="blocks" if feature_seed else "smooth")
    cfg = merge_config(default_config(), {"Training": {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": tracking_itr,
                                                       "static_map_iters": 30, "dynamic_map_iters": 80, "network_init_iters": 50, "gaussian_update_every": 60,
                                                       "gaussian_update_offset": 20, "tracking_graph": graph,
                                                       "fused_grad_accumulation": os.environ.get("GSR_FUSED_ACC", "1") == "1",
                                                       "loss_values": os.environ.get("GSR_LOSS_VALUES", "0") == "1"},
                                          "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 150},
                                          "model_params": {"dynamic_model": dyn}})
    if monocular:      # (kf_interval 2, window 4: the window fills -- and the map counts as initialised -- within the 40 frames)
        cfg = merge_config(cfg, {"Dataset": {"sensor_type": "monocular"}, "Training": {"kf_interval": 2, "window_size": 4}})
        if mono_sweep:
            cfg = merge_config(cfg, {"Training": {"mono_sweep": {"enabled": True}}})
    if pose_prior:
        cfg = merge_config(cfg, {"Training": {"pose_prior": {"enabled": True}}})
    if pose_prior_terms:
        cfg = merge_config(cfg, {"Training": {"pose_prior_terms": {"enabled": True, "against": pose_prior_against}}})
    if loop_closure:
        cfg = merge_config(cfg, {"Training": {"loop_closure": {"enabled": True}}})
    if feature_seed:
        cfg = merge_config(cfg, {"Training": {"feature_seed": {"enabled": True, "solver": feature_solver}}})
    for i in range(len(ds)):          # the sensor stream is "pre-recorded": rendering the synthetic frames is not part of the SLAM time
        ds[i]
    slam = SLAM(cfg, ds)
    if profile:
        import cProfile
        import pstats
        pr = cProfile.Profile()
        res = pr.runcall(slam.run)
        pstats.Stats(pr, stream=sys.stderr).sort_stats("cumulative").print_stats(25)
        pstats.Stats(pr, stream=sys.stderr).sort_stats("tottime").print_stats(20)
    else:
        res = slam.run()
    if save_map:
        res = dict(res, saved_map=slam.save_map(os.path.join(save_map, name)))
    res["graph_stats"] = slam.frontend.graph_stats
    res["mapping_graph_stats"] = {"static": dict(getattr(slam.backend, "graph_stats", {}) or {}), "dynamic": dict(getattr(slam.backend, "dynamic_graph_stats", {}) or {}),
                              "initialize_map": dict(getattr(slam.backend, "init_graph_stats", {}) or {}),
                              "initialize_network": dict(getattr(slam.backend, "network_init_graph_stats", {}) or {})}
    res["resolution"] = list(wh)
    out[name] = res
print(json.dumps(out, indent=1))
