#!/usr/bin/env python
"""Device time of the calls of include/feature_matching.h (slam/features.py) and of what uses them. gsr_feat_extract, gsr_feat_match,
gsr_feat_pose and gsr_feat_pose_pnp (the same pairs without B's depth) at 640 x 480 (cell 32, 4 per cell: 1200 slots) and at 320 x 240 (cell 16, 4 per cell: 1200 slots) on the analytic scene
of tests/features_reference.py (the `wide` pair); LoopCloser.verify on that pair at 320 x 240 with and without the seed (the one host read
of a verify is inside its window); and -- on the synthetic room with the blocks texture, camera steps of DESIGN.md's loop-verification
table (step 0.02, rot_step 0.012), points at --spacing (default: 3, 1.5 and 1 cm) -- the share of pairs (i, i + gap), i = 0 .. 6, whose
stored poses claim the identity between them, that verify accepts with and without the seed, per gap. With --map DIR (a map saved from a blocks-texture run, tools/run_slam_demo.py
--feature-seed --save-map) also MapLocaliser.localise per frame with and without. Each time from device events over --reps calls after
--feature-solver {points,pnp}: the solver of the seeded verify and localise runs (pnp: no depth of the second frame is used); --calls-only
stops after the calls. --warmup, in --rounds rounds (median and spread over the rounds); the device's name and clock are in the output. Prints one JSON line and
writes it to --out (default profiles/features.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
from slam import features  # noqa: E402
from slam.stages import loop_closure_options  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": round(float(np.median(v)), 5), "min": round(float(v.min()), 5), "max": round(float(v.max()), 5), "n": int(v.size)}


class Frame:
    """What LoopCloser.verify reads of a camera; the stored pose is the identity"""

    def __init__(self, image, depth, dev):
        self.original_image, self._depth = torch.as_tensor(np.array(image.cpu() if torch.is_tensor(image) else image)).to(dev), torch.tensor(np.array(depth, np.float32)).to(dev)
        self.R, self.T = torch.eye(3, device=dev), torch.zeros(3, device=dev)

    def depth_device(self):
        return self._depth


def closer(frames, size, K, seed_block, dev):
    from slam.loop_closure import LoopCloser
    seed = None
    if seed_block is not None:
        seed = features.feature_seed_options({"loop_closure": {"enabled": True}, "feature_seed": {"enabled": True, **seed_block}})
    return LoopCloser(loop_closure_options({"loop_closure": {"enabled": True}}), frames, lambda: None, size, K, dev, feature_seed=seed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--map", default=None)
    ap.add_argument("--spacing", type=float, nargs="+", default=[0.03, 0.015, 0.01])
    ap.add_argument("--feature-solver", choices=features.SOLVERS, default="points")
    ap.add_argument("--calls-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "features.json"))
    args = ap.parse_args()
    import features_reference as ref
    dev = "cuda:0"
    prop = torch.cuda.get_device_properties(0)
    out = {"device": prop.name, "clock_mhz": getattr(prop, "clock_rate", 0) / 1000.0, "compute_units": prop.multi_processor_count,
           "reps": args.reps, "rounds": args.rounds, "feature_solver": args.feature_solver, "calls": [], "verify": {}, "baselines": []}
    rounds = lambda fn: spread([timed(fn, args.reps, args.warmup) for _ in range(args.rounds)])
    for (W, H), cell in (((640, 480), 32), ((320, 240), 16)):
        image_a, depth_a, image_b, depth_b, K, _ = ref.scene("wide", W, H)
        opt = features.default_options(cell=cell, per_cell=4)
        seeder = features.FeatureSeeder((W, H), K, opt, dev)
        ia, ib, da, db = (torch.tensor(v).to(dev) for v in (image_a, image_b, depth_a, depth_b))
        a, b = seeder.features(ia), seeder.features(ib)
        T, stats = seeder.pose(a, da, b, db)
        matches, ws = seeder._matches, seeder._workspace
        Tb, sb = torch.empty((4, 4), device=dev), torch.empty(8, dtype=torch.int32, device=dev)
        gate = dict(seed=opt["seed"], hypotheses=opt["hypotheses"], tau_px=opt["tau_px"], refine_iters=opt["refine_iters"],
                    min_matches=opt["min_matches"], min_inliers=opt["min_inliers"], min_share=opt["min_share"], max_translation=opt["max_translation"],
                    max_rotation=np.deg2rad(opt["max_rotation"]), workspace=ws)
        features.pose_pnp(a[0], da, b[0], matches, seeder.K, seeder.K, Tb, sb, **gate)
        out["calls"].append({"size": [W, H], "slots": seeder.slots, "stats": dict(zip(features.STATS, stats.tolist())),
                             "stats_pnp": dict(zip(features.STATS, sb.tolist())),
                             "extract_ms": rounds(lambda: seeder.features(ia)),
                             "match_ms": rounds(lambda: features.match(a[0], a[1], b[0], b[1], opt["max_distance"], opt["ratio_eighths"], matches, ws)),
                             "pose_ms": rounds(lambda: features.pose(a[0], da, b[0], db, matches, seeder.K, seeder.K, Tb, sb,
                                                                     tau_depth=opt["tau_depth"], **gate)),
                             "pose_pnp_ms": rounds(lambda: features.pose_pnp(a[0], da, b[0], matches, seeder.K, seeder.K, Tb, sb, **gate))})
    if args.calls_only:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
        print(json.dumps(out))
        return
    solver = {"solver": args.feature_solver}
    W, H = 320, 240
    image_a, depth_a, image_b, depth_b, K, _ = ref.scene("wide", W, H)
    frames = {0: Frame(image_a, depth_a, dev), 1: Frame(image_b, depth_b, dev)}
    for name, block in (("without_seed", None), ("with_seed", {"cell": 16, "per_cell": 4, **solver})):
        c = closer(frames, (W, H), K, block, dev)
        ok, _, info = c.verify(0, 1)
        out["verify"][name] = {"accepted": bool(ok), "info": info, "device_ms": rounds(lambda: c.verify(0, 1))}
    from slam.dataset import SyntheticRGBDDataset
    for spacing in args.spacing:
        ds = SyntheticRGBDDataset(num_frames=28, width=W, height=H, seed=0, step=0.02, rot_step=0.012, texture="blocks", device=dev, spacing=spacing)
        room = {i: Frame(ds[i][0], ds[i][1], dev) for i in range(len(ds))}
        Kd = (ds.fx, ds.fy, ds.cx, ds.cy)
        with_seed, without = closer(room, (W, H), Kd, {"cell": 16, "per_cell": 4, **solver}, dev), closer(room, (W, H), Kd, None, dev)
        keypoints = int((with_seed.seeder.cached(0, room[0].original_image)[0][:, 0] >= 0).sum())
        for gap in (4, 8, 12, 20):
            pairs = [(i, i + gap) for i in range(7)]
            results = [with_seed.verify(i, j) for i, j in pairs]
            out["baselines"].append({"spacing": spacing, "gap": gap, "pairs": len(pairs), "keypoints_frame0": keypoints,
                                     "accepted_without": sum(bool(without.verify(i, j)[0]) for i, j in pairs),
                                     "accepted_with": sum(bool(r[0]) for r in results),
                                     "seeds_accepted": sum(bool(r[2]["seeded"]) for r in results)})
    if args.map:
        from slam.map_io import load_map
        from slam.relocalise import MapLocaliser
        from slam.system import default_config, merge_config
        loaded = load_map(args.map, dev)
        frames_ds = SyntheticRGBDDataset(num_frames=40, width=int(loaded.meta["width"]), height=int(loaded.meta["height"]), seed=0, texture="blocks", device=dev)
        out["localise"] = {}
        for name, on in (("without_seed", False), ("with_seed", True)):
            loc = MapLocaliser(loaded, merge_config(default_config(), {"Training": {"tracking_itr_num": 60, "feature_seed": {"enabled": on, **solver}}}))
            ms, found = [], 0
            for i in range(1, 40, 4):
                viewpoint = loc.camera(frames_ds, i)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                found += bool(loc.localise(viewpoint)["accepted"])
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            out["localise"][name] = {"frames": len(ms), "found": found, "ms": spread(ms[1:])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
