#!/usr/bin/env python
"""Device time of the relocaliser (slam/relocalise.py, include/relocalisation.h): gsr_reloc_encode, gsr_reloc_search and gsr_reloc_score at
640 x 480 with the default options (512 ferns on a 40 x 30 grid) and a database of K = 1000 codes, each from device events over --reps
calls after --warmup, in --rounds rounds (median and spread over the rounds); and a whole MapLocaliser.localise() -- query, one or more
candidates of render, alignment, tracking, score, and the host reads of the candidates and the verdict -- on the map of a short synthetic
SLAM run at 320 x 240, by wall clock around a synchronised call, median and spread over the run's non-keyframes. Prints one JSON line and
writes it to --out (default profiles/relocalise.json)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import relocalise  # noqa: E402


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
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4), "n": int(v.size)}


def kernels(W, H, K, reps, warmup, rounds):
    g = torch.Generator(device="cuda").manual_seed(0)
    image, render = (torch.rand((3, H, W), device="cuda", generator=g) for _ in range(2))
    depth, rdepth = (0.3 + 5.7 * torch.rand((H, W), device="cuda", generator=g) for _ in range(2))
    opacity = torch.rand((H, W), device="cuda", generator=g)
    index = relocalise.KeyframeIndex(device="cuda:0", capacity=K)
    index.database.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (K, index.words), device="cuda", generator=g, dtype=torch.int64).to(torch.int32))
    index.ids = list(range(K))
    code = torch.zeros(index.words, dtype=torch.int32, device="cuda")
    best = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    distance = torch.zeros(K, dtype=torch.int32, device="cuda")
    counts = torch.zeros(8, dtype=torch.int32, device="cuda")
    calls = {"encode": lambda: relocalise.encode(image, depth, None, index.grid, index.table, index.depth_scale, code, index._workspace),
             "search": lambda: relocalise.search(index.database, K, code, index.ferns, 0xF, 4, distance, best),
             "score": lambda: relocalise.score_counts(render, rdepth, opacity, image, depth, None, 48, 0.05, counts)}
    return {"resolution": [W, H], "ferns": index.ferns, "grid": list(index.grid), "rows": K, "topk": 4,
            "device_ms": {name: spread([timed(fn, reps, warmup) for _ in range(rounds)]) for name, fn in calls.items()}}


def whole_localise(frames):
    from slam.dataset import SyntheticRGBDDataset
    from slam.map_io import load_map
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=frames, width=320, height=240, seed=0)
    cfg = merge_config(default_config(), {"Training": {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": 60,
                                                       "static_map_iters": 30, "gaussian_update_every": 60, "gaussian_update_offset": 20,
                                                       "tracking_graph": True},
                                          "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 150},
                                          "Results": {"eval_rendering": False}})
    slam = SLAM(cfg, ds)
    slam.run()
    with tempfile.TemporaryDirectory() as tmp:
        slam.save_map(os.path.join(tmp, "map"))
        loaded = load_map(os.path.join(tmp, "map"))
    loc = relocalise.MapLocaliser(loaded, cfg)
    others = [i for i in sorted(slam.frontend.cameras) if i not in slam.frontend.kf_indices]
    ms, tried, accepted = [], [], 0
    for n, i in enumerate(others[:2] + others):                     # the first two calls warm up (allocator, kernels' first launch)
        viewpoint = loc.camera(ds, i)
        viewpoint.update_RT(torch.eye(3), torch.tensor([5.0, -4.0, 6.0]))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loc.localise(viewpoint)
        torch.cuda.synchronize()
        if n >= 2:
            ms.append(1e3 * (time.perf_counter() - t0))
            tried.append(out["candidates_tried"])
            accepted += int(out["accepted"])
    return {"resolution": [320, 240], "frames": len(others), "keyframes": len(loaded.kf_indices), "gaussians": int(loaded.gaussians.get_xyz.shape[0]),
            "accepted": accepted, "candidates_tried": spread(tried), "wall_ms_per_localise": spread(ms),
            "tracking_itr_num": cfg["Training"]["tracking_itr_num"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=40, help="frames of the synthetic run whose map localise() is timed in")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "relocalise.json"))
    args = ap.parse_args()
    doc = {"reps": args.reps, "rounds": args.rounds, "kernels": kernels(640, 480, 1000, args.reps, args.warmup, args.rounds),
           "localise": whole_localise(args.frames), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
