#!/usr/bin/env python
"""Device time of the motion segmenter (slam/motion_segmentation.py) on one 640 x 480 frame: the rigid fit (gsr_flow_rigid_fit, stage A) and
the mask cleaning (gsr_motion_mask_clean, stage B) separately, from device events over --reps calls after --warmup, with the number of
launches each stage enqueues. The input is seeded: a slanted wall and a floor seen by a camera that moves by a small twist, a box that
moves on its own over about a sixth of the frame, Gaussian flow noise of 0.2 px and 5 % depth holes. Prints one JSON line and writes it to
--out (default profiles/motion_segmentation.json). The flow pair a recorded sequence needs per frame is not part of this figure: it is
what tools/bench_raft.py measures, and it is the larger cost."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import motion_segmentation as ms  # noqa: E402
from slam.camera import SE3_exp  # noqa: E402


def scene(W, H, seed=0, noise_px=0.2, holes=0.05):
    """(flow_ij [H, W, 2] float32 NDC, depth [H, W] float32, intrinsics, the mover's pixels)."""
    rng = np.random.default_rng(seed)
    s = W / 640.0
    fx, fy, cx, cy = 535.4 * s, 539.2 * s, 320.1 * s, 247.6 * s
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    a, b = (u - cx) / fx, (v - cy) / fy
    z = np.minimum(3.0 / (1.0 - 0.3 * a), np.where(b > 0, 0.8 / np.maximum(b, 1e-9), np.inf))
    box = (np.abs(a + 0.15) < 0.22) & (np.abs(b - 0.05) < 0.2)
    z = np.where(box, 1.9, z)
    X = np.stack([a * z, b * z, z], -1) + box[..., None] * np.array([0.06, -0.02, 0.015])
    T = SE3_exp(torch.tensor([0.03, -0.01, 0.02, 0.004, -0.0175, 0.003], dtype=torch.float64)).numpy()
    Y = X @ T[:3, :3].T + T[:3, 3]
    flow = np.stack([fx * Y[..., 0] / Y[..., 2] + cx - u, fy * Y[..., 1] / Y[..., 2] + cy - v], -1) + rng.normal(0, noise_px, (H, W, 2))
    depth = np.where(rng.random((H, W)) < holes, 0.0, z)
    return (flow * np.array([2.0 / W, 2.0 / H])).astype(np.float32), depth.astype(np.float32), (fx, fy, cx, cy), box


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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "motion_segmentation.json"))
    args = ap.parse_args()
    W, H = args.width, args.height
    flow_h, depth_h, K, box = scene(W, H)
    flow, depth = torch.tensor(flow_h).cuda(), torch.tensor(depth_h).cuda()
    seg = ms.FlowMotionSegmenter()
    lib = ms._C.load_library()
    ws_fit = torch.empty(int(lib.gsr_flow_rigid_fit_workspace_size(W, H)), dtype=torch.uint8, device="cuda")
    ws_clean = torch.empty(int(lib.gsr_motion_mask_clean_workspace_size(W, H)), dtype=torch.uint8, device="cuda")
    fit = lambda: ms.flow_rigid_fit(flow, depth, K, workspace=ws_fit, **seg.fit_params)
    cand = fit()["candidate"]
    clean = lambda: ms.motion_mask_clean(cand, workspace=ws_clean, **seg.clean_params)
    fit_ms, clean_ms = timed(fit, args.reps, args.warmup), timed(clean, args.reps, args.warmup)
    both_ms = timed(lambda: seg.segment(flow, depth, K), args.reps, args.warmup)
    out = seg.segment(flow, depth, K)
    moving = out["moving"].bool().cpu().numpy()
    doc = {"resolution": [W, H], "reps": args.reps, **seg.fit_params, **seg.clean_params,
           "fit_device_ms": round(fit_ms, 4), "clean_device_ms": round(clean_ms, 4), "segment_device_ms": round(both_ms, 4),
           "fit_launches": 3 * seg.fit_params["iters"] + 3, "fit_memset_nodes": 1, "clean_launches": 8,
           "cutoff_px": float(out["stats"][0].item()), "usable_share": float(out["stats"][1].item()) / (W * H),
           "mover_share": float(box.mean()), "moving_share": float(moving.mean()), "mover_recall": float((moving & box).sum() / box.sum()),
           "workspace_MB": round((ws_fit.numel() + ws_clean.numel()) / 1e6, 2), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
