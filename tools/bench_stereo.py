#!/usr/bin/env python
"""Device time of one stereo depth call (slam/stereo.py StereoMatcher: rectify, census, eight path launches, selection, depth) at 752 x 480
for 64 and 128 disparities, from device events over --reps calls after --warmup, with and without rectification maps; and the host side of
one frame as EurocDataset does it (upload of the pair, the call, the depth copy to pinned memory and the wait for it). The pair is a
blurred-noise scene of two depth layers. Prints one JSON line and writes it to --out (default profiles/stereo.json)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import stereo  # noqa: E402


def scene(H, W, seed=0, near=40, far=8):
    """A left / right pair of 8-bit grey images: blurred noise, a central rectangle at disparity `near` on a background at `far`."""
    rng = np.random.default_rng(seed)

    def texture():
        t = np.pad(rng.uniform(0, 1, (H, W + near)), 2, mode="edge")
        b = sum(t[i:i + H, j:j + W + near] for i in range(5) for j in range(5)) / 25.0
        return 40 + (b - b.min()) / (b.max() - b.min()) * 170

    back, front = texture(), texture()
    ys, xs = np.mgrid[0:H, 0:W]
    rect = lambda y, x: (y >= H // 4) & (y < 3 * H // 4) & (x >= W // 3) & (x < 2 * W // 3)
    left = np.where(rect(ys, xs), front[ys, xs], back[ys, xs]) + rng.normal(0, 4, (H, W))
    right = 0.9 * np.where(rect(ys, xs + near), front[ys, xs + near], back[ys, xs + far]) + 10 + rng.normal(0, 4, (H, W))
    u8 = lambda a: torch.tensor(np.clip(np.rint(a), 0, 255).astype(np.uint8))
    return u8(left), u8(right)


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
    ap.add_argument("--width", type=int, default=752)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stereo.json"))
    args = ap.parse_args()
    H, W = args.height, args.width
    left_h, right_h = (t.pin_memory() for t in scene(H, W))
    left, right = left_h.cuda(), right_h.cuda()
    # a mild lens model, so that the rectifying call does real bilinear taps
    K = [[0.61 * W, 0, 0.49 * W], [0, 0.61 * W, 0.52 * H], [0, 0, 1]]
    maps = tuple(torch.tensor(stereo.rectify_map(K, [-0.28, 0.07, 2e-4, 2e-5, 0.0], np.eye(3), K, W, H)).cuda() for _ in range(2))
    rows = []
    for D in (64, 128):
        m = stereo.StereoMatcher(W, H, num_disparities=D, bf=0.11 * 0.61 * W)
        plain = timed(lambda: m(left, right), args.reps, args.warmup)
        rectified = timed(lambda: m(left, right, maps=maps), args.reps, args.warmup)
        _, disp, _ = m(left, right)
        depth_h = torch.empty((H, W), dtype=torch.float32).pin_memory()

        def frame():
            _, _, depth = m(left_h.cuda(non_blocking=True), right_h.cuda(non_blocking=True))
            depth_h.copy_(depth, non_blocking=True)
            torch.cuda.current_stream().synchronize()

        for _ in range(args.warmup):
            frame()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            frame()
        host = (time.perf_counter() - t0) * 1e3 / args.reps
        rows.append({"num_disparities": D, "device_ms_per_call": round(plain, 4), "device_ms_per_call_with_maps": round(rectified, 4),
                     "host_ms_per_frame_upload_call_copy_wait": round(host, 4), "density": round(float((disp >= 0).float().mean()), 4),
                     "workspace_MB": round(stereo.stereo_workspace_size(W, H, D) / 1e6, 2)})
    doc = {"resolution": [W, H], "reps": args.reps, "calls": rows, "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
