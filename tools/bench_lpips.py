#!/usr/bin/env python
"""Device time of the LPIPS metric per 640x480 image pair (slam/perceptual.py) for B = 1, 4, 16 pairs per call: the network (AlexNet's
features with seeded weights; fp32 convolutions, ReLU and max-pool on MIOpen / ATen, both images of every pair in one batch) and the HIP
kernels (gsr_lpips_prepare; gsr_lpips_distance on the taps), each from device events over --reps calls after --warmup. Prints one JSON
line."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import perceptual  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    args = ap.parse_args()
    H, W = 480, 640
    m = perceptual.Lpips(*perceptual.recipe_state_dicts(0), "cuda:0")
    g = torch.Generator().manual_seed(0)
    rows = []
    for B in args.batches:
        x, y = torch.rand((B, 3, H, W), generator=g).cuda(), torch.rand((B, 3, H, W), generator=g).cuda()
        batch = perceptual.prepare(x, y)
        with torch.no_grad():
            feats = [f.contiguous() for f in m.features(batch)]
            net = timed(lambda: m.features(batch), args.reps, args.warmup)
        prep = timed(lambda: perceptual.prepare(x, y), args.reps * 5, args.warmup)
        dist = timed(lambda: perceptual.distance(feats, m.lins, m.norm, m._ws), args.reps * 5, args.warmup)
        total = timed(lambda: m(x, y), args.reps, args.warmup)
        rows.append({"pairs": B, "network_ms_per_pair": round(net / B, 4), "prepare_ms_per_pair": round(prep / B, 4),
                     "distance_ms_per_pair": round(dist / B, 4), "forward_ms_per_pair": round(total / B, 4)})
    print(json.dumps({"resolution": [W, H], "norm": m.norm, "batches": rows, "feature_MB_per_pair": round(sum(
        2 * c * h * w * 4 for c, (h, w) in zip(perceptual.CHANNELS, perceptual.tap_sizes(H, W))) / 1e6, 2),
        "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
