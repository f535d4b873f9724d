#!/usr/bin/env python
"""Device time of one plane-sweep call (slam/sweep.py PlaneSweep on grey bytes: census, cost, eight path launches, selection) at 640 x 480
with 3 partners, per stage from the library's event timers (gsr_profile_enable: events around each stage on the launch stream) and for the
whole call from device events over --reps calls after --warmup; next to it the stereo matcher's call at the same frame size and 64
disparities, whose eight-path aggregation is the same recurrence. The scene is seeded: blurred noise in two depth layers, the partners
displaced sideways, downwards and to the other side. Prints one JSON line and writes it to --out (default profiles/sweep.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from diff_gaussian_rasterization import _C  # noqa: E402
from slam import stereo, sweep  # noqa: E402

STAGES = ("sweep_census", "sweep_cost", "sweep_paths", "sweep_select")
SHIFTS = ((0, 1), (1, 0), (0, -1), (-1, 0))          # (rows, columns) per pixel of shift: right, down, left, up


def scene(H, W, partners, seed=0, near=20, far=5, margin=24):
    """(reference u8 [H, W], partners u8 [J, H, W], transforms f32 [J, 12], K, w_step): a central rectangle whose image moves by `near`
    pixels between the reference and a partner, on a background that moves by `far`; a shift of s pixels is hypothesis 2 s."""
    rng = np.random.default_rng(seed)

    def texture():
        t = np.pad(rng.uniform(0, 1, (H + 2 * margin, W + 2 * margin)), 2, mode="edge")
        b = sum(t[i:i + H + 2 * margin, j:j + W + 2 * margin] for i in range(5) for j in range(5)) / 25.0
        return 40 + (b - b.min()) / (b.max() - b.min()) * 170

    back, front = texture(), texture()
    ys, xs = np.mgrid[0:H, 0:W]
    rect = lambda y, x: (y >= H // 4) & (y < 3 * H // 4) & (x >= W // 3) & (x < 2 * W // 3)
    tex = lambda t, y, x: t[y + margin, x + margin]
    u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    ref = u8(np.where(rect(ys, xs), tex(front, ys, xs), tex(back, ys, xs)) + rng.normal(0, 4, (H, W)))
    f, baseline = 0.8 * W, 0.16
    w_step = 0.5 / (f * baseline)                     # half a pixel of shift per hypothesis
    images, transforms = [], []
    for dy, dx in SHIFTS[:partners]:
        img = np.where(rect(ys + dy * near, xs + dx * near), tex(front, ys + dy * near, xs + dx * near), tex(back, ys + dy * far, xs + dx * far))
        images.append(u8(0.9 * img + 10 + rng.normal(0, 4, (H, W))))
        transforms.append([1, 0, 0, -baseline * dx, 0, 1, 0, -baseline * dy, 0, 0, 1, 0])
    return ref, np.stack(images), np.asarray(transforms, np.float32), (f, f, 0.5 * W - 0.5, 0.5 * H - 0.5), w_step


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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--partners", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sweep.json"))
    args = ap.parse_args()
    H, W, J = args.height, args.width, args.partners
    ref_h, partners_h, transforms_h, K, w_step = scene(H, W, J)
    ref, partners, transforms = (torch.tensor(a).cuda() for a in (ref_h, partners_h, transforms_h))
    s = sweep.PlaneSweep()
    call = lambda: s.sweep_grey(ref, partners, K, transforms, 0.0, w_step)
    whole = timed(call, args.reps, args.warmup)
    _C.profile_reset()
    _C.profile_enable(STAGES)
    for _ in range(args.reps):
        call()
    torch.cuda.synchronize()
    _C.profile_enable(False)
    stats = _C.profile_read()
    _C.profile_reset()
    stages = {k: round(stats[k][0] / args.reps, 4) for k in STAGES}
    out = call()
    m = stereo.StereoMatcher(W, H, num_disparities=64, bf=0.11 * 0.61 * W)
    stereo_ms = timed(lambda: m(ref, partners[0]), args.reps, args.warmup)
    doc = {"resolution": [W, H], "partners": J, "reps": args.reps, "device_ms_per_call": round(whole, 4), "device_ms_per_stage": stages,
           "valid_share": round(float(out["valid"].float().mean()), 4), "workspace_MB": round(sweep.sweep_workspace_size(W, H, J) / 1e6, 2),
           "stereo_64_device_ms_per_call_same_size": round(stereo_ms, 4), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
