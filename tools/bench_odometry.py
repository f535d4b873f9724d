#!/usr/bin/env python
"""Device time of one dense odometry call (slam/odometry.py DenseOdometry.align: the current frame's pyramid, then 22 passes of sums and
solve over three levels, then the gate) at 640 x 480 and 320 x 240, per stage from the library's event timers (gsr_profile_enable: events
around each stage on the launch stream) and for the whole call from device events over --reps calls after --warmup. The scene is analytic:
a textured plane seen from two poses 1.4 degrees and 39 mm apart, the previous depth exact. The same frames are timed through
gsr_odometry_align_rgbd (affine brightness and the depth term on, device_ms_per_call_with_terms) in the same process. Prints one JSON line and writes it to --out
(default profiles/odometry.json)."""
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
from slam import odometry  # noqa: E402

STAGES = ("odometry_pyramid", "odometry_sums", "odometry_solve")
PLANE, PLANE_D = np.array([0.15, 0.1, 1.0]), 2.0
MOTION = (0.03, -0.02, 0.015, np.deg2rad(0.8), np.deg2rad(-1.0), np.deg2rad(0.6))      # [rho | theta]


def texture(x, y):
    return (0.5 + 0.12 * np.sin(3.1 * x + 0.4) + 0.1 * np.sin(4.3 * y + 1) + 0.08 * np.sin(7.7 * x + 5.1 * y) + 0.06 * np.sin(13 * x - 9 * y + 2)
            + 0.05 * np.sin(21 * x + 17 * y))


def motion_matrix(xi):
    """exp of a small twist through the matrix series (40 terms: exact to double precision at this size)."""
    rho, (wx, wy, wz) = xi[:3], xi[3:]
    A = np.zeros((4, 4))
    A[:3, :3] = [[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]]
    A[:3, 3] = rho
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 40):
        term = term @ A / k
        E = E + term
    return E


def scene(W, H):
    """(previous image [3, H, W], previous depth [H, W], current image [3, H, W], K, T): both images and the depth by ray-plane intersection."""
    fx = fy = 0.9 * W
    cx, cy = (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2
    T = motion_matrix(np.asarray(MOTION))
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    z = PLANE_D / (ray @ PLANE)
    prev = texture(ray[..., 0] * z, ray[..., 1] * z)
    R, t = T[:3, :3], T[:3, 3]
    origin, direction = -R.T @ t, ray @ R
    point = origin + direction * ((PLANE_D - PLANE @ origin) / (direction @ PLANE))[..., None]
    cur = texture(point[..., 0], point[..., 1])
    rgb = lambda g: torch.tensor(np.broadcast_to(g.astype(np.float32)[None], (3, H, W)).copy()).cuda()
    return rgb(prev), torch.tensor(z.astype(np.float32)).cuda(), rgb(cur), (fx, fy, cx, cy), T


def current_depth(W, H, K, T):
    """The current frame's depth [H, W] of the same plane: the step along each of its rays (they have z = 1)."""
    fx, fy, cx, cy = K
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    origin, direction = -T[:3, :3].T @ T[:3, 3], ray @ T[:3, :3]
    return torch.tensor(((PLANE_D - PLANE @ origin) / (direction @ PLANE)).astype(np.float32)).cuda()


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


def measure(W, H, reps, warmup):
    prev, depth, cur, K, T_true = scene(W, H)
    odo = odometry.DenseOdometry(W, H, K)
    odo.keep(prev, depth, None)
    call = lambda: odo.align(cur)
    whole = timed(call, reps, warmup)
    keep_ms = timed(lambda: odo.keep(prev, depth, None), reps, warmup)
    _C.profile_reset()
    _C.profile_enable(STAGES)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    _C.profile_enable(False)
    prof = _C.profile_read()
    _C.profile_reset()
    # the same frames through gsr_odometry_align_rgbd: affine brightness and the depth term, the current pyramid built with its depth
    terms = odometry.DenseOdometry(W, H, K, affine=True, geometric_weight=1.0)
    terms.keep(prev, depth, None)
    depth_cur = current_depth(W, H, K, T_true)
    terms_ms = timed(lambda: terms.align(cur, depth=depth_cur), reps, warmup)
    T, stats = call()
    T, stats = T.double().cpu().numpy(), stats.cpu().numpy()
    dR = T[:3, :3] @ T_true[:3, :3].T
    return {"device_ms_per_call_with_terms": round(terms_ms, 4), "resolution": [W, H], "levels": odo.levels, "iters": odo.iters, "launches_per_call": 2 * sum(odo.iters) + 2 + odo.levels + 1,
            "device_ms_per_call": round(whole, 4), "device_ms_per_keep": round(keep_ms, 4),
            "device_ms_per_stage": {k: round(prof[k][0] / reps, 4) for k in STAGES},
            "accepted": bool(stats[0]), "inlier_share": round(float(stats[1]), 4),
            "rotation_error_deg": round(float(np.rad2deg(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))), 5),
            "translation_error_mm": round(1e3 * float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), 4),
            "workspace_bytes": odometry.align_workspace_size(W, H, odo.levels), "pyramid_bytes": odometry.pyramid_size(W, H, odo.levels)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "odometry.json"))
    args = ap.parse_args()
    doc = {"reps": args.reps, "sizes": [measure(W, H, args.reps, args.warmup) for W, H in ((640, 480), (320, 240))],
           "device": torch.cuda.get_device_name(0)}
    print(json.dumps(doc))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
