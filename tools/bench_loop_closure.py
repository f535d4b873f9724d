#!/usr/bin/env python
"""Device time of the two calls of include/loop_closure.h (slam/loop_closure.py): gsr_pose_graph_solve on a chain of N = 100 and N = 1000
keyframes with N - 1 odometry edges and N / 10 loop edges (a closed ring whose loop edges disagree with the drifted odometry by 2 mm per
node; the default options of Training.loop_closure: outer_iters, cg_iters, lambda, step_tolerance; the 1000-node graph a second time with
2000 passes of conjugate gradients, which a chain that long needs; `converged` says whether the last step fell to step_tolerance), and gsr_map_correct --
its prologue and its streaming launch together -- on P = 200 000 and P = 2 000 000 Gaussians seeded by 100 keyframes, every one of them
moved. Each from device events over --reps calls after --warmup, in --rounds rounds (median and spread over the rounds). The solve changes
its poses, so every timed call starts from a fresh copy of them (the copy, 12 N doubles, is inside the window). For gsr_map_correct the
bytes the algorithm needs -- 4 read and 28 read and written per Gaussian: 60 -- over the time give the achieved bytes per second, set
beside the 6.29 TB/s of a float4 copy on this part. Prints one JSON line and writes it to --out (default profiles/loop_closure.json)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)
from slam import loop_closure as lc  # noqa: E402
from slam.stages import loop_closure_options  # noqa: E402

COPY_TBPS = 6.29                                   # float4 copy, measured on an MI355X (the microarchitecture notes the project follows)


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


def graph(N):
    """A ring of N poses; odometry edges that drift by 2 mm and 0.05 degrees per node; exact loop edges every ten nodes."""
    import pose_graph_reference as ref
    gt = ref.ring(N, radius=5.0)
    drifted = ref.bend(gt, np.array([0.0012, -0.001, 0.0012, 0.0005, -0.0005, 0.0005]))
    T, Td = ref.to44(gt), ref.to44(drifted)
    odo = [(k, k + 1) for k in range(N - 1)]
    loops = [(k, (k + N // 2) % N) for k in range(0, N, 10)]
    en = np.asarray(odo + loops, np.int32)
    Z = np.concatenate([ref.to12(Td[[j for _, j in odo]] @ ref.inv44(Td[[i for i, _ in odo]])),
                        ref.to12(T[[j for _, j in loops]] @ ref.inv44(T[[i for i, _ in loops]]))])
    return drifted, en, Z, len(odo), len(loops)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "loop_closure.json"))
    args = ap.parse_args()
    opt = loop_closure_options({"loop_closure": {"enabled": True}})
    out = {"reps": args.reps, "rounds": args.rounds, "options": {k: opt[k] for k in ("outer_iters", "cg_iters", "lambda", "step_tolerance")},
           "solve": [], "map_correct": []}
    dev = "cuda:0"
    for N, cg_iters in ((100, opt["cg_iters"]), (1000, opt["cg_iters"]), (1000, 2000)):
        X0, en, Z, n_odo, n_loop = graph(N)
        w = np.concatenate([np.tile(opt["odometry_weights"], (n_odo, 1)), np.tile(opt["loop_weights"], (n_loop, 1))])
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        start, poses = t(X0, np.float64), t(X0, np.float64)
        fixed = torch.zeros(N, dtype=torch.int32, device=dev)
        fixed[0] = 1
        en_d, Z_d, w_d = t(en, np.int32), t(Z, np.float64), t(w, np.float64)
        D, stats = torch.empty((N, 12), dtype=torch.float32, device=dev), torch.empty(8, dtype=torch.float64, device=dev)
        ws = torch.empty(lc.pose_graph_workspace_size(N, len(en)), dtype=torch.uint8, device=dev)

        def call():
            poses.copy_(start)
            lc.pose_graph_solve(poses, fixed, en_d, Z_d, w_d, len(en), opt["outer_iters"], cg_iters, opt["lambda"], opt["step_tolerance"], D, stats, ws)

        ms = [timed(call, args.reps, args.warmup) for _ in range(args.rounds)]
        values = dict(zip(lc.STATS, stats.tolist()))
        out["solve"].append({"nodes": N, "edges": int(len(en)), "loop_edges": n_loop, "cg_iters": cg_iters, "workspace_bytes": int(ws.numel()),
                             "device_ms": spread(ms), "converged": values["last_step"] <= opt["step_tolerance"], "stats": values})
    nodes = 100
    import pose_graph_reference as ref
    rng = np.random.default_rng(0)
    tau = rng.normal(size=(nodes, 6)) * np.array([0.05, 0.05, 0.05, 0.01, 0.01, 0.01])
    D = torch.from_numpy(ref.to12(ref.Exp(tau)).astype(np.float32)).to(dev)
    table = torch.arange(nodes, dtype=torch.int32, device=dev)
    quat = torch.empty((nodes, 4), dtype=torch.float32, device=dev)
    for P in (200_000, 2_000_000):
        xyz = torch.randn((P, 3), device=dev)
        rot = torch.randn((P, 4), device=dev)
        kf = torch.randint(0, nodes, (P,), dtype=torch.int32, device=dev)
        ms = [timed(lambda: lc.map_correct(xyz, rot, kf, table, D, quat), max(args.reps, 100), args.warmup) for _ in range(args.rounds)]
        needed = 60 * P
        med = float(np.median(ms))
        out["map_correct"].append({"gaussians": P, "nodes": nodes, "bytes_needed": needed, "device_ms": spread(ms),
                                   "achieved_TBps": round(needed / (med * 1e-3) / 1e12, 3), "float4_copy_TBps": COPY_TBPS,
                                   "share_of_copy_rate": round(needed / (med * 1e-3) / 1e12 / COPY_TBPS, 3)})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
