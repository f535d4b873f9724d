#!/usr/bin/env python
"""Generates tests/golden/golden_gma.npz by running the reference's OWN GMA module (GMA/network.py RAFTGMA, imported through
make_golden_raft.py's path and cv2 stub, authoring container only) on the CPU with the seeded stand-in weights of slam/optical_flow.py
gma_recipe_state_dict. Data only: the state_dict's (key, shape) list, the to_qk gain, and for the two image pairs of make_golden_raft.py
(the same canvases, row-difference coded, and shifts) per direction: 8 attention rows with the mean row entropy / log N, 256 values of
iteration 0's motion_features_global, flow1, flow20, the subsampled flow_up, and flow20_uniform -- the same run with the attention
replaced by 1 / N, which must differ from flow20 by at least 100 times the bar the test puts on flow20, so that a network test cannot
pass with a wrong attention. Each stored quantity comes with the reference's own max-abs deviation between runs with 1 and 8 threads
(*_threads_dev). No weights are stored."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_raft import FLOW_UP_STEP, as_input, pair_images, textured_canvas   # noqa: E402  (also sets the paths and stubs cv2)
from GMA.network import RAFTGMA                                                      # noqa: E402
from GMA.utils.utils import InputPadder                                              # noqa: E402
from slam.optical_flow import GMA_QK_GAIN, gma_recipe_state_dict                     # noqa: E402

SEED = 0
ATT_ROWS = 8
GLOBAL_VALUES = 256
FLOW20_REL_TOL = 1e-4          # the bar tests/test_hip_gma.py puts on flow20, relative to max |flow20|


def run(model, p1, p2, threads, uniform=False):
    """One direction: attention, iteration 0's motion_features_global, flow1, flow20 and the upsampled flow, with `threads` threads."""
    torch.set_num_threads(threads)
    rec = {}
    def on_attention(module, inputs, o):                # o: [1, 1, N, N]; a returned tensor replaces the module's output
        rec["attention"] = o[0, 0].clone()
        return torch.full_like(o, 1.0 / o.shape[-1]) if uniform else None

    def on_aggregate(module, inputs, o):
        rec.setdefault("motion_global", o[0].clone())

    hooks = [model.att.register_forward_hook(on_attention), model.update_block.aggregator.register_forward_hook(on_aggregate)]
    try:
        with torch.no_grad():
            low20, up20 = model(p1, p2, iters=20, test_mode=True)
            rec["flow20"], rec["up"] = low20[0].clone(), up20[0].clone()
            if not uniform:
                rec["flow1"] = model(p1, p2, iters=1, test_mode=True)[0][0].clone()
    finally:
        for h in hooks:
            h.remove()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "golden_gma.npz"))
    args = ap.parse_args()
    model = RAFTGMA(types.SimpleNamespace())
    sd = model.state_dict()
    out = {"keys": np.array(list(sd.keys())), "shapes": np.array([",".join(str(s) for s in v.shape) for v in sd.values()]),
           "seed": np.array(SEED), "qk_gain": np.array(GMA_QK_GAIN)}
    model.load_state_dict(gma_recipe_state_dict(SEED))
    model.eval()
    rng = np.random.default_rng(5)                      # make_golden_raft.py's generator and order: the same two canvases
    for name, (H, W), shift in (("a", (130, 170), (3, -2)), ("b", (240, 320), (-5, 4))):
        canvas = textured_canvas(rng, H, W)
        u1, u2 = pair_images(canvas, shift)
        out[f"{name}/canvas_rowdiff"] = np.diff(canvas, axis=1, prepend=np.zeros_like(canvas[:, :1]))
        out[f"{name}/shift"] = np.array(shift)
        for d, (x1, x2) in (("12", (u1, u2)), ("21", (u2, u1))):
            i1, i2 = as_input(x1), as_input(x2)
            padder = InputPadder(i1.shape)
            p1, p2 = padder.pad(i1, i2)
            r8, r1 = run(model, p1, p2, 8), run(model, p1, p2, 1)
            uni = run(model, p1, p2, 8, uniform=True)
            s = f"{name}/{d}"
            att = r8["attention"]
            N = int(att.shape[0])
            a64 = att.double()
            ratio = float((-(a64 * torch.log(a64.clamp_min(1e-300))).sum(1)).mean() / np.log(N))
            assert 0.3 <= ratio <= 0.8, (s, ratio, "choose another GMA_QK_GAIN in 100..150")
            out[f"{s}/entropy_ratio"] = np.array(ratio)
            rows = np.random.default_rng(int(H * 13 + W + (d == "21"))).choice(N, size=ATT_ROWS, replace=False)
            gidx = np.random.default_rng(int(H * 17 + W + (d == "21"))).choice(r8["motion_global"].numel(), size=GLOBAL_VALUES, replace=False)
            step = FLOW_UP_STEP[name]
            pick = {"attention": lambda r: r["attention"][rows].numpy(),
                    "motion_global": lambda r: r["motion_global"].reshape(-1)[gidx].numpy(),
                    "flow1": lambda r: r["flow1"].numpy(), "flow20": lambda r: r["flow20"].numpy(),
                    "flow_up": lambda r: padder.unpad(r["up"]).permute(1, 2, 0).numpy()[::step, ::step]}
            out[f"{s}/attention_rows"], out[f"{s}/motion_global_idx"], out[f"{s}/flow_up_step"] = rows, gidx, np.array(step)
            for tag, f in pick.items():
                out[f"{s}/{tag}"] = f(r8)
                out[f"{s}/{tag}_threads_dev"] = np.array(float(np.abs(f(r8).astype(np.float64) - f(r1)).max()))
            out[f"{s}/flow20_uniform"] = uni["flow20"].numpy()
            gap = float(np.abs(out[f"{s}/flow20"] - out[f"{s}/flow20_uniform"]).max())
            tol = FLOW20_REL_TOL * float(np.abs(out[f"{s}/flow20"]).max())
            assert gap >= 100 * tol, (s, gap, tol, "raise GMA_QK_GAIN within the entropy window")
            print(s, "N", N, "entropy ratio", round(ratio, 3), "row max", float(att.max()), "|flow20|", float(np.abs(out[f'{s}/flow20']).max()),
                  "uniform gap / tol", gap / tol, "threads dev", {t: float(out[f"{s}/{t}_threads_dev"]) for t in pick})
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes;", len(out["keys"]), "state_dict entries")


if __name__ == "__main__":
    main()
