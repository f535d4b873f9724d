#!/usr/bin/env python
"""One RAFT pair (both directions, 20 iterations) at 640x480 with the recipe weights (slam/optical_flow.py): total ms, ms per stage
(encoders, correlation pyramid, lookup per iteration, update-block convolutions per iteration, upsampling) and the pyramid kernel's
achieved TFLOP/s and GB/s. Stages are timed with events around each, after warm-up; the total is a pair with no events inside.
Prints one JSON line. --save-weights PATH also writes the recipe weights as a checkpoint (for tools/run_slam.py --raft-weights).
--gma adds a `gma` block from the same process (GmaFlow with its recipe weights on the same pair): ms per pair, first and rest, by
device events around each pair; the device time of the attention and of the 20 aggregate launches; and the aggregate kernel's achieved
TFLOP/s and GB/s with their fractions of 157 TFLOP/s (fp32 MFMA) and 8 TB/s. With it, --save-weights writes the GMA recipe instead
(for --gma-weights)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import optical_flow as of  # noqa: E402
from slam import pretrained  # noqa: E402

PEAK_FP32_MFMA_TFLOPS, PEAK_HBM_GBPS = 157.0, 8000.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--save-weights", default=None)
    ap.add_argument("--gma", action="store_true", help="also time GmaFlow and its attention and aggregate kernels")
    args = ap.parse_args()
    sd = of.recipe_state_dict(0)
    if args.save_weights:
        torch.save({"module." + k: v for k, v in (of.gma_recipe_state_dict(0) if args.gma else sd).items()}, args.save_weights)
    dev = "cuda:0"
    est = of.RaftFlow(sd, dev)
    g = torch.Generator().manual_seed(0)
    H, W = args.height, args.width
    a = torch.rand(3, H, W, generator=g).to(dev)
    b = torch.roll(a, shifts=(3, -5), dims=(1, 2)).contiguous()
    for _ in range(2):
        est.pair(a, b)
    torch.cuda.synchronize()
    total, _ = timed(lambda: est.pair(a, b), args.reps)

    enc, (fi, ni, ii, _) = timed(lambda: est.encode(a), args.reps)
    fj = est.encode(b)[0]
    pyr_ms, levels = timed(lambda: of.corr_pyramid(fi, fj, both=True), args.reps * 5)
    _, h, w = fi.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    coords = torch.stack([xs, ys]).float()[None].expand(2, 2, h, w).contiguous() + 0.3
    corr = torch.empty((2, of.CORR_CHANNELS, h, w), device=dev)
    look_ms, _ = timed(lambda: of.corr_lookup(levels, coords, corr), args.reps * 20)
    net = torch.stack([ni, ni])
    inp = torch.stack([ii, ii])
    flow = coords - 0.3
    upd_ms, _ = timed(lambda: est._update(net, inp, corr, flow, with_mask=False), args.reps * 5)
    updm_ms, (_, mask, _) = timed(lambda: est._update(net, inp, corr, flow, with_mask=True), args.reps)
    pad = of.pad_amounts(H, W)
    up_ms, _ = timed(lambda: of.upsample(flow.contiguous(), mask.contiguous(), pad, (H, W)), args.reps * 20)
    N = h * w
    flops = 2.0 * N * N * fi.shape[0]
    bytes_l0 = 2 * N * N * 4 + 2 * fi.numel() * 4
    bytes_all = sum(t.numel() * 4 for t in levels) + sum(t.numel() * 4 for t in levels[:-1])    # written + read by the pooling
    iters = of.ITERS
    res = {"metric": "raft_pair", "size": [W, H], "iters": iters, "total_ms": round(total, 3),
                      "encoders_ms (4 passes: fnet+cnet x 2 images)": round(2 * enc, 3),
                      "corr_pyramid_ms": round(pyr_ms, 4), "lookup_ms_per_iter": round(look_ms, 4),
                      "update_convs_ms_per_iter": round(upd_ms, 3), "mask_head_ms_last_iter": round(updm_ms - upd_ms, 3),
                      "upsample_ms": round(up_ms, 4),
                      "update_share_of_total": round((iters * upd_ms + updm_ms - upd_ms) / total, 3),
                      "pyramid_tflops": round(flops / (pyr_ms * 1e-3) / 1e12, 2),
                      "pyramid_gbps_level0_plus_pool": round((bytes_l0 + bytes_all) / (pyr_ms * 1e-3) / 1e9, 1)}
    if args.gma:
        res["gma"] = gma_block(args, dev, a, b, inp, total)
    print(json.dumps(res))


def gma_block(args, dev, a, b, inp, raft_ms):
    """GmaFlow on the pair (a, b): whole pairs by device events (the first includes MIOpen's and the allocator's warm-up), then the two
    kernels alone on the pair's own context features."""
    est = of.GmaFlow(of.gma_recipe_state_dict(0), dev)
    log = pretrained.EventLog(dev)
    for _ in range(args.reps + 1):
        with log.timed():
            est.pair(a, b)
    t = log.summary()
    B, D, h, w = inp.shape
    N = h * w
    qk = torch.nn.functional.conv2d(inp, est.p["att.to_qk.weight"])
    q, k = qk[:, :D].contiguous(), qk[:, D:].contiguous()
    attn = torch.empty((B, N, N), device=dev)
    att_ms, _ = timed(lambda: of.gma_attention(q, k, est.scale, attn), args.reps * 5)
    g = torch.Generator().manual_seed(1)
    v, x = (torch.randn(B, D, h, w, generator=g).to(dev) for _ in range(2))
    out = torch.empty_like(x)
    agg_ms, _ = timed(lambda: of.gma_aggregate(attn, v, x, est.gamma, out), args.reps * 20)
    tflops = 2.0 * B * N * N * D / (agg_ms * 1e-3) / 1e12
    gbps = (B * N * N * 4 + 3 * B * D * N * 4) / (agg_ms * 1e-3) / 1e9          # attn, v, x read once and out written
    rest = t["ms_per_item_rest"]
    return {"pair_ms_first": round(t["ms_first"], 3), "pair_ms_rest": round(rest, 3), "raft_pair_ms": round(raft_ms, 3),
            "low_res_pixels": N, "attention_bytes": B * N * N * 4, "attention_ms": round(att_ms, 4),
            "aggregate_ms_per_launch": round(agg_ms, 4), "aggregate_ms_20_launches": round(of.ITERS * agg_ms, 3),
            "attention_share_of_pair": round(att_ms / rest, 4), "aggregate_share_of_pair": round(of.ITERS * agg_ms / rest, 4),
            "aggregate_tflops": round(tflops, 2), "aggregate_fraction_of_157_tflops": round(tflops / PEAK_FP32_MFMA_TFLOPS, 4),
            "aggregate_gbps": round(gbps, 1), "aggregate_fraction_of_8_tbps": round(gbps / PEAK_HBM_GBPS, 4)}


if __name__ == "__main__":
    main()
