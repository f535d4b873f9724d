#!/usr/bin/env python
"""Device time of the YOLO segmenter per 640x480 frame (slam/segmentation.py): the network (yolov9e-seg's topology at full width with
seeded weights, slam/yolo_stand_in.py; fp32 convolutions on MIOpen) and the HIP post-processing (decode, sort, NMS, masks), each from
device events over --reps calls after --warmup. The post-processing runs on head tensors with planted detections (--dets per class) so
that NMS and the mask stage have work. Prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import segmentation as seg  # noqa: E402
from slam import yolo_stand_in  # noqa: E402


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


def planted_heads(H, W, n_per_class, classes, nc=80, nm=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    heads = []
    for s in (8, 16, 32):
        h = torch.randn((64 + nc, H // s, W // s), generator=g)
        h[64:] = -6.0
        heads.append([h, torch.randn((nm, H // s, W // s), generator=g)])
    lh, lw = H // 8, W // 8
    idx = torch.randperm(lh * lw, generator=g)
    k = 0
    for c in classes:
        for _ in range(n_per_class):
            y, x = divmod(int(idx[k]), lw)
            heads[0][0][64 + c, y, x] = float(torch.rand((), generator=g)) * 4
            k += 1
    proto = torch.randn((nm, H // 4, W // 4), generator=g)
    return [(h.cuda().contiguous(), c.cuda().contiguous()) for h, c in heads], proto.cuda().contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=1, help="channel divisor of the stand-in network (1: yolov9e-seg)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dets", type=int, default=20, help="planted detections per class for the post-processing")
    args = ap.parse_args()
    H, W = 480, 640
    with tempfile.TemporaryDirectory() as d:
        path = yolo_stand_in.write_checkpoint(os.path.join(d, "stand_in.pt"), width=args.width)
        y = seg.YoloSeg.from_checkpoint(path, "cuda:0")
    img = torch.rand((3, H, W), generator=torch.Generator().manual_seed(0)).cuda()
    net_ms = timed(lambda: y.forward(img), args.reps, args.warmup)
    heads, proto = planted_heads(H, W, args.dets, [0, 56])
    motion = torch.ones((H, W), dtype=torch.bool, device="cuda:0")
    post_ms = timed(lambda: y.postprocess(heads, proto, [0, 56], motion), args.reps * 5, args.warmup)
    res = y.postprocess(heads, proto, [0, 56], motion)
    counts = res.counts.tolist()
    print(json.dumps({"resolution": [W, H], "width_divisor": args.width, "network_ms": round(net_ms, 3), "postprocess_ms": round(post_ms, 4),
                      "detections": counts[0], "candidates": counts[1], "params_M": round(sum(op.w.numel() for op in _convs(y)) / 1e6, 2),
                      "device": torch.cuda.get_device_name(0)}))


def _convs(y):
    """Every folded convolution of the compiled network (closures walked for _ConvOp cells)."""
    seen, out = set(), []

    def walk(fn):
        if id(fn) in seen:
            return
        seen.add(id(fn))
        if isinstance(fn, seg._ConvOp):
            out.append(fn)
            return
        for attr in vars(fn).values() if isinstance(fn, seg._SegmentHead) else ():
            for f in (attr if isinstance(attr, list) else [attr]):
                if callable(f):
                    walk(f)
        for cell in getattr(fn, "__closure__", None) or ():
            v = cell.cell_contents
            for f in (v if isinstance(v, list) else [v]):
                if callable(f):
                    walk(f)

    for _, _, fn in y.layers:
        walk(fn)
    return out


if __name__ == "__main__":
    main()
