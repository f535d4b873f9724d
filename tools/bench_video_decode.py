#!/usr/bin/env python
"""Device time of the JPEG decoder (slam/mjpeg.py jpeg_decode, include/video_io.h gsr_jpeg_decode) per 640 x 480 frame at chunk sizes 1, 4
and 16, from device events over --reps calls after --warmup; the split between the entropy part (restart markers + entropy decoding) and
the rest (inverse DCT, upsampling, colour) from the library's event timers; and PIL's decode time for the same frames in the same process.
The frames are --video PATH (a Motion-JPEG AVI file or a folder of .jpg files), or 16 rendered-looking pictures with noise compressed at
--quality: once by the device encoder (no restart markers: one lane decodes a whole frame) and once by PIL with a restart marker per MCU
row (one lane per row). Prints one JSON line and writes it to --out (default profiles/video_decode.json)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from diff_gaussian_rasterization import _C  # noqa: E402
from slam import jpeg_decode, mjpeg  # noqa: E402


def pictures(n, H, W):
    """uint8 [n, H, W, 3]: low frequencies, edges and sensor-like noise."""
    out = []
    for k in range(n):
        rng = np.random.default_rng(k)
        y, x = np.mgrid[0:H, 0:W]
        base = 128 + 80 * np.sin(x / 37.0 + k)[..., None] * np.cos(y / 29.0)[..., None] * np.array([1.0, -0.6, 0.4])
        base += 50 * (((x // 40 + y // 40 + k) & 1)[..., None] - 0.5)
        out.append(np.clip(np.rint(base + rng.normal(0, 4, (H, W, 3))), 0, 255).astype(np.uint8))
    return np.stack(out)


def device_files(pics, quality):
    dev = torch.device("cuda:0")
    n, H, W, _ = pics.shape
    q = mjpeg.quant_tables(quality)
    scan = torch.zeros((n, W * H * 3), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(n, dtype=torch.int32, device=dev)
    mjpeg.jpeg_encode(torch.from_numpy(pics).to(dev), torch.from_numpy(q.astype(np.int16)).to(dev), scan, sizes)
    sizes = sizes.cpu().numpy()
    return [mjpeg.jfif_header(W, H, q) + scan[k, :sizes[k]].cpu().numpy().tobytes() + mjpeg.EOI for k in range(n)]


def pil_files(pics, quality, **options):
    out = []
    for p in pics:
        b = io.BytesIO()
        Image.fromarray(p).save(b, "JPEG", quality=quality, **options)
        out.append(b.getvalue())
    return out


def measure(files, reps, warmup):
    """{chunk: ms per frame ...} of the device decoder, and PIL's ms per frame, for a list of files of one size."""
    dev = torch.device("cuda:0")
    parsed = [jpeg_decode.parse_frame(d, f"frame {k}") for k, d in enumerate(files)]
    W, H = parsed[0].width, parsed[0].height
    row = {"frames": len(files), "width": W, "height": H, "sampling": jpeg_decode.SAMPLING_NAMES[parsed[0].sampling],
           "restart_intervals_per_frame": parsed[0].intervals, "bytes_per_frame": float(np.mean([len(d) for d in files])), "chunks": {}}
    for chunk in (1, 4, 16):
        group = [parsed[k % len(parsed)] for k in range(chunk)]
        p = jpeg_decode.pack(group)
        t = {k: torch.from_numpy(p[k].view(np.int16) if k == "qtables" else p[k]).to(dev) for k in ("scans", "offsets", "qtables", "huffman", "descriptors")}
        rgb = torch.empty((chunk, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(chunk, dtype=torch.int32, device=dev)
        ws = torch.empty(mjpeg.jpeg_decode_workspace_size(chunk, W, H, p["sampling"], p["max_intervals"]), dtype=torch.uint8, device=dev)
        call = lambda: mjpeg.jpeg_decode(t["scans"], t["offsets"], t["qtables"], t["huffman"], t["descriptors"], rgb, status, p["sampling"],  # noqa: E731
                                         p["max_intervals"], None, ws)
        for _ in range(warmup):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            call()
        b.record()
        b.synchronize()
        if int(status.abs().sum()):
            raise SystemExit(f"a frame did not decode: status {status.tolist()}")
        _C.profile_reset()
        _C.profile_enable(["jpeg_decode_entropy", "jpeg_decode_pixels"])
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        prof = _C.profile_read()
        _C.profile_enable(False)
        split = {k: prof[k][0] / max(prof[k][1], 1) / chunk for k in ("jpeg_decode_entropy", "jpeg_decode_pixels")}
        row["chunks"][str(chunk)] = {"ms_per_frame": a.elapsed_time(b) / reps / chunk, "entropy_ms_per_frame": split["jpeg_decode_entropy"],
                                     "rest_ms_per_frame": split["jpeg_decode_pixels"]}
    for d in files[:2]:
        np.array(Image.open(io.BytesIO(d)).convert("RGB"))
    t0 = time.perf_counter()
    n = 0
    for _ in range(max(1, reps // 4)):
        for d in files:
            np.array(Image.open(io.BytesIO(d)).convert("RGB"))
            n += 1
    row["pil_ms_per_frame"] = (time.perf_counter() - t0) * 1e3 / n
    for v in row["chunks"].values():
        v["faster_than_pil"] = v["ms_per_frame"] < row["pil_ms_per_frame"]
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--video", default=None, help="a Motion-JPEG AVI file or a folder of .jpg files (default: generated 640 x 480 frames)")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "video_decode.json"))
    args = ap.parse_args()
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "quality": args.quality, "sets": {}}
    if args.video:
        src = jpeg_decode.open_source(args.video)
        result["sets"][os.path.basename(args.video.rstrip("/"))] = measure([src.read(k) for k in range(min(len(src), 16))], args.reps, args.warmup)
    else:
        pics = pictures(16, 480, 640)
        result["sets"]["device_encoder_no_restart"] = measure(device_files(pics, args.quality), args.reps, args.warmup)
        result["sets"]["pil_restart_per_mcu_row"] = measure(pil_files(pics, args.quality, restart_marker_rows=1), args.reps, args.warmup)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
