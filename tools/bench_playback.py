#!/usr/bin/env python
"""Measures the playback (slam/playback.py) at 640x480 on the dynamic synthetic map and writes profiles/playback.json:
  * gsr_frame_export per view by device events at V = 1 and V = 12, the bytes it moves and the resulting GB/s;
  * playback frames/s without files (render + export + copy to pinned memory) and with files, and the time the loop waited for the writer;
  * the yardstick: the same frames produced without this module -- per-frame render(), (clamp * 255).to(uint8).permute(1, 2, 0).cpu(),
    PIL's Image.save, matplotlib's jet for the depth picture.
--frames N: frames played (default 120, resampled along the tracked path); --out PATH.
--video [--repeats R] [--quality Q]: the video mode instead. On the same map and path it alternates Playback.write (PNG files of rgb and
depth_vis) and Playback.write_video (Motion-JPEG AVI, compressed on the device), each with files and with files=False, R times each, and
times gsr_jpeg_encode by device events at V = 1 and 12; writes profiles/playback_video.json. --encode-only: only that last timing (the
form to run under a kernel profiler).
--device-png [--repeats R]: the lossless mode. On the same map and path it alternates Playback.write with the host's zlib and with
device_png=True (gsr_png_encode), each without and with the 16-bit depth, R times each, and times gsr_png_encode by device events at V = 1
and 12 for both picture kinds, with the bytes per picture beside zlib level 1's; writes profiles/playback_device_png.json."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)
from slam import frame_io  # noqa: E402
from slam.dataset import SyntheticRGBDDataset  # noqa: E402
from slam.map_io import load_map  # noqa: E402
from slam.playback import DEPTH_SCALE, DEPTH_VMAX, Playback, resampled  # noqa: E402
from slam.system import SLAM, default_config, merge_config  # noqa: E402


def build_map(directory, frames=36):
    """tools/run_slam_demo.py's dynamic_640x480_graph scenario, saved."""
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=frames, width=640, height=480, seed=0, dynamic=True, dystart=6, spacing=0.025)
    cfg = merge_config(default_config(), {"Training": {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": 60,
                                                       "static_map_iters": 30, "dynamic_map_iters": 80, "network_init_iters": 50, "gaussian_update_every": 60,
                                                       "gaussian_update_offset": 20, "tracking_graph": True},
                                          "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 150},
                                          "model_params": {"dynamic_model": True}, "Results": {"eval_rendering": False}})
    slam = SLAM(cfg, ds)
    slam.run()
    return slam.save_map(directory)


def time_export(colour, depth, repeats=50):
    """ms per call of gsr_frame_export with all three outputs, by device events around `repeats` back-to-back launches (after a warm-up)."""
    V, _, H, W = colour.shape
    dev = colour.device
    lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    vis, u16 = torch.empty_like(rgb), torch.empty((V, H, W), dtype=torch.int16, device=dev)
    for _ in range(5):
        frame_io.frame_export(colour, depth, lut, DEPTH_VMAX, DEPTH_SCALE, rgb, vis, u16)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        frame_io.frame_export(colour, depth, lut, DEPTH_VMAX, DEPTH_SCALE, rgb, vis, u16)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / repeats
    moved = V * H * W * (16 + 3 + 3 + 2)                         # four float planes read; two RGB pictures and one 16-bit plane written
    return {"views": V, "ms_per_call": ms, "us_per_view": ms * 1e3 / V, "bytes_moved": moved, "GB_per_s": moved / (ms * 1e-3) / 1e9}


def time_encode(pb, colour, depth, quality, repeats=20):
    """ms per call of gsr_jpeg_encode on the exported bytes of the given views, by device events around `repeats` back-to-back calls."""
    from slam import mjpeg
    V, _, H, W = colour.shape
    dev = colour.device
    lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    frame_io.frame_export(colour, depth, lut, DEPTH_VMAX, DEPTH_SCALE, rgb)
    q = torch.from_numpy(mjpeg.quant_tables(quality).astype(np.int16)).to(dev)
    scan = torch.empty((V, W * H * 3), dtype=torch.uint8, device=dev)
    sizes = torch.empty((V,), dtype=torch.int32, device=dev)
    ws = torch.empty(mjpeg.jpeg_workspace_size(V, W, H), dtype=torch.uint8, device=dev)
    for _ in range(3):
        mjpeg.jpeg_encode(rgb, q, scan, sizes, None, ws)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        mjpeg.jpeg_encode(rgb, q, scan, sizes, None, ws)
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / repeats
    out = [int(v) for v in sizes.cpu()]
    return {"views": V, "quality": quality, "ms_per_call": ms, "us_per_view": ms * 1e3 / V, "scan_bytes_per_view": sum(out) / V,
            "rgb_bytes_per_view": W * H * 3, "workspace_bytes": int(ws.numel())}


def video_mode(pb, poses, times, tmp, repeats, quality):
    keep = ("frames", "seconds", "fps", "writer_wait_s", "writer_wait_at_end_s", "export_ms_per_view")
    vkeep = keep + ("encode_ms_per_view", "bytes")
    pb.write(poses[:24], times[:24], os.path.join(tmp, "warm_png"))                      # first-use costs stay out of every figure
    pb.write_video(poses[:24], times[:24], os.path.join(tmp, "warm_avi"), quality=quality)
    runs = {"png_files": [], "png_no_files": [], "video_files": [], "video_no_files": []}
    for r in range(repeats):
        a = pb.write(poses, times, os.path.join(tmp, f"png{r}"))
        runs["png_files"].append({k: a[k] for k in keep})
        b = pb.write_video(poses, times, os.path.join(tmp, f"avi{r}"), quality=quality)
        runs["video_files"].append({k: b[k] for k in vkeep})
        c = pb.write(poses, times, os.path.join(tmp, f"png_none{r}"), files=False)
        runs["png_no_files"].append({k: c[k] for k in keep})
        d = pb.write_video(poses, times, os.path.join(tmp, f"avi_none{r}"), quality=quality, files=False)
        runs["video_no_files"].append({k: d[k] for k in vkeep})
    summary = {k: {"fps_min": min(x["fps"] for x in v), "fps_max": max(x["fps"] for x in v)} for k, v in runs.items()}
    return {"runs": runs, "summary": summary}


def time_png_encode(colour, depth, repeats=20):
    """Per picture kind: ms per call of gsr_png_encode (filter Up) on the exported bytes of the given views, by device events around `repeats`
    back-to-back calls, and the stream bytes per view beside zlib level 1 on the same filtered bytes."""
    import zlib
    from slam import png, png_device
    V, _, H, W = colour.shape
    dev = colour.device
    lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    vis, u16 = torch.empty_like(rgb), torch.empty((V, H, W), dtype=torch.int16, device=dev)
    frame_io.frame_export(colour, depth, lut, DEPTH_VMAX, DEPTH_SCALE, rgb, vis, u16)
    out = []
    for name, pixels, kind in (("rgb", rgb, 0), ("depth_vis", vis, 0), ("depth", u16, 1)):
        stream = torch.empty((V, png_device.png_stream_bound(W, H, kind)), dtype=torch.uint8, device=dev)
        sizes = torch.empty((V,), dtype=torch.int32, device=dev)
        ws = torch.empty(png_device.png_workspace_size(V, W, H, kind), dtype=torch.uint8, device=dev)
        for _ in range(3):
            png_device.png_encode(pixels, stream, sizes, "up", ws)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            png_device.png_encode(pixels, stream, sizes, "up", ws)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / repeats
        host = pixels.cpu().numpy()
        host = host.view(np.uint16) if kind == 1 else host
        zl = [len(png.encode(host[v], "up", 1)) - 57 for v in range(V)]                  # the file less signature, IHDR, IEND and chunk framing
        got = [int(v) for v in sizes.cpu()]
        out.append({"picture": name, "views": V, "ms_per_call": ms, "us_per_view": ms * 1e3 / V, "stream_bytes_per_view": sum(got) / V,
                    "zlib_level1_bytes_per_view": sum(zl) / V, "ratio": sum(got) / sum(zl), "raw_bytes_per_view": int(pixels[0].numel()) * pixels.element_size(),
                    "workspace_bytes": int(ws.numel())})
    return out


def device_png_mode(pb, poses, times, tmp, repeats):
    keep = ("frames", "seconds", "fps", "writer_wait_s", "writer_wait_at_end_s", "export_ms_per_view")
    dkeep = keep + ("encode_ms_per_view", "bytes")
    pb.write(poses[:24], times[:24], os.path.join(tmp, "warm_host"), depth16=True)       # first-use costs stay out of every figure
    pb.write(poses[:24], times[:24], os.path.join(tmp, "warm_device"), depth16=True, device_png=True)
    runs = {"host": [], "device": [], "host_depth16": [], "device_depth16": [], "device_no_files": []}
    for r in range(repeats):
        for d16 in (False, True):
            tag = "_depth16" if d16 else ""
            a = pb.write(poses, times, os.path.join(tmp, f"host{tag}{r}"), depth16=d16)
            runs["host" + tag].append({k: a[k] for k in keep})
            b = pb.write(poses, times, os.path.join(tmp, f"device{tag}{r}"), depth16=d16, device_png=True)
            runs["device" + tag].append({k: b[k] for k in dkeep})
        c = pb.write(poses, times, os.path.join(tmp, f"device_none{r}"), files=False, device_png=True)
        runs["device_no_files"].append({k: c[k] for k in dkeep})
    summary = {k: {"fps_min": min(x["fps"] for x in v), "fps_max": max(x["fps"] for x in v)} for k, v in runs.items()}
    return {"runs": runs, "summary": summary}


def yardstick(pb, poses, times, out_dir):
    """The frames as the code before this module could produce them: one render() per frame, torch's clamp / scale / permute / .cpu(), PIL's
    encoder, matplotlib's colormap for the depth picture."""
    import matplotlib
    from matplotlib.colors import Normalize
    from PIL import Image
    from gaussian_renderer import render
    from slam.map_io import deltas_at
    jet, norm = matplotlib.colormaps["jet"], Normalize(0, DEPTH_VMAX)
    for k in ("rgb", "depth_vis"):
        os.makedirs(os.path.join(out_dir, k), exist_ok=True)
    cams = pb._cameras(poses, times)
    stage = {"render_and_copy_s": 0.0, "rgb_png_s": 0.0, "depth_colour_s": 0.0, "depth_png_s": 0.0}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for i, c in enumerate(cams):
            a = time.perf_counter()
            dx, ds, dr = deltas_at(pb.gaussians, c)
            pkg = render(c, pb.gaussians, pb.pipe, pb.background, dx=dx, ds=ds, dr=dr)
            rgb = (torch.clamp(pkg["render"], 0.0, 1.0) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
            depth = pkg["depth"][0].cpu().numpy()
            b = time.perf_counter()
            Image.fromarray(rgb).save(os.path.join(out_dir, "rgb", f"{i}.png"))
            c_ = time.perf_counter()
            vis = jet(norm(depth), bytes=True)[..., :3]
            d = time.perf_counter()
            Image.fromarray(np.ascontiguousarray(vis)).save(os.path.join(out_dir, "depth_vis", f"{i}.png"))
            e = time.perf_counter()
            stage["render_and_copy_s"] += b - a
            stage["rgb_png_s"] += c_ - b
            stage["depth_colour_s"] += d - c_
            stage["depth_png_s"] += e - d
    seconds = time.perf_counter() - t0
    return {"frames": len(cams), "seconds": seconds, "fps": len(cams) / seconds, **stage}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--map", default=None, help="a saved map to play (default: run the dynamic 640x480 synthetic SLAM first)")
    ap.add_argument("--out", default=None, help="default: profiles/playback.json, or profiles/playback_video.json with --video")
    ap.add_argument("--video", action="store_true", help="the video mode: PNG files and Motion-JPEG AVI files alternated on the same path")
    ap.add_argument("--encode-only", action="store_true", help="with --video: only the gsr_jpeg_encode timing")
    ap.add_argument("--device-png", action="store_true", help="the lossless mode: PNG files by the host's zlib and by the device's encoder, alternated")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args(argv)
    if args.video and args.device_png:
        ap.error("--video and --device-png are two modes: pick one")
    args.out = args.out or os.path.join(REPO, "profiles", "playback_video.json" if args.video else
                                        "playback_device_png.json" if args.device_png else "playback.json")
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        directory = args.map or build_map(os.path.join(tmp, "map"))
        built = time.perf_counter() - t0
        loaded = load_map(directory, "cuda:0")
        pb = Playback(loaded)
        poses, times = resampled(loaded, args.frames)
        colour, depth, _ = pb.render(poses[:12], times[:12])
        if args.video:
            out = {"device": torch.cuda.get_device_name(0), "resolution": [pb.width, pb.height], "frames": args.frames,
                   "gaussians": int(loaded.gaussians.get_xyz.shape[0]), "quality": args.quality,
                   "gsr_jpeg_encode": [time_encode(pb, colour[:1], depth[:1], args.quality), time_encode(pb, colour, depth, args.quality)]}
            if not args.encode_only:
                out.update(video_mode(pb, poses, times, tmp, args.repeats, args.quality))
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
            print(json.dumps(out))
            return
        if args.device_png:
            out = {"device": torch.cuda.get_device_name(0), "resolution": [pb.width, pb.height], "frames": args.frames,
                   "gaussians": int(loaded.gaussians.get_xyz.shape[0]),
                   "gsr_png_encode": [time_png_encode(colour[:1], depth[:1]), time_png_encode(colour, depth)]}
            out.update(device_png_mode(pb, poses, times, tmp, args.repeats))
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
            print(json.dumps(out))
            return
        export = [time_export(colour[:1], depth[:1]), time_export(colour, depth)]
        pb.write(poses[:24], times[:24], os.path.join(tmp, "warm"))                      # first-use costs (streams, pinned memory, zlib) stay out
        keep = ("frames", "seconds", "fps", "writer_wait_s", "writer_wait_at_end_s", "export_ms_per_view")
        no_files = pb.write(poses, times, os.path.join(tmp, "none"), files=False)
        with_files = pb.write(poses, times, os.path.join(tmp, "files"))
        with_files_16 = pb.write(poses, times, os.path.join(tmp, "files16"), depth16=True)
        t0 = time.perf_counter()
        pb.render(poses, times)
        torch.cuda.synchronize()
        render_only = time.perf_counter() - t0
        yard = yardstick(pb, poses, times, os.path.join(tmp, "yardstick"))
        out = {"device": torch.cuda.get_device_name(0), "resolution": [pb.width, pb.height], "gaussians": int(loaded.gaussians.get_xyz.shape[0]),
               "dynamic_gaussians": int(loaded.gaussians.dygs.sum()), "map_seconds": None if args.map else built,
               "gsr_frame_export": export,
               "render_only": {"frames": args.frames, "seconds": render_only, "fps": args.frames / render_only},
               "playback_without_files": {k: no_files[k] for k in keep},
               "playback_rgb_and_depth_vis_files": {k: with_files[k] for k in keep},
               "playback_rgb_depth_vis_and_depth16_files": {k: with_files_16[k] for k in keep},
               "yardstick_per_frame_render_pil_matplotlib": yard}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
