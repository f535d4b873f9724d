#!/usr/bin/env python
"""Play a saved 4D map (slam/map_io.py) back to image files (slam/playback.py):
  play_map.py --map DIR --path tracked|frozen-time:T|frozen-camera:I:N|resample:N --out DIR [--depth16] [--no-depth-vis]
writes rgb/*.png, depth_vis/*.png (jet, 0-6 m) and, with --depth16, depth/*.png plus the lists of a TUM sequence; prints one JSON line with
the frames written, the seconds, frames per second and the time the loop waited for the writer thread.
  play_map.py --map DIR --path ... --out DIR --video [--fps F] [--quality Q] [--no-depth-vis]
writes rgb.avi and depth_vis.avi instead: Motion-JPEG in AVI, compressed on the device (slam/mjpeg.py); the JSON line gains "video": true,
"bytes" and "encode_ms".
  play_map.py --map DIR --path ... --out DIR --device-png [--depth16] [--no-depth-vis]
writes the same PNG files and lists as the first form, compressed on the device (slam/png_device.py); the JSON line gains
"device_png": true, "bytes" and "encode_ms"."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--map", required=True, help="directory written by SLAM.save_map / run_slam.py --save-map")
    ap.add_argument("--path", default="tracked", help="tracked | frozen-time:T | frozen-camera:I:N | resample:N")
    ap.add_argument("--out", required=True)
    ap.add_argument("--depth16", action="store_true", help="also write 16-bit depth and the TUM lists")
    ap.add_argument("--no-depth-vis", action="store_true", help="do not write the jet-coloured depth pictures")
    ap.add_argument("--video", action="store_true", help="write Motion-JPEG AVI files (rgb.avi, depth_vis.avi) instead of PNG folders")
    ap.add_argument("--device-png", action="store_true", help="compress the PNG files on the device instead of with the host's zlib")
    ap.add_argument("--fps", type=float, default=30.0, help="frame rate of the video files")
    ap.add_argument("--quality", type=int, default=90, help="JPEG quality of the video frames, 1 .. 100")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from slam.map_io import load_map
    from slam.playback import Playback, parse_path
    loaded = load_map(args.map, args.device)
    poses, times = parse_path(loaded, args.path)
    if args.video and args.depth16:
        ap.error("--depth16 has no video form: the 16-bit depth is written as PNG files only")
    if args.video and args.device_png:
        ap.error("--device-png compresses PNG files: it does not go with --video")
    extra = {}
    if args.video:
        res = Playback(loaded).write_video(poses, times, args.out, fps=args.fps, quality=args.quality, depth_colour=not args.no_depth_vis)
        extra = {"video": True, "bytes": res["bytes"], "encode_ms": res["encode_ms"]}
    else:
        res = Playback(loaded).write(poses, times, args.out, depth16=args.depth16, depth_colour=not args.no_depth_vis, device_png=args.device_png)
        if args.device_png:
            extra = {"device_png": True, "bytes": res["bytes"], "encode_ms": res["encode_ms"]}
    print(json.dumps({"map": args.map, "path": args.path, "out": args.out, "frames": res["frames"], "seconds": res["seconds"],
                      "fps": res["fps"], "writer_wait_s": res["writer_wait_s"], "gaussians": int(loaded.gaussians.get_xyz.shape[0]),
                      "dynamic": loaded.dynamic, **extra}))


if __name__ == "__main__":
    main()
