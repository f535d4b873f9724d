"""Playing a 4D map back: rendering it from any pose at any time, and writing the frames as image files.

Playback(map_like) takes a map_io.LoadedMap or the live SLAM object. render(poses, times) is forward-only: chunks of at most 12 views through
gaussian_renderer.render_views (one launch per pipeline stage for the chunk), with ONE batched evaluation of the node network and one blend
launch for the distinct times of a chunk (ControlNodes.begin_iteration(blend=...)). write(...) exports every chunk with one gsr_frame_export
launch, copies the bytes into pinned ring buffers on a side stream and hands them to one writer thread (slam/png.py); the loop waits only
when it must reuse a ring slot, and once at the end. write_video(...) sends the same exported bytes through the device's JPEG encoder
(slam/mjpeg.py, gsr_jpeg_encode) instead and writes one Motion-JPEG AVI file per image kind; the host copies only the compressed bytes.
write(..., device_png=True) does the same for the lossless files: the device's deflate encoder (slam/png_device.py, gsr_png_encode) makes
each picture's zlib stream and the writer thread only frames and writes it.

Camera paths are plain functions that return (poses, times): poses float32 [N, 4, 4] world-to-camera matrices on the host, times a list of
floats in the map's normalised time. The reference's `novel=` argument of render() is dead code there and has no counterpart."""
import os
import queue
import threading
import time as _time

import numpy as np
import torch

from . import frame_io, mjpeg, png
from .map_io import LoadedMap

CHUNK = 12                     # views per render_views call (diff_gaussian_rasterization.views.MAX_VIEWS)
RING = 3                       # pinned slots: one being filled by the device, one with the writer, one spare
DEPTH_VMAX = 6.0               # the reference's depth pictures: imshow(cmap="jet", vmin=0, vmax=6) (utils/eval_utils.py:62)
DEPTH_SCALE = 5000.0           # TUM's 16-bit depth unit


# ---- camera paths ------------------------------------------------------------------------------------------------------------------
def _view(map_like):
    """(gaussians, {uid: camera}, background, pipeline_params) of a LoadedMap or a live SLAM object."""
    if isinstance(map_like, LoadedMap):
        return map_like.gaussians, map_like.cameras, map_like.background, map_like.pipeline_params
    return map_like.gaussians, map_like.frontend.cameras, map_like.background, map_like.pipeline_params


def _tracked_cameras(map_like):
    cams = _view(map_like)[1]
    return [cams[k] for k in sorted(cams.keys())]


def _w2c(cameras):
    """float32 [N, 4, 4] world-to-camera matrices of cameras' estimated poses, bit for bit (one stack on their device, one copy)."""
    R = torch.stack([c.R.detach() for c in cameras]).to(torch.float32).cpu()
    T = torch.stack([c.T.detach() for c in cameras]).to(torch.float32).cpu()
    out = torch.eye(4, dtype=torch.float32).repeat(len(cameras), 1, 1)
    out[:, :3, :3], out[:, :3, 3] = R, T
    return out


def tracked(map_like):
    """The estimated poses of the tracked frames at their own times."""
    cams = _tracked_cameras(map_like)
    return _w2c(cams), [float(c.time) for c in cams]


def frozen_time(map_like, t):
    """The tracked poses with the scene held at time t."""
    poses, times = tracked(map_like)
    return poses, [float(t)] * len(times)


def frozen_camera(map_like, frame, n):
    """The pose of tracked frame `frame` (its position in the run), with n times from the run's first to its last."""
    poses, times = tracked(map_like)
    return poses[frame:frame + 1].repeat(n, 1, 1).clone(), [float(v) for v in np.linspace(times[0], times[-1], n)]


def _quaternion(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix, float64 (Shepperd's method)."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = ((R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s)
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = ((R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s)
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = ((R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s)
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def _rotation(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float64)


def slerp(q0, q1, u):
    """Spherical interpolation of unit quaternions on the shorter arc (q1 is negated when the two are more than 90 degrees apart in
    quaternion space, i.e. the rotation between them is taken the short way round)."""
    d = float(np.dot(q0, q1))
    if d < 0.0:
        q1, d = -q1, -d
    if d > 1.0 - 1e-12:                                   # (nearly) the same rotation: the linear form, renormalised
        q = (1.0 - u) * q0 + u * q1
        return q / np.linalg.norm(q)
    th = np.arccos(d)
    return (np.sin((1.0 - u) * th) * q0 + np.sin(u * th) * q1) / np.sin(th)


def interpolate_poses(poses, times, n):
    """n poses along the polyline of the given K world-to-camera poses: between two consecutive knots the camera-to-world rotation by slerp
    on the shorter arc, the camera centre and the time linearly. With n >= K every knot is among the samples, bit for bit (pose and time),
    and the n - K others are spread over the segments as evenly as integers allow, evenly spaced inside a segment; with n < K the parameter
    runs evenly from the first knot to the last, and the two ends (and any knot a sample falls on) are exact."""
    poses = torch.as_tensor(poses, dtype=torch.float32)
    K = int(poses.shape[0])
    if K < 2 or n < 2:
        raise ValueError("interpolate_poses needs at least two knots and two samples")
    if n >= K:
        extra = n - K
        samples = []                                                          # (segment, numerator, denominator): u = numerator / denominator
        for j in range(K - 1):
            inside = (j + 1) * extra // (K - 1) - j * extra // (K - 1)
            samples += [(j, m, inside + 1) for m in range(inside + 1)]
        samples.append((K - 2, 1, 1))
    else:
        samples = [divmod(i * (K - 1), n - 1) + (n - 1,) for i in range(n - 1)] + [(K - 2, 1, 1)]
    P = poses.numpy().astype(np.float64)
    Rc = np.transpose(P[:, :3, :3], (0, 2, 1))                                # camera-to-world rotations
    C = -np.einsum("kij,kj->ki", Rc, P[:, :3, 3])                             # camera centres
    Q = [_quaternion(r) for r in Rc]
    out = torch.eye(4, dtype=torch.float32).repeat(n, 1, 1)
    out_t = []
    for i, (k, num, den) in enumerate(samples):
        if num == 0 or num == den:
            k += num == den
            out[i] = poses[k]
            out_t.append(float(times[k]))
            continue
        u = num / den
        R = _rotation(slerp(Q[k], Q[k + 1], u)).T                             # back to world-to-camera
        c = (1.0 - u) * C[k] + u * C[k + 1]
        out[i, :3, :3] = torch.from_numpy(R.astype(np.float32))
        out[i, :3, 3] = torch.from_numpy((-R @ c).astype(np.float32))
        out_t.append(float((1.0 - u) * times[k] + u * times[k + 1]))
    return out, out_t


def resampled(map_like, n):
    """n poses interpolated between consecutive tracked poses, times alike (interpolate_poses)."""
    return interpolate_poses(*tracked(map_like), n)


def parse_path(map_like, spec):
    """tracked | frozen-time:T | frozen-camera:I:N | resample:N -> (poses, times)."""
    kind, _, rest = spec.partition(":")
    args = rest.split(":") if rest else []
    try:
        if kind == "tracked" and not args:
            return tracked(map_like)
        if kind == "frozen-time" and len(args) == 1:
            return frozen_time(map_like, float(args[0]))
        if kind == "frozen-camera" and len(args) == 2:
            return frozen_camera(map_like, int(args[0]), int(args[1]))
        if kind == "resample" and len(args) == 1:
            return resampled(map_like, int(args[0]))
    except ValueError as e:
        raise ValueError(f"camera path {spec!r}: {e}") from None
    raise ValueError(f"camera path {spec!r}: expected tracked, frozen-time:T, frozen-camera:I:N or resample:N")


# ---- rendering ---------------------------------------------------------------------------------------------------------------------
def _as_batch(tensors):
    """The equally shaped, contiguous tensors as ONE [V, ...] tensor without a copy when they lie at a constant distance in one allocation
    (the multi-view rasterizer's output block); a stack otherwise."""
    first = tensors[0]
    if len(tensors) == 1:
        return first[None]
    if all(t.is_contiguous() and t.shape == first.shape and t.dtype == first.dtype for t in tensors):
        base, step = first.data_ptr(), tensors[1].data_ptr() - first.data_ptr()
        same = all(t.untyped_storage().data_ptr() == first.untyped_storage().data_ptr() for t in tensors)
        if same and step >= first.numel() * first.element_size() and step % first.element_size() == 0 and \
                all(t.data_ptr() == base + v * step for v, t in enumerate(tensors)):
            return torch.as_strided(first, (len(tensors),) + tuple(first.shape), (step // first.element_size(),) + tuple(first.stride()))
    return torch.stack(tensors)


class Playback:
    def __init__(self, map_like):
        self.map = map_like
        self.gaussians, cams, self.background, self.pipe = _view(map_like)
        if not cams:
            raise ValueError("Playback: the map has no tracked frame")
        self._like = cams[sorted(cams.keys())[0]]                         # intrinsics, projection and image size of every view
        self.device = self.gaussians.get_xyz.device
        self.height, self.width = int(self._like.image_height), int(self._like.image_width)

    # -- cameras: built once per call, ahead of the render loop (their uploads would otherwise sit between its launches) --
    def _cameras(self, poses, times):
        from .camera import Camera
        poses = torch.as_tensor(poses, dtype=torch.float32)
        if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] != len(times):
            raise ValueError(f"poses must be [N, 4, 4] world-to-camera matrices with one time each, got {tuple(poses.shape)} and {len(times)} times")
        k = self._like
        dev_poses = poses.to(self.device)
        gt = torch.eye(4)
        cams = []
        for i, t in enumerate(times):
            c = Camera(i, None, None, gt, k.projection_matrix, k.fx, k.fy, k.cx, k.cy, k.FoVx, k.FoVy, self.height, self.width, float(t),
                       device=self.device)
            c._R.copy_(dev_poses[i, :3, :3])
            c._T.copy_(dev_poses[i, :3, 3])
            c.refresh_matrices()
            cams.append(c)
        return cams

    def _deltas(self, cams):
        """(d_xyz, d_scaling, d_rotation) per camera of a chunk, from one batched node-network evaluation and one blend launch for the
        chunk's distinct times; None per camera for a map without an initialised node network (BackEnd._deltas(train=False)'s rule)."""
        g = self.gaussians
        if not (g.deform is not None and g.deform_init and g.dyn_rows().shape[0] > 0):
            return [None] * len(cams)
        nodes = g.deform.deform
        x, mask = g.get_dygs_xyz.detach(), g.motion_mask
        nodes.begin_iteration([c.time for c in cams], blend=(x, mask))
        try:
            out = []
            for c in cams:
                d = g.deform.step(x, nodes.expand_time(c.fid), iteration=0, feature=None, motion_mask=mask, camera_center=c.camera_center,
                                  time_interval=g.time_interval, t_key=c.time)
                out.append((d["d_xyz"], d["d_scaling"], d["d_rotation"]))
            return out
        finally:
            nodes.end_iteration()

    def _chunks(self, cams):
        """(first index, colour [V,3,H,W], depth [V,1,H,W], opacity [V,1,H,W]) per chunk of at most CHUNK views."""
        from gaussian_renderer import render_views
        for lo in range(0, len(cams), CHUNK):
            part = cams[lo:lo + CHUNK]
            pkgs = render_views(part, self.gaussians, self.pipe, self.background, deltas=self._deltas(part))
            if any(p is None for p in pkgs):
                raise RuntimeError("Playback: the map has no Gaussians")
            yield lo, _as_batch([p["render"] for p in pkgs]), _as_batch([p["depth"] for p in pkgs]), _as_batch([p["opacity"] for p in pkgs])

    @torch.no_grad()
    def render(self, poses, times):
        """(colour [N,3,H,W], depth [N,1,H,W], opacity [N,1,H,W]) on the device."""
        cams = self._cameras(poses, times)
        N, H, W = len(cams), self.height, self.width
        colour = torch.empty((N, 3, H, W), dtype=torch.float32, device=self.device)
        depth, opacity = (torch.empty((N, 1, H, W), dtype=torch.float32, device=self.device) for _ in range(2))
        for lo, c, d, o in self._chunks(cams):
            colour[lo:lo + c.shape[0]], depth[lo:lo + c.shape[0]], opacity[lo:lo + c.shape[0]] = c, d, o
        return colour, depth, opacity

    # -- files ----------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def write(self, poses, times, out_dir, depth16=False, depth_colour=True, depth_vmax=DEPTH_VMAX, depth_scale=DEPTH_SCALE, png_filter="up",
              png_level=1, files=True, device_png=False):
        """Render and write rgb/<stamp>.png, depth_vis/<stamp>.png (jet, 0 .. depth_vmax; depth_colour=False: not written) and, with
        depth16, depth/<stamp>.png (16 bit, depth * depth_scale) plus rgb.txt, depth.txt and groundtruth.txt, so that the folder is a TUM
        sequence; <stamp> as recorded.write_tum_sequence names frames. files=False runs everything but the encoding and the disk (for
        measurements). Returns {"frames", "seconds", "fps", "writer_wait_s", "export_ms", "calibration"}. device_png=True compresses on
        the device instead (slam/png_device.py, one gsr_png_encode per chunk and image kind): the host copies only the compressed bytes and
        the writer thread only frames them (png.assemble) and writes; the same file names, pixels and lists; the dict gains "encode_ms" and
        "bytes" (the PNG bytes of all frames); files=False then still encodes. png_level has no meaning there and must be left alone."""
        from . import recorded
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Playback.write allocates pinned buffers and synchronises with its writer: not while a graph is being captured")
        if device_png:
            if png_level != 1:
                raise ValueError(f"png_level has no meaning with device_png (the device's encoder has one setting), got {png_level!r}")
            if png_filter not in png.FILTERS:
                raise ValueError(f"png_filter must be one of {sorted(png.FILTERS)}, got {png_filter!r}")
            return self._write_device_png(poses, times, out_dir, depth16, depth_colour, depth_vmax, depth_scale, png_filter, files)
        dev, H, W = self.device, self.height, self.width
        t0 = _time.perf_counter()                                    # (the cameras and the buffers are part of the time reported)
        cams = self._cameras(poses, times)
        N = len(cams)
        stamps = [recorded.tum_stamp(i) for i in range(N)]
        kinds = ["rgb"] + (["depth_vis"] if depth_colour else []) + (["depth"] if depth16 else [])
        if files:
            for k in kinds:
                os.makedirs(os.path.join(out_dir, k), exist_ok=True)
        u16 = getattr(torch, "uint16", torch.int16)
        shapes = {"rgb": ((CHUNK, H, W, 3), torch.uint8), "depth_vis": ((CHUNK, H, W, 3), torch.uint8), "depth": ((CHUNK, H, W), u16)}
        # pinned buffers on the calling thread, before the loop (recorded.py: the host allocator is not touched from the writer thread, and
        # never during a capture); the device byte buffers belong to the slot as well, so a slot is reused only when its copy has been written
        slots = [{"dev": {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in kinds},
                  "host": {k: torch.empty(shapes[k][0], dtype=shapes[k][1]).pin_memory() for k in kinds}}
                 for _ in range(min(RING, max(1, -(-N // CHUNK))))]
        lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
        free, jobs, errors = queue.Queue(), queue.Queue(), []
        for s in slots:
            free.put(s)

        def writer():
            while True:
                job = jobs.get()
                if job is None:
                    return
                slot, lo, n, done = job
                try:
                    done.synchronize()
                    if files and not errors:
                        for k in kinds:
                            a = slot["host"][k].numpy() if slot["host"][k].dtype != torch.int16 else slot["host"][k].numpy().view(np.uint16)
                            for v in range(n):
                                png.write(os.path.join(out_dir, k, stamps[lo + v] + ".png"), a[v], png_filter, png_level)
                except BaseException as e:                           # surfaced by the caller after the loop
                    errors.append(e)
                finally:
                    free.put(slot)

        thread = threading.Thread(target=writer, name="playback-writer", daemon=True)
        thread.start()
        main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
        timing = []
        wait = 0.0
        try:
            for lo, colour, depth, _ in self._chunks(cams):
                n = int(colour.shape[0])
                w0 = _time.perf_counter()
                slot = free.get()                                    # the only wait inside the loop: every slot is still with the writer
                wait += _time.perf_counter() - w0
                out = {k: t[:n] for k, t in slot["dev"].items()}
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record(main)
                frame_io.frame_export(colour, depth, lut, depth_vmax, depth_scale, out["rgb"], out.get("depth_vis"), out.get("depth"), main)
                ev[1].record(main)
                timing.append((ev, n))
                side.wait_event(ev[1])
                with torch.cuda.stream(side):
                    for k in kinds:
                        slot["host"][k][:n].copy_(out[k], non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(side)
                jobs.put((slot, lo, n, done))
        finally:
            jobs.put(None)
            w0 = _time.perf_counter()
            thread.join()                                            # the one wait at the end
            wait_end = _time.perf_counter() - w0
        if errors:
            raise errors[0]
        torch.cuda.synchronize(dev)
        seconds = _time.perf_counter() - t0
        if files and depth16:
            c2w = [np.linalg.inv(p) for p in torch.as_tensor(poses, dtype=torch.float32).numpy().astype(np.float64)]
            recorded.write_tum_lists(out_dir, stamps, c2w, origin="played back from a saved map")
        k = self._like
        export_ms = sum(a.elapsed_time(b) for (a, b), _ in timing)
        return {"frames": N, "seconds": seconds, "fps": N / seconds if seconds > 0 else float("inf"), "writer_wait_s": wait,
                "writer_wait_at_end_s": wait_end, "export_ms": export_ms, "export_ms_per_view": export_ms / max(N, 1),
                "calibration": {"fx": float(k.fx), "fy": float(k.fy), "cx": float(k.cx), "cy": float(k.cy), "k1": 0.0, "k2": 0.0, "p1": 0.0,
                                "p2": 0.0, "k3": 0.0, "distorted": False, "width": W, "height": H, "depth_scale": float(depth_scale)}}

    def _compressed(self, cams, kinds, shapes, cap, depth_vmax, depth_scale, encode, emit, check=None, name="playback-writer"):
        """The loop write_video and write(device_png=True) share. Per chunk: one gsr_frame_export, then encode(kind, pixels [n, ...], out
        [n, cap[kind]], sizes [n], stream) per image kind on the main stream; the chunk's sizes are copied on a side stream, and the ONE writer
        thread, once they are on the host, runs check(sizes [kinds, n], first frame) (it may raise), copies just the used bytes and calls
        emit(kind, frame, bytes) per picture. The loop waits only for a free slot and once at the end. Returns (writer_wait_s,
        writer_wait_at_end_s, export_ms, encode_ms); the writer's first error is raised after the loop."""
        dev = self.device
        # a slot owns the exported bytes, the compressed bytes and their sizes on the device, and the pinned copies of the last two
        slots = [{"dev": {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in kinds},
                  "scan": {k: torch.empty((CHUNK, cap[k]), dtype=torch.uint8, device=dev) for k in kinds},
                  "sizes": torch.empty((len(kinds), CHUNK), dtype=torch.int32, device=dev),
                  "host": {k: torch.empty((CHUNK, cap[k]), dtype=torch.uint8).pin_memory() for k in kinds},
                  "host_sizes": torch.empty((len(kinds), CHUNK), dtype=torch.int32).pin_memory()}
                 for _ in range(min(RING, max(1, -(-len(cams) // CHUNK))))]
        lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
        free, jobs, errors = queue.Queue(), queue.Queue(), []
        for s in slots:
            free.put(s)
        main, side = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)

        def writer():
            while True:
                job = jobs.get()
                if job is None:
                    return
                slot, lo, n, sized = job
                try:
                    sized.synchronize()                              # the sizes are on the host: copy just the bytes that were used
                    sizes = slot["host_sizes"].numpy()[:, :n].copy()
                    if check is not None:
                        check(sizes, lo)
                    if errors:
                        continue
                    with torch.cuda.stream(side):
                        for ki, k in enumerate(kinds):
                            for v in range(n):
                                slot["host"][k][v, :int(sizes[ki, v])].copy_(slot["scan"][k][v, :int(sizes[ki, v])], non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(side)
                    done.synchronize()
                    for ki, k in enumerate(kinds):
                        a = slot["host"][k].numpy()
                        for v in range(n):
                            emit(k, lo + v, a[v, :int(sizes[ki, v])].tobytes())
                except BaseException as e:                           # surfaced by the caller after the loop
                    errors.append(e)
                finally:
                    free.put(slot)

        thread = threading.Thread(target=writer, name=name, daemon=True)
        thread.start()
        timing, export_timing = [], []
        wait = 0.0
        try:
            for lo, colour, depth, _ in self._chunks(cams):
                n = int(colour.shape[0])
                w0 = _time.perf_counter()
                slot = free.get()                                    # the only wait inside the loop: every slot is still with the writer
                wait += _time.perf_counter() - w0
                if errors:
                    break
                out = {k: t[:n] for k, t in slot["dev"].items()}
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record(main)
                frame_io.frame_export(colour, depth, lut, depth_vmax, depth_scale, out["rgb"], out.get("depth_vis"), out.get("depth"), main)
                ev[1].record(main)
                for ki, k in enumerate(kinds):
                    encode(k, out[k], slot["scan"][k][:n], slot["sizes"][ki, :n], main)
                ev[2].record(main)
                export_timing.append((ev[0], ev[1]))
                timing.append((ev[1], ev[2]))
                side.wait_event(ev[2])
                with torch.cuda.stream(side):
                    slot["host_sizes"].copy_(slot["sizes"], non_blocking=True)
                    sized = torch.cuda.Event()
                    sized.record(side)
                jobs.put((slot, lo, n, sized))
        finally:
            jobs.put(None)
            w0 = _time.perf_counter()
            thread.join()                                            # the one wait at the end
            wait_end = _time.perf_counter() - w0
        if errors:
            raise errors[0]
        torch.cuda.synchronize(dev)
        return wait, wait_end, sum(a.elapsed_time(b) for a, b in export_timing), sum(a.elapsed_time(b) for a, b in timing)

    def _result(self, N, t0, wait, wait_end, export_ms, encode_ms, total, depth_scale, **more):
        seconds = _time.perf_counter() - t0
        k = self._like
        return {"frames": N, "seconds": seconds, "fps": N / seconds if seconds > 0 else float("inf"), "writer_wait_s": wait,
                "writer_wait_at_end_s": wait_end, "export_ms": export_ms, "export_ms_per_view": export_ms / max(N, 1), **more,
                "bytes": total, "encode_ms": encode_ms, "encode_ms_per_view": encode_ms / max(N, 1),
                "calibration": {"fx": float(k.fx), "fy": float(k.fy), "cx": float(k.cx), "cy": float(k.cy), "k1": 0.0, "k2": 0.0, "p1": 0.0,
                                "p2": 0.0, "k3": 0.0, "distorted": False, "width": self.width, "height": self.height,
                                "depth_scale": float(depth_scale)}}

    def _write_device_png(self, poses, times, out_dir, depth16, depth_colour, depth_vmax, depth_scale, png_filter, files):
        """write(device_png=True): gsr_png_encode per chunk and image kind; the writer thread frames each stream as a file and writes it."""
        from . import png_device, recorded
        dev, H, W = self.device, self.height, self.width
        t0 = _time.perf_counter()
        cams = self._cameras(poses, times)
        N = len(cams)
        stamps = [recorded.tum_stamp(i) for i in range(N)]
        kinds = ["rgb"] + (["depth_vis"] if depth_colour else []) + (["depth"] if depth16 else [])
        if files:
            for k in kinds:
                os.makedirs(os.path.join(out_dir, k), exist_ok=True)
        u16 = getattr(torch, "uint16", torch.int16)
        shapes = {"rgb": ((CHUNK, H, W, 3), torch.uint8), "depth_vis": ((CHUNK, H, W, 3), torch.uint8), "depth": ((CHUNK, H, W), u16)}
        code = {k: 1 if k == "depth" else 0 for k in kinds}                       # the encoder's picture kind
        cap = {k: png_device.png_stream_bound(W, H, code[k]) for k in kinds}      # the worst case: no picture can fail to fit
        if min(cap.values()) == 0:
            raise ValueError(f"Playback.write: {W} x {H} pictures are outside what the device's PNG encoder takes")
        workspace = torch.empty(max(png_device.png_workspace_size(CHUNK, W, H, c) for c in set(code.values())), dtype=torch.uint8,
                                device=dev)                                      # shared: the encodes run in stream order
        total = [0]

        def encode(k, pixels, out, sizes, main):
            png_device.png_encode(pixels, out, sizes, png_filter, workspace, main)

        def emit(k, i, stream):
            data = png.assemble(W, H, code[k], stream)
            total[0] += len(data)
            if files:
                with open(os.path.join(out_dir, k, stamps[i] + ".png"), "wb") as f:
                    f.write(data)

        timings = self._compressed(cams, kinds, shapes, cap, depth_vmax, depth_scale, encode, emit, name="playback-png-writer")
        result = self._result(N, t0, *timings, total[0], depth_scale)                 # (the lists stay out of the time, as in write())
        if files and depth16:
            c2w = [np.linalg.inv(p) for p in torch.as_tensor(poses, dtype=torch.float32).numpy().astype(np.float64)]
            recorded.write_tum_lists(out_dir, stamps, c2w, origin="played back from a saved map")
        return result

    @torch.no_grad()
    def write_video(self, poses, times, out_dir, fps=30.0, quality=90, depth_colour=True, depth_vmax=DEPTH_VMAX, files=True, capacity=None):
        """Render and write rgb.avi and depth_vis.avi (jet, 0 .. depth_vmax; depth_colour=False: not written): Motion-JPEG in AVI 1.0
        (slam/mjpeg.py), each frame a baseline JPEG of the given quality, compressed on the device from the bytes gsr_frame_export writes (one
        gsr_jpeg_encode call per chunk and image kind). capacity: the bytes a compressed frame may take (default max(W * H * 3, 65536)); a
        frame that needs more raises RuntimeError with its index and its size, after the files are closed validly. files=False runs everything
        but the disk (for measurements). Returns write()'s dict plus "files", "bytes" (the JPEG bytes of all frames) and "encode_ms"
        (gsr_jpeg_encode by device events, read after the last chunk)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("Playback.write_video allocates pinned buffers and synchronises with its writer: not while a graph is being captured")
        dev, H, W = self.device, self.height, self.width
        t0 = _time.perf_counter()
        qtables = mjpeg.quant_tables(quality)
        header = mjpeg.jfif_header(W, H, qtables)
        cap = int(capacity) if capacity is not None else max(W * H * 3, 65536)
        if cap < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        cams = self._cameras(poses, times)
        N = len(cams)
        kinds = ["rgb"] + (["depth_vis"] if depth_colour else [])
        paths = {k: os.path.join(out_dir, k + ".avi") for k in kinds}
        writers = {}
        if files:
            os.makedirs(out_dir, exist_ok=True)
            writers = {k: mjpeg.AviWriter(paths[k], W, H, fps) for k in kinds}
        q_dev = torch.from_numpy(qtables.astype(np.int16)).to(dev)
        workspace = torch.empty(mjpeg.jpeg_workspace_size(CHUNK, W, H), dtype=torch.uint8, device=dev)   # shared: the encodes run in stream order
        total = [0]

        def encode(k, pixels, out, sizes, main):
            mjpeg.jpeg_encode(pixels, q_dev, out, sizes, None, workspace, main)

        def check(sizes, lo):
            if (sizes < 0).any():
                ki, v = (int(a[0]) for a in np.nonzero(sizes < 0))
                raise RuntimeError(f"frame {lo + v} ({kinds[ki]}) needs {-int(sizes[ki, v])} bytes as a JPEG, its capacity is {cap}: "
                                   f"pass a larger capacity or a lower quality")

        def emit(k, i, scan):
            total[0] += len(header) + len(scan) + 2
            if files:
                writers[k].add(header + scan + mjpeg.EOI)

        try:
            timings = self._compressed(cams, kinds, {k: ((CHUNK, H, W, 3), torch.uint8) for k in kinds}, {k: cap for k in kinds}, depth_vmax,
                                       DEPTH_SCALE, encode, emit, check, name="playback-video-writer")
        finally:
            for w in writers.values():
                w.close()
        return self._result(N, t0, *timings, total[0], DEPTH_SCALE, files=[paths[k] for k in kinds] if files else [])
