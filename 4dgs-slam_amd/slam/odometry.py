"""Dense frame-to-frame visual odometry: the checked ctypes binding of include/visual_odometry.h (gsr_odometry_pyramid: an intensity / depth
pyramid of a frame; gsr_odometry_align: coarse-to-fine photometric Gauss-Newton on SE(3) with Student-t weights and an acceptance gate on the
device, csrc/gs_odometry.h) and ``DenseOdometry``, which keeps the previous frame's pyramid. The front-end starts a frame's tracking from its
result (slam/stages.py, ``Training.pose_prior``); the reference starts at the previous pose and has no counterpart.
tests/odometry_reference.py restates the contract in numpy. No CPU path.

gsr_odometry_align_rgbd (``align_pyramids_rgbd``; ``DenseOdometry(affine=..., geometric_weight=...)``) adds an affine brightness between the two
frames and an inverse-depth term against the current frame's depth; tests/odometry_rgbd_reference.py restates it.

Limits: without ``affine`` brightness changes between the two frames are not modelled (the tracker's exposure terms come after this step); a
mover that is not masked is only down-weighted; nothing here has been run on real images, real depth noise or a rolling shutter."""
import ctypes
import math

import torch

from diff_gaussian_rasterization import _C

from .camera import frame_tensors
from .pretrained import EventLog

STATS = ("accepted", "inlier_share", "sigma", "last_step", "pixels_in", "translation", "angle", "valid_depths")
TRACE_ROW = 32
STATS_RGBD = STATS + ("alpha", "beta", "sigma_depth", "depth_terms")          # of gsr_odometry_align_rgbd
TRACE_ROW_RGBD = 64


def pyramid_size(width, height, levels):
    return int(_C.load_library().gsr_odometry_pyramid_size(int(width), int(height), int(levels)))


def align_workspace_size(width, height, levels):
    return int(_C.load_library().gsr_odometry_align_workspace_size(int(width), int(height), int(levels)))


def build_pyramid(image, depth, mask, levels, pyramid, depth_min=0.0, depth_max=1e6, stream=None):
    """One call of gsr_odometry_pyramid. image float32 [3, H, W]; depth None or float32 [H, W]; mask None or uint8 / bool [H, W] (0 =
    exclude); pyramid uint8 [>= pyramid_size(W, H, levels)]. The library checks the ranges and raises RuntimeError with its text."""
    _C._require_device(image, "image")
    if image.dim() != 3 or image.shape[0] != 3:
        raise RuntimeError(f"image must be [3, H, W], got {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    args = [_C.dev_ptr(image, "image", _C.F32, (3, H, W)), _C.dev_ptr(depth, "depth", _C.F32, (H, W)),
            _C.dev_ptr(mask, "mask", (torch.uint8, torch.bool), (H, W))]
    pyramid = _C.workspace(pyramid, 0, image.device, "pyramid")
    with torch.cuda.device(image.device):
        _C.load_library().gsr_odometry_pyramid(W, H, int(levels), *args, float(depth_min), float(depth_max), pyramid.data_ptr() or None,
                                               int(pyramid.numel()), _C.stream_handle(stream, image.device))


def align_pyramids(width, height, levels, K, previous, current, iters, T, stats, T_init=None, trace=None, workspace=None, nu=5.0, sigma_init=0.1,
                   sigma_min=1e-3, min_share=0.3, max_last_step=1e-2, max_translation=0.5, max_rotation=math.radians(20.0), stream=None):
    """One call of gsr_odometry_align (include/visual_odometry.h has the rules). previous, current: pyramid buffers of build_pyramid; K =
    (fx, fy, cx, cy) of level 0; iters: passes per level, finest first; T float32 [4, 4] and stats float64 [8] are written; T_init None or
    float32 [4, 4]; trace None or float64 [sum(iters), 32]; max_rotation in radians. No synchronisation, no host read."""
    W, H, levels = int(width), int(height), int(levels)
    iters = [int(v) for v in iters]
    if len(iters) != levels:
        raise RuntimeError(f"iters must hold one pass count per level ({levels}), got {iters}")
    dev, f32, f64, u8 = previous.device, _C.F32, (torch.float64,), (torch.uint8,)
    args = [_C.dev_ptr(previous, "previous", u8), _C.dev_ptr(current, "current", u8), _C.dev_ptr(T_init, "T_init", f32, (4, 4)),
            (ctypes.c_int * levels)(*iters)]
    outs = [_C.dev_ptr(T, "T", f32, (4, 4)), _C.dev_ptr(stats, "stats", f64, (len(STATS),)),
            _C.dev_ptr(trace, "trace", f64, (sum(iters), TRACE_ROW))]
    lib = _C.load_library()
    need = int(lib.gsr_odometry_pyramid_size(W, H, levels))
    if need and (previous.numel() < need or current.numel() < need):
        raise RuntimeError(f"previous and current must hold {need} bytes (gsr_odometry_pyramid_size), got {previous.numel()} and {current.numel()}")
    workspace = _C.workspace(workspace, int(lib.gsr_odometry_align_workspace_size(W, H, levels)) if workspace is None else 0, dev)
    fx, fy, cx, cy = (float(v) for v in K)
    with torch.cuda.device(dev):
        lib.gsr_odometry_align(W, H, levels, fx, fy, cx, cy, *args, float(nu), float(sigma_init), float(sigma_min), float(min_share),
                               float(max_last_step), float(max_translation), float(max_rotation), *outs, workspace.data_ptr() or None,
                               int(workspace.numel()), _C.stream_handle(stream, dev))


def align_rgbd_workspace_size(width, height, levels):
    return int(_C.load_library().gsr_odometry_align_rgbd_workspace_size(int(width), int(height), int(levels)))


def align_pyramids_rgbd(width, height, levels, K, previous, current, iters, T, stats, T_init=None, trace=None, workspace=None, affine=False,
                        geometric_weight=0.0, edge_ratio=0.05, nu=5.0, sigma_init=0.1, sigma_min=1e-3, sigma_depth_init=0.02, sigma_depth_min=1e-4,
                        min_share=0.3, max_last_step=1e-2, max_translation=0.5, max_rotation=math.radians(20.0), max_gain=0.5, max_offset=0.3,
                        stream=None):
    """One call of gsr_odometry_align_rgbd (include/visual_odometry.h has the rules): align_pyramids with an affine brightness (affine) and
    an inverse-depth term against the depth `current` was built with (geometric_weight > 0). stats float64 [12] (STATS_RGBD) and T are
    written; trace None or float64 [sum(iters), 64]. No synchronisation, no host read."""
    W, H, levels = int(width), int(height), int(levels)
    iters = [int(v) for v in iters]
    if len(iters) != levels:
        raise RuntimeError(f"iters must hold one pass count per level ({levels}), got {iters}")
    dev, f32, f64, u8 = previous.device, _C.F32, (torch.float64,), (torch.uint8,)
    args = [_C.dev_ptr(previous, "previous", u8), _C.dev_ptr(current, "current", u8), _C.dev_ptr(T_init, "T_init", f32, (4, 4)),
            (ctypes.c_int * levels)(*iters)]
    outs = [_C.dev_ptr(T, "T", f32, (4, 4)), _C.dev_ptr(stats, "stats", f64, (len(STATS_RGBD),)),
            _C.dev_ptr(trace, "trace", f64, (sum(iters), TRACE_ROW_RGBD))]
    lib = _C.load_library()
    need = int(lib.gsr_odometry_pyramid_size(W, H, levels))
    if need and (previous.numel() < need or current.numel() < need):
        raise RuntimeError(f"previous and current must hold {need} bytes (gsr_odometry_pyramid_size), got {previous.numel()} and {current.numel()}")
    workspace = _C.workspace(workspace, int(lib.gsr_odometry_align_rgbd_workspace_size(W, H, levels)) if workspace is None else 0, dev)
    fx, fy, cx, cy = (float(v) for v in K)
    with torch.cuda.device(dev):
        lib.gsr_odometry_align_rgbd(W, H, levels, fx, fy, cx, cy, *args, int(bool(affine)), float(geometric_weight), float(edge_ratio), float(nu),
                                    float(sigma_init), float(sigma_min), float(sigma_depth_init), float(sigma_depth_min), float(min_share),
                                    float(max_last_step), float(max_translation), float(max_rotation), float(max_gain), float(max_offset), *outs,
                                    workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, dev))


class DenseOdometry:
    """The alignment of consecutive frames of one size with one set of options (the keys of ``Training.pose_prior``: max_rotation in degrees,
    iters finest first; and those of ``Training.pose_prior_terms``: affine, geometric_weight and what goes with them, all off by default --
    with one of the two on, align() calls gsr_odometry_align_rgbd and its stats are STATS_RGBD; with both off it makes gsr_odometry_align's call).
    It owns two pyramid buffers -- the kept previous frame's and the current frame's, swapped by keep() -- and the workspace.

        odo.keep(image, depth, mask)            # the frame the next one is aligned against
        T, stats = odo.align(next_image)        # [4, 4] float32: previous camera -> current camera; identity where the gate refused
        odo.keep(next_image, next_depth, None)

    Everything stays on the device and on the current stream: no synchronisation and no host copy. The time of every align() is held in
    device events until summary() asks."""

    def __init__(self, width, height, K, levels=3, iters=(5, 7, 10), nu=5.0, sigma_init=0.1, sigma_min=1e-3, min_share=0.3, max_last_step=1e-2,
                 max_translation=0.5, max_rotation=20.0, depth_min=0.0, depth_max=1e6, device="cuda:0", affine=False, geometric_weight=0.0,
                 edge_ratio=0.05, sigma_depth_init=0.02, sigma_depth_min=1e-4, max_gain=0.5, max_offset=0.3):
        self.width, self.height, self.K, self.levels = int(width), int(height), tuple(float(v) for v in K), int(levels)
        self.device = torch.device(device)
        self.iters = [int(v) for v in iters]
        self.depth_range = (float(depth_min), float(depth_max))
        self.params = dict(nu=float(nu), sigma_init=float(sigma_init), sigma_min=float(sigma_min), min_share=float(min_share),
                           max_last_step=float(max_last_step), max_translation=float(max_translation),
                           max_rotation=math.radians(float(max_rotation)))
        need = pyramid_size(self.width, self.height, self.levels)
        if need == 0:
            raise ValueError(f"a {width} x {height} frame with {self.levels} levels is outside what gsr_odometry_pyramid takes (1 to 6 levels, "
                             "the coarsest at least 8 x 8, width * height below 2^31)")
        self._previous = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._current = torch.empty(need, dtype=torch.uint8, device=self.device)
        # the terms of gsr_odometry_align_rgbd, None while both are off: align() then makes gsr_odometry_align's call
        self.terms = None
        if affine or float(geometric_weight) > 0.0:
            self.terms = dict(affine=bool(affine), geometric_weight=float(geometric_weight), edge_ratio=float(edge_ratio),
                              sigma_depth_init=float(sigma_depth_init), sigma_depth_min=float(sigma_depth_min), max_gain=float(max_gain),
                              max_offset=float(max_offset))
        size = align_workspace_size if self.terms is None else align_rgbd_workspace_size
        self._workspace = torch.empty(size(self.width, self.height, self.levels), dtype=torch.uint8, device=self.device)
        self.has_previous = False
        self.log, self._stats = EventLog(self.device), []

    def keep(self, image, depth=None, mask=None):
        """Build the frame's pyramid (depth None: no pixel can be aligned from it) and make it the previous frame."""
        build_pyramid(*frame_tensors(image, depth, mask, self.device), self.levels, self._current, *self.depth_range)
        self._previous, self._current = self._current, self._previous
        self.has_previous = depth is not None

    def drop(self):
        self.has_previous = False

    def align(self, image, T_init=None, trace=None, depth=None, mask=None):
        """T [4, 4] float32 and stats float64 (STATS; STATS_RGBD with a term on) of `image` against the kept frame, both on the device. depth,
        mask: the current frame's, for the depth term; without a depth every pixel adds its photometric term alone."""
        if not self.has_previous:
            raise RuntimeError("DenseOdometry.align: no previous frame is kept (keep() with a depth comes first)")
        with self.log.timed():
            if depth is None:
                build_pyramid(*frame_tensors(image, None, None, self.device), self.levels, self._current)
            else:
                build_pyramid(*frame_tensors(image, depth, mask, self.device), self.levels, self._current, *self.depth_range)
            T = torch.empty((4, 4), dtype=torch.float32, device=self.device)
            stats = torch.empty(len(STATS if self.terms is None else STATS_RGBD), dtype=torch.float64, device=self.device)
            if T_init is not None:
                T_init = T_init.detach().to(device=self.device, dtype=torch.float32).contiguous()
            if self.terms is None:
                align_pyramids(self.width, self.height, self.levels, self.K, self._previous, self._current, self.iters, T, stats, T_init=T_init,
                               trace=trace, workspace=self._workspace, **self.params)
            else:
                align_pyramids_rgbd(self.width, self.height, self.levels, self.K, self._previous, self._current, self.iters, T, stats,
                                    T_init=T_init, trace=trace, workspace=self._workspace, **self.params, **self.terms)
        self._stats.append(stats)
        return T, stats

    def summary(self):
        """Frames aligned, the share the gate accepted, their mean inlier share, device ms per frame: the one host read, at the end of a run.
        With a term on also the mean |alpha| and |beta| and the share of the aligned pixels that had a depth term."""
        stats = torch.stack(self._stats) if self._stats else None
        accepted, share = stats[:, :2].mean(dim=0).tolist() if self._stats else (0.0, 0.0)
        out = {"frames": len(self._stats), "accepted_share": accepted, "inlier_share": share,
               "device_ms_per_frame": self.log.summary()["ms_per_item"] or 0.0}
        if self.terms is not None:
            gain, offset, terms, pixels = (stats[:, 8].abs().mean(), stats[:, 9].abs().mean(), stats[:, 11].sum(), stats[:, 4].sum()) \
                if self._stats else (0.0, 0.0, 0.0, 0.0)
            out.update(mean_abs_alpha=float(gain), mean_abs_beta=float(offset), depth_term_share=float(terms) / float(pixels) if float(pixels) else 0.0)
        return out
