"""Class-agnostic motion masks from optical flow and depth: the checked ctypes binding of include/motion_segmentation.h and
``FlowMotionSegmenter``. gsr_flow_rigid_fit fits the one rigid camera motion that explains most of a frame pair's flow (Tukey-weighted
Gauss-Newton whose cutoff follows the median residual of the same pass, csrc/gs_motion.h); what it cannot explain is a candidate, and
gsr_motion_mask_clean turns the candidates into a few solid regions (opening, 8-connected components, an area filter, a dilation). The
reference has nothing of the kind: its masks come from files or from YOLO classes (slam/segmentation.py), so a Bonn sequence whose mover is
in no COCO class runs as a static scene there. Thresholds are in pixels at the frame's own resolution. Nothing here has been run on real
Bonn / TUM frames or on RAFT's real flow noise: the tests use analytic and synthetic scenes with Gaussian flow noise
(tests/motion_reference.py restates both stages in float64 numpy / scipy). No CPU path."""
import numpy as np
import torch

from diff_gaussian_rasterization import _C

from . import pretrained

TRACE_ROW = 32          # doubles per pass of gsr_flow_rigid_fit's trace: 21 of H, 6 of g, sum w, sum w e^2, pixels with w > 0, median bin, c


_dev, _stream = _C.dev_ptr, _C.stream_handle
_BYTES = (torch.uint8, torch.bool)
_F32 = _C.F32


def _size_refused(what, W, H):
    return ValueError(f"a {W} x {H} frame is outside what {what} takes (positive sizes, width * height below 2^31)")


def flow_rigid_fit(flow_ij, depth_i, intrinsics, flow_ji=None, fit_mask=None, T_init=None, iters=10, scale_multiplier=2.0, c_min=1.0,
                   c_max=16.0, occlusion_px=1.0, residual_px=1.0, candidate=True, trace=False, workspace=None, stream=None):
    """One call of gsr_flow_rigid_fit (include/motion_segmentation.h has the rules). flow_ij, flow_ji: float32 [H, W, 2] in NDC units;
    depth_i float32 [H, W]; intrinsics (fx, fy, cx, cy); fit_mask bool / uint8 [H, W] or None; T_init float32 [4, 4] or None. Returns a dict:
    T float32 [4, 4] (camera i -> camera j), residual float32 [H, W] in pixels (-1 = not usable), stats float64 [4] (final cutoff, usable
    pixels, pixels of the fit set, sum of weights of the last pass), candidate uint8 [H, W] (None with candidate=False) and trace float64
    [iters, 32] (None without trace=True). The library checks the parameter ranges and raises RuntimeError with its text."""
    _C._require_device(flow_ij, "flow_ij")
    if flow_ij.dim() != 3 or flow_ij.shape[2] != 2:
        raise RuntimeError(f"flow_ij must be [H, W, 2], got {tuple(flow_ij.shape)}")
    H, W, dev = int(flow_ij.shape[0]), int(flow_ij.shape[1]), flow_ij.device
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    lib = _C.load_library()
    need = int(lib.gsr_flow_rigid_fit_workspace_size(W, H))
    if need == 0:
        raise _size_refused("gsr_flow_rigid_fit", W, H)
    workspace = _C.workspace(workspace, need, dev)
    out = {"T": torch.empty((4, 4), dtype=torch.float32, device=dev), "residual": torch.empty((H, W), dtype=torch.float32, device=dev),
           "stats": torch.empty(4, dtype=torch.float64, device=dev),
           "candidate": torch.empty((H, W), dtype=torch.uint8, device=dev) if candidate else None,
           "trace": torch.empty((int(iters), TRACE_ROW), dtype=torch.float64, device=dev) if trace and 1 <= int(iters) <= 64 else None}
    args = [_dev(flow_ij, "flow_ij", _F32, (H, W, 2)), _dev(depth_i, "depth_i", _F32, (H, W)), _dev(flow_ji, "flow_ji", _F32, (H, W, 2)),
            _dev(fit_mask, "fit_mask", _BYTES, (H, W)), _dev(T_init, "T_init", _F32, (4, 4))]
    with torch.cuda.device(dev):
        lib.gsr_flow_rigid_fit(W, H, fx, fy, cx, cy, *args, int(iters), float(scale_multiplier), float(c_min), float(c_max), float(occlusion_px),
                               float(residual_px), out["T"].data_ptr(), out["residual"].data_ptr(), out["stats"].data_ptr(),
                               None if out["candidate"] is None else out["candidate"].data_ptr(),
                               None if out["trace"] is None else out["trace"].data_ptr(), workspace.data_ptr(), int(workspace.numel()),
                               _stream(stream, dev))
    return out


def motion_mask_clean(candidate, open_radius=1, grow_radius=2, min_area=64, motion=None, workspace=None, stream=None):
    """One call of gsr_motion_mask_clean. candidate: bool / uint8 [H, W] on the device. Returns (moving uint8 [H, W], labels int32 [H, W],
    counts int32 [4]): labels are -1 or the smallest linear index of the pixel's component; counts are the components found, the components
    kept, the moving pixels before and after the grow. motion: bool / uint8 [H, W] or None, cleared in place where moving is set."""
    _C._require_device(candidate, "candidate")
    if candidate.dim() != 2:
        raise RuntimeError(f"candidate must be [H, W], got {tuple(candidate.shape)}")
    H, W, dev = int(candidate.shape[0]), int(candidate.shape[1]), candidate.device
    lib = _C.load_library()
    need = int(lib.gsr_motion_mask_clean_workspace_size(W, H))
    if need == 0:
        raise _size_refused("gsr_motion_mask_clean", W, H)
    workspace = _C.workspace(workspace, need, dev)
    moving = torch.empty((H, W), dtype=torch.uint8, device=dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        lib.gsr_motion_mask_clean(W, H, _dev(candidate, "candidate", _BYTES, (H, W)), int(open_radius), int(grow_radius), int(min_area),
                                  moving.data_ptr(), labels.data_ptr(), counts.data_ptr(), _dev(motion, "motion", _BYTES, (H, W)),
                                  workspace.data_ptr(), int(workspace.numel()), _stream(stream, dev))
    return moving, labels, counts


class FlowMotionSegmenter:
    """The moving regions of frame i from its flow to a partner frame j, its depth and the intrinsics:

        out = seg.segment(flow_ij, depth_i, (fx, fy, cx, cy), flow_ji=None, motion=None, T_init=None, stream=None)
        out["T"], out["residual"], out["moving"], out["labels"], out["stats"]

    Everything stays on the device; the workspaces are kept per frame size, so the calls of one segmenter belong on one stream. motion
    ([H, W] bool, True = static), when given, keeps the pixels it already marks as moving out of the fit and is AND-ed in place with
    ~moving. gap: how many frames apart a recorded dataset takes the partner frame (slam/recorded.py)."""

    def __init__(self, iters=10, scale_multiplier=2.0, c_min=1.0, c_max=16.0, residual_px=1.0, occlusion_px=1.0, open_radius=1, min_area=64,
                 grow_radius=2, gap=5):
        if int(gap) < 1:
            raise ValueError(f"gap must be at least 1 frame, got {gap}")
        self.fit_params = dict(iters=int(iters), scale_multiplier=float(scale_multiplier), c_min=float(c_min), c_max=float(c_max),
                               residual_px=float(residual_px), occlusion_px=float(occlusion_px))
        self.clean_params = dict(open_radius=int(open_radius), min_area=int(min_area), grow_radius=int(grow_radius))
        self.gap = int(gap)
        self._ws = {}
        self._logs = {}          # device -> (fit log, clean log)
        self._per_frame = []     # (stats [4] float64, counts [4] int32, pixels): read only when the stats are asked for

    def segment(self, flow_ij, depth_i, intrinsics, flow_ji=None, motion=None, T_init=None, stream=None):
        pretrained.refuse_capture("FlowMotionSegmenter.segment", "segment frames before capture")
        _C._require_device(flow_ij, "flow_ij")
        H, W, dev = int(flow_ij.shape[0]), int(flow_ij.shape[1]), flow_ij.device
        lib = _C.load_library()
        need = (int(lib.gsr_flow_rigid_fit_workspace_size(W, H)), int(lib.gsr_motion_mask_clean_workspace_size(W, H)))
        if 0 in need:
            raise _size_refused("FlowMotionSegmenter", W, H)
        ws_fit = pretrained.workspace(self._ws, ("fit", W, H, dev), need[0], dev)
        ws_clean = pretrained.workspace(self._ws, ("clean", W, H, dev), need[1], dev)
        if dev not in self._logs:
            self._logs[dev] = (pretrained.EventLog(dev), pretrained.EventLog(dev))
        fit_log, clean_log = self._logs[dev]
        with fit_log.timed(stream):
            fit = flow_rigid_fit(flow_ij, depth_i, intrinsics, flow_ji=flow_ji, fit_mask=motion, T_init=T_init, workspace=ws_fit, stream=stream,
                                 **self.fit_params)
        with clean_log.timed(stream):
            moving, labels, counts = motion_mask_clean(fit["candidate"], motion=motion, workspace=ws_clean, stream=stream, **self.clean_params)
        self._per_frame.append((fit["stats"], counts, H * W))
        return {"T": fit["T"], "residual": fit["residual"], "moving": moving, "labels": labels, "stats": fit["stats"], "counts": counts}

    @property
    def stats(self):
        """Frames segmented, the device ms per frame of the fit and of the cleaning, the mean share of moving pixels and the mean final
        cutoff in pixels (reads the per-frame device records: synchronises)."""
        fit = [l[0].summary() for l in self._logs.values()]
        clean = [l[1].summary() for l in self._logs.values()]
        frames = sum(t["calls"] for t in fit)
        ms = lambda ts: float(sum(t["ms_per_item"] * t["calls"] for t in ts if t["calls"]) / frames) if frames else None
        share = [float(c[3].item()) / n for _, c, n in self._per_frame]
        cut = [float(s[0].item()) for s, _, _ in self._per_frame]
        return {"frames": frames, "gap": self.gap, **self.fit_params, **self.clean_params, "fit_ms_per_frame": ms(fit),
                "clean_ms_per_frame": ms(clean), "moving_share_mean": float(np.mean(share)) if share else None,
                "cutoff_px_mean": float(np.mean(cut)) if cut else None}
