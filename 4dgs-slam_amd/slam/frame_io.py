"""ctypes binding of include/frame_io.h (gsr_frame_prepare, gsr_frame_export) on libgs_rasterizer_hip.so. No CPU path."""
import functools

import numpy as np
import torch

from diff_gaussian_rasterization import _C


_U8, _F32 = (torch.uint8,), _C.F32


def frame_prepare(rgb, map_xy, lut, mask_l, mask_threshold, image, motion, stream=None):
    """One launch: image [3,H,W] = lut[remap(rgb)] (map_xy None = no undistortion), motion [H,W] = !(mask_l / 255 > threshold) (all
    True without mask_l). rgb uint8 [H,W,3]; map_xy float32 [H,W,2] or None; lut float32 [256]; mask_l uint8 [H,W] or None; motion
    bool / uint8 [H,W] or None. stream: a torch stream (default: the current stream of rgb's device)."""
    if rgb.dim() != 3 or rgb.shape[2] != 3:
        raise RuntimeError(f"rgb must be [H, W, 3], got {tuple(rgb.shape)}")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    dev = _C.dev_ptr
    args = (dev(rgb, "rgb", _U8, (H, W, 3)), dev(map_xy, "map_xy", _F32, (H, W, 2)), dev(lut, "lut", _F32, (256,)),
            dev(mask_l, "mask_l", _U8, (H, W)), float(mask_threshold), dev(image, "image", _F32, (3, H, W)),
            dev(motion, "motion", (torch.uint8, torch.bool), (H, W)))
    _C.load_library().gsr_frame_prepare(W, H, *args, _C.stream_handle(stream, rgb.device))


# matplotlib's "jet" as data: (x, y) knots of its three piecewise-linear segments (_cm.py _jet_data; y0 == y1 at every knot)
JET_SEGMENTS = {"red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
                "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
                "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0))}


@functools.lru_cache(maxsize=None)
def jet_lut():
    """The 256 x 3 bytes of matplotlib.colormaps["jet"](i, bytes=True): LinearSegmentedColormap's table (colors._create_lookup_table, N = 256,
    gamma 1, float64) and its byte conversion (lut * 255 truncated). Read-only."""
    lut = np.empty((256, 3), np.float64)
    xind = 255 * np.linspace(0, 1, 256)
    for c, name in enumerate(("red", "green", "blue")):
        knots = np.array(JET_SEGMENTS[name], np.float64)
        x, y = knots[:, 0] * 255, knots[:, 1]
        ind = np.searchsorted(x, xind)[1:-1]
        distance = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, c] = np.clip(np.concatenate([[y[0]], distance * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]]), 0.0, 1.0)
    out = (lut * 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def _views(t, name, channels, V, H, W):
    """Address and view stride (in floats) of a float32 device batch [V, channels, H, W] whose views are each contiguous."""
    _C._require_device(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != (V, channels, H, W) or tuple(t.stride()[1:]) != (H * W, W, 1) or (V > 1 and t.stride(0) < channels * H * W):
        raise RuntimeError(f"{name} must be a float32 device tensor of shape {(V, channels, H, W)} with contiguous views, got {t.dtype} "
                           f"{tuple(t.shape)} strides {tuple(t.stride())}")
    return t.data_ptr(), int(t.stride(0)) if V > 1 else channels * H * W


def frame_export(colour, depth, lut, depth_vmax, depth_scale, rgb8, depth_rgb8=None, depth_u16=None, stream=None):
    """One launch: V rendered views to file bytes (include/frame_io.h gsr_frame_export). colour float32 [V,3,H,W] and depth float32 [V,1,H,W]
    (each view contiguous, any view stride: the multi-view rasterizer's output block is taken as it is); lut uint8 [256,3] (jet_lut());
    rgb8 / depth_rgb8 uint8 [V,H,W,3]; depth_u16 uint16 (or int16, same bits) [V,H,W]. depth_rgb8 and depth_u16 may each be None, and depth
    may be None when both are. stream: a torch stream (default: the current stream of colour's device)."""
    if colour.dim() != 4 or colour.shape[1] != 3:
        raise RuntimeError(f"colour must be [V, 3, H, W], got {tuple(colour.shape)}")
    V, _, H, W = (int(v) for v in colour.shape)
    if depth is None and (depth_rgb8 is not None or depth_u16 is not None):
        raise RuntimeError("a depth output was asked for without depth")
    c_ptr, c_stride = _views(colour, "colour", 3, V, H, W)
    d_ptr, d_stride = _views(depth, "depth", 1, V, H, W) if depth is not None else (None, 0)
    if depth_u16 is not None and depth_u16.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)):
        raise RuntimeError(f"depth_u16 must be a 16-bit integer tensor, got {depth_u16.dtype}")
    dev = _C.dev_ptr
    args = (c_ptr, c_stride, d_ptr, d_stride, dev(lut, "lut", _U8, (256, 3)), float(depth_vmax), float(depth_scale),
            dev(rgb8, "rgb8", _U8, (V, H, W, 3)), dev(depth_rgb8, "depth_rgb8", _U8, (V, H, W, 3)),
            dev(depth_u16, "depth_u16", (torch.int16, getattr(torch, "uint16", torch.int16)), (V, H, W)))
    with torch.cuda.device(colour.device):
        _C.load_library().gsr_frame_export(V, W, H, *args, _C.stream_handle(stream, colour.device))
