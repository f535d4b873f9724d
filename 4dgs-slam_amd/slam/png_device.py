"""Lossless PNG compression on the device: the checked ctypes binding of the deflate encoder of include/video_io.h (gsr_png_encode,
csrc/gs_png.h). It turns the two picture kinds frame_io.frame_export writes -- 8-bit RGB [V, H, W, 3] (kind 0) and 16-bit grey [V, H, W]
(kind 1) -- into one complete zlib stream per view, the payload of that view's IDAT chunk; png.assemble(W, H, kind, stream) makes the file.
The host runs no compressor."""
import torch

from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization._abi import GSR_PNG_SEGMENT

from .png import FILTERS

SEGMENT = GSR_PNG_SEGMENT                                           # filtered bytes per independently coded segment
_U16 = (torch.int16, getattr(torch, "uint16", torch.int16))


def png_workspace_size(views, width, height, kind):
    return int(_C.load_library().gsr_png_workspace_size(views, width, height, kind))


def png_stream_bound(width, height, kind):
    """The most bytes one view's stream can take: 2 + n + 10 * ceil(n / SEGMENT) + 9 with n = height * (width * D + 1); 0 outside the range."""
    return int(_C.load_library().gsr_png_stream_bound(width, height, kind))


def png_encode(pixels, out, sizes, filter="up", workspace=None, stream=None):
    """zlib streams of the filtered scanlines of V views, on the device (include/video_io.h gsr_png_encode). pixels uint8 [V, H, W, 3] or a
    16-bit integer tensor [V, H, W] as frame_io.frame_export writes them; out uint8 [V, capacity] with capacity >= png_stream_bound(W, H, kind):
    view v's stream from out[v, 0]; sizes int32 [V]: the bytes written; filter "none" or "up" (png.FILTERS); workspace None (allocated here)
    or uint8 [>= png_workspace_size(V, W, H, kind)]. stream: a torch stream (default: the current stream of pixels' device). A file is
    png.assemble(W, H, kind, out[v, :sizes[v]]). Returns kind."""
    _C._require_device(pixels, "pixels")
    if pixels.dtype == torch.uint8 and pixels.dim() == 4 and pixels.shape[3] == 3:
        kind = 0
    elif pixels.dtype in _U16 and pixels.dim() == 3:
        kind = 1
    else:
        raise RuntimeError(f"pixels must be uint8 [V, H, W, 3] or 16-bit [V, H, W], got {pixels.dtype} {tuple(pixels.shape)}")
    if filter not in FILTERS:
        raise RuntimeError(f"filter must be one of {sorted(FILTERS)}, got {filter!r}")
    V, H, W = (int(v) for v in pixels.shape[:3])
    _C._require_device(out, "out")
    if out.dim() != 2:
        raise RuntimeError(f"out must be [V, capacity], got {tuple(out.shape)}")
    lib = _C.load_library()
    bound, need = int(lib.gsr_png_stream_bound(W, H, kind)), int(lib.gsr_png_workspace_size(V, W, H, kind))
    if bound == 0 or need == 0:
        raise RuntimeError(f"pixels: {V} views of {W} x {H} are outside what gsr_png_encode takes")
    if out.shape[1] < bound:
        raise RuntimeError(f"out must hold png_stream_bound = {bound} bytes per view, got {int(out.shape[1])}")
    _dev = _C.dev_ptr
    args = [_dev(pixels, "pixels", (pixels.dtype,), tuple(pixels.shape)), _dev(out, "out", (torch.uint8,), (V, out.shape[1])), int(out.shape[1]),
            _dev(sizes, "sizes", (torch.int32,), (V,))]
    workspace = _C.workspace(workspace, need, pixels.device)
    with torch.cuda.device(pixels.device):
        lib.gsr_png_encode(V, W, H, kind, FILTERS[filter], *args, workspace.data_ptr(), int(workspace.numel()), _C.stream_handle(stream, pixels.device))
    return kind
