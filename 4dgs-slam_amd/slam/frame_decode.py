"""Host decoding of one recorded frame (PIL + numpy only, no torch): what slam/recorded.py's read-ahead thread runs. It makes no device
call, so it cannot invalidate a graph capture running on the SLAM loop's thread."""
import time

import numpy as np


class HostFrame:
    __slots__ = ("rgb", "mask", "depth", "decode_ms")

    def __init__(self, rgb, mask, depth, decode_ms):
        self.rgb, self.mask, self.depth, self.decode_ms = rgb, mask, depth, decode_ms

    def __getstate__(self):
        return (self.rgb, self.mask, self.depth, self.decode_ms)

    def __setstate__(self, s):
        self.rgb, self.mask, self.depth, self.decode_ms = s


def _load(path, mode=None):
    from PIL import Image
    with Image.open(path) as im:
        if mode is not None and im.mode != mode:
            im = im.convert(mode)
        return np.array(im)


def decode_frame(color_path, depth_path, mask_path, width, height, depth_scale, depth_float32):
    """Colour HWC uint8, mask L uint8 (or None), depth float32 [H,W]: float32(u16 / scale) divided in float64 (TUM), or
    float32(u16) / float32(scale) (CoFusion, depth_float32). depth_path None (a monocular sequence): depth None."""
    t0 = time.perf_counter()
    rgb = _load(color_path, "RGB")
    mask = None if mask_path is None else _load(mask_path, "L")
    d = None if depth_path is None else _load(depth_path)
    for what, path, a, want in (("colour", color_path, rgb, (height, width, 3)), ("mask", mask_path, mask, (height, width)),
                                ("depth", depth_path, d, (height, width))):
        if a is not None and a.shape != want:
            raise ValueError(f"{path}: {what} image of shape {a.shape}, the calibration says {want}")
    if d is None:
        depth = None
    else:
        depth = (d.astype(np.float32) / np.float32(depth_scale)) if depth_float32 else (d / depth_scale).astype(np.float32)
    return HostFrame(rgb, mask, depth, (time.perf_counter() - t0) * 1e3)


class StereoFrame:
    __slots__ = ("left", "right", "decode_ms")

    def __init__(self, left, right, decode_ms):
        self.left, self.right, self.decode_ms = left, right, decode_ms


def decode_stereo_frame(left_path, right_path, width, height):
    """The left and the right image of a stereo frame as 8-bit grey [H, W] (cv2.imread(path, 0) of the reference's StereoDataset)."""
    t0 = time.perf_counter()
    left, right = _load(left_path, "L"), _load(right_path, "L")
    for path, a in ((left_path, left), (right_path, right)):
        if a.shape != (height, width):
            raise ValueError(f"{path}: grey image of shape {a.shape}, the calibration says {(height, width)}")
    return StereoFrame(left, right, (time.perf_counter() - t0) * 1e3)
