"""Stereo depth at ingestion: the checked ctypes binding of include/stereo_depth.h (gsr_stereo_depth: rectification, census cost, eight-path
semi-global matching, selection and bf / disparity on the device, csrc/gs_stereo.h), ``StereoMatcher`` with its cached workspace, and
``rectify_map``, cv2.initUndistortRectifyMap restated in float64 numpy. This stands where the reference's StereoDataset runs
cv2.StereoSGBM on the host (utils/dataset.py:460-487). The matcher is this project's own (tests/stereo_reference.py restates it in numpy and
the kernels equal that bit for bit); it keeps OpenCV's public semantics -- disparity x 16 as int16, -16 for "no match", uniquenessRatio,
disp12MaxDiff -- so the reference's parameters carry over, but equality with cv2's output is not claimed: the cost is a census transform,
and cv2's blockSize has no counterpart. No CPU path."""
import numpy as np
import torch

from diff_gaussian_rasterization import _C

REFERENCE_BF = 47.90639384423901        # utils/dataset.py:475: baseline * fx of the EuRoC rig, following ORB-SLAM2's configuration


def rectify_map(K_raw, dist, R, K_opt, width, height, dtype=np.float32):
    """cv2.initUndistortRectifyMap(K_raw, dist = (k1, k2, p1, p2, k3), R, K_opt, (width, height), CV_32FC1) in float64, stored as float32
    [H, W, 2] = (map_x, map_y): an output pixel goes through K_opt^-1, then R^T, is normalised, distorted and projected with K_raw.
    recorded.undistort_map is the special case R = I, K_opt = K_raw. dtype=np.float64 keeps the unrounded map (tests)."""
    K_raw, K_opt, R = (np.asarray(a, np.float64).reshape(3, 3) for a in (K_raw, K_opt, R))
    k1, k2, p1, p2, k3 = (float(v) for v in (list(np.asarray(dist, np.float64).reshape(-1)) + [0.0] * 5)[:5])
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    fx, fy, cx, cy = K_opt[0, 0], K_opt[1, 1], K_opt[0, 2], K_opt[1, 2]
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R          # row vector times R = R^T applied to the column
    x, y = ray[..., 0] / ray[..., 2], ray[..., 1] / ray[..., 2]
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    mx = K_raw[0, 0] * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + K_raw[0, 2]
    my = K_raw[1, 1] * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + K_raw[1, 2]
    return np.stack([mx, my], -1).astype(dtype)


def stereo_workspace_size(width, height, num_disparities):
    return int(_C.load_library().gsr_stereo_workspace_size(int(width), int(height), int(num_disparities)))


_U16 =(torch.int16, getattr(torch, "uint16", torch.int16))


def stereo_depth(left, right, disparity16, depth=None, image=None, lut=None, maps=None, left_rect=None, right_rect=None, cost_sum=None,
                 num_disparities=64, p1=10, p2=120, uniqueness_ratio=40, disp12_max_diff=1, bf=REFERENCE_BF, workspace=None, stream=None):
    """One call of gsr_stereo_depth (include/stereo_depth.h has the rules). left, right uint8 [H, W]; disparity16 int16 [H, W]; depth
    float32 [H, W] or None; image float32 [3, H, W] or None (needs lut float32 [256]); maps None or (map_left, map_right) float32 [H, W, 2]
    each, then left_rect / right_rect uint8 [H, W] are required; cost_sum None or 16-bit integers [H, W, D]; workspace None (allocated here)
    or uint8 [>= stereo_workspace_size(W, H, D)]. stream: a torch stream (default: the current stream of left's device). The library
    checks the parameter ranges and raises RuntimeError with its text."""
    _C._require_device(left, "left")
    if left.dim() != 2:
        raise RuntimeError(f"left must be [H, W], got {tuple(left.shape)}")
    H, W, D = int(left.shape[0]), int(left.shape[1]), int(num_disparities)
    map_l, map_r = maps if maps is not None else (None, None)
    u8, f32, _dev = (torch.uint8,), _C.F32, _C.dev_ptr
    args = [_dev(left, "left", u8, (H, W)), _dev(right, "right", u8, (H, W)), _dev(map_l, "map_left", f32, (H, W, 2)),
            _dev(map_r, "map_right", f32, (H, W, 2)), _dev(lut, "lut", f32, (256,)), _dev(left_rect, "left_rect", u8, (H, W)),
            _dev(right_rect, "right_rect", u8, (H, W)), _dev(image, "image", f32, (3, H, W)),
            _dev(disparity16, "disparity16", (torch.int16,), (H, W)), _dev(depth, "depth", f32, (H, W)),
            _dev(cost_sum, "cost_sum", _U16, (H, W, D))]
    lib = _C.load_library()
    # a size the library refuses asks for 0 bytes, and the byte count of a given workspace is left to the library as well: the call below
    # raises with the library's text, which names the size query
    workspace = _C.workspace(workspace, int(lib.gsr_stereo_workspace_size(W, H, D)) if workspace is None else 0, left.device)
    with torch.cuda.device(left.device):
        lib.gsr_stereo_depth(W, H, D, int(p1), int(p2), int(uniqueness_ratio), int(disp12_max_diff), float(bf), *args,
                             workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, left.device))


class StereoMatcher:
    """The matcher for one image size and one set of parameters, with its workspace and byte table kept between calls.

        image, disparity16, depth = matcher(left_u8, right_u8, maps=None)

    left_u8 / right_u8: uint8 [H, W] device tensors; maps: None (a rectified pair) or (map_left, map_right) float32 [H, W, 2] from
    rectify_map. image is the (rectified) left picture as float32 [3, H, W] in [0, 1], grey in all three channels; disparity16 int16
    [H, W], 16 x disparity, -16 without a match; depth float32 [H, W] = bf / disparity, 0 without a match. The outputs are new tensors on
    the stream the call ran on (``stream=``, default the current one); the workspace is reused, so calls of one matcher belong on one stream."""

    def __init__(self, width, height, num_disparities=64, p1=10, p2=120, uniqueness_ratio=40, disp12_max_diff=1, bf=REFERENCE_BF, device="cuda:0"):
        self.width, self.height, self.device = int(width), int(height), torch.device(device)
        self.params = dict(num_disparities=int(num_disparities), p1=int(p1), p2=int(p2), uniqueness_ratio=int(uniqueness_ratio),
                           disp12_max_diff=int(disp12_max_diff), bf=float(bf))
        need = stereo_workspace_size(self.width, self.height, num_disparities)
        if need == 0:
            raise ValueError(f"a {width} x {height} pair with {num_disparities} disparities is outside what gsr_stereo_depth takes "
                             "(positive sizes, 64 or 128 disparities, width * height * disparities below 2^31)")
        self._workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._lut = torch.tensor((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32), device=self.device)
        self._rect = None

    def __call__(self, left_u8, right_u8, maps=None, stream=None, cost_sum=None):
        H, W, dev = self.height, self.width, self.device
        image = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        disparity16 = torch.empty((H, W), dtype=torch.int16, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        if maps is not None and self._rect is None:
            self._rect = torch.empty((2, H, W), dtype=torch.uint8, device=dev)
        rect = self._rect if maps is not None else (None, None)
        stereo_depth(left_u8, right_u8, disparity16, depth=depth, image=image, lut=self._lut, maps=maps, left_rect=rect[0], right_rect=rect[1],
                     cost_sum=cost_sum, workspace=self._workspace, stream=stream, **self.params)
        return image, disparity16, depth
