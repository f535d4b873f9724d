"""Plane-sweep depth of one view from up to four others with known relative poses: the checked ctypes binding of include/multiview_depth.h
(gsr_sweep_depth: census, a cost over 64 inverse-depth hypotheses, eight-path semi-global aggregation, selection and depth on the device,
csrc/gs_sweep.h) and ``PlaneSweep`` with its cached workspaces. The monocular front-end seeds a new keyframe with it from the window's
keyframes (slam/stages.py, ``Training.mono_sweep``); the reference has no counterpart. tests/sweep_reference.py restates the contract in
numpy and the kernels equal that bit for bit. No CPU path.

Limits: census windows are compared fronto-parallel, so strong rotation or forward motion between the views weakens the cost; the depth is
only as good as the poses handed in; nothing here has been run on real images."""
import torch

from diff_gaussian_rasterization import _C

HYPOTHESES = 64
MAX_PARTNERS = 4
GREY_WEIGHTS = (0.299, 0.587, 0.114)            # ITU-R BT.601 luma, as cv2.cvtColor(RGB2GRAY) weighs the channels

_U16 = (torch.int16, getattr(torch, "uint16", torch.int16))


def sweep_workspace_size(width, height, partners):
    return int(_C.load_library().gsr_sweep_workspace_size(int(width), int(height), int(partners)))


def grey_bytes(image):
    """uint8 [..., H, W] from float [..., 3, H, W] in [0, 1]: the BT.601 luma times 255, rounded to nearest and clipped."""
    r, g, b = image.detach().to(torch.float32).unbind(-3)
    y = GREY_WEIGHTS[0] * r + GREY_WEIGHTS[1] * g + GREY_WEIGHTS[2] * b
    return torch.clamp(torch.round(y * 255.0), 0.0, 255.0).to(torch.uint8).contiguous()


def relative_transforms(reference, partners):
    """float32 [J, 12] on the device: per partner the row-major 3 x 4 [R | t] that takes a point of `reference`'s camera frame to the
    partner's. The cameras hold world-to-camera R [3, 3] and T [3] on the device (slam/camera.py); nothing is read by the host."""
    R_r, T_r = reference.R.detach().to(torch.float32), reference.T.detach().to(torch.float32)
    rows = []
    for cam in partners:
        R = cam.R.detach().to(torch.float32) @ R_r.T
        t = cam.T.detach().to(torch.float32) - R @ T_r
        rows.append(torch.cat([R, t[:, None]], dim=1).reshape(12))
    return torch.stack(rows).contiguous()


def sweep_depth(ref_grey, partner_grey, K, transforms, w_min, w_step, index16, depth, cost=None, cost_sum=None, p1=10, p2=120,
                uniqueness_ratio=40, min_span_px=8, workspace=None, stream=None):
    """One call of gsr_sweep_depth (include/multiview_depth.h has the rules). ref_grey uint8 [H, W]; partner_grey uint8 [J, H, W]; K =
    (fx, fy, cx, cy); transforms float32 [J, 12]; index16 int16 [H, W]; depth float32 [H, W]; cost None or uint8 [H, W, 64]; cost_sum None
    or 16-bit integers [H, W, 64]; workspace None (allocated here) or uint8 [>= sweep_workspace_size(W, H, J)]. stream: a torch stream
    (default: the current stream of ref_grey's device). The library checks the parameter ranges and raises RuntimeError with its text."""
    _C._require_device(ref_grey, "ref_grey")
    if ref_grey.dim() != 2:
        raise RuntimeError(f"ref_grey must be [H, W], got {tuple(ref_grey.shape)}")
    if partner_grey is None or partner_grey.dim() != 3:
        raise RuntimeError(f"partner_grey must be [J, H, W], got {None if partner_grey is None else tuple(partner_grey.shape)}")
    H, W, J = int(ref_grey.shape[0]), int(ref_grey.shape[1]), int(partner_grey.shape[0])
    u8, f32, _dev = (torch.uint8,), _C.F32, _C.dev_ptr
    args = [_dev(ref_grey, "ref_grey", u8, (H, W)), _dev(partner_grey, "partner_grey", u8, (J, H, W)), _dev(transforms, "transforms", f32, (J, 12)),
            _dev(index16, "index16", (torch.int16,), (H, W)), _dev(depth, "depth", f32, (H, W)), _dev(cost, "cost", u8, (H, W, HYPOTHESES)),
            _dev(cost_sum, "cost_sum", _U16, (H, W, HYPOTHESES))]
    fx, fy, cx, cy = (float(v) for v in K)
    lib = _C.load_library()
    # a size the library refuses asks for 0 bytes, and the byte count of a given workspace is left to the library as well: the call below
    # raises with the library's text, which names the size query
    workspace = _C.workspace(workspace, int(lib.gsr_sweep_workspace_size(W, H, J)) if workspace is None else 0, ref_grey.device)
    with torch.cuda.device(ref_grey.device):
        lib.gsr_sweep_depth(W, H, J, fx, fy, cx, cy, float(w_min), float(w_step), int(p1), int(p2), int(uniqueness_ratio), int(min_span_px),
                            *args, workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, ref_grey.device))


class PlaneSweep:
    """The sweep with one set of parameters; the workspace of every (width, height, partners) it has met is kept between calls.

        out = sweeper.sweep(ref_image, partner_images, K, transforms, w_min, w_step)      # {"depth", "index16", "valid"}

    ref_image float [3, H, W] in [0, 1]; partner_images float [J, 3, H, W] or a list of [3, H, W]; K = (fx, fy, cx, cy); transforms float32
    [J, 12] (relative_transforms). depth float32 [H, W] (0 where invalid), index16 int16 [H, W] (16 x the hypothesis, -16 where invalid),
    valid bool [H, W]. The outputs are new tensors on the stream the call ran on (``stream=``, default the current one); a workspace is
    reused, so calls of one object belong on one stream."""

    grey_bytes = staticmethod(grey_bytes)                              # float frames -> the bytes the sweep matches
    relative_transforms = staticmethod(relative_transforms)            # cameras -> the [J, 12] rows it projects with

    def __init__(self, p1=10, p2=120, uniqueness_ratio=40, min_span_px=8, device="cuda:0"):
        self.device = torch.device(device)
        self.params = dict(p1=int(p1), p2=int(p2), uniqueness_ratio=int(uniqueness_ratio), min_span_px=int(min_span_px))
        self._workspaces = {}

    def workspace(self, width, height, partners):
        key = (int(width), int(height), int(partners))
        if key not in self._workspaces:
            need = sweep_workspace_size(*key)
            if need == 0:
                raise ValueError(f"a {width} x {height} view with {partners} partners is outside what gsr_sweep_depth takes (positive sizes, "
                                 "1 to 4 partners, width * height * 64 below 2^31)")
            self._workspaces[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._workspaces[key]

    def sweep_grey(self, ref_grey, partner_grey, K, transforms, w_min, w_step, stream=None, cost=None, cost_sum=None):
        """sweep() on grey bytes: ref_grey uint8 [H, W], partner_grey uint8 [J, H, W]."""
        H, W = int(ref_grey.shape[-2]), int(ref_grey.shape[-1])
        index16 = torch.empty((H, W), dtype=torch.int16, device=self.device)
        depth = torch.empty((H, W), dtype=torch.float32, device=self.device)
        sweep_depth(ref_grey, partner_grey, K, transforms, w_min, w_step, index16, depth, cost=cost, cost_sum=cost_sum,
                    workspace=self.workspace(W, H, int(partner_grey.shape[0])), stream=stream, **self.params)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            return {"depth": depth, "index16": index16, "valid": index16 >= 0}

    def sweep(self, ref_image, partner_images, K, transforms, w_min, w_step, stream=None):
        if not torch.is_tensor(partner_images):
            partner_images = torch.stack([p.to(self.device) for p in partner_images])
        return self.sweep_grey(grey_bytes(ref_image.to(self.device)), grey_bytes(partner_images.to(self.device)), K,
                               transforms.to(device=self.device, dtype=torch.float32).contiguous(), w_min, w_step, stream=stream)
