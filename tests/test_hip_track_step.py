"""gsr_track_step (include/slam_map.h, csrc/gs_capi.hip) -- the tracking iteration as one C call: the loss epilogue of render_fwd
(csrc/gs_render.h, render_fwd_track_kernel), the pose-only backward pass and track_tail_kernel (csrc/gs_map.h) -- called directly through
ctypes on scenes built here, at the frame sizes, Gaussian counts and option values where it can go wrong: partly filled tiles, the second
and third trip of the tail kernel's 64 x 8 loops, every NULL-able operand, opacity weights off, the gather route, both SH widths.

Each case runs the same iteration from the same state through the unfused pieces (gaussian_renderer._render_fused ->
slam_losses.weighted_l1_loss -> backward -> Camera.pose_step) and asserts: outputs, pixel cotangents and the pose gradient bit for bit; the
two exposure gradients and every tile's partial sums against an fp64 sum of the loss's per-pixel terms (tests/fp64_references.py); the camera
step bit for bit on the pose side. The workspace is NaN-filled and the outputs sentinel-filled before every call: a tile or a lane that does
not write shows.

Every case prints the figures it bounds (`track-step ...` lines, visible with -s) before it asserts."""
import ctypes as C
import dataclasses
import functools
import itertools
import math
import types

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)
import fp64_references as ref64
from util import make_camera, make_gaussians, keyframe_pose

pytestmark = pytest.mark.gpu

LRS = (0.003, 0.001, 0.01)                 # cam_rot_delta, cam_trans_delta, exposure: the learning rates of the shipped configurations
EXPOSURE = (0.03, -0.01)                   # a non-trivial pair, so that exp(a) and b matter
SENT_F, SENT_I = -12345.0, -99             # no rendered colour / depth / opacity is negative, no radius or count either
U = 2.0 ** -24                             # unit roundoff of fp32
# The per-term constant of the exposure-gradient bounds: rounding of one pixel's term (expf, alpha / (3 N) in fp32, three products) plus
# whatever the UNFUSED route's own two-level sum adds. Measured, not guessed: test_exposure_gradients_and_tile_partials_match_fp64's docstring.
C_TERM = 3


def ws_layout(W, H):
    """The float offsets of gsr_track_step's workspace (include/slam_map.h states the layout; nothing else here does the arithmetic)."""
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    return types.SimpleNamespace(N=N, T=T, gx=(W + 15) // 16, gy=(H + 15) // 16, g_image=slice(0, 3 * N), g_depth=slice(3 * N, 4 * N),
                                 partials=slice(4 * N, 4 * N + 2 * T), tau6=slice(4 * N + 2 * T, 4 * N + 2 * T + 6),
                                 g_exp=slice(4 * N + 2 * T + 6, 4 * N + 2 * T + 8), floats=4 * N + 2 * T + 8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _report(what, case, **figures):
    print("track-step", what, case.id, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


# ---- cases ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    W: int
    H: int
    P: int
    w_rgb: bool = True
    w_depth: bool = True
    exposure: bool = True
    opacity_weights: int = 1
    alpha: float = 0.95
    gather: str = "none"          # "none" | "third" (every third Gaussian; "third256" / "third257": P chosen so that the subset has that length)
    sh: int = 0                   # active_sh_degree 0 with M = 1, or 3 with M = 16
    bg: str = "black"
    latched: bool = False         # latch set and `converged` already 1: the step is a no-op
    scene: str = "random"         # "random" | "behind" (every Gaussian behind the camera, no speculation: R = 0) | "one" (one Gaussian, one pixel)

    @property
    def id(self):
        opts = [f"{self.W}x{self.H}", f"P{self.P}"]
        opts += [n for n, on in (("noWrgb", not self.w_rgb), ("noWdepth", not self.w_depth), ("noExp", not self.exposure),
                                 ("noOpacityW", not self.opacity_weights), ("latched", self.latched)) if on]
        opts += [f"alpha{self.alpha:g}"] if self.alpha != 0.95 else []
        opts += [v for v, on in ((self.gather, self.gather != "none"), (f"sh{self.sh}", self.sh != 0), (self.bg, self.bg != "black"),
                                 (self.scene, self.scene != "random")) if on]
        return "-".join(opts)


# Frame sizes: W, H, Gaussians, exposure pair given. (tiles: what the size reaches)
FRAMES = [(1, 1, 32, True),           # 1: one pixel
          (16, 16, 200, False),       # 1: one full tile
          (17, 16, 200, True),        # 2: a one-column tile
          (37, 23, 600, True),        # 6: ragged right and bottom
          (128, 128, 4000, False),    # 64: exactly one term per lane of the tail kernel
          (200, 70, 3000, True),      # 65: lane 0 gets a second term
          (512, 256, 8000, False),    # 512: exactly one trip of 64 x 8
          (427, 301, 8000, True),     # 513: second trip, ragged on both edges
          (640, 480, 20000, True)]    # 1200: three trips (the workload's frame)
FRAME_CASES = [Case(W, H, P, exposure=e) for W, H, P, e in FRAMES]
# Gaussian counts through the (P + 255) / 256 rows of tau_partials: 1, 1, 1, 2 | 64, 65 | 512, 513 rows
COUNTS = [1, 255, 256, 257, 16384, 16385, 131072, 131073]
COUNT_CASES = [Case(W, H, P) for (W, H) in ((37, 23), (200, 70)) for P in COUNTS]
# Options: a pairwise-covering set (every pair of values of two different options occurs in some row; checked below) plus the two
# configurations the front end runs (static map, and the gather route of a dynamic one).
#          w_rgb, w_depth, exposure, opacity_weights, alpha, gather, sh, bg, latched
OPTION_ROWS = [(1, 1, 1, 0, 1.0, "third256", 0, "grey", 1),
               (0, 0, 0, 1, 0.0, "third257", 3, "black", 0),
               (0, 1, 0, 1, 0.95, "none", 0, "black", 1),
               (0, 0, 1, 0, 0.95, "third", 3, "grey", 1),
               (1, 0, 0, 0, 1.0, "none", 3, "black", 0),
               (1, 1, 1, 0, 0.0, "third", 0, "black", 0),
               (1, 0, 1, 1, 0.95, "third257", 0, "grey", 0),
               (0, 1, 0, 1, 0.0, "third256", 3, "grey", 0),
               (0, 0, 0, 1, 1.0, "third", 3, "grey", 0),
               (0, 1, 1, 0, 1.0, "third257", 3, "black", 1),
               (1, 0, 1, 1, 0.0, "none", 0, "grey", 1),
               (1, 0, 0, 0, 0.95, "third256", 3, "black", 0),
               (1, 1, 1, 1, 0.95, "none", 0, "black", 0),
               (1, 1, 1, 1, 0.95, "third", 0, "black", 0)]
OPTION_NAMES = ("w_rgb", "w_depth", "exposure", "opacity_weights", "alpha", "gather", "sh", "bg", "latched")
OPTION_VALUES = ((1, 0), (1, 0), (1, 0), (1, 0), (0.95, 0.0, 1.0), ("none", "third", "third256", "third257"), (0, 3), ("black", "grey"), (0, 1))
for (_i, _vi), (_j, _vj) in itertools.combinations(enumerate(OPTION_VALUES), 2):
    for _a, _b in itertools.product(_vi, _vj):
        assert any(r[_i] == _a and r[_j] == _b for r in OPTION_ROWS), (OPTION_NAMES[_i], _a, OPTION_NAMES[_j], _b)


def _option_case(W, H, P, row):
    kw = dict(zip(OPTION_NAMES, row))
    P = {"third256": 768, "third257": 769}.get(kw["gather"], P)          # rows 0, 3, ..., 765 and 0, 3, ..., 768
    return Case(W, H, P, w_rgb=bool(kw["w_rgb"]), w_depth=bool(kw["w_depth"]), exposure=bool(kw["exposure"]), opacity_weights=kw["opacity_weights"],
                alpha=kw["alpha"], gather=kw["gather"], sh=kw["sh"], bg=kw["bg"], latched=bool(kw["latched"]))


OPTION_CASES = [_option_case(W, H, P, row) for (W, H, P) in ((37, 23, 600), (427, 301, 8000)) for row in OPTION_ROWS]
# Empty and near-empty renders: the cotangents come from the background alone, so it is not black and the rendered opacity (zero) is no weight
EMPTY_CASES = [Case(37, 23, 600, scene="behind", opacity_weights=0, bg="grey"), Case(37, 23, 1, scene="one", opacity_weights=0, bg="grey")]
TEN_ITERATIONS_CASE = Case(427, 301, 8000)                             # partly tiled, 513 tiles: two trips
CASES = list(dict.fromkeys(FRAME_CASES + COUNT_CASES + OPTION_CASES + EMPTY_CASES))
all_cases = pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)


# ---- scene, cameras, loss operands ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _scene(W, H, P, sh, scene):
    """util.make_gaussians in front of a camera at keyframe_pose(1), as the raw parameter tensors the rasterizer's fused prologue takes.
    Large counts are spread over a wider cone than the frustum, so that about 2 000 stay visible and no tile list grows long; the visible
    ones then sit in every 256-row block of the backward pass."""
    arr = make_camera(W, H)
    spread = max(1.0, math.sqrt(P / max(2000, W * H // 8)))
    g = make_gaussians(P, dataclasses.replace(arr, tanfovx=arr.tanfovx * spread, tanfovy=arr.tanfovy * spread), seed=P, sh_degree=sh)
    xyz_cam = g["means3D"].astype(np.float64)
    scales, opac = g["scales"], np.clip(g["opacities"].reshape(P, 1), 1e-4, 1 - 1e-4)
    if scene == "behind":
        xyz_cam[:, 2] *= -1.0
    elif scene == "one":         # centred on pixel (W // 2, H // 2): pix = f * x / z + c - 0.5. Alone above 1 / 255 there: 0.01 at the centre, 0.01 * exp(-1 / 0.6) beside it
        z = 2.0
        xyz_cam[0] = ((W // 2 + 0.5 - arr.cx) * z / arr.fx, (H // 2 + 0.5 - arr.cy) * z / arr.fy, z)
        scales, opac = np.full((P, 3), 1e-4, np.float32), np.full((P, 1), 0.01)
    elif P < 16:
        xyz_cam[:, :2] *= 0.5    # a handful of Gaussians: well inside the frustum, so that there is a pose gradient
    R, t = keyframe_pose(1)
    xyz = (xyz_cam - t) @ R      # camera = R world + t
    rng = np.random.default_rng(P + 1)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda")
    m = types.SimpleNamespace(_xyz=T(xyz), _scaling=T(np.log(scales)), _rotation=T(g["rotations"] * rng.uniform(0.5, 2.0, size=(P, 1))),
                              _opacity=T(np.log(opac / (1 - opac))), _features_dc=T(g["shs"][:, :1]), _features_rest=T(g["shs"][:, 1:]),
                              active_sh_degree=sh)
    m.get_xyz = m._xyz
    return types.SimpleNamespace(model=m, arr=arr, R=torch.tensor(R, dtype=torch.float32), t=torch.tensor(t, dtype=torch.float32), P=P,
                                 M=int(g["shs"].shape[1]))


CAM_KEYS = ("R", "T", "view", "full", "campos", "adam", "conv", "rot", "trans", "a", "b")


def _cam_state(c):
    t = dict(R=c._R, T=c._T, view=c._view, full=c._full, campos=c._campos, adam=c._adam, conv=c._converged, rot=c.cam_rot_delta,
             trans=c.cam_trans_delta, a=c.exposure_a, b=c.exposure_b)
    return {k: v.detach().cpu().clone() for k, v in t.items()}


def _setup(case, fresh_adam=False):
    """The state both routes start from: two cameras on blank_camera buffers in the same state, the model, and the seeded loss operands."""
    from slam.camera import Camera
    from slam.keyframe_slots import blank_camera
    from diff_gaussian_rasterization import raw as _raw
    W, H = case.W, case.H
    sc = _scene(W, H, case.P, case.sh, case.scene)
    arr = sc.arr
    proto = Camera(0, None, None, torch.eye(4), torch.tensor(arr.projmatrix_raw), arr.fx, arr.fy, arr.cx, arr.cy, 2 * math.atan(arr.tanfovx),
                   2 * math.atan(arr.tanfovy), H, W, 0.0)
    g = torch.Generator().manual_seed(1000 * W + H)
    adam0 = torch.cat([(torch.rand(8, generator=g) - 0.5) * 2e-3, torch.rand(8, generator=g) * 1e-6, torch.tensor([3.0])])
    cams = []
    for uid in (1, 2):
        c = blank_camera(proto, uid, proto.device)
        c.update_RT(sc.R, sc.t)
        c.reset_pose_optimizer()
        with torch.no_grad():
            if not fresh_adam:
                c._adam.copy_(adam0)              # moments and a step count that matter, the same on both sides
            if case.exposure:
                c.exposure_a.fill_(EXPOSURE[0]); c.exposure_b.fill_(EXPOSURE[1])
            if case.latched:
                c._converged.fill_(1)
        cams.append(c)
    cu = lambda t: t.cuda().contiguous()
    ops = types.SimpleNamespace(gt_image=cu(torch.rand(3, H, W, generator=g) * 0.7), gt_depth=cu(0.5 + 5.0 * torch.rand(1, H, W, generator=g)),
                                w_rgb=cu(torch.randint(0, 3, (1, H, W), generator=g).float()) if case.w_rgb else None,
                                w_depth=cu(torch.randint(0, 3, (1, H, W), generator=g).float()) if case.w_depth else None)
    for w in (ops.w_rgb, ops.w_depth):
        if w is not None:
            w.view(-1)[0] = 2.0                   # (the only pixel of the 1 x 1 frame carries weight)
    mask = gather = None
    if case.gather != "none":
        mask = torch.zeros(case.P, dtype=torch.bool, device="cuda")
        mask[::3] = True
        gather = mask._gsr_gather = _raw.gather_from_mask(mask)
        if case.gather != "third":
            assert int(gather.shape[0]) == int(case.gather[5:])
    bg = torch.tensor([0.0, 0.0, 0.0] if case.bg == "black" else [0.2, 0.5, 0.7], device="cuda")
    return types.SimpleNamespace(case=case, scene=sc, fused_cam=cams[0], auto_cam=cams[1], ops=ops, mask=mask, gather=gather, bg=bg, thr=0.95,
                                 means2D=torch.zeros_like(sc.model._xyz), one=torch.ones((), device="cuda"),
                                 alpha32=float(np.float32(case.alpha)), classes=None)


def _exposure_values(case):
    return tuple(float(np.float32(v)) for v in EXPOSURE) if case.exposure else (0.0, 0.0)


def _plant_pixel_classes(st, image, depth, opacity):
    """Build the pixels that stress the loss's per-pixel function into the drawn operands, from the unfused render: a rectangle where the
    target IS the render (residual exactly 0 without the exposure pair), a rectangle of gt_depth = 0, and the opacity threshold set to a
    rendered opacity (pixels above it, below it and exactly on it). Zero weights come with the drawn weights. Then every target whose fp64
    residual is within 1e-5 of zero without being zero moves by 1e-3: the sign of an fp32 residual that small is not determined, and the
    exposure sums are compared with fp64 sums that must not depend on it."""
    case, ops = st.case, st.ops
    H, W = case.H, case.W
    eq = torch.zeros((1, H, W), dtype=torch.bool, device="cuda")
    eq[:, H // 4:H // 2, W // 4:W // 2] = True
    zd = torch.zeros_like(eq)
    zd[:, H // 2:(3 * H) // 4, W // 2:(3 * W) // 4] = True
    ops.gt_image = torch.where(eq, image.detach(), ops.gt_image).contiguous()
    ops.gt_depth = torch.where(eq, depth.detach(), ops.gt_depth)
    ops.gt_depth = torch.where(zd, torch.zeros_like(ops.gt_depth), ops.gt_depth).contiguous()
    u = torch.unique(opacity.detach())
    at = torch.zeros_like(eq)
    if case.opacity_weights and int(u.numel()) >= 3:              # (fewer distinct opacities: a handful of Gaussians; the production 0.95 stays)
        st.thr = float(u[int(u.numel()) // 2])
        at = opacity.detach() == st.thr
    st.classes = types.SimpleNamespace(eq=eq.cpu(), zero_depth=zd.cpu(), at_thr=at.cpu())
    a, b = _exposure_values(case)
    r = math.exp(a) * image.detach().double() + b - ops.gt_image.double()
    ops.gt_image = torch.where((r.abs() < 1e-5) & (r != 0), ops.gt_image + 1e-3, ops.gt_image).contiguous()


def _unfused_forward(st):
    import gaussian_renderer
    return gaussian_renderer._render_fused(st.auto_cam, st.scene.model, st.bg, 1.0, st.means2D, None, None, None, st.mask, False)


def _unfused_backward_and_step(st, image, depth, opacity):
    """weighted_l1_loss(compute_value=False) -> backward -> pose_step(latch=True) on the render `image, depth, opacity`; returns the gradients."""
    import slam_losses
    case, ops, c = st.case, st.ops, st.auto_cam
    image.retain_grad(); depth.retain_grad()
    loss = slam_losses.weighted_l1_loss(image, depth, ops.gt_image, ops.gt_depth, ops.w_rgb, ops.w_depth, c.exposure_a if case.exposure else None,
                                        c.exposure_b if case.exposure else None, case.alpha, opacity=opacity if case.opacity_weights else None,
                                        opacity_depth_threshold=st.thr, compute_value=False)
    loss.backward(st.one)
    cpu = lambda t: t.detach().cpu().clone()
    out = types.SimpleNamespace(g_image=cpu(image.grad), g_depth=cpu(depth.grad), g_rot=cpu(c.cam_rot_delta.grad), g_trans=cpu(c.cam_trans_delta.grad),
                                g_a=cpu(c.exposure_a.grad) if case.exposure else None, g_b=cpu(c.exposure_b.grad) if case.exposure else None)
    c.pose_step(*LRS, optimize_exposure=case.exposure, latch=True)
    return out


def track_step(st, cam, loss_fields=None, step_fields=None, P=None, workspace_offset=0):
    """gsr_track_step through ctypes, the way TrackingGraph._fused_iteration calls it, on camera `cam`. loss_fields / step_fields: values
    for fields of gsr_track_loss / gsr_camera_step that replace the case's own (None = a NULL pointer); P: replaces the Gaussian count;
    workspace_offset: bytes added to the workspace address. The whole workspace is NaN and every output holds a sentinel before the call.
    A refused call comes back with rc = None and the binding's message in `error`."""
    from diff_gaussian_rasterization import _C
    from diff_gaussian_rasterization import raw as _raw
    from diff_gaussian_rasterization._abi import gsr_track_loss
    case, ops, m = st.case, st.ops, st.scene.model
    dev, lib = cam.device, _C.load_library()
    H, W = case.H, case.W
    rows = int(m._xyz.shape[0] if st.gather is None else st.gather.shape[0])
    img = torch.full((_C.NUM_CHANNELS + 2, H, W), SENT_F, dtype=torch.float32, device=dev)
    ints = torch.full((2, rows), SENT_I, dtype=torch.int32, device=dev)
    means2D = torch.full_like(m._xyz, SENT_F)
    nbytes = int(lib.gsr_track_workspace_size(W, H))
    ws = torch.full((nbytes // 4 + 4,), float("nan"), dtype=torch.float32, device=dev)
    geom, binning, imgbuf = _C._Arena(dev), _C._Arena(dev), _C._Arena(dev)
    keep = []
    desc = _raw._describe(m._xyz, m._scaling, m._rotation, m._opacity, m._features_dc, m._features_rest if m._features_rest.numel() else None,
                          None, None, None, None, keep, st.gather)
    ptr = lambda t: None if t is None else t.data_ptr()
    loss = gsr_track_loss()
    loss.gt_image, loss.gt_depth, loss.w_rgb, loss.w_depth = ptr(ops.gt_image), ptr(ops.gt_depth), ptr(ops.w_rgb), ptr(ops.w_depth)
    loss.alpha, loss.opacity_depth_threshold, loss.opacity_weights = float(case.alpha), float(st.thr), int(case.opacity_weights)
    for k, v in (loss_fields or {}).items():
        setattr(loss, k, v)
    step = cam._step_desc(None, LRS, True, 1e-4, True)
    if not case.exposure:
        step.exposure_a = step.exposure_b = None
    for k, v in (step_fields or {}).items():
        setattr(step, k, v)
    error = None
    try:
        with torch.cuda.device(dev):
            rc = lib.gsr_track_step(geom.cb, None, binning.cb, None, imgbuf.cb, None, rows if P is None else P, int(m.active_sh_degree), st.scene.M,
                                    st.bg.data_ptr(), W, H, C.byref(desc), 1.0, cam.projection_matrix.data_ptr(), math.tan(cam.FoVx * 0.5),
                                    math.tan(cam.FoVy * 0.5), img[:3].data_ptr(), img[3:4].data_ptr(), img[4:].data_ptr(), ints[0].data_ptr(),
                                    ints[1].data_ptr(), C.byref(loss), C.byref(step), means2D.data_ptr(), ws.data_ptr() + workspace_offset,
                                    _C._stream(dev))
    except RuntimeError as e:          # the binding's one error path: a negative return code, raised with the code and gsr_last_error()'s text
        rc, error = None, str(e)
    torch.cuda.synchronize(dev)
    return types.SimpleNamespace(rc=rc, error=error, color=img[:3].cpu(), depth=img[3:4].cpu(), opacity=img[4:].cpu(), radii=ints[0].cpu(), n_touched=ints[1].cpu(),
                                 means2D=means2D.cpu(), ws=ws[:nbytes // 4].cpu(), ws_all=ws.cpu())


@functools.lru_cache(maxsize=None)
def _run(case):
    """One iteration of both routes from the same state; everything the tests look at, on the host."""
    from diff_gaussian_rasterization import _C
    st = _setup(case)
    speculate = _C.set_option("speculate", 0) if case.scene == "behind" else None        # R = 0 on the route that waits for the count
    try:
        cam0 = _cam_state(st.auto_cam)
        assert all(same_bits(cam0[k], v) for k, v in _cam_state(st.fused_cam).items())
        image, radii, depth, opacity, n_touched = _unfused_forward(st)
        if case.scene == "random" and case.W * case.H >= 256:          # (the only pixel of the 1 x 1 frame stays an ordinary one)
            _plant_pixel_classes(st, image, depth, opacity)
        cpu = lambda t: t.detach().cpu().clone()
        auto = types.SimpleNamespace(color=cpu(image), depth=cpu(depth), opacity=cpu(opacity), radii=cpu(radii), n_touched=cpu(n_touched))
        auto.__dict__.update(_unfused_backward_and_step(st, image, depth, opacity).__dict__)
        auto.cam = _cam_state(st.auto_cam)
        fused = track_step(st, st.fused_cam)
        fused.cam = _cam_state(st.fused_cam)
    finally:
        if speculate is not None:
            _C.set_option("speculate", speculate)
    ops = types.SimpleNamespace(gt_image=st.ops.gt_image.cpu(), gt_depth=st.ops.gt_depth.cpu(), w_rgb=None if st.ops.w_rgb is None else st.ops.w_rgb.cpu(),
                                w_depth=None if st.ops.w_depth is None else st.ops.w_depth.cpu())
    return types.SimpleNamespace(case=case, cam0=cam0, auto=auto, fused=fused, ops=ops, thr=st.thr, alpha32=st.alpha32, classes=st.classes,
                                 gather=None if st.gather is None else st.gather.cpu().long(), L=ws_layout(case.W, case.H))


# ---- 1, 2: outputs and pixel cotangents -----------------------------------------------------------------------------------------------
@all_cases
def test_outputs_and_pixel_cotangents_are_the_unfused_bits(case):
    """Everything is written (no NaN left in the workspace, no sentinel in an output), the forward outputs are the unfused pass's bits, and
    ws[:3N] / ws[3N:4N] are image.grad / depth.grad bit for bit ("same function, same bits": gs_device.h l1_bwd_pixel) -- on inputs that
    contain render == target, zero weights, gt_depth = 0 and opacities above, below and exactly on the threshold."""
    r = _run(case)
    f, a, L, H, W = r.fused, r.auto, r.L, case.H, case.W
    assert f.rc >= 0
    assert f.ws.numel() == L.floats and int((~torch.isfinite(f.ws)).sum()) == 0                       # every float of 4N + 2T + 8 was written
    for name in ("color", "depth", "opacity"):
        assert int((getattr(f, name) == SENT_F).sum()) == 0, name
    assert int((f.radii == SENT_I).sum()) == 0 and int((f.n_touched == SENT_I).sum()) == 0
    assert bool(torch.isnan(f.ws_all[L.floats:]).all())                                                # ... and nothing behind it
    rows = torch.arange(case.P) if r.gather is None else r.gather
    untouched = torch.ones(case.P, dtype=torch.bool)
    untouched[rows] = False
    assert int((f.means2D[rows] == SENT_F).sum()) == 0 and bool((f.means2D[untouched] == SENT_F).all())  # the rendered rows, and only they
    for name in ("color", "depth", "opacity"):
        assert same_bits(getattr(f, name), getattr(a, name)), name
    assert torch.equal(f.radii, a.radii) and torch.equal(f.n_touched, a.n_touched)
    g_image, g_depth = f.ws[L.g_image].view(3, H, W), f.ws[L.g_depth].view(1, H, W)
    _report("cotangents", case, image_mismatches=int((g_image.view(torch.int32) != a.g_image.view(torch.int32)).sum()),
            depth_mismatches=int((g_depth.view(torch.int32) != a.g_depth.view(torch.int32)).sum()), thr=r.thr, visible=int((f.radii > 0).sum()))
    assert same_bits(g_image, a.g_image) and same_bits(g_depth, a.g_depth)
    if case.scene == "behind":
        assert int((f.radii > 0).sum()) == 0 and bool((f.opacity == 0).all())                          # the background alone ...
        assert bool((g_image != 0).any()) and bool((g_depth != 0).any())                               # ... and cotangents all the same
    if case.scene == "one":
        assert int((f.opacity > 0).sum()) == 1
    if r.classes is None:
        return
    # the classes are there, and the fused cotangents are what the loss defines for them
    k = r.classes
    assert int(k.eq.sum()) > 0 and int(k.zero_depth.sum()) > 0
    assert bool((r.ops.gt_depth[k.zero_depth] == 0).all()) and bool((g_depth[k.eq] == 0).all())       # depth == gt_depth there: sign 0
    if not case.exposure:
        assert same_bits(r.ops.gt_image[k.eq.expand(3, H, W)], a.color[k.eq.expand(3, H, W)])
        assert bool((g_image[k.eq.expand(3, H, W)] == 0).all())                                       # residual exactly 0: sign 0
    if case.w_rgb:
        assert int((r.ops.w_rgb == 0).sum()) > 0 and bool((g_image[(r.ops.w_rgb == 0).expand(3, H, W)] == 0).all())
    if case.w_depth:
        assert int((r.ops.w_depth == 0).sum()) > 0 and bool((g_depth[r.ops.w_depth == 0] == 0).all())
    # (a scene of a handful of Gaussians may render fewer than three distinct opacities: the threshold then stays 0.95)
    assert int(k.at_thr.sum()) > 0 or not case.opacity_weights or case.P < 200
    if case.opacity_weights and int(k.at_thr.sum()) > 0:
        assert int((a.opacity > r.thr).sum()) > 0 and int((a.opacity < r.thr).sum()) > 0
        assert bool((g_depth[a.opacity <= r.thr] == 0).all())                                          # the comparison is strict
        live = (a.opacity > r.thr) & (a.depth != r.ops.gt_depth) & ((r.ops.w_depth > 0) if case.w_depth else torch.ones_like(k.eq))
        if case.alpha != 1.0:
            assert int(live.sum()) > 0 and bool((g_depth[live] != 0).all())


# ---- 3: the pose gradient ---------------------------------------------------------------------------------------------------------------
@all_cases
def test_pose_gradient_is_the_unfused_bits(case):
    """tau6 = [rho | theta]: track_tail_kernel claims tau_sum_body's order, so tau6[3:] is cam_rot_delta.grad and tau6[:3] is
    cam_trans_delta.grad bit for bit -- past one trip of its 64 x 8 loop too (131 072 / 131 073 Gaussians: 512 / 513 rows)."""
    r = _run(case)
    tau = r.fused.ws[r.L.tau6]
    _report("tau", case, rows=(int(r.fused.radii.numel()) + 255) // 256, fused=[float(v) for v in tau],
            unfused=[float(v) for v in torch.cat([r.auto.g_trans.view(-1), r.auto.g_rot.view(-1)])])
    assert same_bits(tau[3:], r.auto.g_rot.view(-1)) and same_bits(tau[:3], r.auto.g_trans.view(-1))
    if case.scene == "behind":
        assert bool((tau == 0).all())
    elif case.scene == "random":
        assert float(r.auto.g_rot.abs().max()) > 0 and float(r.auto.g_trans.abs().max()) > 0


# ---- 4, 5: exposure gradients and the tiles' partial sums ---------------------------------------------------------------------------------
def _exposure_terms(r):
    case, a = r.case, r.auto
    ea, eb = _exposure_values(case)
    ta, tb, _ = ref64.weighted_l1_exposure_terms64(a.color, r.ops.gt_image, r.ops.w_rgb, ea, eb, r.alpha32, opacity=a.opacity if case.opacity_weights else None)
    return ta, tb


def _in_units(err, scale):
    """err / (2^-24 scale); a zero scale asks for a zero error."""
    return err / (U * scale) if scale > 0 else (0.0 if err == 0 else math.inf)


def _tile_sums(t, L):
    """[3, H, W] -> [T]: the sum over each 16 x 16 tile, tile = tile_y * gx + tile_x."""
    _, H, W = t.shape
    p = torch.nn.functional.pad(t, (0, L.gx * 16 - W, 0, L.gy * 16 - H))
    return p.view(3, L.gy, 16, L.gx, 16).sum(dim=(0, 2, 4)).reshape(-1)


@all_cases
def test_exposure_gradients_and_tile_partials_match_fp64(case):
    """g_exp[k] against the fp64 sum of the loss's per-pixel terms (fp64_references.weighted_l1_exposure_terms64, evaluated on the unfused
    fp32 render and the case's operands):  |g_exp[k] - sum term64| <= (d + c) 2^-24 sum |term64|.

    d, the additions on the longest chain of the fused sum: 2 (a pixel's three channels) + 6 (butterfly over the wave's 64 pixels) + 2 (the
    four waves, pairwise)  = 8 per tile; then ceil(T / 64) (lane 0 of the tail kernel adds that many tiles, one after the other) + 6 (final
    butterfly). T = 1200: 8 + 19 + 6 = 33. A tile's partial sum alone: (8 + c) 2^-24 sum_tile |term64|; a tile without a pixel of non-zero
    weight holds exactly 0.
    c covers a term's own rounding (expf, alpha / (3 N), the products). It is twice the largest error of the UNFUSED route against the same
    fp64 sums, in units of 2^-24 sum |term64|, rounded up -- and the unfused route is held to the same bound here, so that c cannot hide a
    defect of the fused route alone. Nothing in the bound comes from the fused route's output.
    Measured on the MI355X over all cases of this module, in units of 2^-24 sum |term64|: the unfused route is off by at most 1.34 (d/da,
    one Gaussian on one pixel) and 0.83 (d/db), so c = ceil(2 * 1.34) = 3; the fused route by at most 1.35 (d/da) and 0.90 (d/db) against
    bounds of 18 to 36, a tile's partial sum by at most 3.04 against 11.
    Without the exposure pair g_exp is formed all the same (exp(a) = 1, b = 0) and checked; the unfused route then has no such gradient."""
    r = _run(case)
    L, f = r.L, r.fused
    ta, tb = _exposure_terms(r)
    d = 8 + -(-L.T // 64) + 6
    g_exp, partials = f.ws[L.g_exp].double(), f.ws[L.partials].double().view(L.T, 2)
    fig = {}
    for k, (t, name) in enumerate(((ta, "a"), (tb, "b"))):
        want, scale = float(t.sum()), float(t.abs().sum())
        fig[f"fused_{name}"] = _in_units(abs(float(g_exp[k]) - want), scale)
        if case.exposure:
            got = float((r.auto.g_a, r.auto.g_b)[k].double())
            fig[f"unfused_{name}"] = _in_units(abs(got - want), scale)
        tiles, tile_scale = _tile_sums(t, L), _tile_sums(t.abs(), L)
        err = (partials[:, k] - tiles).abs()
        live = tile_scale > 0
        fig[f"tiles_{name}"] = float((err[live] / (U * tile_scale[live])).max()) if bool(live.any()) else 0.0
        fig[f"dead_tiles_{name}"] = float(partials[~live, k].abs().max()) if bool((~live).any()) else 0.0
    _report("exposure", case, T=L.T, d=d, c=C_TERM, **fig)
    for name in ("a", "b"):
        assert fig[f"fused_{name}"] <= d + C_TERM
        if case.exposure:
            assert fig[f"unfused_{name}"] <= d + C_TERM
        assert fig[f"tiles_{name}"] <= 8 + C_TERM
        assert fig[f"dead_tiles_{name}"] == 0.0
    if case.alpha != 0.0 and case.scene == "random" and case.W * case.H >= 256:
        assert float(ta.abs().sum()) > 0 and float(tb.abs().sum()) > 0


# ---- 6: the camera step ---------------------------------------------------------------------------------------------------------------------
POSE_SIDE = ("R", "T", "view", "full", "campos", "conv", "rot", "trans")


@all_cases
def test_camera_step_equals_the_unfused_step(case):
    """After the call: R, T, the view matrix, full_proj, campos, the Adam state of the pose (moments, step counter), the zeroed deltas and the
    convergence flag are the unfused route's bits. Without the exposure pair nothing differs between the routes, so the whole Adam state and
    the untouched exposure are bit-identical as well; with it, exposure_a / exposure_b and their Adam slots agree to rtol 1e-5 (their
    gradients are sums in another order). A latched, already converged camera is left alone by both."""
    r = _run(case)
    f, a, c0 = r.fused.cam, r.auto.cam, r.cam0
    for k in POSE_SIDE:
        assert same_bits(f[k], a[k]), k
    pose_slots = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12, 13, 16]
    assert same_bits(f["adam"][pose_slots], a["adam"][pose_slots])
    if not case.exposure:
        assert same_bits(f["adam"], a["adam"])
        for k in ("a", "b"):
            assert same_bits(f[k], a[k]) and same_bits(f[k], c0[k])
    else:
        for k in ("a", "b"):
            torch.testing.assert_close(f[k], a[k], rtol=1e-5, atol=1e-8)
        torch.testing.assert_close(f["adam"][[6, 7, 14, 15]], a["adam"][[6, 7, 14, 15]], rtol=1e-5, atol=1e-8)
    if case.latched:
        for k in CAM_KEYS:
            assert same_bits(f[k], c0[k]) and same_bits(a[k], c0[k]), k
        assert int(f["conv"]) == 1
        return
    assert float(f["adam"][16]) == float(c0["adam"][16]) + 1.0                       # one Adam step, also when the pose gradient is zero
    assert bool((f["rot"] == 0).all()) and bool((f["trans"] == 0).all())              # update_pose zeroes the deltas
    assert not same_bits(f["R"], c0["R"]) and not same_bits(f["T"], c0["T"]) and not same_bits(f["full"], c0["full"])
    slots = pose_slots[:-1] + ([6, 7, 14, 15] if case.exposure else [])
    assert bool((f["adam"][slots] != c0["adam"][slots]).all())


# ---- 7: ten iterations ------------------------------------------------------------------------------------------------------------------------
def test_ten_iterations_follow_the_unfused_route():
    """Ten iterations of both routes on a partly tiled frame of 513 tiles: the poses agree to 2e-6 and both Adam counters read 10."""
    case = TEN_ITERATIONS_CASE
    st = _setup(case, fresh_adam=True)
    image, _radii, depth, opacity, _n = _unfused_forward(st)
    _plant_pixel_classes(st, image, depth, opacity)
    R0, T0 = st.auto_cam.R.clone(), st.auto_cam.T.clone()
    _unfused_backward_and_step(st, image, depth, opacity)
    for _ in range(9):
        image, _radii, depth, opacity, _n = _unfused_forward(st)
        _unfused_backward_and_step(st, image, depth, opacity)
    for _ in range(10):
        out = track_step(st, st.fused_cam)
        assert out.rc >= 0 and int((~torch.isfinite(out.ws)).sum()) == 0
    f, a = st.fused_cam, st.auto_cam
    _report("ten", case, dR=float((f.R - a.R).abs().max()), dT=float((f.T - a.T).abs().max()), moved=float((a.T - T0).abs().max()))
    assert float((a.R - R0).abs().max()) > 0 and float((a.T - T0).abs().max()) > 1e-4          # the pose moved
    torch.testing.assert_close(f.R, a.R, rtol=0, atol=2e-6)
    torch.testing.assert_close(f.T, a.T, rtol=0, atol=2e-6)
    assert float(f._adam[16]) == 10.0 == float(a._adam[16])
    torch.testing.assert_close(f.exposure_a.detach(), a.exposure_a.detach(), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(f.exposure_b.detach(), a.exposure_b.detach(), rtol=1e-4, atol=1e-7)


# ---- refusals, workspace size -------------------------------------------------------------------------------------------------------------------
REFUSALS = {"no_gaussians": dict(P=0),
            "misaligned_workspace": dict(workspace_offset=4),
            "exposure_a_alone": dict(step_fields=dict(exposure_b=None)),
            "exposure_b_alone": dict(step_fields=dict(exposure_a=None)),
            "no_gt_depth": dict(loss_fields=dict(gt_depth=None)),
            "no_full_proj": dict(step_fields=dict(full_proj=None)),
            "no_campos": dict(step_fields=dict(campos=None))}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_invalid_arguments_are_refused_before_anything_is_written(name):
    """Each argument gsr_track_step names as invalid: GSR_ERR_INVALID_ARGUMENT (-1; the binding raises with the code), and neither the
    NaN-filled workspace nor an output nor the camera has been touched."""
    st = _setup(Case(37, 23, 600))
    before = _cam_state(st.fused_cam)
    out = track_step(st, st.fused_cam, **REFUSALS[name])
    assert out.rc is None and "gsr_track_step failed (code -1)" in out.error, out.error
    assert bool(torch.isnan(out.ws_all).all())
    assert bool((out.color == SENT_F).all()) and bool((out.depth == SENT_F).all()) and bool((out.opacity == SENT_F).all())
    assert bool((out.radii == SENT_I).all()) and bool((out.n_touched == SENT_I).all()) and bool((out.means2D == SENT_F).all())
    assert all(same_bits(before[k], v) for k, v in _cam_state(st.fused_cam).items())


def test_workspace_size():
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    for W, H in ((0, 5), (5, 0), (-1, 5), (5, -3), (0, 0)):
        assert int(lib.gsr_track_workspace_size(W, H)) == 0
    for W, H, _P, _e in FRAMES:
        assert int(lib.gsr_track_workspace_size(W, H)) == ws_layout(W, H).floats * 4
    assert [ws_layout(W, H).T for W, H, _P, _e in FRAMES] == [1, 1, 2, 6, 64, 65, 512, 513, 1200]
