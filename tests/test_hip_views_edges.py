"""gsr_forward_views / gsr_backward_views (include/gs_rasterizer.h, csrc/gs_views.h, the host code in csrc/gs_capi.hip,
diff_gaussian_rasterization/views.py) at the sizes, view counts and option values where the batched path has logic of its own: partly
filled tiles and the last batched frame size, the Gaussian counts at which tile_offsets / the eager scatter change variant, one to twelve
views with views that see nothing, tile lists exactly at the bounds of the shared sort capacity, overflow inside a batch (by count and by
list length), the option table (and M = 9, which it leaves out), the delta_mode entry point and the view slot groups.

The reference of every case is V single-view calls on the same inputs (raw.rasterize_gaussians_raw), and everything is compared bit for
bit (torch.equal): per view the five outputs, dL_dmean2D, the delta gradients, theta and rho; the parameter gradients either as the
attached GradBucket after V single-view backward passes in view order, or -- without a bucket -- as the fp32 sum formed HERE, in view order,
of the V per-view gradients (rows a view did not see are zero and 0 + g is exact). The list-length cases additionally hold view 0's
single-view result to the CPU oracle under test_hip_parity's bars, so that the reference itself stays anchored.

Capacity estimates live per host thread and view slot and survive from test to test, so a case calls its scene three times: the first call
may go view by view or overflow on stale estimates, the second and third must be batched (views_batched + 1 each) without overflow
(forward_status_views unchanged), and all three must give the reference's bits. Every option a case changes is restored in a finally.
Cases marshalled through ctypes run with torch.empty poisoned (floats NaN, ints 0x7f7f7f7f): fresh buffers must not help.

Every case prints what it asserts about its route (`views-edges ...` lines, visible with -s)."""
import ctypes as C
import contextlib
import dataclasses
import functools
import itertools
import math
import threading
import types

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)
from util import make_camera, make_gaussians, keyframe_pose, oracle_run, rel_l1
from test_hip_parity import IMG_TOL, GRAD_TOL, _check  # noqa: F401  (the bars of the single-view parity tests; _check applies both)

pytestmark = pytest.mark.gpu

SENT_I = 0x7f7f7f7f
NAN_BITS = 0x7fc00000                      # torch's float("nan") in fp32
PARAMS = ("xyz", "f_dc", "f_rest", "logit", "log_scales", "rot")          # the optimizer's order (mapping_shard.GradBucket, views._param_grads)
AWAY = (np.diag([-1.0, 1.0, -1.0]), np.zeros(3))                          # a camera that looks along -z: every Gaussian is behind it


def _report(what, **figures):
    print("views-edges", what, " ".join(f"{k}={v}" for k, v in figures.items()))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _wide(cam, spread):
    return dataclasses.replace(cam, tanfovx=cam.tanfovx * spread, tanfovy=cam.tanfovy * spread)


def _build(g, poses_Rt, W, H, D=0, iso=False, dyn=False, seed=0, debug=False):
    """Gaussians `g` (util.make_gaussians' layout, activated values) seen from the cameras `poses_Rt` (world -> camera R, t), as the raw
    parameter leaves of the fused prologue, one settings tuple, cotangent pair, delta triple and pose pair per view."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    dev = torch.device("cuda", 0)
    P, M = int(g["means3D"].shape[0]), int(g["shs"].shape[1])
    T = lambda a, rg=False: torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev, requires_grad=rg)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    opac = np.clip(g["opacities"].astype(np.float64).reshape(P, 1), 1e-4, 1 - 1e-4)
    scales = g["scales"][:, :1] if iso else g["scales"]
    par = {"xyz": T(g["means3D"], True), "log_scales": T(np.log(scales.astype(np.float64)), True), "rot": T(g["rotations"] * 1.7, True),
           "logit": T(np.log(opac / (1 - opac)), True), "f_dc": T(g["shs"][:, :1], True), "f_rest": T(g["shs"][:, 1:], True)}
    bg = T([1.0, 1.0, 1.0])
    cams, settings, cots = [], [], []
    for R_w, t_w in poses_Rt:
        cam = make_camera(W, H, R=R_w, t=t_w)
        cams.append(cam)
        settings.append(GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, bg, 1.0, T(cam.viewmatrix), T(cam.projmatrix),
                                                      T(cam.projmatrix_raw), D, T(cam.campos), False, debug))
        cots.append(((torch.randn((3, H, W), generator=gen) / (3 * H * W)).to(dev), (torch.randn((1, H, W), generator=gen) / (H * W)).to(dev)))
    V = len(cams)
    slot = deltas = None
    if dyn:
        dyn_mask = torch.zeros(P, dtype=torch.bool)
        dyn_mask[torch.randperm(P, generator=gen)[: max(1, P // 4)]] = True
        K = int(dyn_mask.sum())
        slot = torch.full((P,), -1, dtype=torch.int32)
        slot[dyn_mask] = torch.arange(K, dtype=torch.int32)
        slot = slot.to(dev)
        deltas = [tuple((torch.randn((K, c), generator=gen) * s).to(dev).requires_grad_(True) for c, s in ((3, 0.01), (3, 0.001), (4, 0.01)))
                  for _ in range(V)]
    poses = [(torch.zeros(3, device=dev, requires_grad=True), torch.zeros(3, device=dev, requires_grad=True)) for _ in range(V)]
    return types.SimpleNamespace(par=par, settings=settings, cots=cots, slot=slot, deltas=deltas, poses=poses, cams=cams, g=g, P=P, V=V, M=M,
                                 W=W, H=H, bg=np.ones(3, np.float32))


def _random_scene(P, V, W, H, D=0, M=None, iso=False, dyn=False, scale_mean=0.02, seed=0, spread=1.0, poses=None, visible=None, debug=False):
    """P random Gaussians in (spread times) the frustum of the camera at the origin, seen from keyframe_pose(2 v) or `poses`.
    visible: rows that stay in front of the cameras; every other Gaussian is moved behind them."""
    cam0 = make_camera(W, H)
    max_deg = {None: D, 1: 0, 4: 1, 9: 2, 16: 3}[M]
    g = make_gaussians(P, _wide(cam0, spread), seed=seed, sh_degree=D, max_sh_degree=max_deg, scale_mean=scale_mean)
    if P < 16:
        g["means3D"][:, :2] *= 0.5              # a handful of Gaussians: well inside the frustum
    if visible is not None:
        hide = np.ones(P, bool)
        hide[visible] = False
        g["means3D"][hide, 2] *= -1.0
    return _build(g, poses or [keyframe_pose(2 * k) for k in range(V)], W, H, D=D, iso=iso, dyn=dyn, seed=seed, debug=debug)


# ---- the two routes ---------------------------------------------------------------------------------------------------------------------
def _leaves(sc):
    return [t for d in (sc.deltas or []) for t in d] + [t for p in sc.poses for t in p]


def _clear(sc):
    for t in list(sc.par.values()) + _leaves(sc):
        t.grad = None


def _plist(sc):
    return [sc.par[k] for k in PARAMS if sc.par[k].numel()]


@contextlib.contextmanager
def _attached_bucket(sc):
    from diff_gaussian_rasterization.autograd import ACCUMULATE_ATTR
    from mapping_shard import GradBucket
    bucket = GradBucket(_plist(sc)).attach()
    try:
        yield bucket
    finally:
        for p in _plist(sc):
            p.grad = None
            setattr(p, ACCUMULATE_ATTR, False)


def _inputs(sc, detached):
    par = {k: t.detach() for k, t in sc.par.items()} if detached else sc.par
    deltas = [tuple(t.detach() for t in d) for d in sc.deltas] if (detached and sc.deltas) else sc.deltas
    return par, deltas


def _grab(sc, outs, m2d, detached, param):
    d = None if (detached or not sc.deltas) else [[t.grad.clone() for t in dv] for dv in sc.deltas]
    return types.SimpleNamespace(img=[tuple(t.detach().clone() for t in o) for o in outs], m2d=[p.grad.clone() for p in m2d], d=d,
                                 pose=[(th.grad.clone(), rh.grad.clone()) for th, rh in sc.poses], param=param)


def _single(sc, mode):
    """V single-view calls. mode "bucket": back-propagated one after the other into the attached bucket (param = the bucket). "returned":
    every view with a fresh .grad; param = the sum of the V per-view gradients formed here, in view order, in fp32 (per_view keeps the
    terms). "detached": the pose-only backward (param = None). Also the single-view num_rendered of every view."""
    from diff_gaussian_rasterization import _C, raw
    par, deltas = _inputs(sc, mode == "detached")
    outs, m2d, per_view, rendered = [], [], [], []
    for v, rs in enumerate(sc.settings):
        if mode == "returned":
            for t in sc.par.values():
                t.grad = None
        pts = torch.zeros((sc.P, 3), device="cuda", requires_grad=True)
        d = deltas[v] if deltas else (None, None, None)
        o = raw.rasterize_gaussians_raw(rs, par["xyz"], pts, par["log_scales"], par["rot"], par["logit"], par["f_dc"],
                                        par["f_rest"] if par["f_rest"].shape[1] else None, sc.slot, d[0], d[1], d[2], sc.poses[v][0], sc.poses[v][1])
        torch.cuda.synchronize()
        rendered.append(_C.forward_status()[1])
        torch.autograd.backward([o[0], o[2]], list(sc.cots[v]))
        outs.append(o)
        m2d.append(pts)
        if mode == "returned":
            per_view.append({k: sc.par[k].grad.clone() for k in PARAMS if sc.par[k].grad is not None})
    param = None
    if mode == "returned":
        param = {k: g.clone() for k, g in per_view[0].items()}
        for term in per_view[1:]:
            for k in param:
                param[k] = param[k] + term[k]                      # one fp32 rounding per view, in view order
    ref = _grab(sc, outs, m2d, mode == "detached", param)
    ref.per_view, ref.rendered = per_view, rendered
    ref.seen = torch.stack([o[1] > 0 for o in outs]).any(0)
    return ref


def _multi(sc, mode):
    from diff_gaussian_rasterization import views
    par, deltas = _inputs(sc, mode == "detached")
    m2d = [torch.zeros((sc.P, 3), device="cuda", requires_grad=True) for _ in sc.settings]
    outs = views.rasterize_views_raw(sc.settings, par["xyz"], m2d, par["log_scales"], par["rot"], par["logit"], par["f_dc"],
                                     par["f_rest"] if par["f_rest"].shape[1] else None, sc.slot, deltas, sc.poses)
    torch.autograd.backward([o[k] for o in outs for k in (0, 2)], [c for cv in sc.cots for c in cv])
    torch.cuda.synchronize()
    param = None if mode != "returned" else {k: sc.par[k].grad.clone() for k in PARAMS if sc.par[k].grad is not None}
    return _grab(sc, outs, m2d, mode == "detached", param)


def _assert_same(got, ref, tag, views_compared=None, params=True):
    for v in (range(len(ref.img)) if views_compared is None else views_compared):
        for k in range(5):
            a, b = got.img[v][k], ref.img[v][k]
            assert a.shape == b.shape and torch.equal(a, b), (tag, "output", v, k, "differing elements", int((a != b).sum()), "largest difference",
                                                              float((a.double() - b.double()).abs().max()))
        assert torch.equal(got.m2d[v], ref.m2d[v]), (tag, "dL_dmean2D", v)
        assert torch.equal(got.pose[v][0], ref.pose[v][0]) and torch.equal(got.pose[v][1], ref.pose[v][1]), (tag, "theta / rho", v)
        assert (got.d is None) == (ref.d is None)
        for a, b in zip(got.d[v] if got.d else (), ref.d[v] if ref.d else ()):
            assert torch.equal(a, b), (tag, "delta gradient", v)
    if not params:
        return
    if isinstance(ref.param, dict):
        assert set(got.param) == set(ref.param), (tag, set(got.param), set(ref.param))
        for k, want in ref.param.items():
            assert torch.equal(got.param[k], want), (tag, "parameter gradient", k, float((got.param[k] - want).abs().max()))
    elif ref.param is not None:
        assert torch.equal(got.param, ref.param), (tag, "bucket", float((got.param - ref.param).abs().max()))


# ---- fresh buffers must not help -------------------------------------------------------------------------------------------------------
def _poisoned_empty(scratch_bytes):
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        if t.is_cuda and t.dtype == torch.float32:
            t.fill_(float("nan"))
        elif t.is_cuda and t.dtype == torch.int32:
            t.fill_(SENT_I)
        elif t.is_cuda and t.dtype == torch.uint8 and int(t.numel()) == scratch_bytes:
            t.fill_(0xFF)                                          # the scratch rows of gsr_backward_views: every float of them a NaN
        return t
    return empty


def _assert_all_written(got, tag):
    for v, o in enumerate(got.img):
        for k in (0, 2, 3):
            assert not bool(torch.isnan(o[k]).any()), (tag, "NaN left in output", v, k)
        assert not bool((o[1] == SENT_I).any()) and not bool((o[4] == SENT_I).any()), (tag, "sentinel left in radii / n_touched", v)
        assert not bool(torch.isnan(got.m2d[v]).any()), (tag, "NaN left in dL_dmean2D", v)
        assert not bool(torch.isnan(got.pose[v][0]).any()) and not bool(torch.isnan(got.pose[v][1]).any()), (tag, "NaN left in the tau row", v)


# ---- one case ----------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _options(**values):
    from diff_gaussian_rasterization import _C
    old = {}
    try:
        for k, v in values.items():
            old[k] = _C.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _C.set_option(k, v)


def _scratch_bytes(sc):
    from diff_gaussian_rasterization import _C
    return int(_C.load_library().gsr_views_scratch_size(sc.V, sc.P, sc.M, int(sc.par["log_scales"].shape[1])))


def _check_case(sc, monkeypatch, tag, mode="bucket", native=True, batched=True, options=None, lazy=False, calls=3):
    """The hygiene of the module's docstring around `calls` multi-view calls of scene sc; mode as in _single. options: set for both routes;
    lazy: the multi-view calls after the first run in lazy mode (a lazy call that overflows on the stale estimates of another test would
    leave its outputs undefined; the reference never runs lazily). Returns the reference."""
    from diff_gaussian_rasterization import _C, views
    marshalling = views._NATIVE_MARSHALLING
    views._NATIVE_MARSHALLING = bool(native)
    ctypes_route = views._glue() is None
    try:
        with contextlib.ExitStack() as stack:
            stack.enter_context(_options(**(options or {})))
            bucket = stack.enter_context(_attached_bucket(sc)) if mode == "bucket" else None
            _clear(sc) if bucket is None else (bucket.zero_grads(), [setattr(t, "grad", None) for t in _leaves(sc)])
            ref = _single(sc, mode)
            if bucket is not None:
                ref.param = bucket.flat.clone()
            for call in range(calls):
                _clear(sc) if bucket is None else (bucket.zero_grads(), [setattr(t, "grad", None) for t in _leaves(sc)])
                b0, o0 = _C.set_option("views_batched"), _C.forward_status_views()
                with contextlib.ExitStack() as inner:
                    if lazy and call > 0:
                        inner.enter_context(_options(lazy=1))
                    if ctypes_route:
                        m = inner.enter_context(monkeypatch.context())
                        m.setattr(torch, "empty", _poisoned_empty(_scratch_bytes(sc)))
                    got = _multi(sc, mode)
                if bucket is not None:
                    got.param = bucket.flat.clone()
                db, do = _C.set_option("views_batched") - b0, _C.forward_status_views() - o0
                _report(tag, call=call, mode=mode, route="ctypes" if ctypes_route else "native", batched=db, overflows=do,
                        rendered=ref.rendered if call == 0 else "")
                if not batched:
                    assert db == 0, (tag, call, "must not batch", db)
                elif call > 0:
                    assert db == 1 and do == 0, (tag, call, "must be batched without overflow", db, do)
                _assert_same(got, ref, (tag, call))
                if ctypes_route:
                    _assert_all_written(got, (tag, call))
                if mode == "returned":
                    for k, g in got.param.items():
                        assert bool((g[~ref.seen] == 0).all()), (tag, call, "rows of Gaussians no view saw must be zeros", k)
            if bucket is not None and ctypes_route:
                # one accumulating call into a NaN-filled bucket: the rows no view saw keep the NaN's bits
                bucket.flat.fill_(float("nan"))
                with monkeypatch.context() as m:
                    m.setattr(torch, "empty", _poisoned_empty(_scratch_bytes(sc)))
                    _multi(sc, mode)
                for p in _plist(sc):
                    rows = p.grad[~ref.seen].contiguous().view(torch.int32)
                    assert bool((rows == NAN_BITS).all()), (tag, "accumulate mode must leave the rows no view saw alone")
    finally:
        views._NATIVE_MARSHALLING = marshalling
    return ref


# ---- 1: frame sizes ----------------------------------------------------------------------------------------------------------------------
FRAMES = [(1, 1, True), (16, 16, True), (17, 16, True), (16, 17, True), (37, 23, True), (427, 301, True), (640, 480, True),
          (2048, 1536, True),          # 12 288 tiles: the last batched size
          (2064, 1536, False)]         # 12 384 tiles: view by view


@pytest.mark.parametrize("W,H,batched", FRAMES, ids=lambda v: str(v))
@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_frame_sizes(W, H, batched, mode, monkeypatch):
    big = W * H > 10 ** 6
    sc = _random_scene(700, 3, W, H, dyn=True, scale_mean=0.005 if big else 0.02, seed=W)
    if big:
        assert ((W + 15) // 16) * ((H + 15) // 16) == {2048: 12288, 2064: 12384}[W]
    _check_case(sc, monkeypatch, f"frame-{W}x{H}", mode=mode, native=False, batched=batched)


# ---- 2: Gaussian counts ------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 1023, 1024, 1025, 262144, 262145, 524288, 524289]     # 1, 1, 1, 2 blocks | tile_offsets' variants (256 / 257 blocks) | eager scatter ends


@pytest.mark.parametrize("P", COUNTS)
@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_gaussian_counts(P, mode, monkeypatch):
    """Large counts are spread over a wider cone than the frustum, so that some 10 000 stay visible (R in the tens of thousands) and the
    visible ones sit in every block."""
    sc = _random_scene(P, 2, 64, 48, dyn=P <= 2048, scale_mean=0.01, seed=P % 1000, spread=max(1.0, math.sqrt(P / 10000)))
    ref = _check_case(sc, monkeypatch, f"count-{P}", mode=mode, native=False)
    assert all(0 < r < 100000 for r in ref.rendered), ref.rendered
    assert (P + 1023) // 1024 == {1: 1, 1023: 1, 1024: 1, 1025: 2, 262144: 256, 262145: 257, 524288: 512, 524289: 513}[P]


@pytest.mark.parametrize("which", ["last", "first"])
@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_only_one_gaussian_of_1025_visible(which, mode, monkeypatch):
    row = 1024 if which == "last" else 0
    sc = _random_scene(1025, 2, 64, 48, scale_mean=0.05, seed=7, visible=[row])
    with torch.no_grad():
        sc.par["xyz"][row] = torch.tensor([0.05, -0.03, 2.0])
    ref = _check_case(sc, monkeypatch, f"one-of-1025-{which}", mode=mode, native=False)
    assert [int(i) for i in ref.seen.nonzero().view(-1)] == [row]
    assert all(r > 0 for r in ref.rendered)


# ---- 3: view counts and empty views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2, 11, 12])
@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_view_counts(V, mode, monkeypatch):
    sc = _random_scene(3000, V, 96, 64, dyn=True, seed=V)
    _check_case(sc, monkeypatch, f"views-{V}", mode=mode, native=False, batched=V > 1)


def test_thirteen_views_are_refused():
    from diff_gaussian_rasterization import _C, views
    from diff_gaussian_rasterization._abi import gsr_view, gsr_alloc_fn
    sc = _random_scene(300, 13, 37, 23)
    assert views.MAX_VIEWS == 12 and not views.views_supported(sc.settings) and views.views_supported(sc.settings[:12])
    m2d = [torch.zeros((sc.P, 3), device="cuda", requires_grad=True) for _ in sc.settings]
    with pytest.raises(RuntimeError, match="the views must share image size, field of view, background, SH degree and scale modifier"):
        views.rasterize_views_raw(sc.settings, sc.par["xyz"], m2d, sc.par["log_scales"], sc.par["rot"], sc.par["logit"], sc.par["f_dc"])
    # the C call: GSR_ERR_INVALID_ARGUMENT before any launch (no allocation is asked for, nothing is counted)
    from diff_gaussian_rasterization import raw
    asked, keep, p = [], [], sc.par
    cb = gsr_alloc_fn(lambda user, nbytes: asked.append(nbytes) or 0)
    desc = raw._describe(p["xyz"], p["log_scales"], p["rot"], p["logit"], p["f_dc"], None, None, None, None, None, keep)
    rs = sc.settings[0]
    before = _C.set_option("views_batched"), _C.debug_view_slots(97)
    with pytest.raises(RuntimeError, match=r"gsr_forward_views failed \(code -1\).*1 <= V <= GSR_MAX_VIEWS"):
        _C.load_library().gsr_forward_views(13, (gsr_view * 13)(), cb, cb, cb, sc.P, 0, 1, rs.bg.data_ptr(), 37, 23, C.byref(desc), 1.0,
                                            float(rs.tanfovx), float(rs.tanfovy), 0, None)
    assert asked == [] and (_C.set_option("views_batched"), _C.debug_view_slots(97)) == before


@pytest.mark.parametrize("away", [(0,), (2,), (3,), (0, 1, 2, 3)], ids=lambda a: "away" + "".join(map(str, a)))
@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_views_that_see_nothing(away, mode, monkeypatch):
    """A camera that faces away from the scene (every radius 0, num_rendered 0) first, in the middle, last, and in all four positions
    (max_R = 0: gsr_backward_views skips render_bwd)."""
    poses = [AWAY if v in away else keyframe_pose(2 * v) for v in range(4)]
    sc = _random_scene(3000, 4, 96, 64, dyn=True, seed=11, poses=poses)
    ref = _check_case(sc, monkeypatch, f"away-{away}", mode=mode, native=False)
    for v in range(4):
        assert (ref.rendered[v] == 0) == (v in away) and (int((ref.img[v][1] > 0).sum()) == 0) == (v in away), (v, ref.rendered)
    if len(away) == 4:
        assert not bool(ref.seen.any())
        assert all(bool((o[0] == 1.0).all()) and bool((o[3] == 0).all()) for o in ref.img)          # the background alone


@pytest.mark.parametrize("mode", ["bucket", "returned"])
def test_gaussians_seen_by_the_first_view_only_the_last_only_and_by_none(mode, monkeypatch):
    poses = [keyframe_pose(-15), keyframe_pose(0), keyframe_pose(15)]          # +- 0.3 rad about y, +- 0.45 along x
    sc = _random_scene(3000, 3, 96, 64, dyn=True, seed=5, spread=2.0, poses=poses)
    ref = _check_case(sc, monkeypatch, "seen-by", mode=mode, native=False)
    vis = [o[1] > 0 for o in ref.img]
    first_only, last_only, none = vis[0] & ~vis[1] & ~vis[2], vis[2] & ~vis[0] & ~vis[1], ~ref.seen
    _report("seen-by", first_only=int(first_only.sum()), last_only=int(last_only.sum()), none=int(none.sum()), all=int((vis[0] & vis[1] & vis[2]).sum()))
    assert int(first_only.sum()) > 0 and int(last_only.sum()) > 0 and int(none.sum()) > 0 and int((vis[0] & vis[1] & vis[2]).sum()) > 0


# ---- 4: exact tile-list lengths -------------------------------------------------------------------------------------------------------------
LENGTHS = [1023, 1024, 1025, 2048, 2049, 4096, 4097, 8193]
SPREAD = 300


def _list_poses(W):
    """16 x 16 (one tile): the cameras of the mapping window. 48 x 32: cameras far enough apart that a stack along one ray of view 1 falls
    into several tiles of the other views."""
    if W == 16:
        return [keyframe_pose(0), keyframe_pose(2), keyframe_pose(4)]
    return [keyframe_pose(0), keyframe_pose(10), keyframe_pose(5)]


def _longest_lists(g, cams):
    out = []
    for cam in cams:
        _, st, _ = oracle_run(g, cam, np.ones(3, np.float32))
        r = st.state()["ranges"].astype(np.int64)
        out.append(int((r[:, 1] - r[:, 0]).max()))
    return out


@functools.lru_cache(maxsize=None)
def _list_gaussians(W, H, L):
    """SPREAD frustum-filling Gaussians plus n small ones of opacity 0.02 stacked along one ray -- the optical axis of view 0 at 16 x 16, the
    ray of view 1 through the middle of tile (0, 0) at 48 x 32 --, n chosen with the CPU oracle such that the longest tile list over the
    views is exactly L. L >= 4097: every seventh of the stack at one depth (ties keep the instance order across the sort's chunks)."""
    poses = _list_poses(W)
    cams = [make_camera(W, H, R=R, t=t) for R, t in poses]
    k = 0 if W == 16 else 1
    cam = cams[k]
    rng = np.random.default_rng(L)
    n_max = L + SPREAD
    z = rng.uniform(1.0, 3.0, n_max)
    if L >= 4097:
        z[::7] = z[3]
    px, py = (cam.cx - 0.5, cam.cy - 0.5) if W == 16 else (7.5, 7.5)
    ray = np.stack([(px + 0.5 - cam.cx) / cam.fx * z, (py + 0.5 - cam.cy) / cam.fy * z, z], 1)
    R_k, t_k = poses[k]
    world = (ray - t_k) @ R_k                                               # camera = R world + t
    spread = make_gaussians(SPREAD, make_camera(W, H), seed=L, scale_mean=0.01)
    q = rng.normal(0, 1, (n_max, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)

    def scene(n):
        stack = dict(means3D=f32(world[:n]), scales=f32(np.full((n, 3), 0.002)), rotations=f32(q[:n]), opacities=f32(np.full((n, 1), 0.02)),
                     shs=f32(rng.uniform(-1, 1, (n_max, 1, 3))[:n]))
        g = {key: np.concatenate([spread[key], stack[key]]) for key in stack}
        g["sh_degree"] = 0
        return g

    n = L - SPREAD // 2
    for _ in range(8):
        g = scene(n)
        lens = _longest_lists(g, cams)
        if max(lens) == L:
            return g, lens
        n += L - max(lens)
    raise AssertionError(("no stack height gives a longest list of", L, lens))


def _raw_gradients_from_oracle(sc, go):
    """The oracle differentiates with respect to the activated values; the chain rule to the raw leaves, in fp64: opacity = sigmoid(logit),
    scale = exp(log_scale), rotation = raw / |raw|."""
    o = 1.0 / (1.0 + np.exp(-sc.par["logit"].detach().cpu().numpy().astype(np.float64)))
    s = np.exp(sc.par["log_scales"].detach().cpu().numpy().astype(np.float64))
    raw = sc.par["rot"].detach().cpu().numpy().astype(np.float64)
    norm = np.linalg.norm(raw, axis=1, keepdims=True)
    qh = raw / norm
    gq = go["dL_drotations"].astype(np.float64).reshape(-1, 4)
    return {"logit": go["dL_dopacity"].astype(np.float64).reshape(-1, 1) * o * (1 - o), "log_scales": go["dL_dscales"].astype(np.float64).reshape(-1, 3) * s,
            "rot": (gq - qh * (qh * gq).sum(1, keepdims=True)) / norm}


def _check_view0_against_oracle(sc, ref):
    """View 0's single-view result (the reference of this module) against util.oracle_run under test_hip_parity's bars."""
    P = sc.P
    act = dict(sc.g)
    act["opacities"] = (1.0 / (1.0 + np.exp(-sc.par["logit"].detach().cpu().numpy().astype(np.float64)))).astype(np.float32)
    cot = [c.cpu().numpy() for c in sc.cots[0]]
    oo, _, go = oracle_run(act, sc.cams[0], sc.bg, cot[0], cot[1])
    n = lambda t: t.detach().cpu().numpy()
    img, pv = ref.img[0], ref.per_view[0]
    m = {"color": rel_l1(n(img[0]), oo["color"]), "depth": rel_l1(n(img[2]), oo["depth"]), "opacity": rel_l1(n(img[3]), oo["opacity"]),
         "radii_mismatch": int((n(img[1]) != oo["radii"]).sum()), "visible_mismatch": int(((n(img[1]) > 0) != (oo["radii"] > 0)).sum()),
         "n_touched_mismatch": int((n(img[4]) != oo["n_touched"]).sum()), "n_touched_gt0_mismatch": int(((n(img[4]) > 0) != (oo["n_touched"] > 0)).sum()), "P": P}
    want = _raw_gradients_from_oracle(sc, go)
    m["g_means3D"] = rel_l1(n(pv["xyz"]).reshape(-1), go["dL_dmeans3D"].reshape(-1))
    m["g_means2D"] = rel_l1(n(ref.m2d[0]).reshape(-1), go["dL_dmeans2D"].reshape(-1))
    m["g_shs"] = rel_l1(n(pv["f_dc"]).reshape(-1), go["dL_dsh"].reshape(-1))
    for k in ("logit", "log_scales", "rot"):
        m["g_" + k] = rel_l1(n(pv[k]).reshape(-1), want[k].reshape(-1))
    tau = go["dL_dtau"].sum(0)
    m["g_rho"], m["g_theta"] = rel_l1(n(ref.pose[0][1]).reshape(-1), tau[:3]), rel_l1(n(ref.pose[0][0]).reshape(-1), tau[3:])
    _report("oracle", **{k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in m.items()})
    _check(m)


@pytest.mark.parametrize("margin", [1000000, 0], ids=["default-margin", "no-margin"])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("W,H", [(16, 16), (48, 32)])
def test_exact_tile_list_lengths(W, H, L, margin, monkeypatch):
    """The shared sort capacity: cap_tile = tile_list_capacity(longest list of ANY view, + cap_tile_margin_permille) picks no sort kernel
    (lists sorted inside render_fwd), <2048, 1024>, <4096, 1024> or the long-list chunk / rank kernels for all views. The per-view longest
    lists are the CPU oracle's; at 48 x 32 they differ and a view other than view 0 holds the longest."""
    g, lens = _list_gaussians(W, H, L)
    sc = _build(g, _list_poses(W), W, H, seed=L)
    _report(f"lists-{W}x{H}-{L}", oracle_longest=lens, P=sc.P, margin=margin)
    assert max(lens) == L
    if W == 48:
        assert len(set(lens)) > 1 and lens[0] < L and max(lens[1:]) == L, lens
    with _options(cap_tile_margin_permille=margin):
        ref = _check_case(sc, monkeypatch, f"lists-{W}x{H}-{L}-{margin}", mode="returned", native=False)
        if margin == 0:
            _check_case(sc, monkeypatch, f"lists-{W}x{H}-{L}-{margin}-bucket", mode="bucket", native=True, calls=2)
    if margin == 0:
        _check_view0_against_oracle(sc, ref)


# ---- 5: overflow inside a batch ------------------------------------------------------------------------------------------------------------
def _overflow_scenes():
    """The priming cameras see the whole scene from slots 0 and 1; the cameras of the test see less than half of it there, and the same as
    the priming ones from slots 2 and 3: with buffers laid out for half of the last count, views 2 and 3 overflow and views 0 and 1 fit."""
    primer = [keyframe_pose(0), keyframe_pose(1), keyframe_pose(4), keyframe_pose(6)]
    test = [keyframe_pose(32), keyframe_pose(-32), keyframe_pose(4), keyframe_pose(6)]
    return (_random_scene(3000, 4, 96, 64, dyn=True, seed=21, poses=primer), _random_scene(3000, 4, 96, 64, dyn=True, seed=21, poses=test))


def _slot_estimates(V, group=0, flow=False):
    from diff_gaussian_rasterization import _C
    s = _C.debug_view_slots(100)
    first = 1 + group * 24 + (12 if flow else 0)
    return [s[first + v] for v in range(V)]


@pytest.mark.parametrize("lazy", [0, 1], ids=["eager", "lazy"])
def test_count_overflow_inside_a_batch(lazy, monkeypatch):
    """cap_test_shrink_permille = 500: a view whose num_rendered exceeds half of its slot's estimate (+ 1) overflows and is redone through
    the single-view path inside the call; the sticky counter rises by exactly the number of such views. Lazy mode does not redo: the
    overflowed views' outputs are undefined and only the others are compared."""
    from diff_gaussian_rasterization import _C
    primer, sc = _overflow_scenes()
    _clear(primer)
    for _ in range(2):
        _multi(primer, "returned")
    _clear(sc)
    ref = _single(sc, "returned")
    try:
        for call in range(2):
            est = [s["estimate_R_alloc"] for s in _slot_estimates(4)]
            over = [v for v in range(4) if ref.rendered[v] > est[v] * 500 // 1000 + 1]
            _clear(sc)
            b0, o0 = _C.set_option("views_batched"), _C.forward_status_views()
            with _options(cap_test_shrink_permille=500, lazy=lazy):
                got = _multi(sc, "returned")
            db, do = _C.set_option("views_batched") - b0, _C.forward_status_views() - o0
            _report("count-overflow", lazy=lazy, call=call, rendered=ref.rendered, estimates=est, overflowed=over, counter=do, batched=db)
            assert db == 1 and (call > 0 or 0 < len(over) < 4)           # first call: some views overflow, some fit. The redo leaves the
            assert do == len(over), (do, over)                            # scene's own counts as estimates: every view overflows in the second
            if lazy:
                _assert_same(got, ref, ("lazy overflow", call), views_compared=[v for v in range(4) if v not in over], params=False)
                break                                  # (lazy calls do not refresh the estimates: a second call would repeat the first)
            _assert_same(got, ref, ("count overflow", call))
    finally:
        _C.set_option("cap_test_shrink_permille", 0)
        _C.set_option("lazy", 0)
    _check_case(sc, monkeypatch, "after-count-overflow", mode="returned", native=False, calls=2)


@functools.lru_cache(maxsize=None)
def _list_overflow_gaussians():
    """Two scenes of the same P at 48 x 32 from cameras 0.4 rad apart: A's longest list is about 300; in B, view 1 (and only view 1) holds a
    list of 1 500 in one tile -- the stack sits outside the other two cameras' frusta."""
    W, H, n_a, n_b = 48, 32, 300, 1500
    poses = [keyframe_pose(0), keyframe_pose(20), keyframe_pose(-20)]
    cams = [make_camera(W, H, R=R, t=t) for R, t in poses]
    cam = cams[1]
    rng = np.random.default_rng(3)
    z = rng.uniform(1.0, 3.0, n_b)
    ray = np.stack([(7.5 + 0.5 - cam.cx) / cam.fx * z, (7.5 + 0.5 - cam.cy) / cam.fy * z, z], 1)
    world = (ray - poses[1][1]) @ poses[1][0]
    spread = make_gaussians(SPREAD, make_camera(W, H), seed=4, scale_mean=0.01)
    q = rng.normal(0, 1, (n_b, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    stack = dict(means3D=f32(world), scales=f32(np.full((n_b, 3), 0.002)), rotations=f32(q), opacities=f32(np.full((n_b, 1), 0.02)),
                 shs=f32(rng.uniform(-1, 1, (n_b, 1, 3))))
    b = {k: np.concatenate([spread[k], stack[k]]) for k in stack}
    a = {k: v.copy() for k, v in b.items()}
    a["means3D"][SPREAD + n_a:] = np.array([0.0, 0.0, -5.0], np.float32)     # behind every camera
    a["sh_degree"] = b["sh_degree"] = 0
    return a, b, poses, _longest_lists(a, cams), _longest_lists(b, cams)


def test_tile_list_overflow_with_room_in_the_instance_count(monkeypatch):
    """A view whose longest list outgrows the shared cap_tile while its instance count still fits (scan_body: mx > cap_tile_list) raises
    FLAG_OVERFLOW and is redone through the single-view path inside the call."""
    from diff_gaussian_rasterization import _C
    a, b, poses, lens_a, lens_b = _list_overflow_gaussians()
    _report("list-overflow", oracle_longest_a=lens_a, oracle_longest_b=lens_b)
    assert max(lens_a) <= 400 and lens_b[1] >= 1400 and lens_b[0] <= 819 and lens_b[2] <= 819      # 819 * 1.25 <= 1024
    sa, sb = _build(a, poses, 48, 32, seed=1), _build(b, poses, 48, 32, seed=1)
    _clear(sa)
    for _ in range(2):
        _multi(sa, "returned")
    slots = _slot_estimates(3)
    assert [s["estimate_longest_tile"] for s in slots] == lens_a                                       # cap_tile = 1024 for the next call
    _clear(sb)
    ref = _single(sb, "returned")
    assert all(r < s["estimate_R_alloc"] + 4096 for r, s in zip(ref.rendered, slots)), (ref.rendered, slots)   # room to spare in the count
    _clear(sb)
    b0, o0 = _C.set_option("views_batched"), _C.forward_status_views()
    got = _multi(sb, "returned")
    db, do = _C.set_option("views_batched") - b0, _C.forward_status_views() - o0
    _report("list-overflow", rendered=ref.rendered, counter=do, batched=db, estimates_after=[s["estimate_longest_tile"] for s in _slot_estimates(3)])
    assert db == 1 and do == 1
    _assert_same(got, ref, "list overflow")
    assert [s["estimate_longest_tile"] for s in _slot_estimates(3)] == lens_b
    for call in range(2):                                                                              # the following calls: batched, no overflow
        _clear(sb)
        b0, o0 = _C.set_option("views_batched"), _C.forward_status_views()
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", _poisoned_empty(_scratch_bytes(sb)))
            got = _multi(sb, "returned")
        assert _C.set_option("views_batched") - b0 == 1 and _C.forward_status_views() == o0, call
        _assert_same(got, ref, ("after the list overflow", call))


# ---- 6: the option table ---------------------------------------------------------------------------------------------------------------------
OPTION_NAMES = ("order_items", "sh_rows", "mailbox", "lazy", "MD", "iso", "dyn", "bucket", "detached", "native")
OPTION_VALUES = ((0, 1), (0, 1), (0, 1), (0, 1), ((1, 0), (4, 1), (16, 3), (16, 1)), (0, 1), (0, 1), (0, 1), (0, 1), (0, 1))
OPTION_ROWS = [(0, 0, 0, 0, (1, 0), 0, 0, 0, 0, 0),
               (1, 1, 1, 1, (1, 0), 1, 1, 1, 1, 1),
               (0, 1, 0, 1, (4, 1), 0, 1, 0, 1, 0),
               (1, 0, 1, 0, (4, 1), 1, 0, 1, 0, 1),
               (0, 0, 1, 1, (16, 3), 0, 0, 1, 1, 0),
               (1, 1, 0, 0, (16, 3), 1, 1, 0, 0, 1),
               (0, 1, 1, 0, (16, 1), 1, 0, 0, 1, 1),
               (1, 0, 0, 1, (16, 1), 0, 1, 1, 0, 0),
               (0, 0, 0, 0, (4, 1), 1, 1, 1, 1, 1),
               (1, 1, 1, 1, (16, 3), 0, 0, 0, 0, 0),
               (0, 1, 0, 1, (1, 0), 1, 0, 1, 0, 0),
               (1, 0, 1, 0, (1, 0), 0, 1, 0, 1, 1),
               (1, 0, 0, 1, (4, 1), 1, 0, 0, 1, 0),
               (0, 1, 1, 0, (16, 3), 0, 1, 1, 0, 1),
               (0, 0, 1, 1, (16, 1), 1, 1, 0, 0, 1),
               (1, 1, 0, 0, (16, 1), 0, 0, 1, 1, 0)]


def _uncovered_pairs(rows):
    missing = []
    for (i, vi), (j, vj) in itertools.combinations(enumerate(OPTION_VALUES), 2):
        for a, b in itertools.product(vi, vj):
            if not any(r[i] == a and r[j] == b for r in rows):
                missing.append((OPTION_NAMES[i], a, OPTION_NAMES[j], b))
    return missing


def test_option_table_covers_all_pairs():
    print("views-edges option table:", OPTION_NAMES)
    for r in OPTION_ROWS:
        print("views-edges option row:  ", r)
    missing = _uncovered_pairs(OPTION_ROWS)
    print("views-edges uncovered pairs:", missing)
    assert len(OPTION_ROWS) <= 16 and missing == []


@pytest.mark.parametrize("row", OPTION_ROWS, ids=lambda r: "-".join(f"{n}{''.join(map(str, v)) if isinstance(v, tuple) else v}" for n, v in zip(OPTION_NAMES, r)))
@pytest.mark.parametrize("W,H", [(37, 23), (427, 301)])
def test_option_table(W, H, row, monkeypatch):
    """(a bucket is not read by the pose-only backward: a row with `detached` compares outputs, dL_dmean2D and the pose gradients, with the
    bucket attached or not)"""
    o = dict(zip(OPTION_NAMES, row))
    M, D = o["MD"]
    sc = _random_scene(2500, 3, W, H, D=D, M=M, iso=bool(o["iso"]), dyn=bool(o["dyn"]), seed=W + sum(row[:4]))
    assert sc.M == M and int(sc.par["log_scales"].shape[1]) == (1 if o["iso"] else 3)
    mode = "detached" if o["detached"] else ("bucket" if o["bucket"] else "returned")
    opts = dict(order_items=o["order_items"], sh_rows=o["sh_rows"], mailbox=o["mailbox"])
    if o["detached"] and o["bucket"]:
        with _attached_bucket(sc) as bucket:
            bucket.zero_grads()
            _check_case(sc, monkeypatch, f"options-{W}x{H}", mode="detached", native=bool(o["native"]), options=opts, lazy=bool(o["lazy"]))
            assert not bool(bucket.flat.any())
    else:
        _check_case(sc, monkeypatch, f"options-{W}x{H}", mode=mode, native=bool(o["native"]), options=opts, lazy=bool(o["lazy"]))


@pytest.mark.parametrize("sh_rows", [0, 1])
@pytest.mark.parametrize("D", [1, 2])
def test_nine_coefficients_per_gaussian(D, sh_rows, monkeypatch):
    """M = 9 is the one value at which preprocess takes the SH row windows (sh_rows, D > 0, M = 9 or 16) that the option table does not reach."""
    sc = _random_scene(2500, 3, 37, 23, D=D, M=9, seed=9 + D)
    assert sc.M == 9
    _check_case(sc, monkeypatch, f"m9-D{D}-sh_rows{sh_rows}", mode="bucket", options=dict(sh_rows=sh_rows))


@pytest.mark.parametrize("how", ["speculate0", "debug"])
@pytest.mark.parametrize("W,H", [(37, 23), (427, 301)])
def test_no_speculation_and_debug_mode_go_view_by_view(W, H, how, monkeypatch):
    sc = _random_scene(2500, 3, W, H, dyn=True, seed=3, debug=how == "debug")
    _check_case(sc, monkeypatch, f"{how}-{W}x{H}", mode="bucket", native=False, batched=False, options=dict(speculate=0) if how == "speculate0" else None)


def test_rasterize_views_net_equals_single_calls_on_the_sums(monkeypatch):
    """delta_mode (views.rasterize_views_net): the deformation network's output [V, P, 10] = (dx | ds | dr) per view is added in front of the
    activations inside the kernels. Per view that is raw.rasterize_gaussians_raw on (xyz + dx, log_scales + ds, rot + dr), what
    render(dynamic=True) calls per camera: outputs and per-view gradients bit for bit, the network output's gradient row by row, and the
    parameter gradients as the view-order sum.

    The delta_mode instantiation of the kernels (<RAW, PRE>) and the plain one are compiled separately; the loaders of gs_device.h hand
    the sums over as values the optimiser cannot look into (pre_value), so that floating-point contraction fuses what follows alike in
    both. Without that the product build differed here in the last bits (colours by up to 2.4e-7, depths by up to 9.5e-7)."""
    from diff_gaussian_rasterization import _C, raw, views
    W, H, V, P = 37, 23, 3, 2500
    sc = _random_scene(P, V, W, H, D=1, M=4, seed=9)
    par = sc.par
    gen = torch.Generator(device="cpu").manual_seed(4)
    net = (torch.randn((V, P, 10), generator=gen) * torch.tensor([0.01] * 3 + [0.05] * 3 + [0.02] * 4)).cuda().requires_grad_(True)
    _clear(sc)
    outs, m2d, per_view = [], [], []
    for v, rs in enumerate(sc.settings):
        for t in par.values():
            t.grad = None
        pts = torch.zeros((P, 3), device="cuda", requires_grad=True)
        o = raw.rasterize_gaussians_raw(rs, par["xyz"] + net[v, :, 0:3], pts, par["log_scales"] + net[v, :, 3:6], par["rot"] + net[v, :, 6:10],
                                        par["logit"], par["f_dc"], par["f_rest"], None, None, None, None, sc.poses[v][0], sc.poses[v][1])
        torch.autograd.backward([o[0], o[2]], list(sc.cots[v]))
        outs.append(o); m2d.append(pts)
        per_view.append({k: par[k].grad.clone() for k in PARAMS})
    param = {k: g.clone() for k, g in per_view[0].items()}
    for term in per_view[1:]:
        for k in param:
            param[k] = param[k] + term[k]
    ref = _grab(sc, outs, m2d, False, param)
    ref_net = net.grad.clone()
    for call in range(3):
        _clear(sc)
        net.grad = None
        b0, o0 = _C.set_option("views_batched"), _C.forward_status_views()
        with monkeypatch.context() as m:
            m.setattr(torch, "empty", _poisoned_empty(_scratch_bytes(sc)))
            pts = [torch.zeros((P, 3), device="cuda", requires_grad=True) for _ in range(V)]
            o = views.rasterize_views_net(sc.settings, par["xyz"], pts, par["log_scales"], par["rot"], par["logit"], par["f_dc"], par["f_rest"], net, sc.poses)
            torch.autograd.backward([x[k] for x in o for k in (0, 2)], [c for cv in sc.cots for c in cv])
            torch.cuda.synchronize()
        got = _grab(sc, o, pts, False, {k: par[k].grad.clone() for k in PARAMS})
        db, do = _C.set_option("views_batched") - b0, _C.forward_status_views() - o0
        _report("net", call=call, batched=db, overflows=do,
                differing=[[int((a != b).sum()) for a, b in zip(x, y)] for x, y in zip(got.img, ref.img)],
                largest=[[f"{float((a.double() - b.double()).abs().max()):.2e}" for a, b in zip(x, y)] for x, y in zip(got.img, ref.img)])
        assert call == 0 or (db == 1 and do == 0)
        _assert_same(got, ref, ("net", call))
        _assert_all_written(got, ("net", call))
        assert torch.equal(net.grad, ref_net), (call, float((net.grad - ref_net).abs().max()))


# ---- 7: view slot groups -----------------------------------------------------------------------------------------------------------------------
def _in_fresh_thread(fn):
    """Capacity estimates, view_slot_group and the views_batched counter are per host thread: a new thread starts without any."""
    box = []

    def run():
        try:
            fn()
        except BaseException as e:          # noqa: BLE001  (re-raised in the test's thread)
            box.append(e)
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if box:
        raise box[0]


def test_view_slot_groups_keep_separate_estimates():
    from diff_gaussian_rasterization import _C, views

    def body():
        V, W, H = 3, 37, 23
        sc = _random_scene(2500, V, W, H, dyn=True, seed=13)
        ref = _single(sc, "returned")
        key = lambda s: (s["estimate_R_alloc"], s["estimate_longest_tile"], s["seq"])
        assert _C.set_option("view_slot_group") == 0 and _C.set_option("views_batched") == 0
        assert all(key(s) == (0, 0, 0) for s in _C.debug_view_slots(97)[1:])
        for call, want in ((0, 0), (1, 1)):                                   # group 0: view by view, then batched
            _clear(sc)
            _assert_same(_multi(sc, "returned"), ref, ("group 0", call))
            assert _C.set_option("views_batched") == want
        group0 = [key(s) for s in _slot_estimates(V, 0)]
        assert all(k[0] > 0 for k in group0) and [s["num_rendered"] for s in _slot_estimates(V, 0)] == ref.rendered
        assert _C.set_option("view_slot_group", 2) == 0
        for call, want in ((0, 1), (1, 2)):                                   # group 2 starts without estimates, whatever group 0 knows
            _clear(sc)
            _assert_same(_multi(sc, "returned"), ref, ("group 2", call))
            assert _C.set_option("views_batched") == want, (call, want)
        assert [key(s) for s in _slot_estimates(V, 0)] == group0              # slots 1 + 0 * 24 + v untouched
        group2 = [key(s) for s in _slot_estimates(V, 2)]                      # slots 1 + 2 * 24 + v
        assert [k[:2] for k in group2] == [k[:2] for k in group0]
        assert all(key(s) == (0, 0, 0) for s in _slot_estimates(12, 1) + _slot_estimates(12, 3) + _slot_estimates(12, 2, flow=True))
        # a flow batch in group 2: slots 1 + 2 * 24 + 12 + v, and the plain slots stay as they are
        K = int((sc.slot >= 0).sum())
        gen = torch.Generator(device="cpu").manual_seed(6)
        zero_bg = torch.zeros(3, device="cuda")
        fs = [rs._replace(bg=zero_bg, sh_degree=0) for rs in sc.settings[:2]]
        dx2 = [(torch.randn((K, 3), generator=gen) * 0.02).cuda().requires_grad_(True) for _ in range(2)]
        flows = [(sc.deltas[v][0], dx2[v], sc.deltas[v][1], sc.deltas[v][2], fs[v].projmatrix, fs[1 - v].projmatrix) for v in range(2)]
        p = sc.par
        for call, want in ((0, 2), (1, 3)):
            pts = [torch.zeros((sc.P, 3), device="cuda", requires_grad=True) for _ in range(2)]
            fo = views.rasterize_flow_views_raw(fs, p["xyz"], pts, p["log_scales"].detach(), p["rot"].detach(), p["logit"].detach(), sc.slot, flows)
            torch.autograd.backward([o[0] for o in fo], [c[0] for c in sc.cots[:2]])
            torch.cuda.synchronize()
            assert _C.set_option("views_batched") == want, (call, want)
        assert all(k[0] > 0 for k in map(key, _slot_estimates(2, 2, flow=True)))
        assert [key(s) for s in _slot_estimates(V, 2)] == group2 and [key(s) for s in _slot_estimates(V, 0)] == group0
        assert all(key(s) == (0, 0, 0) for s in _slot_estimates(12, 0, flow=True) + _slot_estimates(12, 1) + _slot_estimates(12, 3))
        # a value above 3 clamps to 3
        assert _C.set_option("view_slot_group", 7) == 2 and _C.set_option("view_slot_group") == 3
        _clear(sc)
        _assert_same(_multi(sc, "returned"), ref, "group 3")
        assert _C.set_option("views_batched") == 3 and all(k[0] > 0 for k in map(key, _slot_estimates(V, 3)))
        _C.set_option("view_slot_group", 0)

    group = _C.set_option("view_slot_group")
    try:
        _in_fresh_thread(body)
    finally:
        assert _C.set_option("view_slot_group") == group                     # (the option is per thread: this thread's is untouched)
