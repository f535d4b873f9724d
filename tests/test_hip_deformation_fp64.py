"""The HexPlane field (csrc/gs_hexplane.h, csrc/gs_hexplane_binned.h) and the fused deformation MLP (csrc/gs_mlp.h) against the explicit fp64
reference of tests/deformation_fp64_reference.py, ELEMENT BY ELEMENT: |got - ref64| <= bar, the bar a counted number of fp32 roundings times the
element's unit (the same expression with every term replaced by its absolute value), on lattice inputs where coordinates and weights are exact
so that the arithmetic is the only error. tests/test_deformation_fp64_host.py pins the reference, the inputs and the bars on the CPU (a fp32
stand-in passes them, five planted defects fail them).

Field: every case runs forward, forward_views, the direct backward, the binned backward in the ordered and the float-atomic mode, and the
batched-views backward in both modes; features, all plane gradients and dL/dxyz are checked on each. MLP: the fp32-MFMA forward (in_dim 16, 48,
80, 112), the bf16-split forward (32, 64, 128) and the backward of every width at row counts around the 16 / 64 / 128-row tiles and at
32897 rows (second trip of the persistent loops), the row-list backward, and the whole network at feat_dim 80 with five levels.

Every test prints the worst error / bar ratio per quantity (`fp64-check ...` lines, visible with -s) and asserts it is <= 1.

Measured on MI355X (worst error / bar per group):
  field, one time per point   features 0.20   planes 0.18 (direct), 0.45 (binned, ordered), 0.18 (binned, float atomics)   dL/dxyz 0.035
  field, batched views        features 0.25   planes 0.47 (ordered), 0.18 (float atomics)                                dL/dxyz 0.025
  MLP, fp32-MFMA forward      out 0.046   dF 0.037   parameter gradients 0.092 (tile edges), 0.152 (32897 rows)
  MLP, bf16-split forward     out 0.028   dF 0.044   parameter gradients 0.082 (tile edges), 0.093 (32897 rows)
  MLP, row lists              dF 0.044    parameter gradients 0.105
  network, feat_dim 80        out 6e-4 of its propagated bar; gradients rel-L1 3.5e-7 (bar 1e-4)"""
import contextlib
import ctypes

import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)
import deformation
import deformation_fp64_reference as R
import hexplane
from diff_gaussian_rasterization import _C

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_GRADS = 1e-4            # the aggregate gradient bar of tests/test_hip_deformation.py (end-to-end case only)


@contextlib.contextmanager
def hex_ordered(value):
    old = _C.set_option("hex_ordered", value)
    try:
        yield
    finally:
        _C.set_option("hex_ordered", old)


def _levels_on_device(d):
    return [[p.to(DEV).requires_grad_(True) for p in lv] for lv in d.levels]       # .to keeps the strides: channels-last stays channels-last


def _plane_grads(levels):
    return [[p.grad for p in lv] for lv in levels]


def _check(tag, ratios):
    R.report(tag, **ratios)
    assert max(ratios.values()) <= 1, (tag, ratios)


SINGLE_ROUTES = [(name, route) for name in R.FIELD_CASE_NAMES for route in ("direct", "binned_ordered", "binned_float")
                 if route == "direct" or "planar" not in name]               # the sorted backward takes channels-last planes only


@pytest.mark.parametrize("name,route", SINGLE_ROUTES)
def test_field_single_time_matches_fp64_per_element(name, route, monkeypatch):
    """hexplane_features with one time per point. direct: hexplane_bwd_lane_kernel (planar: hexplane_bwd_kernel), float atomics; binned: the counting
    sort and hexsort_phase2_kernel<C, 4 or 8 levels, ordered or not>."""
    d, ref = R.field_case(name), R.field_case_reference(name, "single")
    monkeypatch.setenv("GSR_HEX_BINNED", "0" if route == "direct" else "1")
    mode = "ordered" if route == "binned_ordered" else "float"
    levels = _levels_on_device(d)
    pts = d.pts.to(DEV).requires_grad_(True)
    with hex_ordered(1 if mode == "ordered" else 0):
        feat = hexplane.hexplane_features(pts, d.time_pp.reshape(-1, 1).to(DEV), d.aabb.to(DEV), levels)
        feat.backward(d.cot_pp.to(DEV))
        torch.cuda.synchronize()
    assert feat.shape == (d.n, d.L * d.C)
    _check(f"field single {name} {route}", R.field_ratios(feat, _plane_grads(levels), pts.grad, ref, mode))


VIEW_ROUTES = [(name, mode) for name in R.FIELD_CASE_NAMES if "planar" not in name for mode in ("ordered", "float")]


@pytest.mark.parametrize("name,mode", VIEW_ROUTES)
def test_field_views_match_fp64_per_element(name, mode):
    """hexplane_features_views: the same points at V times (V in 1, 4, 5, 12; times on and beyond +-1), cotangent rows that are zero in some or
    all views. One sort, hexsort_phase2_views_kernel for the spatial planes, hexsort_phase2_time_kernel (LDS window, or straight to memory for
    runs outside it) for the time planes; five and more levels take the 8-level instantiations."""
    d, ref = R.field_case(name), R.field_case_reference(name, "views")
    levels = _levels_on_device(d)
    pts = d.pts.to(DEV).requires_grad_(True)
    with hex_ordered(1 if mode == "ordered" else 0):
        feat = hexplane.hexplane_features_views(pts, d.times, d.aabb.to(DEV), levels)
        feat.backward(d.cot.to(DEV))
        torch.cuda.synchronize()
    assert feat.shape == (d.V, d.n, d.L * d.C)
    _check(f"field views {name} V={d.V} {mode}", R.field_ratios(feat, _plane_grads(levels), pts.grad, ref, mode))


def test_field_views_forward_of_planar_planes():
    d, ref = R.field_case("c16_l2_planar"), R.field_case_reference("c16_l2_planar", "views")
    with torch.no_grad():
        feat = hexplane.hexplane_features_views(d.pts.to(DEV), d.times, d.aabb.to(DEV), [[p.to(DEV) for p in lv] for lv in d.levels])
    _check("field views forward planar", R.field_ratios(feat, None, None, ref, "float"))


# ---- the MLP -----------------------------------------------------------------------------------------------------------------------------
MLP_DIMS = [16, 32, 48, 64, 80, 96, 112, 128]       # 16, 48, 80, 96, 112: deform_mlp_fwd_kernel<1, 3, 5, 6, 7> (fp32 MFMA); 32, 64, 128: deform_mlp_fwd3_kernel
MLP_SMALL = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129]
MLP_LARGE = [32768 + 129]                       # second trip of the persistent loops (fp32 forward 32768, bf16 forward 16384, backward 16384 rows), ragged tail


def _mlp_run(case, n):
    rows = torch.arange(n) % R.MLP_ROWS
    feat = case.x[rows].to(DEV).requires_grad_(True)
    params = [p.to(DEV).requires_grad_(True) for p in case.params]
    out = deformation._FusedDeformMLP.apply(feat, *params)
    out.backward(case.dout[rows].to(DEV))
    torch.cuda.synchronize()
    return out, feat.grad, [p.grad for p in params]


@pytest.mark.parametrize("counts", [MLP_SMALL, MLP_LARGE], ids=["tile_edges", "second_trip"])
@pytest.mark.parametrize("in_dim", MLP_DIMS)
def test_fused_mlp_matches_fp64_per_element(in_dim, counts):
    case = R.mlp_case(in_dim)
    assert R.mlp_margin(case.ref) > 1                              # no ReLU mask can flip within the bars: the backward is comparable per element
    worst = {}
    for n in counts:
        out, dF, grads = _mlp_run(case, n)
        assert out.shape == (n, 10) and dF.shape == (n, in_dim)
        r = R.mlp_ratios(out, dF, grads, R.mlp_reference_rows(case, n))
        R.report(f"mlp in_dim={in_dim} n={n}", **r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    _check(f"mlp in_dim={in_dim} worst over n={counts[0]}..{counts[-1]}", worst)


ROW_LISTS = {
    "first_and_last": [0, R.MLP_ROWS - 1],
    "straddles_a_tile": list(range(40, 110)),                      # 70 entries: two trips over the list, rows on both sides of row 64
    "skips_whole_tiles": list(range(0, 10)) + list(range(130, R.MLP_ROWS)),
    "empty": [],
}
SENTINEL = 12345.0


@pytest.mark.parametrize("which", list(ROW_LISTS))
@pytest.mark.parametrize("in_dim", MLP_DIMS)
def test_mlp_backward_over_a_row_list(in_dim, which):
    """gsr_deform_mlp_backward_rows: only the listed rows take part -- dF of the others keeps what it held, the parameter gradients are those of a
    cotangent that is zero on the unlisted rows; an empty list gives gradients that are exactly zero."""
    case = R.mlp_case(in_dim)
    n = R.MLP_ROWS
    listed = torch.tensor(ROW_LISTS[which], dtype=torch.int32)
    feat, dout = case.x.to(DEV), case.dout.to(DEV)
    params = [p.to(DEV) for p in case.params]
    lib = _C.load_library()
    dfeat = torch.full((n, in_dim), SENTINEL, dtype=torch.float32, device=DEV)
    flat = torch.full((lib.gsr_deform_mlp_grad_count(in_dim),), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.empty((lib.gsr_deform_mlp_workspace_size(in_dim),), dtype=torch.uint8, device=DEV)
    rows = torch.cat([listed, torch.zeros(1, dtype=torch.int32)]).to(DEV)             # never a null pointer, also for the empty list
    n_rows = torch.tensor([len(listed)], dtype=torch.int32, device=DEV)
    m = deformation._FusedDeformMLP._describe(in_dim, params)
    with torch.cuda.device(feat.device):
        rc = lib.gsr_deform_mlp_backward_rows(ctypes.byref(m), n, feat.data_ptr(), dout.data_ptr(), dfeat.data_ptr(), flat.data_ptr(), ws.data_ptr(),
                                              rows.data_ptr(), n_rows.data_ptr(), _C._stream(feat.device))
    torch.cuda.synchronize()
    assert rc == 0
    grads, off = [], 0
    for p in params:
        grads.append(flat[off:off + p.numel()].view(p.shape).cpu())
        off += p.numel()
    assert off == flat.numel()
    unlisted = torch.ones(n, dtype=torch.bool)
    unlisted[listed.long()] = False
    assert bool((dfeat.cpu()[unlisted] == SENTINEL).all())                             # untouched
    if len(listed) == 0:
        assert all(float(g.abs().max()) == 0.0 for g in grads)
        R.report(f"mlp rows in_dim={in_dim} {which}", dF=0.0, params=0.0)
        return
    ref = R.mlp_reference_rows(case, n, listed)
    r = R.mlp_ratios(None, dfeat, None, ref, rows=listed)
    r.update(R.mlp_ratios(None, None, grads, ref))
    _check(f"mlp rows in_dim={in_dim} {which}", r)


# ---- the network shape no other test runs: 16 channels x 5 levels = feat_dim 80 -----------------------------------------------------------
def _network_80():
    args = deformation.default_hidden_params(bounds=2.0, multires=[1, 2, 3, 4, 5],
                                             kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 16, "resolution": [5, 5, 5, 5]})
    torch.manual_seed(11)
    net = deformation.deform_network(args, DEV).to(DEV)
    with torch.no_grad():
        for lv in net.deformation_net.grid.grids:
            for p in lv:
                p.uniform_(0.2, 1.3)                               # informative time planes (they start as ones)
    dn = net.deformation_net
    mlp = [dn.feature_out[0].weight, dn.feature_out[0].bias]
    for h in (dn.pos_deform, dn.scales_deform, dn.rotations_deform):
        mlp += [h[1].weight, h[1].bias, h[3].weight, h[3].bias]
    planes = [[p for p in lv] for lv in dn.grid.grids]
    return net, planes, mlp


def _network_reference(d, planes, mlp, times, cot, per_point):
    """the composed fp64 reference: field -> MLP (its input unit the features' bar) -> back through the field"""
    levels = [[p.detach().cpu() for p in lv] for lv in planes]
    aabb = torch.tensor([[d.bound] * 3, [-d.bound] * 3])
    f = R.field_reference(d.pts, times, aabb, levels, None, per_point=per_point)
    m = R.mlp_reference(f.feat.reshape(-1, f.feat.shape[-1]), [p.detach().cpu() for p in mlp], cot.reshape(-1, 10), e_x=R.feature_bar(f).reshape(-1, f.feat.shape[-1]))
    b = R.field_reference(d.pts, times, aabb, levels, m.dF.reshape(f.feat.shape), per_point=per_point)
    return m, b


def _network_gradient_ratios(pts, planes, mlp, m, b):
    worst = R.rel_l1(pts.grad, b.gxyz)
    for l, lv in enumerate(planes):
        for p, plane in enumerate(lv):
            worst = max(worst, R.rel_l1(plane.grad, b.gplanes[l][p]))
    for k, w in enumerate(mlp):
        worst = max(worst, R.rel_l1(w.grad, m.grads[k]))
    return worst


def test_network_with_feat_dim_80_forward_and_forward_views():
    """deform_network with output_coordinate_dim 16 and five levels on lattice points: the fp32-MFMA forward and the MLP backward at NT = 5 in both
    halves. The `forward` half (257 points, fewer than hexplane.BINNED_MIN_POINTS) takes the field's direct backward; only the `forward_views`
    half reaches the 8-level walks of the sorted backward, and the row-list MLP backward. Outputs per element against the propagated unit;
    gradients at the aggregate bar of tests/test_hip_deformation.py, because a ReLU mask at a pre-activation within rounding of zero cannot be
    excluded here."""
    d = R.field_case("c8_l6")                                      # 257 lattice points in a +-2 box, its times and cotangent seeds
    net, planes, mlp = _network_80()
    assert net.deformation_net.grid.feat_dim == 80 and net.deformation_net._fused_mlp_ok(d.pts.to(DEV))
    g = torch.Generator().manual_seed(5)
    z = lambda k: torch.zeros((d.n, k), device=DEV)
    # ---- forward: one time per point ----
    cot = torch.randn(d.n, 10, generator=g)
    pts = d.pts.to(DEV).requires_grad_(True)
    means, scales, rots, dx, ds, dr = net(pts, z(3), z(4), z(1), z(48), d.time_pp.reshape(-1, 1).to(DEV))
    out = torch.cat([dx, ds, dr], -1)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    m, b = _network_reference(d, planes, mlp, d.time_pp, cot.double(), True)
    ratios = {"out": R.worst_ratio(out, m.out, m.e_out)}
    moved = torch.cat([means, scales, rots], -1)
    moved_ref = m.out + torch.cat([d.pts.double(), torch.zeros(d.n, 7, dtype=torch.float64)], -1)
    ratios["moved"] = R.worst_ratio(moved, moved_ref, m.e_out + R.EPS32 * moved_ref.abs())          # one more rounding: raw parameter + delta
    grad_rel = _network_gradient_ratios(pts, planes, mlp, m, b)
    R.report("network feat_dim=80 forward", gradients_rel_l1=grad_rel, **ratios)
    assert max(ratios.values()) <= 1 and grad_rel < REL_GRADS, (ratios, grad_rel)
    # ---- forward_views: three views, rows of the cotangent that are zero ----
    for w in [pts] + [p for lv in planes for p in lv] + mlp:
        w.grad = None
    times = (0.0, -1.25, 1.0)
    cot = torch.randn(3, d.n, 10, generator=g)
    cot[torch.rand(3, d.n, generator=g) < 0.4] = 0.0
    cot[:, ::7] = 0.0
    out = net.forward_views(pts, times)
    assert out is not None and out.shape == (3, d.n, 10)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    m, b = _network_reference(d, planes, mlp, times, cot.double(), False)
    ratios = {"out": R.worst_ratio(out.reshape(-1, 10), m.out, m.e_out)}
    grad_rel = _network_gradient_ratios(pts, planes, mlp, m, b)
    R.report("network feat_dim=80 forward_views V=3", gradients_rel_l1=grad_rel, **ratios)
    assert max(ratios.values()) <= 1 and grad_rel < REL_GRADS, (ratios, grad_rel)
