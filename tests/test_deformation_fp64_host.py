"""CPU only: pins tests/deformation_fp64_reference.py -- the explicit fp64 restatement of the HexPlane field and the deformation MLP, its units
and the per-element bars of tests/test_hip_deformation_fp64.py -- before any GPU time is spent:
  * the restatement equals autograd through oracle/deformation_oracle.py in fp64 to 1e-12 on every lattice input set, and reproduces the golden
    vectors of the reference's own HexPlaneField at that file's tolerances;
  * the same restatement run in fp32 (a correct kernel's stand-in) passes every bar on every input set, in both accumulation modes;
  * five planted defects, applied to the fp32 stand-in, each fail the per-element bar while passing the aggregate rel-L1 bar of
    tests/test_hip_deformation.py (1e-5 values, 1e-4 gradients). Both figures are printed (`fp64-check ...` lines, visible with -s)."""
import os

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)
import deformation_fp64_reference as R
from oracle import deformation_oracle as O

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_deformation.npz"))
REL_VALUES, REL_GRADS = 1e-5, 1e-4          # the aggregate bars of tests/test_hip_deformation.py


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


def oracle_autograd(d, route):
    pts = d.pts.double().requires_grad_(True)
    levels = [[p.double().contiguous().requires_grad_(True) for p in lv] for lv in d.levels]
    if route == "single":
        feat = O.hexplane_field(pts, d.time_pp.double().reshape(-1, 1), d.aabb.double(), levels)
        (feat * d.cot_pp.double()).sum().backward()
    else:
        feat = torch.stack([O.hexplane_field(pts, torch.full((d.n, 1), float(t), dtype=torch.float64), d.aabb.double(), levels) for t in d.times])
        (feat * d.cot.double()).sum().backward()
    return feat.detach(), pts.grad, [[p.grad for p in lv] for lv in levels]


@pytest.mark.parametrize("route", ["single", "views"])
@pytest.mark.parametrize("name", R.FIELD_CASE_NAMES)
def test_explicit_field_reference_equals_oracle_autograd(name, route):
    d, ref = R.field_case(name), R.field_case_reference(name, route)
    feat, gxyz, gplanes = oracle_autograd(d, route)
    assert ref.feat.shape == feat.shape and close(ref.feat, feat)
    assert close(ref.gxyz, gxyz)
    for l in range(d.L):
        for p in range(6):
            assert close(ref.gplanes[l][p], gplanes[l][p]), (l, p)
    # units bound the values they belong to, and are zero only where the value is
    assert bool((ref.feat.abs() <= ref.feat_unit * (1 + 1e-12)).all()) and bool((ref.gxyz.abs() <= ref.gxyz_unit * (1 + 1e-12) + 1e-300).all())


def test_lattice_inputs_contain_what_the_bars_need():
    for name in R.FIELD_CASE_NAMES:
        d = R.field_case(name)
        q = d.q
        assert np.all(np.abs(q) <= R.LATTICE_MAX)
        assert torch.equal(d.pts.double() * (R.LATTICE / d.bound), torch.tensor(q, dtype=torch.float64))      # exact in fp32
        assert all(float(t) * R.LATTICE == int(float(t) * R.LATTICE) for t in d.times)
        assert max(max(r) for r in d.res) <= 1024
        if d.n >= 35:
            for a in range(3):
                for v in (-R.LATTICE, 0, R.LATTICE):
                    assert np.any(q[:, a] == v), (name, a, v)
                assert np.any(q[:, a] > R.LATTICE) and np.any(q[:, a] < -R.LATTICE)
        if d.V >= 4:
            assert max(d.times) > 1 and min(d.times) < -1 and 1.0 in d.times and 0.0 in d.times
        assert float(d.time_pp.abs().max()) > 1 or d.n < 3
        if d.n >= 2049:
            fine = d.res[-1]
            cell = np.stack([np.floor((-q[:, a] / R.LATTICE + 1) / 2 * (fine[a] - 1)) for a in range(3)], 1)
            inside = np.all(np.abs(q) < R.LATTICE, axis=1)
            cells, counts = np.unique(cell[inside], axis=0, return_counts=True)
            k = counts.argmax()
            members = q[inside][np.all(cell[inside] == cells[k], axis=1)]
            assert counts[k] >= 300 and len(np.unique(members, axis=0)) >= 300, (name, counts[k])
            assert d.n - len(np.unique(q, axis=0)) >= d.n // 10                                       # exact duplicates
        if d.n > 1:
            zero = (d.cot == 0).all(dim=2)
            assert bool(zero.any()) and bool(zero.all(dim=0).any()) and not bool(zero.all())


def test_explicit_reference_reproduces_the_golden_field():
    levels = [[torch.tensor(G[f"field/plane_{l}_{p}"]) for p in range(6)] for l in range(2)]
    ref = R.field_reference(torch.tensor(G["field/pts"]), torch.tensor(G["field/time"]).reshape(-1), torch.tensor(G["field/aabb"]), levels,
                            torch.tensor(G["field/cotangent"]), per_point=True)
    assert R.rel_l1(ref.feat, G["field/features"]) < 2e-6
    assert R.rel_l1(ref.gxyz[8:], G["field/g_pts"][8:]) < 2e-5            # rows 0-7 sit on texel centres (tests/test_deformation_oracle.py)
    for l in range(2):
        for p in range(6):
            assert R.rel_l1(ref.gplanes[l][p], G[f"field/g_plane_{l}_{p}"]) < 2e-5, (l, p)


@pytest.mark.parametrize("mode", ["float", "ordered"])
@pytest.mark.parametrize("route", ["single", "views"])
@pytest.mark.parametrize("name", R.FIELD_CASE_NAMES)
def test_fp32_stand_in_passes_every_field_bar(name, route, mode):
    d, ref = R.field_case(name), R.field_case_reference(name, route)
    if route == "single":
        got = R.field_reference(d.pts, d.time_pp, d.aabb, d.levels, d.cot_pp, per_point=True, dtype=torch.float32, accumulate=mode)
    else:
        got = R.field_reference(d.pts, d.times, d.aabb, d.levels, d.cot, dtype=torch.float32, accumulate=mode)
    r = R.field_ratios(got.feat, got.gplanes, got.gxyz, ref, mode)
    R.report(f"stand-in field {name} {route} {mode}", **r)
    assert max(r.values()) <= 1, r
    # exact zeros: a unit of zero means the fp64 value is zero, too
    assert bool((ref.gxyz[ref.gxyz_unit == 0] == 0).all())


def _defect_case():
    name = "c32_l4_morton"
    d = R.field_case(name)
    return name, d, R.field_case_reference(name, "single")


def _stand_in(d, defect):
    return R.field_reference(d.pts, d.time_pp, d.aabb, d.levels, d.cot_pp, per_point=True, dtype=torch.float32, defect=defect)


def _quiet_rows(d, cond):
    """points with a scaled-down, non-zero cotangent row that satisfy cond(normalised lattice numerator row)"""
    qn = -d.q                                                            # the aabb's row 0 is the max corner: the field is sampled mirrored
    return [i for i in range(d.n) if bool(d.quiet[i]) and bool((d.cot_pp[i] != 0).any()) and cond(qn[i])]


def test_planted_defect_dropped_corner_at_a_border_texel():
    name, d, ref = _defect_case()
    l, p = 3, 0                                                          # finest level, plane xy: border texel row y = 0 (normalised y <= -1)
    rows = _quiet_rows(d, lambda q: q[1] <= -R.LATTICE and abs(q[0]) < R.LATTICE)
    assert rows
    got = _stand_in(d, dict(kind="drop_corner", row=rows[0], level=l, plane=p, corner=0))
    per_element = R.worst_ratio(got.gplanes[l][p], ref.gplanes[l][p], R.plane_bar(ref, l, p, "float"))
    aggregate = R.rel_l1(got.gplanes[l][p], ref.gplanes[l][p])
    R.report("defect dropped_corner", per_element=per_element, aggregate=aggregate)
    assert per_element > 1 and aggregate < REL_GRADS


def test_planted_defect_weights_swapped_at_the_upper_border():
    name, d, ref = _defect_case()
    l, p = 2, 1                                                          # plane xz, x exactly on the upper face: u == res - 1
    rows = _quiet_rows(d, lambda q: q[0] == R.LATTICE)
    assert rows
    got = _stand_in(d, dict(kind="swap_w", row=rows[0], level=l, plane=p))
    per_element = R.worst_ratio(got.gplanes[l][p], ref.gplanes[l][p], R.plane_bar(ref, l, p, "float"))
    aggregate = R.rel_l1(got.gplanes[l][p], ref.gplanes[l][p])
    R.report("defect swapped_weights", per_element=per_element, aggregate=aggregate)
    assert per_element > 1 and aggregate < REL_GRADS


def test_planted_defect_two_channels_exchanged():
    name, d, ref = _defect_case()
    l, (a, b) = 1, (3, 17)
    # the point at which the two channels differ least while still differing by far more than their bars: a small mistake, not a loud one
    fa, fb, bar = ref.feat[:, l * d.C + a], ref.feat[:, l * d.C + b], R.feature_bar(ref)
    diff = (fa - fb).abs()
    diff[diff < 1000 * torch.maximum(bar[:, l * d.C + a], bar[:, l * d.C + b])] = float("inf")
    got = _stand_in(d, dict(kind="swap_channels", row=int(diff.argmin()), level=l, channels=(a, b)))
    per_element = R.worst_ratio(got.feat, ref.feat, R.feature_bar(ref))
    aggregate = R.rel_l1(got.feat, ref.feat)
    R.report("defect exchanged_channels", per_element=per_element, aggregate=aggregate)
    assert per_element > 1 and aggregate < REL_VALUES


def test_planted_defect_dmult_on_the_lower_border():
    name, d, ref = _defect_case()
    rows = _quiet_rows(d, lambda q: q[0] == -R.LATTICE)                  # normalised x == -1: u == 0 on every level
    assert rows
    row = rows[0]
    assert float(ref.gxyz_unit[row, 0]) == 0.0 and float(ref.gxyz[row, 0]) == 0.0
    got = _stand_in(d, dict(kind="dmult", row=row, level=0, axis=0))
    per_element = R.worst_ratio(got.gxyz, ref.gxyz, R.xyz_bar(ref))
    aggregate = R.rel_l1(got.gxyz, ref.gxyz)
    R.report("defect dmult_at_u0", per_element=per_element, aggregate=aggregate, planted=float(got.gxyz[row, 0]))
    assert float(got.gxyz[row, 0]) != 0.0 and per_element > 1 and aggregate < REL_GRADS


# ---- the MLP -----------------------------------------------------------------------------------------------------------------------------
MLP_DIMS = [16, 32, 48, 64, 80, 96, 112, 128]


@pytest.mark.parametrize("in_dim", MLP_DIMS)
def test_mlp_rows_clear_their_relu_margins(in_dim):
    case = R.mlp_case(in_dim)
    margin = R.mlp_margin(case.ref)
    R.report(f"mlp margin in_dim={in_dim}", margin=margin)
    assert margin > 2
    assert len(torch.unique(case.x, dim=0)) == R.MLP_ROWS
    assert all(float(b.abs().min()) >= 0.05 for b in case.params[1::2]) and all(float(w.abs().min()) > 0 for w in case.params[0::2])
    # the masks are not trivial: every unit of h0, and at least half of the units of the u_j, is active for some rows and idle for others
    on = (case.ref.h0 > 0).double().mean(0)
    assert bool(((on > 0) & (on < 1)).all())
    on = torch.cat([(u > 0).double().mean(0) for u in case.ref.u])
    assert float(((on > 0.1) & (on < 0.9)).double().mean()) > 0.5


@pytest.mark.parametrize("in_dim", MLP_DIMS)
def test_explicit_mlp_reference_equals_autograd(in_dim):
    case = R.mlp_case(in_dim)
    x = case.x.double().requires_grad_(True)
    P = [p.double().requires_grad_(True) for p in case.params]
    a = torch.relu(x @ P[0].t() + P[1])
    out = torch.cat([torch.relu(a @ P[2 + 4 * j].t() + P[3 + 4 * j]) @ P[4 + 4 * j].t() + P[5 + 4 * j] for j in range(3)], -1)
    (out * case.dout.double()).sum().backward()
    assert close(case.ref.out, out.detach()) and close(case.ref.dF, x.grad)
    for k in range(14):
        assert close(case.ref.grads[k], P[k].grad), k
    # repeated rows: per-row results and repeat counts against the batch written out
    n = 192 + 77
    rows = torch.arange(n) % R.MLP_ROWS
    full = R.mlp_reference(case.x[rows], case.params, case.dout[rows])
    short = R.mlp_reference_rows(case, n)
    assert close(short.out, full.out) and close(short.dF, full.dF)
    for k in range(14):
        assert close(short.grads[k], full.grads[k]) and close(short.e_grads[k], full.e_grads[k], 1e-9), k


@pytest.mark.parametrize("n", [1, 65, 192, 32897])
@pytest.mark.parametrize("in_dim", MLP_DIMS)
def test_fp32_stand_in_passes_every_mlp_bar(in_dim, n):
    case = R.mlp_case(in_dim)
    rows = torch.arange(n) % R.MLP_ROWS
    got = R.mlp_reference(case.x[rows], case.params, case.dout[rows], dtype=torch.float32)
    r = R.mlp_ratios(got.out, got.dF, got.grads, R.mlp_reference_rows(case, n))
    R.report(f"stand-in mlp in_dim={in_dim} n={n}", **r)
    assert max(r.values()) <= 1, r


def test_planted_defect_head_column_in_a_tile_tail_row():
    case = R.mlp_case(80)
    n, row = 128, 63                                                     # the last row of the first 64-row tile
    column = int((case.ref.out[row].abs() / case.ref.e_out[row]).argmax())   # the column whose bar is tightest relative to its value
    got = R.mlp_reference(case.x[:n], case.params, dtype=torch.float32, defect=dict(kind="scale_output", row=row, column=column, factor=1 + 1e-4))
    ref = R.mlp_reference_rows(case, n)
    per_element = R.worst_ratio(got.out, ref.out, ref.e_out)
    aggregate = R.rel_l1(got.out, ref.out)
    R.report("defect head_column", per_element=per_element, aggregate=aggregate)
    assert per_element > 1 and aggregate < REL_VALUES


MLP_NAMES = ["feature_out.0", "pos_deform.1", "pos_deform.3", "scales_deform.1", "scales_deform.3", "rotations_deform.1", "rotations_deform.3"]
# every lattice input set whose feature width the fused MLP takes (a multiple of 16 up to 128)
COMPOSED = [name for name in R.FIELD_CASE_NAMES if R.field_case(name).L * R.field_case(name).C in MLP_DIMS]


@pytest.mark.parametrize("route", ["single", "views"])
@pytest.mark.parametrize("name", COMPOSED)
def test_composed_reference_equals_oracle_network(name, route):
    """the field restatement feeding the MLP restatement against autograd through oracle.deformation_oracle.deform_network, fp64, to 1e-12"""
    d = R.field_case(name)
    case = R.mlp_case(d.L * d.C)
    pre = "deformation_net."
    state = {pre + "grid.aabb": d.aabb.double()}
    for l, lv in enumerate(d.levels):
        for p, plane in enumerate(lv):
            state[f"{pre}grid.grids.{l}.{p}"] = plane.double().contiguous().requires_grad_(True)
    for k, nm in enumerate(MLP_NAMES):
        state[f"{pre}{nm}.weight"] = case.params[2 * k].double().requires_grad_(True)
        state[f"{pre}{nm}.bias"] = case.params[2 * k + 1].double().requires_grad_(True)
    pts = d.pts.double().requires_grad_(True)
    z = lambda k: torch.zeros((d.n, k), dtype=torch.float64)
    times = [d.time_pp.double().reshape(-1, 1)] if route == "single" else [torch.full((d.n, 1), float(t), dtype=torch.float64) for t in d.times]
    out = torch.stack([torch.cat(O.deform_network(state, pts, z(3), z(4), z(1), z(48), t)[3:], -1) for t in times])      # [V, n, 10]
    V = len(times)
    cot = case.dout[torch.arange(V * d.n) % R.MLP_ROWS].double().reshape(V, d.n, 10)
    (out * cot).sum().backward()
    field = (lambda c: R.field_reference(d.pts, d.time_pp, d.aabb, d.levels, c, per_point=True)) if route == "single" else \
            (lambda c: R.field_reference(d.pts, d.times, d.aabb, d.levels, c))
    f = field(None)
    m = R.mlp_reference(f.feat.reshape(V * d.n, -1), case.params, cot.reshape(-1, 10))
    f = field(m.dF.reshape(f.feat.shape))
    assert close(m.out, out.detach().reshape(-1, 10)) and close(f.gxyz, pts.grad)
    for k, nm in enumerate(MLP_NAMES):
        assert close(m.grads[2 * k], state[f"{pre}{nm}.weight"].grad) and close(m.grads[2 * k + 1], state[f"{pre}{nm}.bias"].grad), nm
    for l in range(d.L):
        for p in range(6):
            assert close(f.gplanes[l][p], state[f"{pre}grid.grids.{l}.{p}"].grad), (l, p)


def test_composed_reference_reproduces_the_golden_network():
    """net1 of the golden file -- the reference's own deform_network with defor_depth 1, width 64, two levels of 32 channels, the structure
    csrc/gs_mlp.h fuses -- at that file's tolerances (tests/test_deformation_oracle.py: 1e-5 values, 1e-4 gradients)."""
    tag, pre = "net1", "deformation_net."
    S = lambda k: torch.tensor(G[f"{tag}/state/{k}"])
    levels = [[S(f"{pre}grid.grids.{l}.{p}") for p in range(6)] for l in range(2)]
    params = [S(f"{pre}{nm}.{w}") for nm in MLP_NAMES for w in ("weight", "bias")]
    I = lambda k: torch.tensor(G[f"{tag}/{k}"]).double()
    pts, tim, aabb = I("in_point"), I("in_time").reshape(-1), S(pre + "grid.aabb")
    f = R.field_reference(pts, tim, aabb, levels, None, per_point=True)
    # the recorded loss weighs all six outputs; means3D, scales and rotations are the raw inputs plus the deltas
    cot = torch.cat([I("cot_dx") + I("cot_means3D"), I("cot_ds") + I("cot_scales"), I("cot_dr") + I("cot_rotations")], -1)
    m = R.mlp_reference(f.feat, params, cot)
    for name, sl, raw in (("dx", slice(0, 3), None), ("ds", slice(3, 6), None), ("dr", slice(6, 10), None),
                          ("means3D", slice(0, 3), "in_point"), ("scales", slice(3, 6), "in_scales"), ("rotations", slice(6, 10), "in_rotations")):
        want = m.out[:, sl] + (I(raw) if raw else 0.0)
        assert R.rel_l1(want, G[f"{tag}/out_{name}"]) < REL_VALUES, name
    b = R.field_reference(pts, tim, aabb, levels, m.dF, per_point=True)
    assert R.rel_l1(b.gxyz + I("cot_means3D"), G[f"{tag}/g_in_point"]) < REL_GRADS
    for k, nm in enumerate(MLP_NAMES):
        assert R.rel_l1(m.grads[2 * k], G[f"{tag}/grad/{pre}{nm}.weight"]) < REL_GRADS, nm
        assert R.rel_l1(m.grads[2 * k + 1], G[f"{tag}/grad/{pre}{nm}.bias"]) < REL_GRADS, nm
    for l in range(2):
        for p in range(6):
            assert R.rel_l1(b.gplanes[l][p], G[f"{tag}/grad/{pre}grid.grids.{l}.{p}"]) < REL_GRADS, (l, p)
