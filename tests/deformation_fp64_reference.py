"""Test infrastructure: the HexPlane field and the fused deformation MLP (csrc/gs_hexplane.h, csrc/gs_hexplane_binned.h, csrc/gs_mlp.h) restated
with explicit index arithmetic -- no autograd, no F.grid_sample -- in whatever dtype is asked for, every result together with its UNIT: the same
expression with every term replaced by its absolute value. fp64 is the reference the GPU tests compare with element by element; the same code in
fp32 stands in for a correct kernel on the CPU (tests/test_deformation_fp64_host.py), optionally with one planted defect.

What is restated is what oracle/deformation_oracle.py describes (normalize_aabb, bilinear sampling with border padding and align_corners=True,
the product over the six planes, the concatenation over levels) and the MLP of csrc/gs_mlp.h (W0, ReLU, three heads 64 -> 64 -> 3 / 3 / 4).

Units
  sample of one plane      S_p = sum over the four corners of |w_c * texel_c|
  feature                  prod over the six planes of S_p
  plane gradient, a texel  sum over the (view, point) rows that reach it of |gs| * w_c,  |gs| = |g| * prod_{q != p} S_q
  dL/dxyz, a component     the ATen formula with |.| on every term (|ne| + |nw|, ... ), times dmult, summed over channels, planes, levels and views,
                           times |dscale|
  MLP                      e_out = e_in |W|^T + c (|a| |W|^T + |b|) layer by layer, ReLU passes e through; the backward the same way with the
                           transposed products (c = C_MLP)

Bars (field, on lattice inputs where coordinates, weights and weight products are exact in fp32, so that the arithmetic is the only error):
|got - ref64| <= K * 2^-23 * unit, K from `field_roundings`; an element whose unit is 0 must be exactly 0. The accumulation of a texel's N_T
contributions is accounted separately (`plane_bar`): one rounding to the fixed-point quantum each in the ordered mode, one fp32 rounding of the
running sum each where float atomics add in whatever order."""
import functools
import itertools
import math
import types

import numpy as np
import torch

COMBOS = list(itertools.combinations(range(4), 2))     # plane p spans coordinates (c0, c1): xy, xz, xt, yz, yt, zt; c0 indexes the width
EPS32 = 2.0 ** -23
C_MLP = 2e-6            # tests/test_hip_dense.py's per-element bound of the six-term bf16 product, relative to |X| |W|^T + |b|
ORD_BUDGET = 40         # HexOrd: the largest |dL/dsample| of a call is scaled to just below 2^40 (csrc/gs_capi.hip hexord_carve_tail, n < 2^20)


# ---- the field ---------------------------------------------------------------------------------------------------------------------------
def field_roundings(L, V, C):
    """The fp32 roundings on the longest chain of each quantity, each at most 2^-24 of the running magnitude, which the unit bounds.

    sample       1 product + 3 fma                                                          4   (the weight products w_x * w_y are exact on the lattice)
    feature      6 samples x 4, 5 products (1 * s_0 is exact)                               29
    dL/dsample   5 samples x 4, 5 products (g, prefix, suffix)                              25  = gs
    plane texel  a spatial plane: gs, the V - 1 adds where the batched path sums gs over the views, gs * w, the ordered mode's conversion to float
                 (26 + V); a time family of the batched path: gs, gs * w_x, the conversion, sum * w_t and the V adds of the views in their
                 order (28 + V)                                                             28 + V
                 (the sum over the N_T contributions of the texel itself is `plane_bar`'s second term)
    dL/dxyz      one term: gs (25, + V - 1 for a view-summed spatial plane), corner * gs (1; the four-channels-per-lane kernel's dot4: 1 + 3
                 adds, but two shuffle steps fewer), the difference, * w, the add of the two halves, * dmult (4); the log2 C shuffle steps;
                 * dscale is exact (a power of two)                                         32 + V + log2 C
                 The running sum of the terms -- per level the V time-plane terms in view order, then the spatial planes', over the L levels --
                 is not counted but followed: add k rounds a partial sum that the units of the first k terms bound, and the reference
                 returns the sum of those bounds in the kernels' order (`gxyz_chain`, at most L (V + 2) units).
    Single time (V = 1), 8 levels, 64 channels: 29, 29 and at most 39 + 24 = 63 roundings, i.e. K <= 32 in units of 2^-23."""
    return {"feature": 29, "plane": 28 + V, "xyz_terms": 32 + V + int(math.log2(C))}


def field_K(quantity, L, V, C):
    """`field_roundings` in units of EPS32 = 2^-23 (two roundings of 2^-24 each)."""
    return (field_roundings(L, V, C)[quantity] + 1) // 2


def _axis(coord, size):
    """hex_axis (csrc/gs_hexplane.h) = ATen's unnormalise + clip_coordinates_set_grad: i0, i1 (a valid index), w0, w1, has1, dmult."""
    hi = float(size - 1)
    u = ((coord + 1.0) * 0.5) * hi
    inside = (u > 0) & (u < hi)
    dmult = torch.where(inside, torch.full_like(u, 0.5 * hi), torch.zeros_like(u))
    u = u.clamp(0.0, hi)
    f = torch.floor(u)
    i0 = f.long()
    has1 = (i0 + 1) < size
    return types.SimpleNamespace(i0=i0, i1=torch.where(has1, i0 + 1, i0), w0=(f + 1.0) - u, w1=u - f, has1=has1, dmult=dmult)


def level_resolution(planes):
    """(res_x, res_y, res_z, res_t) of a level from its six [1, C, res[c1], res[c0]] planes."""
    return [planes[0].shape[3], planes[0].shape[2], planes[1].shape[2], planes[2].shape[2]]


def field_reference(pts, times, aabb, levels, cot, *, dtype=torch.float64, per_point=False, accumulate="float", defect=None):
    """pts [n, 3]; times: V floats (the same points at V times, cot [V, n, L C]) or, per_point, a tensor of n times (cot [n, L C]); aabb [2, 3]
    (row 0 the corner that maps to -1) or None; levels: lists of six [1, C, H, W] planes. cot None: forward only.
    -> features, plane gradients (summed over the views) and dL/dxyz, each with its unit; `count` N_T per texel; `gsmax` the largest |dL/dsample|
    as the ordered mode sees it. accumulate = "ordered" (fp32 stand-in only): the contributions are rounded to the ordered mode's quantum and
    summed exactly. defect: one planted mistake, dict(kind=..., row=flattened (view, point) row, level=, plane=, ...)."""
    T = dtype
    pts = torch.as_tensor(pts).to(T)
    n = pts.shape[0]
    if aabb is None:
        p, dscale = pts[:, :3], torch.ones((n, 3), dtype=T)
    else:
        a = torch.as_tensor(aabb).to(T)
        s = 2.0 / (a[1] - a[0])
        v = (pts[:, :3] - a[0]) * s - 1.0
        dscale = torch.where((v >= -1) & (v <= 1), s.expand_as(v), torch.zeros_like(v))
        p = v.clamp(-1.0, 1.0)
    if per_point:
        V, t = 1, torch.as_tensor(times).to(T).reshape(1, n)
    else:
        V = len(times)
        t = torch.tensor([float(x) for x in times], dtype=T).reshape(V, 1).expand(V, n)
    M = V * n
    c4 = torch.cat([p.unsqueeze(0).expand(V, n, 3), t.unsqueeze(-1)], -1).reshape(M, 4)
    L, C = len(levels), levels[0][0].shape[1]
    g_all = None if cot is None else torch.as_tensor(cot).to(T).reshape(M, L * C)
    active = None if cot is None else (g_all != 0).any(dim=1)
    D = defect or {}
    ordered = accumulate == "ordered"
    if ordered:
        gsmax = field_reference(pts, times, aabb, levels, cot, dtype=dtype, per_point=per_point, defect=defect).gsmax
        e = math.floor(math.log2(gsmax)) if gsmax > 0 else 0
        quantum_inv = 2.0 ** (ORD_BUDGET - 1 - e)
    out = types.SimpleNamespace(feat=[], feat_unit=[], gplanes=[], gplane_unit=[], count=[], gsmax=0.0)
    gc = torch.zeros((M, 3), dtype=T)
    gc_unit = torch.zeros((M, 3), dtype=T)
    run, chain = torch.zeros((n, 3), dtype=T), torch.zeros((n, 3), dtype=T)       # dL/dxyz: the units of the terms added so far, and their sum over the adds
    for l, planes in enumerate(levels):
        res = level_resolution(planes)
        ax = [_axis(c4[:, k], res[k]) for k in range(4)]
        if D.get("kind") == "dmult" and D["level"] == l:                  # dmult left non-zero on the border
            ax[D["axis"]].dmult = ax[D["axis"]].dmult.clone()
            ax[D["axis"]].dmult[D["row"]] = 0.5 * (res[D["axis"]] - 1)
        sam = []
        for pi, (c0, c1) in enumerate(COMBOS):
            X, Y, W, H = ax[c0], ax[c1], res[c0], res[c1]
            tex_all = planes[pi][0].permute(1, 2, 0).reshape(H * W, C).to(T)
            wx1, wy1 = torch.where(X.has1, X.w1, torch.zeros_like(X.w1)), torch.where(Y.has1, Y.w1, torch.zeros_like(Y.w1))
            idx = [Y.i0 * W + X.i0, Y.i0 * W + X.i1, Y.i1 * W + X.i0, Y.i1 * W + X.i1]          # nw, ne, sw, se
            w = [X.w0 * Y.w0, wx1 * Y.w0, X.w0 * wy1, wx1 * wy1]
            tex = [tex_all[i] for i in idx]
            s = tex[0] * w[0][:, None]
            S = tex[0].abs() * w[0][:, None]
            for k in range(1, 4):
                s = s + tex[k] * w[k][:, None]
                S = S + tex[k].abs() * w[k][:, None]
            sam.append(types.SimpleNamespace(X=X, Y=Y, W=W, H=H, idx=idx, w=w, tex=tex, s=s, S=S, c0=c0, c1=c1))
        prod, unit = torch.ones((M, C), dtype=T), torch.ones((M, C), dtype=T)
        for q in sam:
            prod, unit = prod * q.s, unit * q.S
        if D.get("kind") == "swap_channels" and D["level"] == l:
            a_, b_ = D["channels"]
            prod = prod.clone()
            prod[D["row"], a_], prod[D["row"], b_] = prod[D["row"], b_].clone(), prod[D["row"], a_].clone()
        out.feat.append(prod)
        out.feat_unit.append(unit)
        if g_all is None:
            continue
        g = g_all[:, l * C:(l + 1) * C]
        suffix, suffix_u = [None] * 6, [None] * 6
        suffix[5], suffix_u[5] = torch.ones((M, C), dtype=T), torch.ones((M, C), dtype=T)
        for pi in range(4, -1, -1):
            suffix[pi], suffix_u[pi] = suffix[pi + 1] * sam[pi + 1].s, suffix_u[pi + 1] * sam[pi + 1].S
        prefix, prefix_u = g, g.abs()
        gp_l, gu_l, cnt_l, term_unit = [], [], [], {}
        for pi, q in enumerate(sam):
            gs, gs_u = prefix * suffix[pi], prefix_u * suffix_u[pi]
            prefix, prefix_u = prefix * q.s, prefix_u * q.S
            spatial_summed = not per_point and q.c1 != 3          # the batched path adds a spatial plane's dL/dsample over the views first
            seen = gs.reshape(V, n, C).sum(0) if spatial_summed else gs
            out.gsmax = max(out.gsmax, float(seen.abs().max()))
            X, Y, W, H = q.X, q.Y, q.W, q.H
            w = list(q.w)
            here = D.get("level") == l and D.get("plane") == pi
            if here and D["kind"] == "swap_w":                    # w0 and w1 exchanged along x for one row (scatter only)
                r = D["row"]
                wx0, wx1 = X.w0.clone(), torch.where(X.has1, X.w1, torch.zeros_like(X.w1))
                wx0[r], wx1[r] = X.w1[r], (X.w0[r] if bool(X.has1[r]) else 0.0)
                wy1 = torch.where(Y.has1, Y.w1, torch.zeros_like(Y.w1))
                w = [wx0 * Y.w0, wx1 * Y.w0, wx0 * wy1, wx1 * wy1]
            if spatial_summed:                                    # one contribution per point: the cells do not depend on the view
                fold = lambda a_: a_.reshape(V, n, -1).sum(0)
                sc_gs, sc_gu, sc_active = fold(gs), fold(gs_u), active.reshape(V, n).any(0)
                sc_idx, sc_w, sc_qw = [i[:n] for i in q.idx], [x[:n] for x in w], [x[:n] for x in q.w]
            else:
                sc_gs, sc_gu, sc_active, sc_idx, sc_w, sc_qw = gs, gs_u, active, q.idx, w, q.w
            gp = torch.zeros((H * W, C), dtype=torch.float64 if ordered else T)
            gu = torch.zeros((H * W, C), dtype=T)
            cnt = torch.zeros((H * W,), dtype=torch.float64)
            for k in range(4):
                contrib = sc_gs * sc_w[k][:, None]
                if here and D["kind"] == "drop_corner" and D["corner"] == k:
                    contrib = contrib.clone()
                    contrib[D["row"]] = 0
                if ordered:
                    contrib = torch.round(contrib.double() * quantum_inv)
                gp.index_add_(0, sc_idx[k], contrib)
                gu.index_add_(0, sc_idx[k], sc_gu * sc_qw[k][:, None])
                cnt.index_add_(0, sc_idx[k], ((sc_qw[k] > 0) & sc_active).double())
            if ordered:
                gp = (gp / quantum_inv).to(T)
            back = lambda a_: a_.reshape(H, W, -1).permute(2, 0, 1).unsqueeze(0)
            gp_l.append(back(gp))
            gu_l.append(back(gu))
            cnt_l.append(back(cnt))
            # the coordinate gradient (ATen grid_sampler_2d_backward): d sample / d (u, v) from the same four corners
            hx, hy = X.has1.to(T)[:, None], Y.has1.to(T)[:, None]
            nw, ne, sw, se = q.tex[0] * gs, q.tex[1] * gs * hx, q.tex[2] * gs * hy, q.tex[3] * gs * (hx * hy)
            nw_u, ne_u, sw_u, se_u = q.tex[0].abs() * gs_u, q.tex[1].abs() * gs_u * hx, q.tex[2].abs() * gs_u * hy, q.tex[3].abs() * gs_u * (hx * hy)
            if q.c0 < 3:
                gc[:, q.c0] += ((ne - nw) * Y.w0[:, None] + (se - sw) * Y.w1[:, None]).sum(-1) * X.dmult
                term_unit[pi, q.c0] = ((ne_u + nw_u) * Y.w0[:, None] + (se_u + sw_u) * Y.w1[:, None]).sum(-1) * X.dmult
                gc_unit[:, q.c0] += term_unit[pi, q.c0]
            if q.c1 < 3:
                gc[:, q.c1] += ((sw - nw) * X.w0[:, None] + (se - ne) * X.w1[:, None]).sum(-1) * Y.dmult
                term_unit[pi, q.c1] = ((sw_u + nw_u) * X.w0[:, None] + (se_u + ne_u) * X.w1[:, None]).sum(-1) * Y.dmult
                gc_unit[:, q.c1] += term_unit[pi, q.c1]
        # the running sum of dL/dxyz in the kernels' order (hexplane_bwd_lane_kernel / hexsort_phase1_body: planes 0..5; hexsort_phase1_views_body:
        # the time planes view by view, then the view-summed spatial planes)
        if per_point:
            order = [(a_, term_unit[pi, a_]) for pi in range(6) for a_ in COMBOS[pi] if a_ < 3]
        else:
            order = [(j, term_unit[pi, j].reshape(V, n)[v]) for v in range(V) for j, pi in enumerate((2, 4, 5))]
            order += [(a_, term_unit[pi, a_].reshape(V, n).sum(0)) for pi in (0, 1, 3) for a_ in COMBOS[pi]]
        for a_, term in order:
            run[:, a_] += term
            chain[:, a_] += run[:, a_]
        out.gplanes.append(gp_l)
        out.gplane_unit.append(gu_l)
        out.count.append(cnt_l)
    shape = (n, L * C) if per_point else (V, n, L * C)
    out.feat = torch.cat(out.feat, -1).reshape(shape)
    out.feat_unit = torch.cat(out.feat_unit, -1).reshape(shape)
    out.gxyz = gc.reshape(V, n, 3).sum(0) * dscale
    out.gxyz_unit = gc_unit.reshape(V, n, 3).sum(0) * dscale.abs()
    out.gxyz_chain = chain * dscale.abs()
    out.L, out.V, out.C = L, V, C
    return out


def feature_bar(ref):
    return field_K("feature", ref.L, ref.V, ref.C) * EPS32 * ref.feat_unit.double()


def xyz_bar(ref):
    """2^-24 x (the roundings of a term and of the shuffle steps x the unit + the followed running sum), see `field_roundings`"""
    return 2.0 ** -24 * (field_roundings(ref.L, ref.V, ref.C)["xyz_terms"] * ref.gxyz_unit.double() + ref.gxyz_chain.double())


def plane_bar(ref, l, p, mode):
    """mode "ordered": each of the N_T contributions is rounded once to the quantum; half a quantum is at most 2^-40 of the call's largest
    |dL/dsample| (budget 40), and the bar allows 2^-39 of it per contribution. mode "float" (float atomics, the direct kernel included): the
    order of the N_T adds is free, one fp32 rounding of a running sum that the unit bounds per add. N_T counts a point once where the batched
    path sums a spatial plane's dL/dsample over the views first, and once per view in its time families."""
    unit, cnt = ref.gplane_unit[l][p].double(), ref.count[l][p]
    bar = field_K("plane", ref.L, ref.V, ref.C) * EPS32 * unit
    return bar + (cnt * 2.0 ** -39 * ref.gsmax if mode == "ordered" else cnt * EPS32 * unit)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar; where the bar is 0 the element has to be exact (ratio inf if it is not)."""
    err = (torch.as_tensor(got).detach().double().cpu() - ref.double()).abs()
    bar = bar.double().expand_as(err)
    ratio = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(ratio.max()) if ratio.numel() else 0.0


def rel_l1(got, ref):
    """the aggregate bar of tests/test_hip_deformation.py"""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return float((got - ref).abs().sum() / ref.abs().sum().clamp_min(1e-30))


def field_ratios(got_feat, got_planes, got_xyz, ref, mode):
    """worst error / bar of the three quantities; got_planes[l][p] may be None (not computed on this route)"""
    r = {}
    if got_feat is not None:
        r["features"] = worst_ratio(got_feat, ref.feat, feature_bar(ref))
    if got_planes is not None:
        r["planes"] = max(worst_ratio(got_planes[l][p], ref.gplanes[l][p], plane_bar(ref, l, p, mode)) for l in range(ref.L) for p in range(6))
    if got_xyz is not None:
        r["xyz"] = worst_ratio(got_xyz, ref.gxyz, xyz_bar(ref))
    return r


# ---- lattice inputs: the arithmetic is the only error -----------------------------------------------------------------------------------------
LATTICE = 1024          # coordinates and times are multiples of 2^-10 in [-1.25, 1.25]: u = ((c + 1) / 2)(res - 1) and both weights are exact in
LATTICE_MAX = 1280      # fp32 for res <= 1024, and so are the products of two weights (multiples of 2^-22 up to 1)

# (name, C, base resolution, level multipliers of the spatial axes, n, V, aabb bound, layout)
FIELD_CASES = [
    ("c32_l4_morton", 32, [5, 5, 5, 5], (1, 2, 4, 8), 2049, 12, 1.0, "channels_last"),      # equal key bits; a block's 2048 points span all 40 columns
    ("c8_l6", 8, [5, 5, 5, 5], (1, 2, 3, 4, 5, 6), 257, 5, 2.0, "channels_last"),
    ("c16_l3_unequal", 16, [9, 3, 17, 2], (1, 2, 4), 65, 4, 1.0, "channels_last"),
    ("c16_l5_unequal", 16, [9, 3, 17, 2], (1, 2, 3, 4, 5), 64, 1, 2.0, "channels_last"),
    ("c16_l7", 16, [5, 5, 5, 5], (1, 2, 3, 4, 5, 6, 7), 7, 5, 1.0, "channels_last"),
    ("c16_l8", 16, [5, 5, 5, 5], (1, 2, 3, 4, 5, 6, 7, 8), 2049, 5, 1.0, "channels_last"),
    ("c64_l4", 64, [9, 3, 17, 2], (1, 2, 4, 8), 257, 4, 1.0, "channels_last"),
    ("c8_l1_big", 8, [129, 129, 129, 9], (1,), 2049, 12, 2.0, "channels_last"),            # > 8192 counters per family; 129 columns in one block
    ("c32_l2_not_nested", 32, [5, 5, 5, 5], (1, 3), 1, 1, 1.0, "channels_last"),
    ("c32_l1_one_time_texel", 32, [5, 5, 5, 1], (1,), 65, 4, 1.0, "channels_last"),
    ("c16_l2_planar", 16, [9, 3, 17, 2], (1, 3), 257, 4, 2.0, "planar"),
]
FIELD_CASE_NAMES = [c[0] for c in FIELD_CASES]

_SPECIAL = [(-1, 0, 1), (1.25, -1.25, 1.125), (0, 1, -1), (-1.25, 1.25, -1.0625), (1, -1, 0), (0, 0, 0), (-1, -1, -1), (1, 1, 1)]
_SPECIAL_T = [0.0, -1.25, 1.0, 1.25, -1.0, 0.3125, -0.5, 1.125, 0.0009765625, -1.0009765625, 0.75, -0.25]


@functools.lru_cache(maxsize=None)
def field_case(name):
    """The inputs of one case, on the CPU in fp32 (bitwise what the GPU test uploads): pts [n, 3], the V times, per-point times [n], aabb,
    planes, cotangents [V, n, L C] and [n, L C]. Contains, as far as n allows: coordinates exactly -1, 0, +1 on every axis, coordinates
    beyond both faces, times beyond +-1, 320 points at distinct offsets inside one finest-level texel, n / 8 exact duplicates, a few `quiet`
    points whose cotangent rows are scaled by 2^-8, cotangent rows that are exactly zero, and points that are zero in every view."""
    _, C, base, mults, n, V, bound, layout = FIELD_CASES[FIELD_CASE_NAMES.index(name)]
    rng = np.random.default_rng(abs(hash_name(name)))
    L = len(mults)
    res = [[base[0] * m, base[1] * m, base[2] * m, base[3]] for m in mults]
    q = np.zeros((n, 3), dtype=np.int64)                                  # lattice numerators
    special = [tuple(int(round(v * LATTICE)) for v in s) for s in _SPECIAL] + [tuple(int(v) * LATTICE for v in s) for s in itertools.product((-1, 0, 1), repeat=3)]
    k = min(n, len(special))
    q[:k] = special[:k]
    crowd = 320 if n >= 2049 else 0
    if k < n:
        q[k:] = rng.integers(-LATTICE_MAX, LATTICE_MAX + 1, size=(n - k, 3))
    if crowd:                                                             # one finest-level texel per axis: the cell that holds coordinate 0.3
        lo_hi = []
        for a in range(3):
            r = res[-1][a]
            cell = math.floor((0.3 + 1) / 2 * (r - 1))
            lo, hi = math.ceil((2 * cell / (r - 1) - 1) * LATTICE), math.ceil((2 * (cell + 1) / (r - 1) - 1) * LATTICE)   # [lo, hi) in lattice steps
            lo_hi.append((lo + 1, hi))
        cells = np.array(list(itertools.product(*[range(lo, hi) for lo, hi in lo_hi])))
        q[k:k + crowd] = cells[rng.choice(len(cells), size=crowd, replace=False)]
    dup = n // 8
    if dup:
        q[n - dup:] = q[rng.integers(0, n - dup, size=dup)]
    if n > 64:
        q = q[rng.permutation(n)]
    pts = torch.tensor(q.astype(np.float64) / LATTICE * bound, dtype=torch.float32)
    times = tuple(_SPECIAL_T[:V]) if V > 1 else (1.25,)
    tq = rng.integers(-LATTICE_MAX, LATTICE_MAX + 1, size=(n,))
    tq[:min(n, 5)] = [int(v * LATTICE) for v in (-1, 0, 1.25, 1, -1.25)][:min(n, 5)]
    time_pp = torch.tensor(tq.astype(np.float64) / LATTICE, dtype=torch.float32)
    aabb = torch.tensor([[bound] * 3, [-bound] * 3], dtype=torch.float32)
    levels = []
    for r in res:
        lv = []
        for c0, c1 in COMBOS:
            p = torch.tensor(rng.uniform(-1.0, 1.0, size=(1, C, r[c1], r[c0])).astype(np.float32))
            lv.append(p.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else p.contiguous())
        levels.append(lv)
    cot = rng.normal(size=(V, n, L * C)).astype(np.float32)
    quiet = np.zeros(n, dtype=bool)
    quiet[rng.choice(n, size=max(1, n // 16), replace=False)] = True
    if n >= 27:                                                           # and so is every other point with a coordinate exactly on a face
        quiet |= (np.abs(q) == LATTICE).any(axis=1) & (np.arange(n) % 2 == 0)
    cot[:, quiet] *= 2.0 ** -8
    if n > 1:
        zero = (rng.random(size=(V, n)) < 0.3) | (rng.random(size=n) < 0.1)[None, :]
        zero[:, 0], zero[:, n - 1] = False, True                          # whatever n: point 0 is seen by every view, the last point by none
        cot[zero] = 0.0
    cot_pp = cot[0].copy()
    return types.SimpleNamespace(name=name, C=C, L=L, V=V, n=n, res=res, layout=layout, pts=pts, times=times, time_pp=time_pp, aabb=aabb, levels=levels,
                                 cot=torch.tensor(cot), cot_pp=torch.tensor(cot_pp), quiet=torch.tensor(quiet), q=q, bound=bound)


def hash_name(name):
    """a seed from the case name that does not depend on PYTHONHASHSEED"""
    h = 0
    for ch in name.encode():
        h = (h * 131 + ch) % (2 ** 31 - 1)
    return h


@functools.lru_cache(maxsize=None)
def field_case_reference(name, route):
    """fp64 reference of a case; route "single" (per-point times, cot_pp) or "views" (the V times, cot). Cached: one object serves every test."""
    d = field_case(name)
    if route == "single":
        return field_reference(d.pts, d.time_pp, d.aabb, d.levels, d.cot_pp, per_point=True)
    return field_reference(d.pts, d.times, d.aabb, d.levels, d.cot)


# ---- the MLP ---------------------------------------------------------------------------------------------------------------------------------
MLP_OUT_DIMS = (3, 3, 4)
MLP_ROWS = 192
MLP_SEEDS = {16: 5, 32: 0, 48: 1, 64: 4, 80: 18, 96: 5, 112: 9, 128: 1}  # the first seeds at which every pre-activation of the 192 rows is more than twice its own bar away from zero (asserted on the CPU)


def mlp_reference(x, params, dout=None, *, dtype=torch.float64, e_x=None, row_weight=None, c=C_MLP, defect=None):
    """The MLP of csrc/gs_mlp.h: h0 = x W0^T + b0, a = relu(h0), per head j: u = a W1^T + b1, v = relu(u), out_j = v W2^T + b2, out = (dx | ds | dr).
    params: W0, b0, then (W1, b1, W2, b2) per head. Every result with its propagated error unit `e_*` (module docstring); e_x: the unit of the
    input features (None: exact). With dout [n, 10]: dF and the 14 parameter gradients, rows weighted by row_weight (how often each row occurs)
    in the sums over rows. defect = dict(kind="scale_output", row=, column=, factor=): one output scaled."""
    T = dtype
    x = torch.as_tensor(x).to(T)
    P = [torch.as_tensor(p).detach().cpu().to(T) for p in params]
    W0, b0 = P[0], P[1]
    ex = torch.zeros_like(x) if e_x is None else torch.as_tensor(e_x).to(T)
    r = types.SimpleNamespace(u=[], e_u=[], v=[])
    r.h0 = x @ W0.t() + b0
    r.e_h0 = ex @ W0.abs().t() + c * (x.abs() @ W0.abs().t() + b0.abs())
    a = torch.relu(r.h0)
    outs, e_outs = [], []
    for j in range(3):
        W1, b1, W2, b2 = P[2 + 4 * j:6 + 4 * j]
        u = a @ W1.t() + b1
        e_u = r.e_h0 @ W1.abs().t() + c * (a @ W1.abs().t() + b1.abs())
        v = torch.relu(u)
        outs.append(v @ W2.t() + b2)
        e_outs.append(e_u @ W2.abs().t() + c * (v @ W2.abs().t() + b2.abs()))
        r.u.append(u); r.e_u.append(e_u); r.v.append(v)
    r.out, r.e_out = torch.cat(outs, -1), torch.cat(e_outs, -1)
    if defect is not None and defect["kind"] == "scale_output":
        r.out = r.out.clone()
        r.out[defect["row"], defect["column"]] *= defect["factor"]
    if dout is None:
        return r
    d = torch.as_tensor(dout).to(T)
    rw = torch.ones((x.shape[0], 1), dtype=T) if row_weight is None else torch.as_tensor(row_weight).to(T).reshape(-1, 1)
    grads, e_grads = [None] * 14, [None] * 14
    da, e_da = torch.zeros_like(a), torch.zeros_like(a)
    off = 0
    for j, o in enumerate(MLP_OUT_DIMS):
        W1, b1, W2, b2 = P[2 + 4 * j:6 + 4 * j]
        dj = d[:, off:off + o]
        off += o
        dw = dj * rw                                                   # the row's weight in every sum over rows
        grads[5 + 4 * j], e_grads[5 + 4 * j] = dw.sum(0), c * dw.abs().sum(0)
        grads[4 + 4 * j] = dw.t() @ r.v[j]
        e_grads[4 + 4 * j] = dw.abs().t() @ r.e_u[j] + c * (dw.abs().t() @ r.v[j])
        mask = (r.u[j] > 0).to(T)
        du, e_du = (dj @ W2) * mask, c * (dj.abs() @ W2.abs()) * mask
        grads[3 + 4 * j], e_grads[3 + 4 * j] = (du * rw).sum(0), (e_du * rw).sum(0) + c * (du.abs() * rw).sum(0)
        grads[2 + 4 * j] = (du * rw).t() @ a
        e_grads[2 + 4 * j] = (e_du * rw).t() @ a + (du.abs() * rw).t() @ r.e_h0 + c * ((du.abs() * rw).t() @ a)
        da = da + du @ W1
        e_da = e_da + e_du @ W1.abs() + c * (du.abs() @ W1.abs())
    mask0 = (r.h0 > 0).to(T)
    dh0, e_dh0 = da * mask0, e_da * mask0
    grads[1], e_grads[1] = (dh0 * rw).sum(0), (e_dh0 * rw).sum(0) + c * (dh0.abs() * rw).sum(0)
    grads[0] = (dh0 * rw).t() @ x
    e_grads[0] = (e_dh0 * rw).t() @ x.abs() + (dh0.abs() * rw).t() @ ex + c * ((dh0.abs() * rw).t() @ x.abs())
    r.dF, r.e_dF = dh0 @ W0, e_dh0 @ W0.abs() + c * (dh0.abs() @ W0.abs())
    r.grads, r.e_grads = grads, e_grads
    return r


def mlp_params(in_dim, seed):
    """Seeded fp32 weights. Every weight is non-zero: a dense background of size 2 / fan_in plus, per row, a few large entries (6 of 0.25..0.5 in
    W0, 4 of 0.2..0.4 in the W1) and biases of 0.05..0.4, so that the pre-activations spread over both signs -- every unit of h0 and most of the
    u_j are active for some of the 192 rows and idle for others -- while the rows of |W| stay short: the propagated unit remains a few c of the
    values, and a head output off by 1e-4 of itself is far outside its bar. The output biases (0.25..1) dominate the outputs."""
    g = torch.Generator().manual_seed(1000 * in_dim + seed)
    U = lambda *s: torch.rand(*s, generator=g) * 2 - 1

    def weight(o, i, k, big):
        w = U(o, i) * (2.0 / i)
        for r in range(o):
            cols = torch.randperm(i, generator=g)[:k]
            w[r, cols] = big * (0.5 + 0.5 * torch.rand(k, generator=g)) * torch.sign(U(k))
        return w

    bias = lambda k, lo, hi: (lo + (hi - lo) * torch.rand(k, generator=g)) * torch.sign(U(k))
    params = [weight(64, in_dim, 6, 0.5), bias(64, 0.05, 0.4)]
    for o in MLP_OUT_DIMS:
        params += [weight(64, 64, 4, 0.4), bias(64, 0.05, 0.3), U(o, 64) * (2.0 / 64), bias(o, 0.25, 1.0)]
    return [p.float().contiguous() for p in params], g


@functools.lru_cache(maxsize=None)
def mlp_case(in_dim):
    """params (14 fp32 tensors), x [192, in_dim] distinct feature rows, dout [192, 10], and the fp64 reference of the 192 rows."""
    params, g = mlp_params(in_dim, MLP_SEEDS[in_dim])
    x = (torch.rand(MLP_ROWS, in_dim, generator=g) * 2 - 1).float()
    dout = torch.randn(MLP_ROWS, 10, generator=g).float()
    return types.SimpleNamespace(in_dim=in_dim, params=params, x=x, dout=dout, ref=mlp_reference(x, params, dout))


def mlp_margin(ref):
    """min over the pre-activations h0 and u_j of |value| / e: > 1 means no ReLU mask can flip within the bar"""
    m = float((ref.h0.abs() / ref.e_h0).min())
    for u, e in zip(ref.u, ref.e_u):
        m = min(m, float((u.abs() / e).min()))
    return m


def mlp_reference_rows(case, n, listed=None):
    """fp64 reference of the batch that repeats the case's 192 rows cyclically up to n rows, from per-row results and repeat counts:
    out / dF / their units [n, ...] by indexing, the parameter gradients with row weights. listed (tensor of row indices): the cotangent of every
    other row is zero."""
    rows = torch.arange(n) % MLP_ROWS
    if listed is None:
        weight = torch.bincount(rows, minlength=MLP_ROWS).double()
        ref = mlp_reference(case.x, case.params, case.dout, row_weight=weight) if n != MLP_ROWS else case.ref
        return types.SimpleNamespace(out=ref.out[rows], e_out=ref.e_out[rows], dF=ref.dF[rows], e_dF=ref.e_dF[rows], grads=ref.grads, e_grads=ref.e_grads)
    keep = torch.zeros(n, dtype=torch.bool)
    keep[listed.long()] = True
    dout = case.dout[rows] * keep[:, None]
    ref = mlp_reference(case.x[rows], case.params, dout)
    return types.SimpleNamespace(out=ref.out, e_out=ref.e_out, dF=ref.dF, e_dF=ref.e_dF, grads=ref.grads, e_grads=ref.e_grads)


def mlp_ratios(got_out, got_dF, got_grads, ref, rows=None):
    r = {}
    sel = (lambda t: t) if rows is None else (lambda t: t[rows.long()])
    if got_out is not None:
        r["out"] = worst_ratio(sel(got_out.detach().cpu()), sel(ref.out), sel(ref.e_out))
    if got_dF is not None:
        r["dF"] = worst_ratio(sel(got_dF.detach().cpu()), sel(ref.dF), sel(ref.e_dF))
    if got_grads is not None:
        r["params"] = max(worst_ratio(g, w, e) for g, w, e in zip(got_grads, ref.grads, ref.e_grads))
    return r


def report(kernel, **figures):
    print("fp64-check", kernel, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))
