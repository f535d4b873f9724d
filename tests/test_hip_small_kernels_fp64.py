"""The small kernels that close every SLAM iteration -- the fused weighted L1 and SSIM losses, the Kabsch rotations, the ARAP and elastic
regularisers of the node graph, the edge-mask median and the fused Adam step (csrc/gs_loss.h, csrc/gs_map.h) -- against fp64 references
computed here on the CPU, at the smallest shapes that reach each code path: the second trip of a grid-stride loop, images smaller than
the SSIM window or one pixel into the next tile, rank-deficient cross-covariances, nodes without edges, heavy ties in the median,
exactly 32 and 33 Adam segments. tests/test_fp64_references.py pins the references themselves to the recorded reference outputs.

Every test prints the figures it bounds (`fp64-check ...` lines, visible with -s) before it asserts."""
import functools
import types

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)
import fp64_references as ref64

pytestmark = pytest.mark.gpu


def _report(kernel, **figures):
    print("fp64-check", kernel, " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in figures.items()))


def _within_rel_l1(got, want, tol):
    """sum |got - want| <= tol * sum |want| (rel-L1 without the division: an all-zero reference asks for an all-zero result);
    returns the ratio for the report."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    num, den = float((got - want).abs().sum()), float(want.abs().sum())
    return num <= tol * den, (num / den if den > 0 else num)


# ---- 1. weighted L1 -------------------------------------------------------------------------------------------------------------
L1_SHAPES = [(1, 1), (3, 5), (16, 16), (512, 513)]      # 512 x 513 = 262 656 pixels: threads 0..511 of block 0, 1 take a second loop trip
L1_VARIANTS = ["plain", "exposure", "weights_opacity", "backward_only"]
L1_ALPHA, L1_UPSTREAM = 0.9, 1.7
L1_THR = float(np.float32(0.95))                         # the threshold as the kernel holds it (fp32); the planted opacities equal it


@functools.lru_cache(maxsize=None)
def _l1_inputs(H, W):
    g = torch.Generator().manual_seed(1000 * H + W)
    N = H * W
    R = lambda *s: torch.rand(*s, generator=g)
    d = types.SimpleNamespace(image=R(3, H, W), depth=R(1, H, W), gt_image=R(3, H, W), gt_depth=R(1, H, W), opacity=0.8 + 0.2 * R(1, H, W),
                              w_rgb=torch.randint(0, 3, (1, H, W), generator=g).float(), w_depth=torch.randint(0, 3, (1, H, W), generator=g).float())
    p = torch.arange(N)
    d.same_rgb, d.same_depth, d.at_thr = (p % 5 == 2).view(1, H, W), (p % 7 == 3).view(1, H, W), (p % 11 == 4).view(1, H, W)
    d.image_planted = torch.where(d.same_rgb, d.gt_image, d.image)          # image == gt bitwise there (no-exposure variants only)
    d.depth = torch.where(d.same_depth, d.gt_depth, d.depth)
    d.opacity = torch.where(d.at_thr, torch.tensor(L1_THR), d.opacity)
    d.w_rgb[d.at_thr | d.same_rgb], d.w_depth[d.at_thr | d.same_depth] = 1.0, 2.0   # the planted pixels carry weight: their zeros are the kernel's
    d.w_rgb.view(-1)[0], d.w_depth.view(-1)[0] = 2.0, 1.0                           # (so does the only pixel of the 1 x 1 image)
    return d


@functools.lru_cache(maxsize=None)
def _l1_reference(H, W, variant):
    from oracle.loss_oracle import weighted_l1_loss_reference
    d = _l1_inputs(H, W)
    exposure = variant in ("exposure", "backward_only")
    weights = variant in ("weights_opacity", "backward_only")
    D = lambda t: t.double()
    image = D(d.image if exposure else d.image_planted).requires_grad_(True)
    depth = D(d.depth).requires_grad_(True)
    a = torch.tensor([0.05], dtype=torch.float32).double().requires_grad_(True) if exposure else None
    b = torch.tensor([-0.02], dtype=torch.float32).double().requires_grad_(True) if exposure else None
    kw = dict(w_rgb=D(d.w_rgb), w_depth=D(d.w_depth), opacity=D(d.opacity), opacity_depth_threshold=L1_THR) if weights else {}
    loss = weighted_l1_loss_reference(image, depth, D(d.gt_image), D(d.gt_depth), exposure_a=a, exposure_b=b, alpha=L1_ALPHA, **kw)
    (loss * L1_UPSTREAM).backward()
    r = types.SimpleNamespace(exposure=exposure, weights=weights, value=float(loss.detach()), g_image=image.grad, g_depth=depth.grad)
    with torch.no_grad():
        ea = torch.exp(a) if exposure else torch.ones(1, dtype=torch.float64)
        r.res_rgb = ea * image + (b if exposure else 0.0) - D(d.gt_image)
        r.res_depth = depth - D(d.gt_depth)
        r.ea, r.image64 = float(ea), image.detach()
        r.g_a = float(a.grad) if exposure else None
        r.g_b = float(b.grad) if exposure else None
    return r


@pytest.mark.parametrize("route", ["cpp_node", "python_node"])
@pytest.mark.parametrize("variant", L1_VARIANTS)
@pytest.mark.parametrize("H,W", L1_SHAPES)
def test_weighted_l1_matches_fp64(H, W, variant, route):
    import slam_losses
    from diff_gaussian_rasterization import _C
    if route == "cpp_node" and (_C._glue is None or not hasattr(_C._glue, "weighted_l1_autograd")):
        pytest.skip("native glue not built")
    d, ref = _l1_inputs(H, W), _l1_reference(H, W, variant)
    cu = lambda t: t.cuda()

    def run():
        image = cu(d.image if ref.exposure else d.image_planted).requires_grad_(True)
        depth = cu(d.depth).requires_grad_(True)
        kw = {}
        if ref.exposure:
            kw.update(exposure_a=torch.tensor([0.05], device="cuda", requires_grad=True), exposure_b=torch.tensor([-0.02], device="cuda", requires_grad=True))
        if ref.weights:
            kw.update(w_rgb=cu(d.w_rgb), w_depth=cu(d.w_depth), opacity=cu(d.opacity), opacity_depth_threshold=0.95)
        loss = slam_losses.weighted_l1_loss(image, depth, cu(d.gt_image), cu(d.gt_depth), alpha=L1_ALPHA, compute_value=variant != "backward_only", **kw)
        (loss * L1_UPSTREAM).backward()
        out = [loss.detach().cpu(), image.grad.cpu(), depth.grad.cpu()]
        return out + ([kw["exposure_a"].grad.cpu(), kw["exposure_b"].grad.cpu()] if ref.exposure else [])

    slam_losses._NATIVE_NODE = route == "cpp_node"
    try:
        first, again = run(), run()
    finally:
        slam_losses._NATIVE_NODE = True
    assert len(first) == len(again) and all(torch.equal(x, y) for x, y in zip(first, again))          # fixed summation order: identical bits
    value, g_image, g_depth = float(first[0]), first[1].double(), first[2].double()

    if variant == "backward_only":
        assert value == 0.0                                                     # the defined placeholder, not the loss
        value_err = 0.0
    else:
        value_err = abs(value - ref.value) / abs(ref.value)
    # elements whose fp64 residual is below 1e-5 and not planted: the fp32 sign is not determined there
    planted_rgb = (d.same_rgb.expand(3, H, W) if not ref.exposure else torch.zeros(3, H, W, dtype=torch.bool))
    loose_rgb = (ref.res_rgb.abs() < 1e-5) & ~planted_rgb
    loose_depth = (ref.res_depth.abs() < 1e-5) & ~d.same_depth
    share = float(loose_rgb.sum() + loose_depth.sum()) / (4 * H * W)
    ok_i, err_i = _within_rel_l1(g_image[~loose_rgb], ref.g_image[~loose_rgb], 2e-5)
    ok_d, err_d = _within_rel_l1(g_depth[~loose_depth], ref.g_depth[~loose_depth], 2e-5)
    _report("weighted_l1", shape=f"{H}x{W}", variant=variant, route=route, value_rel=value_err, g_image_rel_l1=err_i, g_depth_rel_l1=err_d, loose_share=share)
    assert value_err <= 2e-5
    assert share <= 1e-4
    assert ok_i and ok_d
    # there the result is one of -m, 0, +m, m the magnitude every sign gives
    coef = L1_UPSTREAM * L1_ALPHA / (3 * H * W) * ref.ea * ((d.w_rgb * d.opacity).double() if ref.weights else torch.ones(1, H, W, dtype=torch.float64))
    mag = coef.expand(3, H, W)[loose_rgb]
    assert bool(((g_image[loose_rgb].abs() - mag).abs() <= 1e-5 * mag).logical_or(g_image[loose_rgb] == 0).all())
    # exact zeros where the residual is exactly zero, and where the opacity only EQUALS the threshold (the comparison is strict)
    if not ref.exposure:
        assert bool((g_image[planted_rgb] == 0).all()) and bool((ref.g_image[planted_rgb] == 0).all())
    assert bool((g_depth[d.same_depth] == 0).all()) and bool((ref.g_depth[d.same_depth] == 0).all())
    if ref.weights:
        assert bool((g_depth[d.at_thr] == 0).all()) and bool((ref.g_depth[d.at_thr] == 0).all())
        above = (d.opacity > L1_THR) & (d.w_depth > 0) & ~d.same_depth & ~loose_depth
        assert bool((g_depth[above] != 0).all())
    if ref.exposure:
        # |got - ref| <= 2e-6 * sum |terms|: the sums' natural unit. Where the sign is not determined the reference takes the kernel's own
        # element (bounded above), so that this bound is about the two-level sum alone.
        gi = torch.where(loose_rgb, g_image, ref.g_image)
        terms_a, terms_b = gi * ref.image64, gi / ref.ea
        want_a, want_b = float(terms_a.sum()), float(terms_b.sum())
        if not bool(loose_rgb.any()):
            assert abs(want_a - ref.g_a) <= 1e-12 * float(terms_a.abs().sum()) and abs(want_b - ref.g_b) <= 1e-12 * float(terms_b.abs().sum())
        assert float(terms_a.abs().sum()) > 0 and float(terms_b.abs().sum()) > 0
        err_a = abs(float(first[3]) - want_a) / float(terms_a.abs().sum())
        err_b = abs(float(first[4]) - want_b) / float(terms_b.abs().sum())
        _report("weighted_l1_exposure", shape=f"{H}x{W}", variant=variant, route=route, g_a_over_terms=err_a, g_b_over_terms=err_b)
        assert err_a <= 2e-6 and err_b <= 2e-6


# ---- 2. SSIM ----------------------------------------------------------------------------------------------------------------------
SSIM_SHAPES = [(3, 5, 7), (1, 16, 16), (3, 17, 33), (3, 1, 40)]     # below the 11-wide window; one tile; one pixel into the next tiles; one row
SSIM_CASES = ["rand", "same", "const", "const2", "rand_mask70", "rand_mask0"]
SSIM_ZERO_GRADIENT = ("same", "const", "rand_mask0")


@functools.lru_cache(maxsize=None)
def _ssim_case(shape, case):
    from oracle.loss_oracle import ssim_reference
    C, H, W = shape
    g = torch.Generator().manual_seed(100 * H + W)
    img1 = torch.rand(C, H, W, generator=g)
    img2 = (img1 + 0.1 * torch.randn(C, H, W, generator=g)).clamp(0.0, 1.0)
    mask = None
    if case == "same":
        img2 = img1.clone()
    elif case == "const":
        img1, img2 = torch.full((C, H, W), 0.7), torch.full((C, H, W), 0.7)
    elif case == "const2":
        img1, img2 = torch.full((C, H, W), 1.0), torch.full((C, H, W), 0.25)
    elif case == "rand_mask70":
        mask = torch.rand(H, W, generator=g) < 0.7
    elif case == "rand_mask0":
        mask = torch.zeros(H, W, dtype=torch.bool)
    out = types.SimpleNamespace(img1=img1, img2=img2, mask=mask)
    for name, dtype in (("64", torch.float64), ("32", torch.float32)):      # the fp64 reference and its fp32 restatement, both on the CPU
        x = img1.to(dtype).clone().requires_grad_(True)
        v = ssim_reference(x, img2.to(dtype), mask)
        v.backward()
        setattr(out, "v" + name, float(v.detach()))
        setattr(out, "g" + name, x.grad.double())
    return out


@pytest.mark.parametrize("case", SSIM_CASES)
@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_matches_fp64(shape, case):
    from slam_losses import ssim
    c = _ssim_case(shape, case)
    img1 = c.img1.cuda().requires_grad_(True)
    v = ssim(img1, c.img2.cuda(), mask=None if c.mask is None else c.mask.cuda())
    v.backward()
    g = img1.grad.double().cpu()
    v = v.detach()
    err, err32 = abs(float(v) - c.v64), abs(c.v32 - c.v64)
    _report("ssim", shape=shape, case=case, value_err=err, value_err_fp32_cpu=err32)
    assert err <= max(4 * err32, 2e-6)
    if case in SSIM_ZERO_GRADIENT:
        scale = float(_ssim_case(shape, "rand").g64.abs().max())
        _report("ssim", shape=shape, case=case, g_max_over_rand_scale=float(g.abs().max()) / scale,
                g_fp32_cpu_over_rand_scale=float(c.g32.abs().max()) / scale)
        assert float(c.g64.abs().max()) <= 1e-9 * scale                         # zero in fp64
        assert float(g.abs().max()) <= 1e-3 * scale
        if case == "rand_mask0":
            assert float(g.abs().max()) == 0.0 and abs(float(v) - 1.0) <= 2e-6
    else:
        rel = lambda t: float((t - c.g64).abs().sum() / c.g64.abs().sum())
        _report("ssim", shape=shape, case=case, g_rel_l1=rel(g), g_rel_l1_fp32_cpu=rel(c.g32))
        assert rel(g) <= max(4 * rel(c.g32), 2e-5)
        if c.mask is not None:
            assert float(g[:, ~c.mask].abs().max()) == 0.0                      # the mask masks the gradient


# ---- 3. Kabsch rotations ---------------------------------------------------------------------------------------------------------------
def _random_rotations(n, g):
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1))[:, None, :]
    return q * torch.det(q)[:, None, None]                                      # det +1


KABSCH_CASES = {   # name: (sigma, reflect, scale, unique answer)
    "full": ((3.0, 2.0, 1.0), False, 1.0, True), "reflection": ((3.0, 2.0, 1.0), True, 1.0, True),
    "planar": ((3.0, 2.0, 0.0), False, 1.0, True), "collinear": ((3.0, 0.0, 0.0), False, 1.0, False),
    "tied_top": ((2.0, 2.0, 1.0), False, 1.0, True), "tied_top_reflection": ((2.0, 2.0, 1.0), True, 1.0, True),
    "tied_bottom": ((3.0, 1.0, 1.0), False, 1.0, True), "tied_bottom_reflection": ((3.0, 1.0, 1.0), True, 1.0, False),
    "full_tiny": ((3.0, 2.0, 1.0), False, 2.0 ** -40, True), "reflection_tiny": ((3.0, 2.0, 1.0), True, 2.0 ** -40, True),
    "full_huge": ((3.0, 2.0, 1.0), False, 2.0 ** 40, True), "reflection_huge": ((3.0, 2.0, 1.0), True, 2.0 ** 40, True),
}


def _kabsch_inputs(name, n):
    """S = U diag(sigma) V^T in fp64 from random rotations (one column of U negated for a reflection), rounded to fp32; the scaled cases
    are the unscaled matrices times a power of two."""
    sigma, reflect, scale, _ = KABSCH_CASES[name]
    g = torch.Generator().manual_seed(17 * n + (1 if reflect else 0))
    U, V = _random_rotations(n, g), _random_rotations(n, g)
    if reflect:
        U = U.clone()
        U[:, :, 1] *= -1
    S = U @ torch.diag(torch.tensor(sigma, dtype=torch.float64)) @ V.transpose(-1, -2)
    return S.float() * scale


def _check_rotations(name, S32, R, unique):
    S64, R64 = S32.double(), R.double().cpu()
    n = S64.shape[0]
    eye = torch.eye(3, dtype=torch.float64).expand(n, 3, 3)
    orth = float((R64 @ R64.transpose(-1, -2) - eye).abs().max()) if n else 0.0
    det = float((torch.det(R64) - 1).abs().max()) if n else 0.0
    sv = torch.linalg.svdvals(S64)                                              # of the matrix the kernel sees, descending
    best = sv[:, 0] + sv[:, 1] + torch.sign(torch.det(S64)) * sv[:, 2]          # max of tr(R S) over proper rotations
    short = float(((best - torch.einsum("nab,nba->n", R64, S64)) / sv[:, 0]).max()) if n else 0.0
    _report("kabsch", case=name, n=n, orthonormality=orth, det_minus_1=det, trace_shortfall_over_sigma1=short)
    assert orth <= 1e-5 and det <= 1e-5 and short <= 1e-5
    if unique and n:
        diff = float((R64 - ref64.svd_rotations64(S64)).abs().max())
        _report("kabsch", case=name, n=n, against_fp64_svd=diff)
        assert diff <= 2e-5


@pytest.mark.parametrize("n", [1, 63, 64, 65, 0])
@pytest.mark.parametrize("name", list(KABSCH_CASES))
def test_kabsch_rotations_match_the_fp64_svd_rule(name, n):
    from slam.deform_model import kabsch_rotations
    S = _kabsch_inputs(name, n)
    R = kabsch_rotations(S.cuda())
    assert R.shape == (n, 3, 3) and R.dtype == torch.float32
    _check_rotations(name, S, R, KABSCH_CASES[name][3])
    scale = KABSCH_CASES[name][2]
    if scale != 1.0 and n:
        plain = kabsch_rotations((S / scale).cuda())                            # (exact: a power of two)
        diff = float((R - plain).abs().max())
        _report("kabsch", case=name, n=n, scaled_against_unscaled=diff)
        assert diff <= 1e-6


def test_kabsch_rotations_of_exactly_rank_deficient_matrices():
    """Integer outer products are exact in fp32: exactly rank one (the 'any orthogonal vector' branch, with and without zero components in
    the singular vector) and exactly rank two (the Gram-Schmidt branch with an exactly zero third singular value)."""
    from slam.deform_model import kabsch_rotations
    a = torch.tensor([[1, 2, 2], [0, 0, 3], [0, 4, 3], [2, -1, 2], [1, 1, 1], [5, 0, 0]], dtype=torch.float64)
    b = torch.tensor([[2, -1, 2], [0, 1, 0], [1, 0, 0], [0, 0, -7], [1, -2, 3], [0, 0, 2]], dtype=torch.float64)
    rank1 = a[:, :, None] * b[:, None, :]
    rank2 = rank1 + torch.roll(a, 1, 0)[:, :, None] * torch.roll(b, 1, 0)[:, None, :]
    sv = torch.linalg.svdvals(rank2)
    assert float((sv[:, 1] / sv[:, 0]).min()) > 1e-2 and float((sv[:, 2] / sv[:, 0]).max()) < 1e-14
    for name, S, unique in (("exact_rank1", rank1, False), ("exact_rank2", rank2, True)):
        assert torch.equal(S.float().double(), S)
        _check_rotations(name, S.float(), kabsch_rotations(S.float().cuda()), unique)


# ---- 4. ARAP ------------------------------------------------------------------------------------------------------------------------------
def _grid(t):
    return torch.round(t * 1024.0) / 1024.0                                    # values whose sums and differences are exact in fp32


@functools.lru_cache(maxsize=None)
def _arap_case(V, T, M, K):
    """Rest pose plus, per (view, sample), a rotation of up to ~0.3 rad about the origin and 0.02 of noise; random neighbour sets without self
    loops. Planted: node M // 2 of view 0 keeps no edge (and is nobody's neighbour); view 1 at its last sample is the rest pose translated
    rigidly, on a grid where that is exact; view 2 lies in the plane z = 1/4 and moves in it."""
    g = torch.Generator().manual_seed(7 * M + K)
    base = _grid(torch.randn(M, 3, generator=g) * 0.3)
    axis_angle = torch.randn(V, T, 3, generator=g) * 0.17
    seq = torch.empty(V, T, M, 3)
    for v in range(V):
        for t in range(T):
            w = axis_angle[v, t]
            Wx = torch.tensor([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            seq[v, t] = base @ torch.linalg.matrix_exp(Wx).T + 0.02 * torch.randn(M, 3, generator=g)
    nn_idx = torch.zeros(V, M, K, dtype=torch.int64)
    if M > 1:
        for v in range(V):
            for m in range(M):
                others = torch.randperm(M - 1, generator=g)[:K] if M - 1 >= K else torch.randint(0, M - 1, (K,), generator=g)
                nn_idx[v, m] = (m + 1 + others) % M
    keep = torch.rand(V, M, K, generator=g) < 0.7
    keep[:, :, :2] = True                                                       # two edges at least: the fit is determined
    planted = torch.zeros(V, T - 1, M, dtype=torch.bool)                        # (view, sample, node) whose S the rule zeroes or that has no edge
    lonely = M // 2
    if M > 1:
        keep[0, lonely] = False
        hit = nn_idx[0] == lonely
        nn_idx[0][hit] = (lonely + 1) % M
        assert M > K + 2
        nn_idx[0, (lonely + 1) % M] = (lonely + 2 + torch.arange(K)) % M        # (the replacement made a self loop there)
        assert not bool((nn_idx[0] == lonely).any()) and not bool((nn_idx[0] == torch.arange(M)[:, None]).any())
        planted[0, :, lonely] = True
    else:
        planted[:] = True                                                       # one node: its only possible neighbour is itself, every edge is 0
    if V > 1:
        seq[1, 0] = base
        seq[1, T - 1] = base + torch.tensor([3.0 / 64, -5.0 / 128, 1.0 / 32])
        planted[1, T - 2] = True
    if V > 2:
        seq[2, :, :, 2] = 0.25
        planted[2] = True
    return seq, nn_idx, keep, planted


@pytest.mark.parametrize("V,T,M,K", [(1, 2, 1, 1), (2, 2, 65, 3), (3, 4, 130, 10)])
def test_arap_matches_the_fp64_program(V, T, M, K, monkeypatch):
    from slam import deform_model as dm
    seq, nn_idx, keep, planted = _arap_case(V, T, M, K)
    cot = torch.tensor([1.0, 0.5, 2.0])[:V]
    # fp64 side: value, gradient, and the conditioning of every fit that is not planted
    s64 = seq.double().requires_grad_(True)
    want = ref64.arap_reference64(s64, nn_idx, keep)
    (want * cot.double()).sum().backward()
    with torch.no_grad():
        S, unchanged = ref64.arap_covariances64(ref64.arap_edges64(s64.detach(), nn_idx, keep), keep)
    assert torch.equal(unchanged | ~keep.any(-1)[:, None, :], planted)          # the rule fires exactly where it was planted
    if not bool(planted.all()):
        sv = torch.linalg.svdvals(S[~planted])
        gap = float((torch.minimum(sv[:, 0] - sv[:, 1], sv[:, 1] - sv[:, 2]) / sv[:, 0]).min())
        _report("arap", shape=(V, T, M, K), smallest_singular_value_gap_over_sigma1=gap)
        assert gap >= 1e-3                                                      # otherwise R is ill-conditioned in the reference itself
    # device side, through the fused kernels
    calls = []
    real = dm._ArapTerm

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(1)
            return real.apply(*a)
    monkeypatch.setattr(dm, "_ArapTerm", Spy)
    d = seq.cuda().requires_grad_(True)
    got = dm.arap_error(d, nn_idx.cuda(), keep.cuda())
    (got * cot.cuda()).sum().backward()
    assert calls == [1]
    value_err = float(((got.detach().cpu().double() - want.detach()).abs() / want.detach().abs().clamp_min(1e-300)).max())
    ok, g_err = _within_rel_l1(d.grad, s64.grad, 2e-4)
    _report("arap", shape=(V, T, M, K), value_rel=value_err, grad_rel_l1=g_err)
    assert bool(((got.detach().cpu().double() - want.detach()).abs() <= 2e-4 * want.detach().abs()).all())
    assert ok
    if M > 1:
        lonely = M // 2                                                         # no kept edge, nobody's neighbour: no gradient at all
        assert float(d.grad[0, :, lonely].abs().max()) == 0.0 and float(s64.grad[0, :, lonely].abs().max()) == 0.0
        # its partial is 0, and R = I wherever S was zeroed (seen through the kernel's own forward outputs)
        nb = torch.gather(d.detach(), 2, nn_idx.cuda()[:, None, :, :, None].expand(V, T, M, K, 3).reshape(V, T, M * K, 3)).reshape(V, T, M, K, 3)
        ctx = types.SimpleNamespace(save_for_backward=lambda *t: setattr(ctx, "saved", t))
        partial = real.forward(ctx, d.detach(), nb, keep.cuda().float())
        assert float(partial[0, :, lonely].abs().max()) == 0.0
        R = ctx.saved[3].view(V, T - 1, M, 3, 3)[planted.cuda()]
        assert torch.equal(R, torch.eye(3, device="cuda").expand_as(R))
    else:
        assert float(got.detach().abs().max()) == 0.0 and float(d.grad.abs().max()) == 0.0


# ---- 5. elastic --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _elastic_case(T, K, M):
    """Two views of M nodes over T samples. Planted (M >= 4): in view 0 the first neighbour of node 0 coincides with it at one sample (edge
    length 0); in both views the last neighbour of node 1 keeps the exact offset (1/4, 0, 0) (constant length, variance exactly 0)."""
    g = torch.Generator().manual_seed(1000 * T + 10 * M + K)
    V = 2
    nodes_t = torch.randn(M, 1, 3, generator=g) * 0.3 + 0.02 * torch.randn(V, M, T, 3, generator=g)
    nn_idx = torch.zeros(M, K, dtype=torch.int64)
    if M > 1:
        for m in range(M):
            nn_idx[m] = (m + 1 + torch.randperm(M - 1, generator=g)[:K]) % M
    weights = torch.rand(M, K, generator=g)
    if M >= 4:
        nn_idx[0, 0], nn_idx[1, K - 1] = 2, 3
        nodes_t[0, 2, T // 2] = nodes_t[0, 0, T // 2]
        nodes_t[:, 1] = _grid(nodes_t[:, 1])
        nodes_t[:, 3] = nodes_t[:, 1] + torch.tensor([0.25, 0.0, 0.0])
    return nodes_t, nn_idx, weights


@pytest.mark.parametrize("M", [1, 65, 200])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("T", [2, 3, 16, 17])
def test_elastic_matches_the_fp64_program(T, K, M, monkeypatch):
    """T = 2 .. 16 through the fused kernels; T = 17 is past their limit and must take the tensor program, with the same value."""
    from slam import deform_model as dm
    nodes_t, nn_idx, weights = _elastic_case(T, K, M)
    cot = torch.tensor([1.0, 0.5])
    x64, w64 = nodes_t.double().requires_grad_(True), weights.double().requires_grad_(True)
    want = ref64.elastic_reference64(x64, w64, nn_idx)
    (want * cot.double()).sum().backward()
    calls = []
    real = dm._ElasticRatio

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(1)
            return real.apply(*a)
    monkeypatch.setattr(dm, "_ElasticRatio", Spy)
    x, w = nodes_t.cuda().requires_grad_(True), weights.cuda().requires_grad_(True)
    got = dm.elastic_error(x, w, nn_idx.cuda())
    (got * cot.cuda()).sum().backward()
    assert calls == ([1] if T <= 16 else [])
    diff = (got.detach().cpu().double() - want.detach()).abs()
    ok_x, err_x = _within_rel_l1(x.grad, x64.grad, 2e-4)
    ok_w, err_w = _within_rel_l1(w.grad, w64.grad, 2e-4)
    _report("elastic", shape=(T, K, M), route="fused" if calls else "tensor program",
            value_rel=float((diff / want.detach().abs().clamp_min(1e-300)).max()), grad_rel_l1=err_x, grad_weights_rel_l1=err_w)
    assert bool((diff <= 2e-4 * want.detach().abs()).all())
    assert ok_x and ok_w
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(x64.grad).all())       # the zero-length edge: gradient 0 there, not 0/0
    if M >= 4:
        assert float(w64.grad[1, K - 1]) == 0.0 and float(w.grad[1, K - 1]) == 0.0            # the constant edge: ratio exactly 0
    if M == 1:
        assert float(got.detach().abs().max()) == 0.0 and float(x.grad.abs().max()) == 0.0


# ---- 6. edge-mask median ---------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [(2, 2), (16, 16), (17, 33), (65, 1024)]                          # 65 x 1024 = 66 560 > 64 blocks x 1024: a second trip of the select loop
EDGE_INPUTS = ["smooth", "constant", "mostly_invalid", "two_halves", "stripes"]
EDGE_THRESHOLD = 1.1


def _edge_image(kind, H, W):
    g = torch.Generator().manual_seed(3 * H + W)
    if kind == "constant":
        return torch.full((3, H, W), 0.4)
    if kind == "two_halves":                                                   # two or three distinct intensities: massive ties
        img = torch.full((3, H, W), 0.25)
        img[:, :, W // 2:] = 0.75
        return img
    if kind == "stripes":                                                      # two columns of 1/4, two of 3/4, ...: most pixels share ONE
        return (0.25 + 0.5 * ((torch.arange(W) // 2) % 2).float()).expand(3, H, W).contiguous()   # non-zero intensity, the median among them
    img = 0.1 + 0.8 * torch.rand(3, H, W, generator=g)                          # (every grey value well above the validity eps of 0.01)
    img = torch.nn.functional.avg_pool2d(img[None], 3, stride=1, padding=1, count_include_pad=False)[0].contiguous()
    if kind == "mostly_invalid":
        img[:, : (3 * H + 3) // 5] = 0.0                                        # more than half of the pixels have an invalid tap
    return img


@pytest.mark.parametrize("kind", EDGE_INPUTS)
@pytest.mark.parametrize("H,W", EDGE_SIZES)
def test_edge_mask_intensity_median_and_mask(H, W, kind):
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    img = _edge_image(kind, H, W)
    want = ref64.edge_intensity64(img)
    dev = img.cuda()
    results = []
    for _ in range(2):                                                          # twice in a row: the select's state must be clean again
        intensity = torch.full((H * W,), -1.0, device="cuda")
        median = torch.full((1,), -1.0, device="cuda")
        mask = torch.full((H * W,), 7, dtype=torch.uint8, device="cuda")
        rc = lib.gsr_edge_mask(dev.data_ptr(), H, W, EDGE_THRESHOLD, 0.01, intensity.data_ptr(), median.data_ptr(), mask.data_ptr(), _C._stream(dev.device))
        assert rc == 0
        results.append((intensity.cpu(), median.cpu(), mask.cpu()))
    intensity, median, mask = results[0]
    err = float((intensity.double().view(H, W) - want).abs().max()) / (float(want.max()) or 1.0)     # (absolute where the reference is all zero)
    rank = int((intensity < median).sum()), int((intensity <= median).sum())
    _report("edge_mask", size=f"{H}x{W}", input=kind, intensity_err_over_max=err, median=float(median), below=rank[0], not_above=rank[1], k=(H * W - 1) // 2)
    if kind == "constant":
        assert float(want.abs().max()) == 0.0 and float(intensity.abs().max()) == 0.0
    else:
        assert err <= 1e-5
    if kind == "mostly_invalid":
        assert int((want == 0).sum()) > H * W // 2 and float(median) == 0.0
    if kind in ("two_halves", "stripes"):
        assert len(torch.unique(intensity)) <= 3
    if kind == "stripes" and W > 2:
        assert float(median) == 0.5 and int((intensity == median).sum()) > H * W // 2
    assert torch.equal(median, torch.median(intensity).view(1))                 # the exact lower median of the kernel's own intensities, bit for bit
    assert torch.equal(mask, (intensity > median * torch.tensor(EDGE_THRESHOLD)).to(torch.uint8))
    assert all(torch.equal(a, b) for a, b in zip(results[0], results[1]))


# ---- 7. Adam ---------------------------------------------------------------------------------------------------------------------------------
def _adam_params(n, dev):
    g = torch.Generator().manual_seed(n)
    sizes = [(1, 255, 256, 257, 1000)[k % 5] for k in range(n)]
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in sizes]


@pytest.mark.parametrize("n", [32, 33])
def test_fused_adam_at_its_segment_limit_and_past_it(n, monkeypatch):
    """32 tensors of 1 / 255 / 256 / 257 / 1000 elements: one fused launch (asserted); 33: torch's own step. Five steps against
    torch.optim.Adam on the CPU, then one more at step count 100 001 (the bias corrections at large t)."""
    import fused_adam
    ref_p, dev_p = _adam_params(n, "cpu"), _adam_params(n, "cuda")
    groups = lambda ps: [{"params": [p], "lr": (1.6e-4, 2.5e-3, 0.05)[k % 3]} for k, p in enumerate(ps)]     # the model's learning rates
    ref = torch.optim.Adam(groups(ref_p), lr=0.0, eps=1e-15)
    opt = fused_adam.FusedAdam(groups(dev_p), lr=0.0, eps=1e-15)
    torch_steps, fused_steps = [], []
    real_step = torch.optim.Adam.step
    monkeypatch.setattr(torch.optim.Adam, "step", lambda self, *a, **k: (torch_steps.append(type(self).__name__), real_step(self, *a, **k))[1])
    lib = fused_adam._C.load_library()

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        @staticmethod
        def gsr_adam_step(*a):
            fused_steps.append(a[0])
            return lib.gsr_adam_step(*a)
    monkeypatch.setattr(fused_adam._C, "load_library", lambda: Spy())
    gen = torch.Generator().manual_seed(4)
    worst = {"param": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}

    def step_and_check(it):
        for pr, pf in zip(ref_p, dev_p):
            gr = torch.randn(pr.shape, generator=gen) * (10.0 ** (-(it % 4)))
            pr.grad, pf.grad = gr.clone(), gr.cuda()
        ref.step()
        opt.step()
        for k, (pr, pf) in enumerate(zip(ref_p, dev_p)):
            pairs = (("param", pf.detach().cpu(), pr.detach(), 1e-7), ("exp_avg", opt.state[pf]["exp_avg"].cpu(), ref.state[pr]["exp_avg"], 1e-12),
                     ("exp_avg_sq", opt.state[pf]["exp_avg_sq"].cpu(), ref.state[pr]["exp_avg_sq"], 1e-20))
            for name, a, b, atol in pairs:
                worst[name] = max(worst[name], float(((a - b).abs() / (b.abs().clamp_min(1e-30) if name != "param" else 1.0)).max()))
                assert torch.allclose(a, b, rtol=2e-6, atol=atol), (it, k, name)
            assert float(opt.state[pf]["step"]) == float(ref.state[pr]["step"])

    for it in range(5):
        step_and_check(it)
    for o, ps in ((ref, ref_p), (opt, dev_p)):
        for p in ps:
            o.state[p]["step"].fill_(100000.0)
    step_and_check(5)
    assert float(ref.state[ref_p[0]]["step"]) == 100001.0
    _report("adam", tensors=n, **{k + ("_max_abs" if k == "param" else "_max_rel"): v for k, v in worst.items()})
    assert torch_steps.count("Adam") == 6
    if n == 32:
        assert fused_steps == [32] * 6 and "FusedAdam" not in torch_steps       # the fused path, every step
    else:
        assert fused_steps == [] and torch_steps.count("FusedAdam") == 6        # the torch fallback
