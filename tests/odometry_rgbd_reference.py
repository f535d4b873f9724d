"""numpy restatement of gsr_odometry_align_rgbd (include/visual_odometry.h): one pass with the affine brightness and the inverse-depth term,
the full fit and the gate in float64 on the float32 pyramid of tests/odometry_reference.py, and the scene the tests align: three planes seen
from two poses, both images and both depths from exact ray-plane intersection, optionally without texture, with a gain and an offset on the
current image, with depth holes and masks. Needs neither a GPU nor the library."""
import numpy as np

from odometry_reference import (F32, MIN_Z, PLANTED_SIZES, PLANTED_XI, intrinsics, level_intrinsics, planted_motion, pyramid, rotation_angle,
                                se3_exp, texture)

TAIL = 6                                     # sum w_I, sum w_I r_I^2, n_I, sum w_D, sum w_D r_D^2, n_D
ROW = 64
MIN_PIVOT = 1e-6
# n . X = d in the previous camera's frame; every ray takes its nearest positive hit
PLANES = np.array([[0.15, 0.1, 1.0, 2.0], [1.0, 0.05, 0.35, 1.1], [0.05, 1.0, 0.3, 0.9]])
FLAT_COLOUR = 0.5
TERMS = dict(edge_ratio=0.05, sigma_depth_init=0.02, sigma_depth_min=1e-4, max_gain=0.5, max_offset=0.3)
GATE = dict(nu=5.0, sigma_init=0.1, sigma_min=1e-3, min_share=0.3, max_last_step=1e-2, max_translation=1.0, max_rotation=np.deg2rad(30.0))


def sizes(n):
    """(unknowns, entries of H's upper triangle, sums of a pass)."""
    return n, n * (n + 1) // 2, n * (n + 1) // 2 + n + TAIL


# ---- the scene --------------------------------------------------------------------------------------------------------------------------------
def _hit(origin, direction):
    """The nearest positive hit of every ray origin + s direction with PLANES: the points [.., 3] and s."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (PLANES[:, 3] - PLANES[:, :3] @ origin) / (direction @ PLANES[:, :3].T)
    s = np.where(s > 0, s, np.inf).min(axis=-1)
    return origin + direction * s[..., None], s


def scene(W, H, s=1.0, flat=False, gain=1.0, offset=0.0, T=None):
    """image_prev [3, H, W], depth_prev [H, W], image_cur, depth_cur (float32), K, T_true (previous camera -> current camera). flat: both
    images one colour. The current image is gain * image + offset."""
    fx, fy, cx, cy = K = intrinsics(W, H)
    T = planted_motion(s) if T is None else np.asarray(T, np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    colour = lambda p: np.full(p.shape[:-1], FLAT_COLOUR) if flat else texture(p[..., 0] + 0.7 * p[..., 2], p[..., 1] - 0.4 * p[..., 2])
    point, z_prev = _hit(np.zeros(3), ray)                          # the rays have z = 1: the step is the depth
    prev = colour(point)
    R, t = T[:3, :3], T[:3, 3]
    point, z_cur = _hit(-R.T @ t, ray @ R)
    cur = gain * colour(point) + offset
    as_rgb = lambda g: np.ascontiguousarray(np.broadcast_to(g.astype(F32)[None], (3, H, W)))
    return as_rgb(prev), z_prev.astype(F32), as_rgb(cur), z_cur.astype(F32), K, T


# ---- one pass -------------------------------------------------------------------------------------------------------------------------------------
def one_pass(P_I, P_D, C_I, C_D, K_level, T, sigma_i, sigma_d, alpha=0.0, beta=0.0, affine=True, weight=1.0, edge_ratio=0.05, nu=5.0,
             dtype=np.float64):
    """The sums of one pass. Returns sums [NS] (H's upper triangle row-major, g, the six of TAIL), scale [NS] and the flip margins.
    scale: the sum of the absolute values of a sum's per-pixel terms (both terms of a pixel counted apart), where a residual is one factor of
    the term with |r_I| replaced by |C| + |(1 + alpha) P| + |beta| and |r_D| by |W| + |1 / Y_z|: a residual is a difference formed in
    float32, and its rounding error goes with the size of what is subtracted, not with the size of the difference.
    margins: px and z as odometry_reference.one_pass; edge: the nearest (max - min - edge_ratio min) / min to 0 among the cells with four
    positive depths; cell: how near, in pixels, a projected pixel is to the next cell of four neighbours where that cell decides the depth
    term otherwise or has another gradient of W (by more than 1e-3 of it: inside one plane W is linear and the two agree).
    dtype = numpy.float32 forms every per-pixel term in float32, the sums still in float64: an estimate of what the kernel's rounding does."""
    n, NH, NS = sizes(8 if affine else 6)
    f = dtype
    P_I, P_D, C_I, C_D = (np.asarray(a, f) for a in (P_I, P_D, C_I, C_D))
    Tm = np.asarray(T, f)
    fx, fy, cx, cy = (f(k) for k in K_level)
    sigma_i, sigma_d, nu = f(sigma_i), f(sigma_d), f(nu)
    gain, offset = f(F32(1) + F32(alpha)), f(F32(beta))
    h, w = P_I.shape
    v, u = np.nonzero(P_D > 0)
    d = P_D[v, u]
    X0, X1 = (u.astype(f) - cx) / fx * d, (v.astype(f) - cy) / fy * d
    Y = np.stack([Tm[i, 0] * X0 + Tm[i, 1] * X1 + Tm[i, 2] * d + Tm[i, 3] for i in range(3)], -1)
    front = Y[:, 2] > f(MIN_Z)
    margins = {"z": float(np.min(np.abs(Y[:, 2].astype(np.float64) - MIN_Z) / MIN_Z)) if len(d) else np.inf}
    Y, u, v = Y[front], u[front], v[front]
    iz = f(1) / Y[:, 2]
    x, y = fx * Y[:, 0] * iz + cx, fy * Y[:, 1] * iz + cy
    signed = np.stack([x - f(1), f(w - 2) - x, y - f(1), f(h - 2) - y], -1).astype(np.float64)
    holds = np.stack([signed[:, 0] >= 0, signed[:, 1] > 0, signed[:, 2] >= 0, signed[:, 3] > 0], -1)
    inside = holds.all(axis=1)
    margins["px"] = np.inf
    if len(x):
        flip_in = np.abs(signed).min(axis=1)
        flip_out = np.where(holds, -np.inf, np.abs(signed)).max(axis=1)
        margins["px"] = float(np.min(np.where(inside, flip_in, flip_out)))
    Y, u, v, x, y, iz = Y[inside], u[inside], v[inside], x[inside], y[inside], iz[inside]
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    ax, ay = x - x0.astype(f), y - y0.astype(f)
    bx, by = f(1) - ax, f(1) - ay
    gxi, gyi = np.zeros_like(C_I), np.zeros_like(C_I)
    gxi[:, 1:-1] = f(0.5) * (C_I[:, 2:] - C_I[:, :-2])
    gyi[1:-1, :] = f(0.5) * (C_I[2:, :] - C_I[:-2, :])
    sample = lambda img: by * (bx * img[y0, x0] + ax * img[y0, x0 + 1]) + ay * (bx * img[y0 + 1, x0] + ax * img[y0 + 1, x0 + 1])
    Cs, gx, gy, Pv = sample(C_I), sample(gxi), sample(gyi), P_I[v, u]
    xz, yz = Y[:, 0] * iz, Y[:, 1] * iz

    def pose_columns(a, b):
        return [a, b, -(a * xz + b * yz), -a * xz * Y[:, 1] - b * (Y[:, 2] + yz * Y[:, 1]), a * (Y[:, 2] + xz * Y[:, 0]) + b * yz * Y[:, 0],
                -a * Y[:, 1] + b * Y[:, 0]]

    sums, scale = np.zeros(NS), np.zeros(NS)
    add = lambda k, term, size: (sums.__setitem__(k, sums[k] + term.astype(np.float64).sum()),
                                 scale.__setitem__(k, scale[k] + np.abs(size.astype(np.float64)).sum()))
    # photometric
    r = (Cs - gain * Pv) - offset if affine else Cs - Pv
    size_r = np.abs(Cs) + np.abs(gain * Pv) + abs(offset) if affine else np.abs(Cs) + np.abs(Pv)
    q = r / sigma_i
    wgt = (nu + f(1)) / (nu + q * q)
    wh = wgt * (f(1) / (sigma_i * sigma_i))
    J = pose_columns(gx * fx * iz, gy * fy * iz) + ([-Pv, -np.ones_like(Pv)] if affine else [])
    k = 0
    for i in range(n):
        for j in range(i, n):
            add(k, wh * (J[i] * J[j]), wh * (J[i] * J[j]))
            k += 1
    for i in range(n):
        add(NH + i, wh * (J[i] * r), wh * (J[i] * size_r))
    add(NH + n, wgt, wgt)
    add(NH + n + 1, wgt * (r * r), wgt * (np.abs(r) * size_r))
    sums[NH + n + 2] = scale[NH + n + 2] = float(len(r))
    margins["edge"] = margins["cell"] = np.inf
    if weight > 0:
        def decide(cx0, cy0):
            """(the four depths positive, the edge test's margin, the cell's gradient of W) of the cells at (cx0, cy0), clipped into the level."""
            cx0, cy0 = np.clip(cx0, 0, w - 2), np.clip(cy0, 0, h - 2)
            four = np.stack([C_D[cy0, cx0], C_D[cy0, cx0 + 1], C_D[cy0 + 1, cx0], C_D[cy0 + 1, cx0 + 1]]).astype(np.float64)
            lo, hi = four.min(axis=0), four.max(axis=0)
            with np.errstate(divide="ignore", invalid="ignore"):
                slack = np.where(lo > 0, (edge_ratio * lo - (hi - lo)) / lo, -np.inf)
                W4 = 1.0 / four
            return lo > 0, slack, np.stack([W4[1] - W4[0] + W4[3] - W4[2], W4[2] - W4[0] + W4[3] - W4[1]]) * 0.5

        positive, slack, slope = decide(x0, y0)
        take = positive & (slack >= 0)
        if positive.any():
            margins["edge"] = float(np.abs(slack[positive]).min())
        for dx, dy, dist in ((-1, 0, ax), (1, 0, bx), (0, -1, ay), (0, 1, by)):
            other_positive, other_slack, other_slope = decide(x0 + dx, y0 + dy)
            other_take = other_positive & (other_slack >= 0)
            with np.errstate(invalid="ignore"):                    # the gradient of W belongs to a cell: it jumps where two planes meet
                jump = take & other_take & (np.abs(other_slope - slope).max(axis=0) > 1e-3 * np.abs(slope).max(axis=0) + 1e-9)
            differs = (other_take != take) | jump
            if differs.any():
                margins["cell"] = min(margins["cell"], float(dist[differs].min()))
        sel = lambda a: a[take]
        x0, y0, ax, ay, bx, by, Y, iz, xz, yz = (sel(a) for a in (x0, y0, ax, ay, bx, by, Y, iz, xz, yz))
        with np.errstate(divide="ignore"):
            W00, W01, W10, W11 = (f(1) / C_D[y0 + j, x0 + i] for j in (0, 1) for i in (0, 1))
        Ws = by * (bx * W00 + ax * W01) + ay * (bx * W10 + ax * W11)
        gx, gy = by * (W01 - W00) + ay * (W11 - W10), bx * (W10 - W00) + ax * (W11 - W01)
        r = Ws - iz
        size_r = np.abs(Ws) + np.abs(iz)
        q = r / sigma_d
        wgt = (nu + f(1)) / (nu + q * q)
        wh = wgt * (f(weight) / (sigma_d * sigma_d))
        iz2 = iz * iz
        J = pose_columns(gx * fx * iz, gy * fy * iz)
        J[2], J[3], J[4] = J[2] + iz2, J[3] + iz2 * Y[:, 1], J[4] - iz2 * Y[:, 0]
        k = 0
        for i in range(n):
            for j in range(i, n):
                if j < 6:
                    add(k, wh * (J[i] * J[j]), wh * (J[i] * J[j]))
                k += 1
        for i in range(6):
            add(NH + i, wh * (J[i] * r), wh * (J[i] * size_r))
        add(NH + n + 3, wgt, wgt)
        add(NH + n + 4, wgt * (r * r), wgt * (np.abs(r) * size_r))
        sums[NH + n + 5] = scale[NH + n + 5] = float(len(r))
    return sums, scale, margins


def solve_step(sums, n):
    """xi of (H + 1e-9 tr(H) / n I) xi = -g, or None where the matrix is not positive definite (a pivot not above MIN_PIVOT of its diagonal
    entry) or the pass has fewer than n pixels."""
    n, NH, _ = sizes(n)
    if sums[NH + n + 2] < n:
        return None
    H = np.zeros((n, n))
    k = 0
    for i in range(n):
        for j in range(i, n):
            H[i, j] = H[j, i] = sums[k]
            k += 1
    A = H + 1e-9 * np.trace(H) / n * np.eye(n)
    L = np.zeros((n, n))
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0 or not d > MIN_PIVOT * A[j, j]:
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    xi = np.linalg.solve(L.T, np.linalg.solve(L, -sums[NH:NH + n]))
    return xi if np.all(np.isfinite(xi)) else None


# ---- the full fit and the gate ----------------------------------------------------------------------------------------------------------------------
def align(prev, cur, valid0, K, iters, T_init=None, affine=True, weight=1.0, edge_ratio=0.05, nu=5.0, sigma_init=0.1, sigma_min=1e-3,
          sigma_depth_init=0.02, sigma_depth_min=1e-4, min_share=0.3, max_last_step=1e-2, max_translation=1.0, max_rotation=np.deg2rad(30.0),
          max_gain=0.5, max_offset=0.3):
    """prev, cur: pyramids of odometry_reference.pyramid(), cur with its depth. Returns T [4, 4] (identity when refused), stats [12] as the
    header lists them, trace [passes, 64] and T_fit (the aligned motion before the gate)."""
    n, NH, NS = sizes(8 if affine else 6)
    T = np.eye(4) if T_init is None else np.asarray(T_init, np.float64).copy()
    T[3] = (0, 0, 0, 1)
    bad_init = not np.all(np.isfinite(T))
    if bad_init:
        T = np.eye(4)
    sigma_i, sigma_d, alpha, beta = float(F32(sigma_init)), float(F32(sigma_depth_init)), 0.0, 0.0
    last_xi, n_i, n_d, trace = 0.0, 0.0, 0.0, []
    for level in range(len(iters) - 1, -1, -1):
        K_level = level_intrinsics(K, level)
        for _ in range(iters[level]):
            sums, _, _ = one_pass(prev[level][0], prev[level][1], cur[level][0], cur[level][1], K_level, T, float(F32(sigma_i)),
                                  float(F32(sigma_d)), alpha, beta, affine, float(F32(weight)), float(F32(edge_ratio)), nu)
            row = np.zeros(ROW)
            row[:NS], row[NS:NS + 5] = sums, (sigma_i, sigma_d, alpha, beta, level)
            trace.append(row)
            n_i, n_d = sums[NH + n + 2], sums[NH + n + 5]
            xi = solve_step(sums, n)
            last_xi = np.inf
            if xi is not None:
                T = se3_exp(xi[:6]) @ T
                if affine:
                    alpha, beta = alpha + xi[6], beta + xi[7]
                last_xi = float(np.linalg.norm(xi))
            if n_i > 0:
                sigma_i = max(float(F32(sigma_min)), float(np.sqrt(sums[NH + n + 1] / n_i)))
            if n_d > 0:
                sigma_d = max(float(F32(sigma_depth_min)), float(np.sqrt(sums[NH + n + 4] / n_d)))
    share = n_i / valid0 if valid0 > 0 else 0.0
    tn, angle = float(np.linalg.norm(T[:3, 3])), rotation_angle(T[:3, :3])
    accepted = (not bad_init and bool(np.all(np.isfinite(T))) and share >= F32(min_share) and last_xi <= F32(max_last_step)
                and tn <= F32(max_translation) and angle <= F32(max_rotation))
    if affine:
        accepted = accepted and bool(abs(alpha) <= F32(max_gain)) and bool(abs(beta) <= F32(max_offset))
    stats = np.array([float(accepted), share, sigma_i, last_xi, n_i, tn, angle, float(valid0), alpha, beta, sigma_d, n_d])
    return (T if accepted else np.eye(4)), stats, np.array(trace).reshape(-1, ROW), T


def align_scene(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, mask_prev=None, mask_cur=None, **options):
    prev, valid0 = pyramid(image_prev, depth_prev, mask_prev, levels=levels)
    cur, _ = pyramid(image_cur, depth_cur, mask_cur, levels=levels)
    return align(prev, cur, valid0, K, iters, **options)


# ---- the inputs of the one-pass comparison ------------------------------------------------------------------------------------------------------------
# (W, H, levels, level, from identity) -> (the start as a share of the planted motion, edge_ratio): chosen on the CPU among a few values each so
# that every flip margin of every variant is at least MIN_MARGIN (tests/test_odometry_rgbd_host.py asserts it).
# The bars: pixels for px and cell (a projected coordinate of up to 64 carries a float32 rounding of some 1e-5), relative for z and edge (a
# rounding of some 1e-7). The start is a share of PLANTED_XI, or one share per component of it.
MIN_MARGIN = {"px": 1e-3, "z": 1e-3, "cell": 1e-3, "edge": 1e-4}
_SHIFTED = [0.3, 0.5, 0.5, 0.5, 0.5, 0.5]      # at half of the motion two of the sizes have a pixel within 2e-5 px of a bound
ONE_PASS_SIZES = {(16, 12, 1, 0, True): (0.0, 0.05), (16, 12, 1, 0, False): (0.5, 0.05), (33, 21, 2, 0, False): (_SHIFTED, 0.04),
                  (33, 21, 2, 1, False): (0.5, 0.05), (64, 48, 3, 0, False): (0.5, 0.05), (64, 48, 3, 1, False): (_SHIFTED, 0.04),
                  (64, 48, 3, 2, False): (0.5, 0.05)}
# variant -> (affine, geometric weight, holes and masks in either frame)
ONE_PASS_VARIANTS = {"affine": (True, 0.0, False), "depth": (False, 1.0, False), "both": (True, 1.0, False), "both_holes": (True, 1.0, True)}
ONE_PASS_CASES = [size + (variant,) for size in ONE_PASS_SIZES for variant in ONE_PASS_VARIANTS]


def one_pass_case(W, H, levels, level, from_identity, variant):
    """The textured scene with gain 1.25 and offset 0.06 on the current image, one pass at `level` of `levels`. Returns a dict: the frames,
    masks (None without holes), K, iters, T_init (None: identity), affine, weight. With holes: a hole, a NaN and a masked run in the previous
    depth, a hole, a NaN and a masked block in the current one. From identity a pixel projects onto itself: the mask takes out the pixels
    that sit on the in / out bounds, and the pixels around the current frame's holes, whose cell of four neighbours a rounding would choose;
    and the current depth is a wall at 2 m, so that the two cells a rounding chooses between hold the same inverse depths."""
    affine, weight, holes = ONE_PASS_VARIANTS[variant]
    image_prev, depth_prev, image_cur, depth_cur, K, _ = scene(W, H, s=1.0, gain=1.25, offset=0.06)
    mask_prev = mask_cur = None
    if from_identity:
        depth_cur = np.full_like(depth_cur, 2.0)
    if holes or from_identity:
        mask_prev = np.ones((H, W), np.uint8)
    if holes:
        depth_prev, depth_cur = depth_prev.copy(), depth_cur.copy()
        depth_prev[H // 3:H // 3 + 2, W // 2:W // 2 + 3] = 0
        depth_prev[H // 2, W // 4] = np.nan
        mask_prev[2 * H // 3, :W // 4] = 0
        mask_cur = np.ones((H, W), np.uint8)
        spots = [(H // 4, W // 3), (H // 2 + 1, 2 * W // 3), (2 * H // 3, W // 2)]
        depth_cur[spots[0]] = 0
        depth_cur[spots[1]] = np.nan
        mask_cur[spots[2]] = 0
        if from_identity:
            for y, x in spots:
                mask_prev[y - 1:y + 2, x - 1:x + 2] = 0
    if from_identity:
        assert levels == 1 and level == 0
        mask_prev[[1, H - 2], :] = 0
        mask_prev[:, [1, W - 2]] = 0
    iters = [1 if k == level else 0 for k in range(levels)]
    start, edge_ratio = ONE_PASS_SIZES[(W, H, levels, level, from_identity)]
    return dict(image_prev=image_prev, depth_prev=depth_prev, mask_prev=mask_prev, image_cur=image_cur, depth_cur=depth_cur, mask_cur=mask_cur,
                K=K, iters=iters, T_init=None if from_identity else se3_exp(np.asarray(start) * PLANTED_XI), affine=affine, weight=weight,
                edge_ratio=edge_ratio)


_one_pass = {}


def one_pass_reference(case, dtype=np.float64):
    """(sums, scale, margins) of the restatement for one_pass_case(*case): computed once per case, shared."""
    if (case, dtype) not in _one_pass:
        c = one_pass_case(*case)
        levels, level = case[2], case[3]
        prev, _ = pyramid(c["image_prev"], c["depth_prev"], c["mask_prev"], levels=levels)
        cur, _ = pyramid(c["image_cur"], c["depth_cur"], c["mask_cur"], levels=levels)
        T = np.eye(4) if c["T_init"] is None else c["T_init"]
        _one_pass[(case, dtype)] = one_pass(prev[level][0], prev[level][1], cur[level][0], cur[level][1], level_intrinsics(c["K"], level), T,
                                            float(F32(GATE["sigma_init"])), float(F32(TERMS["sigma_depth_init"])), 0.0, 0.0, c["affine"],
                                            c["weight"], float(F32(c["edge_ratio"])), GATE["nu"], dtype)
    return _one_pass[(case, dtype)]


# ---- the full fits the host and the device tests share -----------------------------------------------------------------------------------------------
# case -> (flat, gain, offset, affine, geometric weight)
FIT_VARIANTS = {"gain_affine": (False, 1.25, 0.06, True, 0.0), "textured_depth": (False, 1.0, 0.0, False, 1.0),
                "gain_affine_depth": (False, 1.25, 0.06, True, 1.0)}
FIT_CASES = {f"{name}_{s}": (name, s) for name in FIT_VARIANTS for s in (1.0, 2.5)}
FLAT_SIZES = {(64, 48): (2, [8, 10]), (96, 72): (3, [5, 7, 10])}          # a 16 x 12 coarsest level diverges on the flat scene: not 64 x 48 with 3
_fits = {}


def fit(size, levels, iters, flat, gain, offset, affine, weight, s):
    """(T after the gate, stats, T before the gate, T_true) of the restatement: computed once per input, shared."""
    key = (size, levels, tuple(iters), flat, gain, offset, affine, weight, s)
    if key not in _fits:
        image_prev, depth_prev, image_cur, depth_cur, K, T_true = scene(*size, s=s, flat=flat, gain=gain, offset=offset)
        T, stats, _, T_fit = align_scene(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, affine=affine, weight=weight)
        _fits[key] = (T, stats, T_fit, T_true)
    return _fits[key]


def planted_fit(size, case):
    levels, iters, _, _ = PLANTED_SIZES[size]
    name, s = FIT_CASES[case]
    return fit(size, levels, iters, *FIT_VARIANTS[name], s)
