"""numpy restatement of include/visual_odometry.h: the pyramid in float32 (the kernels equal it bit for bit), one pass, the full fit and the
gate in float64 on that pyramid, and the planted scene the tests align: a textured plane seen from two poses, both images and the previous
depth from exact ray-plane intersection. Needs neither a GPU nor the library."""
import numpy as np

MIN_Z = 1e-3
MIN_IN = 6
F32 = np.float32

PLANE = np.array([0.15, 0.1, 1.0])            # the plane PLANE . X = PLANE_D in the previous camera's frame
PLANE_D = 2.0
PLANTED_XI = np.array([0.03, -0.02, 0.015, np.deg2rad(0.8), np.deg2rad(-1.0), np.deg2rad(0.6)])
DEFAULTS = dict(nu=5.0, sigma_init=0.1, sigma_min=1e-3, min_share=0.3, max_last_step=1e-2, max_translation=1.0, max_rotation=np.deg2rad(30.0))


# ---- SE(3) ----------------------------------------------------------------------------------------------------------------------------
def se3_exp(xi):
    """exp of xi = [rho | theta] as a 4 x 4 (the closed forms of slam/camera.py SE3_exp)."""
    xi = np.asarray(xi, np.float64)
    wx, wy, wz = xi[3:]
    K = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
    th = np.sqrt(wx * wx + wy * wy + wz * wz)
    A, B, C = 1.0, 0.5, 1.0 / 6.0
    if th >= 1e-5:
        A, B, C = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    E = np.eye(4)
    E[:3, :3] = np.eye(3) + A * K + B * K @ K
    E[:3, 3] = (np.eye(3) + B * K + C * K @ K) @ xi[:3]
    return E


def rotation_angle(R):
    s = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(0.5 * np.linalg.norm(s), 0.5 * (np.trace(R) - 1.0)))


def pose_error(T, T_true):
    """(rotation error in degrees, translation error in millimetres for a scene in metres)."""
    T, T_true = np.asarray(T, np.float64), np.asarray(T_true, np.float64)
    return np.rad2deg(rotation_angle(T[:3, :3] @ T_true[:3, :3].T)), 1e3 * float(np.linalg.norm(T[:3, 3] - T_true[:3, 3]))


# ---- the planted scene -------------------------------------------------------------------------------------------------------------------
def intrinsics(W, H):
    return 0.9 * W, 0.9 * W, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2


def texture(x, y):
    return (0.5 + 0.12 * np.sin(3.1 * x + 0.4) + 0.1 * np.sin(4.3 * y + 1) + 0.08 * np.sin(7.7 * x + 5.1 * y) + 0.06 * np.sin(13 * x - 9 * y + 2)
            + 0.05 * np.sin(21 * x + 17 * y))


def planted_motion(s):
    return se3_exp(s * PLANTED_XI)


def planted_scene(W, H, s=1.0, patch=False, T=None):
    """image_prev [3, H, W] float32, depth_prev [H, W] float32, image_cur [3, H, W] float32, K = (fx, fy, cx, cy), T_true (previous camera ->
    current camera). patch: a rectangle of 3 % of the current image is set to 0.9."""
    fx, fy, cx, cy = K = intrinsics(W, H)
    T = planted_motion(s) if T is None else np.asarray(T, np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    z = PLANE_D / (ray @ PLANE)
    prev = texture(ray[..., 0] * z, ray[..., 1] * z)
    R, t = T[:3, :3], T[:3, 3]
    origin, direction = -R.T @ t, ray @ R                         # the current camera's rays in the previous frame (R^T applied to each ray)
    step = (PLANE_D - PLANE @ origin) / (direction @ PLANE)
    point = origin + direction * step[..., None]
    cur = texture(point[..., 0], point[..., 1])
    if patch:
        ph, pw = int(round(0.15 * H)), int(round(0.2 * W))
        y0, x0 = int(0.35 * H), int(0.4 * W)
        cur[y0:y0 + ph, x0:x0 + pw] = 0.9
    as_rgb = lambda g: np.ascontiguousarray(np.broadcast_to(g.astype(F32)[None], (3, H, W)))
    return as_rgb(prev), z.astype(F32), as_rgb(cur), K, T


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------
def level_intrinsics(K, level):
    """The float32 values the library hands its kernels for one level, as float64."""
    fx, fy, cx, cy = (F32(k) for k in K)
    s = F32(1.0 / (1 << level))
    return (float(F32(fx * s)), float(F32(fy * s)), float(F32((float(cx) + 0.5) * float(s) - 0.5)), float(F32((float(cy) + 0.5) * float(s) - 0.5)))


def pyramid(image, depth=None, mask=None, depth_min=0.0, depth_max=np.inf, levels=3):
    """[(I, D)] per level in float32, and the count of D > 0 at level 0. image [3, H, W] float32."""
    image = np.asarray(image, F32)
    r, g, b = image
    I = (F32(0.299) * r + F32(0.587) * g) + F32(0.114) * b
    d = np.zeros(I.shape, F32) if depth is None else np.asarray(depth, F32)
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(d) & (d > 0) & (d >= F32(depth_min)) & (d <= F32(depth_max))
    if mask is not None:
        valid &= np.asarray(mask) != 0
    D = np.where(valid, d, F32(0)).astype(F32)
    out = [(I, D)]
    for _ in range(1, levels):
        h, w = I.shape[0] // 2, I.shape[1] // 2
        a, b_, c, e = (I[dy:2 * h:2, dx:2 * w:2] for dy in (0, 1) for dx in (0, 1))
        I = (((a + b_) + (c + e)) * F32(0.25)).astype(F32)
        four = np.stack([D[dy:2 * h:2, dx:2 * w:2] for dy in (0, 1) for dx in (0, 1)])
        m = np.where(four > 0, four, np.inf).min(axis=0)
        D = np.where(np.isfinite(m), m, 0).astype(F32)
        out.append((I, D))
    return out, int(valid.sum())


def pyramid_bytes(pyr, valid0):
    """The buffer gsr_odometry_pyramid writes, as bytes: the head, then I and D per level, each on a multiple of 16 bytes."""
    parts = [np.array([valid0, 0, 0, 0], np.int32).tobytes()]
    for I, D in pyr:
        for a in (I, D):
            raw = np.ascontiguousarray(a, F32).tobytes()
            parts.append(raw + b"\0" * (-len(raw) % 16))
    return b"".join(parts)


# ---- one pass -------------------------------------------------------------------------------------------------------------------------------
def one_pass(P_I, P_D, C_I, K_level, T, sigma, nu=5.0):
    """The sums of one pass in float64. Returns sums [30] (21 of H upper triangle row-major, 6 of g, sum w, sum w r^2, n), scale [30] (the sum
    of the absolute values of each sum's terms, with |r| replaced by |C| + |P| in g's), margin_px (how far the nearest projected pixel is
    from flipping its in / out decision, in pixels) and margin_z (the same for Y_z against MIN_Z, relative)."""
    P_I, P_D, C_I, T = (np.asarray(a, np.float64) for a in (P_I, P_D, C_I, T))
    fx, fy, cx, cy = K_level
    h, w = P_I.shape
    v, u = np.nonzero(P_D > 0)
    d = P_D[v, u]
    X = np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], -1)
    Y = X @ T[:3, :3].T + T[:3, 3]
    front = Y[:, 2] > MIN_Z
    margin_z = float(np.min(np.abs(Y[:, 2] - MIN_Z) / MIN_Z)) if len(d) else np.inf
    Y, u, v = Y[front], u[front], v[front]
    iz = 1.0 / Y[:, 2]
    x, y = fx * Y[:, 0] * iz + cx, fy * Y[:, 1] * iz + cy
    signed = np.stack([x - 1.0, (w - 2.0) - x, y - 1.0, (h - 2.0) - y], -1)          # positive: the condition holds (the upper ones strictly)
    inside = (signed[:, 0] >= 0) & (signed[:, 1] > 0) & (signed[:, 2] >= 0) & (signed[:, 3] > 0)
    margin_px = np.inf
    if len(x):
        holds = np.stack([signed[:, 0] >= 0, signed[:, 1] > 0, signed[:, 2] >= 0, signed[:, 3] > 0], -1)
        flip_in = np.abs(signed).min(axis=1)                                          # an inside pixel leaves when its nearest bound flips
        flip_out = np.where(holds, -np.inf, np.abs(signed)).max(axis=1)               # an outside pixel enters when all its failing ones flip
        margin_px = float(np.min(np.where(inside, flip_in, flip_out)))
    Y, u, v, x, y, iz = Y[inside], u[inside], v[inside], x[inside], y[inside], iz[inside]
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    ax, ay = x - x0, y - y0
    gxi = np.zeros_like(C_I)
    gyi = np.zeros_like(C_I)
    gxi[:, 1:-1] = 0.5 * (C_I[:, 2:] - C_I[:, :-2])
    gyi[1:-1, :] = 0.5 * (C_I[2:, :] - C_I[:-2, :])
    sample = lambda img: ((1 - ay) * ((1 - ax) * img[y0, x0] + ax * img[y0, x0 + 1]) + ay * ((1 - ax) * img[y0 + 1, x0] + ax * img[y0 + 1, x0 + 1]))
    Cs, gx, gy, Pv = sample(C_I), sample(gxi), sample(gyi), P_I[v, u]
    r = Cs - Pv
    wgt = (nu + 1.0) / (nu + (r / sigma) ** 2)
    a, b, xz, yz = gx * fx * iz, gy * fy * iz, Y[:, 0] * iz, Y[:, 1] * iz
    J = np.stack([a, b, -(a * xz + b * yz), -a * xz * Y[:, 1] - b * (Y[:, 2] + yz * Y[:, 1]), a * (Y[:, 2] + xz * Y[:, 0]) + b * yz * Y[:, 0],
                  -a * Y[:, 1] + b * Y[:, 0]], -1)
    sums, scale = np.zeros(30), np.zeros(30)
    k = 0
    for i in range(6):
        for j in range(i, 6):
            term = wgt * J[:, i] * J[:, j]
            sums[k], scale[k] = term.sum(), np.abs(term).sum()
            k += 1
    for i in range(6):
        sums[21 + i] = (wgt * J[:, i] * r).sum()
        scale[21 + i] = (wgt * np.abs(J[:, i]) * (np.abs(Cs) + np.abs(Pv))).sum()
    sums[27] = scale[27] = wgt.sum()
    sums[28] = scale[28] = (wgt * r * r).sum()
    sums[29] = scale[29] = float(len(r))
    return sums, scale, margin_px, margin_z


def solve_step(sums):
    """xi of (H + 1e-9 tr(H) / 6 I) xi = -g, or None where the matrix is not positive definite or the pass has fewer than MIN_IN pixels."""
    if sums[29] < MIN_IN:
        return None
    H = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = sums[k]
            k += 1
    H = H + 1e-9 * np.trace(H) / 6.0 * np.eye(6)
    try:
        L = np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return None
    xi = np.linalg.solve(L.T, np.linalg.solve(L, -sums[21:27]))
    return xi if np.all(np.isfinite(xi)) else None


# ---- the full fit and the gate -----------------------------------------------------------------------------------------------------------------
def align(prev, cur, valid0, K, iters, T_init=None, nu=5.0, sigma_init=0.1, sigma_min=1e-3, min_share=0.3, max_last_step=1e-2,
          max_translation=1.0, max_rotation=np.deg2rad(30.0)):
    """prev, cur: pyramids of pyramid(). iters: per level, finest first. Returns T [4, 4] (identity when refused), stats [8] as the header lists
    them, trace [passes, 32] and T_fit (the aligned motion before the gate)."""
    T = np.eye(4) if T_init is None else np.asarray(T_init, np.float64).copy()
    T[3] = (0, 0, 0, 1)
    bad_init = not np.all(np.isfinite(T))
    if bad_init:
        T = np.eye(4)
    sigma, last_xi, n_last, trace = float(F32(sigma_init)), 0.0, 0.0, []
    for level in range(len(iters) - 1, -1, -1):
        K_level = level_intrinsics(K, level)
        for _ in range(iters[level]):
            sums, _, _, _ = one_pass(prev[level][0], prev[level][1], cur[level][0], K_level, T, float(F32(sigma)), nu)
            trace.append(np.concatenate([sums, [sigma, level]]))
            n_last = sums[29]
            xi = solve_step(sums)
            last_xi = np.inf
            if xi is not None:
                T = se3_exp(xi) @ T
                last_xi = float(np.linalg.norm(xi))
            if n_last > 0:
                sigma = max(float(F32(sigma_min)), float(np.sqrt(sums[28] / n_last)))
    share = n_last / valid0 if valid0 > 0 else 0.0
    tn, angle = float(np.linalg.norm(T[:3, 3])), rotation_angle(T[:3, :3])
    accepted = (not bad_init and bool(np.all(np.isfinite(T))) and share >= F32(min_share) and last_xi <= F32(max_last_step)
                and tn <= F32(max_translation) and angle <= F32(max_rotation))
    stats = np.array([float(accepted), share, sigma, last_xi, n_last, tn, angle, float(valid0)])
    return (T if accepted else np.eye(4)), stats, np.array(trace).reshape(-1, 32), T


def align_scene(image_prev, depth_prev, image_cur, K, levels, iters, mask=None, depth_min=0.0, depth_max=np.inf, **options):
    prev, valid0 = pyramid(image_prev, depth_prev, mask, depth_min, depth_max, levels)
    cur, _ = pyramid(image_cur, None, None, 0.0, np.inf, levels)
    return align(prev, cur, valid0, K, iters, **options)


# ---- the inputs of the one-pass comparison ---------------------------------------------------------------------------------------------------
ONE_PASS_START = 0.5             # the given T_init is exp(ONE_PASS_START * PLANTED_XI): half of the planted motion
ONE_PASS_CASES = [(16, 12, 1, 0, True), (16, 12, 1, 0, False), (33, 21, 1, 0, True), (33, 21, 2, 0, False), (33, 21, 2, 1, False),
                  (64, 48, 1, 0, True), (64, 48, 3, 0, False), (64, 48, 3, 1, False), (64, 48, 3, 2, False)]


def one_pass_case(W, H, levels, level, from_identity):
    """The planted scene with a depth hole and a mask, one pass at `level` of `levels`: image_prev, depth_prev, mask, image_cur, K, iters,
    T_init (None: identity). From identity a pixel projects onto itself, so the pixels of column and row 1 and of column W - 2 and row
    H - 2 would sit on the in / out bounds themselves; the mask takes them out (level 0 only: the identity cases have one level)."""
    image_prev, depth_prev, image_cur, K, _ = planted_scene(W, H, s=1.0)
    depth_prev = depth_prev.copy()
    depth_prev[H // 3:H // 3 + 2, W // 2:W // 2 + 3] = 0
    depth_prev[H // 2, W // 4] = np.nan
    mask = np.ones((H, W), np.uint8)
    mask[2 * H // 3, :W // 4] = 0
    if from_identity:
        assert levels == 1 and level == 0
        mask[[1, H - 2], :] = 0
        mask[:, [1, W - 2]] = 0
    iters = [1 if k == level else 0 for k in range(levels)]
    return image_prev, depth_prev, mask, image_cur, K, iters, (None if from_identity else se3_exp(ONE_PASS_START * PLANTED_XI))


def one_pass_reference(case, sigma=0.1, nu=5.0):
    """(sums, scale, margin_px, margin_z) of the restatement for one_pass_case(*case)."""
    image_prev, depth_prev, mask, image_cur, K, iters, T_init = one_pass_case(*case)
    levels, level = case[2], case[3]
    prev, _ = pyramid(image_prev, depth_prev, mask, levels=levels)
    cur, _ = pyramid(image_cur, levels=levels)
    T = np.eye(4) if T_init is None else T_init
    return one_pass(prev[level][0], prev[level][1], cur[level][0], level_intrinsics(K, level), T, float(F32(sigma)), nu)


# ---- the full fits the host and the device tests share ------------------------------------------------------------------------------------------
# size -> (levels, iters finest first, the device bars in degrees and millimetres)
PLANTED_SIZES = {(160, 120): (3, [5, 7, 10], 0.01, 0.5), (64, 48): (3, [5, 7, 10], 0.1, 3.0), (33, 21): (2, [8, 10], 0.5, 15.0)}
PLANTED_CASES = {"clean_1": (1.0, False), "clean_2.5": (2.5, False), "patch_1": (1.0, True), "patch_2.5": (2.5, True)}
_fits = {}


def planted_fit(size, case):
    """(T after the gate, stats, T before the gate, T_true) of the restatement on the planted scene: computed once per case, shared."""
    if (size, case) not in _fits:
        levels, iters, _, _ = PLANTED_SIZES[size]
        s, patch = PLANTED_CASES[case]
        image_prev, depth_prev, image_cur, K, T_true = planted_scene(*size, s=s, patch=patch)
        T, stats, _, T_fit = align_scene(image_prev, depth_prev, image_cur, K, levels, iters)
        _fits[(size, case)] = (T, stats, T_fit, T_true)
    return _fits[(size, case)]
