"""include/feature_matching.h restated in numpy: keypoints and descriptors of a frame, the mutual match of two sets, the pose of the matched
pairs. Integers wherever the header has integers; the float32 steps of the pose are float32 numpy operations, one at a time, in the header's
order; the refinement is float64. The device's keypoints, descriptors, matches, counts and stats equal these bit for bit, its T to the last
float32 digit or two (tests/test_hip_features.py). Also the analytic scene of the tests: a textured plane seen from two poses, with exact
depth for both views."""
import numpy as np

import odometry_reference as odo
import reloc_reference as reloc

F32 = np.float32
BORDER, RADIUS, CLAMP, NONE = 18, 15, 16, 257
CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))


# ---- extract ------------------------------------------------------------------------------------------------------------------------------
def luma(image):
    q = reloc.quant(np.asarray(image, F32))
    return (77 * q[0] + 150 * q[1] + 29 * q[2] + 128) >> 8


def _shifted(a, dx, dy, pad):
    """a(p + (dx, dy)) for every pixel p of the image inside the array `a` padded by `pad` zeros on every side"""
    H, W = a.shape[0] - 2 * pad, a.shape[1] - 2 * pad
    return a[pad + dy:pad + dy + H, pad + dx:pad + dx + W]


def fast_score(L):
    Lp = np.pad(np.asarray(L, np.int64), 3)
    d = np.stack([_shifted(Lp, ox, oy, 3) for ox, oy in CIRCLE]) - np.asarray(L, np.int64)[None]
    bright = np.full(L.shape, -255, np.int64)
    dark = bright.copy()
    for s in range(16):
        run = d[[(s + j) % 16 for j in range(9)]]
        bright = np.maximum(bright, run.min(axis=0))
        dark = np.maximum(dark, (-run).min(axis=0))
    return np.maximum(np.maximum(bright, dark), 0)


def corner_map(L, mask, threshold):
    """c(p): the score at a corner, 0 elsewhere"""
    H, W = L.shape
    score = fast_score(L)
    ok = score > threshold
    if mask is not None:
        ok &= np.asarray(mask).reshape(H, W) != 0
    inside = np.zeros((H, W), bool)
    if W > 2 * BORDER and H > 2 * BORDER:
        inside[BORDER:H - BORDER, BORDER:W - BORDER] = True
    return np.where(ok & inside, score, 0)


def suppress(c):
    cp = np.pad(c, 1)
    kept = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            nc = _shifted(cp, dx, dy, 1)
            earlier = dy < 0 or (dy == 0 and dx < 0)
            kept &= ~((nc > c) | ((nc == c) & earlier))
    return kept


def box_sums(L):
    Lp = np.pad(np.asarray(L, np.int64), 2)
    return sum(_shifted(Lp, dx, dy, 2) for dy in range(-2, 3) for dx in range(-2, 3))


def slots(W, H, cell, per_cell):
    return -(-W // cell) * -(-H // cell) * per_cell


def extract(image, mask, cell, per_cell, threshold, directions, pattern):
    """(keypoints int32 [slots, 4], descriptors uint32 [slots, 8])"""
    L = luma(image)
    H, W = L.shape
    c = corner_map(L, mask, threshold)
    kept = suppress(c)
    S = box_sums(L)
    cells_x, cells_y = -(-W // cell), -(-H // cell)
    n = cells_x * cells_y * per_cell
    keypoints = np.tile(np.array([-1, -1, 0, 0], np.int32), (n, 1))
    descriptors = np.zeros((n, 8), np.uint32)
    directions = np.asarray(directions, np.int64).reshape(32, 2)
    pattern = np.clip(np.asarray(pattern, np.int64).reshape(32, 256, 4), -CLAMP, CLAMP)
    dy, dx = np.mgrid[-RADIUS:RADIUS + 1, -RADIUS:RADIUS + 1]
    disc = dx * dx + dy * dy <= RADIUS * RADIUS
    ys, xs = np.nonzero(kept)
    for j in range(cells_y):
        for i in range(cells_x):
            here = (xs // cell == i) & (ys // cell == j)
            found = sorted(zip(-c[ys[here], xs[here]], ys[here] * W + xs[here]))[:per_cell]
            for rank, (neg, index) in enumerate(found):
                x, y = int(index % W), int(index // W)
                patch = L[y - RADIUS:y + RADIUS + 1, x - RADIUS:x + RADIUS + 1]
                m10, m01 = int((dx * patch)[disc].sum()), int((dy * patch)[disc].sum())
                k = int(np.argmax(directions[:, 0] * m10 + directions[:, 1] * m01))
                slot = (j * cells_x + i) * per_cell + rank
                keypoints[slot] = (x, y, -neg, k)
                pairs = pattern[k]
                bits = S[y + pairs[:, 1], x + pairs[:, 0]] < S[y + pairs[:, 3], x + pairs[:, 2]]
                descriptors[slot] = np.packbits(bits.reshape(8, 32), axis=1, bitorder="little").view(np.uint32).reshape(8)
    return keypoints, descriptors


# ---- match --------------------------------------------------------------------------------------------------------------------------------
def hamming(desc_a, desc_b):
    """int64 [A, B]: the differing bits of every pair (two exact float32 products of 0 / 1 matrices)"""
    bits = lambda d: np.unpackbits(np.ascontiguousarray(d, np.uint32).view(np.uint8), axis=1, bitorder="little").astype(F32)
    a, b = bits(desc_a), bits(desc_b)
    return (a @ (1 - b).T + (1 - a) @ b.T).astype(np.int64)


def _best(D, valid_rows, valid_cols):
    """per row: (the column of the smallest (d, column) over the valid columns or -1, its d or 257, the smallest d of the others or 257)"""
    n = D.shape[0]
    best, dist, second = np.full(n, -1, np.int64), np.full(n, NONE, np.int64), np.full(n, NONE, np.int64)
    cols = np.nonzero(valid_cols)[0]
    if cols.size:
        sub = D[:, cols]
        at = np.argmin(sub, axis=1)                                    # the first of the smallest: the lowest column
        best, dist = cols[at], sub[np.arange(n), at]
        if cols.size > 1:
            rest = sub.copy()
            rest[np.arange(n), at] = NONE
            second = rest.min(axis=1)
    best, dist, second = (np.where(valid_rows, v, fill) for v, fill in ((best, -1), (dist, NONE), (second, NONE)))
    return best, dist, second


def match(kp_a, desc_a, kp_b, desc_b, max_distance, ratio_eighths):
    """int32 [slots_a, 2]"""
    va, vb = np.asarray(kp_a)[:, 0] >= 0, np.asarray(kp_b)[:, 0] >= 0
    D = hamming(desc_a, desc_b)
    b, d, second = _best(D, va, vb)
    a_of_b, _, _ = _best(D.T, vb, va)
    ok = (b >= 0) & (d <= max_distance) & (8 * d <= ratio_eighths * second)
    ok &= a_of_b[np.maximum(b, 0)] == np.arange(len(b))
    return np.stack([np.where(ok, b, -1), d], axis=1).astype(np.int32)


# ---- pose ---------------------------------------------------------------------------------------------------------------------------------
def lowbias32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def pair_list(kp_a, depth_a, kp_b, depth_b, matches, K_a, K_b):
    """(P_a float32 [M, 3], P_b float32 [M, 3], uv float32 [M, 2], the slots a of the list)"""
    H, W = depth_a.shape
    PA, PB, UV, slots_a = [], [], [], []
    Ka, Kb = np.asarray(K_a, F32), np.asarray(K_b, F32)
    for a, (b, _) in enumerate(np.asarray(matches)):
        xa, ya = int(kp_a[a][0]), int(kp_a[a][1])
        if not (0 <= b < len(kp_b) and 0 <= xa < W and 0 <= ya < H):
            continue
        xb, yb = int(kp_b[b][0]), int(kp_b[b][1])
        if not (0 <= xb < W and 0 <= yb < H):
            continue
        za, zb = F32(depth_a[ya, xa]), F32(depth_b[yb, xb])
        if not (np.isfinite(za) and za > 0 and np.isfinite(zb) and zb > 0):
            continue
        PA.append([(F32(xa) - Ka[2]) * za / Ka[0], (F32(ya) - Ka[3]) * za / Ka[1], za])
        PB.append([(F32(xb) - Kb[2]) * zb / Kb[0], (F32(yb) - Kb[3]) * zb / Kb[1], zb])
        UV.append([F32(xb), F32(yb)])
        slots_a.append(a)
    shape = lambda v, k: np.asarray(v, F32).reshape(-1, k)
    return shape(PA, 3), shape(PB, 3), shape(UV, 2), np.asarray(slots_a, np.int64)


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _norm(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def triad(p1, p2, p3, min_area):
    """(e1, e2, e3 float32 [..., 3], valid); every operation float32"""
    with np.errstate(all="ignore"):
        d = p2 - p1
        e1 = d / _norm(d)[..., None]
        c = _cross(e1, p3 - p1)
        n3 = _norm(c)
        e3 = c / n3[..., None]
        return e1, _cross(e3, e1), e3, n3 >= F32(min_area)


def hypotheses(PA, PB, seed, count, min_area):
    """(R float32 [count, 3, 3], t float32 [count, 3], valid [count]) of the hypotheses 0 .. count - 1"""
    M = len(PA)
    R, t = np.zeros((count, 3, 3), F32), np.zeros((count, 3), F32)
    if M < 3:
        return R, t, np.zeros(count, bool)
    base = (np.uint64(seed) * np.uint64(0x9E3779B9) + 3 * np.arange(count, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    idx = np.stack([lowbias32(base + np.uint64(k)) % np.uint64(M) for k in range(3)], axis=1).astype(np.int64)
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    a, b = PA[idx], PB[idx]                                            # [count, 3 points, 3]
    with np.errstate(all="ignore"):
        ea = triad(a[:, 0], a[:, 1], a[:, 2], min_area)
        eb = triad(b[:, 0], b[:, 1], b[:, 2], min_area)
        valid &= ea[3] & eb[3]
        ma, mb = (a[:, 0] + a[:, 1] + a[:, 2]) / F32(3), (b[:, 0] + b[:, 1] + b[:, 2]) / F32(3)
        for i in range(3):
            for j in range(3):
                R[:, i, j] = eb[0][:, i] * ea[0][:, j] + eb[1][:, i] * ea[1][:, j] + eb[2][:, i] * ea[2][:, j]
        for i in range(3):
            t[:, i] = mb[:, i] - (R[:, i, 0] * ma[:, 0] + R[:, i, 1] * ma[:, 1] + R[:, i, 2] * ma[:, 2])
    return R, t, valid


def inliers(R, t, PA, PB, UV, K_b, tau_px, tau_depth):
    """bool [..., M] for R [..., 3, 3], t [..., 3]: the header's test in float32"""
    R, t, K = np.asarray(R, F32), np.asarray(t, F32), np.asarray(K_b, F32)
    tau_px, tau_depth = F32(tau_px), F32(tau_depth)
    with np.errstate(all="ignore"):
        Q = [R[..., i, 0, None] * PA[:, 0] + R[..., i, 1, None] * PA[:, 1] + R[..., i, 2, None] * PA[:, 2] + t[..., i, None] for i in range(3)]
        ex = K[0] * (Q[0] / Q[2]) + K[2] - UV[:, 0]
        ey = K[1] * (Q[1] / Q[2]) + K[3] - UV[:, 1]
        zb = PB[:, 2]
        return (Q[2] > 0) & (ex * ex + ey * ey <= tau_px * tau_px) & (np.abs(Q[2] - zb) <= tau_depth * zb)


def exp_apply(xi, R, t):
    """exp(xi) (R, t), xi = [rho | theta], float64: the closed form of csrc/gs_features.h"""
    w = xi[3:]
    a2 = float(w @ w)
    a = np.sqrt(a2)
    A, B, C = (np.sin(a) / a, (1 - np.cos(a)) / a2, (a - np.sin(a)) / (a2 * a)) if a >= 1e-6 else (1.0, 0.5, 1.0 / 6.0)
    Wm = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    dR = np.eye(3) + A * Wm + B * (Wm @ Wm)
    V = np.eye(3) + B * Wm + C * (Wm @ Wm)
    return dR @ R, dR @ t + V @ xi[:3]


def refine(R, t, PA, PB, iters):
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    PA, PB = np.asarray(PA, np.float64), np.asarray(PB, np.float64)
    for _ in range(iters):
        q = PA @ R.T + t
        r = q - PB
        J = np.zeros((len(q), 3, 6))
        J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
        J[:, 0, 4], J[:, 0, 5] = q[:, 2], -q[:, 1]
        J[:, 1, 3], J[:, 1, 5] = -q[:, 2], q[:, 0]
        J[:, 2, 3], J[:, 2, 4] = q[:, 1], -q[:, 0]
        Hm, g = np.einsum("nri,nrj->ij", J, J), np.einsum("nri,nr->i", J, r)
        try:
            Lc = np.linalg.cholesky(Hm)
        except np.linalg.LinAlgError:
            break
        xi = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        if not np.all(np.isfinite(xi)):
            break
        R, t = exp_apply(xi, R, t)
    return R, t


def pose(kp_a, depth_a, kp_b, depth_b, matches, K_a, K_b, seed=0, count=256, min_area=0.01, tau_px=2.0, tau_depth=0.05, refine_iters=3,
         min_matches=12, min_inliers=8, min_share=0.5, max_translation=1.5, max_rotation=np.deg2rad(45.0)):
    """{"T" float32 [4, 4], "stats" int32 [8], "counts" int32 [count], "T_refined" float64 [4, 4] or None (the pose before the gate)}"""
    PA, PB, UV, _ = pair_list(kp_a, np.asarray(depth_a, F32), kp_b, np.asarray(depth_b, F32), matches, K_a, K_b)
    M = len(PA)
    R, t, valid = hypotheses(PA, PB, seed, count, min_area)
    counts = np.where(valid, inliers(R, t, PA, PB, UV, K_b, tau_px, tau_depth).sum(axis=-1), 0).astype(np.int32) if M else np.zeros(count, np.int32)
    winner = int(np.argmax(counts))                                    # the first of the largest: the lowest h
    stats = np.array([(np.asarray(kp_a)[:, 0] >= 0).sum(), (np.asarray(kp_b)[:, 0] >= 0).sum(), M, winner, counts[winner], 0, 0, 0], np.int32)
    T, refined = np.eye(4, dtype=F32), None
    if counts[winner] >= 3:
        keep = inliers(R[winner], t[winner], PA, PB, UV, K_b, tau_px, tau_depth)
        R64, t64 = refine(R[winner], t[winner], PA[keep], PB[keep], refine_iters)
        R32, t32 = R64.astype(F32), t64.astype(F32)
        final = int(inliers(R32, t32, PA, PB, UV, K_b, tau_px, tau_depth).sum())
        refined = np.eye(4)
        refined[:3, :3], refined[:3, 3] = R64, t64
        Rd, td = R32.astype(np.float64), t32.astype(np.float64)
        ax = np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
        angle = np.arctan2(0.5 * np.sqrt(ax @ ax), 0.5 * (np.trace(Rd) - 1.0))
        accepted = (np.all(np.isfinite(R32)) and np.all(np.isfinite(t32)) and M >= min_matches and final >= min_inliers and
                    final >= float(F32(min_share)) * M and np.sqrt(td @ td) <= float(F32(max_translation)) and angle <= float(F32(max_rotation)))
        stats[5], stats[6] = final, int(accepted)
        if accepted:
            T[:3, :3], T[:3, 3] = R32, t32
    return {"T": T, "stats": stats, "counts": counts, "T_refined": refined}


# ---- the analytic scene -------------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
PLANE_D = 2.5
CENTRE = np.array([0.0, 0.0, PLANE_D / PLANE_N[2]])                   # where the optical axis of view A meets the plane


def cell_hash(ix, iy, salt):
    """An integer hash of two integer coordinates, mapped to [0, 1]"""
    x = (np.asarray(ix, np.int64) * 73856093) ^ (np.asarray(iy, np.int64) * 19349663) ^ (int(salt) * 83492791)
    return lowbias32(x & 0xFFFFFFFF).astype(np.float64) / 4294967295.0


def blocks_texture(x, y):
    h = lambda s, ox, oy, salt: cell_hash(np.floor(x / s + ox), np.floor(y / s + oy), salt)
    return 0.15 + 0.7 * (0.5 * h(0.16, 0.0, 0.0, 1) + 0.3 * h(0.37, 0.3, 0.1, 2) + 0.2 * h(0.07, 0.0, 0.0, 3))


def rotation(axis, degrees):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    Wm = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Wm + (1 - np.cos(a)) * (Wm @ Wm)


def _motion(axis, degrees, follow, extra):
    """P_b = R P_a + t: a rotation, `follow` of the translation that keeps CENTRE on the optical axis, and `extra`"""
    T = np.eye(4)
    T[:3, :3] = rotation(axis, degrees)
    T[:3, 3] = follow * (CENTRE - T[:3, :3] @ CENTRE) + np.asarray(extra, np.float64)
    return T


MOTIONS = {"small": _motion((0.3, 1.0, 0.2), 2.0, 0.5, (0.0, 0.01, -0.01)),       # 2 degrees, 5 cm
           "wide": _motion((0.2, 1.0, 0.1), 16.0, 0.9, (0.0, 0.0, 0.0)),          # 16 degrees, 0.63 m
           "roll": _motion((0.0, 0.0, 1.0), 30.0, 0.0, (0.25, -0.15, 0.07)),      # 30 degrees about the axis, 0.3 m
           "wider": _motion((-0.1, 1.0, 0.05), 26.0, 0.86, (0.0, 0.0, 0.0)),      # 26 degrees, 0.97 m
           "unrelated": _motion((0.3, 1.0, 0.2), 2.0, 0.5, (0.0, 0.01, -0.01))}   # the small motion; the texture of B is shifted by 50 m


def view(W, H, T=None, shift=0.0):
    """(image float32 [3, H, W] grey, depth float32 [H, W]) of the plane from the camera with P = R P_a + t, T = None: view A"""
    fx, fy, cx, cy = odo.intrinsics(W, H)
    T = np.eye(4) if T is None else T
    Rt, t = T[:3, :3].T, T[:3, 3]
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    grey, depth = np.zeros((H, W)), None
    for sy in (-1 / 3, 0.0, 1 / 3):
        for sx in (-1 / 3, 0.0, 1 / 3):
            ray = np.stack([(u + sx - cx) / fx, (v + sy - cy) / fy, np.ones_like(u)], axis=-1)
            s = (PLANE_D + PLANE_N @ (Rt @ t)) / (ray @ (Rt.T @ PLANE_N))          # n . R^T (s ray - t) = d
            X = (s[..., None] * ray - t) @ Rt.T
            grey += blocks_texture(X[..., 0] + shift, X[..., 1] + shift) / 9.0
            if sx == 0.0 and sy == 0.0:
                depth = s
    return np.repeat(grey[None], 3, axis=0).astype(F32), depth.astype(F32)


_scenes = {}


def scene(name, W, H):
    """(image_a, depth_a, image_b, depth_b, K, T_true) of one of MOTIONS; computed once, shared, never modified"""
    if (name, W, H) not in _scenes:
        T = MOTIONS[name]
        a, b = view(W, H), view(W, H, T, 50.0 if name == "unrelated" else 0.0)
        for arr in (*a, *b):
            arr.setflags(write=False)
        _scenes[(name, W, H)] = (*a, *b, tuple(float(F32(k)) for k in odo.intrinsics(W, H)), T)
    return _scenes[(name, W, H)]
