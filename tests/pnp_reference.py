"""gsr_feat_pose_pnp of include/feature_matching.h restated in numpy: the pose of frame B from the 3D points of frame A and the pixels of B.
What it shares with gsr_feat_pose comes from tests/features_reference.py (the draw, the triad, exp_apply, the scenes); the ranges are float64
numpy operations, one at a time, in the header's order; the refinement is float64. The device's counts, winner and stats equal these bit for
bit, its T to the last float32 digit or two (tests/test_hip_pnp.py)."""
import numpy as np

import features_reference as ref

F32, F64 = np.float32, np.float64
NEWTON = 8


def pair_list(kp_a, depth_a, kp_b, matches, K_a, K_b):
    """(P_a float32 [M, 3], the bearings u float32 [M, 3], uv float32 [M, 2], the slots a of the list); no depth of B"""
    H, W = depth_a.shape
    PA, U, UV, slots_a = [], [], [], []
    Ka, Kb = np.asarray(K_a, F32), np.asarray(K_b, F32)
    for a, (b, _) in enumerate(np.asarray(matches)):
        xa, ya = int(kp_a[a][0]), int(kp_a[a][1])
        if not (0 <= b < len(kp_b) and 0 <= xa < W and 0 <= ya < H):
            continue
        xb, yb = int(kp_b[b][0]), int(kp_b[b][1])
        if not (0 <= xb < W and 0 <= yb < H):
            continue
        za = F32(depth_a[ya, xa])
        if not (np.isfinite(za) and za > 0):
            continue
        PA.append([(F32(xa) - Ka[2]) * za / Ka[0], (F32(ya) - Ka[3]) * za / Ka[1], za])
        U.append([(F32(xb) - Kb[2]) / Kb[0], (F32(yb) - Kb[3]) / Kb[1], F32(1)])
        UV.append([F32(xb), F32(yb)])
        slots_a.append(a)
    shape = lambda v, k: np.asarray(v, F32).reshape(-1, k)
    return shape(PA, 3), shape(U, 3), shape(UV, 2), np.asarray(slots_a, np.int64)


def residuals(l1, l2, l3, c, d):
    """F1, F2, F3 of the pairs (1, 2), (1, 3), (2, 3)"""
    return (l1 * l1 + l2 * l2 - 2.0 * l1 * l2 * c[0] - d[0], l1 * l1 + l3 * l3 - 2.0 * l1 * l3 * c[1] - d[1],
            l2 * l2 + l3 * l3 - 2.0 * l2 * l3 * c[2] - d[2])


def ranges(P, U, start=None, steps=NEWTON):
    """The ranges of the header for triples P [..., 3 points, 3] (float32, frame A) and bearings U [..., 3, 3] (float32, frame B):
    (l float64 [..., 3], f float64 [..., 3, 3], valid [...]). start: other first ranges than |P_k| (the reach test alone)."""
    P, U = np.asarray(P, F32).astype(F64), np.asarray(U, F32).astype(F64)
    with np.errstate(all="ignore"):
        n = np.sqrt(U[..., 0] * U[..., 0] + U[..., 1] * U[..., 1] + U[..., 2] * U[..., 2])
        f = U / n[..., None]
        l = np.sqrt(P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1] + P[..., 2] * P[..., 2]) if start is None else np.asarray(start, F64)
        c, d = [], []
        for i, j in ((0, 1), (0, 2), (1, 2)):
            c.append(f[..., i, 0] * f[..., j, 0] + f[..., i, 1] * f[..., j, 1] + f[..., i, 2] * f[..., j, 2])
            D = P[..., i, :] - P[..., j, :]
            d.append(D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2])
        l1, l2, l3 = l[..., 0], l[..., 1], l[..., 2]
        valid = np.ones(l1.shape, bool)
        for _ in range(steps):
            F1, F2, F3 = residuals(l1, l2, l3, c, d)
            ja, jb = 2.0 * l1 - 2.0 * l2 * c[0], 2.0 * l2 - 2.0 * l1 * c[0]
            jc, jd = 2.0 * l1 - 2.0 * l3 * c[1], 2.0 * l3 - 2.0 * l1 * c[1]
            je, jg = 2.0 * l2 - 2.0 * l3 * c[2], 2.0 * l3 - 2.0 * l2 * c[2]
            det = -ja * jd * je - jb * jc * jg
            valid &= (det != 0.0) & np.isfinite(det)
            w = F2 * jg - jd * F3
            n1, n2, n3 = -F1 * jd * je - jb * w, ja * w - F1 * jc * jg, -ja * F2 * je - jb * jc * F3 + F1 * jc * je
            l1, l2, l3 = l1 - n1 / det, l2 - n2 / det, l3 - n3 / det
        F1, F2, F3 = residuals(l1, l2, l3, c, d)
        for lk in (l1, l2, l3):
            valid &= np.isfinite(lk) & (lk > 0.0)
        valid &= (np.abs(F1) <= 1e-9 * d[0]) & (np.abs(F2) <= 1e-9 * d[1]) & (np.abs(F3) <= 1e-9 * d[2])
    return np.stack([l1, l2, l3], axis=-1), f, valid


def draw(seed, count, M):
    """int64 [count, 3]: the indices of the hypotheses 0 .. count - 1 into a list of M >= 3 pairs (the draw of gsr_feat_pose)"""
    base = (np.uint64(seed) * np.uint64(0x9E3779B9) + 3 * np.arange(count, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    return np.stack([ref.lowbias32(base + np.uint64(k)) % np.uint64(M) for k in range(3)], axis=1).astype(np.int64)


def hypotheses(PA, U, seed, count, min_area):
    """(R float32 [count, 3, 3], t float32 [count, 3], valid [count]) of the hypotheses 0 .. count - 1"""
    M = len(PA)
    R, t = np.zeros((count, 3, 3), F32), np.zeros((count, 3), F32)
    if M < 3:
        return R, t, np.zeros(count, bool)
    idx = draw(seed, count, M)
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    a = PA[idx]                                                        # [count, 3 points, 3]
    l, f, found = ranges(a, U[idx])
    with np.errstate(all="ignore"):
        b = (l[..., None] * f).astype(F32)                             # Pb: every product rounded to float32 once
        valid &= found
        ea = ref.triad(a[:, 0], a[:, 1], a[:, 2], min_area)
        eb = ref.triad(b[:, 0], b[:, 1], b[:, 2], min_area)
        valid &= ea[3] & eb[3]
        ma, mb = (a[:, 0] + a[:, 1] + a[:, 2]) / F32(3), (b[:, 0] + b[:, 1] + b[:, 2]) / F32(3)
        for i in range(3):
            for j in range(3):
                R[:, i, j] = eb[0][:, i] * ea[0][:, j] + eb[1][:, i] * ea[1][:, j] + eb[2][:, i] * ea[2][:, j]
        for i in range(3):
            t[:, i] = mb[:, i] - (R[:, i, 0] * ma[:, 0] + R[:, i, 1] * ma[:, 1] + R[:, i, 2] * ma[:, 2])
    return R, t, valid


def inliers(R, t, PA, UV, K_b, tau_px):
    """bool [..., M]: the header's test in float32, the reprojection alone"""
    R, t, K = np.asarray(R, F32), np.asarray(t, F32), np.asarray(K_b, F32)
    tau_px = F32(tau_px)
    with np.errstate(all="ignore"):
        Q = [R[..., i, 0, None] * PA[:, 0] + R[..., i, 1, None] * PA[:, 1] + R[..., i, 2, None] * PA[:, 2] + t[..., i, None] for i in range(3)]
        ex = K[0] * (Q[0] / Q[2]) + K[2] - UV[:, 0]
        ey = K[1] * (Q[1] / Q[2]) + K[3] - UV[:, 1]
        return (Q[2] > 0) & (ex * ex + ey * ey <= tau_px * tau_px)


def refine(R, t, PA, UV, K_b, iters):
    """Gauss-Newton on the reprojection error, float64"""
    R, t = np.asarray(R, F64), np.asarray(t, F64)
    PA, UV = np.asarray(PA, F64), np.asarray(UV, F64)
    fx, fy, cx, cy = (float(F32(k)) for k in K_b)
    for _ in range(iters):
        q = PA @ R.T + t
        with np.errstate(all="ignore"):
            r = np.stack([fx * q[:, 0] / q[:, 2] + cx - UV[:, 0], fy * q[:, 1] / q[:, 2] + cy - UV[:, 1]], axis=1)
            dp = np.zeros((len(q), 2, 3))
            dp[:, 0, 0], dp[:, 0, 2] = fx / q[:, 2], -fx * q[:, 0] / (q[:, 2] * q[:, 2])
            dp[:, 1, 1], dp[:, 1, 2] = fy / q[:, 2], -fy * q[:, 1] / (q[:, 2] * q[:, 2])
        G = np.zeros((len(q), 3, 6))                                   # [I | -[q]x]
        G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1.0
        G[:, 0, 4], G[:, 0, 5] = q[:, 2], -q[:, 1]
        G[:, 1, 3], G[:, 1, 5] = -q[:, 2], q[:, 0]
        G[:, 2, 3], G[:, 2, 4] = q[:, 1], -q[:, 0]
        J = dp @ G
        Hm, g = np.einsum("nri,nrj->ij", J, J), np.einsum("nri,nr->i", J, r)
        if not (np.all(np.isfinite(Hm)) and np.all(np.isfinite(g))):
            break
        try:
            Lc = np.linalg.cholesky(Hm)
        except np.linalg.LinAlgError:
            break
        xi = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
        if not np.all(np.isfinite(xi)):
            break
        R, t = ref.exp_apply(xi, R, t)
    return R, t


def pose(kp_a, depth_a, kp_b, matches, K_a, K_b, seed=0, count=256, min_area=0.05, tau_px=2.0, refine_iters=3, min_matches=12, min_inliers=8,
         min_share=0.5, max_translation=1.5, max_rotation=np.deg2rad(45.0)):
    """{"T" float32 [4, 4], "stats" int32 [8], "counts" int32 [count], "T_refined" float64 [4, 4] or None (the pose before the gate)}"""
    PA, U, UV, _ = pair_list(kp_a, np.asarray(depth_a, F32), kp_b, matches, K_a, K_b)
    M = len(PA)
    R, t, valid = hypotheses(PA, U, seed, count, min_area)
    counts = np.where(valid, inliers(R, t, PA, UV, K_b, tau_px).sum(axis=-1), 0).astype(np.int32) if M else np.zeros(count, np.int32)
    winner = int(np.argmax(counts))                                    # the first of the largest: the lowest h
    stats = np.array([(np.asarray(kp_a)[:, 0] >= 0).sum(), (np.asarray(kp_b)[:, 0] >= 0).sum(), M, winner, counts[winner], 0, 0, 0], np.int32)
    T, refined = np.eye(4, dtype=F32), None
    if counts[winner] >= 3:
        keep = inliers(R[winner], t[winner], PA, UV, K_b, tau_px)
        R64, t64 = refine(R[winner], t[winner], PA[keep], UV[keep], K_b, refine_iters)
        R32, t32 = R64.astype(F32), t64.astype(F32)
        final = int(inliers(R32, t32, PA, UV, K_b, tau_px).sum())
        refined = np.eye(4)
        refined[:3, :3], refined[:3, 3] = R64, t64
        Rd, td = R32.astype(F64), t32.astype(F64)
        ax = np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
        angle = np.arctan2(0.5 * np.sqrt(ax @ ax), 0.5 * (np.trace(Rd) - 1.0))
        accepted = (np.all(np.isfinite(R32)) and np.all(np.isfinite(t32)) and M >= min_matches and final >= min_inliers and
                    final >= float(F32(min_share)) * M and np.sqrt(td @ td) <= float(F32(max_translation)) and angle <= float(F32(max_rotation)))
        stats[5], stats[6] = final, int(accepted)
        if accepted:
            T[:3, :3], T[:3, 3] = R32, t32
    return {"T": T, "stats": stats, "counts": counts, "T_refined": refined}
