"""include/loop_closure.h restated in float64 numpy: Exp and Log of the header, the residual and the cost of a pose graph, the Jacobian
blocks of the header's linearisation, a scipy.optimize.least_squares solve of the SAME cost (the yardstick of the device's solver: it shares
no line of the method with it, its Jacobian is a central difference) and the map correction. Poses are [.., 12]: the rows of [R | t]."""
import numpy as np


def skew(v):
    v = np.asarray(v, np.float64)
    W = np.zeros(v.shape[:-1] + (3, 3))
    W[..., 0, 1], W[..., 0, 2], W[..., 1, 0], W[..., 1, 2], W[..., 2, 0], W[..., 2, 1] = -v[..., 2], v[..., 1], v[..., 2], -v[..., 0], -v[..., 1], v[..., 0]
    return W


def to44(X):
    X = np.asarray(X, np.float64).reshape(-1, 3, 4)
    out = np.zeros((X.shape[0], 4, 4))
    out[:, :3], out[:, 3, 3] = X, 1.0
    return out


def to12(T):
    return np.asarray(T, np.float64).reshape(-1, 4, 4)[:, :3].reshape(-1, 12)


def inv44(T):
    R, t = T[..., :3, :3], T[..., :3, 3]
    out = np.zeros_like(T)
    out[..., :3, :3] = np.swapaxes(R, -1, -2)
    out[..., :3, 3] = -np.einsum("...ji,...j->...i", R, t)
    out[..., 3, 3] = 1.0
    return out


def _abc(a):
    small = a < 1e-5
    s = np.where(small, 1.0, a)
    A = np.where(small, 1.0, np.sin(s) / s)
    B = np.where(small, 0.5, (1.0 - np.cos(s)) / (s * s))
    C = np.where(small, 1.0 / 6.0, (s - np.sin(s)) / (s * s * s))
    return A, B, C


def Exp(tau):
    """tau [.., 6] = (rho | theta) -> [.., 4, 4]: SE3_exp of slam/camera.py."""
    tau = np.asarray(tau, np.float64)
    rho, th = tau[..., :3], tau[..., 3:]
    a = np.linalg.norm(th, axis=-1)
    A, B, C = (v[..., None, None] for v in _abc(a))
    W = skew(th)
    W2 = W @ W
    I = np.eye(3)
    T = np.zeros(tau.shape[:-1] + (4, 4))
    T[..., :3, :3] = I + A * W + B * W2
    T[..., :3, 3] = np.einsum("...ij,...j->...i", I + B * W + C * W2, rho)
    T[..., 3, 3] = 1.0
    return T


def Log(T):
    """[.., 4, 4] -> [.., 6], the header's branches."""
    T = np.asarray(T, np.float64)
    R, t = T[..., :3, :3], T[..., :3, 3]
    ax = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    c = np.clip(0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0), -1.0, 1.0)
    s = 0.5 * np.linalg.norm(ax, axis=-1)
    a = np.arctan2(s, c)
    th_small = 0.5 * ax
    with np.errstate(divide="ignore", invalid="ignore"):
        th_mid = (a / (2.0 * np.where(s > 0, s, 1.0)))[..., None] * ax
        S = 0.5 * (R + np.swapaxes(R, -1, -2)) - c[..., None, None] * np.eye(3)
        diag = np.stack([R[..., 0, 0], R[..., 1, 1], R[..., 2, 2]], axis=-1)
        k = np.argmax(diag, axis=-1)                                       # the lowest index on a tie
        v = np.take_along_axis(S, k[..., None, None], axis=-1)[..., 0]
        n = np.linalg.norm(v, axis=-1)
        v = v / np.where(n > 0, n, 1.0)[..., None]
        v = np.where((np.einsum("...i,...i->...", v, ax) < 0)[..., None], -v, v)
        th_pi = a[..., None] * v
    th = np.where((a < 1e-5)[..., None], th_small, np.where((c > -0.99)[..., None], th_mid, th_pi))
    safe = np.where(a < 1e-5, 1.0, a)
    G = np.where(a < 1e-5, 1.0 / 12.0, (1.0 - 0.5 * safe * np.cos(0.5 * safe) / np.sin(0.5 * safe)) / (safe * safe))
    W = skew(th)
    Vinv = np.eye(3) - 0.5 * W + G[..., None, None] * (W @ W)
    return np.concatenate([np.einsum("...ij,...j->...i", Vinv, t), th], axis=-1)


# ---- the graph ---------------------------------------------------------------------------------------------------------------------
def usable_edges(nodes, edge_nodes, edge_Z, edge_w):
    """The header's rule: the mask of the edges that are used."""
    edge_nodes = np.asarray(edge_nodes).reshape(-1, 2)
    i, j = edge_nodes[:, 0], edge_nodes[:, 1]
    Z, w = np.asarray(edge_Z, np.float64).reshape(-1, 12), np.asarray(edge_w, np.float64).reshape(-1, 2)
    ok = (i >= 0) & (i < nodes) & (j >= 0) & (j < nodes) & (i != j)
    return ok & np.isfinite(Z).all(axis=1) & np.isfinite(w).all(axis=1) & (w >= 0).all(axis=1)


def residuals(X, edge_nodes, edge_Z):
    """r_e = Log(Z^-1 X_j X_i^-1), [E, 6]; X [N, 12]."""
    T = to44(X)
    e = np.asarray(edge_nodes).reshape(-1, 2)
    return Log(inv44(to44(edge_Z)) @ T[e[:, 1]] @ inv44(T[e[:, 0]]))


def cost(X, edge_nodes, edge_Z, edge_w):
    r, w = residuals(X, edge_nodes, edge_Z), np.asarray(edge_w, np.float64).reshape(-1, 2)
    return float(np.sum(w[:, 0] * np.sum(r[:, :3] ** 2, axis=1) + w[:, 1] * np.sum(r[:, 3:] ** 2, axis=1)))


def apply_delta(X, delta):
    """X_k <- Exp(delta_k) X_k."""
    return to12(Exp(np.asarray(delta).reshape(-1, 6)) @ to44(X))


def jinv(r):
    """Jinv(r) of the header, [.., 6, 6]: I - ad / 2 + ad^2 / 12 - ad^4 / 720."""
    r = np.asarray(r, np.float64)
    ad = np.zeros(r.shape[:-1] + (6, 6))
    ad[..., :3, :3] = ad[..., 3:, 3:] = skew(r[..., 3:])
    ad[..., :3, 3:] = skew(r[..., :3])
    ad2 = ad @ ad
    return np.eye(6) - 0.5 * ad + ad2 / 12.0 - (ad2 @ ad2) / 720.0


def adjoint(T):
    R, t = T[..., :3, :3], T[..., :3, 3]
    Ad = np.zeros(T.shape[:-2] + (6, 6))
    Ad[..., :3, :3] = Ad[..., 3:, 3:] = R
    Ad[..., :3, 3:] = skew(t) @ R
    return Ad


def jacobian_blocks(X, edge_nodes, edge_Z):
    """(A_i, A_j) of the header, each [E, 6, 6]."""
    r = residuals(X, edge_nodes, edge_Z)
    return -jinv(-r), jinv(r) @ adjoint(inv44(to44(edge_Z)))


def solve(X0, fixed, edge_nodes, edge_Z, edge_w):
    """The minimiser of the header's cost over the nodes that are not fixed, by scipy's trust-region least squares from X0 (broken edges dropped):
    the unknowns are delta with X_k = Exp(delta_k) X0_k, the Jacobian a central difference taken edge by edge. Returns (X [N, 12], cost)."""
    from scipy.optimize import least_squares
    X0 = np.asarray(X0, np.float64).reshape(-1, 12)
    N = X0.shape[0]
    keep = usable_edges(N, edge_nodes, edge_Z, edge_w)
    en, Z, w = np.asarray(edge_nodes).reshape(-1, 2)[keep], np.asarray(edge_Z, np.float64).reshape(-1, 12)[keep], np.asarray(edge_w, np.float64).reshape(-1, 2)[keep]
    touched = np.zeros(N, bool)
    touched[en[(w > 0).all(axis=1)].reshape(-1)] = True
    free = np.flatnonzero((np.asarray(fixed).reshape(-1) == 0) & touched)
    if free.size == 0 or en.shape[0] == 0:
        return X0.copy(), cost(X0, en, Z, w)
    column = -np.ones(N, np.int64)
    column[free] = np.arange(free.size)
    sw = np.sqrt(np.repeat(w, 3, axis=1))                                  # [E, 6]
    T0, Zinv = to44(X0), inv44(to44(Z))

    def edge_res(di, dj):
        return sw * Log(Zinv @ Exp(dj) @ T0[en[:, 1]] @ inv44(Exp(di) @ T0[en[:, 0]]))

    def full(x):
        d = np.zeros((N, 6))
        d[free] = x.reshape(-1, 6)
        return d

    def fun(x):
        d = full(x)
        return edge_res(d[en[:, 0]], d[en[:, 1]]).reshape(-1)

    def jac(x):
        d, h = full(x), 1e-6
        J = np.zeros((en.shape[0], 6, free.size * 6))
        for side in (0, 1):
            for c in range(6):
                step = np.zeros(6)
                step[c] = h
                di, dj = d[en[:, 0]], d[en[:, 1]]
                plus = edge_res(di + step, dj) if side == 0 else edge_res(di, dj + step)
                minus = edge_res(di - step, dj) if side == 0 else edge_res(di, dj - step)
                col = column[en[:, side]]
                rows = np.flatnonzero(col >= 0)
                J[rows, :, col[rows] * 6 + c] = ((plus - minus) / (2 * h))[rows]
        return J.reshape(-1, free.size * 6)

    x = np.zeros(free.size * 6)
    out = least_squares(fun, x, jac=jac, method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=200)
    X = apply_delta(X0, full(out.x))
    return X, cost(X, en, Z, w)


def correction(X_new, X_old):
    """D_k = X_new^-1 X_old in float64, [N, 12]."""
    return to12(inv44(to44(X_new)) @ to44(X_old))


# ---- the map correction ------------------------------------------------------------------------------------------------------------
def quat_of(R):
    """The header's unit quaternion (w, x, y, z) of one rotation matrix, float64."""
    R = np.asarray(R, np.float64)
    T = R[0, 0] + R[1, 1] + R[2, 2]
    if T > 0.0:
        s = 2.0 * np.sqrt(1.0 + T)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif R[0, 0] >= R[1, 1] and R[0, 0] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif R[1, 1] >= R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q) / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def hamilton(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def slots(kf_id, slot_of_frame, nodes):
    kf_id, table = np.asarray(kf_id, np.int64), np.asarray(slot_of_frame, np.int64).reshape(-1)
    inside = (kf_id >= 0) & (kf_id < table.size)
    s = np.where(inside, table[np.clip(kf_id, 0, max(table.size - 1, 0))] if table.size else -1, -1)
    return np.where((s < 0) | (s >= nodes), -1, s)


def map_correct(xyz, rotation, kf_id, slot_of_frame, D):
    """Float64 restatement of gsr_map_correct on float32 inputs: (xyz, rotation, moved mask, bar_xyz, bar_q) -- the exact results from the
    float32 D and the float32-rounded q_D, and the header's componentwise error bars 4 * 2^-24 * (|R| |x| + |t|) and its quaternion form."""
    D = np.asarray(D, np.float32).astype(np.float64).reshape(-1, 3, 4)
    x, q = np.asarray(xyz, np.float32).astype(np.float64), np.asarray(rotation, np.float32).astype(np.float64)
    s = slots(kf_id, slot_of_frame, D.shape[0])
    moved = s >= 0
    qD = np.stack([quat_of(Dk[:, :3]) for Dk in D]).astype(np.float32).astype(np.float64)
    sk = np.where(moved, s, 0)
    R, t = D[sk, :, :3], D[sk, :, 3]
    x_new = np.where(moved[:, None], np.einsum("nij,nj->ni", R, x) + t, x)
    q_new = np.where(moved[:, None], hamilton(qD[sk], q), q)
    u = 4.0 * 2.0 ** -24
    bar_x = u * (np.einsum("nij,nj->ni", np.abs(R), np.abs(x)) + np.abs(t))
    bar_q = u * _abs_product(np.abs(qD[sk]), np.abs(q))
    return x_new, q_new, moved, bar_x, bar_q


def _abs_product(a, b):
    """sum of |a_m| |b_n| over the four products of each component of the Hamilton product."""
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw + ax * bx + ay * by + az * bz, aw * bx + ax * bw + ay * bz + az * by,
                     aw * by + ax * bz + ay * bw + az * bx, aw * bz + ax * by + ay * bx + az * bw], axis=-1)


# ---- test graphs ---------------------------------------------------------------------------------------------------------------------
def ring(N, radius=2.0):
    """N world-to-camera poses on a circle, each looking at the centre with a tilt that changes along the way: [N, 12]."""
    out = []
    for k in range(N):
        a = 2.0 * np.pi * k / max(N, 1)
        c2w = Exp(np.array([0.0, 0.0, 0.0, 0.0, a, 0.0]))[None] @ Exp(np.array([radius, 0.1 * np.sin(3 * a), 0.0, 0.2 * np.sin(a), 0.0, 0.1 * np.cos(2 * a)]))[None]
        out.append(to12(inv44(c2w))[0])
    return np.stack(out)


def ring_edges(X, loops=None):
    """Exact odometry edges (k, k + 1) and loop edges of the poses X: the last node to the first, and every `loops`-th node to the one
    a third of the ring further on. Returns (edge_nodes int32 [E, 2], Z [E, 12])."""
    N = X.shape[0]
    pairs = [(k, k + 1) for k in range(N - 1)]
    if N > 2:
        pairs.append((N - 1, 0))
    if loops and N > 3:
        pairs += [(k, (k + N // 3) % N) for k in range(0, N, loops) if (k + N // 3) % N != k]
    en = np.asarray(pairs, np.int32).reshape(-1, 2)
    T = to44(X)
    return en, to12(T[en[:, 1]] @ inv44(T[en[:, 0]]))


def bend(X, eps):
    """X_k <- Exp(k eps) X_k: an accumulating drift."""
    k = np.arange(X.shape[0])[:, None]
    return apply_delta(X, k * np.asarray(eps, np.float64)[None])
