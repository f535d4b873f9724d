"""include/motion_segmentation.h restated in float64 numpy and scipy.ndimage: ``fit`` (gsr_flow_rigid_fit: the cutoff of a pass comes from
the residuals of that same pass), ``clean`` (gsr_motion_mask_clean), ``candidate`` and ``segment`` (both with the candidate rule between
them), plus the analytic scene the tests fit: a slanted wall, a floor and a sphere that moves on its own, seen by a camera that moves by
a known twist. Not a test module; imported by tests/test_motion_host.py and tests/test_hip_motion.py."""
import numpy as np
from scipy import ndimage

BINS, BINS_PER_PX, MIN_Z, BEHIND = 1024, 16.0, 1e-3, 3.0e38
TWIST = np.array([0.03, -0.01, 0.02, 0.004, -0.0175, 0.003])      # the analytic scene's camera motion, [rho | theta]
SPHERE_CENTRE = np.array([-0.3, 0.1, 1.9])
SPHERE_SHIFT = np.array([0.06, -0.02, 0.015])
DEFAULTS = dict(iters=10, scale_multiplier=2.0, c_min=1.0, c_max=16.0, residual_px=1.0, occlusion_px=1.0, open_radius=1, min_area=64,
                grow_radius=2)


def skew(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp of xi = [rho | theta] as a 4 x 4 (slam/camera.py SE3_exp in float64)."""
    xi = np.asarray(xi, np.float64)
    K = skew(xi[3:])
    K2 = K @ K
    th = float(np.linalg.norm(xi[3:]))
    A, B, C = (1.0, 0.5, 1.0 / 6.0) if th < 1e-5 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * K2
    T[:3, 3] = (np.eye(3) + B * K + C * K2) @ xi[:3]
    return T


def pixel_grid(W, H):
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return u, v


def bilinear(f, x, y):
    """f [H, W, 2] at (x, y) inside the image; the neighbour past the last row / column is the last one."""
    H, W = f.shape[:2]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    ax, ay = (x - x0)[..., None], (y - y0)[..., None]
    return (1 - ay) * ((1 - ax) * f[y0, x0] + ax * f[y0, x1]) + ay * ((1 - ax) * f[y1, x0] + ax * f[y1, x1])


def usable_pixels(flow_ij, depth, flow_ji=None, occlusion_px=1.0):
    """(usable [H, W] bool, target x, target y)."""
    flow_ij, depth = np.asarray(flow_ij, np.float64), np.asarray(depth, np.float64)
    H, W = depth.shape
    u, v = pixel_grid(W, H)
    with np.errstate(invalid="ignore"):
        px, py = flow_ij[..., 0] * (W / 2), flow_ij[..., 1] * (H / 2)
        tx, ty = u + px, v + py
        ok = (depth > 0) & np.isfinite(depth) & np.isfinite(px) & np.isfinite(py) & (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
        if flow_ji is not None:
            back = bilinear(np.asarray(flow_ji, np.float64), np.where(ok, tx, 0.0), np.where(ok, ty, 0.0))
            sx, sy = px + back[..., 0] * (W / 2), py + back[..., 1] * (H / 2)
            ok &= np.isfinite(sx) & np.isfinite(sy) & (np.hypot(sx, sy) <= occlusion_px)
    return ok, tx, ty


def residuals(T, depth, K, tx, ty):
    """(Y [H, W, 3], r [H, W, 2], e [H, W]) under T; e = BEHIND where Y_z <= MIN_Z."""
    fx, fy, cx, cy = K
    H, W = depth.shape
    u, v = pixel_grid(W, H)
    X = np.stack([(u - cx) / fx * depth, (v - cy) / fy * depth, depth], -1)
    Y = X @ T[:3, :3].T + T[:3, 3]
    front = Y[..., 2] > MIN_Z
    z = np.where(front, Y[..., 2], 1.0)
    r = np.stack([fx * Y[..., 0] / z + cx - tx, fy * Y[..., 1] / z + cy - ty], -1)
    e = np.where(front, np.hypot(r[..., 0], r[..., 1]), BEHIND)
    return Y, r, e, front


def median_bin(e):
    """The first bin of the 1/16 px histogram whose cumulative count reaches (n + 1) // 2; 0 for no residuals."""
    if e.size == 0:
        return 0
    bins = np.minimum(np.floor(np.minimum(e, 1e6) * BINS_PER_PX), BINS - 1).astype(np.int64)
    cum = np.cumsum(np.bincount(bins, minlength=BINS))
    return int(np.searchsorted(cum, (e.size + 1) // 2, side="left"))


def cutoff(b, scale_multiplier, c_min, c_max):
    return float(np.clip(scale_multiplier * 1.4826 * (b + 1) / BINS_PER_PX, c_min, c_max))


def fit(flow_ij, depth, K, flow_ji=None, fit_mask=None, T_init=None, iters=10, scale_multiplier=2.0, c_min=1.0, c_max=16.0, occlusion_px=1.0):
    """The fit of include/motion_segmentation.h. Returns a dict: T [4, 4], residual [H, W] (-1 = not usable), c (the final cutoff), usable
    and fit (bool [H, W]), and trace: per pass a dict with sums [30] (21 of H, 6 of g, sum w, sum w e^2, pixels with w > 0), abs_sums [30]
    (the sums of the absolute values of the same terms), bin, c and e (the residuals of the fit set in that pass)."""
    depth = np.asarray(depth, np.float64)
    usable, tx, ty = usable_pixels(flow_ij, depth, flow_ji, occlusion_px)
    sel = usable & (np.ones_like(usable) if fit_mask is None else np.asarray(fit_mask).astype(bool))
    T = np.eye(4) if T_init is None else np.asarray(T_init, np.float64).copy()
    fx, fy = K[0], K[1]
    iu = np.triu_indices(6)
    trace = []
    for _ in range(iters):
        Y, r, e, front = residuals(T, depth, K, tx, ty)
        Y, r, e, front = Y[sel], r[sel], e[sel], front[sel]
        b = median_bin(e)
        c = cutoff(b, scale_multiplier, c_min, c_max)
        w = np.where(front & (e < c), (1 - np.minimum(e / c, 1.0) ** 2) ** 2, 0.0)
        z = np.where(front, Y[:, 2], 1.0)
        a, bb, xz, yz = fx / z, fy / z, Y[:, 0] / z, Y[:, 1] / z
        zero = np.zeros_like(a)
        J0 = np.stack([a, zero, -a * xz, -a * xz * Y[:, 1], a * (Y[:, 2] + xz * Y[:, 0]), -a * Y[:, 1]], -1)          # d r_x / d xi, [N, 6]
        J1 = np.stack([zero, bb, -bb * yz, -bb * (Y[:, 2] + yz * Y[:, 1]), bb * yz * Y[:, 0], bb * Y[:, 0]], -1)     # d r_y / d xi
        JtJ = J0[:, iu[0]] * J0[:, iu[1]] + J1[:, iu[0]] * J1[:, iu[1]]
        terms = np.concatenate([w[:, None] * JtJ, w[:, None] * (J0 * r[:, :1] + J1 * r[:, 1:]), w[:, None],
                                (w * np.where(front, e, 0.0) ** 2)[:, None], (w > 0).astype(np.float64)[:, None]], 1)
        sums, abs_sums = terms.sum(0), np.abs(terms).sum(0)
        trace.append({"sums": sums, "abs_sums": abs_sums, "bin": b, "c": c, "e": e})
        Hm = np.zeros((6, 6))
        Hm[iu] = sums[:21]
        Hm = Hm + np.triu(Hm, 1).T
        A = Hm + 1e-9 * np.trace(Hm) / 6 * np.eye(6)
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            continue
        xi = np.linalg.solve(L.T, np.linalg.solve(L, -sums[21:27]))
        T = se3_exp(xi) @ T
    _, _, e, _ = residuals(T, depth, K, tx, ty)
    c = cutoff(median_bin(e[sel]), scale_multiplier, c_min, c_max)
    return {"T": T, "residual": np.where(usable, e, -1.0), "c": c, "usable": usable, "fit": sel, "trace": trace}


def candidate(residual, usable, c, residual_px=1.0):
    return usable & (residual > max(residual_px, c))


def canonical_labels(mask):
    """8-connected components of a bool image: int32 [H, W], -1 for background, else the smallest linear index of the component."""
    lab, n = ndimage.label(mask, np.ones((3, 3), dtype=int))
    out = np.full(mask.shape, -1, np.int32)
    if n:
        first = ndimage.minimum(np.arange(mask.size).reshape(mask.shape), lab, np.arange(1, n + 1)).astype(np.int32)
        out[lab > 0] = first[lab[lab > 0] - 1]
    return out, n


def clean(cand, open_radius=1, grow_radius=2, min_area=64):
    """(moving bool [H, W], labels int32 [H, W], counts [4]) of gsr_motion_mask_clean."""
    m = np.asarray(cand).astype(bool)
    square = lambda r: np.ones((2 * r + 1, 2 * r + 1), dtype=bool)
    m = ndimage.binary_dilation(ndimage.binary_erosion(m, square(open_radius)), square(open_radius))
    labels, found = canonical_labels(m)
    keep = np.zeros(m.size, dtype=bool)
    roots, areas = np.unique(labels[labels >= 0], return_counts=True)
    keep[roots[areas >= min_area]] = True
    kept = (labels >= 0) & keep[np.maximum(labels, 0)]
    labels = np.where(kept, labels, -1).astype(np.int32)
    moving = ndimage.binary_dilation(kept, square(grow_radius))
    return moving, labels, np.array([found, int((areas >= min_area).sum()), int(kept.sum()), int(moving.sum())], np.int32)


def segment(flow_ij, depth, K, flow_ji=None, motion=None, T_init=None, **params):
    """fit, the candidate rule and clean with FlowMotionSegmenter's parameters (DEFAULTS overridden by params)."""
    p = dict(DEFAULTS, **params)
    f = fit(flow_ij, depth, K, flow_ji=flow_ji, fit_mask=motion, T_init=T_init,
            **{k: p[k] for k in ("iters", "scale_multiplier", "c_min", "c_max", "occlusion_px")})
    cand = candidate(f["residual"], f["usable"], f["c"], p["residual_px"])
    moving, labels, counts = clean(cand, p["open_radius"], p["grow_radius"], p["min_area"])
    return dict(f, candidate=cand, moving=moving, labels=labels, counts=counts)


def intrinsics(W):
    """TUM fr3 scaled by W / 640."""
    s = W / 640.0
    return (535.4 * s, 539.2 * s, 320.1 * s, 247.6 * s)


def analytic_scene(W, H, radius, seed, noise_px=0.2, holes=0.05, twist=TWIST):
    """A wall z = 3 / (1 - 0.3 x / z), a floor at y = 0.8 and a sphere of `radius` at SPHERE_CENTRE seen from camera i; camera j = exp(twist)
    camera i, and the sphere's points are displaced by SPHERE_SHIFT (in camera i's frame) in between. Returns flow_ij float32 [H, W, 2] in
    NDC units with Gaussian noise of noise_px, depth float32 [H, W] with a share `holes` of zeros, K, T_true and the sphere's pixels."""
    rng = np.random.default_rng(seed)
    K = intrinsics(W)
    fx, fy, cx, cy = K
    u, v = pixel_grid(W, H)
    a, b = (u - cx) / fx, (v - cy) / fy
    z = 3.0 / (1.0 - 0.3 * a)
    with np.errstate(divide="ignore", invalid="ignore"):
        zf = np.where(b > 0, 0.8 / b, np.inf)
    z = np.minimum(z, zf)
    dd, dc = a * a + b * b + 1.0, a * SPHERE_CENTRE[0] + b * SPHERE_CENTRE[1] + SPHERE_CENTRE[2]
    disc = dc * dc - dd * (SPHERE_CENTRE @ SPHERE_CENTRE - radius ** 2)
    zs = np.where(disc >= 0, (dc - np.sqrt(np.maximum(disc, 0.0))) / dd, np.inf)
    sphere = (zs > 0) & (zs < z)
    z = np.where(sphere, zs, z)
    X = np.stack([a * z, b * z, z], -1) + sphere[..., None] * SPHERE_SHIFT
    T = se3_exp(twist)
    Y = X @ T[:3, :3].T + T[:3, 3]
    flow_px = np.stack([fx * Y[..., 0] / Y[..., 2] + cx - u, fy * Y[..., 1] / Y[..., 2] + cy - v], -1) + rng.normal(0.0, noise_px, (H, W, 2))
    depth = np.where(rng.random((H, W)) < holes, 0.0, z)
    flow = (flow_px * np.array([2.0 / W, 2.0 / H])).astype(np.float32)
    return {"flow_ij": flow, "depth": depth.astype(np.float32), "K": K, "T_true": T, "sphere": sphere}


def pose_error(T, T_true):
    """(translation error in metres, rotation error in radians) of T against T_true."""
    D = np.asarray(T, np.float64) @ np.linalg.inv(T_true)
    S = (D[:3, :3] - D[:3, :3].T) / 2                # sin(angle) * axis: exact for small angles, where arccos of the trace loses a float32 T
    return float(np.linalg.norm(D[:3, 3])), float(np.arcsin(min(1.0, np.linalg.norm([S[2, 1], S[0, 2], S[1, 0]]))))


def mask_scores(moving, truth, halo=3):
    """(recall of the true pixels, share of the frame that is marked moving outside the truth dilated by (2 halo + 1)^2)."""
    moving, truth = np.asarray(moving).astype(bool), np.asarray(truth).astype(bool)
    wide = ndimage.binary_dilation(truth, np.ones((2 * halo + 1, 2 * halo + 1), dtype=bool))
    return float((moving & truth).sum() / max(int(truth.sum()), 1)), float((moving & ~wide).sum() / moving.size)
