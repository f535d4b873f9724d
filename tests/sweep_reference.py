"""The plane sweep's contract (include/multiview_depth.h) restated in numpy -- integer for the matching, float32 element by element for the
projection -- and the planted scene the sweep tests share. Census, popcount, the eight-path aggregation and the truncating division are
the stereo matcher's (tests/stereo_reference.py): the sweep only forms another cost volume and selects under other validity rules.

Every float32 step below is ONE numpy operation on float32 arrays, in the header's order, so that each rounds once as the kernel's
uncontracted operators do. Where the header is silent this file decides:
  * the uniqueness scan looks at every k in [0, 64) outside [k* - 1, k* + 1], visible or not;
  * the three validity tests of a pixel are independent: a pixel that fails one is -16 whatever the others say;
  * a comparison with NaN is false (an overflowing transform makes a hypothesis invisible); the larger of the two spans is
    `du > dv ? du : dv`, so a NaN in du yields dv and a NaN in dv fails the test.
"""
import numpy as np

from stereo_reference import _texture, aggregate, census, popcount64, trunc_div

D = 64
INVISIBLE = 62
DEFAULTS = dict(p1=10, p2=120, uniqueness_ratio=40, min_span_px=8)
F = np.float32


def project(H, W, K, transform, w_min, w_step):
    """(visible bool [H, W, 64], xq int [H, W, 64], yq int [H, W, 64], up float32 [H, W, 64], vp float32 [H, W, 64], in front bool
    [H, W, 64]) of one partner; transform: 12 floats, row-major [R | t], reference camera to partner camera. xq / yq are 0 where the hypothesis is not visible."""
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(transform, F).reshape(3, 4)
    v, u = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    w = F(w_min) + np.arange(D, dtype=F) * F(w_step)                                  # w_k = w_min + float(k) * w_step
    with np.errstate(all="ignore"):
        rx = (u - cx) / fx
        ry = (v - cy) / fy
        X = []
        for i in range(3):
            a = (T[i, 0] * rx + T[i, 1] * ry) + T[i, 2]
            X.append(a[..., None] + T[i, 3] * w)                                         # [H, W, 64]
        up = fx * (X[0] / X[2]) + cx
        vp = fy * (X[1] / X[2]) + cy
        visible = (X[2] > F(1e-6)) & (up >= F(-0.5)) & (up < F(W) - F(0.5)) & (vp >= F(-0.5)) & (vp < F(H) - F(0.5))
        xq = np.where(visible, np.floor(np.where(visible, up, F(0)) + F(0.5)), 0).astype(np.int64)
        yq = np.where(visible, np.floor(np.where(visible, vp, F(0)) + F(0.5)), 0).astype(np.int64)
    return visible, xq, yq, up.astype(F), vp.astype(F), X[2] > F(1e-6)


def cost_volume(ref_grey, partners, K, transforms, w_min, w_step, min_span_px):
    """(C int64 [H, W, 64], observable bool [H, W])."""
    code_ref = census(ref_grey)
    H, W = code_ref.shape
    C = np.zeros((H, W, D), np.int64)
    observable = np.zeros((H, W), bool)
    for img, T in zip(partners, np.asarray(transforms, F).reshape(-1, 12)):
        code = census(img)
        visible, xq, yq, up, vp, front = project(H, W, K, T, w_min, w_step)
        C += np.where(visible, popcount64(code_ref[..., None] ^ code[yq, xq]), INVISIBLE)
        with np.errstate(all="ignore"):
            du, dv = np.abs(up[..., 63] - up[..., 0]), np.abs(vp[..., 63] - vp[..., 0])
            span = np.where(du > dv, du, dv)
            observable |= front[..., 0] & front[..., 63] & (np.trunc(span) >= F(min_span_px))
    return C, observable


def select(S, observable, uniqueness_ratio):
    """index16 int16 [H, W]: 16 k* + the parabola term, -16 where the pixel is invalid."""
    S = np.asarray(S, np.int64)
    H, W, _ = S.shape
    best = S.argmin(-1)                                            # the first minimum
    ks = np.arange(D)
    out = np.full((H, W), -16, np.int16)
    for y in range(H):
        for x in range(W):
            k, s = int(best[y, x]), S[y, x]
            if not observable[y, x] or k == 0 or k == D - 1:
                continue
            if np.any(s[np.abs(ks - k) > 1] * (100 - uniqueness_ratio) < s[k] * 100):
                continue
            den = max(int(s[k - 1] + s[k + 1] - 2 * s[k]), 1)
            out[y, x] = 16 * k + trunc_div((int(s[k - 1]) - int(s[k + 1])) * 16 + den, 2 * den)
    return out


def depth_from_index(index16, w_min, w_step):
    """1 / (w_min + (float(index16) / 16) * w_step) where index16 >= 0, else 0; four float32 operations."""
    i = np.asarray(index16).astype(F)
    with np.errstate(all="ignore"):
        d = F(1) / (F(w_min) + (i / F(16)) * F(w_step))
    return np.where(np.asarray(index16) >= 0, d, F(0)).astype(F)


def sweep(ref_grey, partners, K, transforms, w_min, w_step, p1=10, p2=120, uniqueness_ratio=40, min_span_px=8, aggregated=True):
    """{"cost" u8 [H, W, 64], "cost_sum" u16 [H, W, 64], "index16" i16 [H, W], "depth" f32 [H, W], "observable" bool [H, W]}.
    aggregated=False is winner-take-all on the raw cost under the same selection."""
    C, observable = cost_volume(ref_grey, partners, K, transforms, w_min, w_step, min_span_px)
    S = aggregate(C, p1, p2) if aggregated else C
    index16 = select(S, observable, uniqueness_ratio)
    return {"cost": C.astype(np.uint8), "cost_sum": S.astype(np.uint16), "index16": index16, "depth": depth_from_index(index16, w_min, w_step),
            "observable": observable}


# ---- the planted scene ----------------------------------------------------------------------------------------------------------------
PLANTED_K = (100.0, 100.0, 55.5, 23.5)
PLANTED_BASELINE = 0.16
PLANTED_W_MIN, PLANTED_W_STEP = 0.0, 1.0 / 32.0
PLANTED_SHIFTS = {"right": (0, 1), "down": (1, 0), "left": (0, -1)}              # (rows, columns) per pixel of shift
MARGIN = 24


def planted_transform(name, baseline=PLANTED_BASELINE):
    """[R | t] with R = I: the partner's camera centre lies `baseline` to the right of / below / to the left of the reference's."""
    dy, dx = PLANTED_SHIFTS[name]
    T = np.zeros((3, 4), F)
    T[:, :3] = np.eye(3, dtype=F)
    T[0, 3], T[1, 3] = -baseline * dx, -baseline * dy
    return T.reshape(12)


def planted_scene(partners=("right", "down"), height=48, width=112, seed=0, background=5, foreground=20, gain=0.9, offset=10.0, sigma=4.0):
    """(ref u8 [H, W], partner images u8 [J, H, W], transforms f32 [J, 12], truth int [H, W]): a fronto-parallel background whose image
    moves by `background` pixels between the reference and a partner, and a central rectangle (rows H/4 .. 3H/4, columns W/3 .. 2W/3 of the
    reference view) that moves by `foreground`. With PLANTED_K, PLANTED_BASELINE and PLANTED_W_STEP a shift of s pixels is hypothesis
    2 s, so truth is 10 and 40. The partners have gain and offset, every image its own Gaussian noise."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    back, front = _texture(rng, H + 2 * MARGIN, W + 2 * MARGIN), _texture(rng, H + 2 * MARGIN, W + 2 * MARGIN)
    ys, xs = np.mgrid[0:H, 0:W]
    in_rect = lambda y, x: (y >= H // 4) & (y < 3 * H // 4) & (x >= W // 3) & (x < 2 * W // 3)
    tex = lambda t, y, x: t[y + MARGIN, x + MARGIN]
    rect = in_rect(ys, xs)
    truth = np.where(rect, 2 * foreground, 2 * background)
    ref = np.where(rect, tex(front, ys, xs), tex(back, ys, xs)) + rng.normal(0.0, sigma, (H, W))
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    images = []
    for name in partners:
        dy, dx = PLANTED_SHIFTS[name]
        yf, xf = ys + dy * foreground, xs + dx * foreground
        yb, xb = ys + dy * background, xs + dx * background
        img = np.where(in_rect(yf, xf), tex(front, yf, xf), tex(back, yb, xb))
        images.append(to_u8(gain * img + offset + rng.normal(0.0, sigma, (H, W))))
    return to_u8(ref), np.stack(images), np.stack([planted_transform(n) for n in partners]), truth


def quality(index16, truth):
    """(valid share of all pixels, share of the valid pixels more than 2 hypotheses from the truth)."""
    index16 = np.asarray(index16)
    valid = index16 >= 0
    err = np.abs(index16.astype(np.float64) / 16.0 - truth)
    return float(valid.mean()), float((err[valid] > 2.0).sum() / max(int(valid.sum()), 1))
