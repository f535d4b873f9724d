"""The stereo matcher's contract (include/stereo_depth.h) restated in integer numpy, and the planted-pair generator the stereo tests share.

The paths are walked pixel by pixel, vectorised over the disparities (and over the paths of one direction that advance together). Where
the header is silent this file decides:
  * the census bit order (irrelevant: only popcounts of xors are used);
  * the order of the eight directions (irrelevant: S is an integer sum);
  * dR's candidates are all d in [0, D) with x' + d < W, whether or not that d is itself a valid match of pixel x' + d;
  * the uniqueness scan looks at every d in [0, D) outside [d* - 1, d* + 1], including those with x - d < 0 (their C is 62);
  * the tests of a pixel are independent: a pixel that fails one is -16 whatever the others say.
"""
import numpy as np

CENSUS_BITS = 62
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))
DEFAULTS = dict(num_disparities=64, p1=10, p2=120, uniqueness_ratio=40, disp12_max_diff=1)


def census(img):
    """uint64 [H, W]: one bit per neighbour of the 9 x 7 window (centre excluded), set where neighbour < centre; coordinates clamped."""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    ys, xs = np.arange(H), np.arange(W)
    code = np.zeros((H, W), np.uint64)
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dy == 0 and dx == 0:
                continue
            nb = img[np.clip(ys + dy, 0, H - 1)[:, None], np.clip(xs + dx, 0, W - 1)[None, :]]
            code = (code << np.uint64(1)) | (nb < img).astype(np.uint64)
    return code


def popcount64(v):
    v = np.asarray(v, np.uint64)
    n = np.zeros(v.shape, np.int64)
    for k in range(8):
        n += _POP8[((v >> np.uint64(8 * k)) & np.uint64(255)).astype(np.int64)]
    return n


_POP8 = np.array([bin(k).count("1") for k in range(256)], np.int64)


def cost_volume(left, right, D):
    """C [H, W, D] int64: popcount(cL(x, y) xor cR(x - d, y)) for x - d >= 0, 62 otherwise."""
    cl, cr = census(left), census(right)
    H, W = cl.shape
    C = np.full((H, W, D), CENSUS_BITS, np.int64)
    for d in range(min(D, W)):
        C[:, d:, d] = popcount64(cl[:, d:] ^ cr[:, :W - d])
    return C


def _step(C_p, L_q, p1, p2):
    """L_r(p, .) from L_r(q, .) for any leading shape [..., D]."""
    big = np.iinfo(np.int64).max // 4
    m = L_q.min(axis=-1, keepdims=True)
    below = np.concatenate([np.full_like(L_q[..., :1], big), L_q[..., :-1]], -1)      # L_r(q, d - 1); absent at d = 0
    above = np.concatenate([L_q[..., 1:], np.full_like(L_q[..., :1], big)], -1)       # L_r(q, d + 1); absent at d = D - 1
    return C_p + np.minimum(np.minimum(L_q, m + p2), np.minimum(below, above) + p1) - m


def aggregate_direction(C, dx, dy, p1, p2):
    """L_r [H, W, D] of one direction r = (dx, dy): a pixel whose predecessor p - r is outside the image starts a path with L = C."""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for k, x in enumerate(xs):
            L[:, x] = C[:, x] if k == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for k, y in enumerate(ys):
        if k == 0:
            L[y] = C[y]
            continue
        xq = np.arange(W) - dx                                   # the predecessor's column
        inside = (xq >= 0) & (xq < W)
        L[y] = C[y]                                              # a diagonal that came in through a side border starts here
        L[y, inside] = _step(C[y, inside], L[y - dy, xq[inside]], p1, p2)
    return L


def aggregate(C, p1, p2):
    """S [H, W, D] = the sum of L_r over the eight directions."""
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS:
        S += aggregate_direction(C, dx, dy, p1, p2)
    return S


def trunc_div(a, b):
    """C's integer division (truncation towards zero), b > 0."""
    a, b = int(a), int(b)
    return -((-a) // b) if a < 0 else a // b


def select(S, uniqueness_ratio, disp12_max_diff):
    """disparity16 int16 [H, W] from an aggregated (or raw) volume S, by the header's selection rules."""
    S = np.asarray(S, np.int64)
    H, W, D = S.shape
    best = S.argmin(-1)                                           # numpy's argmin is the first minimum
    ds = np.arange(D)
    right = np.zeros((H, W), np.int64)                            # dR(x', y)
    for x in range(W):
        n = min(D, W - x)
        right[:, x] = S[:, x + ds[:n], ds[:n]].argmin(-1)
    out = np.full((H, W), -16, np.int16)
    for y in range(H):
        for x in range(W):
            d, s = int(best[y, x]), S[y, x]
            if x - d < 0:
                continue
            far = np.abs(ds - d) > 1
            if np.any(s[far] * (100 - uniqueness_ratio) < s[d] * 100):
                continue
            if disp12_max_diff >= 0 and abs(int(right[y, x - d]) - d) > disp12_max_diff:
                continue
            v = 16 * d
            if 0 < d < D - 1:
                den = max(int(s[d - 1] + s[d + 1] - 2 * s[d]), 1)
                v += trunc_div((int(s[d - 1]) - int(s[d + 1])) * 16 + den, 2 * den)
            out[y, x] = v
    return out


def depth_from_disparity(disparity16, bf):
    """float32(16 bf) / float32(disparity16) where disparity16 > 0, else 0: one float32 division."""
    d = np.asarray(disparity16).astype(np.float32)
    bf16 = np.float32(float(bf) * 16.0)
    out = np.zeros(d.shape, np.float32)
    np.divide(bf16, d, out=out, where=d > 0)
    return out


def match(left, right, num_disparities=64, p1=10, p2=120, uniqueness_ratio=40, disp12_max_diff=1, aggregated=True):
    """(disparity16 int16 [H, W], S uint16 [H, W, D]). aggregated=False is winner-take-all on the raw cost under the same selection."""
    C = cost_volume(left, right, num_disparities)
    S = aggregate(C, p1, p2) if aggregated else C
    return select(S, uniqueness_ratio, disp12_max_diff), S.astype(np.uint16)


# ---- the planted pair -----------------------------------------------------------------------------------------------------------------
def _texture(rng, h, w):
    """Uniform noise, box-blurred 5 x 5 (edge-replicated), stretched to 40 .. 210."""
    t = np.pad(rng.uniform(0.0, 1.0, (h, w)), 2, mode="edge")
    b = sum(t[i:i + h, j:j + w] for i in range(5) for j in range(5)) / 25.0
    return 40.0 + (b - b.min()) / (b.max() - b.min()) * 170.0


def planted_pair(height=48, width=112, seed=0, background=5, foreground=20, gain=0.9, offset=10.0, sigma=4.0):
    """(left u8, right u8, truth int [H, W], evaluated bool [H, W]): a fronto-parallel background at disparity `background` and a central
    rectangle (rows H/4 .. 3H/4, columns W/3 .. 2W/3 of the left image) at `foreground`. The right image has gain and offset, both have
    independent Gaussian noise. `evaluated` leaves out the left pixels hidden in the right view and those with x - d < 0."""
    rng = np.random.default_rng(seed)
    H, W = height, width
    back, front = _texture(rng, H, W + foreground), _texture(rng, H, W + foreground)      # indexed by the LEFT image's column
    ys, xs = np.mgrid[0:H, 0:W]
    in_rect = lambda y, x: (y >= H // 4) & (y < 3 * H // 4) & (x >= W // 3) & (x < 2 * W // 3)
    rect = in_rect(ys, xs)
    truth = np.where(rect, foreground, background)
    left = np.where(rect, front[ys, xs], back[ys, xs])
    front_r = in_rect(ys, xs + foreground)                                             # right pixels that show the rectangle
    right = np.where(front_r, front[ys, xs + foreground], back[ys, xs + background])
    xr = xs - truth
    hidden = ~rect & (xr >= 0) & in_rect(ys, np.maximum(xr, 0) + foreground)             # background behind the rectangle in the right view
    evaluated = (xr >= 0) & ~hidden
    left = left + rng.normal(0.0, sigma, (H, W))
    right = gain * right + offset + rng.normal(0.0, sigma, (H, W))
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to_u8(left), to_u8(right), truth, evaluated


def quality(disparity16, truth, evaluated):
    """(density, bad share): valid pixels among the evaluated ones, and among those the share more than one pixel off the truth."""
    valid = (np.asarray(disparity16) >= 0) & evaluated
    density = valid.sum() / max(int(evaluated.sum()), 1)
    err = np.abs(np.asarray(disparity16, np.float64) / 16.0 - truth)
    bad = (err[valid] > 1.0).sum() / max(int(valid.sum()), 1)
    return float(density), float(bad)
