"""include/relocalisation.h restated in numpy: the fern code of a frame, the search of a code in a database, the verdict counts. Integers
throughout; where floats occur (the two quantisations, the depth test of the score) every operation is a float32 numpy operation, one at a
time, as the header states them. The device's outputs equal these bit for bit (tests/test_hip_relocalise.py)."""
import numpy as np

F32 = np.float32


def quant(v):
    """q(v) = (int)(min(max(v, 0), 1) * 255.0f + 0.5f); a NaN gives 0."""
    v = np.asarray(v, F32)
    c = np.where(v > F32(0), v, F32(0)).astype(F32)              # a NaN fails v > 0
    c = np.where(c < F32(1), c, F32(1)).astype(F32)
    return ((c * F32(255.0)).astype(F32) + F32(0.5)).astype(F32).astype(np.int64)


def depth_quant(d, mask, depth_scale):
    """dq per pixel, 0 where the pixel has no valid depth."""
    d = np.asarray(d, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(d) & (d > F32(0))
        if mask is not None:
            ok &= np.asarray(mask) != 0
        s = (np.where(ok, d, F32(0)) * F32(depth_scale)).astype(F32)
        big = s >= F32(65535.0)
        dq = np.where(big, 65535, (np.where(big, F32(0), s) + F32(0.5)).astype(F32).astype(np.int64))
    return np.where(ok, dq, 0).astype(np.int64)


def cell_sums(image, depth, mask, grid_w, grid_h, depth_scale):
    """int64 [grid_h * grid_w, 6]: S_R, S_G, S_B, n, S_D, n_D per cell (cell j grid_w + i)."""
    image = np.asarray(image, F32)
    _, H, W = image.shape
    q = quant(image)
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask).reshape(H, W) != 0
    dq = np.zeros((H, W), np.int64) if depth is None else depth_quant(np.asarray(depth, F32).reshape(H, W), m, depth_scale)
    out = np.zeros((grid_w * grid_h, 6), np.int64)
    for j in range(grid_h):
        y0, y1 = j * H // grid_h, (j + 1) * H // grid_h
        for i in range(grid_w):
            x0, x1 = i * W // grid_w, (i + 1) * W // grid_w
            mm, dd = m[y0:y1, x0:x1], dq[y0:y1, x0:x1]
            out[j * grid_w + i] = [q[0, y0:y1, x0:x1][mm].sum(), q[1, y0:y1, x0:x1][mm].sum(), q[2, y0:y1, x0:x1][mm].sum(), mm.sum(),
                                   dd.sum(), (dd > 0).sum()]
    return out


def _i32(v):
    """modulo 2^32, read as int32"""
    return np.asarray(v, np.int64).astype(np.uint32).astype(np.int32)


def bits_from_sums(sums, table):
    """The nibble of every fern from the cell sums: int64 [F]."""
    sums, table = np.asarray(sums, np.int64), np.asarray(table, np.int64)
    cells = sums.shape[0]
    cell = (table[:, 0].astype(np.int32).astype(np.uint32).astype(np.int64)) % cells
    S = sums[cell]
    n, nD = S[:, 3], S[:, 5]
    bit = lambda s, t, k: ((k != 0) & (_i32(s) > _i32(t * k))).astype(np.int64)
    return bit(S[:, 0], table[:, 1], n) | bit(S[:, 1], table[:, 2], n) << 1 | bit(S[:, 2], table[:, 3], n) << 2 | bit(S[:, 4], table[:, 4], nD) << 3


def pack(nibbles):
    """uint32 [F / 8]: the nibble of fern f at bits 4 (f % 8) of word f / 8."""
    nib = np.asarray(nibbles, np.uint64).reshape(-1, 8)
    return (nib << (4 * np.arange(8, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def unpack(code):
    code = np.asarray(code).astype(np.uint32)
    return ((code[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & np.uint32(15)).reshape(code.shape[:-1] + (-1,)).astype(np.int64)


def encode(image, depth, mask, grid_w, grid_h, table, depth_scale):
    return pack(bits_from_sums(cell_sums(image, depth, mask, grid_w, grid_h, depth_scale), table))


def search(database, query, nibble_mask, topk, ferns):
    """(distance int32 [K], best int32 [topk, 2] rows (index, distance))."""
    database = np.asarray(database).astype(np.uint32).reshape(-1, ferns // 8)
    K = database.shape[0]
    differs = ((unpack(database) ^ unpack(np.asarray(query).astype(np.uint32))[None]) & nibble_mask) != 0 if K else np.zeros((0, ferns), bool)
    distance = differs.sum(axis=1).astype(np.int32)
    order = sorted(range(K), key=lambda k: (int(distance[k]), k))[:topk]
    best = np.array([[k, int(distance[k])] for k in order] + [[-1, ferns + 1]] * (topk - len(order)), np.int32).reshape(topk, 2)
    return distance, best


def score(render, render_depth, opacity, image, depth, mask, tau_colour, tau_depth):
    """int32 [8]."""
    render, image = np.asarray(render, F32), np.asarray(image, F32)
    _, H, W = render.shape
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask).reshape(H, W) != 0
    considered = m & (np.asarray(opacity, F32).reshape(H, W) > F32(0.5))
    diff = np.abs(quant(render) - quant(image)).sum(axis=0)
    counts = np.zeros(8, np.int32)
    counts[0], counts[1], counts[2] = m.sum(), considered.sum(), (considered & (diff <= tau_colour)).sum()
    if depth is not None:
        Df, Dr = np.asarray(depth, F32).reshape(H, W), np.asarray(render_depth, F32).reshape(H, W)
        with np.errstate(invalid="ignore", over="ignore"):
            valid = considered & np.isfinite(Df) & (Df > F32(0))
            gap = np.abs((Dr - Df).astype(F32))
            bar = (F32(tau_depth) * Df).astype(F32)
            counts[3], counts[4] = valid.sum(), (valid & (gap <= bar)).sum()
    return counts
