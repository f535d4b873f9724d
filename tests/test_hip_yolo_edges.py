"""The five launches of the YOLO post-processing (csrc/gs_yolo.h: decode, sort, iou, select, masks) at the counts, head shapes and boxes
where such kernels go wrong, against the fp64 restatement (tests/yolo_reference.py): candidate counts around every wave, block,
power-of-two and 4096 boundary up to the 8192-anchor limit, the limit itself, class and coefficient counts around 64, one to four levels,
the row caps, and the mask kernel on one-tile and non-square frames with boxes that leave the frame, vanish or end exactly on a cell.

Head tensors are free-form (any per-level grid; only the proto fixes the frame), so a case builds the anchor count it needs while the
mask frame stays at 64 x 64: most boxes of the count cases lie outside the frame, which is itself the outside-the-frame path.

Inputs are made as in test_hip_yolo.py: background class logits -6, planted candidates with near one-hot DFL bins (box = anchor centre
-+ whole cells) and class logits from a grid of spacing >= 1e-3 (equal logits are ties). Before any comparison every case asserts, on the
fp64 reference, that no candidate pair of a class has an IoU within MIN_IOU_MARGIN of the threshold and that distinct scores (and conf)
are MIN_SCORE_GAP apart: every NMS decision and every sort comparison is then unambiguous in float32, and a mismatch is the kernel's.

gsr_yolo_detect is called through ctypes into rows filled with a sentinel (and guard rows behind max_dets), so that rows beyond
counts[0] are seen untouched; where the wrapper's max_dets applies, slam.segmentation.postprocess must give the same bytes."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from diff_gaussian_rasterization import _C  # noqa: E402
from slam import segmentation as seg  # noqa: E402
import test_hip_yolo as base  # noqa: E402
import yolo_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CONF, IOU = 0.25, 0.7
MIN_IOU_MARGIN = 5e-3        # a 1-cell shift at half-width 6 has IoU 0.846, a 2-cell shift 0.714, a 3-cell shift 0.6; fp32 moves an IoU by ~3e-4
MIN_SCORE_GAP = 1e-5         # sigmoid' >= 0.017 on [-1, 4]: a 1e-3 logit grid gives 1.7e-5, against a float32 ulp of 6e-8
MAX_LEFT_OUT = 1e-3          # share of the frame's pixels that may be left out as ambiguous (a logit within 1e-4 of 0 but not 0)
SENTINEL, GUARD = -7.25e30, 4
FRAME = (64, 64)
GRID, STRIDE = (64, 128), 8.0          # one level of 8192 anchors: the count cases
UNIT = (0, 0, 1, 1)                    # (l, t, r, b): the anchor's own cell, disjoint from every other anchor's


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _build(levels, plants, nc=2, nm=32, frame=FRAME, seed=0):
    """test_hip_yolo._heads for any per-level grids: levels [(h, w)], plants (level, y, x, class, class logit, (l, t, r, b) in cells).
    Returns (per level (head [64 + nc, h, w], coef [nm, h, w]), proto [nm, H / 4, W / 4]) on the device."""
    g = torch.Generator().manual_seed(seed)
    P = np.array([(l, y, x, c) for l, y, x, c, _, _ in plants], dtype=np.int64).reshape(-1, 4)
    logit = torch.tensor([p[4] for p in plants], dtype=torch.float32)
    ltrb = np.array([p[5] for p in plants], dtype=np.int64).reshape(-1, 4)
    heads = []
    for l, (lh, lw) in enumerate(levels):
        h = torch.randn((64 + nc, lh, lw), generator=g)
        h[64:] = -6.0
        sel = P[:, 0] == l
        y, x = torch.from_numpy(P[sel, 1]), torch.from_numpy(P[sel, 2])
        h[:64, y, x] = 0.0
        for k in range(4):
            h[torch.from_numpy(k * 16 + ltrb[sel, k]), y, x] = 12.0
        h[torch.from_numpy(64 + P[sel, 3]), y, x] = logit[torch.from_numpy(sel)]
        heads.append((h.to(DEV).contiguous(), _factors((nm, lh, lw), g).to(DEV).contiguous()))
    return heads, _factors((nm, frame[0] // 4, frame[1] // 4), g).to(DEV).contiguous()


def _factors(shape, g):
    """Random coefficients or proto values. With one coefficient a logit is a single product, and products of two normal values
    crowd around 0 (one pixel in a hundred within 1e-4 of it): there the values keep a distance of 0.5 from 0."""
    t = torch.randn(shape, generator=g)
    return t if shape[0] > 1 else torch.where(t < 0, t - 0.5, t + 0.5)


def _grid_logits(n, rng, lo=1, hi=4999):
    """n class logits -1 + 1e-3 k with k drawn from [lo, hi]: distinct while n <= hi - lo + 1, tied in pairs beyond."""
    return (-1.0 + 1e-3 * (lo + rng.permutation(n) % (hi - lo + 1))).tolist()


def _yx(a):
    return int(a) // GRID[1], int(a) % GRID[1]


def _count_plants(n, layout, seed):
    """n candidates of class 0 on the one 64 x 128 level.
    disjoint   unit boxes on n anchors spread over the level (four of them inside the 64 x 64 frame): kept = n
    clusters   blocks of 16 x 16 anchors that all decode to one box (a DFL side is at most 15 cells, so 256 anchors is the most that can
               share a box): the first visited box of a block suppresses the other 255, kept = ceil(n / 256)
    chains     every row a chain of 1-cell shifts, boxes 12 cells wide and 1 high: neighbours at 1 and 2 cells (IoU 0.846, 0.714) go,
               at 3 cells (0.6) stay. The lowest score of all sits next to the highest, so the last sorted position is suppressed by
               the first
    ties       unit boxes on all 8192 anchors, logits equal in groups of 8 that straddle sorted positions 63/64, 1023/1024 and
               4095/4096 (groups start at 8 k + 4), one group being the anchors 1020 .. 1027"""
    rng = np.random.default_rng(seed)
    A = GRID[0] * GRID[1]
    if layout == "disjoint":
        inside = [y * GRID[1] + x for y in range(FRAME[0] // 8) for x in range(FRAME[1] // 8)]
        first = rng.permutation(inside)[:min(n, 4)].tolist()
        rest = np.setdiff1d(np.arange(A), first)
        anchors = sorted(first + rng.permutation(rest)[:n - len(first)].tolist())
        return [(0, *_yx(a), 0, v, UNIT) for a, v in zip(anchors, _grid_logits(n, rng))]
    if layout == "clusters":
        return [(0, *_yx(a), 0, v, (_yx(a)[1] % 16, _yx(a)[0] % 16, 15 - _yx(a)[1] % 16, 15 - _yx(a)[0] % 16))
                for a, v in zip(range(n), _grid_logits(n, rng))]
    if layout == "chains":
        logits = _grid_logits(n, rng)
        low, high = 5 * GRID[1] + 50, 5 * GRID[1] + 51
        logits[low], logits[high] = -1.0, 4.0
        return [(0, *_yx(a), 0, v, (6, 0, 6, 1)) for a, v in zip(range(n), logits)]
    if layout == "ties":
        assert n == A
        at = rng.permutation(A)                                        # at[r]: the anchor of rank r (ranks of one group are tied)
        for k, a in enumerate(range(1020, 1028)):                      # anchors 1020 .. 1027 into the group of ranks 2044 .. 2051
            i, j = int(np.nonzero(at == a)[0][0]), 2044 + k
            at[i], at[j] = at[j], at[i]
        return [(0, *_yx(at[r]), 0, 4.0 - 1e-3 * ((r + 4) // 8), UNIT) for r in range(A)]
    raise ValueError(layout)


# ---- the reference of a case, and the conditions on its input ---------------------------------------------------------------------------
_seen = {}


def _note(group, **kw):
    """The figures of a case, printed (pytest -rP shows them), and the extremes per group."""
    s = _seen.setdefault(group, {})
    for k, v in kw.items():
        s[k] = (max if k == "left_out" else min)(s.get(k, v), v)
    print(f"[yolo-edges] {group}: " + " ".join(f"{k}={v:.3g}" for k, v in kw.items()) + f" | so far {s}")


def _reference(group, heads, strides, classes, max_det, max_dets=None):
    boxes, scores, _ = ref.decode(heads, strides)
    best, j = scores.max(1)
    cand = (best > CONF) & torch.isin(j, torch.tensor(sorted(classes), device=j.device))
    xyxy = torch.cat((boxes[:, :2] - boxes[:, 2:] / 2, boxes[:, :2] + boxes[:, 2:] / 2), 1)
    margin, gap = ref.min_iou_margin(xyxy[cand], j[cand], IOU), ref.min_score_gap(best, CONF)      # gap: over all anchors
    _note(group, min_iou_margin=margin, min_score_gap=gap)
    assert margin >= MIN_IOU_MARGIN and gap >= MIN_SCORE_GAP, (margin, gap)
    rows, coef, counts = ref.detections(heads, strides, classes, CONF, IOU, max_det, max_dets=max_dets, counts=True)
    return SimpleNamespace(rows=rows, coef=coef, counts=counts, boxes=boxes, scores=scores, xyxy=xyxy, best=best, cls=j, cand=cand)


# ---- the calls ------------------------------------------------------------------------------------------------------------------------
def _buffers(anchors, nm, max_dets):
    """(dets [max_dets + GUARD, 7 + nm] filled with SENTINEL, counts int32 [3 + GUARD] filled with -77, the workspace filled with 0xA5)."""
    size = int(_C.load_library().gsr_yolo_workspace_size(min(anchors, 8192)))
    return (torch.full((max_dets + GUARD, 7 + nm), SENTINEL, dtype=torch.float32, device=DEV),
            torch.full((3 + GUARD,), -77, dtype=torch.int32, device=DEV), torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV))


def _detect(heads, strides, classes, max_det, max_dets, conf=CONF, iou=IOU, buffers=None):
    """gsr_yolo_detect through ctypes into _buffers(): (dets, counts, workspace)."""
    L = _C.load_library()
    nl, nc, nm = len(heads), int(heads[0][0].shape[0]) - 64, int(heads[0][1].shape[0])
    hw = [int(v) for h, _ in heads for v in h.shape[1:]]
    for h, c in heads:
        assert h.is_contiguous() and c.is_contiguous() and h.dtype == c.dtype == torch.float32
    anchors = sum(hw[2 * l] * hw[2 * l + 1] for l in range(nl))
    dets, counts, ws = buffers if buffers is not None else _buffers(anchors, nm, max_dets)
    classes = sorted(classes)
    with torch.cuda.device(DEV):
        L.gsr_yolo_detect(nl, (C.c_int * (2 * nl))(*hw), (C.c_float * nl)(*[float(s) for s in strides]),
                          (C.c_void_p * nl)(*[h.data_ptr() for h, _ in heads]), (C.c_void_p * nl)(*[c.data_ptr() for _, c in heads]), nc, nm,
                          (C.c_int * len(classes))(*classes), len(classes), float(conf), float(iou), int(max_det), ws.data_ptr(),
                          dets.data_ptr(), int(max_dets), counts.data_ptr(), _C._stream(torch.device(DEV)))
    return dets, counts, ws


def _check_dets(dets, counts, R, max_dets):
    c = counts.tolist()
    assert c[3:] == [-77] * GUARD                                                    # nothing behind the three counts
    assert tuple(c[:3]) == tuple(R.counts), (c[:3], R.counts)                        # emitted, candidates, kept
    n = c[0]
    assert n <= max_dets
    assert bool((dets[n:] == SENTINEL).all())                                        # rows beyond counts[0], guard rows included: untouched
    got = dets[:n].cpu()
    o = got[:, :7].double()
    s, a = o[:, 4], o[:, 6]
    assert bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (a[:-1] < a[1:]))).all())   # score descending, then anchor ascending
    gi, wi = torch.argsort(a), torch.argsort(R.rows[:, 6])
    assert torch.equal(a[gi], R.rows[wi, 6])                                         # the kept set, by anchor (no anchor twice: the order is strict)
    assert torch.equal(o[gi, 5], R.rows[wi, 5])                                      # the class
    np.testing.assert_allclose(o[gi, :5].numpy(), R.rows[wi, :5].numpy(), rtol=1e-5, atol=1e-3)
    assert torch.equal(got[gi, 7:], R.coef.float().cpu()[wi])                        # the coefficient columns: the head's, bit for bit


def _union(rows, coef, proto, shape):
    """ref.union_mask in pieces of detections, the fp64 logits of a piece under 100 MB: (mask, ambiguous pixels)."""
    want = torch.zeros(shape, dtype=torch.bool, device=proto.device)
    amb = torch.zeros(shape, dtype=torch.bool, device=proto.device)
    step = max(1, 12_000_000 // (shape[0] * shape[1]))
    for i in range(0, len(rows), step):
        w, lg = ref.union_mask(rows[i:i + step], coef[i:i + step], proto, shape)
        want |= w
        amb |= ((lg.abs() < 1e-4) & (lg != 0)).any(0)                                 # exact zeros are the crop's and must agree
    return want, amb


def _check_mask(group, mask, rows, coef, proto, shape):
    want, amb = _union(rows, coef, proto, shape)
    left_out = float(amb.double().mean())
    _note(group, left_out=left_out)
    assert left_out <= MAX_LEFT_OUT, left_out
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == tuple(shape) and int(mask.max()) <= 1
    diff = (mask.bool() != want) & ~amb
    assert int(diff.sum()) == 0, int(diff.sum())
    return want


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _run(group, heads, strides, proto, classes, max_det=300, max_dets=None, frame=FRAME, expect_mask=None):
    """One detection case, end to end: reference and input conditions, the ctypes call, detections, counts, sentinels, the masks of
    those detections, and the wrapper where its max_dets is the one asked for."""
    cap = max_det * len(classes) if max_dets is None else max_dets
    R = _reference(group, heads, strides, classes, max_det, max_dets)
    dets, counts, _ = _detect(heads, strides, classes, max_det, cap)
    _check_dets(dets, counts, R, cap)
    mask = seg.masks_from_dets(dets[:cap], counts[:3], proto)
    want = _check_mask(group, mask, R.rows, R.coef, proto, frame)
    if expect_mask is not None:
        assert bool(want.any()) == expect_mask
    if max_dets is None:
        res = seg.postprocess(heads, proto, classes, strides, conf=CONF, iou=IOU, max_det=max_det)
        n = R.counts[0]
        assert torch.equal(res.counts, counts[:3]) and torch.equal(_bits(res.dets[:n]), _bits(dets[:n])) and torch.equal(res.mask, mask)
    return R, dets, counts, mask


# ---- candidate counts -------------------------------------------------------------------------------------------------------------------
COUNTS = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 8192]


@pytest.mark.parametrize("max_det", [8192, 300])
@pytest.mark.parametrize("n", COUNTS)
def test_candidate_counts_disjoint(n, max_det):
    heads, proto = _build([GRID], _count_plants(n, "disjoint", seed=n), seed=n)
    R, *_ = _run("counts", heads, [STRIDE], proto, [0], max_det=max_det, expect_mask=n > 0)
    assert R.counts == (min(n, max_det), n, n)


def _sorted_position_facts(R):
    """Of one class: per suppressed candidate at a sorted position >= 4096, whether a kept box that suppresses it lies before 4096 and
    whether one lies at or behind 4096 (what the second word of the select wave's removed set has to carry)."""
    idx = torch.nonzero(R.cand).flatten()
    idx = idx[torch.sort(R.best[idx], descending=True, stable=True).indices]          # sorted position -> anchor
    pos = torch.empty(len(R.best), dtype=torch.long, device=idx.device)
    pos[idx] = torch.arange(len(idx), device=idx.device)
    kept = torch.zeros(len(R.best), dtype=torch.bool, device=idx.device)
    kept[ref.survivors(R.boxes, R.scores, 0, CONF, IOU)[0]] = True
    late = idx[4096:][~kept[idx[4096:]]]                                              # suppressed, at position >= 4096
    K = idx[kept[idx]]
    lo = torch.zeros(len(late), dtype=torch.bool, device=idx.device)
    hi = torch.zeros(len(late), dtype=torch.bool, device=idx.device)
    for i in range(0, len(late), 512):
        j = late[i:i + 512]
        m = (ref._pair_iou(R.xyxy[j], R.xyxy[K]) > IOU) & (pos[K][None, :] < pos[j][:, None])
        lo[i:i + 512] = (m & (pos[K] < 4096)[None, :]).any(1)
        hi[i:i + 512] = (m & (pos[K] >= 4096)[None, :]).any(1)
    return idx, kept, lo, hi


@pytest.mark.parametrize("layout", ["clusters", "chains"])
@pytest.mark.parametrize("n", [4097, 8192])
def test_suppression_across_sorted_position_4096(n, layout):
    heads, proto = _build([GRID], _count_plants(n, layout, seed=n), seed=n)
    R, *_ = _run("counts", heads, [STRIDE], proto, [0], max_det=8192, expect_mask=True)
    idx, kept, lo, hi = _sorted_position_facts(R)
    assert R.counts[1] == n
    if layout == "clusters":
        assert R.counts[2] == (n + 255) // 256                                        # one box per block of 256 suppresses the rest of it
    else:
        assert n // 5 < R.counts[2] < n // 2                                          # a kept box clears two cells on either side
    assert not kept[idx[n - 1]] and kept[idx[0]]
    assert bool((lo & ~hi).any())                  # a box beyond 4096 that only boxes among the first 4096 suppress: a bit set in words >= 64
    if n == 8192 and layout == "chains":
        assert bool((hi & ~lo).any())              # ... and one that only kept boxes beyond 4096 suppress
        assert bool(kept[idx[4096:]].any())
    # with max_det = 300 the suppression is the same and the cut falls inside the first word
    R2, *_ = _run("counts", heads, [STRIDE], proto, [0], max_det=300)
    assert R2.counts == (min(300, R.counts[2]), n, R.counts[2])


def test_tied_scores_across_block_and_word_boundaries():
    heads, proto = _build([GRID], _count_plants(8192, "ties", seed=3), seed=3)
    R, dets, counts, _ = _run("counts", heads, [STRIDE], proto, [0], max_det=8192, expect_mask=True)
    assert R.counts == (8192, 8192, 8192)
    s, a = dets[:8192, 4].cpu(), dets[:8192, 6].cpu()
    for p in (63, 1023, 4095):                                                        # the groups of 8 straddle these sorted positions
        assert float(s[p - 3]) == float(s[p]) == float(s[p + 1]) == float(s[p + 4]) and float(s[p - 4]) > float(s[p - 3])
        assert a[p - 3:p + 5].tolist() == sorted(a[p - 3:p + 5].tolist())
    assert a[2044:2052].tolist() == list(range(1020, 1028))                           # the group over the anchors 1023 / 1024


# ---- the anchor limit -----------------------------------------------------------------------------------------------------------------
LEVELS4, STRIDES4 = [(64, 96), (32, 48), (16, 24), (8, 16)], [8.0, 16.0, 32.0, 64.0]


def _lattice_plants(levels, classes, rng, step=8):
    """Per level, on a lattice of `step` cells: chains of 1 to 3 anchors a cell apart, of half-width 2 (IoU 0.6: all stay) or, where the
    level is wide enough, 6 (0.846 and 0.714: one stays); plus the last anchor of every level, a unit box."""
    out = []
    for l, (lh, lw) in enumerate(levels):
        for y in range(0, lh, step):
            for x in range(0, lw - 3, 2 * step):
                d = int(rng.choice([2, 6])) if min(lh, lw) >= 32 else 2
                c = int(rng.choice(classes))
                for k in range(int(rng.integers(1, 4))):
                    out.append((l, y, x + k, c, 0.0, (d, d, d, d)))
        out.append((l, lh - 1, lw - 1, int(classes[0]), 0.0, UNIT))
    vals = _grid_logits(len(out), rng)
    return [(l, y, x, c, v, d) for (l, y, x, c, _, d), v in zip(out, vals)]


def test_8192_anchors_over_four_levels():
    assert sum(h * w for h, w in LEVELS4) == 8192
    plants = _lattice_plants(LEVELS4, [0, 1], np.random.default_rng(11))
    heads, proto = _build(LEVELS4, plants, nc=3, seed=11)
    R, dets, counts, _ = _run("A boundary", heads, STRIDES4, proto, [0, 1], expect_mask=True)
    anchors = set(int(a) for a in R.rows[:, 6])
    assert {6143, 7679, 8063, 8191} <= anchors                                                       # the last anchor of every level
    assert R.counts[1] > R.counts[2] > 50 and {0.0, 1.0} == set(R.rows[:, 5].tolist())


def test_8193_anchors_are_refused_before_any_launch():
    L = _C.load_library()
    assert L.gsr_yolo_workspace_size(8192) > 0 and L.gsr_yolo_workspace_size(8193) == 0
    assert L.gsr_yolo_workspace_size(1) > 0 and L.gsr_yolo_workspace_size(0) == 0
    for levels in ([(1, 8193)], LEVELS4[:3] + [(3, 43)]):                                          # the second: 8064 + 129
        assert sum(h * w for h, w in levels) == 8193
        heads, proto = _build(levels, [(0, 0, 0, 0, 2.0, UNIT)], seed=1)
        strides = STRIDES4[:len(levels)]
        with pytest.raises(ValueError, match="8193 anchors"):
            seg.postprocess(heads, proto, [0], strides)
        with pytest.raises(RuntimeError, match=r"code -1\).*anchors") as e:
            _detect(heads, strides, [0], 300, 300)
        assert "8192" in str(e.value)
        # the same call on buffers kept: counts, dets and the workspace stay as they were
        dets, counts, ws = _buffers(8193, 32, 300)
        with pytest.raises(RuntimeError, match="anchors"):
            _detect(heads, strides, [0], 300, 300, buffers=(dets, counts, ws))
        torch.cuda.synchronize()
        assert bool((dets == SENTINEL).all()) and bool((counts == -77).all()) and bool((ws == 0xA5).all())
        assert ws.numel() == L.gsr_yolo_workspace_size(8192)


# ---- head shapes ----------------------------------------------------------------------------------------------------------------------
LEVELS3, STRIDES3 = [(8, 8), (4, 4), (2, 2)], [8.0, 16.0, 32.0]          # the heads of a 64 x 64 frame


def _class_plants(nc, classes):
    """Per requested class: a pair a cell apart at half-width 6 on level 0 (the lower score goes), a box on level 1 and one on level 0
    with a second class above conf below it; and one anchor whose best class is outside the set while a requested class is above conf
    (level 1, cell (3, 3): anchor 79, dropped). Returns (plants, that anchor or None when every class is requested)."""
    out = []
    for k, c in enumerate(sorted(classes)):
        y = 2 * k
        out += [(0, y, 1, c, 1.0 + 0.1 * k, (1, 0, 1, 1)), (0, y, 5, c, 2.0 + 0.1 * k, (6, 0, 6, 1)), (0, y, 6, c, 0.5 + 0.1 * k, (6, 0, 6, 1)),
                (1, k, 0, c, 3.0 + 0.1 * k, (0, 0, 1, 1))]
        if nc > 1:
            out.append((0, y, 1, (c + 1) % nc, -0.5, (1, 0, 1, 1)))                     # a second class above conf, below the best
    outside = [c for c in (max(classes) + 1, min(classes) - 1, max(classes) - 1) if 0 <= c < nc and c not in classes]     # a neighbouring bit
    if not outside:
        return out, None
    out += [(1, 3, 3, outside[0], 3.5, UNIT), (1, 3, 3, min(classes), 1.5, UNIT)]
    return out, 64 + 15


@pytest.mark.parametrize("nc,classes", [(1, [0]), (33, [0]), (33, [31, 32]), (65, [0]), (65, [31, 32]), (65, [64]), (256, [0]),
                                        (256, [31, 32]), (256, [64]), (256, [255]), (256, [0, 255])])
def test_class_counts_and_class_sets(nc, classes):
    plants, dropped = _class_plants(nc, classes)
    heads, proto = _build(LEVELS3, plants, nc=nc, seed=nc + classes[-1])
    R, *_ = _run("head shapes", heads, STRIDES3, proto, classes, expect_mask=True)
    k = len(classes)
    assert R.counts == (3 * k, 4 * k, 3 * k) and sorted(set(R.rows[:, 5].tolist())) == [float(c) for c in classes]
    if nc > 1:
        assert dropped is not None and dropped not in set(int(a) for a in R.rows[:, 6])
        assert float(R.best[dropped]) > CONF and int(R.cls[dropped]) not in classes


@pytest.mark.parametrize("nm", [1, 57, 58, 64])
def test_coefficient_counts(nm):
    plants, _ = _class_plants(4, [0, 2])
    heads, proto = _build(LEVELS3, plants, nc=4, nm=nm, seed=nm)
    R, *_ = _run("head shapes", heads, STRIDES3, proto, [0, 2], expect_mask=True)
    assert R.counts == (6, 8, 6) and R.coef.shape == (6, nm)


@pytest.mark.parametrize("name", ["1x1", "1x65", "four non-square"])
def test_level_counts_and_grids(name):
    if name == "1x1":
        levels, strides, plants = [(1, 1)], [64.0], [(0, 0, 0, 0, 1.0, (0, 0, 1, 1))]           # the box (32, 32) - (96, 96): a corner of it in the frame
    elif name == "1x65":
        levels, strides = [(1, 65)], [8.0]
        plants = [(0, 0, x, 0, v, (1, 0, 1, 1) if x % 3 else (6, 0, 6, 1)) for x, v in zip(range(65), _grid_logits(65, np.random.default_rng(2)))]
    else:
        levels, strides = [(5, 9), (3, 7), (2, 3), (1, 2)], STRIDES4
        plants = [(l, y, x, 0, 0.0, (1, 1, 1, 1)) for l, (lh, lw) in enumerate(levels) for y in range(lh) for x in range(0, lw, 3)]
        plants = [(*p[:4], v, p[5]) for p, v in zip(plants, _grid_logits(len(plants), np.random.default_rng(4)))]
    heads, proto = _build(levels, plants, seed=6)
    R, *_ = _run("head shapes", heads, strides, proto, [0], expect_mask=True)
    assert R.counts[1] == len(plants) and R.counts[0] > 0
    if name == "four non-square":
        first = np.cumsum([0] + [h * w for h, w in levels])
        assert all(any(first[l] <= a < first[l + 1] for a in R.rows[:, 6].tolist()) for l in range(4))     # a detection on every level


def _two_class_heads(seed=8):
    plants = [(0, y, x, c, 0.0, UNIT) for c, ys in ((0, (0, 2, 4)), (1, (1, 3)), (3, (5,))) for y in ys for x in range(0, 8, 2)]
    plants = [(*p[:4], v, p[5]) for p, v in zip(plants, _grid_logits(len(plants), np.random.default_rng(seed)))]
    return _build(LEVELS3, plants, nc=80, seed=seed)                              # 12 boxes of class 0, 8 of class 1, 4 of class 3


def test_max_det_one_with_several_classes():
    heads, proto = _two_class_heads()
    R, *_ = _run("head shapes", heads, STRIDES3, proto, [0, 1, 3], max_det=1)
    assert R.counts == (3, 24, 24) and sorted(R.rows[:, 5].tolist()) == [0.0, 1.0, 3.0]
    for c in (0, 1, 3):                                                                # each class's best box
        assert float(R.rows[R.rows[:, 5] == c][0, 4]) == float(R.best[(R.cls == c) & R.cand].max())


@pytest.mark.parametrize("max_det,max_dets", [(5, 1), (5, 4), (5, 9), (5, 10), (12, 19), (300, 7)])
def test_fewer_rows_than_max_det_times_classes(max_det, max_dets):
    heads, proto = _two_class_heads()
    R, *_ = _run("head shapes", heads, STRIDES3, proto, [0, 1], max_det=max_det, max_dets=max_dets)
    assert R.counts == (min(max_dets, min(12, max_det) + min(8, max_det)), 20, 20)


def test_masks_take_only_the_rows_given():
    heads, proto = _two_class_heads()
    R = _reference("head shapes", heads, STRIDES3, [0, 1], 300)
    rows = torch.cat((R.rows, R.coef.cpu()), 1).float()
    big = torch.cat((rows[:3], torch.zeros((13, rows.shape[1]))))
    big[3:, 2:4] = 64.0                                                                # behind the rows given: whole-frame boxes whose
    big[3:, 7:] = proto[:, 5, 5].cpu()                                                 # coefficients give a positive logit
    big = big.to(DEV).contiguous()
    counts = torch.tensor([16, 0, 0], dtype=torch.int32, device=DEV)
    assert bool(_union(big[3:4, :7].double().cpu(), big[3:4, 7:].double(), proto, FRAME)[0].any())
    mask = seg.masks_from_dets(big[:3], counts, proto)                                 # counts[0] = 16, three rows given: three rows count
    want = _check_mask("head shapes", mask, R.rows[:3], R.coef[:3], proto, FRAME)
    full = seg.masks_from_dets(big, counts, proto)
    assert int(full.sum()) > int(mask.sum()) and not torch.equal(full.bool(), want)


# ---- masks ----------------------------------------------------------------------------------------------------------------------------
FRAMES = [(32, 32), (32, 64), (64, 32), (96, 160)]


def _boxes(H, W):
    """name -> (x1, y1, x2, y2) in pixels; the proto cell is 4 pixels."""
    b = {
        "whole frame": (0, 0, W, H),
        "left": (-10.5, 6.3, 11.2, 20.9), "right": (W - 9.7, 5.1, W + 30.2, 22.6), "top": (5.4, -40.2, 25.1, 9.9),
        "bottom": (3.3, H - 13.2, 28.8, H + 7.7), "top left": (-5.5, -6.6, 9.1, 10.2), "top right": (W - 10.3, -1.2, W + 0.7, 12.4),
        "bottom left": (-100.0, H - 6.1, 8.2, H + 100.0), "bottom right": (W - 7.3, H - 9.9, W + 4.0, H + 4.0),
        "beyond every side": (-20.0, -30.0, W + 40.0, H + 50.0),
        "outside right": (W + 5.0, 3.0, W + 30.0, 20.0), "outside top left": (-50.0, -50.0, -3.0, -3.0), "outside bottom": (2.0, H + 0.5, 30.0, H + 9.0),
        "touching the right edge from outside": (float(W), 0.0, W + 8.0, float(H)),
        "zero width": (8.0, 4.0, 8.0, 24.0), "zero height": (4.0, 12.0, 24.0, 12.0), "a point": (16.0, 16.0, 16.0, 16.0),
        "between two columns": (9.0, 2.0, 11.0, 30.0), "between two rows": (2.0, 13.5, 30.0, 15.9), "inside one cell": (21.0, 21.0, 23.0, 23.0),
        "on cells": (8.0, 4.0, 16.0, 12.0), "on cells, one cell": (20.0, 20.0, 24.0, 24.0), "on the last cell": (W - 4.0, H - 4.0, float(W), float(H)),
    }
    if (H, W) == (96, 160):
        b.update({"four tiles": (26.0, 25.0, 39.5, 38.5), "four tiles, on cells": (28.0, 28.0, 36.0, 36.0), "four tiles, far": (120.5, 58.0, 135.0, 70.2),
                  "two tiles, a cell each side": (60.0, 40.0, 68.0, 44.0)})
    return b


MARK_NOTHING = ("outside right", "outside top left", "outside bottom", "touching the right edge from outside", "zero width", "zero height",
                "a point", "between two columns", "between two rows", "inside one cell")


def _rows_of(boxes, nm, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(boxes)
    rows = torch.cat((torch.tensor(list(boxes), dtype=torch.float32).reshape(n, 4), torch.full((n, 1), 0.5), torch.zeros((n, 1)),
                      torch.arange(float(n))[:, None], _factors((nm, n), g).T), 1)
    return rows.to(DEV).contiguous()


@pytest.mark.parametrize("nm", [1, 32, 64])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_masks_of_hand_built_rows(frame, nm):
    H, W = frame
    boxes = _boxes(H, W)
    g = torch.Generator().manual_seed(H + W + nm)
    proto = _factors((nm, H // 4, W // 4), g).to(DEV).contiguous()
    dets = _rows_of(boxes.values(), nm, seed=nm)
    counts = torch.tensor([len(boxes), 0, 0], dtype=torch.int32, device=DEV)
    rows, coef = dets[:, :7].double().cpu(), dets[:, 7:].double()
    mask = seg.masks_from_dets(dets, counts, proto)
    want = _check_mask("masks", mask, rows, coef, proto, frame)
    assert bool(want.any())
    assert torch.equal(seg.masks_from_dets(dets, counts, proto), mask)                 # two calls: the same bytes
    # every box alone; those that hold no proto cell mark nothing, whatever the coefficients
    for k, name in enumerate(boxes):
        one = dets[k:k + 1].clone()
        one[:, 7:] = one[:, 7:].abs()
        pos = proto.abs().contiguous()                                                 # positive logits wherever the crop keeps a cell
        m = seg.masks_from_dets(one, torch.tensor([1, 0, 0], dtype=torch.int32, device=DEV), pos)
        w = _check_mask("masks", m, rows[k:k + 1], one[:, 7:].double(), pos, frame)
        assert bool(w.any()) == (name not in MARK_NOTHING), name
    # motion as bool, as uint8 and absent: motion == before & ~mask, in place
    before = torch.rand((H, W), generator=g).to(DEV) > 0.2
    for dtype in (torch.bool, torch.uint8):
        motion = before.to(dtype).contiguous()
        assert torch.equal(seg.masks_from_dets(dets, counts, proto, motion), mask)
        assert torch.equal(motion.bool(), before & ~mask.bool()) and int(motion.to(torch.uint8).max()) <= 1
    # no detections: an empty mask, motion as it was
    motion = before.clone()
    none = seg.masks_from_dets(dets, torch.zeros(3, dtype=torch.int32, device=DEV), proto, motion)
    assert not bool(none.any()) and torch.equal(motion, before)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_crop_edges_are_inclusive_left_and_exclusive_right(frame):
    """A box on proto cells, columns [2, 4) and rows [1, 3), over a proto of ones with coefficient one: the cropped logits are 1 on
    those four cells. A bilinear tap reaches column 2 from pixel 6 on and column 3 up to pixel 17; were the right edge inclusive,
    column 4 would be reached up to pixel 21, were the left exclusive, column 2 would be missing and the mask begin at pixel 10."""
    H, W = frame
    proto = torch.ones((1, H // 4, W // 4), device=DEV)
    dets = torch.tensor([[8.0, 4.0, 16.0, 12.0, 0.5, 0.0, 0.0, 1.0]], device=DEV)
    rows, coef = dets[:, :7].double().cpu(), dets[:, 7:].double()
    lg = ref.mask_logits(rows, coef, proto, frame)[0]
    on_x, on_y = (lg > 0).any(0).nonzero().flatten().tolist(), (lg > 0).any(1).nonzero().flatten().tolist()
    assert on_x == list(range(6, 18)) and on_y == list(range(2, 14))                   # the rule, on the reference's own logits
    assert float(lg[lg > 0].min()) >= 0.125 * 0.125
    mask = seg.masks_from_dets(dets, torch.tensor([1, 0, 0], dtype=torch.int32, device=DEV), proto)
    _check_mask("masks", mask, rows, coef, proto, frame)
    assert torch.equal(mask.bool(), lg > 0)


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_postprocess_on_small_frames(frame):
    H, W = frame
    rng = np.random.default_rng(H + W)
    plants = []
    for l, (lh, lw) in enumerate(base._grid(H, W)):
        for y in range(0, lh, 3):
            for x in range(0, lw, 3):
                plants.append((l, y, x, int(rng.choice([0, 56])), 0.0, (1, 1, 1, 1) if l else (2, 1, 2, 1)))
    plants = [(*p[:4], v, p[5]) for p, v in zip(plants, _grid_logits(len(plants), rng))]
    heads, proto = base._heads(H, W, plants, seed=H + W)
    heads = [(h.to(DEV), c.to(DEV)) for h, c in heads]
    R, dets, counts, mask = _run("masks", heads, base.STRIDES, proto.to(DEV), [0, 56], frame=frame, expect_mask=True)
    assert R.counts[0] >= 2
    before = torch.rand((H, W), generator=torch.Generator().manual_seed(1)).to(DEV) > 0.2
    for dtype in (torch.bool, torch.uint8):
        motion = before.to(dtype).contiguous()
        res = seg.postprocess(heads, proto.to(DEV), [0, 56], base.STRIDES, motion)
        assert torch.equal(res.mask, mask) and torch.equal(motion.bool(), before & ~mask.bool())
