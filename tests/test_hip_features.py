"""The feature-seed stage on the device (include/feature_matching.h, csrc/gs_features.h, slam/features.py): the three kernels bit for bit
against the numpy restatement (tests/features_reference.py) at edge sizes and inputs, determinism, guard words, refusals; then the stage in
use: loop verification and localisation in a saved map started from the feature pose."""
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import features_reference as ref  # noqa: E402
import odometry_reference as odo  # noqa: E402
from slam import features  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
DIRECTIONS, PATTERN = features.pattern_tables(0)
EXTRACT_SHAPES = [(36, 36, 16, 1), (37, 37, 16, 2), (64, 48, 16, 3), (161, 97, 16, 3), (160, 120, 32, 1), (320, 240, 16, 4)]
EXTRACT_INPUTS = ["scene", "noise", "constant", "checker", "tiles", "wild", "masked", "clamp"]


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _guarded(n, dtype=torch.int32):
    """(the whole buffer, its first n entries): four guard entries follow the output"""
    buf = torch.full((n + 4,), GUARD, dtype=dtype, device="cuda")
    return buf, buf[:n]


def _guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


# ---- extract ------------------------------------------------------------------------------------------------------------------------------
_views = {}


def _input(kind, W, H):
    """(image, mask, pattern) of one kind of input"""
    rng = np.random.default_rng(W * 1000 + H)
    mask, pattern = None, PATTERN
    if kind in ("scene", "masked", "clamp"):
        if (W, H) not in _views:
            _views[(W, H)] = ref.view(W, H)[0]
        image = _views[(W, H)]
    if kind == "noise":
        image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    if kind == "constant":
        image = np.full((3, H, W), 0.4, np.float32)
    if kind == "checker":
        y, x = np.mgrid[0:H, 0:W]
        image = np.repeat(np.where(((x // 4 + y // 4) % 2) == 0, 0.3, 0.7)[None], 3, axis=0).astype(np.float32)
    if kind == "tiles":                                                  # a checkerboard's crossings are no FAST corners; the corners of tiles are
        y, x = np.mgrid[0:H, 0:W]
        image = np.repeat(np.where((x % 8 < 5) & (y % 8 < 5), 0.7, 0.3)[None], 3, axis=0).astype(np.float32)
    if kind == "wild":
        image = rng.uniform(-0.5, 1.5, (3, H, W)).astype(np.float32)
        flat = image.reshape(-1)
        flat[3::11], flat[5::13], flat[1::17] = np.nan, np.inf, -np.inf
    if kind == "masked":
        mask = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
        mask[:H // 2, W // 3:] = 0                                      # whole cells without a pixel
    if kind == "clamp":
        pattern = PATTERN.copy()
        pattern[:, ::3, 0], pattern[:, 1::3, 3], pattern[:, 2::5, 2] = 127, -127, -128
    return image, mask, pattern


def _extract(image, mask, cell, per_cell, threshold, pattern):
    H, W = image.shape[1:]
    slots = ref.slots(W, H, cell, per_cell)
    kbuf, keypoints = _guarded(4 * slots)
    dbuf, descriptors = _guarded(8 * slots)
    features.extract(_dev(image), _dev(mask), cell, per_cell, threshold, _dev(DIRECTIONS), _dev(pattern), keypoints.view(slots, 4),
                     descriptors.view(slots, 8))
    torch.cuda.synchronize()
    assert _guard_ok(kbuf, 4 * slots) and _guard_ok(dbuf, 8 * slots)
    return keypoints.view(slots, 4).cpu().numpy(), descriptors.view(slots, 8).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", EXTRACT_INPUTS)
@pytest.mark.parametrize("W,H,cell,per_cell", EXTRACT_SHAPES)
def test_extract_equals_the_restatement_bit_for_bit(W, H, cell, per_cell, kind):
    image, mask, pattern = _input(kind, W, H)
    threshold = 20 if kind not in ("checker", "tiles") else 5
    want_k, want_d = ref.extract(image, mask, cell, per_cell, threshold, DIRECTIONS, pattern)
    got_k, got_d = _extract(image, mask, cell, per_cell, threshold, pattern)
    assert got_k.shape == (features.slot_count(W, H, cell, per_cell), 4)
    assert got_k.tobytes() == want_k.tobytes()
    assert got_d.tobytes() == want_d.tobytes()
    found = int((want_k[:, 0] >= 0).sum())
    if W < 37 or kind == "constant":
        assert found == 0 and not want_d.any()
    elif W >= 64 and kind in ("noise", "wild", "scene", "clamp"):
        assert found > 0                                                 # the case says something
        if (W, H, cell) == (160, 120, 32) and kind == "noise":
            assert found == len(want_k)                                  # every cell overflows
    again_k, again_d = _extract(image, mask, cell, per_cell, threshold, pattern)
    assert again_k.tobytes() == got_k.tobytes() and again_d.tobytes() == got_d.tobytes()


def test_extract_finds_the_one_interior_pixel():
    image = np.zeros((3, 37, 37), np.float32)
    image[:, 18, 18] = 1.0
    image[:, 17, 18] = image[:, 18, 19] = 0.9                            # the border: corners in their own right, but not interior
    want_k, want_d = ref.extract(image, None, 16, 2, 20, DIRECTIONS, PATTERN)
    assert [tuple(r[:3]) for r in want_k if r[0] >= 0] == [(18, 18, 255)] and want_k[2 * (3 + 1)][0] == 18      # cell (1, 1), rank 0
    got_k, got_d = _extract(image, None, 16, 2, 20, PATTERN)
    assert got_k.tobytes() == want_k.tobytes() and got_d.tobytes() == want_d.tobytes()


def test_extract_tie_rules_on_two_level_tiles():
    """Every corner of a two-level image has the same score: suppression and selection are decided by the index rules alone."""
    image, _, _ = _input("tiles", 64, 48)
    want_k, _ = ref.extract(image, None, 16, 3, 5, DIRECTIONS, PATTERN)
    kept = want_k[want_k[:, 0] >= 0]
    assert len(kept) > 4 and len(set(kept[:, 2].tolist())) == 1
    got_k, _ = _extract(image, None, 16, 3, 5, PATTERN)
    assert got_k.tobytes() == want_k.tobytes()


def test_extract_refusals_leave_the_outputs_untouched():
    image = _dev(_input("noise", 64, 48)[0])
    slots = ref.slots(64, 48, 16, 3)
    kbuf, keypoints = _guarded(4 * slots)
    dbuf, descriptors = _guarded(8 * slots)
    d, p = _dev(DIRECTIONS), _dev(PATTERN)
    K, D = keypoints.view(slots, 4), descriptors.view(slots, 8)
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    for text, call in (("cell must be in", lambda: features.extract(image, None, 7, 3, 20, d, p, K, D)),
                       ("per_cell must be in", lambda: features.extract(image, None, 16, 9, 20, d, p, K, D)),
                       ("threshold must be in", lambda: features.extract(image, None, 16, 3, 256, d, p, K, D)),
                       ("threshold must be in", lambda: features.extract(image, None, 16, 3, -1, d, p, K, D)),
                       ("workspace must be 16-byte aligned and hold", lambda: features.extract(image, None, 16, 3, 20, d, p, K, D, workspace=small)),
                       ("keypoints must hold 36 slots", lambda: features.extract(image, None, 16, 3, 20, d, p, K[:35], D))):
        with pytest.raises(RuntimeError, match=text):
            call()
    torch.cuda.synchronize()
    assert bool((kbuf == GUARD).all()) and bool((dbuf == GUARD).all())
    assert features.slot_count(640, 480, 8, 8) == 0 and features.slot_count(640, 480, 32, 4) == 1200


# ---- match --------------------------------------------------------------------------------------------------------------------------------
def _set(n, seed, empty_share=0.1, near=None):
    """n slots of random descriptors; a share of them empty; with `near` = another set's descriptors, most are copies with a few bits flipped"""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 2 ** 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    if near is not None:
        take = rng.integers(0, len(near), size=n)
        flips = np.zeros((n, 8), np.uint32)
        for k in range(n):
            for bit in rng.integers(0, 256, size=rng.integers(0, 40)):
                flips[k, bit // 32] ^= np.uint32(1 << (bit % 32))
        copied = rng.uniform(size=n) < 0.7
        desc = np.where(copied[:, None], near[take] ^ flips, desc)
    kp = np.stack([rng.integers(18, 300, n), rng.integers(18, 200, n), rng.integers(21, 255, n), rng.integers(0, 32, n)], axis=1).astype(np.int32)
    empty = rng.uniform(size=n) < empty_share
    kp[empty] = (-1, -1, 0, 0)
    desc[empty] = 0
    return kp, desc


def _match(a, b, max_distance, ratio_eighths):
    n = len(a[0])
    buf, out = _guarded(2 * n)
    words = lambda d: torch.from_numpy(np.ascontiguousarray(d).view(np.int32)).cuda()
    features.match(_dev(a[0]), words(a[1]), _dev(b[0]), words(b[1]), max_distance, ratio_eighths, out.view(n, 2))
    torch.cuda.synchronize()
    assert _guard_ok(buf, 2 * n)
    return out.view(n, 2).cpu().numpy()


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 200), (200, 3), (65, 64), (1200, 1200)])
def test_match_equals_the_restatement(na, nb):
    b = _set(nb, nb, empty_share=0.1 if nb > 3 else 0.0)
    a = _set(na, na + 7, empty_share=0.1 if na > 3 else 0.0, near=b[1])
    if min(na, nb) >= 64:                                                # duplicated descriptors on both sides: ties go to the lower index
        a[1][5], a[1][40], b[1][9], b[1][33] = a[1][2], a[1][2], b[1][1], b[1][1]
        a[0][[2, 5, 40]], b[0][[1, 9, 33]] = (50, 50, 30, 0), (60, 60, 30, 0)
    for max_distance, ratio in ((64, 6), (256, 8), (30, 4)):
        want = ref.match(*a, *b, max_distance, ratio)
        got = _match(a, b, max_distance, ratio)
        assert got.tobytes() == want.tobytes()
    if min(na, nb) >= 64:
        assert (want[:, 0] >= 0).sum() > na // 4
    assert _match(a, b, 30, 4).tobytes() == got.tobytes()


def test_match_against_an_empty_set_and_bounds_met_exactly():
    a = _set(70, 1, empty_share=0.2)
    b = _set(130, 2, empty_share=1.0)
    got = _match(a, b, 64, 6)
    assert got.tolist() == [[-1, 257]] * 70 and got.tobytes() == ref.match(*a, *b, 64, 6).tobytes()
    word = lambda *bits: np.array([sum(1 << k for k in bits)] + [0] * 7, np.uint32)
    kp = lambda n: np.array([[20 + i, 20, 30, 0] for i in range(n)], np.int32)
    A, B = (kp(1), np.stack([word()])), (kp(2), np.stack([word(0, 1, 2), word(3, 4, 5, 6)]))      # d = 3, second = 4
    for max_distance, ratio, want in ((3, 6, [0, 3]), (2, 6, [-1, 3]), (3, 5, [-1, 3]), (256, 8, [0, 3])):
        assert _match(A, B, max_distance, ratio).tolist() == [want] == ref.match(*A, *B, max_distance, ratio).tolist()
    # a pair that fails the mutual test alone: a1's best is b0, whose best is a0
    A, B = (kp(2), np.stack([word(0), word(0, 1, 2, 3)])), (kp(2), np.stack([word(0, 1), word(8, 9, 10, 11, 12, 13, 14, 15, 16, 17)]))
    got = _match(A, B, 64, 8)
    assert got.tolist() == [[0, 1], [-1, 2]] == ref.match(*A, *B, 64, 8).tolist()


def test_match_refusals_leave_the_output_untouched():
    a, b = _set(10, 1), _set(12, 2)
    buf, out = _guarded(20)
    words = lambda d: torch.from_numpy(np.ascontiguousarray(d).view(np.int32)).cuda()
    args = (_dev(a[0]), words(a[1]), _dev(b[0]), words(b[1]))
    for text, call in (("max_distance must be in", lambda: features.match(*args, 257, 6, out.view(10, 2))),
                       ("ratio_eighths must be in", lambda: features.match(*args, 64, 9, out.view(10, 2))),
                       ("workspace must be 16-byte aligned and hold",
                        lambda: features.match(*args, 64, 6, out.view(10, 2), workspace=torch.empty(16, dtype=torch.uint8, device="cuda")))):
        with pytest.raises(RuntimeError, match=text):
            call()
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())


# ---- pose ---------------------------------------------------------------------------------------------------------------------------------
POSE = dict(seed=0, min_area=features.MIN_AREA, tau_px=2.0, tau_depth=0.05, refine_iters=3, min_matches=12, min_inliers=8, min_share=0.5,
            max_translation=1.5, max_rotation=math.radians(45.0))


def _pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses, **over):
    tbuf, T = _guarded(16, torch.float32)
    sbuf, stats = _guarded(8)
    cbuf, counts = _guarded(hypotheses)
    tbuf[16:] = 7.0
    k = _dev(np.asarray(K, np.float32))
    features.pose(_dev(kp_a), _dev(depth_a), _dev(kp_b), _dev(depth_b), _dev(matches), k, k, T.view(4, 4), stats, hypotheses=hypotheses,
                  counts=counts, **{**POSE, **over})
    torch.cuda.synchronize()
    assert bool((tbuf[16:] == 7.0).all()) and _guard_ok(sbuf, 8) and _guard_ok(cbuf, hypotheses)
    return T.view(4, 4).cpu().numpy(), stats.cpu().numpy(), counts.cpu().numpy()


def _check_pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses, **over):
    opt = {**POSE, **over}
    want = ref.pose(kp_a, depth_a, kp_b, depth_b, matches, K, K, count=hypotheses, **opt)
    T, stats, counts = _pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses, **over)
    assert counts.tolist() == want["counts"].tolist()
    assert stats.tolist() == want["stats"].tolist()
    assert np.all(np.abs(T.astype(np.float64) - want["T"]) <= 2.4e-7 * np.maximum(1.0, np.abs(want["T"])))
    if stats[6] == 0:
        assert T.tobytes() == np.eye(4, dtype=np.float32).tobytes()      # a refusal returns the identity exactly
    T2, stats2, counts2 = _pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses, **over)
    assert T2.tobytes() == T.tobytes() and stats2.tobytes() == stats.tobytes() and counts2.tobytes() == counts.tobytes()
    return T, stats, want


_scene_cases = {}


def _scene_case(name):
    """keypoints and matches of a scene at 160 x 120 by the restatement: the pose kernels are tested on their own"""
    if name not in _scene_cases:
        image_a, depth_a, image_b, depth_b, K, T_true = ref.scene(name, 160, 120)
        a = ref.extract(image_a, None, 16, 3, 20, DIRECTIONS, PATTERN)
        b = ref.extract(image_b, None, 16, 3, 20, DIRECTIONS, PATTERN)
        _scene_cases[name] = (a[0], depth_a, b[0], depth_b, ref.match(*a, *b, 64, 6), K, T_true)
    return _scene_cases[name]


@pytest.mark.parametrize("hypotheses", [1, 64, 1024])
@pytest.mark.parametrize("name", ["wider", "roll", "unrelated"])
def test_pose_on_the_scene_equals_the_restatement(name, hypotheses):
    kp_a, depth_a, kp_b, depth_b, matches, K, T_true = _scene_case(name)
    T, stats, want = _check_pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses)
    if name != "unrelated" and hypotheses >= 64:
        assert stats[6] == 1
        degrees, mm = odo.pose_error(T.astype(np.float64), T_true)
        assert degrees <= 0.5 and mm <= 10.0
    if name == "unrelated":
        assert stats[6] == 0


@pytest.mark.parametrize("M", [0, 2, 3])
def test_pose_with_few_pairs(M):
    kp_a, depth_a, kp_b, depth_b, matches, K, _ = _scene_case("wider")
    few = matches.copy()
    hit = np.nonzero(few[:, 0] >= 0)[0]
    keep = hit[np.linspace(0, len(hit) - 1, M).astype(int)] if M else hit[:0]       # spread over the frame: no thin triangle
    few[np.setdiff1d(hit, keep), 0] = -1
    _, stats, _ = _check_pose(kp_a, depth_a, kp_b, depth_b, few, K, 64, min_matches=0, min_inliers=3, min_share=0.0)
    assert stats[2] == M
    if M == 3:
        assert stats[4] == 3 and stats[6] == 1                           # three exact pairs: one triangle, every pair its inlier


def test_pose_leaves_out_keypoints_on_invalid_depth():
    kp_a, depth_a, kp_b, depth_b, matches, K, _ = _scene_case("wider")
    depth_a, depth_b = depth_a.copy(), depth_b.copy()
    hit = np.nonzero(matches[:, 0] >= 0)[0]
    for k, bad in enumerate((0.0, np.nan, -1.0, np.inf)):
        depth_a[kp_a[hit[k], 1], kp_a[hit[k], 0]] = bad
        b = matches[hit[k + 4], 0]
        depth_b[kp_b[b, 1], kp_b[b, 0]] = bad
    _, stats, _ = _check_pose(kp_a, depth_a, kp_b, depth_b, matches, K, 256)
    assert stats[2] == len(hit) - 8


@pytest.mark.parametrize("hypotheses", [1, 64, 1024])
def test_pose_of_1200_pairs_with_outliers(hypotheses):
    rng = np.random.default_rng(11)
    W, H, n = 320, 240, 1200
    K = tuple(float(np.float32(v)) for v in odo.intrinsics(W, H))
    T_true = ref.MOTIONS["wide"]
    cells = rng.permutation((W // 4) * (H // 4))[:n]                     # distinct pixels of B on a 4-pixel lattice
    kp_b = np.stack([4 * (cells % (W // 4)) + 1, 4 * (cells // (W // 4)) + 1, np.full(n, 30), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    depth_b = rng.uniform(1.5, 3.5, (H, W)).astype(np.float32)
    zb = depth_b[kp_b[:, 1], kp_b[:, 0]].astype(np.float64)
    PB = np.stack([(kp_b[:, 0] - K[2]) * zb / K[0], (kp_b[:, 1] - K[3]) * zb / K[1], zb], axis=1)
    PA = (PB - T_true[:3, 3]) @ T_true[:3, :3]
    depth_a = np.full((H, W), 0.0, np.float32)
    xa = np.rint(K[0] * PA[:, 0] / PA[:, 2] + K[2]).astype(np.int64)
    ya = np.rint(K[1] * PA[:, 1] / PA[:, 2] + K[3]).astype(np.int64)
    inside = (xa >= 0) & (xa < W) & (ya >= 0) & (ya < H) & (PA[:, 2] > 0)
    xa, ya = np.where(inside, xa, 0), np.where(inside, ya, 0)
    depth_a[ya[inside], xa[inside]] = PA[inside, 2]                      # pixels hit twice keep the later depth: a few more outliers
    kp_a = np.stack([xa, ya, np.full(n, 30), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    kp_a[~inside] = (-1, -1, 0, 0)
    matches = np.stack([np.arange(n), np.full(n, 10)], axis=1).astype(np.int32)
    wrong = rng.uniform(size=n) < 0.3
    matches[wrong, 0] = rng.integers(0, n, size=int(wrong.sum()))        # 30 % outliers
    matches[~inside, 0] = -1
    T, stats, _ = _check_pose(kp_a, depth_a, kp_b, depth_b, matches, K, hypotheses)
    if hypotheses >= 64:
        assert stats[6] == 1 and stats[5] >= 0.5 * stats[2]
        degrees, mm = odo.pose_error(T.astype(np.float64), T_true)
        assert degrees <= 0.5 and mm <= 10.0


def test_pose_refusals_leave_the_outputs_untouched():
    kp_a, depth_a, kp_b, depth_b, matches, K, _ = _scene_case("wider")
    tbuf, T = _guarded(16, torch.float32)
    sbuf, stats = _guarded(8)
    k = _dev(np.asarray(K, np.float32))
    args = (_dev(kp_a), _dev(depth_a), _dev(kp_b), _dev(depth_b), _dev(matches), k, k, T.view(4, 4), stats)
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    before = tbuf.clone()
    for text, over in (("hypotheses must be in", {"hypotheses": 0}), ("hypotheses must be in", {"hypotheses": 1025}),
                       ("min_area must be positive", {"min_area": 0.0}), ("tau_px and tau_depth", {"tau_px": -1.0}),
                       ("tau_px and tau_depth", {"tau_depth": float("nan")}), ("refine_iters must be in", {"refine_iters": 17}),
                       ("min_inliers must be at least 3", {"min_inliers": 2}), ("min_share must be in", {"min_share": 1.5}),
                       ("max_translation and max_rotation", {"max_rotation": -0.1}),
                       ("workspace must be 16-byte aligned and hold", {"workspace": small})):
        with pytest.raises(RuntimeError, match=text):
            features.pose(*args, **{**POSE, "hypotheses": 64, **over})
    torch.cuda.synchronize()
    assert bool((sbuf == GUARD).all()) and torch.equal(tbuf, before)


# ---- the three calls in a graph, and the stage object ---------------------------------------------------------------------------------------
def test_the_seeder_end_to_end_equals_the_restatement_and_replays_in_a_graph():
    image_a, depth_a, image_b, depth_b, K, T_true = ref.scene("wider", 160, 120)
    opt = features.default_options(cell=16, per_cell=3)
    seeder = features.FeatureSeeder((160, 120), K, opt, "cuda:0")
    ia, ib, da, db = _dev(image_a), _dev(image_b), _dev(depth_a), _dev(depth_b)
    a, b = seeder.features(ia), seeder.cached("b", ib)
    assert seeder.cached("b", ia)[0] is b[0]                             # a cached frame is not extracted again
    T, stats = seeder.pose(a, da, b, db)
    want_a = ref.extract(image_a, None, 16, 3, 20, DIRECTIONS, PATTERN)
    want_b = ref.extract(image_b, None, 16, 3, 20, DIRECTIONS, PATTERN)
    assert a[0].cpu().numpy().tobytes() == want_a[0].tobytes() and b[1].cpu().numpy().view(np.uint32).tobytes() == want_b[1].tobytes()
    want = ref.pose(want_a[0], depth_a, want_b[0], depth_b, ref.match(*want_a, *want_b, 64, 6), K, K, count=256, **POSE)
    assert stats.tolist() == want["stats"].tolist() and stats[6] == 1
    assert np.all(np.abs(T.cpu().numpy().astype(np.float64) - want["T"]) <= 2.4e-7 * np.maximum(1.0, np.abs(want["T"])))
    degrees, mm = odo.pose_error(T.cpu().numpy().astype(np.float64), T_true)
    assert degrees <= 0.5 and mm <= 10.0
    assert seeder.summary() == {"feature_seeds_tried": 1, "feature_seeds_accepted": 1}
    eager = (T.clone(), stats.clone())
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ga, gb = seeder.features(ia), seeder.features(ib)
            gT, gstats = seeder.pose(ga, da, gb, db)
    torch.cuda.current_stream().wait_stream(stream)
    gT.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gT, eager[0]) and torch.equal(gstats, eager[1])


# ---- the stage in use: loop verification ----------------------------------------------------------------------------------------------------
SEED_SMALL = {"enabled": True, "cell": 16, "per_cell": 3}               # 240 slots at 160 x 120


class _Frame:
    """What LoopCloser.verify reads of a camera"""

    def __init__(self, image, depth, T=None):
        T = np.eye(4) if T is None else T
        self.original_image, self._depth = _dev(image), _dev(depth)
        self.R, self.T = _dev(T[:3, :3], torch.float32), _dev(T[:3, 3], torch.float32)

    def depth_device(self):
        return self._depth


def _closer(name, seeded, stored=None):
    """A LoopCloser over the two views of a scene at 160 x 120; stored: the pose the second camera claims (default: the identity)"""
    from slam.loop_closure import LoopCloser
    from slam.stages import loop_closure_options
    image_a, depth_a, image_b, depth_b, K, T_true = ref.scene(name, 160, 120)
    training = {"loop_closure": {"enabled": True}, "feature_seed": SEED_SMALL}
    cameras = {0: _Frame(image_a, depth_a), 1: _Frame(image_b, depth_b, stored)}
    seed = features.feature_seed_options(training) if seeded else None
    return LoopCloser(loop_closure_options(training), cameras, lambda: None, (160, 120), K, "cuda:0", feature_seed=seed), T_true


def test_verify_accepts_a_wide_pair_from_the_feature_seed_and_refuses_it_without():
    """Two cameras whose stored poses claim the identity between them, 26 degrees and 0.97 m apart in truth. Without the seed the
    alignment starts at the identity and the pair is refused; with it the pair is accepted, as close to the truth as verify() gets when it
    is GIVEN the true relative pose as its start (the unchanged path with the true pose stored), within a factor of two."""
    told, T_true = _closer("wider", False, stored=ref.MOTIONS["wider"])
    ok_told, T_told, info_told = told.verify(0, 1)
    base_deg, base_mm = odo.pose_error(T_told.cpu().numpy().astype(np.float64), T_true)
    off, _ = _closer("wider", False)
    ok_off, T_off, info_off = off.verify(0, 1)
    on, _ = _closer("wider", True)
    ok_on, T_on, info_on = on.verify(0, 1)
    deg, mm = odo.pose_error(T_on.cpu().numpy().astype(np.float64), T_true)
    print(f"verify on 'wider': told the truth {ok_told} {base_deg:.4f} deg {base_mm:.3f} mm {info_told}; from the identity {ok_off} {info_off}; "
          f"seeded {ok_on} {deg:.4f} deg {mm:.3f} mm {info_on}")
    assert ok_told and not ok_off and "seeded" not in info_off
    assert ok_on and info_on["seeded"]
    assert deg <= 2.0 * base_deg and mm <= 2.0 * base_mm
    assert on.stats["feature_seeds_tried"] == 1 and on.stats["feature_seeds_accepted"] == 1 and "feature_seeds_tried" not in off.stats
    assert on.summary()["feature_seeds_accepted"] == 1


def test_verify_of_unrelated_frames_is_what_it_is_without_the_seed():
    off, _ = _closer("unrelated", False)
    ok_off, T_off, info_off = off.verify(0, 1)
    on, _ = _closer("unrelated", True)
    ok_on, T_on, info_on = on.verify(0, 1)
    print(f"verify on 'unrelated': without {ok_off} {info_off}; with {ok_on} {info_on}")
    assert info_on.pop("seeded") is False and on.stats["feature_seeds_accepted"] == 0
    assert ok_on == ok_off and torch.equal(T_on, T_off) and info_on == info_off


def test_verify_on_the_blocks_room_reaches_pairs_twelve_frames_apart():
    """The rendered room with the blocks texture (points at 1.5 cm), camera steps of DESIGN.md's loop-verification table: frames 12 apart
    (24 cm, 6 to 8 degrees) whose stored poses claim the identity. Measured on an MI355X: 0 of 7 accepted without the seed, 7 of 7 with
    (and 7 of 7 seeds accepted; the result 1.5 to 1.9 mm and 0.05 degrees from the truth); three of the seven are run here."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.loop_closure import LoopCloser
    from slam.stages import loop_closure_options
    ds = SyntheticRGBDDataset(num_frames=19, width=320, height=240, seed=0, step=0.02, rot_step=0.012, texture="blocks")
    assert ds.spacing == 0.015
    training = {"loop_closure": {"enabled": True}, "feature_seed": {"enabled": True, "cell": 16, "per_cell": 4}}
    cameras = {i: _Frame(ds[i][0].cpu().numpy(), np.asarray(ds[i][1], np.float32)) for i in (1, 3, 6, 13, 15, 18)}
    K = (ds.fx, ds.fy, ds.cx, ds.cy)
    build = lambda seed: LoopCloser(loop_closure_options(training), cameras, lambda: None, (320, 240), K, "cuda:0", feature_seed=seed)
    on, off = build(features.feature_seed_options(training)), build(None)
    for a in (1, 3, 6):
        ok_off, _, info_off = off.verify(a, a + 12)
        ok_on, T_on, info_on = on.verify(a, a + 12)
        truth = ds.poses[a + 12].double().cpu().numpy() @ np.linalg.inv(ds.poses[a].double().cpu().numpy())
        degrees, mm = odo.pose_error(T_on.cpu().numpy().astype(np.float64), truth)
        print(f"blocks room {a} -> {a + 12}: without {ok_off} {info_off}; with {ok_on} {info_on}; {degrees:.3f} deg {mm:.2f} mm from the truth")
        assert not ok_off and ok_on and info_on["seeded"]
        assert degrees <= 0.5 and mm <= 10.0                               # the bars of the sparse pose itself; the alignment refines it
    assert on.stats["feature_seeds_accepted"] == 3


# ---- the stage in use: a saved map, a run -----------------------------------------------------------------------------------------------------
FRAMES, WIDTH, HEIGHT = 40, 320, 240
TRAINING = {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": 60, "static_map_iters": 30,
            "gaussian_update_every": 60, "gaussian_update_offset": 20, "tracking_graph": True}
FAR_R, FAR_T = torch.eye(3), torch.tensor([5.0, -4.0, 6.0])
STAGES = {"relocalisation": {"enabled": True}, "loop_closure": {"enabled": True}}


def _slam(dataset, training_addition):
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    cfg = merge_config(default_config(), {"Training": TRAINING, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 150}, "Results": {"eval_rendering": False}})
    cfg = merge_config(cfg, {"Training": training_addition})
    slam = SLAM(cfg, dataset)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    return slam.run(), slam


def _ate(cameras, ids, poses=None):
    """RMSE of the camera centres over `ids` after one rigid fit over them; poses {id: (R, T)} overrides the cameras' estimates"""
    from slam.eval_utils import align
    centre = lambda R, T: -R.detach().double().cpu().numpy().T @ T.detach().double().cpu().numpy()
    est = lambda i: centre(*(poses[i] if poses is not None else (cameras[i].R, cameras[i].T)))
    gt = lambda i: centre(cameras[i].R_gt, cameras[i].T_gt)
    rot, trans, _ = align(np.stack([est(i) for i in ids]).T, np.stack([gt(i) for i in ids]).T)
    return float(np.sqrt(np.mean([np.linalg.norm(rot @ est(i) + trans[:, 0] - gt(i)) ** 2 for i in ids])))


@pytest.fixture(scope="module")
def blocks_run():
    """The one run of the module on the blocks texture with relocalisation and loop closure on and the seed off: (result, slam, dataset)"""
    from slam.dataset import SyntheticRGBDDataset
    ds = SyntheticRGBDDataset(num_frames=FRAMES, width=WIDTH, height=HEIGHT, seed=0, texture="blocks")
    result, slam = _slam(ds, STAGES)
    return result, slam, ds


@pytest.fixture(scope="module")
def saved_map(blocks_run, tmp_path_factory):
    _, slam, _ = blocks_run
    directory = str(tmp_path_factory.mktemp("features") / "map")
    slam.save_map(directory)
    return directory


def _localise_all(saved_map, blocks_run, seeded):
    from slam.map_io import load_map
    from slam.relocalise import MapLocaliser
    from slam.system import merge_config
    _, slam, ds = blocks_run
    config = merge_config(slam.config, {"Training": {"feature_seed": {"enabled": seeded}}})
    loc = MapLocaliser(load_map(saved_map), config)
    cameras, keyframes = slam.frontend.cameras, set(slam.frontend.kf_indices)
    others = [i for i in sorted(cameras) if i not in keyframes]
    poses, found = {}, []
    for i in others:
        viewpoint = loc.camera(ds, i)
        viewpoint.update_RT(FAR_R, FAR_T)
        found.append(loc.localise(viewpoint))
        poses[i] = (viewpoint.R.detach().clone(), viewpoint.T.detach().clone())
    return loc, others, poses, found


def test_every_frame_is_found_in_the_saved_map_with_the_seed_on(blocks_run, saved_map):
    """The bar of tests/test_hip_relocalise.py on the blocks texture: every non-keyframe is found from a pose metres away, with an ATE of
    at most twice the run's own over these frames; and the seed is accepted for some of them (measured on an MI355X, points at 1.5 cm: 32
    of 32 found, 32 of 32 seeds accepted, ATE 0.64 mm with and without the seed against the run's own 2.01 mm; at 3 cm 3 seeds of 32). With
    the block off the relocaliser has no seeder, makes today's calls, and gives the same poses twice."""
    _, slam, _ = blocks_run
    cameras = slam.frontend.cameras
    loc, others, poses, found = _localise_all(saved_map, blocks_run, True)
    run_ate, loc_ate = _ate(cameras, others), _ate(cameras, others, poses)
    seeds = loc.relocaliser.seeder.summary()
    print(f"saved blocks map, seed on: {len(others)} frames, accepted {sum(o['accepted'] for o in found)}, seeds {seeds}, ATE of the run "
          f"{run_ate * 1000:.2f} mm, of the localised poses {loc_ate * 1000:.2f} mm")
    assert len(others) >= 20 and all(o["accepted"] for o in found)
    assert loc_ate <= 2.0 * run_ate
    assert seeds["feature_seeds_tried"] >= len(others) and seeds["feature_seeds_accepted"] > 0
    off, _, poses_off, found_off = _localise_all(saved_map, blocks_run, False)
    assert off.relocaliser.seeder is None and off.feature_seed is None and all(o["accepted"] for o in found_off)
    again, _, poses_again, _ = _localise_all(saved_map, blocks_run, False)
    assert all(torch.equal(poses_off[i][0], poses_again[i][0]) and torch.equal(poses_off[i][1], poses_again[i][1]) for i in others)
    off_ate = _ate(cameras, others, poses_off)
    print(f"saved blocks map, seed off: ATE of the localised poses {off_ate * 1000:.2f} mm")
    assert off_ate <= 2.0 * run_ate


def test_a_run_with_the_seed_on_loses_no_frame(blocks_run):
    """Relocalisation, loop closure and the seed on against the same run with the seed off. The run is reproducible bit for bit (two runs
    of one configuration give equal poses: tests/test_hip_relocalise.py holds that), so the spread of three repetitions is zero and the
    seeded run may not be worse at all, beyond the rounding of the ATE's own arithmetic. Measured: 2.187 mm both -- no frame is lost and
    no candidate is old enough in 40 frames, so the seed is never asked and every pose is the same."""
    from slam.dataset import SyntheticRGBDDataset
    off, slam_off, _ = blocks_run
    ds = SyntheticRGBDDataset(num_frames=FRAMES, width=WIDTH, height=HEIGHT, seed=0, texture="blocks")
    on, slam_on = _slam(ds, {**STAGES, "feature_seed": {"enabled": True}})
    ids = sorted(slam_on.frontend.cameras)
    ate_on, ate_off = _ate(slam_on.frontend.cameras, ids), _ate(slam_off.frontend.cameras, ids)
    print(f"run with the seed on: ATE {ate_on * 1000:.3f} mm, off {ate_off * 1000:.3f} mm; relocalisation {on['relocalisation']}; "
          f"loop closure {on['loop_closure']}")
    assert on["relocalisation"]["lost"] == 0 and len(ids) == FRAMES
    assert "feature_seeds_tried" in on["relocalisation"] and "feature_seeds_tried" in on["loop_closure"]
    assert "feature_seeds_tried" not in off["relocalisation"] and "feature_seeds_tried" not in off["loop_closure"]
    assert ate_on <= ate_off + 1e-9
