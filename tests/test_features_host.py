"""Host-side checks of the feature-seed stage (slam/features.py, include/feature_matching.h): the numpy restatement of the three kernels
(tests/features_reference.py) on cases small enough to work out by hand and on the analytic scene -- how far the sparse pose reaches, what
it refuses, what depth noise does to it --, the tables, and the ``Training.feature_seed`` options. No GPU needed."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import features_reference as ref  # noqa: E402
import odometry_reference as odo  # noqa: E402
from slam import features  # noqa: E402

SIZES = [(160, 120), (161, 97)]
CELL, PER_CELL, THRESHOLD, MAX_DISTANCE, RATIO = 16, 3, 20, 64, 6       # the prototype's values at these sizes
DIRECTIONS, PATTERN = features.pattern_tables(0)
_poses = {}


def _pose(name, W, H, noise=0.0):
    """The restatement's pipeline on one scene, computed once per case"""
    key = (name, W, H, noise)
    if key not in _poses:
        image_a, depth_a, image_b, depth_b, K, T_true = ref.scene(name, W, H)
        if noise:
            rng = np.random.default_rng(W + H)
            depth_a = (depth_a * (1.0 + noise * rng.standard_normal(depth_a.shape))).astype(np.float32)
            depth_b = (depth_b * (1.0 + noise * rng.standard_normal(depth_b.shape))).astype(np.float32)
        a = ref.extract(image_a, None, CELL, PER_CELL, THRESHOLD, DIRECTIONS, PATTERN)
        b = ref.extract(image_b, None, CELL, PER_CELL, THRESHOLD, DIRECTIONS, PATTERN)
        matches = ref.match(*a, *b, MAX_DISTANCE, RATIO)
        _poses[key] = (ref.pose(a[0], depth_a, b[0], depth_b, matches, K, K, min_area=features.MIN_AREA), T_true)
    return _poses[key]


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------------
def test_luma_and_fast_score_by_hand():
    image = np.zeros((3, 9, 9), np.float32)
    image[:, 4, 4] = 1.0                                                 # one white pixel: every circle pixel is 255 darker
    L = ref.luma(image)
    assert L[4, 4] == 255 and L.sum() == 255
    score = ref.fast_score(L)
    assert score[4, 4] == 255                                            # dark: min over any 9 of (255 - 0)
    assert score[4, 1] == 0 and score[1, 4] == 0                         # one bright pixel on the circle is no arc of 9
    L2 = np.zeros((9, 9), np.int64)
    L2[:, 5:] = 100                                                      # a straight edge: at most 7 of the 16 are brighter than x = 4 ...
    assert ref.fast_score(L2)[4, 4] == 0
    L2[:4, :] = 100                                                      # ... a corner of 270 degrees bright: 11 in a row
    assert ref.fast_score(L2)[4, 4] == 100
    assert ref.luma(np.full((3, 1, 1), np.nan, np.float32))[0, 0] == 0
    weights = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32).reshape(3, 3, 1)
    assert ref.luma(weights)[:, 0].tolist() ==[(77 * 255 + 128) >> 8, (150 * 255 + 128) >> 8, (29 * 255 + 128) >> 8]


def test_suppression_and_selection_tie_rules_by_hand():
    c = np.zeros((6, 6), np.int64)
    c[2, 2] = c[2, 3] = c[3, 2] = 50                                     # three equal neighbours: the smallest index stays
    c[5, 5] = 40
    kept = ref.suppress(c)
    assert kept[2, 2] and not kept[2, 3] and not kept[3, 2] and kept[5, 5] and kept.sum() == 2
    c[3, 3] = 51                                                         # a larger neighbour removes all three
    assert ref.suppress(c).sum() == 2 and ref.suppress(c)[3, 3]


def test_match_rules_by_hand():
    word = lambda *bits: np.array([sum(1 << b for b in bits)] + [0] * 7, np.uint32)
    kp = lambda n, empty=(): np.array([[-1, -1, 0, 0] if i in empty else [20 + i, 20, 30, 0] for i in range(n)], np.int32)
    A = np.stack([word(), word(0, 1, 2, 3), word(5)])
    B = np.stack([word(0), word(), word(), word(0, 1, 2, 3, 4, 6, 7, 8)])
    got = ref.match(kp(3), A, kp(4), B, 64, 8)
    # a0: d = 1, 0, 0, 8 -> best b1 (the lower of two zeros), second 0: 8 * 0 <= 8 * 0 holds; b1's best over A is a0: accepted
    # a1: d = 3, 4, 4, 4 -> best b0, second 4, 24 <= 32; but b0's best over A is a0 (1 < 3): fails the mutual test alone
    # a2: d = 2, 1, 1, 9 -> best b1; b1's best is a0: refused
    assert got.tolist() == [[1, 0], [-1, 3], [-1, 1]]
    assert ref.match(kp(3), A, kp(4), B, 64, 5)[1].tolist() == [-1, 3]
    assert ref.match(kp(3, empty=(0,)), A, kp(4), B, 64, 8)[0].tolist() == [-1, 257]
    assert ref.match(kp(3), A, kp(4, empty=(0, 1, 2, 3)), B, 64, 8).tolist() == [[-1, 257]] * 3
    one = ref.match(kp(1), A[1:2], kp(1), B[3:4], 4, 0)                  # second is 257 where there is no other: ratio 0 needs d = 0
    assert one.tolist() == [[-1, 4]]
    assert ref.match(kp(1), A[1:2], kp(1), B[3:4], 4, 1).tolist() == [[0, 4]]
    assert ref.match(kp(1), A[1:2], kp(1), B[3:4], 3, 8).tolist() == [[-1, 4]]


def test_lowbias32_and_pose_of_a_planted_motion():
    assert int(ref.lowbias32(0)) == 0 and len({int(ref.lowbias32(k)) for k in range(1000)}) == 1000      # a bijection of uint32
    rng = np.random.default_rng(3)
    T_true = ref.MOTIONS["wide"]
    K = odo.intrinsics(64, 48)
    n = 40
    kp_a = np.stack([rng.integers(0, 64, n), rng.integers(0, 48, n), np.full(n, 30), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    depth_a = rng.uniform(1.0, 3.0, (48, 64)).astype(np.float32)
    PA = np.stack([(kp_a[:, 0] - K[2]) * depth_a[kp_a[:, 1], kp_a[:, 0]] / K[0], (kp_a[:, 1] - K[3]) * depth_a[kp_a[:, 1], kp_a[:, 0]] / K[1],
                   depth_a[kp_a[:, 1], kp_a[:, 0]]], axis=1)
    PB = PA @ T_true[:3, :3].T + T_true[:3, 3]
    # frame B is given as a list of points: its keypoints sit on a row of a wide depth image whose pixel k holds the depth of point k
    # and whose intrinsics make the back-projection of pixel k the point: only gsr_feat_pose's algebra is under test here
    matches = np.stack([np.arange(n), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    P_a, P_b, _, _ = ref.pair_list(kp_a, depth_a, kp_a, depth_a, matches, K, K)
    assert len(P_a) == n and np.allclose(P_a, PA, atol=1e-5)
    R, t, valid = ref.hypotheses(P_a, PB.astype(np.float32), 0, 64, 0.05)
    assert valid.sum() > 32
    err = max(np.abs(R[h] - T_true[:3, :3]).max() for h in np.nonzero(valid)[0])
    assert err < 2e-4                                                    # exact pairs: every valid hypothesis is the planted motion
    R2, t2 = ref.refine(R[np.nonzero(valid)[0][0]], t[np.nonzero(valid)[0][0]], P_a, PB, 3)
    assert np.abs(R2 - T_true[:3, :3]).max() < 1e-6 and np.abs(t2 - T_true[:3, 3]).max() < 1e-6


# ---- the analytic scene -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["wide", "roll", "wider"])
def test_wide_baselines_are_accepted_and_accurate(name, W, H):
    """Measured with this restatement (Feature seed): 33 to 65 pairs, inlier shares 0.96 to 0.98, 0.04 to 0.21
    degrees and 0.5 to 3.5 mm after refinement."""
    out, T_true = _pose(name, W, H)
    keypoints_a, keypoints_b, M, winner, best, final, accepted, _ = out["stats"].tolist()
    degrees, mm = odo.pose_error(out["T_refined"], T_true)
    print(f"{name} {W}x{H}: {keypoints_a}/{keypoints_b} keypoints, M {M}, inliers {final}, {degrees:.3f} deg, {mm:.2f} mm")
    assert accepted == 1
    assert M >= 20 and final >= 0.8 * M
    assert degrees <= 0.5 and mm <= 10.0
    assert np.array_equal(out["T"], out["T_refined"].astype(np.float32))


@pytest.mark.parametrize("W,H", SIZES)
def test_unrelated_textures_are_refused(W, H):
    out, _ = _pose("unrelated", W, H)
    print(f"unrelated {W}x{H}: stats {out['stats'].tolist()}")
    assert out["stats"][6] == 0 and out["stats"][2] <= 9 and out["stats"][5] <= 1
    assert np.array_equal(out["T"], np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["wide", "roll", "wider"])
def test_one_percent_depth_noise_keeps_the_seed_usable(name, W, H):
    out, T_true = _pose(name, W, H, noise=0.01)
    assert out["T_refined"] is not None
    degrees, mm = odo.pose_error(out["T_refined"], T_true)
    print(f"{name} {W}x{H} with 1 % depth noise: stats {out['stats'].tolist()}, {degrees:.3f} deg, {mm:.1f} mm")
    assert degrees <= 2.0 and mm <= 100.0


def test_the_motions_are_what_their_names_say():
    size = lambda T: (np.rad2deg(odo.rotation_angle(T[:3, :3])), float(np.linalg.norm(T[:3, 3])))
    for name, (degrees, metres) in {"small": (2.0, 0.05), "wide": (16.0, 0.63), "roll": (30.0, 0.30), "wider": (26.0, 0.97)}.items():
        got = size(ref.MOTIONS[name])
        assert abs(got[0] - degrees) < 0.01 and abs(got[1] - metres) < 0.012, (name, got)


# ---- tables and options -------------------------------------------------------------------------------------------------------------------
def test_pattern_tables():
    for seed in (0, 1, 12345):
        directions, pattern = features.pattern_tables(seed)
        assert directions.dtype == np.int32 and directions.shape == (32, 2) and pattern.dtype == np.int8 and pattern.shape == (32, 256, 4)
        assert pattern.min() >= -16 and pattern.max() <= 16
        assert directions[0].tolist() == [256, 0] and directions[8].tolist() == [0, 256] and directions[16].tolist() == [-256, 0]
        again = features.pattern_tables(seed)
        assert again[0].tobytes() == directions.tobytes() and again[1].tobytes() == pattern.tobytes()
        quarter = np.stack([-pattern[0, :, 1], pattern[0, :, 0], -pattern[0, :, 3], pattern[0, :, 2]], axis=1)
        assert np.abs(pattern[8].astype(int) - quarter).max() <= 1        # bin 8 is bin 0 turned by a quarter, up to the rounding
    assert features.pattern_tables(0)[1].tobytes() != features.pattern_tables(1)[1].tobytes()


def _training(**block):
    return {"relocalisation": {"enabled": True}, "feature_seed": {"enabled": True, **block}}


def test_options_defaults_and_refusals():
    assert features.feature_seed_options({}) is None
    assert features.feature_seed_options({"feature_seed": {"enabled": False, "nonsense": 1}}) is None
    opt = features.feature_seed_options(_training())
    assert {k: opt[k] for k in ("threshold", "cell", "per_cell", "seed", "max_distance", "ratio_eighths", "hypotheses", "tau_px", "tau_depth")} == \
        {"threshold": 20, "cell": 32, "per_cell": 4, "seed": 0, "max_distance": 64, "ratio_eighths": 6, "hypotheses": 256, "tau_px": 2.0,
         "tau_depth": 0.05}
    assert ref.slots(640, 480, opt["cell"], opt["per_cell"]) == 1200
    assert features.feature_seed_options({"loop_closure": {"enabled": True}, "feature_seed": {"enabled": True}}) is not None
    with pytest.raises(ValueError, match=r"Training.feature_seed: unknown keys \['octaves'\]"):
        features.feature_seed_options(_training(octaves=3))
    with pytest.raises(ValueError, match="Training.feature_seed cannot be used with monocular input: a frame has no depth"):
        features.feature_seed_options({**_training(), "monocular": True})
    with pytest.raises(ValueError, match="Training.feature_seed needs Training.relocalisation or Training.loop_closure enabled"):
        features.feature_seed_options({"feature_seed": {"enabled": True}})
    with pytest.raises(ValueError, match="Training.feature_seed needs Training.relocalisation or Training.loop_closure enabled"):
        features.feature_seed_options({"relocalisation": {"enabled": False}, "feature_seed": {"enabled": True}})
    for key, bad, text in (("threshold", 256, r"threshold must be in \[0, 255\], got 256"), ("cell", 7, r"cell must be in \[8, 64\], got 7"),
                           ("cell", 65, r"cell must be in \[8, 64\], got 65"), ("per_cell", 0, r"per_cell must be in \[1, 8\], got 0"),
                           ("per_cell", 9, r"per_cell must be in \[1, 8\], got 9"), ("seed", -1, "seed must be in"),
                           ("max_distance", 257, r"max_distance must be in \[0, 256\], got 257"),
                           ("ratio_eighths", 9, r"ratio_eighths must be in \[0, 8\], got 9"),
                           ("hypotheses", 0, r"hypotheses must be in \[1, 1024\], got 0"),
                           ("hypotheses", 1025, r"hypotheses must be in \[1, 1024\], got 1025"),
                           ("min_inliers", 2, r"min_inliers must be in \[3, 4096\], got 2"),
                           ("refine_iters", 17, r"refine_iters must be in \[0, 16\], got 17"),
                           ("cell", 16.5, "cell must be an integer, got 16.5"), ("tau_px", -1.0, "tau_px must be finite and not negative"),
                           ("tau_depth", float("inf"), "tau_depth must be finite and not negative"),
                           ("tau_px", float("nan"), "tau_px must be a number, got nan"), ("min_share", 1.5, r"min_share must be in \[0, 1\]"),
                           ("max_translation", -0.1, "max_translation must not be negative"),
                           ("max_translation", float("inf"), "max_translation must be finite"),
                           ("max_rotation", 181.0, "max_rotation is in degrees and must not exceed 180")):
        with pytest.raises(ValueError, match="Training.feature_seed." + text):
            features.feature_seed_options(_training(**{key: bad}))
    assert features.default_options(cell=16)["cell"] == 16
