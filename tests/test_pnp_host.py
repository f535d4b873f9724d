"""Host-side checks of the pose from 2D-3D matches (gsr_feat_pose_pnp, include/feature_matching.h) through its numpy restatement
(tests/pnp_reference.py): how far the minimal solver reaches from the keyframe's ranges, that exact correspondences give the planted motion,
the analytic scenes of tests/features_reference.py, that no depth of frame B enters, and the ``solver`` option. No GPU needed."""
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
import pnp_reference as pnp  # noqa: E402
from slam import features  # noqa: E402

SIZES = [(160, 120), (161, 97)]
CELL, PER_CELL, THRESHOLD, MAX_DISTANCE, RATIO = 16, 3, 20, 64, 6
DIRECTIONS, PATTERN = features.pattern_tables(0)
_cases = {}


def _case(name, W, H):
    """(keypoints of A, depth of A, keypoints of B, depth of B, matches, K, the true motion) by the restatement, once per case"""
    if (name, W, H) not in _cases:
        image_a, depth_a, image_b, depth_b, K, T_true = ref.scene(name, W, H)
        a = ref.extract(image_a, None, CELL, PER_CELL, THRESHOLD, DIRECTIONS, PATTERN)
        b = ref.extract(image_b, None, CELL, PER_CELL, THRESHOLD, DIRECTIONS, PATTERN)
        _cases[(name, W, H)] = (a[0], depth_a, b[0], depth_b, ref.match(*a, *b, MAX_DISTANCE, RATIO), K, T_true)
    return _cases[(name, W, H)]


# ---- the minimal solver ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees,metres", [(10.0, 0.3), (30.0, 1.0), (45.0, 1.5)])
def test_the_solver_reaches_the_true_ranges_from_those_of_the_keyframe(degrees, metres):
    """Random triples (pixels 20 px inside a 640 x 480 frame, depths of 1 to 4 m, a triad of A that passes min_area 0.05) under random
    motions of up to `degrees` and `metres`, kept where all three project inside B with z > 0.3; B's pixels are rounded to integers. Newton
    from A's ranges must end within 2 % of B's true ranges for 0.9 of them. Measured: 0.949 to 0.957 of 1413 to 4646 kept triples per class."""
    rng = np.random.default_rng(int(degrees))
    W, H = 640, 480
    fx, fy, cx, cy = (float(np.float32(k)) for k in odo.intrinsics(W, H))
    n = 6000
    x, y = rng.uniform(20, W - 20, (n, 3)), rng.uniform(20, H - 20, (n, 3))
    z = rng.uniform(1.0, 4.0, (n, 3))
    PA = np.stack([(x - cx) * z / fx, (y - cy) * z / fy, z], axis=-1).astype(np.float32)          # [n, 3 points, 3]
    axes = rng.standard_normal((n, 3))
    R = np.stack([ref.rotation(axes[k], rng.uniform(0.0, degrees)) for k in range(n)])
    t = rng.standard_normal((n, 3))
    t *= (rng.uniform(0.0, metres, n) / np.linalg.norm(t, axis=1))[:, None]
    PB = np.einsum("nij,nkj->nki", R, PA.astype(np.float64)) + t[:, None, :]
    with np.errstate(all="ignore"):
        xb, yb = np.rint(fx * PB[..., 0] / PB[..., 2] + cx), np.rint(fy * PB[..., 1] / PB[..., 2] + cy)
    keep = ref.triad(PA[:, 0], PA[:, 1], PA[:, 2], 0.05)[3]
    keep &= np.all((PB[..., 2] > 0.3) & (xb >= 0) & (xb <= W - 1) & (yb >= 0) & (yb <= H - 1), axis=1)
    U = np.stack([(xb.astype(np.float32) - np.float32(cx)) / np.float32(fx), (yb.astype(np.float32) - np.float32(cy)) / np.float32(fy),
                  np.ones_like(xb, dtype=np.float32)], axis=-1)
    l, _, valid = pnp.ranges(PA[keep], U[keep])
    true = np.linalg.norm(PB[keep], axis=-1)
    with np.errstate(all="ignore"):
        reached = np.all(np.abs(l - true) <= 0.02 * true, axis=1)
    share = float(reached.mean())
    print(f"up to {degrees} degrees / {metres} m: {int(keep.sum())} triples kept, {share:.3f} within 2 % of the true ranges, "
          f"{float(valid.mean()):.3f} converged to 1e-9")
    assert keep.sum() >= 1000
    assert share >= 0.9


def _planted(name):
    """The planted-motion case of tests/test_features_host.py with unrounded bearings: (P_a, U, UV, K, T_true)"""
    rng = np.random.default_rng(3)
    T_true = ref.MOTIONS[name]
    K = tuple(float(np.float32(k)) for k in odo.intrinsics(64, 48))
    n = 40
    kp_a = np.stack([rng.integers(0, 64, n), rng.integers(0, 48, n), np.full(n, 30), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    depth_a = rng.uniform(1.0, 3.0, (48, 64)).astype(np.float32)
    matches = np.stack([np.arange(n), np.zeros(n, np.int64)], axis=1).astype(np.int32)
    P_a, _, _, _ = pnp.pair_list(kp_a, depth_a, kp_a, matches, K, K)
    assert len(P_a) == n
    PB = P_a.astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3]
    U = (PB / PB[:, 2:3]).astype(np.float32)                             # the exact bearings, no pixel rounding
    UV = np.stack([K[0] * PB[:, 0] / PB[:, 2] + K[2], K[1] * PB[:, 1] / PB[:, 2] + K[3]], axis=1)
    return P_a, U, UV, K, T_true


def test_exact_correspondences_of_a_small_motion_give_the_planted_motion():
    """Three exact correspondences have up to four poses (the roots of the three-point problem); Newton from A's ranges finds the one
    next to its start. At the identity the start IS the root, and for a motion small against the distance between the roots it lies in
    that root's basin: with the 2 degrees and 5 cm of MOTIONS["small"] every hypothesis that is not void is the planted motion, at the
    bar of the 3D-3D test (2e-4 on R), and the reprojection refinement reaches it to 1e-6."""
    P_a, U, UV, K, T_true = _planted("small")
    R, t, valid = pnp.hypotheses(P_a, U, 0, 64, 0.05)
    assert valid.sum() > 32
    err = max(np.abs(R[h] - T_true[:3, :3]).max() for h in np.nonzero(valid)[0])
    assert err < 2e-4
    first = np.nonzero(valid)[0][0]
    R2, t2 = pnp.refine(R[first], t[first], P_a, UV, K, 3)
    assert np.abs(R2 - T_true[:3, :3]).max() < 1e-6 and np.abs(t2 - T_true[:3, 3]).max() < 1e-6


@pytest.mark.parametrize("name", ["wide", "roll", "wider"])
def test_exact_correspondences_of_a_wide_motion_give_a_root_and_mostly_the_planted_one(name):
    """At 16 to 30 degrees a few triples lead Newton to ANOTHER root of the three-point problem: a pose that maps the three points onto
    their bearings exactly and is not the planted one (measured: 2 of 59 hypotheses for wide, 0 of 60 for roll, 2 of 59 for wider). So
    here every hypothesis that is not void must be a root (its three points land on their bearings within 1e-5 radians), at least 0.9
    of them -- the floor of the reach test -- must be the planted motion at the 3D-3D bar, and so must the consensus: the winner of the
    whole call, refined, to 1e-6. A complete P3P solver would return all four roots per triple; that is not part of the stage."""
    P_a, U, UV, K, T_true = _planted(name)
    R, t, valid = pnp.hypotheses(P_a, U, 0, 64, 0.05)
    hit = np.nonzero(valid)[0]
    assert len(hit) > 32
    idx = pnp.draw(0, 64, len(P_a))
    for h in hit:
        Q = P_a[idx[h]].astype(np.float64) @ R[h].astype(np.float64).T + t[h]
        f = U[idx[h]].astype(np.float64)
        cosine = np.sum(Q * f, axis=1) / (np.linalg.norm(Q, axis=1) * np.linalg.norm(f, axis=1))
        assert np.all(np.arccos(np.minimum(cosine, 1.0)) <= 1e-5)
    errs = np.array([np.abs(R[h] - T_true[:3, :3]).max() for h in hit])
    print(f"{name}: {len(hit)} hypotheses, {int((errs >= 2e-4).sum())} on another root")
    assert (errs < 2e-4).mean() >= 0.9
    counts = np.where(valid, pnp.inliers(R, t, P_a, UV.astype(np.float32), K, 2.0).sum(axis=-1), 0)
    winner = int(np.argmax(counts))
    assert counts[winner] == len(P_a) and errs[list(hit).index(winner)] < 2e-4
    R2, t2 = pnp.refine(R[winner], t[winner], P_a, UV, K, 3)
    assert np.abs(R2 - T_true[:3, :3]).max() < 1e-6 and np.abs(t2 - T_true[:3, 3]).max() < 1e-6


def test_void_rules_of_the_ranges():
    P = np.array([[[0.0, 0.0, 2.0], [0.5, 0.0, 2.0], [0.0, 0.5, 2.5]]], np.float32)
    U = (P / P[..., 2:3]).astype(np.float32)
    l, f, valid = pnp.ranges(P, U)                                       # the identity: the start is the root
    assert valid[0] and np.allclose(l[0], np.linalg.norm(P[0], axis=1), rtol=1e-7)
    assert np.abs((l[..., None] * f)[0] - P[0]).max() < 1e-6
    same = np.repeat(U[:, :1], 3, axis=1)                                # three equal bearings cannot hold three distinct points
    assert not pnp.ranges(P, same)[2][0]
    assert not pnp.ranges(P, np.full_like(U, np.nan))[2][0]
    assert not pnp.ranges(np.zeros_like(P), U)[2][0]                     # ranges of zero: det = 0


# ---- the analytic scenes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["wide", "roll", "wider"])
def test_wide_baselines_are_accepted_without_the_depth_of_b(name, W, H):
    """Measured with this restatement (Feature seed): 33 to 65 pairs, all but one or two of them final inliers, 0.26
    to 2.40 degrees and 11.8 to 105.4 mm from the truth (the worst: roll at 161 x 97) -- coarser than the 3D-3D pose of the same pairs
    (0.04 to 0.21 degrees, 0.5 to 3.5 mm): integer pixels on a plane hold a PnP pose weakly. With B's depth replaced by NaN the result is
    the same bytes: the call has no such argument, and the restatement is given none."""
    kp_a, depth_a, kp_b, depth_b, matches, K, T_true = _case(name, W, H)
    out = pnp.pose(kp_a, depth_a, kp_b, matches, K, K, min_area=features.MIN_AREA)
    keypoints_a, keypoints_b, M, winner, best, final, accepted, zero = out["stats"].tolist()
    degrees, mm = odo.pose_error(out["T_refined"], T_true)
    print(f"{name} {W}x{H}: M {M}, winner {winner} with {best}, inliers {final}, {degrees:.3f} deg, {mm:.2f} mm")
    assert accepted == 1 and zero == 0
    assert final >= 0.8 * M
    assert degrees <= 3.0 and mm <= 150.0
    assert np.array_equal(out["T"], out["T_refined"].astype(np.float32))
    # the pair list is the 3D-3D one wherever B's depth is valid (it is everywhere on the plane); with holes in B it keeps what that loses
    holes = np.full_like(depth_b, np.nan)
    assert len(ref.pair_list(kp_a, depth_a, kp_b, holes, matches, K, K)[0]) == 0
    assert len(ref.pair_list(kp_a, depth_a, kp_b, depth_b, matches, K, K)[0]) == M


@pytest.mark.parametrize("W,H", SIZES)
def test_unrelated_textures_are_refused_with_the_identity(W, H):
    kp_a, depth_a, kp_b, _, matches, K, _ = _case("unrelated", W, H)
    out = pnp.pose(kp_a, depth_a, kp_b, matches, K, K, min_area=features.MIN_AREA)
    print(f"unrelated {W}x{H}: stats {out['stats'].tolist()}")
    assert out["stats"][6] == 0 and out["stats"][2] <= 9
    assert out["T"].tobytes() == np.eye(4, dtype=np.float32).tobytes()


# ---- options --------------------------------------------------------------------------------------------------------------------------------
def _training(**block):
    return {"relocalisation": {"enabled": True}, "feature_seed": {"enabled": True, **block}}


def test_the_solver_option():
    assert features.feature_seed_options(_training())["solver"] == "points"
    assert features.feature_seed_options(_training(solver="pnp"))["solver"] == "pnp"
    for bad in ("p3p", "", None, 1):
        with pytest.raises(ValueError, match=r"Training.feature_seed.solver must be one of \['points', 'pnp'\], got " + repr(bad).replace("'", "'")):
            features.feature_seed_options(_training(solver=bad))
    mono = features.feature_seed_options({**_training(solver="pnp"), "monocular": True})
    assert mono["solver"] == "pnp" and mono["enabled"]
    with pytest.raises(ValueError, match="Training.feature_seed cannot be used with monocular input: a frame has no depth to back-project its "
                                         r"keypoints with, and a pose from 2D-3D matches \(PnP\) is not part of this stage"):
        features.feature_seed_options({**_training(), "monocular": True})
    with pytest.raises(ValueError, match="Training.feature_seed cannot be used with monocular input"):
        features.feature_seed_options({**_training(solver="points"), "monocular": True})
    assert features.default_options(solver="pnp", cell=16)["solver"] == "pnp"
