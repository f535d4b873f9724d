"""Host-side checks of loop closure (slam/loop_closure.py, slam/stages.py LoopClosure, include/loop_closure.h): the ``Training.loop_closure``
options and their refusals, the float64 restatement (tests/pose_graph_reference.py) -- Log against Exp near 0, near pi and below the series
threshold, the header's Jacobian blocks against central differences, the recovery of a zero-residual ring -- and the rule that gives a frame
the correction of a keyframe. No GPU."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_graph_reference as ref  # noqa: E402
from slam import loop_closure as lc  # noqa: E402
from slam import stages  # noqa: E402


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def test_defaults_pass_and_off_means_none():
    opts = stages.loop_closure_options
    assert opts({}) is None and opts({"loop_closure": {}}) is None and opts({"loop_closure": {"enabled": False, "topk": 99}}) is None
    got = opts({"loop_closure": {"enabled": True}})
    assert got["enabled"] is True and set(got) == set(stages.LOOP_CLOSURE_DEFAULTS)
    assert (got["ferns"], got["grid"], got["seed"]) == (512, [40, 30], 0)                     # the relocalisation stage's fern defaults
    assert got["iters"] == [5, 7, 10, 10] and got["consistency"] == [0.02, 1.0] and got["min_gap"] == 10
    assert opts({"loop_closure": {"enabled": True, "levels": 2}})["iters"] == [5, 7]
    shared = opts({"relocalisation": {"enabled": True, "ferns": 256}, "loop_closure": {"enabled": True}})
    assert shared["ferns"] == 256                                                             # as Training.relocalisation
    assert opts({"relocalisation": {"enabled": True, "ferns": 256}, "loop_closure": {"enabled": True, "ferns": 256}})["ferns"] == 256
    assert opts({"loop_closure": {"enabled": True, "ferns": 64, "grid": [8, 6]}})["grid"] == [8, 6]


def test_runs_loop_closure_cannot_serve_are_refused_with_the_reason():
    opts, on = stages.loop_closure_options, {"loop_closure": {"enabled": True}}
    with pytest.raises(ValueError, match="monocular input: the drift of an RGB-only run includes scale.*Sim\\(3\\)"):
        opts({**on, "monocular": True})
    with pytest.raises(ValueError, match="dynamic_model: the deformation field lives in world coordinates"):
        opts(on, dynamic_model=True)
    with pytest.raises(ValueError, match="spherical_harmonics: the coefficients of degree 1 and higher"):
        opts({**on, "spherical_harmonics": True})
    with pytest.raises(ValueError, match="sharded back-end of 2 ranks"):
        opts(on, ranks=2)
    assert opts({"monocular": True, "spherical_harmonics": True}, dynamic_model=True, ranks=8) is None      # off: nothing to refuse


def test_unknown_keys_and_ranges_are_refused():
    opts = stages.loop_closure_options
    for block, text in (({"windows": 3}, "unknown keys \\['windows'\\]"),
                        ({"min_gap": 0}, "loop_closure.min_gap must be at least 1"),
                        ({"min_gap": 2.5}, "loop_closure.min_gap must be an integer"),
                        ({"topk": 0}, "loop_closure.topk must be 1 to 16"),
                        ({"topk": 17}, "loop_closure.topk must be 1 to 16"),
                        ({"max_code_distance": 1.5}, "loop_closure.max_code_distance"),
                        ({"max_code_distance": math.nan}, "loop_closure.max_code_distance must be a number"),
                        ({"consistency": 0.02}, "loop_closure.consistency must be \\[metres, degrees\\]"),
                        ({"consistency": [0.02, -1.0]}, "loop_closure.consistency"),
                        ({"min_correction": [0.1]}, "loop_closure.min_correction must be \\[metres, degrees\\]"),
                        ({"odometry_weights": [1.0, 0.0]}, "loop_closure.odometry_weights must be positive"),
                        ({"loop_weights": [math.inf, 1.0]}, "loop_closure.loop_weights"),
                        ({"outer_iters": 1001}, "loop_closure.outer_iters"),
                        ({"cg_iters": 0}, "loop_closure.cg_iters"),
                        ({"lambda": -1e-6}, "loop_closure.lambda"),
                        ({"step_tolerance": math.inf}, "loop_closure.step_tolerance"),
                        ({"geometric_weight": 0.0}, "loop_closure.geometric_weight must be positive"),
                        ({"levels": 7}, "loop_closure.levels"),
                        ({"iters": [5, 7, 10]}, "loop_closure.iters must hold 4 pass counts"),
                        ({"max_rotation": 181.0}, "loop_closure.max_rotation"),
                        ({"max_translation": -1.0}, "loop_closure.max_translation"),
                        ({"ferns": 12}, "relocalisation.ferns must be a multiple of 8")):
        with pytest.raises(ValueError, match=text):
            opts({"loop_closure": dict({"enabled": True}, **block)})
    with pytest.raises(ValueError, match="loop_closure.ferns = 128 differs from Training.relocalisation.ferns = 256"):
        opts({"relocalisation": {"enabled": True, "ferns": 256}, "loop_closure": {"enabled": True, "ferns": 128}})


def test_the_front_end_builds_the_stage_from_the_block():
    from slam.frontend import FrontEnd
    from slam.system import default_config, merge_config
    assert FrontEnd(default_config()).loop_closure is None
    on = FrontEnd(merge_config(default_config(), {"Training": {"loop_closure": {"enabled": True, "min_gap": 4}}}))
    assert on.loop_closure.options["min_gap"] == 4 and on.loop_closure.closer is None         # built with the map, on the device
    assert on.loop_closure.summary() == {"keyframes_queried": 0, "candidates_verified": 0, "edges_accepted": 0, "solves": 0,
                                         "corrections_applied": 0, "max_correction_m": 0.0, "max_correction_deg": 0.0,
                                         "device_ms_per_verify": 0.0, "device_ms_per_solve": 0.0}
    with pytest.raises(ValueError, match="loop_closure cannot be used with model_params.dynamic_model"):
        FrontEnd(merge_config(default_config(), {"Training": {"loop_closure": {"enabled": True}}, "model_params": {"dynamic_model": True}}))
    with pytest.raises(ValueError, match="sharded back-end of 2 ranks"):
        on.loop_closure.restart(0, None, {}, lambda: None, None, ranks=2)


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@pytest.mark.parametrize("angle,bar", [(0.0, 1e-15), (1e-9, 1e-15), (9.9e-6, 1e-15), (1.01e-5, 1e-11), (1e-3, 1e-11), (0.5, 1e-14), (3.0, 1e-14),
                                       (math.pi - 1e-3, 1e-13), (math.pi - 1e-7, 1e-9), (math.pi - 1e-12, 1e-9)])
def test_log_inverts_exp(angle, bar):
    """The bars: rounding of O(1) numbers through a few dozen operations (1e-15 .. 1e-14); just above the series threshold 1 - cos a loses
    half the digits (1e-11); within 1e-7 of pi the axis comes from the square root of a difference of O(1) numbers (1e-9)."""
    rng = np.random.default_rng(3)
    tau = np.concatenate([rng.normal(size=(16, 3)), angle * _unit(rng, 16)], axis=1)
    back = ref.Log(ref.Exp(tau))
    assert np.abs(ref.Exp(back) - ref.Exp(tau)).max() <= max(bar, 1e-15) * 10                  # the same motion, whatever the branch
    if angle < math.pi - 1e-9:                                                                 # (at pi itself theta and -theta are one rotation)
        assert np.abs(back - tau).max() <= bar * (1.0 + np.abs(tau).max())


def test_exp_is_the_projects_se3_exp():
    import torch
    from slam.camera import SE3_exp
    rng = np.random.default_rng(4)
    for scale in (1e-7, 1e-3, 1.0):
        tau = rng.normal(size=6) * np.array([1, 1, 1, scale, scale, scale])
        assert np.abs(ref.Exp(tau) - SE3_exp(torch.tensor(tau, dtype=torch.float64)).numpy()).max() <= 1e-14


def test_jacobian_blocks_are_the_derivatives_of_the_residual():
    """A_i and A_j of the header against central differences (step 1e-6: truncation 1e-12, rounding 1e-10) at residuals of a few degrees
    and centimetres, where the cut of the series after ad^4 is below 1e-9."""
    N = 6
    X = ref.bend(ref.ring(N), [0.01, -0.02, 0.005, 0.01, 0.02, -0.01])
    en, Z = ref.ring_edges(ref.ring(N), loops=2)
    Ai, Aj = ref.jacobian_blocks(X, en, Z)
    h, worst = 1e-6, 0.0
    for e, (i, j) in enumerate(en):
        for node, A in ((i, Ai), (j, Aj)):
            for c in range(6):
                d = np.zeros((N, 6))
                d[node, c] = h
                plus, minus = ref.residuals(ref.apply_delta(X, d), en[e:e + 1], Z[e:e + 1]), ref.residuals(ref.apply_delta(X, -d), en[e:e + 1], Z[e:e + 1])
                worst = max(worst, float(np.abs((plus - minus)[0] / (2 * h) - A[e][:, c]).max()))
    assert worst <= 1e-7, worst


@pytest.mark.parametrize("N", [3, 12])
def test_the_restatement_recovers_a_zero_residual_ring(N):
    gt = ref.ring(N)
    en, Z = ref.ring_edges(gt, loops=4)
    w = np.tile([1.0, 1.0], (len(en), 1))
    fixed = np.zeros(N, np.int32)
    fixed[0] = 1
    start = ref.bend(gt, [0.003, -0.003, 0.0027, 0.002, -0.002, 0.0021])
    assert ref.cost(gt, en, Z, w) <= 1e-26 and ref.cost(start, en, Z, w) >= 1e-6
    X, cost = ref.solve(start, fixed, en, Z, w)
    r = ref.Log(ref.to44(X) @ ref.inv44(ref.to44(gt)))
    assert np.abs(r).max() <= 1e-9 and cost <= 1e-18
    assert X[0].tobytes() == start[0].tobytes()


def test_broken_edges_of_the_restatement_follow_the_header():
    Z = ref.ring_edges(ref.ring(4))[1][:1]
    rows = [((0, 1), Z[0], (1, 1), True), ((0, 1), Z[0], (0, 0), True), ((-1, 1), Z[0], (1, 1), False), ((0, 4), Z[0], (1, 1), False),
            ((2, 2), Z[0], (1, 1), False), ((0, 1), np.where(np.arange(12) == 3, np.nan, Z[0]), (1, 1), False), ((0, 1), Z[0], (np.inf, 1), False),
            ((0, 1), Z[0], (1, -1e-9), False)]
    got = ref.usable_edges(4, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert got.tolist() == [r[3] for r in rows]


def test_map_correct_restatement_on_a_case_worked_by_hand():
    """A quarter turn about z and a shift: (1, 0, 0) -> (0, 1, 0) + t; the quaternion of the turn is (cos 45, 0, 0, sin 45)."""
    D = np.array([[0, -1, 0, 0.5, 1, 0, 0, -1.0, 0, 0, 1, 2.0], [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], np.float32)
    xyz = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], np.float32)
    q = np.array([[2, 0, 0, 0]] * 4, np.float32)
    x, qn, moved, _, _ = ref.map_correct(xyz, q, [0, 1, 2, -1], [0, -1, 1], D)
    assert moved.tolist() == [True, False, True, False]
    assert np.allclose(x[0], [0.5, 0.0, 2.0]) and np.array_equal(x[1], xyz[1]) and np.array_equal(x[2], xyz[2])
    assert np.allclose(qn[0], 2 * np.array([math.sqrt(0.5), 0, 0, math.sqrt(0.5)]), atol=1e-7) and np.array_equal(qn[2], q[2])
    assert ref.quat_of(np.diag([1.0, -1.0, -1.0])).tolist() == [0.0, 1.0, 0.0, 0.0]           # a half turn: the branch from x


# ---- which correction a frame takes -----------------------------------------------------------------------------------------------------
def test_a_frame_takes_the_correction_of_the_last_keyframe_at_or_before_it():
    ids = [0, 5, 9, 14]
    assert [lc.correction_node(f, ids) for f in (0, 1, 4, 5, 6, 8, 9, 13, 14, 15, 40)] == [0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 3]
    assert lc.correction_node(2, [3, 7]) is None and lc.correction_node(3, [3, 7]) == 0         # before the first keyframe: none
    assert lc.correction_node(0, []) is None
