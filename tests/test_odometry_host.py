"""Host side of the dense odometry (include/visual_odometry.h): what the numpy restatement (tests/odometry_reference.py) does on the planted
scene, the parsing of ``Training.pose_prior``, the pose composition, and that a FrontEnd without the option never meets slam.odometry.
No GPU."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import odometry_reference as ref  # noqa: E402

SIZES, CASES, fit = ref.PLANTED_SIZES, ref.PLANTED_CASES, ref.planted_fit


# ---- the restatement on the planted scene -------------------------------------------------------------------------------------------------
def test_the_planted_scene_is_what_it_says():
    image_prev, depth_prev, image_cur, K, T = ref.planted_scene(64, 48, s=1.0)
    assert K == (57.6, 57.6, 31.8, 23.3)
    angle, shift = np.rad2deg(ref.rotation_angle(T[:3, :3])), 1e3 * np.linalg.norm(T[:3, 3])
    assert abs(angle - 1.41) < 0.01 and abs(shift - 39.0) < 1.0                   # 1.41 degrees / 39 mm
    # a pixel of the previous frame, lifted by its depth and moved by T, lands on the plane point the current frame shows there
    v, u = 20, 30
    X = np.array([(u - K[2]) / K[0], (v - K[3]) / K[1], 1.0]) * depth_prev[v, u]
    assert abs(ref.PLANE @ X - ref.PLANE_D) < 1e-6
    assert abs(image_prev[0, v, u] - ref.texture(X[0], X[1])) < 1e-6
    Y = T[:3, :3] @ X + T[:3, 3]
    x, y = K[0] * Y[0] / Y[2] + K[2], K[1] * Y[1] / Y[2] + K[3]
    x0, y0 = int(x), int(y)
    near = image_cur[0, y0:y0 + 2, x0:x0 + 2]
    assert near.min() - 1e-6 <= ref.texture(X[0], X[1]) <= near.max() + 1e-6 or abs(near.mean() - ref.texture(X[0], X[1])) < 0.02


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("size", sorted(SIZES))
def test_reference_recovers_the_planted_motion_within_half_the_device_bars(size, case):
    T, stats, T_fit, T_true = fit(size, case)
    _, _, bar_deg, bar_mm = SIZES[size]
    deg, mm = ref.pose_error(T_fit, T_true)
    print(size, case, f"{deg:.4f} deg {mm:.3f} mm accepted {stats[0]:.0f} share {stats[1]:.3f} sigma {stats[2]:.4f}")
    assert deg <= 0.5 * bar_deg and mm <= 0.5 * bar_mm
    assert stats[0] == 1.0 and np.array_equal(T, T_fit)


def test_reference_reproduces_the_prototype_figures():
    for size, case, deg_is, mm_is in (((160, 120), "clean_1", 0.0010, 0.04), ((160, 120), "clean_2.5", 0.0021, 0.08), ((64, 48), "clean_1", 0.021, 0.83),
                                      ((64, 48), "clean_2.5", 0.018, 0.64), ((33, 21), "clean_1", 0.057, 1.95), ((33, 21), "clean_2.5", 0.134, 5.2)):
        deg, mm = ref.pose_error(fit(size, case)[2], fit(size, case)[3])
        assert abs(deg - deg_is) <= 0.1 * deg_is + 1e-4 and abs(mm - mm_is) <= 0.1 * mm_is + 5e-3, (size, case, deg, mm)


def test_student_t_weights_shrug_off_the_patch():
    clean, patched = (ref.pose_error(fit((160, 120), c)[2], fit((160, 120), c)[3]) for c in ("clean_1", "patch_1"))
    assert patched[0] <= 3 * clean[0] + 1e-3 and patched[1] <= 3 * clean[1] + 0.05


def test_pyramid_rules():
    rng = np.random.default_rng(0)
    image = rng.uniform(0, 1, (3, 21, 33)).astype(np.float32)
    depth = rng.uniform(0.5, 4.0, (21, 33)).astype(np.float32)
    depth[0, 0], depth[0, 1], depth[1, 0], depth[1, 1] = np.nan, np.inf, 9.0, 0.2          # a block with no usable depth
    depth[2, 2], depth[2, 3], depth[3, 2], depth[3, 3] = 3.0, 1.5, 2.0, -1.0               # the foreground wins
    mask = np.ones((21, 33), np.uint8)
    mask[3, 2] = 0
    pyr, valid0 = ref.pyramid(image, depth, mask, 0.4, 5.0, 2)
    (I0, D0), (I1, D1) = pyr
    assert I0.dtype == D0.dtype == I1.dtype == D1.dtype == np.float32 and I1.shape == (10, 16)      # the odd row and column are dropped
    assert D0[0, 0] == D0[0, 1] == D0[1, 0] == D0[1, 1] == 0 and D1[0, 0] == 0
    assert D0[3, 2] == 0 and D0[3, 3] == 0 and D1[1, 1] == np.float32(1.5)
    assert valid0 == int((D0 > 0).sum()) == 21 * 33 - 6
    assert I1[4, 5] == ((I0[8, 10] + I0[8, 11]) + (I0[9, 10] + I0[9, 11])) * np.float32(0.25)
    assert ref.level_intrinsics((57.6, 57.6, 31.8, 23.3), 1) == tuple(float(np.float32(v)) for v in (28.8, 28.8, 15.65, 11.4))
    assert len(ref.pyramid_bytes(pyr, valid0)) == 16 + 2 * (21 * 33 * 4 + 12) + 2 * 10 * 16 * 4


def test_one_pass_at_the_true_motion_has_a_small_gradient_and_margins_say_how_fair_a_count_is():
    image_prev, depth_prev, image_cur, K, T_true = ref.planted_scene(64, 48, s=1.0)
    prev, _ = ref.pyramid(image_prev, depth_prev, levels=1)
    cur, _ = ref.pyramid(image_cur, levels=1)
    at_truth, _, _, _ = ref.one_pass(prev[0][0], prev[0][1], cur[0][0], ref.level_intrinsics(K, 0), T_true, 0.1)
    at_identity, scale, margin_px, margin_z = ref.one_pass(prev[0][0], prev[0][1], cur[0][0], ref.level_intrinsics(K, 0), np.eye(4), 0.1)
    assert at_truth[28] < 0.05 * at_identity[28]                                  # sum w r^2
    assert np.linalg.norm(at_truth[21:27]) < 0.1 * np.linalg.norm(at_identity[21:27])
    assert np.all(scale[:27] >= np.abs(at_identity[:27])) and margin_z > 100
    assert margin_px < 1e-3                  # from identity the pixels of column 1 project onto x = 1 itself: such a count is not comparable
    assert ref.solve_step(np.zeros(30)) is None and ref.solve_step(at_identity) is not None


@pytest.mark.parametrize("case", ref.ONE_PASS_CASES)
def test_the_one_pass_cases_of_the_device_test_count_fairly(case):
    sums, _, margin_px, margin_z = ref.one_pass_reference(case)
    assert margin_px >= 1e-3 and margin_z >= 1e-3 and sums[29] >= 50


def test_gate_refuses_and_hands_out_identity():
    image_prev, depth_prev, image_cur, K, T_true = ref.planted_scene(33, 21, s=1.0)
    T, stats, _, T_fit = ref.align_scene(image_prev, depth_prev, image_cur, K, 2, [8, 10], max_translation=0.01)
    assert stats[0] == 0.0 and np.array_equal(T, np.eye(4)) and stats[5] > 0.01 and not np.array_equal(T_fit, np.eye(4))
    T, stats, trace, _ = ref.align_scene(image_prev, 0 * depth_prev, image_cur, K, 2, [8, 10])
    assert stats[0] == 0.0 and np.array_equal(T, np.eye(4)) and stats[4] == 0 and stats[7] == 0 and np.isinf(stats[3]) and trace.shape == (18, 32)
    T, stats, trace, _ = ref.align_scene(image_prev, depth_prev, image_cur, K, 2, [0, 0], T_init=T_true)
    assert stats[0] == 0.0 and np.array_equal(T, np.eye(4)) and trace.shape == (0, 32)
    bad = np.eye(4)
    bad[0, 3] = np.nan
    T, stats, _, _ = ref.align_scene(image_prev, depth_prev, image_cur, K, 2, [8, 10], T_init=bad)
    assert stats[0] == 0.0 and np.array_equal(T, np.eye(4))


# ---- Training.pose_prior ---------------------------------------------------------------------------------------------------------------------
def _config(pose_prior=None, monocular=False):
    training = {"monocular": monocular, "kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3, "window_size": 4,
                "rgb_boundary_threshold": 0.01}
    if pose_prior is not None:
        training["pose_prior"] = pose_prior
    return {"Training": training, "Results": {}, "model_params": {"dynamic_model": False}}


def test_pose_prior_block_parses_with_defaults_and_is_off_unless_enabled():
    from slam.frontend import FrontEnd
    from slam.stages import POSE_PRIOR_DEFAULTS, pose_prior_options
    assert pose_prior_options({}) is None and pose_prior_options({"pose_prior": {}}) is None
    assert pose_prior_options({"pose_prior": {"enabled": False, "levels": 99}}) is None
    assert FrontEnd(_config()).pose_prior is None
    got = pose_prior_options({"pose_prior": {"enabled": True}})
    assert got == dict(POSE_PRIOR_DEFAULTS, enabled=True)
    assert (got["levels"], got["iters"], got["nu"], got["sigma_init"], got["sigma_min"], got["min_share"], got["max_last_step"],
            got["constant_velocity"]) == (3, [5, 7, 10], 5.0, 0.1, 1e-3, 0.3, 1e-2, False)
    assert set(got) == {"enabled", "levels", "iters", "nu", "sigma_init", "sigma_min", "min_share", "max_last_step", "max_translation",
                        "max_rotation", "depth_min", "depth_max", "constant_velocity"}
    got = FrontEnd(_config({"enabled": True, "levels": 2, "iters": (8, 10), "nu": 4, "max_translation": 0.2, "max_rotation": 10,
                            "depth_min": 0.1, "depth_max": 8, "constant_velocity": 1})).pose_prior.options
    assert (got["levels"], got["iters"], got["nu"], got["max_translation"], got["max_rotation"], got["depth_min"], got["depth_max"],
            got["constant_velocity"]) == (2, [8, 10], 4.0, 0.2, 10.0, 0.1, 8.0, True)


@pytest.mark.parametrize("block, names", [
    ({"itres": [5, 7, 10]}, "unknown keys \\['itres'\\]"), ({"levels": 0}, "levels"), ({"levels": 7, "iters": [1] * 7}, "levels"),
    ({"levels": 2}, "iters"), ({"iters": [5, 7]}, "iters"), ({"iters": [5, 7, 65]}, "iters"), ({"iters": [5, -1, 3]}, "iters"), ({"iters": 5}, "iters"),
    ({"nu": 0}, "nu"), ({"sigma_init": -1}, "sigma_init"), ({"sigma_min": 0}, "sigma_min"), ({"sigma_init": float("inf")}, "sigma_init"),
    ({"min_share": 1.5}, "min_share"), ({"max_last_step": -1e-3}, "max_last_step"), ({"max_translation": -1}, "max_translation"),
    ({"max_rotation": 200}, "max_rotation"), ({"max_rotation": float("nan")}, "max_rotation"), ({"depth_min": -1}, "depth_min"),
    ({"depth_min": 3, "depth_max": 2}, "depth_min")])
def test_pose_prior_refusals_name_what_is_wrong(block, names):
    from slam.stages import pose_prior_options
    with pytest.raises(ValueError, match="Training.pose_prior.*" + names):
        pose_prior_options({"pose_prior": dict(block, enabled=True)})


def test_pose_composition_is_T_times_the_previous_world_to_camera():
    from slam.camera import compose_pose
    rng = np.random.default_rng(3)
    for _ in range(8):
        W2C_prev, W2C_cur = (ref.se3_exp(rng.uniform(-1, 1, 6)) for _ in range(2))
        T = W2C_cur @ np.linalg.inv(W2C_prev)                                   # previous camera -> current camera
        R, t = compose_pose(torch.tensor(T, dtype=torch.float32), torch.tensor(W2C_prev[:3, :3], dtype=torch.float32),
                            torch.tensor(W2C_prev[:3, 3], dtype=torch.float32))
        assert R.dtype == t.dtype == torch.float32
        assert np.abs(R.numpy() - W2C_cur[:3, :3]).max() < 1e-5 and np.abs(t.numpy() - W2C_cur[:3, 3]).max() < 1e-5
    R, t = compose_pose(torch.eye(4), torch.tensor(W2C_prev[:3, :3]), torch.tensor(W2C_prev[:3, 3]))      # a refused prior: the previous pose
    assert np.array_equal(R.numpy(), W2C_prev[:3, :3]) and np.array_equal(t.numpy(), W2C_prev[:3, 3])


def test_frontend_without_the_option_never_meets_the_odometry():
    """In a fresh interpreter: constructing and initialising the state of a FrontEnd without the block imports no slam.odometry; with the
    block the import still waits for the first frame that is kept."""
    code = ("import sys\n"
            f"sys.path[:0] = [{REPO!r}, {os.path.join(REPO, '4dgs-slam_amd')!r}]\n"
            "from slam.frontend import FrontEnd\n"
            "cfg = lambda t: {'Training': dict({'monocular': False}, **t), 'Results': {}, 'model_params': {'dynamic_model': False}}\n"
            "off = FrontEnd(cfg({}))\n"
            "assert off.pose_prior is None\n"
            "assert 'slam.odometry' not in sys.modules\n"
            "on = FrontEnd(cfg({'pose_prior': {'enabled': True}}))\n"
            "assert on.pose_prior.options['enabled'] and on.pose_prior.odometry is None and 'slam.odometry' not in sys.modules\n"
            "assert on.pose_prior.summary() == {'frames': 0, 'accepted_share': 0.0, 'inlier_share': 0.0, 'device_ms_per_frame': 0.0}\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stderr


class _Odometry:
    """Stands in for DenseOdometry: records its calls, aligns to a fixed motion."""

    def __init__(self, T):
        self.T, self.calls, self.has_previous = T, [], False

    def keep(self, image, depth=None, mask=None):
        self.calls.append(("keep", depth, mask))
        self.has_previous = depth is not None

    def drop(self):
        self.calls.append(("drop",))
        self.has_previous = False

    def align(self, image, T_init=None):
        self.calls.append(("align", T_init))
        return self.T, torch.zeros(8, dtype=torch.float64)


def _camera(R, t, depth, mask=None):
    cam = types.SimpleNamespace(R=R.clone(), T=t.clone(), original_image=torch.zeros(3, 2, 2), motion_mask=mask, depth=depth)
    cam.depth_device = lambda: cam.depth
    cam.update_RT = lambda R_, t_: (setattr(cam, "R", R_.clone()), setattr(cam, "T", t_.clone()))
    return cam


def test_the_prior_moves_the_start_and_keeps_the_right_depth():
    from slam.frontend import FrontEnd
    T = torch.tensor(ref.planted_motion(1.0), dtype=torch.float32)
    W2C = torch.tensor(ref.se3_exp([0.3, -0.2, 0.1, 0.2, 0.1, -0.3]), dtype=torch.float32)
    previous = _camera(W2C[:3, :3], W2C[:3, 3], torch.ones(2, 2))
    # RGB-D, constant velocity: the first alignment starts at identity, the second at the first one's result
    fe = FrontEnd(_config({"enabled": True, "constant_velocity": True}))
    fe.pose_prior.odometry = odo = _Odometry(T)
    fe.pose_prior.keep(previous)
    assert odo.calls == [("keep", previous.depth, None)] and odo.has_previous
    cam = _camera(previous.R, previous.T, 2 * torch.ones(2, 2))
    fe.pose_prior.start(cam, previous)
    want = T.double() @ W2C.double()
    assert odo.calls[-1] == ("align", None)
    assert (cam.R.double() - want[:3, :3]).abs().max() < 1e-6 and (cam.T.double() - want[:3, 3]).abs().max() < 1e-6
    fe.pose_prior.start(cam, previous)
    assert odo.calls[-1][0] == "align" and odo.calls[-1][1] is T
    # monocular: the rendered depth where the opacity is above one half; no rendering yet, nothing kept
    fe = FrontEnd(_config({"enabled": True}, monocular=True))
    fe.pose_prior.odometry = odo = _Odometry(T)
    fe.pose_prior.keep(cam)
    assert odo.calls == [("drop",)] and not odo.has_previous
    pkg = {"depth": torch.tensor([[[1.0, 2.0], [3.0, 4.0]]]), "opacity": torch.tensor([[[0.9, 0.5], [0.51, 0.0]]])}
    fe.pose_prior.keep(cam, pkg)
    assert torch.equal(odo.calls[-1][1], torch.tensor([[[1.0, 0.0], [3.0, 0.0]]])) and odo.calls[-1][2] is None
    # a dynamic model hands the motion mask on
    fe = FrontEnd(_config({"enabled": True}))
    fe.pose_prior.dynamic_model, fe.pose_prior.odometry = True, _Odometry(T)
    masked = _camera(previous.R, previous.T, torch.ones(2, 2), mask=torch.tensor([[True, False], [True, True]]))
    fe.pose_prior.keep(masked)
    assert fe.pose_prior.odometry.calls[-1][2] is masked.motion_mask
