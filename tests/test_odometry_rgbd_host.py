"""Host side of gsr_odometry_align_rgbd (include/visual_odometry.h): what the numpy restatement (tests/odometry_rgbd_reference.py) does on
the three-plane scene, that the inputs of the device's one-pass comparison keep every decision clear of its bound, the parsing of
``Training.pose_prior_terms``, that a disabled block changes nothing, and the keyframe bookkeeping of ``PosePrior`` on a fake odometry.
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

import odometry_reference as ref0  # noqa: E402
import odometry_rgbd_reference as ref  # noqa: E402

SIZE, LEVELS, ITERS = (160, 120), 3, [5, 7, 10]


# ---- the restatement on the three-plane scene ----------------------------------------------------------------------------------------------------
# The float64 prototype this contract was written from gave, at 160 x 120 with 3 levels and iters [5, 7, 10], s in {1, 2.5}:
#   current image x 1.25 + 0.06   photometric fit 17-18 deg / 590-620 mm off and accepted   affine: <= 0.003 deg / 0.08 mm, (alpha, beta) = (0.2485, 0.0607)
#   constant-colour image         photometric fit refused (H not positive definite)         depth term: 0.0002 deg / 0.006 mm
#   textured, no gain             photometric fit 0.0015 deg / 0.06 mm                      depth term added: 0.0001 deg / 0.007 mm
# The bars below are twice what this restatement measured (the larger of s = 1 and s = 2.5): 0.0024 deg / 0.076 mm, 0.0004 deg / 0.009 mm at
# 96 x 72 and 0.0010 deg / 0.013 mm at 64 x 48 for the flat scene, 0.0001 deg / 0.007 mm.
@pytest.mark.parametrize("s", [1.0, 2.5])
def test_affine_brightness_recovers_the_motion_under_a_gain_that_misleads_the_photometric_fit(s):
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(*SIZE, s=s, gain=1.25, offset=0.06)
    _, stats, T_fit, _ = ref.planted_fit(SIZE, f"gain_affine_{s}")
    deg, mm = ref0.pose_error(T_fit, T_true)
    T0, stats0, _, _ = ref0.align_scene(image_prev, depth_prev, image_cur, K, LEVELS, ITERS)
    deg0, mm0 = ref0.pose_error(T0, T_true)
    print(s, f"affine {deg:.4f} deg {mm:.3f} mm alpha {stats[8]:.4f} beta {stats[9]:.4f} | photometric {deg0:.2f} deg {mm0:.1f} mm accepted {stats0[0]:.0f}")
    assert stats[0] == 1.0 and deg <= 0.005 and mm <= 0.16
    assert abs(stats[8] - 0.2485) <= 2e-4 and abs(stats[9] - 0.0607) <= 2e-4
    assert stats0[0] == 1.0 and deg0 > 5.0 and mm0 > 200.0             # the dangerous one: wrong, and the gate's step test passes it


@pytest.mark.parametrize("s", [1.0, 2.5])
@pytest.mark.parametrize("size", sorted(ref.FLAT_SIZES))
def test_the_depth_term_aligns_what_has_no_texture(size, s):
    levels, iters = ref.FLAT_SIZES[size]
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(*size, s=s, flat=True)
    _, stats, T_fit, _ = ref.fit(size, levels, iters, True, 1.0, 0.0, False, 1.0, s)
    deg, mm = ref0.pose_error(T_fit, T_true)
    print(size, s, f"{deg:.4f} deg {mm:.3f} mm")
    assert stats[0] == 1.0 and deg <= 0.002 and mm <= 0.026
    T0, stats0, _, _ = ref0.align_scene(image_prev, depth_prev, image_cur, K, levels, iters)
    assert stats0[0] == 0.0 and np.array_equal(T0, np.eye(4)) and np.isinf(stats0[3])


@pytest.mark.parametrize("s", [1.0, 2.5])
def test_the_depth_term_adds_to_a_textured_fit(s):
    _, stats, T_fit, T_true = ref.planted_fit(SIZE, f"textured_depth_{s}")
    deg, mm = ref0.pose_error(T_fit, T_true)
    assert stats[0] == 1.0 and deg <= 0.0003 and mm <= 0.014 and stats[11] > 0.9 * stats[4]


@pytest.mark.parametrize("case", sorted(ref.FIT_CASES))
@pytest.mark.parametrize("size", sorted(ref0.PLANTED_SIZES))
def test_the_restatement_meets_the_device_bars(size, case):
    _, stats, T_fit, T_true = ref.planted_fit(size, case)
    _, _, bar_deg, bar_mm = ref0.PLANTED_SIZES[size]
    deg, mm = ref0.pose_error(T_fit, T_true)
    assert stats[0] == 1.0 and deg <= bar_deg and mm <= bar_mm


def test_a_constant_image_with_the_affine_term_takes_no_step():
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(64, 48, flat=True)
    for weight in (0.0, 1.0):
        T, stats, trace, T_fit = ref.align_scene(image_prev, depth_prev, image_cur, depth_cur, K, 2, [8, 10], affine=True, weight=weight)
        assert stats[0] == 0.0 and np.isinf(stats[3]) and np.array_equal(T_fit, np.eye(4)) and stats[8] == 0.0 and stats[9] == 0.0


def test_the_scene_is_what_it_says():
    image_prev, depth_prev, image_cur, depth_cur, K, T = ref.scene(64, 48, s=1.0)
    v, u = 20, 30
    X = np.array([(u - K[2]) / K[0], (v - K[3]) / K[1], 1.0]) * depth_prev[v, u]
    on_plane = np.abs(ref.PLANES[:, :3] @ X - ref.PLANES[:, 3])
    assert on_plane.min() < 1e-5                                              # the pixel's point lies on one of the planes
    assert abs(image_prev[0, v, u] - ref0.texture(X[0] + 0.7 * X[2], X[1] - 0.4 * X[2])) < 1e-6
    assert len({int(np.argmin(np.abs(ref.PLANES[:, :3] @ (np.array([(uu - K[2]) / K[0], (vv - K[3]) / K[1], 1.0]) * depth_prev[vv, uu])
                                     - ref.PLANES[:, 3]))) for vv in range(0, 48, 4) for uu in range(0, 64, 4)}) == 3     # all three are seen
    flat = ref.scene(64, 48, flat=True)
    assert np.all(flat[0] == np.float32(ref.FLAT_COLOUR)) and np.all(flat[2] == np.float32(ref.FLAT_COLOUR)) and np.array_equal(flat[1], depth_prev)
    gained = ref.scene(64, 48, gain=1.25, offset=0.06)[2]
    assert np.abs(gained - (1.25 * image_cur + 0.06)).max() < 1e-6                  # (not clipped: the brightest pixels pass 1)


@pytest.mark.parametrize("case", ref.ONE_PASS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_one_pass_cases_of_the_device_test_count_fairly(case):
    sums, scale, margins = ref.one_pass_reference(case)
    for name, least in ref.MIN_MARGIN.items():
        assert margins[name] >= least, (name, margins[name])
    # the same pass with every per-pixel term in float32 takes the same decisions and stays inside the device test's bar
    low, _, _ = ref.one_pass_reference(case, np.float32)
    used = scale > 0
    n, NH, NS = ref.sizes(8 if ref.ONE_PASS_VARIANTS[case[5]][0] else 6)
    assert low[NH + n + 2] == sums[NH + n + 2] and low[NH + n + 5] == sums[NH + n + 5]
    assert np.all(np.abs(low[used] - sums[used]) <= 1e-6 * scale[used]) and np.all(scale >= np.abs(sums) * (1 - 1e-12))


def test_the_edge_test_and_the_holes_take_depth_terms_out():
    counts = {}
    for variant in ref.ONE_PASS_VARIANTS:
        sums, _, _ = ref.one_pass_reference((64, 48, 3, 1, False, variant))
        n, NH, NS = ref.sizes(8 if ref.ONE_PASS_VARIANTS[variant][0] else 6)
        counts[variant] = (sums[NH + n + 2], sums[NH + n + 5])
    assert counts["affine"][1] == 0 and 0 < counts["both"][1] < counts["both"][0] and counts["both_holes"][1] < counts["both"][1]
    assert counts["depth"] == counts["both"]


# ---- Training.pose_prior_terms ------------------------------------------------------------------------------------------------------------------------
def _config(terms=None, pose_prior={"enabled": True}, monocular=False):
    training = {"monocular": monocular, "kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3, "window_size": 4,
                "rgb_boundary_threshold": 0.01}
    if pose_prior is not None:
        training["pose_prior"] = pose_prior
    if terms is not None:
        training["pose_prior_terms"] = terms
    return {"Training": training, "Results": {}, "model_params": {"dynamic_model": False}}


def test_terms_block_parses_with_defaults_and_is_off_unless_enabled():
    from slam.frontend import FrontEnd
    from slam.stages import POSE_PRIOR_TERMS_DEFAULTS, pose_prior_terms_options
    on = {"pose_prior": {"enabled": True}}
    assert pose_prior_terms_options({}) is None and pose_prior_terms_options(dict(on, pose_prior_terms={})) is None
    assert pose_prior_terms_options({"pose_prior_terms": {"enabled": False, "against": "nothing"}}) is None        # off: not even looked at
    got = pose_prior_terms_options(dict(on, pose_prior_terms={"enabled": True}))
    assert got == dict(POSE_PRIOR_TERMS_DEFAULTS, enabled=True)
    assert got == {"enabled": True, "affine": True, "geometric_weight": 1.0, "edge_ratio": 0.05, "sigma_depth_init": 0.02, "sigma_depth_min": 1e-4,
                   "max_gain": 0.5, "max_offset": 0.3, "against": "previous"}
    got = FrontEnd(_config({"enabled": True, "affine": 0, "geometric_weight": 2, "against": "keyframe", "max_gain": 1})).pose_prior.terms
    assert (got["affine"], got["geometric_weight"], got["against"], got["max_gain"]) == (False, 2.0, "keyframe", 1.0)
    assert isinstance(got["geometric_weight"], float) and isinstance(got["max_gain"], float)


@pytest.mark.parametrize("block, names", [
    ({"afine": True}, "unknown keys \\['afine'\\]"), ({"geometric_weight": -1}, "geometric_weight"), ({"geometric_weight": float("inf")}, "geometric_weight"),
    ({"edge_ratio": -0.1}, "edge_ratio"), ({"edge_ratio": float("nan")}, "edge_ratio"), ({"sigma_depth_init": 0}, "sigma_depth_init"),
    ({"sigma_depth_min": -1}, "sigma_depth_min"), ({"sigma_depth_min": float("inf")}, "sigma_depth_min"), ({"max_gain": -0.5}, "max_gain"),
    ({"max_offset": -1}, "max_offset"), ({"max_offset": float("nan")}, "max_offset"), ({"against": "map"}, "against"),
    ({"affine": False, "geometric_weight": 0}, "would change nothing")])
def test_terms_refusals_name_what_is_wrong(block, names):
    from slam.stages import pose_prior_terms_options
    with pytest.raises(ValueError, match="Training.pose_prior_terms.*" + names):
        pose_prior_terms_options({"pose_prior": {"enabled": True}, "pose_prior_terms": dict(block, enabled=True)})


@pytest.mark.parametrize("pose_prior", [None, {}, {"enabled": False}])
def test_terms_without_the_prior_are_refused(pose_prior):
    from slam.frontend import FrontEnd
    with pytest.raises(ValueError, match="Training.pose_prior_terms is enabled but Training.pose_prior is not"):
        FrontEnd(_config({"enabled": True}, pose_prior=pose_prior))


def test_the_block_of_a_yaml_config_reaches_the_front_end(tmp_path):
    from slam.config import load_config
    from slam.frontend import FrontEnd
    path = tmp_path / "config.yaml"
    path.write_text("Training:\n  monocular: false\n  pose_prior: {enabled: true}\n"
                    "  pose_prior_terms: {enabled: true, affine: true, geometric_weight: 1.0, edge_ratio: 0.05, sigma_depth_init: 0.02,\n"
                    "                     sigma_depth_min: 0.0001, max_gain: 0.5, max_offset: 0.3, against: keyframe}\n"
                    "Results: {}\nmodel_params: {dynamic_model: false}\n")
    from slam.stages import POSE_PRIOR_TERMS_DEFAULTS
    prior = FrontEnd(load_config(str(path))).pose_prior
    assert prior.terms == dict(POSE_PRIOR_TERMS_DEFAULTS, enabled=True, against="keyframe") and prior.against_keyframe


def test_a_disabled_block_changes_nothing():
    """In a fresh interpreter: with the block absent or off PosePrior has no terms, imports no slam.odometry, and its idle summary and its
    options are the ones without the block; with the block on the import still waits for the first frame that is kept."""
    code = ("import sys\n"
            f"sys.path[:0] = [{REPO!r}, {os.path.join(REPO, '4dgs-slam_amd')!r}]\n"
            "from slam.frontend import FrontEnd\n"
            "cfg = lambda t: {'Training': dict({'monocular': False}, **t), 'Results': {}, 'model_params': {'dynamic_model': False}}\n"
            "plain = FrontEnd(cfg({'pose_prior': {'enabled': True}}))\n"
            "for block in ({}, {'enabled': False}, {'enabled': False, 'against': 'keyframe', 'bogus': 1}):\n"
            "    off = FrontEnd(cfg({'pose_prior': {'enabled': True}, 'pose_prior_terms': block}))\n"
            "    assert off.pose_prior.terms is None and not off.pose_prior.against_keyframe and off.pose_prior.options == plain.pose_prior.options\n"
            "    assert off.pose_prior.summary() == {'frames': 0, 'accepted_share': 0.0, 'inlier_share': 0.0, 'device_ms_per_frame': 0.0}\n"
            "assert FrontEnd(cfg({'pose_prior_terms': {'enabled': False}})).pose_prior is None\n"
            "on = FrontEnd(cfg({'pose_prior': {'enabled': True}, 'pose_prior_terms': {'enabled': True, 'against': 'keyframe'}}))\n"
            "assert on.pose_prior.terms['against'] == 'keyframe' and on.pose_prior.odometry is None and 'slam.odometry' not in sys.modules\n"
            "assert on.pose_prior.summary() == {'frames': 0, 'accepted_share': 0.0, 'inlier_share': 0.0, 'device_ms_per_frame': 0.0,\n"
            "                                   'mean_abs_alpha': 0.0, 'mean_abs_beta': 0.0, 'depth_term_share': 0.0, 'against': 'keyframe'}\n"
            "print('ok')\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert done.returncode == 0 and done.stdout.strip().endswith("ok"), done.stderr


# ---- PosePrior on a fake odometry ---------------------------------------------------------------------------------------------------------------------------
class _Odometry:
    """Stands in for DenseOdometry: records its calls; align() hands out the next of `answers`, (T, accepted)."""

    def __init__(self, answers):
        self.answers, self.calls, self.has_previous = list(answers), [], False

    def keep(self, image, depth=None, mask=None):
        self.calls.append(("keep", image, depth, mask))
        self.has_previous = depth is not None

    def drop(self):
        self.calls.append(("drop",))
        self.has_previous = False

    def align(self, image, T_init=None, trace=None, depth=None, mask=None):
        self.calls.append(("align", T_init, depth, mask))
        T, accepted = self.answers.pop(0)
        stats = torch.zeros(12, dtype=torch.float64)
        stats[0] = float(accepted)
        return (T if accepted else torch.eye(4)), stats


def _camera(W2C, depth, tag):
    cam = types.SimpleNamespace(R=W2C[:3, :3].clone(), T=W2C[:3, 3].clone(), original_image=torch.full((3, 2, 2), float(tag)), motion_mask=None, depth=depth)
    cam.depth_device = lambda: cam.depth
    cam.update_RT = lambda R_, t_: (setattr(cam, "R", R_.clone()), setattr(cam, "T", t_.clone()))
    return cam


def _pose(xi):
    return torch.tensor(ref0.se3_exp(xi), dtype=torch.float32)


def _w2c(cam):
    M = torch.eye(4)
    M[:3, :3], M[:3, 3] = cam.R, cam.T
    return M


def test_against_keyframes_the_kept_frame_changes_with_keyframes_alone():
    from slam.frontend import FrontEnd
    fe = FrontEnd(_config({"enabled": True, "against": "keyframe"}))
    prior = fe.pose_prior
    T1, T2, T3 = _pose([0.01, 0, 0, 0, 0.01, 0]), _pose([0.02, 0, 0, 0, 0.02, 0]), _pose([0.005, 0, 0, 0, 0, 0.01])
    prior.odometry = odo = _Odometry([(T1, True), (T2, False), (T2, True), (T3, True)])
    first = _camera(_pose([0.3, -0.2, 0.1, 0.2, 0.1, -0.3]), torch.ones(2, 2), 0)
    prior.restart(first)                                                  # the map starts: its first frame is kept
    assert [c[0] for c in odo.calls] == ["keep"] and prior.anchor is first and prior.motion is None
    # frame 1: aligned from identity against the kept frame, accepted: T1 times the keyframe's pose
    a = _camera(_w2c(first), 2 * torch.ones(2, 2), 1)
    prior.start(a, first)
    assert odo.calls[-1][0] == "align" and odo.calls[-1][1] is None and odo.calls[-1][2] is a.depth
    assert torch.allclose(_w2c(a), T1 @ _w2c(first), atol=1e-6) and torch.equal(prior.motion, T1)
    prior.keep(a)                                                         # a tracked frame that is no keyframe: the kept frame stays
    assert [c[0] for c in odo.calls] == ["keep", "align"] and prior.anchor is first
    # the back-end moves the keyframe: the next start is composed with its pose as it is then
    first.update_RT(*(_pose([0.31, -0.2, 0.1, 0.2, 0.1, -0.3])[:3, :3], _pose([0.31, -0.2, 0.1, 0.2, 0.1, -0.3])[:3, 3]))
    # frame 2: starts at the last accepted motion against the keyframe; refused: the previous frame's pose, and the motion stays
    b = _camera(_w2c(a), 2 * torch.ones(2, 2), 2)
    prior.start(b, a)
    assert odo.calls[-1][1] is not None and torch.equal(odo.calls[-1][1], T1)
    assert torch.equal(_w2c(b), _w2c(a)) and torch.equal(prior.motion, T1)
    prior.drop()                                                          # a lost frame: the keyframe has a pose of its own and stays
    assert odo.has_previous and prior.anchor is first
    # frame 3: again from T1; accepted
    c = _camera(_w2c(b), 2 * torch.ones(2, 2), 3)
    prior.start(c, b)
    assert torch.equal(odo.calls[-1][1], T1) and torch.allclose(_w2c(c), T2 @ _w2c(first), atol=1e-6) and torch.equal(prior.motion, T2)
    # the front-end makes frame 3 a keyframe: it replaces the kept frame and the next alignment starts at identity
    prior.keyframe(c)
    assert odo.calls[-1][0] == "keep" and odo.calls[-1][1] is c.original_image and prior.anchor is c and prior.motion is None
    d = _camera(_w2c(c), 2 * torch.ones(2, 2), 4)
    prior.start(d, c)
    assert odo.calls[-1][1] is None and torch.allclose(_w2c(d), T3 @ _w2c(c), atol=1e-6)
    assert [c_[0] for c_ in odo.calls] == ["keep", "align", "align", "align", "keep", "align"]
    prior.restart(d)                                                      # the map starts over
    assert odo.calls[-1][0] == "keep" and prior.anchor is d and prior.motion is None


def test_against_the_previous_frame_every_tracked_frame_is_kept_and_depth_is_handed_on():
    from slam.frontend import FrontEnd
    T1 = _pose([0.01, 0, 0, 0, 0.01, 0])
    fe = FrontEnd(_config({"enabled": True}))
    prior = fe.pose_prior
    prior.odometry = odo = _Odometry([(T1, True), (T1, False)])
    first = _camera(_pose([0.3, -0.2, 0.1, 0.2, 0.1, -0.3]), torch.ones(2, 2), 0)
    prior.restart(first)
    a = _camera(_w2c(first), 2 * torch.ones(2, 2), 1)
    prior.start(a, first)
    assert odo.calls[-1] == ("align", None, a.depth, None) and torch.allclose(_w2c(a), T1 @ _w2c(first), atol=1e-6)
    prior.keep(a)
    prior.keyframe(a)                                                     # against the previous frame a keyframe is nothing special
    assert [c[0] for c in odo.calls] == ["keep", "align", "keep"] and prior.anchor is None
    b = _camera(_w2c(a), 2 * torch.ones(2, 2), 2)
    prior.start(b, a)                                                     # refused: identity, the previous pose
    assert torch.equal(_w2c(b), _w2c(a))
    prior.drop()
    assert not odo.has_previous
    assert prior.summary.__self__ is prior and prior.terms["against"] == "previous"
    # monocular: no depth when the frame is aligned, and the summary says so
    fe = FrontEnd(_config({"enabled": True}, monocular=True))
    prior = fe.pose_prior
    prior.odometry = odo = _Odometry([(T1, True)])
    pkg = {"depth": torch.ones(1, 2, 2), "opacity": torch.ones(1, 2, 2)}
    prior.keep(first, pkg)
    prior.start(a, first)
    assert odo.calls[-1][0] == "align" and odo.calls[-1][2] is None and odo.calls[-1][3] is None
    odo.summary = lambda: {"frames": 1}
    assert prior.summary() == {"frames": 1, "against": "previous", "depth_term": "off: a monocular frame has no depth when it is aligned"}
