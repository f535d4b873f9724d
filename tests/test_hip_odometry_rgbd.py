"""gsr_odometry_align_rgbd on the device (include/visual_odometry.h, csrc/gs_odometry.h, slam/odometry.py) against the numpy restatement
(tests/odometry_rgbd_reference.py): the sums of one pass within the float32 rounding of their terms, the full fit on the three-plane scene
against the planted motion, what gsr_odometry_align does on the same inputs, the gate, refusals, determinism, that DenseOdometry with the
new keywords at their defaults makes the old call, the stage on flickering frames, and the SLAM system with ``Training.pose_prior_terms``."""
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

import odometry_reference as ref0  # noqa: E402
import odometry_rgbd_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# err <= ONE_PASS_BAR * S for every sum of a pass, S the scale the restatement returns with it.
ONE_PASS_BAR = 1e-6
GATE = dict(ref.GATE, max_rotation=math.radians(30.0))


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _pyramid(image, depth, mask, levels):
    from slam import odometry
    H, W = image.shape[-2:]
    buf = torch.zeros(odometry.pyramid_size(W, H, levels), dtype=torch.uint8, device="cuda")
    odometry.build_pyramid(_dev(image), _dev(depth), _dev(mask), levels, buf)
    return buf


def _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, mask_prev=None, mask_cur=None, T_init=None, **options):
    """T [4, 4] float64, stats [12], trace [passes, 64] of the device on host arrays."""
    from slam import odometry
    H, W = image_prev.shape[-2:]
    prev, cur = _pyramid(image_prev, depth_prev, mask_prev, levels), _pyramid(image_cur, depth_cur, mask_cur, levels)
    T = torch.full((4, 4), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.full((12,), 7.0, dtype=torch.float64, device="cuda")
    trace = torch.full((sum(iters), 64), 7.0, dtype=torch.float64, device="cuda")
    odometry.align_pyramids_rgbd(W, H, levels, K, prev, cur, iters, T, stats, T_init=_dev(T_init, torch.float32), trace=trace,
                                 **dict(dict(GATE, **ref.TERMS), **options))
    torch.cuda.synchronize()
    return T.double().cpu().numpy(), stats.cpu().numpy(), trace.cpu().numpy()


def _align_today(image_prev, depth_prev, image_cur, K, levels, iters):
    """gsr_odometry_align on the same frames: T [4, 4] float64 and stats [8]."""
    from slam import odometry
    H, W = image_prev.shape[-2:]
    prev, cur = _pyramid(image_prev, depth_prev, None, levels), _pyramid(image_cur, None, None, levels)
    T, stats = torch.empty((4, 4), device="cuda"), torch.empty((8,), dtype=torch.float64, device="cuda")
    odometry.align_pyramids(W, H, levels, K, prev, cur, iters, T, stats, **GATE)
    torch.cuda.synchronize()
    return T.double().cpu().numpy(), stats.cpu().numpy()


# ---- one pass -------------------------------------------------------------------------------------------------------------------------------------
def test_the_one_pass_cases_are_all_there():
    assert len(ref.ONE_PASS_CASES) == 7 * 4 and len(set(ref.ONE_PASS_CASES)) == 28
    assert {c[:5] for c in ref.ONE_PASS_CASES} == {(16, 12, 1, 0, True), (16, 12, 1, 0, False), (33, 21, 2, 0, False), (33, 21, 2, 1, False),
                                                   (64, 48, 3, 0, False), (64, 48, 3, 1, False), (64, 48, 3, 2, False)}
    assert {c[5] for c in ref.ONE_PASS_CASES} == {"affine", "depth", "both", "both_holes"}


@pytest.mark.parametrize("case", ref.ONE_PASS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_one_pass_sums_follow_the_float64_restatement(case):
    c = ref.one_pass_case(*case)
    want, scale, margins = ref.one_pass_reference(case)
    for name, least in ref.MIN_MARGIN.items():                          # no decision is near enough to its bound for float32 to take it otherwise
        assert margins[name] >= least, (name, margins[name])
    n, NH, NS = ref.sizes(8 if c["affine"] else 6)
    _, stats, trace = _align(c["image_prev"], c["depth_prev"], c["image_cur"], c["depth_cur"], c["K"], case[2], c["iters"], c["mask_prev"],
                             c["mask_cur"], T_init=c["T_init"], affine=c["affine"], geometric_weight=c["weight"], edge_ratio=c["edge_ratio"])
    assert trace.shape == (1, 64)
    got = trace[0]
    assert got[NH + n + 2] == want[NH + n + 2] == stats[4] and got[NH + n + 5] == want[NH + n + 5] == stats[11]
    assert want[NH + n + 2] >= 50 and (c["weight"] == 0 or want[NH + n + 5] >= 20)
    assert list(got[NS:NS + 5]) == [float(np.float32(0.1)), float(np.float32(0.02)), 0.0, 0.0, float(case[3])] and not got[NS + 5:].any()
    used = scale > 0                                                    # without the depth term its three sums are 0 on both sides
    assert np.array_equal(got[:NS][~used], want[~used])
    ratio = np.abs(got[:NS][used] - want[used]) / scale[used]
    print(case, "n_I", int(want[NH + n + 2]), "n_D", int(want[NH + n + 5]), "largest err / S %.2e at sum %d" % (ratio.max(), np.flatnonzero(used)[ratio.argmax()]))
    assert np.all(ratio <= ONE_PASS_BAR), (ratio.max(), int(np.flatnonzero(used)[ratio.argmax()]))


# ---- the full fit ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ref.FIT_CASES))
@pytest.mark.parametrize("size", sorted(ref0.PLANTED_SIZES))
def test_full_fit_recovers_the_planted_motion(size, case):
    """The restatement on the CPU, the closest to the bars at 33 x 21: gain_affine 0.15 deg / 5.4 mm, textured_depth 1.4 mm,
    gain_affine_depth 1.4 mm."""
    levels, iters, bar_deg, bar_mm = ref0.PLANTED_SIZES[size]
    name, s = ref.FIT_CASES[case]
    flat, gain, offset, affine, weight = ref.FIT_VARIANTS[name]
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(*size, s=s, flat=flat, gain=gain, offset=offset)
    T, stats, trace = _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, affine=affine, geometric_weight=weight)
    _, ref_stats, ref_fit, _ = ref.planted_fit(size, case)
    (deg, mm), (ref_deg, ref_mm) = ref0.pose_error(T, T_true), ref0.pose_error(ref_fit, T_true)
    against = ref0.pose_error(T, ref_fit)
    print(size, case, f"device {deg:.4f} deg {mm:.3f} mm alpha {stats[8]:.4f} beta {stats[9]:.4f} n_D {stats[11]:.0f} | restatement {ref_deg:.4f} deg "
          f"{ref_mm:.3f} mm alpha {ref_stats[8]:.4f} beta {ref_stats[9]:.4f} | apart {against[0]:.4f} deg {against[1]:.3f} mm")
    assert stats[0] == 1.0 and ref_stats[0] == 1.0
    assert deg <= bar_deg and mm <= bar_mm                                                   # against the truth
    assert against[0] <= bar_deg and against[1] <= bar_mm                                    # against the restatement's fit
    assert abs(stats[1] - ref_stats[1]) <= 0.02 and abs(stats[8] - ref_stats[8]) <= 1e-3 and abs(stats[9] - ref_stats[9]) <= 1e-3
    assert trace.shape == (sum(iters), 64)
    n, NH, NS = ref.sizes(8 if affine else 6)
    assert list(trace[:, NS + 4]) == [float(k) for k in range(levels - 1, -1, -1) for _ in range(iters[k])]
    assert (stats[11] > 0) == (weight > 0) and (affine or (stats[8] == 0 and stats[9] == 0))


@pytest.mark.parametrize("s", [1.0, 2.5])
@pytest.mark.parametrize("size", sorted(ref.FLAT_SIZES))
def test_the_depth_term_aligns_a_scene_without_texture(size, s):
    """One colour everywhere: the depth term alone, affine = 0. The restatement gave at most 0.001 deg / 0.013 mm on both sizes. The bar is the
    64 x 48 row of PLANTED_SIZES. gsr_odometry_align has nothing to align there and refuses."""
    levels, iters = ref.FLAT_SIZES[size]
    _, _, bar_deg, bar_mm = ref0.PLANTED_SIZES[(64, 48)]
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(*size, s=s, flat=True)
    T, stats, _ = _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, affine=False, geometric_weight=1.0)
    deg, mm = ref0.pose_error(T, T_true)
    ref_fit = ref.fit(size, levels, iters, True, 1.0, 0.0, False, 1.0, s)[2]
    against = ref0.pose_error(T, ref_fit)
    print(size, s, f"device {deg:.4f} deg {mm:.3f} mm, from the restatement's fit {against[0]:.4f} deg {against[1]:.3f} mm")
    assert stats[0] == 1.0 and deg <= bar_deg and mm <= bar_mm and against[0] <= bar_deg and against[1] <= bar_mm
    T_today, stats_today = _align_today(image_prev, depth_prev, image_cur, K, levels, iters)
    assert stats_today[0] == 0.0 and np.array_equal(T_today, np.eye(4)) and np.isinf(stats_today[3])


@pytest.mark.parametrize("s", [1.0, 2.5])
def test_a_gain_change_misleads_the_photometric_fit_and_its_gate(s):
    """Why the affine term exists: under current = 1.25 image + 0.06, gsr_odometry_align ends more than 5 degrees off and its gate accepts."""
    size = (160, 120)
    levels, iters, _, _ = ref0.PLANTED_SIZES[size]
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(*size, s=s, gain=1.25, offset=0.06)
    T_today, stats_today = _align_today(image_prev, depth_prev, image_cur, K, levels, iters)
    deg, mm = ref0.pose_error(T_today, T_true)
    print(s, f"gsr_odometry_align under the gain: accepted {stats_today[0]:.0f}, {deg:.2f} deg {mm:.1f} mm off, last step {stats_today[3]:.2e}")
    assert stats_today[0] == 1.0 and deg > 5.0


@pytest.mark.parametrize("case", ["gain_affine_1.0", "gain_affine_depth_2.5"])
def test_alpha_and_beta_are_the_gain_and_the_offset(case):
    """(0.2485, 0.0607) in the restatement at 160 x 120 for (0.25, 0.06) planted."""
    size = (160, 120)
    levels, iters, _, _ = ref0.PLANTED_SIZES[size]
    name, s = ref.FIT_CASES[case]
    flat, gain, offset, affine, weight = ref.FIT_VARIANTS[name]
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(*size, s=s, flat=flat, gain=gain, offset=offset)
    _, stats, trace = _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, affine=affine, geometric_weight=weight)
    print(case, "alpha %.4f beta %.4f" % (stats[8], stats[9]))
    assert stats[0] == 1.0 and abs(stats[8] - 0.25) <= 0.01 and abs(stats[9] - 0.06) <= 0.01
    n, NH, NS = ref.sizes(8)
    assert trace[0, NS + 2] == 0.0 and trace[0, NS + 3] == 0.0 and trace[-1, NS + 2] != 0.0            # both start at 0 and carry


# ---- the gate -------------------------------------------------------------------------------------------------------------------------------------------------
def test_gate_refuses_on_the_device_and_hands_out_identity():
    W, H, levels, iters = 64, 48, 3, [5, 7, 10]
    image_prev, depth_prev, image_cur, depth_cur, K, T_true = ref.scene(W, H, gain=1.25, offset=0.06)
    identity = np.eye(4)
    run = lambda **kw: _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, iters, **dict(dict(affine=True, geometric_weight=1.0), **kw))
    T, stats, _ = run()
    assert stats[0] == 1 and ref0.pose_error(T, T_true)[0] <= 0.1
    T, stats, _ = run(max_gain=0.1)
    assert np.array_equal(T, identity) and stats[0] == 0 and stats[8] > 0.1
    T, stats, _ = run(max_offset=0.01)
    assert np.array_equal(T, identity) and stats[0] == 0 and stats[9] > 0.01
    T, stats, _ = run(max_gain=0.1, affine=False)                      # without the affine term its two bounds are not looked at
    assert stats[8] == 0 and stats[9] == 0 and stats[3] < np.inf
    T, stats, _ = run(max_translation=0.01)
    assert np.array_equal(T, identity) and stats[0] == 0 and stats[5] > 0.01
    bad = T_true.copy()
    bad[1, 3] = np.nan
    T, stats, _ = run(T_init=bad)
    assert np.array_equal(T, identity) and stats[0] == 0
    T, stats, trace = _align(image_prev, depth_prev, image_cur, depth_cur, K, levels, [0, 0, 0], T_init=T_true, affine=True, geometric_weight=1.0)
    assert np.array_equal(T, identity) and stats[0] == 0 and trace.shape == (0, 64)
    # a constant image: alpha and beta cannot be told apart, no pass takes a step, with or without the depth term
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(W, H, flat=True)
    for weight in (0.0, 1.0):
        T, stats, trace = _align(image_prev, depth_prev, image_cur, depth_cur, K, 2, [8, 10], affine=True, geometric_weight=weight)
        assert np.array_equal(T, identity) and stats[0] == 0 and np.isinf(stats[3]) and stats[8] == 0 and stats[9] == 0
        assert stats[4] > 2000 and np.all(np.isfinite(trace))


def test_bad_arguments_are_refused_with_text_and_touch_nothing():
    from slam import odometry
    lib = odometry._C.load_library()
    W, H, levels, iters = 33, 21, 2, [8, 10]
    assert odometry.align_rgbd_workspace_size(64, 48, 4) == 0 and odometry.align_rgbd_workspace_size(W, H, levels) > 0
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(W, H)
    prev, cur = _pyramid(image_prev, depth_prev, None, levels), _pyramid(image_cur, depth_cur, None, levels)
    need = odometry.align_rgbd_workspace_size(W, H, levels)
    guard = 256                                                         # bytes either side of every output
    Tb, sb = torch.full((guard // 4 * 2 + 16,), 7.0, device="cuda"), torch.full((guard // 8 * 2 + 12,), 7.0, dtype=torch.float64, device="cuda")
    tb = torch.full((guard // 8 * 2 + 18 * 64,), 7.0, dtype=torch.float64, device="cuda")
    wb = torch.full((need + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    T, stats = Tb[guard // 4:guard // 4 + 16].view(4, 4), sb[guard // 8:guard // 8 + 12]
    trace, ws = tb[guard // 8:guard // 8 + 18 * 64].view(18, 64), wb[guard:guard + need]
    base = dict(dict(GATE, **ref.TERMS), affine=True, geometric_weight=1.0, workspace=ws, trace=trace)
    call = lambda **kw: odometry.align_pyramids_rgbd(W, H, levels, K, prev, cur, kw.pop("iters", iters), T, stats, **dict(base, **kw))
    for text, kw in (("workspace must be 16-byte aligned and hold %d bytes \\(gsr_odometry_align_rgbd_workspace_size\\)" % need, dict(workspace=ws[:need - 16])),
                     ("iters\\[1\\] must be in \\[0, 64\\], got 65", dict(iters=[8, 65], trace=None)),
                     ("iters must hold one pass count per level", dict(iters=[8], trace=None)),
                     ("nu, sigma_init and sigma_min must be positive", dict(nu=0.0)), ("min_share must be in \\[0, 1\\]", dict(min_share=1.5)),
                     ("geometric_weight and edge_ratio must be finite and not negative", dict(geometric_weight=-1.0)),
                     ("geometric_weight and edge_ratio must be finite and not negative", dict(edge_ratio=float("nan"))),
                     ("sigma_depth_init and sigma_depth_min must be positive", dict(sigma_depth_init=0.0)),
                     ("sigma_depth_init and sigma_depth_min must be positive", dict(sigma_depth_min=float("inf"))),
                     ("max_gain and max_offset must not be negative", dict(max_gain=-0.1)),
                     ("max_gain and max_offset must not be negative", dict(max_offset=float("nan"))),
                     ("stats must be a contiguous torch.float64 device tensor of shape \\(12,\\)", dict())):
        with pytest.raises(RuntimeError, match=text):
            if text.startswith("stats"):
                odometry.align_pyramids_rgbd(W, H, levels, K, prev, cur, iters, T, sb[:8], **base)
            else:
                call(**kw)
    with pytest.raises(RuntimeError, match="fx and fy must be positive"):
        odometry.align_pyramids_rgbd(W, H, levels, (0.0, K[1], K[2], K[3]), prev, cur, iters, T, stats, **base)
    with pytest.raises(RuntimeError, match="previous and current must hold"):
        odometry.align_pyramids_rgbd(W, H, levels, K, prev[:64], cur, iters, T, stats, **base)
    raw = lambda lv, affine: lib.gsr_odometry_align_rgbd(W, H, lv, *K, prev.data_ptr(), cur.data_ptr(), None, (odometry.ctypes.c_int * 9)(), affine, 1.0, 0.05,
                                                         5.0, 0.1, 1e-3, 0.02, 1e-4, 0.3, 1e-2, 1.0, 1.0, 0.5, 0.3, T.data_ptr(), stats.data_ptr(), None,
                                                         ws.data_ptr(), need, None)
    with pytest.raises(RuntimeError, match="gsr_odometry_align_rgbd: levels must be in \\[1, 6\\]"):
        raw(9, 1)
    with pytest.raises(RuntimeError, match="gsr_odometry_align_rgbd: affine must be 0 or 1, got 2"):
        raw(levels, 2)
    torch.cuda.synchronize()
    assert bool((Tb == 7.0).all()) and bool((sb == 7.0).all()) and bool((tb == 7.0).all()) and bool((wb == 0x5A).all())
    call()                                                                                             # exactly enough
    torch.cuda.synchronize()
    assert stats[0] == 1 and bool((trace != 7.0).all())
    g4, g8 = guard // 4, guard // 8                                      # the guards either side of every output
    assert bool((Tb[:g4] == 7.0).all()) and bool((Tb[g4 + 16:] == 7.0).all()) and bool((sb[:g8] == 7.0).all()) and bool((sb[g8 + 12:] == 7.0).all())
    assert bool((tb[:g8] == 7.0).all()) and bool((tb[g8 + 18 * 64:] == 7.0).all())
    assert bool((wb[:guard] == 0x5A).all()) and bool((wb[guard + need:] == 0x5A).all())


# ---- determinism and compatibility ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(160, 120, s=2.5, gain=1.25, offset=0.06)
    runs = [_align(image_prev, depth_prev, image_cur, depth_cur, K, 3, [5, 7, 10], affine=True, geometric_weight=1.0) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert runs[0][1][0] == 1


def test_dense_odometry_with_the_new_keywords_at_their_defaults_makes_the_old_call():
    from slam import odometry
    image_prev, depth_prev, image_cur, depth_cur, K, _ = ref.scene(64, 48, s=1.0)
    prev, cur = _pyramid(image_prev, depth_prev, None, 3), _pyramid(image_cur, None, None, 3)
    T, stats = torch.empty((4, 4), device="cuda"), torch.empty((8,), dtype=torch.float64, device="cuda")
    odometry.align_pyramids(64, 48, 3, K, prev, cur, [5, 7, 10], T, stats)
    for keywords in ({}, dict(affine=False, geometric_weight=0.0, edge_ratio=0.05, sigma_depth_init=0.02, sigma_depth_min=1e-4, max_gain=0.5, max_offset=0.3)):
        odo = odometry.DenseOdometry(64, 48, K, **keywords)
        assert odo.terms is None and odo._workspace.numel() == odometry.align_workspace_size(64, 48, 3)
        odo.keep(_dev(image_prev), _dev(depth_prev), None)
        for depth in (None, _dev(depth_cur)):                           # a current depth without a term that uses it changes no byte of the result
            T2, stats2 = odo.align(_dev(image_cur), depth=depth)
            torch.cuda.synchronize()
            assert stats2.shape == (8,) and T2.cpu().numpy().tobytes() == T.cpu().numpy().tobytes()
            assert stats2.cpu().numpy().tobytes() == stats.cpu().numpy().tobytes()
        assert set(odo.summary()) == {"frames", "accepted_share", "inlier_share", "device_ms_per_frame"}
    on = odometry.DenseOdometry(64, 48, K, affine=True, geometric_weight=1.0, max_translation=1.0)
    on.keep(_dev(image_prev), _dev(depth_prev), None)
    T3, stats3 = on.align(_dev(image_cur), depth=_dev(depth_cur))
    assert stats3.shape == (12,) and stats3[0] == 1 and stats3[11] > 0
    s = on.summary()
    assert s["frames"] == 1 and 0.5 < s["depth_term_share"] <= 1.0 and s["mean_abs_alpha"] < 0.02 and s["mean_abs_beta"] < 0.02


# ---- the stage on flickering frames, no SLAM run ---------------------------------------------------------------------------------------------------------------
def test_the_terms_keep_the_prior_on_frames_whose_brightness_flickers():
    """Consecutive frames of the synthetic sequence at 320 x 240, every second current image times 0.8. The median relative-pose error against
    the dataset's poses over the accepted pairs, measured on an MI355X (printed again by every run; README.md quotes them):
        photometric alone   plain 0.0088 deg / 0.538 mm (20 of 20 accepted)   flickered: all 19 refused
        both terms on       plain 0.0030 deg / 0.088 mm (20 of 20)            flickered 0.0029 deg / 0.091 mm (19 of 19)"""
    from slam import odometry
    from slam.dataset import SyntheticRGBDDataset
    ds = SyntheticRGBDDataset(num_frames=40, width=320, height=240, seed=0)
    frames = [ds[i] for i in range(40)]
    K = (ds.fx, ds.fy, ds.cx, ds.cy)
    today, new = odometry.DenseOdometry(320, 240, K), odometry.DenseOdometry(320, 240, K, affine=True, geometric_weight=1.0)
    results = []
    for i in range(39):
        (image_i, depth_i, pose_i, _), (image_j, depth_j, pose_j, _) = frames[i], frames[i + 1]
        flicker = i % 2 == 1
        image_j = image_j * 0.8 if flicker else image_j
        T_true = (pose_j.double() @ torch.linalg.inv(pose_i.double())).cpu().numpy()
        today.keep(image_i, torch.as_tensor(depth_i), None)
        new.keep(image_i, torch.as_tensor(depth_i), None)
        results.append((flicker, T_true, today.align(image_j), new.align(image_j, depth=torch.as_tensor(depth_j))))
    torch.cuda.synchronize()
    err = {(mode, flicker): [] for mode in ("today", "new") for flicker in (False, True)}
    refused = {k: 0 for k in err}
    for flicker, T_true, (T_a, stats_a), (T_b, stats_b) in results:
        for mode, T, stats in (("today", T_a, stats_a), ("new", T_b, stats_b)):
            if stats[0] == 0:
                refused[(mode, flicker)] += 1
            else:
                err[(mode, flicker)].append(ref0.pose_error(T.double().cpu().numpy(), T_true))
    med = {k: (np.median(np.array(v), axis=0) if v else np.array([np.inf, np.inf])) for k, v in err.items()}
    for k in sorted(err):
        print(k, "accepted %d refused %d median %.4f deg %.3f mm" % (len(err[k]), refused[k], med[k][0], med[k][1]))
    assert refused[("new", True)] == 0 and refused[("new", False)] == 0
    assert np.all(med[("new", True)] <= 2.0 * med[("new", False)])                    # the same optimiser on other input: within 2 x
    all_refused = not err[("today", True)]
    assert all_refused or np.all(med[("today", True)] >= 5.0 * med[("new", True)])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
def _run(training_addition):
    """40 frames at 320 x 240 through the SLAM system with the training block of tests/test_hip_odometry.py's _run."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=40, width=320, height=240, seed=0)
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "gaussian_update_every": 60, "gaussian_update_offset": 20, "tracking_graph": True}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 100}})
    cfg = merge_config(cfg, {"Training": training_addition})
    slam = SLAM(cfg, ds)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    result = slam.run()
    poses = torch.stack([torch.cat([slam.frontend.cameras[k].R.reshape(-1), slam.frontend.cameras[k].T.reshape(-1)]) for k in sorted(slam.frontend.cameras)])
    return result, poses.cpu().numpy()


_photometric = {}


def _photometric_run():
    if not _photometric:
        _photometric["result"] = _run({"pose_prior": {"enabled": True}})[0]
    return _photometric["result"]


@pytest.mark.parametrize("against", ["previous", "keyframe"])
def test_slam_run_with_the_terms_on(against):
    """Measured on an MI355X, ATE RMSE on the clean sequence: photometric prior 6.76 mm; the terms against the previous frame 8.85 mm,
    against keyframes 6.76 mm; every alignment accepted, depth terms on 0.72 of the aligned pixels, mean |alpha| 0.002."""
    block = {"pose_prior": {"enabled": True}, "pose_prior_terms": {"enabled": True, "against": against}}
    (on, poses), (again, poses_again) = _run(block), _run(block)
    base = _photometric_run()
    print(against, {k: on[k] for k in ("frames", "keyframes", "ate_rmse", "odometry")}, "| photometric prior:", {k: base[k] for k in ("ate_rmse", "odometry")})
    assert on["frames"] == 40 and set(base["odometry"]) == {"frames", "accepted_share", "inlier_share", "device_ms_per_frame"}
    odo = on["odometry"]
    assert set(odo) == {"frames", "accepted_share", "inlier_share", "device_ms_per_frame", "mean_abs_alpha", "mean_abs_beta", "depth_term_share", "against"}
    assert odo["against"] == against and odo["frames"] == 39 and odo["accepted_share"] > 0 and 0 < odo["depth_term_share"] <= 1
    assert poses.tobytes() == poses_again.tobytes() and on["ate_rmse"] == again["ate_rmse"]
    assert on["ate_rmse"] <= 2.0 * base["ate_rmse"]
