"""The dense odometry on the device (include/visual_odometry.h, csrc/gs_odometry.h, slam/odometry.py) against the numpy restatement
(tests/odometry_reference.py): the pyramid bit for bit, the sums of one pass within the float32 rounding of their terms, the full fit on the
planted scene against the planted motion, the gate, determinism, the prior against ground-truth motion on rendered frames, and the SLAM
system with ``Training.pose_prior`` on and off."""
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

import odometry_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

# err <= ONE_PASS_BAR * S for every sum of a pass, S the sum of the absolute values of its terms (|r| as |C| + |P| in g's terms).
# Measured on an MI355X over ONE_PASS_CASES against the float64 restatement, the largest err / S: 4.7e-7 among H's sums, 3.4e-8 among g's,
# 1.3e-8 for sum w, 1.0e-6 for sum w r^2 (S of that one is sum w r^2 itself, and r is a difference of two numbers near 0.5). The bar is 8 x
# the largest of them.
ONE_PASS_BAR = 8e-6
GATE = dict(nu=5.0, sigma_init=0.1, sigma_min=1e-3, min_share=0.3, max_last_step=1e-2, max_translation=1.0, max_rotation=math.radians(30.0))


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _pyramid(image, depth, mask, levels, depth_min=0.0, depth_max=1e6, slack=0):
    from slam import odometry
    H, W = image.shape[-2:]
    buf = torch.zeros(odometry.pyramid_size(W, H, levels) + slack, dtype=torch.uint8, device="cuda")
    odometry.build_pyramid(_dev(image), _dev(depth), _dev(mask), levels, buf, depth_min, depth_max)
    return buf


def _align(image_prev, depth_prev, mask, image_cur, K, levels, iters, T_init=None, with_trace=True, **options):
    """T [4, 4] float64, stats [8], trace [passes, 32] of the device on host arrays."""
    from slam import odometry
    H, W = image_prev.shape[-2:]
    prev, cur = _pyramid(image_prev, depth_prev, mask, levels), _pyramid(image_cur, None, None, levels)
    T = torch.full((4, 4), 7.0, dtype=torch.float32, device="cuda")
    stats = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    trace = torch.full((sum(iters), 32), 7.0, dtype=torch.float64, device="cuda") if with_trace else None
    odometry.align_pyramids(W, H, levels, K, prev, cur, iters, T, stats, T_init=_dev(T_init, torch.float32), trace=trace, **dict(GATE, **options))
    torch.cuda.synchronize()
    return T.double().cpu().numpy(), stats.cpu().numpy(), (None if trace is None else trace.cpu().numpy())


# ---- pyramid ------------------------------------------------------------------------------------------------------------------------------------
def _frame(W, H, seed):
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    depth = rng.uniform(0.3, 6.0, (H, W)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.05] = np.nan
    depth[rng.uniform(size=(H, W)) < 0.05] = np.inf
    depth[rng.uniform(size=(H, W)) < 0.05] = -np.inf
    depth[rng.uniform(size=(H, W)) < 0.05] = 0.0
    depth[rng.uniform(size=(H, W)) < 0.05] = -1.0
    depth[1:5, 2:8] = 0.0                                               # whole blocks without a depth at every level
    mask = (rng.uniform(size=(H, W)) > 0.2).astype(np.uint8) * rng.integers(1, 255, (H, W)).astype(np.uint8)
    return image, depth, mask


@pytest.mark.parametrize("W, H, levels", [(16, 12, 1), (33, 21, 2), (64, 48, 3), (161, 97, 3)])
@pytest.mark.parametrize("inputs", ["depth_and_mask", "depth", "image_alone", "bool_mask"])
def test_pyramid_equals_numpy_float32_bit_for_bit(W, H, levels, inputs):
    from slam import odometry
    image, depth, mask = _frame(W, H, seed=W)
    depth = None if inputs == "image_alone" else depth
    mask = mask if inputs in ("depth_and_mask", "bool_mask") else None
    mask = mask.astype(bool) if inputs == "bool_mask" else mask
    want_pyr, valid0 = ref.pyramid(image, depth, mask, 0.5, 5.0, levels)
    want = ref.pyramid_bytes(want_pyr, valid0)
    assert len(want) == odometry.pyramid_size(W, H, levels)
    got = _pyramid(image, depth, mask, levels, 0.5, 5.0, slack=64).cpu().numpy().tobytes()
    assert got[:len(want)] == want and got[len(want):] == b"\0" * 64      # nothing is written past the size
    if depth is not None:
        assert 0 < valid0 < W * H and any((D > 0).any() for _, D in want_pyr[-1:])
    else:
        assert valid0 == 0


# ---- one pass -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.ONE_PASS_CASES)
def test_one_pass_sums_follow_the_float64_restatement(case):
    image_prev, depth_prev, mask, image_cur, K, iters, T_init = ref.one_pass_case(*case)
    want, scale, margin_px, margin_z = ref.one_pass_reference(case)
    assert margin_px >= 1e-3 and margin_z >= 1e-3                       # no pixel is near enough to a bound for float32 to decide otherwise
    _, stats, trace = _align(image_prev, depth_prev, mask, image_cur, K, case[2], iters, T_init=T_init)
    assert trace.shape == (1, 32)
    got = trace[0]
    assert got[29] == want[29] == stats[4] and got[30] == float(np.float32(0.1)) and got[31] == case[3]
    ratio = np.abs(got[:29] - want[:29]) / scale[:29]
    print(case, "n", int(got[29]), "err / S: H %.2e g %.2e sum w %.2e sum w r^2 %.2e" % (ratio[:21].max(), ratio[21:27].max(), ratio[27], ratio[28]))
    assert np.all(ratio <= ONE_PASS_BAR), (ratio.max(), int(ratio.argmax()))


# ---- the full fit on the planted scene ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(ref.PLANTED_CASES))
@pytest.mark.parametrize("size", sorted(ref.PLANTED_SIZES))
def test_full_fit_recovers_the_planted_motion(size, case):
    levels, iters, bar_deg, bar_mm = ref.PLANTED_SIZES[size]
    s, patch = ref.PLANTED_CASES[case]
    image_prev, depth_prev, image_cur, K, T_true = ref.planted_scene(*size, s=s, patch=patch)
    T, stats, trace = _align(image_prev, depth_prev, None, image_cur, K, levels, iters)
    _, ref_stats, ref_fit, _ = ref.planted_fit(size, case)
    deg, mm = ref.pose_error(T, T_true)
    print(size, case, f"device {deg:.4f} deg {mm:.3f} mm share {stats[1]:.3f} | restatement %.4f deg %.3f mm share {ref_stats[1]:.3f}" % ref.pose_error(ref_fit, T_true))
    assert stats[0] == 1.0 and deg <= bar_deg and mm <= bar_mm
    assert abs(stats[1] - ref_stats[1]) <= 0.02
    assert trace.shape == (sum(iters), 32) and list(trace[:, 31]) == [float(k) for k in range(levels - 1, -1, -1) for _ in range(iters[k])]
    assert stats[7] == size[0] * size[1] and abs(stats[5] - np.linalg.norm(T[:3, 3])) < 1e-6 and abs(stats[6] - ref.rotation_angle(T[:3, :3])) < 1e-6


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------------------------
def test_gate_refuses_on_the_device_and_hands_out_identity():
    from slam import odometry
    W, H, levels, iters = 33, 21, 2, [8, 10]
    image_prev, depth_prev, image_cur, K, T_true = ref.planted_scene(W, H, s=1.0)
    identity = np.eye(4)
    # all depth zero: nothing to align; the workspace beyond its size is not touched
    prev, cur = _pyramid(image_prev, 0 * depth_prev, None, levels), _pyramid(image_cur, None, None, levels)
    need = odometry.align_workspace_size(W, H, levels)
    ws = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    T, stats = torch.full((4, 4), 7.0, device="cuda"), torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    odometry.align_pyramids(W, H, levels, K, prev, cur, iters, T, stats, workspace=ws, **GATE)
    torch.cuda.synchronize()
    assert np.array_equal(T.cpu().numpy(), identity) and stats[0] == 0 and stats[1] == 0 and stats[4] == 0 and stats[7] == 0
    assert bool((ws[need:] == 0x5A).all())
    # the planted motion is larger than the gate lets through
    T, stats, _ = _align(image_prev, depth_prev, None, image_cur, K, levels, iters, max_translation=0.01)
    assert np.array_equal(T, identity) and stats[0] == 0 and stats[5] > 0.01 and stats[1] > 0.5
    T, stats, _ = _align(image_prev, depth_prev, None, image_cur, K, levels, iters, max_rotation=math.radians(0.5))
    assert np.array_equal(T, identity) and stats[0] == 0 and stats[6] > math.radians(0.5)
    T, stats, _ = _align(image_prev, depth_prev, None, image_cur, K, levels, iters, min_share=0.99)
    assert np.array_equal(T, identity) and stats[0] == 0 and 0.5 < stats[1] < 0.99
    # no pass at all: identity in, identity out -- and a T_init is never handed back
    for T_init in (None, T_true):
        T, stats, trace = _align(image_prev, depth_prev, None, image_cur, K, levels, [0, 0], T_init=T_init)
        assert np.array_equal(T, identity) and stats[0] == 0 and trace.shape == (0, 32)
    # a T_init that is not finite lives on the device, where the host cannot see it: the device refuses it
    bad = T_true.copy()
    bad[1, 3] = np.nan
    T, stats, _ = _align(image_prev, depth_prev, None, image_cur, K, levels, iters, T_init=bad)
    assert np.array_equal(T, identity) and stats[0] == 0
    # with T_init at the planted motion the fit stays there and is accepted
    T, stats, _ = _align(image_prev, depth_prev, None, image_cur, K, levels, iters, T_init=T_true)
    assert stats[0] == 1 and ref.pose_error(T, T_true)[0] <= 0.5


def test_bad_arguments_are_refused_with_text_and_touch_nothing():
    from slam import odometry
    lib = odometry._C.load_library()
    assert odometry.pyramid_size(64, 48, 0) == 0 and odometry.pyramid_size(64, 48, 7) == 0 and odometry.pyramid_size(0, 48, 1) == 0
    assert odometry.pyramid_size(64, 48, 4) == 0 and odometry.pyramid_size(64, 63, 4) == 0 and odometry.pyramid_size(64, 64, 4) > 0      # 8 x 6 is too coarse
    assert odometry.align_workspace_size(64, 48, 4) == 0 and odometry.align_workspace_size(64, 48, 3) > 0
    W, H, levels, iters = 33, 21, 2, [8, 10]
    image_prev, depth_prev, image_cur, K, _ = ref.planted_scene(W, H, s=1.0)
    need = odometry.pyramid_size(W, H, levels)
    buf = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="gsr_odometry_pyramid: levels must be in \\[1, 6\\], the coarsest level at least 8 x 8"):
        odometry.build_pyramid(_dev(image_prev), _dev(depth_prev), None, 3, buf)
    with pytest.raises(RuntimeError, match="gsr_odometry_pyramid: workspace must be 16-byte aligned and hold %d bytes \\(gsr_odometry_pyramid_size\\)" % need):
        odometry.build_pyramid(_dev(image_prev), _dev(depth_prev), None, levels, buf[:need - 16])
    with pytest.raises(RuntimeError, match="0 <= depth_min <= depth_max"):
        odometry.build_pyramid(_dev(image_prev), _dev(depth_prev), None, levels, buf, 2.0, 1.0)
    with pytest.raises(RuntimeError, match="depth must be a contiguous float32 device tensor of shape \\(21, 33\\)"):
        odometry.build_pyramid(_dev(image_prev), _dev(depth_prev).double(), None, levels, buf)
    torch.cuda.synchronize()
    assert bool((buf == 0x5A).all())
    prev, cur = _pyramid(image_prev, depth_prev, None, levels), _pyramid(image_cur, None, None, levels)
    T, stats = torch.full((4, 4), 7.0, device="cuda"), torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    ws_need = odometry.align_workspace_size(W, H, levels)
    ws = torch.full((ws_need,), 0x5A, dtype=torch.uint8, device="cuda")
    call = lambda **kw: odometry.align_pyramids(W, H, levels, K, prev, cur, kw.pop("iters", iters), T, stats, **dict(dict(GATE, workspace=ws), **kw))
    with pytest.raises(RuntimeError, match="workspace must be 16-byte aligned and hold %d bytes \\(gsr_odometry_align_workspace_size\\)" % ws_need):
        call(workspace=ws[:ws_need - 16])
    with pytest.raises(RuntimeError, match="iters\\[1\\] must be in \\[0, 64\\], got 65"):
        call(iters=[8, 65])
    with pytest.raises(RuntimeError, match="iters must hold one pass count per level"):
        call(iters=[8])
    with pytest.raises(RuntimeError, match="nu, sigma_init and sigma_min must be positive"):
        call(nu=0.0)
    with pytest.raises(RuntimeError, match="min_share must be in \\[0, 1\\]"):
        call(min_share=1.5)
    with pytest.raises(RuntimeError, match="fx and fy must be positive"):
        odometry.align_pyramids(W, H, levels, (0.0, K[1], K[2], K[3]), prev, cur, iters, T, stats, workspace=ws, **GATE)
    with pytest.raises(RuntimeError, match="gsr_odometry_align: levels must be in \\[1, 6\\]"):
        lib.gsr_odometry_align(W, H, 9, *K, prev.data_ptr(), cur.data_ptr(), None, (odometry.ctypes.c_int * 9)(), 5.0, 0.1, 1e-3, 0.3, 1e-2, 1.0, 1.0,
                               T.data_ptr(), stats.data_ptr(), None, ws.data_ptr(), ws_need, None)
    with pytest.raises(RuntimeError, match="previous and current must hold"):
        odometry.align_pyramids(W, H, levels, K, prev[:64], cur, iters, T, stats, workspace=ws, **GATE)
    torch.cuda.synchronize()
    assert bool((T == 7.0).all()) and bool((stats == 7.0).all()) and bool((ws == 0x5A).all())
    call()                                                                                             # exactly enough
    torch.cuda.synchronize()
    assert stats[0] == 1


# ---- determinism --------------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    image_prev, depth_prev, image_cur, K, _ = ref.planted_scene(160, 120, s=2.5, patch=True)
    runs = [_align(image_prev, depth_prev, None, image_cur, K, 3, [5, 7, 10]) for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert runs[0][1][0] == 1


# ---- the object ------------------------------------------------------------------------------------------------------------------------------------------------
def test_dense_odometry_keeps_swaps_and_summarises():
    from slam import odometry
    image_prev, depth_prev, image_cur, K, T_true = ref.planted_scene(64, 48, s=1.0)
    odo = odometry.DenseOdometry(64, 48, K, max_translation=1.0, max_rotation=30.0)
    with pytest.raises(RuntimeError, match="no previous frame is kept"):
        odo.align(_dev(image_cur))
    odo.keep(_dev(image_prev), _dev(depth_prev), None)
    first = odo._previous.data_ptr()
    T, stats = odo.align(_dev(image_cur))
    want, _, _ = _align(image_prev, depth_prev, None, image_cur, K, 3, [5, 7, 10])
    assert T.is_cuda and stats.is_cuda and np.array_equal(T.double().cpu().numpy(), want)
    odo.keep(_dev(image_cur), _dev(depth_prev), torch.ones(48, 64, dtype=torch.bool, device="cuda"))
    assert odo._current.data_ptr() == first and odo.has_previous                      # the two buffers changed places
    T2, _ = odo.align(_dev(image_cur), T_init=T)                                      # the same picture: no motion, whatever the start
    assert ref.pose_error(T2.double().cpu().numpy(), np.eye(4))[0] < 0.05
    odo.keep(_dev(image_cur))
    assert not odo.has_previous
    s = odo.summary()
    assert s["frames"] == 2 and s["accepted_share"] == 1.0 and 0.5 < s["inlier_share"] <= 1.0 and s["device_ms_per_frame"] > 0.0
    with pytest.raises(ValueError, match="outside what gsr_odometry_pyramid takes"):
        odometry.DenseOdometry(64, 48, K, levels=4, iters=[1, 1, 1, 1])


# ---- the prior against ground truth on rendered frames ---------------------------------------------------------------------------------------------------------------
def test_the_prior_halves_the_error_of_starting_at_the_previous_pose():
    from slam import odometry
    from slam.dataset import SyntheticRGBDDataset
    ds = SyntheticRGBDDataset(num_frames=20, width=160, height=120, seed=0)
    frames = [ds[i] for i in range(20)]
    odo = odometry.DenseOdometry(160, 120, (ds.fx, ds.fy, ds.cx, ds.cy))
    for gap in (1, 3):
        pairs = []
        for i in range(0, 20 - gap):
            (image_i, depth_i, pose_i, _), (image_j, _, pose_j, _) = frames[i], frames[i + gap]
            odo.keep(image_i, torch.as_tensor(depth_i), None)
            pairs.append((odo.align(image_j), pose_j.double() @ torch.linalg.inv(pose_i.double())))
        torch.cuda.synchronize()
        ratios, accepted = [], 0
        for (T, stats), T_true in pairs:
            T, T_true = T.double().cpu().numpy(), T_true.cpu().numpy()
            (deg, mm), (deg0, mm0) = ref.pose_error(T, T_true), ref.pose_error(np.eye(4), T_true)
            ratios.append((deg / deg0, mm / mm0))
            accepted += int(stats[0])
        rot, trans = np.median(np.array(ratios), axis=0)
        print(f"gap {gap}: {len(pairs)} pairs, {accepted} accepted, median err(prior) / err(identity): rotation {rot:.3f}, translation {trans:.3f}")
        assert rot <= 0.5 and trans <= 0.5


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------------------
def _run(training_addition, monocular=False):
    """20 frames at 160 x 120 through the SLAM system, tracking graph on. `training_addition` is merged into Training."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=20, width=160, height=120, seed=0, sensor_depth=not monocular)
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "gaussian_update_every": 60, "gaussian_update_offset": 20, "tracking_graph": True}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 100}})
    if monocular:
        cfg = merge_config(cfg, {"Dataset": {"sensor_type": "monocular"}, "Training": {"kf_interval": 2, "window_size": 4}})
    cfg = merge_config(cfg, {"Training": training_addition})
    slam = SLAM(cfg, ds)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    return slam.run(), slam


def test_slam_run_with_the_prior_on_and_off():
    on, slam_on = _run({"pose_prior": {"enabled": True}})
    off, slam_off = _run({})
    print("prior on:", {k: on[k] for k in ("frames", "keyframes", "ate_rmse", "odometry")}, "| off:", {k: off[k] for k in ("frames", "keyframes", "ate_rmse")})
    assert "odometry" not in off and slam_off.frontend.pose_prior is None
    assert on["frames"] == off["frames"] == 20
    block = on["odometry"]
    assert block["frames"] == 19 and block["accepted_share"] >= 0.8 and block["inlier_share"] > 0.3 and block["device_ms_per_frame"] > 0.0
    assert on["ate_rmse"] <= 1.25 * off["ate_rmse"]


def test_monocular_slam_run_with_the_prior_on():
    on, slam_on = _run({"pose_prior": {"enabled": True}}, monocular=True)
    off, slam_off = _run({}, monocular=True)
    print("prior on:", {k: on[k] for k in ("frames", "keyframes", "ate_rmse", "resets", "odometry")}, "| off:", {k: off[k] for k in ("frames", "keyframes", "ate_rmse", "resets")})
    assert on["frames"] == 20 and "odometry" in on and on["odometry"]["frames"] >= 1
    assert on["resets"] <= off["resets"]                                  # the prior causes no reset
    assert "odometry" not in off and slam_off.frontend.pose_prior is None
