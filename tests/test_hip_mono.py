"""Monocular (RGB-only) input on the device: the keyframe-depth kernels (gsr_mono_keyframe_depth, include/slam_map.h), the fused tracking
step and the mapping graphs with RGB-only operands against their eager routes, and one whole run on the synthetic sequence with the depth
withheld."""
import math

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)

pytestmark = pytest.mark.gpu

THRESHOLD = 0.01


# ---- 1. gsr_mono_keyframe_depth ------------------------------------------------------------------------------------------------------
def _mono_case(H, W, kind):
    """(depth, opacity, gt_image, noise) CPU tensors. Colour sums sit far from the threshold (0 or >= 0.3) and opacities far from 0.95, so
    the masks do not hang on a rounding."""
    g = torch.Generator().manual_seed(1000 * H + W + sum(map(ord, kind)))
    n = H * W
    depth = 0.5 + 3.0 * torch.rand(H, W, generator=g)
    opacity = torch.full((H, W), 0.99)
    image = 0.1 + 0.8 * torch.rand(3, H, W, generator=g)
    noise = torch.randn(H, W, generator=g)

    def keep_only(k):                       # exactly k valid pixels, spread over the image
        order = torch.randperm(n, generator=g)
        opacity.view(-1)[order[k:]] = 0.5

    if kind == "opacity":                   # about 60 % knocked out (never all but one)
        drop = torch.rand(H, W, generator=g) < 0.6
        drop.view(-1)[:2] = False
        opacity[drop] = 0.5
    elif kind == "rgb_band":
        image[:, : max(1, H // 3)] = 0.0
        if n > 4:
            depth.view(-1)[-1] = 0.0        # one pixel without rendered depth as well
    elif kind == "constant":
        depth.fill_(1.75)
        opacity.view(-1)[n // 2:] = 0.5
    elif kind == "even":
        keep_only(n - (n % 2) - (2 if n > 4 else 0))
    elif kind == "odd":
        keep_only(n - 1 - (n % 2))
    elif kind == "none":
        keep_only(0)
    elif kind == "one":
        keep_only(1)
    else:
        assert kind == "all"
    return depth, opacity, image, noise


def _expected_masks(depth, opacity, image):
    rgb_ok = (image[0] + image[1]) + image[2] > THRESHOLD
    return rgb_ok, (depth > 0) & (opacity > 0.95) & rgb_ok


def _call(depth, opacity, image, noise, stream=None):
    from slam.keyframes import mono_keyframe_depth
    dev = "cuda"
    args = [t.to(dev) for t in (depth, opacity, image)]
    if stream is None:
        out, stats = mono_keyframe_depth(*args, THRESHOLD, noise.to(dev))
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out, stats = mono_keyframe_depth(*args, THRESHOLD, noise.to(dev))
        torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    return out.cpu(), stats.cpu()


SIZES = [(2, 2), (16, 16), (17, 33), (65, 1024)]       # the last: a second trip of the select's strided loop (64 blocks x 1024 threads)
KINDS = ["all", "opacity", "rgb_band", "constant", "even", "odd", "none", "one"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_mono_keyframe_depth(H, W, kind):
    depth, opacity, image, noise = _mono_case(H, W, kind)
    rgb_ok, valid = _expected_masks(depth, opacity, image)
    n_valid = int(valid.sum())
    out, stats = _call(depth, opacity, image, noise)
    median, std, got_n = stats[0], stats[1], int(stats.view(torch.int32)[2])
    print(f"mono_keyframe_depth {H}x{W} {kind}: n_valid {got_n} (want {n_valid}) median {float(median)} std {float(std)}")
    assert got_n == n_valid
    assert {"even": n_valid % 2 == 0 and n_valid >= 2, "odd": n_valid % 2 == 1 and n_valid >= 3, "none": n_valid == 0, "one": n_valid == 1}.get(kind, n_valid >= 2)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(stats[:2]).all())
    if n_valid < 2:
        assert float(out.abs().max()) == 0.0 and float(median) == 0.0 and float(std) == 0.0
    else:
        values = depth[valid]
        assert torch.equal(median, values.median())                                     # the lower of the two middle values, bit for bit
        want_std = float(values.double().std())
        assert abs(float(std) - want_std) <= 1e-5 * want_std
        # the rule, in fp32 on the host from the kernel's own median and std
        bad = ~valid | (depth > median + std) | (depth < median - std)
        want = torch.where(bad, median, depth) + noise * torch.where(bad, 0.5 * std, 0.2 * std)
        want[~rgb_ok] = 0
        assert torch.equal(out, want), f"{int((out != want).sum())} of {out.numel()} pixels differ, max {float((out - want).abs().max())}"
        if kind == "constant":
            assert float(std) == 0.0 and torch.equal(out[rgb_ok], depth[rgb_ok])
        if kind == "rgb_band":
            assert float(out[: max(1, H // 3)].abs().max()) == 0.0 and int((~rgb_ok).sum()) == max(1, H // 3) * W
    # twice in a row, and once on a side stream: the same bits
    again, stats_again = _call(depth, opacity, image, noise)
    side, stats_side = _call(depth, opacity, image, noise, stream=torch.cuda.Stream())
    for o, s in ((again, stats_again), (side, stats_side)):
        assert torch.equal(o, out) and torch.equal(s.view(torch.int32), stats.view(torch.int32))


def test_mono_keyframe_depth_refuses_bad_arguments():
    from diff_gaussian_rasterization import _C
    L = _C.load_library()
    z = torch.zeros(64, device="cuda")
    with pytest.raises(RuntimeError, match="gsr_mono_keyframe_depth"):
        L.gsr_mono_keyframe_depth(z.data_ptr(), z.data_ptr(), z.data_ptr(), 0, 4, THRESHOLD, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None)
    with pytest.raises(RuntimeError, match="gsr_mono_keyframe_depth"):
        L.gsr_mono_keyframe_depth(z.data_ptr(), None, z.data_ptr(), 2, 2, THRESHOLD, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None)
    assert L.gsr_mono_keyframe_depth_workspace_size(3, 5) == 2080 + 4 * 15


# ---- shared set-up of 2. - 4. ----------------------------------------------------------------------------------------------------------
def _mono_config(**training):
    from slam.system import default_config, merge_config
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 2, "window_size": 4}
    t.update(training)
    return merge_config(default_config(), {"Training": t, "Dataset": {"sensor_type": "monocular", "pcd_downsample": 32, "pcd_downsample_init": 8},
                                           "opt_params": {"densify_from_iter": 100}})


class _NoDepth:
    """A dataset whose frames carry depth = None, whatever the wrapped dataset knows: any read of sensor depth fails loudly."""

    def __init__(self, inner):
        self._inner = inner

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def __len__(self):
        return len(self._inner)

    def __getitem__(self, idx):
        color, _depth, pose, motion = self._inner[idx]
        return color, None, pose, motion


def _mono_slam(num_frames, width, height, seed=0, **training):
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM
    torch.manual_seed(0)
    ds = _NoDepth(SyntheticRGBDDataset(num_frames=num_frames, width=width, height=height, seed=0))
    slam = SLAM(_mono_config(**training), ds)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(seed)          # the seeding noise
    return slam, ds


# ---- 2. the fused tracking step with RGB-only input ---------------------------------------------------------------------------------------
def test_fused_tracking_step_equals_the_autograd_iteration_for_monocular_input():
    """The conditions of tests/test_hip_slam.py::test_fused_tracking_step_equals_the_autograd_iteration with RGB-only operands (alpha = 1,
    zero depth planes), at 48x64 with a few hundred Gaussians; the depth cotangent is all zero on both routes."""
    import gaussian_renderer
    import slam.tracking_graph as tgm
    import slam_losses
    from slam.camera import Camera
    slam, ds = _mono_slam(4, 64, 48, init_itr_num=100, tracking_itr_num=12)      # (no densification after iteration 0: the 384 seeded Gaussians)
    cfg, fe = slam.config, slam.frontend
    fe.run(max_frames=1)
    assert 100 < fe.gaussians.get_xyz.shape[0] < 1000
    cam = Camera.init_from_dataset(ds, 1, ds.projection_matrix)
    assert cam.depth is None
    cam.compute_grad_mask(cfg)
    cam.update_RT(fe.cameras[0].R, fe.cameras[0].T)
    fused = tgm.TrackingGraph(fe.gaussians, fe.pipeline_params, fe.background, cfg, cam)
    assert fused.fused and fused.alpha == 1.0
    old = tgm.FUSED_STEP
    tgm.FUSED_STEP = False
    try:
        auto = tgm.TrackingGraph(fe.gaussians, fe.pipeline_params, fe.background, cfg, cam)
    finally:
        tgm.FUSED_STEP = old
    assert not auto.fused
    fused.load(cam); auto.load(cam)
    for t in (fused, auto):
        assert float(t.gt_depth.abs().max()) == 0.0 and float(t.w_dep.abs().max()) == 0.0 and float(t.w_rgb.max()) == 1.0
    with torch.no_grad():
        for t in (fused, auto):
            t.cam.exposure_a.fill_(0.03); t.cam.exposure_b.fill_(-0.01)
    c = auto.cam
    image, radii, depth, opacity, n_touched = gaussian_renderer._render_fused(c, auto.frozen, auto.background, 1.0, auto.means2D, None, None, None,
                                                                              auto.static, False)
    image.retain_grad(); depth.retain_grad()
    loss = slam_losses.weighted_l1_loss(image, depth, auto.gt_image, auto.gt_depth, auto.w_rgb, auto.w_dep, c.exposure_a, c.exposure_b, auto.alpha,
                                        opacity=opacity, opacity_depth_threshold=0.95, compute_value=False)
    loss.backward(auto._one)
    g_img, g_dep = image.grad.clone(), depth.grad.clone()
    g_rot, g_trans = c.cam_rot_delta.grad.clone(), c.cam_trans_delta.grad.clone()
    g_a, g_b = c.exposure_a.grad.clone(), c.exposure_b.grad.clone()
    c.pose_step(*auto.lrs, latch=True)
    pkg = fused.iteration()
    H, W = int(c.image_height), int(c.image_width)
    N, T = H * W, ((W + 15) // 16) * ((H + 15) // 16)
    ws = fused.workspace.view(torch.float32)
    assert torch.equal(pkg["render"], image.detach()) and torch.equal(pkg["depth"], depth.detach()) and torch.equal(pkg["opacity"], opacity.detach())
    assert float(g_img.abs().max()) > 0
    assert torch.equal(ws[:3 * N].view(3, H, W), g_img) and torch.equal(ws[3 * N:4 * N].view(1, H, W), g_dep)
    assert float(g_dep.abs().max()) == 0.0 and float(ws[3 * N:4 * N].abs().max()) == 0.0
    tau = ws[4 * N + 2 * T:4 * N + 2 * T + 6]
    assert float(g_rot.abs().max()) > 0 and float(g_trans.abs().max()) > 0
    assert torch.equal(tau[3:], g_rot.view(-1)) and torch.equal(tau[:3], g_trans.view(-1))
    g_exp = ws[4 * N + 2 * T + 6:4 * N + 2 * T + 8]
    torch.testing.assert_close(g_exp[0:1], g_a.view(-1), rtol=2e-5, atol=1e-8)
    torch.testing.assert_close(g_exp[1:2], g_b.view(-1), rtol=2e-5, atol=1e-8)
    assert torch.equal(fused.cam.R, auto.cam.R) and torch.equal(fused.cam.T, auto.cam.T)
    torch.testing.assert_close(fused.cam.exposure_a.detach(), auto.cam.exposure_a.detach(), rtol=1e-5, atol=1e-8)
    for _ in range(9):
        fused.iteration(); auto.iteration()
    torch.testing.assert_close(fused.cam.R, auto.cam.R, rtol=0, atol=2e-6)
    torch.testing.assert_close(fused.cam.T, auto.cam.T, rtol=0, atol=2e-6)
    torch.testing.assert_close(fused.cam.exposure_a.detach(), auto.cam.exposure_a.detach(), rtol=1e-4, atol=1e-7)
    torch.testing.assert_close(fused.cam.exposure_b.detach(), auto.cam.exposure_b.detach(), rtol=1e-4, atol=1e-7)
    assert float(fused.cam._adam[16]) == 10.0 == float(auto.cam._adam[16])


# ---- 3. static mapping as graph replays -----------------------------------------------------------------------------------------------------
def _mono_map_static_outcome(graph, calls):
    """tests/test_hip_slam.py::_map_static_outcome for monocular input: seven keyframes without depth, a window of the four newest (the
    window size, so that the pruning call prunes by covisibility), states after consecutive map_static calls and after the pruning call."""
    from test_hip_slam import _map_static_state
    from slam.camera import Camera
    slam, ds = _mono_slam(14, 160, 120, init_itr_num=60, gaussian_update_every=30, gaussian_update_offset=12, mapping_graph="strict" if graph else False)
    cfg, fe, be = slam.config, slam.frontend, slam.backend
    fe.run(max_frames=1)
    for idx in range(2, 14, 2):
        cam = Camera.init_from_dataset(ds, idx, ds.projection_matrix)
        cam.compute_grad_mask(cfg)
        cam.update_RT(cam.R_gt, cam.T_gt)
        fe.cameras[idx] = cam
        be.viewpoints[idx] = cam
        be.add_next_kf(idx, cam, depth_map=fe.add_new_keyframe(idx))
        cam.reset_pose_optimizer()
    window = [12, 10, 8, 6]
    for k, idx in enumerate(window):
        cam = be.viewpoints[idx]
        cam.update_RT(cam.R_gt, cam.T_gt + torch.tensor([0.004 * (k + 1), -0.003, 0.002], device=cam.T_gt.device))
    out = []
    for n in calls:
        be.map_static(window, iters=n)
        torch.cuda.synchronize()
        out.append(_map_static_state(be))
    be.map_static(window, prune=True)
    torch.cuda.synchronize()
    out.append(_map_static_state(be))
    return out, window, be


def test_static_mapping_graph_replays_are_bit_identical_to_eager_for_monocular_input():
    from test_hip_slam import _first_difference
    calls = (10, 20, 20)
    eager, window, be_eager = _mono_map_static_outcome(False, calls)
    graph, _, be_graph = _mono_map_static_outcome(True, calls)
    st = graph[-1]["graph_stats"]
    print(st)
    assert eager[-1]["graph_stats"] is None
    diffs = [_first_difference(e, g, window) for e, g in zip(eager, graph)]
    assert diffs == [None] * len(diffs), diffs
    assert st is not None and st["runs"] >= 3 and st["replays"] >= 30 and st["failed"] == 0 and st["redone"] == 0, st
    assert max(float(graph[-1]["poses"][k][4].abs().max()) for k in window) > 0          # the poses did move
    # the pruning call pruned by covisibility, alike on both sides, and the map counts as initialised
    assert be_eager.initialized and be_graph.initialized
    assert eager[-1]["params"][0].shape[0] < eager[-2]["params"][0].shape[0]
    for k in window:
        assert eager[-1]["visibility"][k].shape[0] == eager[-1]["params"][0].shape[0]


# ---- 4. one whole run ------------------------------------------------------------------------------------------------------------------------
RUN_FRAMES = 20


def run_monocular_sequence(seed):
    """The run the whole-sequence test asserts on (measurement scripts call it with other seeds): 20 frames at 160x120, window 4,
    kf_interval 2. Returns (slam, result, estimated camera-to-world poses, scale-aligned ATE of the stationary trajectory)."""
    from slam.eval_utils import _pose_c2w, ate_sim3
    slam, ds = _mono_slam(RUN_FRAMES, 160, 120, seed=seed)
    res = slam.run()
    fe = slam.frontend
    ids = sorted(fe.cameras)
    gt = [_pose_c2w(fe.cameras[i].R_gt, fe.cameras[i].T_gt) for i in ids]
    est = [_pose_c2w(fe.cameras[i].R, fe.cameras[i].T) for i in ids]
    stationary = ate_sim3(gt, [est[0]] * len(ids))[0]
    return slam, res, est, stationary


# Measured on MI355X with the seeding noise seeded 0, 1, 2: (ATE RMSE after the Sim(3) fit in metres, mean PSNR in dB). Every run: no reset,
# keyframes 0, 5, 10, 15, both halves initialised, ~1250 Gaussians; the stationary trajectory (the first pose for every frame) scores 0.03378 m.
MEASURED = ((0.015644, 18.866), (0.015787, 19.038), (0.012011, 19.076))
ATE_BAR = 1.5 * max(a for a, _ in MEASURED)            # the worst of the three plus one half of it: 0.02368 m
PSNR_BAR = min(p for _, p in MEASURED) - 1.0           # the worst of the three minus 1 dB: 17.866 dB


def test_monocular_run_on_the_synthetic_sequence():
    slam, res, est, stationary = run_monocular_sequence(0)
    fe, be = slam.frontend, slam.backend
    print({k: res[k] for k in ("frames", "keyframes", "gaussians", "ate_rmse", "sensor_type", "resets")}, res["before_opt"], "stationary", stationary)
    assert res["frames"] == RUN_FRAMES and res["sensor_type"] == "monocular"
    assert fe.initialized and be.initialized
    assert all(np.isfinite(p).all() for p in est)
    assert res["gaussians"] > 0
    assert res["resets"] <= RUN_FRAMES // slam.config["Training"]["window_size"]
    assert res["before_opt"]["l1_depth"] is None and math.isfinite(res["before_opt"]["mean_psnr"])
    assert res["ate_rmse"] < stationary, (res["ate_rmse"], stationary)
    assert res["ate_rmse"] < ATE_BAR, res
    assert res["before_opt"]["mean_psnr"] > PSNR_BAR, res


@pytest.mark.parametrize("cause", ["overlap", "no_valid_depth"])
def test_monocular_run_starts_over_after_a_failed_initialisation(cause, monkeypatch):
    """Both ways an initialisation fails, forced once at the first keyframe: a window entry evicted before the map is initialised (a test
    double of add_to_window), and a keyframe rendering without a single valid depth (the opacity withheld from the kernel). The next frame
    re-initialises the map -- the back-end drops every Gaussian of the old one -- and the run goes on: a later keyframe is seeded and mapped."""
    import slam.frontend as frontend_module
    slam, ds = _mono_slam(13, 160, 120)
    fe = slam.frontend
    fired = []
    if cause == "overlap":
        real = fe.add_to_window

        def add_to_window(cur, visibility, occ, window):
            new_window, removed = real(cur, visibility, occ, window)
            if not fired:
                fired.append(cur)
                return [cur] + list(window[:-1]), window[-1]
            return new_window, removed
        fe.add_to_window = add_to_window
    else:
        real = frontend_module.kf.mono_keyframe_depth

        def mono_keyframe_depth(depth, opacity, gt_image, threshold, noise):
            if not fired:
                fired.append(fe.kf_indices[-1])
                opacity = torch.zeros_like(opacity)
            return real(depth, opacity, gt_image, threshold, noise)
        monkeypatch.setattr(frontend_module.kf, "mono_keyframe_depth", mono_keyframe_depth)
    res = slam.run()
    print({k: res[k] for k in ("frames", "keyframes", "gaussians", "resets")}, fe.log)
    assert fired and res["resets"] == 1 and len([e for e in fe.log if e[0] == "reset"]) == 1
    restart = fired[0] + 1                                             # the frame after the failed keyframe
    assert res["frames"] == 13 and res["keyframes"][0] == restart and len(res["keyframes"]) >= 2 and fe.current_window[-1] == restart
    assert res["gaussians"] > 0 and bool((slam.gaussians.unique_kfIDs >= restart).all())
    assert all(bool(torch.isfinite(c.R).all()) and bool(torch.isfinite(c.T).all()) for c in fe.cameras.values())
    assert [e[0] for e in fe.log][0] == "reset" and "keyframe" in [e[0] for e in fe.log][1:]
    assert math.isfinite(res["ate_rmse"]) and math.isfinite(res["before_opt"]["mean_psnr"])
