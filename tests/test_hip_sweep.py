"""gsr_sweep_depth (include/multiview_depth.h, csrc/gs_sweep.h) against its numpy restatement (tests/sweep_reference.py): the cost volume C,
the aggregated volume S, index16 and the bits of the depth are equal, on the planted scene with one to three partners, under a general
pose with four (the float path), at sizes that are no multiple of the pixels per block or smaller than the census window, and where every
hypothesis is invisible or every pixel unobservable; then the refusals, the PlaneSweep object and two short monocular runs."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sweep_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
            @ np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def _pose(rot, t):
    return np.concatenate([_rotation(*rot), np.asarray(t, np.float64)[:, None]], 1).astype(np.float32).reshape(12)


def _planted(names, **over):
    def make():
        grey, partners, transforms, _ = ref.planted_scene(names, seed=0)
        return grey, partners, ref.PLANTED_K, transforms, dict(w_min=ref.PLANTED_W_MIN, w_step=ref.PLANTED_W_STEP, **over)
    return make


def _random(H, W, J, seed, K, poses, w_min=0.0, w_step=1.0 / 32.0, **over):
    """Random bytes, the partners partly copies of the reference moved by a few pixels, so that some costs are low."""
    def make():
        rng = np.random.default_rng(seed)
        grey = rng.integers(0, 256, (H, W), dtype=np.uint8)
        partners = rng.integers(0, 256, (J, H, W), dtype=np.uint8)
        for j in range(J):
            s = min(2 + j, W - 1)
            if W > s:
                partners[j, :, :W - s] = np.where(rng.random((H, W - s)) < 0.7, grey[:, s:], partners[j, :, :W - s])
        return grey, partners, K, np.stack(poses[:J]), dict(w_min=w_min, w_step=w_step, **over)
    return make


def _plane(H, W, J, seed, K, poses, depth, w_min=0.0, w_step=1.0 / 32.0, **over):
    """A textured fronto-parallel plane at `depth` in front of the reference camera, seen by every partner through the homography its pose
    induces (bilinear taps of the texture), plus noise: the sweep has something to find under a general pose."""
    def make():
        rng = np.random.default_rng(seed)
        m = 40
        tex = ref._texture(rng, H + 2 * m, W + 2 * m)
        fx, fy, cx, cy = K
        Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)

        def tap(x, y):
            x, y = np.clip(x + m, 0, W + 2 * m - 1.001), np.clip(y + m, 0, H + 2 * m - 1.001)
            x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
            ax, ay = x - x0, y - y0
            return ((1 - ax) * (1 - ay) * tex[y0, x0] + ax * (1 - ay) * tex[y0, x0 + 1] + (1 - ax) * ay * tex[y0 + 1, x0] + ax * ay * tex[y0 + 1, x0 + 1])
        to_u8 = lambda a: np.clip(np.rint(a + rng.normal(0.0, 2.0, a.shape)), 0, 255).astype(np.uint8)
        grey = to_u8(tap(xs, ys))
        partners = []
        for T in poses[:J]:
            T = np.asarray(T, np.float64).reshape(3, 4)
            Hm = Km @ (T[:, :3] + T[:, 3:] @ np.array([[0.0, 0.0, 1.0 / depth]])) @ np.linalg.inv(Km)      # reference pixel -> partner pixel
            back = np.linalg.inv(Hm) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H * W)])
            partners.append(to_u8(tap((back[0] / back[2]).reshape(H, W), (back[1] / back[2]).reshape(H, W))))
        return grey, np.stack(partners), K, np.stack(poses[:J]), dict(w_min=w_min, w_step=w_step, **over)
    return make


GENERAL = [_pose((0.02, -0.03, 0.015), (-0.16, 0.01, 0.03)), _pose((-0.015, 0.02, -0.03), (0.02, -0.14, -0.02)),
           _pose((0.03, 0.025, 0.02), (0.12, 0.05, 0.06)), _pose((-0.01, -0.02, 0.04), (-0.07, 0.11, -0.04))]
SIDEWAYS = [ref.planted_transform("right"), ref.planted_transform("down"), ref.planted_transform("left")]
BEHIND = [_pose((0.0, np.pi, 0.0), (0.1, 0.0, -0.5)), _pose((0.0, np.pi, 0.0), (0.0, 0.1, -1.0))]     # turned round: X_2 < 0 for every ray

# name -> the case: (reference bytes, partner bytes, K, transforms, parameters over DEFAULTS); every name is one parametrised case
CASES = {
    "planted_J1": _planted(("right",)),
    "planted_J2": _planted(("right", "down")),
    "planted_J3": _planted(("right", "down", "left")),
    "general_pose_J4_40x72": _plane(40, 72, 4, 1, (61.3, 60.2, 35.7, 19.4), GENERAL, 1.9, w_step=0.021),
    "65x33_not_a_multiple_of_the_block": _plane(65, 33, 2, 2, (40.0, 41.0, 16.2, 32.1), GENERAL, 1.6, w_step=0.03, uniqueness_ratio=15),
    "random_bytes_J4_23x41": _random(23, 41, 4, 7, (35.0, 36.0, 20.3, 11.2), GENERAL, w_step=0.025, uniqueness_ratio=5),
    "7x9_below_the_census_window": _random(7, 9, 2, 3, (9.0, 9.0, 4.0, 3.0), SIDEWAYS, w_step=0.05, min_span_px=1),
    "one_pixel": _random(1, 1, 1, 4, (1.0, 1.0, 0.0, 0.0), SIDEWAYS, min_span_px=0),
    "w_min_positive": _plane(33, 50, 3, 5, (50.0, 50.0, 24.5, 16.0), GENERAL, 1.6, w_min=0.11, w_step=0.017),
    "partners_behind_the_camera": _random(20, 37, 2, 6, (30.0, 30.0, 18.0, 9.5), BEHIND),
    "span_never_reached": _planted(("right", "down"), min_span_px=32),
    "p1_1_p2_2047_uniqueness_0": _planted(("right", "down"), p1=1, p2=2047, uniqueness_ratio=0),
    "uniqueness_99_span_0": _planted(("right", "down"), uniqueness_ratio=99, min_span_px=0),
}
_reference = {}


def _expected(name):
    """(inputs, parameters, the restatement's result) of a case: computed once, shared, read-only."""
    if name not in _reference:
        grey, partners, K, transforms, over = CASES[name]()
        params = dict(ref.DEFAULTS, **over)
        want = ref.sweep(grey, partners, K, transforms, **params)
        for a in (grey, partners, transforms, *want.values()):
            a.setflags(write=False)
        _reference[name] = ((grey, partners, K, transforms), params, want)
    return _reference[name]


def _run(inputs, params, cost=True, cost_sum=True, **extra):
    from slam import sweep
    grey, partners, K, transforms = inputs
    H, W = grey.shape
    dev = torch.device(DEV)
    out = {"index16": torch.full((H, W), 1234, dtype=torch.int16, device=dev), "depth": torch.full((H, W), -7.0, dtype=torch.float32, device=dev)}
    if cost:
        out["cost"] = torch.full((H, W, 64), 201, dtype=torch.uint8, device=dev)
    if cost_sum:
        out["cost_sum"] = torch.full((H, W, 64), -1, dtype=torch.int16, device=dev)
    sweep.sweep_depth(torch.tensor(np.array(grey), device=dev), torch.tensor(np.array(partners), device=dev), K,
                      torch.tensor(np.array(transforms), device=dev), **out, **params, **extra)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if cost_sum:
        res["cost_sum"] = res["cost_sum"].view(np.uint16)
    return res


def _assert_equal(got, want, name, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(bad[0])
        raise AssertionError(f"{name}: {what} differs at {len(bad)} of {want.size} entries, first at {first}: {got[first]} != {want[first]}; "
                             f"rows {np.unique(bad[:, 0])[:8]}, columns {np.unique(bad[:, 1])[:8]}")


@pytest.mark.parametrize("name", list(CASES))
def test_volumes_index_and_depth_equal_the_reference(name):
    inputs, params, want = _expected(name)
    got = _run(inputs, params)
    _assert_equal(got["cost"], want["cost"], name, "C")                          # the projection and the census ...
    _assert_equal(got["cost_sum"], want["cost_sum"], name, "S")                  # ... the aggregation ...
    _assert_equal(got["index16"], want["index16"], name, "index16")              # ... the selection ...
    _assert_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32), name, "the bits of depth")
    print(name, "valid share", float((want["index16"] >= 0).mean()), "observable", float(want["observable"].mean()), "C max", int(want["cost"].max()),
          "S max", int(want["cost_sum"].max()))


def test_the_cases_reach_what_they_are_there_for():
    """The restatement's side of the edge cases (no device work): invisible partners cost 62 each and leave nothing valid, a span that is
    never reached leaves nothing valid, and the general poses leave pixels valid, invalid, visible and invisible alike."""
    _, _, behind = _expected("partners_behind_the_camera")
    assert (behind["cost"] == 62 * 2).all() and (behind["index16"] == -16).all() and not behind["observable"].any() and not behind["depth"].any()
    _, _, span = _expected("span_never_reached")
    assert not span["observable"].any() and (span["index16"] == -16).all() and (span["cost"] < 124).any()
    for name in ("general_pose_J4_40x72", "w_min_positive", "65x33_not_a_multiple_of_the_block"):
        want = _expected(name)[2]
        valid = want["index16"] >= 0
        assert 0.02 < valid.mean() < 0.98 and 0.05 < want["observable"].mean() and (want["cost"] % 62 != 0).any(), name
    assert (_expected("planted_J3")[2]["cost"] > 124).any()
    for name in ("random_bytes_J4_23x41", "w_min_positive"):                  # the span falls on both sides of min_span_px within one image
        assert 0.5 < _expected(name)[2]["observable"].mean() < 0.95, name


def test_optional_outputs_and_repeatability():
    inputs, params, want = _expected("planted_J2")
    bare = _run(inputs, params, cost=False, cost_sum=False)
    assert np.array_equal(bare["index16"], want["index16"]) and np.array_equal(bare["depth"].view(np.uint32), want["depth"].view(np.uint32))
    one = _run(inputs, params, cost=True, cost_sum=False)
    assert np.array_equal(one["index16"], want["index16"]) and np.array_equal(one["cost"], want["cost"])
    a, b = _run(inputs, params), _run(inputs, params)
    for k in ("index16", "depth", "cost", "cost_sum"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_sweep_object_keeps_its_workspace_and_forms_its_inputs():
    from slam import sweep
    inputs, params, want = _expected("planted_J2")
    grey, partners, K, transforms = inputs
    s = sweep.PlaneSweep(device=DEV, **{k: params[k] for k in ref.DEFAULTS})
    # float frames whose grey bytes are the planted bytes: all three channels equal b / 255
    frame = lambda b: torch.tensor(np.broadcast_to(np.asarray(b, np.float32) / np.float32(255.0), (3,) + b.shape).copy(), device=DEV)
    ref_image, partner_images = frame(grey), torch.stack([frame(p) for p in partners])
    assert np.array_equal(sweep.grey_bytes(ref_image).cpu().numpy(), grey) and sweep.grey_bytes(partner_images).shape == partners.shape
    t = torch.tensor(np.array(transforms), device=DEV)
    ws = None
    for _ in range(2):
        out = s.sweep(ref_image, partner_images, K, t, ref.PLANTED_W_MIN, ref.PLANTED_W_STEP)
        assert np.array_equal(out["index16"].cpu().numpy(), want["index16"]) and np.array_equal(out["valid"].cpu().numpy(), want["index16"] >= 0)
        assert np.array_equal(out["depth"].cpu().numpy().view(np.uint32), want["depth"].view(np.uint32))
        assert ws in (None, s.workspace(112, 48, 2).data_ptr())
        ws = s.workspace(112, 48, 2).data_ptr()
    assert list(s._workspaces) == [(112, 48, 2)] and s.workspace(112, 48, 2).numel() == sweep.sweep_workspace_size(112, 48, 2) > 48 * 112 * 64 * 3
    assert sweep.sweep_workspace_size(112, 48, 5) == 0 and sweep.sweep_workspace_size(112, 48, 0) == 0 and sweep.sweep_workspace_size(0, 48, 1) == 0
    assert sweep.sweep_workspace_size(8192, 4095, 1) > 0 and sweep.sweep_workspace_size(8192, 4096, 1) == 0          # width * height * 64 < 2^31
    with pytest.raises(ValueError, match="1 to 4 partners"):
        s.workspace(112, 48, 5)
    # the transforms from cameras that hold world-to-camera R and T on the device
    import types
    cam = lambda rot, t: types.SimpleNamespace(R=torch.tensor(_rotation(*rot), dtype=torch.float32, device=DEV), T=torch.tensor(t, dtype=torch.float32, device=DEV))
    a, b = cam((0.1, -0.2, 0.05), (0.3, -0.1, 0.2)), cam((-0.05, 0.1, 0.2), (0.0, 0.4, -0.3))
    got = sweep.relative_transforms(a, [b, a]).cpu().numpy().astype(np.float64).reshape(2, 3, 4)
    x_world = np.array([0.7, -0.4, 2.0])
    x_a, x_b = (c.R.cpu().numpy().astype(np.float64) @ x_world + c.T.cpu().numpy() for c in (a, b))
    np.testing.assert_allclose(got[0, :, :3] @ x_a + got[0, :, 3], x_b, atol=1e-6)
    np.testing.assert_allclose(got[1], np.eye(3, 4), atol=1e-6)


def test_bad_arguments_are_refused_with_text_and_touch_nothing():
    from slam import sweep
    (grey, partners, K, transforms), params, want = _expected("65x33_not_a_multiple_of_the_block")
    H, W = grey.shape
    dev = torch.device(DEV)
    g, p, t = (torch.tensor(np.array(a), device=dev) for a in (grey, partners, transforms))
    index16 = torch.full((H, W), 1234, dtype=torch.int16, device=dev)
    depth = torch.full((H, W), -7.0, dtype=torch.float32, device=dev)
    cost = torch.full((H, W, 64), 201, dtype=torch.uint8, device=dev)
    cost_sum = torch.full((H, W, 64), -1, dtype=torch.int16, device=dev)
    need = sweep.sweep_workspace_size(W, H, 2)
    short = torch.empty(need - 1, dtype=torch.uint8, device=dev)
    five = torch.zeros((5, H, W), dtype=torch.uint8, device=dev)
    bad = [({"p1": 120, "p2": 120}, "0 < p1 < p2 <= 2047"),
           ({"p1": 0}, "0 < p1 < p2 <= 2047"),
           ({"p2": 2048}, "0 < p1 < p2 <= 2047"),
           ({"uniqueness_ratio": 100}, "uniqueness_ratio must be in \\[0, 99\\]"),
           ({"uniqueness_ratio": -1}, "uniqueness_ratio must be in \\[0, 99\\]"),
           ({"min_span_px": -1}, "min_span_px must not be negative"),
           ({"w_min": -0.1}, "w_min must be finite and >= 0 and w_step finite and > 0"),
           ({"w_min": float("inf")}, "w_min must be finite and >= 0 and w_step finite and > 0"),
           ({"w_step": 0.0}, "w_min must be finite and >= 0 and w_step finite and > 0"),
           ({"w_step": float("nan")}, "w_min must be finite and >= 0 and w_step finite and > 0"),
           ({"partner_grey": five, "transforms": torch.zeros((5, 12), device=dev)}, "partners in \\[1, 4\\] \\(got 5\\)"),
           ({"index16": None}, "index16, depth and workspace must not be NULL"),
           ({"depth": None}, "index16, depth and workspace must not be NULL"),
           ({"transforms": None}, "index16, depth and workspace must not be NULL"),
           ({"workspace": short}, f"hold {need} bytes \\(gsr_sweep_workspace_size\\), got {need - 1}")]
    for over, text in bad:
        kw = dict(ref_grey=g, partner_grey=p, K=K, transforms=t, index16=index16, depth=depth, cost=cost, cost_sum=cost_sum, **params)
        kw.update(over)
        with pytest.raises(RuntimeError, match="gsr_sweep_depth failed \\(code -1\\): gsr_sweep_depth: .*" + text):
            sweep.sweep_depth(**kw)
    torch.cuda.synchronize()
    assert bool((index16 == 1234).all()) and bool((depth == -7.0).all()) and bool((cost == 201).all()) and bool((cost_sum == -1).all())
    with pytest.raises(RuntimeError, match="partner_grey must be a contiguous torch.uint8 device tensor of shape \\(2, 65, 33\\)"):
        sweep.sweep_depth(g, p[:, :, :20], K, t, 0.0, 0.03, index16, depth)
    with pytest.raises(RuntimeError, match="transforms must be a contiguous float32 device tensor of shape \\(2, 12\\)"):
        sweep.sweep_depth(g, p, K, t[:1], 0.0, 0.03, index16, depth)
    sweep.sweep_depth(g, p, K, t, index16=index16, depth=depth, workspace=torch.empty(need, dtype=torch.uint8, device=dev), **params)      # exactly enough
    torch.cuda.synchronize()
    assert np.array_equal(index16.cpu().numpy(), want["index16"])


# ---- end to end: two short monocular runs ---------------------------------------------------------------------------------------------
def _mono_run(training_addition):
    """12 frames at 160x120 with the sensor depth withheld, window 4, a keyframe every second frame at the earliest; the seeding noise is
    seeded. `training_addition` is merged into Training."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=12, width=160, height=120, seed=0, sensor_depth=False)
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 2, "window_size": 4}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"sensor_type": "monocular", "pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 100}})
    cfg = merge_config(cfg, {"Training": training_addition})
    slam = SLAM(cfg, ds)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    res = slam.run()
    g = slam.gaussians
    tensors = [x.detach().clone() for x in (g.get_xyz, g._features_dc, g._scaling, g._rotation, g._opacity)]
    return res, tensors


def test_monocular_run_with_the_sweep_on():
    res, tensors = _mono_run({"mono_sweep": {"enabled": True}})
    print({k: res[k] for k in ("frames", "keyframes", "gaussians", "ate_rmse", "resets", "sweep")}, res["before_opt"])
    assert res["frames"] == 12 and res["gaussians"] > 0 and all(bool(torch.isfinite(x).all()) for x in tensors)
    assert res["sweep"]["keyframes"] >= 1 and res["sweep"]["valid_share"] > 0.0 and res["sweep"]["device_ms_per_keyframe"] > 0.0


def test_monocular_run_without_the_option_is_the_untouched_path():
    absent, a = _mono_run({})                                                   # an explicitly empty addition: the configuration as it always was
    disabled, b = _mono_run({"mono_sweep": {"enabled": False}})
    print({k: absent[k] for k in ("frames", "keyframes", "gaussians", "ate_rmse", "resets")}, absent["before_opt"])
    assert "sweep" not in absent and "sweep" not in disabled and absent["keyframes"] == disabled["keyframes"]
    assert len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))
