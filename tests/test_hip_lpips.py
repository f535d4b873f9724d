"""The HIP kernels of the LPIPS metric (include/perceptual.h, csrc/gs_lpips.h) against the fp64 restatement of the published definition
(tests/lpips_reference.py): the input scaling, the distance on seeded feature tensors fed in directly (MIOpen is not in that comparison),
its exactness properties, Lpips.forward end to end on the noise ladder, and eval_rendering's mean_lpips on a short synthetic run.

Bounds: 2e-6 absolute on the scaled input (a few roundings per value of magnitude <= 2.7); 1e-5 relative on the per-tap means and scores
of the distance (what tests/test_hip_raft.py puts on fp32 sums of this length); 1e-4 relative end to end (the bound the YOLO and RAFT
tests put on an fp32 network against fp64)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import perceptual  # noqa: E402
import lpips_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NORMS = ("torchmetrics", "lpips")
RS = (1e-1, 1e-2, 1e-3, 1e-4)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lins(seed=0):
    _, lin = perceptual.recipe_state_dicts(seed)
    return [lin[f"lin{l}.model.1.weight"].reshape(-1).to(DEV).contiguous() for l in range(5)]


def _features(H, W, B, r, seed, zero_pixels=0):
    """Seeded taps of an H x W image, fed to the kernel directly: a = relu(randn + 0.5) (about a third of the values are exact zeros, as
    after a ReLU), b = a (1 + r randn); rows 0 .. B-1 hold a, rows B .. 2B-1 hold b. zero_pixels: that many pixels per tap get an all-zero
    feature vector, a third of them in a only, a third in b only, a third in both."""
    g = torch.Generator().manual_seed(seed)
    feats = []
    for c, (h, w) in zip(perceptual.CHANNELS, perceptual.tap_sizes(H, W)):
        a = torch.relu(torch.randn((B, c, h, w), generator=g) + 0.5)
        b = a * (1 + r * torch.randn((B, c, h, w), generator=g))
        if zero_pixels:
            idx = torch.randperm(h * w, generator=g)[:zero_pixels]
            ys, xs = idx // w, idx % w
            k = zero_pixels // 3
            a[:, :, ys[:2 * k], xs[:2 * k]] = 0
            b[:, :, ys[k:], xs[k:]] = 0
        feats.append(torch.cat((a, b)).to(DEV).contiguous())
    return feats


def _check_distance(feats, lins, norm, tag):
    taps, scores = perceptual.distance(feats, lins, norm)
    rtaps, rscores = ref.distance(feats, lins, norm)
    assert torch.isfinite(taps).all() and torch.isfinite(scores).all()
    et = float(((taps.double().cpu() - rtaps).abs() / rtaps).max())
    es = float(((scores.double().cpu() - rscores).abs() / rscores).max())
    print(f"{tag} {norm}: score {float(rscores[0]):.4g} rel. error taps {et:.3g} scores {es:.3g}")
    assert et <= 1e-5 and es <= 1e-5, (tag, norm, et, es)
    return taps, scores


def test_symbols_are_exported():
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    for name in ("gsr_lpips_prepare", "gsr_lpips_workspace_size", "gsr_lpips_distance"):
        assert hasattr(lib, name), name
    chw = (ctypes.c_int * 6)(64, 119, 159, 192, 59, 79)
    assert lib.gsr_lpips_workspace_size(2, 2, chw) == 4 * 2 * (-(-119 * 159 // 64) + -(-59 * 79 // 64))
    assert lib.gsr_lpips_workspace_size(0, 2, chw) == 0 and lib.gsr_lpips_workspace_size(1, 9, chw) == 0


def test_invalid_arguments_are_refused():
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    x = torch.zeros((1, 3, 80, 80), device=DEV)
    with pytest.raises(RuntimeError, match="gsr_lpips_prepare"):
        lib.gsr_lpips_prepare(0, 80, 80, x.data_ptr(), x.data_ptr(), x.data_ptr(), None)
    feats, lins = _features(77, 131, 1, 0.1, 0), _lins()
    with pytest.raises(ValueError, match="norm"):
        perceptual.distance(feats, lins, "l2")
    with pytest.raises(RuntimeError, match="contiguous float32"):
        perceptual.distance([f.double() for f in feats], lins)
    with pytest.raises(RuntimeError, match="lins"):
        perceptual.distance(feats, lins[::-1])


@pytest.mark.parametrize("B", [1, 3])
def test_prepare_against_the_restatement(B):
    g = torch.Generator().manual_seed(B)
    x, y = torch.rand((B, 3, 77, 131), generator=g), torch.rand((B, 3, 77, 131), generator=g)
    x[0, :, 0, :4], y[0, :, 0, :4] = 0.0, 1.0                                              # the ends of the range
    got = perceptual.prepare(x.to(DEV), y.to(DEV))
    want = ref.network_input(x, y)
    assert got.shape == (2 * B, 3, 77, 131)
    err = float((got.double().cpu() - want).abs().max())
    print(f"prepare B={B}: max abs error {err:.3g}, max magnitude {float(want.abs().max()):.3g}")
    assert err <= 2e-6


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", [(480, 640), (77, 131)])
def test_distance_against_the_restatement(size, B, norm):
    lins = _lins()
    for k, r in enumerate(RS):
        _check_distance(_features(size[0], size[1], B, r, seed=10 * B + k), lins, norm, f"{size[1]}x{size[0]} B={B} r={r:g}")


@pytest.mark.parametrize("norm", NORMS)
def test_all_zero_feature_vectors(norm):
    lins = _lins()
    for r in (1e-1, 1e-3):
        feats = _features(77, 131, 2, r, seed=3, zero_pixels=6)
        assert float(feats[2][:2].abs().sum(1).min()) == 0.0 and float(feats[2][2:].abs().sum(1).min()) == 0.0
        _check_distance(feats, lins, norm, f"zeros r={r:g}")


@pytest.mark.parametrize("norm", NORMS)
def test_distance_exactness(norm):
    lins = _lins()
    feats = _features(480, 640, 3, 1e-2, seed=5, zero_pixels=3)
    B = 3
    taps, scores = perceptual.distance(feats, lins, norm)
    # two runs: the same bits (a workspace of its own the second time, and a reused one the third)
    ws = {}
    for _ in range(2):
        t2, s2 = perceptual.distance(feats, lins, norm, ws)
        assert torch.equal(_bits(t2), _bits(taps)) and torch.equal(_bits(s2), _bits(scores))
    # identical inputs: exactly 0.0
    same = [torch.cat((f[:B], f[:B])).contiguous() for f in feats]
    t0, s0 = perceptual.distance(same, lins, norm)
    assert float(t0.abs().max()) == 0.0 and float(s0.abs().max()) == 0.0
    # the two images exchanged: the same bits
    swapped = [torch.cat((f[B:], f[:B])).contiguous() for f in feats]
    ts, ss = perceptual.distance(swapped, lins, norm)
    assert torch.equal(_bits(ts), _bits(taps)) and torch.equal(_bits(ss), _bits(scores))
    # B = 3 in one call: the three pairs in three calls, bit for bit
    for b in range(B):
        one = [torch.cat((f[b:b + 1], f[B + b:B + b + 1])).contiguous() for f in feats]
        t1, s1 = perceptual.distance(one, lins, norm)
        assert torch.equal(_bits(t1[0]), _bits(taps[b])) and torch.equal(_bits(s1), _bits(scores[b:b + 1]))


@pytest.mark.parametrize("norm", NORMS)
def test_forward_end_to_end_on_the_ladder(norm):
    alex, lin = perceptual.recipe_state_dicts(0)
    m = perceptual.Lpips(alex, lin, DEV, norm)
    base, noisy = ref.ladder(480, 640, seed=0)
    want = ref.lpips(alex, lin, torch.cat(noisy), base.expand(3, -1, -1, -1), norm)
    x, y = torch.cat(noisy).to(DEV), base.expand(3, -1, -1, -1).contiguous().to(DEV)
    m(x, y)                                                                                # warm-up: MIOpen picks its algorithms
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                                # forward never waits for the device
    try:
        got, taps = m.forward(x, y, taps=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert got.shape == (3,) and got.is_cuda and taps.shape == (3, 5)
    for k in range(3):
        rel = abs(float(got[k]) - float(want[k])) / float(want[k])
        print(f"ladder rung {k} {norm}: device {float(got[k]):.9g} fp64 {float(want[k]):.9g} rel {rel:.3g}")
    assert float(want[0]) > float(want[1]) > float(want[2]) > 0
    assert float(((got.double().cpu() - want).abs() / want).max()) <= 1e-4
    again = m(x, y)
    assert torch.equal(_bits(again), _bits(got))                                           # the same bits on every call
    single = m(x[1:2], y[1:2])
    assert abs(float(single[0]) - float(want[1])) <= 1e-4 * float(want[1])
    st = m.stats
    assert st["pairs"] == 10 and st["calls"] == 4 and st["ms_per_pair"] > 0
    with pytest.raises(ValueError, match="at least 67"):
        m(x[:, :, :60], y[:, :, :60])
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(graph, stream=s):
                m(x, y)


def test_eval_rendering_reports_mean_lpips(tmp_path):
    from gaussian_renderer import render
    from slam.dataset import SyntheticRGBDDataset
    from slam.eval_utils import eval_rendering
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=8, width=320, height=240, seed=0)
    cfg = merge_config(default_config(), {"Training": {"init_itr_num": 120, "init_gaussian_update": 100, "init_gaussian_reset": 120,
                                                       "tracking_itr_num": 12, "static_map_iters": 10, "gaussian_update_every": 60,
                                                       "gaussian_update_offset": 20, "kf_interval": 4},
                                          "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8}, "opt_params": {"densify_from_iter": 100}})
    m = perceptual.Lpips(*perceptual.recipe_state_dicts(0), DEV)
    slam = SLAM(cfg, ds, save_dir=str(tmp_path), lpips=m)
    res = slam.run()
    assert list(res["before_opt"]) == ["mean_psnr", "mean_ssim", "mean_lpips", "l1_depth", "frames"]
    saved = json.load(open(os.path.join(str(tmp_path), "psnr", "before_opt", "final_result.json")))
    assert saved == res["before_opt"] and 0 < saved["mean_lpips"] < 2
    frames = slam.frontend.cameras
    call = lambda lp: eval_rendering(frames, slam.gaussians, ds, None, slam.pipeline_params, slam.background, slam.frontend.kf_indices, lpips=lp)
    plain, plain2 = call(None), call(None)
    assert list(plain) == ["mean_psnr", "mean_ssim", "l1_depth", "frames"]                # exactly today's keys
    assert plain == plain2                                                                 # floats compare by value: the same bits
    with_lpips = call(m)
    assert {k: v for k, v in with_lpips.items() if k != "mean_lpips"} == plain           # every other key unchanged
    assert with_lpips["mean_lpips"] == res["before_opt"]["mean_lpips"]
    per_frame = []
    for idx in range(0, len(frames) - 1):
        image = torch.clamp(render(frames[idx], slam.gaussians, slam.pipeline_params, slam.background, dynamic=False, dx=0, ds=0, dr=0)["render"], 0, 1)
        per_frame.append(float(m(image[None], ds[idx][0][None])[0]))
    assert with_lpips["frames"] == len(per_frame) == 7
    assert abs(with_lpips["mean_lpips"] - float(np.mean(per_frame))) <= 1e-6 * float(np.mean(per_frame))
