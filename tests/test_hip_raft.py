"""The RAFT optical-flow estimator (slam/optical_flow.py) and its HIP kernels (include/optical_flow.h): the correlation pyramid against an
fp64 product, the lookup against grid_sample, the convex upsampling against a torch restatement, the whole network with the recipe
weights against the reference's own RAFT (tests/golden/golden_raft.npz, tests/golden/make_golden_raft.py), the encoder cache, the
capture guard, and the flow term of a dynamic run on a recorded sequence."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ---- torch restatements of the three kernels ---------------------------------------------------------------------------------------
def pyramid_fp64(f1, f2):
    """RAFT/corr.py CorrBlock.corr + avg_pool2d, in fp64: the 1->2 pyramid [N, h_l, w_l] per level."""
    D, h, w = f1.shape
    c = (f1.double().reshape(D, -1).t() @ f2.double().reshape(D, -1)) / np.sqrt(D)
    c = c.reshape(h * w, 1, h, w)
    out = [c[:, 0]]
    for _ in range(3):
        c = F.avg_pool2d(c, 2, stride=2)
        out.append(c[:, 0])
    return out


def lookup_ref(levels, coords, r=4):
    """CorrBlock.__call__ with bilinear_sampler (grid_sample, align_corners=True, zeros) for one direction: levels [N, h_l, w_l], coords
    [2, h, w] -> [324, h, w]."""
    _, h, w = coords.shape
    c = coords.permute(1, 2, 0).reshape(h * w, 1, 1, 2)
    d = torch.linspace(-r, r, 2 * r + 1, device=coords.device)
    delta = torch.stack(torch.meshgrid(d, d, indexing="ij"), -1).view(1, 2 * r + 1, 2 * r + 1, 2)
    out = []
    for lvl, vol in enumerate(levels):
        pts = c / 2 ** lvl + delta
        H, W = vol.shape[-2:]
        x, y = pts.split([1, 1], -1)
        grid = torch.cat([2 * x / (W - 1) - 1, 2 * y / (H - 1) - 1], -1)
        out.append(F.grid_sample(vol[:, None], grid, align_corners=True).reshape(h * w, -1))
    return torch.cat(out, -1).t().reshape(-1, h, w)


def upsample_ref(flow, mask, pad, H, W, ndc):
    """RAFT.upsample_flow + InputPadder.unpad + camera_utils' / (W, H) * 2 for one [2, h, w] flow -> [H, W, 2]."""
    _, h, w = flow.shape
    m = torch.softmax(mask.view(1, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow[None], [3, 3], padding=1).view(1, 2, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(2, 8 * h, 8 * w)
    up = up[:, pad[2]:8 * h - pad[3], pad[0]:8 * w - pad[1]].permute(1, 2, 0)
    if ndc:
        up = up / torch.tensor([W, H], dtype=torch.float32, device=up.device) * 2
    return up


def _fmaps(D, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(D, h, w, generator=g).to(DEV), torch.randn(D, h, w, generator=g).to(DEV))


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(60, 80), (17, 22), (15, 20)])
def test_corr_pyramid_against_fp64(h, w):
    from slam.optical_flow import corr_pyramid
    f1, f2 = _fmaps(256, h, w, seed=h * w)
    both = corr_pyramid(f1, f2, both=True)
    one = corr_pyramid(f1, f2, both=False)
    r12, r21 = pyramid_fp64(f1, f2), pyramid_fp64(f2, f1)
    for lvl in range(4):
        for got, ref in ((both[lvl][0], r12[lvl]), (both[lvl][1], r21[lvl])):
            assert tuple(got.shape) == tuple(ref.shape), (lvl, tuple(got.shape), tuple(ref.shape))
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            assert err <= 1e-5, (h, w, lvl, err)
        assert torch.equal(one[lvl][0], both[lvl][0]), lvl                          # a pair call writes the single-direction bits
    N = h * w
    assert torch.equal(both[0][0].reshape(N, N).t(), both[0][1].reshape(N, N))     # level 0: 2->1 is 1->2 transposed, bit for bit


def test_corr_lookup_against_grid_sample():
    from slam.optical_flow import corr_lookup, corr_pyramid
    h, w = 17, 22
    f1, f2 = _fmaps(256, h, w, seed=3)
    levels = corr_pyramid(f1, f2, both=True)
    g = torch.Generator().manual_seed(4)
    ys, xs = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    base = torch.stack([xs, ys])
    coords = torch.stack([base + torch.randn(2, h, w, generator=g) * 3,      # fractional, some outside the coarse levels
                          base.clone()]).contiguous()                         # exact integers
    coords[1, :, :3, :3] = torch.tensor([-7.5, -30.0])[:, None, None]        # partly / fully outside every level
    coords[1, :, -2:, -2:] = torch.tensor([w + 40.0, h + 0.25])[:, None, None]
    coords[0, 0, 0, :4] = torch.tensor([-4.0, -4.5, w + 3.0, w + 3.5])
    coords = coords.to(DEV)
    got = corr_lookup(levels, coords)
    assert tuple(got.shape) == (2, 324, h, w)
    errs = [float((got[b] - lookup_ref([t[b] for t in levels], coords[b])).abs().max()) for b in range(2)]
    print("lookup max abs error (fractional, integer coordinates)", errs)
    # the kernel and torch may round a sample coordinate near 20 a unit in the last place (1.9e-6) apart, which moves a bilinear weight
    # by as much and a sample of these volumes (|C| < 6) by ~1e-5 at most
    assert max(errs) <= 1.5e-5, errs
    # the channel order: channel 81 l + 9 a + c samples x + (a - 4), y + (c - 4); at integer coordinates level 0 reads the volume's cell
    # (to the coordinate round trip's rounding; neighbouring cells differ by O(1))
    p, y, x = 5 * w + 9, 5, 9
    vol = levels[0][1][p]
    for a, c in ((0, 4), (4, 0), (8, 1), (2, 7)):
        assert abs(float(got[1, 9 * a + c, y, x]) - float(vol[y + c - 4, x + a - 4])) <= 1e-4, (a, c)


def test_upsample_unpad_ndc_against_torch():
    from slam.optical_flow import pad_amounts, upsample
    H, W = 130, 170                     # pads to 136 x 176: (3, 3, 3, 3)
    pad = pad_amounts(H, W)
    h, w = (H + pad[2] + pad[3]) // 8, (W + pad[0] + pad[1]) // 8
    g = torch.Generator().manual_seed(7)
    flow = (torch.randn(2, 2, h, w, generator=g) * 3).to(DEV)
    mask = (torch.randn(2, 576, h, w, generator=g) * 2).to(DEV)
    for ndc in (True, False):
        got = upsample(flow, mask, pad, (H, W), ndc=ndc)
        assert tuple(got.shape) == (2, H, W, 2)
        for b in range(2):
            ref = upsample_ref(flow[b], mask[b], pad, H, W, ndc)
            err = float((got[b] - ref).abs().max() / ref.abs().max())
            assert err <= 2e-6, (ndc, b, err)


# ---- the network against the reference ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_raft.npz"))


@pytest.fixture(scope="module")
def estimator(golden):
    from slam.optical_flow import RaftFlow, recipe_state_dict
    return RaftFlow(recipe_state_dict(int(golden["seed"])), DEV)


def _image(u8):
    return torch.from_numpy((u8.astype(np.float64) / 255.0).astype(np.float32)).permute(2, 0, 1).contiguous().to(DEV)


def _pair_images(z, name):
    """The fixture's image pair: cut from its row-difference coded canvas as make_golden_raft.py pair_images does."""
    canvas = np.cumsum(z[f"{name}/canvas_rowdiff"], axis=1, dtype=np.uint8)
    dx, dy = (int(v) for v in z[f"{name}/shift"])
    m = 8                                     # make_golden_raft.py MARGIN
    H, W = canvas.shape[0] - 2 * m, canvas.shape[1] - 2 * m
    a = canvas[m:m + H, m:m + W]
    b = canvas[m - dy:m - dy + H, m - dx:m - dx + W].astype(np.float64) * 0.97 + 3
    return _image(a), _image(np.clip(np.rint(b), 0, 255).astype(np.uint8))


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30))


@pytest.mark.parametrize("name", ["a", "b"])
def test_estimator_against_reference_raft(golden, estimator, name):
    z = golden
    img1, img2 = _pair_images(z, name)
    H, W = img1.shape[1:]
    tr = {}
    f12, f21 = estimator.pair(img1, img2, ndc=False, trace=tr)
    t1 = {}
    estimator.pair(img1, img2, iters=1, ndc=False, trace=t1)
    for d, b, fm1, fm2, cn in (("12", 0, "fmap_i", "fmap_j", ("net_i", "inp_i")), ("21", 1, "fmap_j", "fmap_i", ("net_j", "inp_j"))):
        s = f"{name}/{d}"
        for tag, t in (("fmap1", tr[fm1]), ("fmap2", tr[fm2])):
            flat = t.reshape(-1).cpu().numpy()
            assert _rel(flat[z[f"{s}/{tag}_idx"]], z[f"{s}/{tag}_val"]) <= 1e-4, (s, tag)
            sums = z[f"{s}/{tag}_sum"]
            assert abs(float(t.double().abs().sum()) - sums[1]) <= 1e-4 * sums[1], (s, tag)
        # cnet: the raw head output; net = tanh(head), inp = relu(head) -- compare through the same activations
        raw = z[f"{s}/cnet_val"]
        cnet = torch.cat([tr[cn[0]], tr[cn[1]]]).reshape(-1).cpu().numpy()[z[f"{s}/cnet_idx"]]
        split = z[f"{s}/cnet_idx"] < 128 * tr[cn[0]][0].numel()
        ref = np.where(split, np.tanh(raw), np.maximum(raw, 0))
        assert _rel(cnet, ref) <= 1e-4, s
        rows = z[f"{s}/pyr_rows"]
        for lvl in range(4):
            got = tr["pyramid"][lvl][b][rows].cpu().numpy()
            assert got.shape == z[f"{s}/pyr{lvl}"].shape and _rel(got, z[f"{s}/pyr{lvl}"]) <= 1e-4, (s, lvl)
        pix = z[f"{s}/lookup_pixels"]
        assert _rel(t1["corr1"][b].reshape(324, -1)[:, pix].cpu().numpy(), z[f"{s}/corr1"]) <= 1e-4, s
        assert _rel(t1["flow1"][b].cpu().numpy(), z[f"{s}/flow1"]) <= 1e-4, s
        assert _rel(tr["flow_low"][b].cpu().numpy(), z[f"{s}/flow20"]) <= 1e-4, s
        up = (f12 if d == "12" else f21).cpu().numpy()
        ref_up = z[f"{s}/flow_up"]
        step = int(z[f"{s}/flow_up_step"])                  # the fixture keeps every step-th row and column
        up = up[::step, ::step]
        assert up.shape == ref_up.shape
        err = float(np.abs(up - ref_up).max())
        print(s, "flow_up max abs error px", err)
        assert err <= 1e-3, (s, err)
    # NDC output: the same flow / (W, H) * 2
    n12, _ = estimator.pair(img1, img2)
    torch.testing.assert_close(n12, f12 / torch.tensor([W, H], dtype=torch.float32, device=DEV) * 2, rtol=0, atol=1e-6)


def test_estimator_deterministic_and_encodes_each_key_once(golden):
    from slam.optical_flow import RaftFlow, recipe_state_dict
    est = RaftFlow(recipe_state_dict(int(golden["seed"])), DEV)
    a, b = _pair_images(golden, "a")
    c = torch.flip(a, dims=[2]).contiguous()
    x1 = est.pair(a, b)
    x2 = est.pair(a, b)
    assert all(torch.equal(u, v) for u, v in zip(x1, x2))
    y = est.pair(a, b, key_i=0, key_j=1)
    assert all(torch.equal(u, v) for u, v in zip(x1, y))
    assert est.encoder_runs == 6
    est.pair(b, c, key_i=1, key_j=2)          # shares image 1: only image 2 is encoded
    assert est.encoder_runs == 7
    y2 = est.pair(a, b, key_i=0, key_j=1)
    assert est.encoder_runs == 7 and all(torch.equal(u, v) for u, v in zip(x1, y2))


def test_estimator_refuses_graph_capture(golden):
    from slam.optical_flow import RaftFlow, recipe_state_dict
    est = RaftFlow(recipe_state_dict(int(golden["seed"])), DEV)
    a = _pair_images(golden, "a")[0]
    est.pair(a, a, key_i="warm", key_j="warm")               # warm the allocator outside capture
    x = torch.zeros(16, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g, stream=s):
                x.add_(1)
                est.pair(a, a, key_i="warm", key_j="warm")
    torch.cuda.synchronize()


# ---- the flow term of a dynamic recorded run ---------------------------------------------------------------------------------------
def test_dynamic_tum_sequence_with_raft_flow(tmp_path, golden):
    """test_hip_recorded_slam.py's dynamic TUM-layout sequence (320 x 240, masks from files) with an estimator of recipe weights: the
    flow term runs on RAFT's flows. Random weights give meaningless flows, so no accuracy bar beyond finite results."""
    from slam.config import apply_cli_overrides, load_config
    from slam.dataset import SyntheticRGBDDataset
    from slam.optical_flow import RaftFlow, recipe_state_dict
    from slam.recorded import load_dataset, write_tum_sequence
    from slam.system import SLAM
    from test_hip_recorded_slam import _write_configs
    torch.manual_seed(0)
    src = SyntheticRGBDDataset(num_frames=30, width=320, height=240, seed=1, dynamic=True, dystart=6)
    seq = tmp_path / "data" / "dyn"
    calib = write_tum_sequence(src, str(seq), masks=True)
    cfg = apply_cli_overrides(load_config(_write_configs(tmp_path, seq, calib, {"dystart": 6})), dynamic=True)
    est = RaftFlow(recipe_state_dict(int(golden["seed"])), DEV)
    ds = load_dataset(cfg, DEV, flow=est)
    assert hasattr(ds, "gt_flow")
    slam = SLAM(cfg, ds)
    res = slam.run()
    be = slam.backend
    targets6 = dict(be.flow_targets.targets)              # the one store both bodies of BackEnd.map read (slam/keyframe_slots.FlowTargets)
    print(res, ds.flow_stats, len(targets6))
    assert ds.flow_stats["pairs"] > 0 and est.pairs == ds.flow_stats["pairs"]
    assert len(targets6) > 0                                                 # the flow term ran
    # flow_stats right after an estimate, with no synchronisation in between: it waits for the last pair itself
    ds._flow_cache.clear()
    pairs = est.pairs
    ds.gt_flow(0, 1)
    st = ds.flow_stats
    assert st["pairs"] == est.pairs == pairs + 1
    assert all(np.isfinite(st[k]) and st[k] > 0 for k in ("ms_per_pair", "ms_first", "ms_rest_mean")), st
    assert np.isfinite(res["ate_rmse"]) and np.isfinite(res["before_opt"]["mean_psnr"]), res
    # each cached target is pair() on the two keyframe images, masked by the keyframes' motion masks
    checked = 0
    fresh = RaftFlow(recipe_state_dict(int(golden["seed"])), DEV)

    def pair(u, v):           # the dataset estimates a pair in frame order
        a, b = sorted((u, v))
        fab, fba = fresh.pair(ds[a][0], ds[b][0])
        return (fab, fba) if (a, b) == (u, v) else (fba, fab)
    for (u, v), hit in list(targets6.items())[:3]:
        fuv, fvu = pair(u, v)
        m1, m2 = hit[2:3], hit[3:4]
        assert torch.equal(hit[0:2], fuv.permute(2, 0, 1) * m1) and torch.equal(hit[4:6], fvu.permute(2, 0, 1) * m2), (u, v)
        checked += 1
        # ... and the four operands the eager body hands slam_losses.masked_l1 are those planes
        t_back, w1, t_fwd, w2 = be.flow_targets.pair_operands(hit)
        assert torch.equal(t_back, (fuv.permute(2, 0, 1) * m1).contiguous()) and torch.equal(t_fwd, (fvu.permute(2, 0, 1) * m2).contiguous())
        assert torch.equal(w1, m1) and torch.equal(w2, m2) and t_back.is_contiguous() and t_fwd.is_contiguous()
    assert checked > 0
    ds.close()
    del slam, ds
    # without an estimator the term stays skipped
    torch.manual_seed(0)
    ds = load_dataset(cfg, DEV)
    assert not hasattr(ds, "gt_flow")
    slam = SLAM(cfg, ds)
    slam.run()
    assert not slam.backend.flow_targets.targets
    ds.close()
