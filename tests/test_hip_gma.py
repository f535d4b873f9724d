"""The GMA optical-flow estimator (slam/optical_flow.py GmaFlow) and its two HIP kernels (include/optical_flow.h gsr_gma_attention,
gsr_gma_aggregate): each kernel against fp64 with a bar of four times the error of the reference's own fp32 torch expression,
reproducibility, batch equivalence and error codes; the whole network with the stand-in weights against the reference's own RAFTGMA
(tests/golden/golden_gma.npz, tests/golden/make_golden_gma.py), the encoder cache, the capture guard, and a dataset with a GmaFlow."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (h, w, dim): full tiles at the smallest size RAFT admits; N = 374, ragged in both tile directions; N = 1320, rows longer than a
# 1024-thread block; a dim that leaves a tail in the 16-row channel staging. Batch 2 throughout.
SHAPES = [(16, 16, 128), (17, 22, 128), (33, 40, 128), (17, 22, 132)]
GAMMA = 0.8


# ---- inputs and references, computed once on the CPU ---------------------------------------------------------------------------------
def _attention_refs(q, k, scale):
    """fp64 attention, and the reference's own fp32 expression (GMA/gma.py Attention.forward: scale * q, einsum, softmax)."""
    ref = torch.softmax(torch.einsum("bci,bcj->bij", scale * q.double().flatten(2), k.double().flatten(2)), -1)
    t32 = torch.softmax(torch.einsum("bci,bcj->bij", scale * q.flatten(2), k.flatten(2)), -1)
    return ref, t32


def _make_case(h, w, dim, large_logits=False):
    """Seeded q, k [2, dim, h, w] with logits of standard deviation 2 (randn * sqrt(2) each: dim^-1/2 sum_c q k has variance 4), which
    puts the mean row entropy near log N - 2; v and x for the aggregation."""
    g = torch.Generator().manual_seed(1000 * h + w + dim)
    q, k = (torch.randn(2, dim, h, w, generator=g) * 2.0 ** 0.5 for _ in range(2))
    v, x = (torch.randn(2, dim, h, w, generator=g) for _ in range(2))
    scale = float(dim) ** -0.5
    if large_logits:             # constant columns: row 5 of batch 0 has the logit +80 at column 7 and -80 at column 11
        a = (80.0 / dim ** 0.5) ** 0.5
        q[0].flatten(1)[:, 5] = a
        k[0].flatten(1)[:, 7] = a
        k[0].flatten(1)[:, 11] = -a
    ref, t32 = _attention_refs(q, k, scale)
    return {"q": q, "k": k, "v": v, "x": x, "scale": scale, "ref": ref, "torch_err": float((t32.double() - ref).abs().max())}


_cases = {}


def _case(h, w, dim, large_logits=False):
    key = (h, w, dim, large_logits)
    if key not in _cases:
        _cases[key] = _make_case(*key)
    return _cases[key]


def _entropy_ratio(attn64):
    n = attn64.shape[-1]
    return float((-(attn64 * torch.log(attn64.clamp_min(1e-300))).sum(-1)).mean() / np.log(n))


def _attention(c):
    from slam.optical_flow import gma_attention
    return gma_attention(c["q"].to(DEV), c["k"].to(DEV), c["scale"])


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,dim", SHAPES)
def test_attention_against_fp64(h, w, dim):
    c = _case(h, w, dim)
    for b in range(2):
        assert 0.3 <= _entropy_ratio(c["ref"][b]) <= 0.8, (b, _entropy_ratio(c["ref"][b]))      # peaked, not one-hot
    got = _attention(c)
    assert tuple(got.shape) == (2, h * w, h * w) and got.dtype == torch.float32
    got = got.cpu().double()
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-5
    err = float((got - c["ref"]).abs().max())
    print(f"attention {h}x{w} dim {dim}: kernel error {err:.3e}, fp32 torch error {c['torch_err']:.3e}")
    assert err <= 4 * c["torch_err"], (err, c["torch_err"])


def test_attention_with_large_logits_is_finite():
    c = _case(17, 22, 128, True)
    assert abs(float(c["ref"][0, 5, 7]) - 1) < 1e-6 and float(c["ref"][0, 5, 11]) < 1e-60      # logits +80 and -80 in the row
    got = _attention(c).cpu().double()
    assert bool(torch.isfinite(got).all())
    assert float((got.sum(-1) - 1).abs().max()) <= 1e-5
    err = float((got - c["ref"]).abs().max())
    print(f"attention with logits of +-80: kernel error {err:.3e}, fp32 torch error {c['torch_err']:.3e}")
    assert err <= 4 * c["torch_err"], (err, c["torch_err"])


@pytest.mark.parametrize("h,w,dim", SHAPES)
def test_aggregate_against_fp64(h, w, dim):
    from slam.optical_flow import gma_aggregate
    c = _case(h, w, dim)
    attn = _attention(c)
    a, v, x = attn.cpu(), c["v"].flatten(2), c["x"].flatten(2)
    ref = x.double() + GAMMA * torch.einsum("bij,bcj->bci", a.double(), v.double())
    t32 = x + GAMMA * torch.einsum("bij,bcj->bci", a, v)
    torch_err = float((t32.double() - ref).abs().max())
    xd = c["x"].to(DEV)
    got = gma_aggregate(attn, c["v"].to(DEV), xd, GAMMA)
    assert tuple(got.shape) == (2, dim, h, w)
    err = float((got.cpu().double().flatten(2) - ref).abs().max())
    print(f"aggregate {h}x{w} dim {dim}: kernel error {err:.3e}, fp32 torch error {torch_err:.3e}")
    assert err <= 4 * torch_err, (err, torch_err)
    assert torch.equal(gma_aggregate(attn, c["v"].to(DEV), xd, 0.0), xd)                      # gamma = 0: x, bit for bit


@pytest.mark.parametrize("h,w,dim", [(17, 22, 132), (33, 40, 128)])
def test_kernels_reproducible_and_batch_equals_single(h, w, dim):
    from slam.optical_flow import gma_aggregate, gma_attention
    c = _case(h, w, dim)
    q, k, v, x = (c[n].to(DEV) for n in "qkvx")
    a1, a2 = gma_attention(q, k, c["scale"]), gma_attention(q, k, c["scale"])
    assert torch.equal(a1, a2)
    o1, o2 = gma_aggregate(a1, v, x, GAMMA), gma_aggregate(a1, v, x, GAMMA)
    assert torch.equal(o1, o2)
    for b in range(2):
        s = slice(b, b + 1)
        ab = gma_attention(q[s].contiguous(), k[s].contiguous(), c["scale"])
        assert torch.equal(ab, a1[s]), b
        assert torch.equal(gma_aggregate(ab, v[s].contiguous(), x[s].contiguous(), GAMMA), o1[s]), b


def test_bad_arguments_return_error_codes():
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    t = torch.full((2 * 132 * 16 * 16,), 7.0, device=DEV)
    out = torch.full((2 * 256 * 256,), -3.0, device=DEV)
    s = _C._stream(torch.device(DEV))
    with pytest.raises(RuntimeError, match=r"gsr_gma_attention failed \(code -\d+\): gsr_gma_attention: .*dim 130"):
        lib.gsr_gma_attention(2, 130, 16, 16, t.data_ptr(), t.data_ptr(), 0.1, out.data_ptr(), s)
    with pytest.raises(RuntimeError, match=r"gsr_gma_attention failed \(code -\d+\): gsr_gma_attention: a pointer is NULL"):
        lib.gsr_gma_attention(2, 128, 16, 16, t.data_ptr(), t.data_ptr(), 0.1, None, s)
    with pytest.raises(RuntimeError, match=r"gsr_gma_aggregate failed \(code -\d+\): gsr_gma_aggregate: .*dim 130"):
        lib.gsr_gma_aggregate(2, 130, 16, 16, out.data_ptr(), t.data_ptr(), t.data_ptr(), 0.5, out.data_ptr(), s)
    with pytest.raises(RuntimeError, match=r"gsr_gma_aggregate failed \(code -\d+\): gsr_gma_aggregate: a pointer is NULL"):
        lib.gsr_gma_aggregate(2, 128, 16, 16, None, t.data_ptr(), t.data_ptr(), 0.5, out.data_ptr(), s)
    with pytest.raises(RuntimeError, match=r"code -\d+"):
        lib.gsr_gma_attention(2, 128, 0, 16, t.data_ptr(), t.data_ptr(), 0.1, out.data_ptr(), s)
    torch.cuda.synchronize()
    assert bool((out == -3.0).all()) and bool((t == 7.0).all())                               # nothing was launched


# ---- the network against the reference ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_gma.npz"))


@pytest.fixture(scope="module")
def estimator(golden):
    from slam.optical_flow import GmaFlow, gma_recipe_state_dict
    return GmaFlow(gma_recipe_state_dict(int(golden["seed"])), DEV)


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
def test_estimator_against_reference_gma(golden, estimator, name):
    z = golden
    img1, img2 = _pair_images(z, name)
    H, W = img1.shape[1:]
    tr = {}
    f12, f21 = estimator.pair(img1, img2, ndc=False, trace=tr)
    t1 = {}
    estimator.pair(img1, img2, iters=1, ndc=False, trace=t1)
    N = tr["flow_low"].shape[2] * tr["flow_low"].shape[3]
    assert tuple(tr["attention"].shape) == (2, N, N) and tuple(tr["motion_global"].shape) == (2, 128) + tuple(tr["flow_low"].shape[2:])
    for d, b in (("12", 0), ("21", 1)):
        s = f"{name}/{d}"
        # attention rows and iteration 0's aggregated motion features: 1e-4 relative, or 10 x the reference's own deviation between
        # thread counts where that is larger
        for tag, got in (("attention", tr["attention"][b][z[f"{s}/attention_rows"]].cpu().numpy()),
                         ("motion_global", tr["motion_global"][b].reshape(-1)[z[f"{s}/motion_global_idx"]].cpu().numpy())):
            ref = z[f"{s}/{tag}"]
            assert got.shape == ref.shape
            err = float(np.abs(got.astype(np.float64) - ref).max())
            bar = max(1e-4 * float(np.abs(ref).max()), 10 * float(z[f"{s}/{tag}_threads_dev"]))
            print(s, tag, "max abs error", err, "bar", bar)
            assert err <= bar, (s, tag, err, bar)
        assert _rel(t1["flow1"][b].cpu().numpy(), z[f"{s}/flow1"]) <= 1e-4, s
        e20 = _rel(tr["flow_low"][b].cpu().numpy(), z[f"{s}/flow20"])
        print(s, "flow20 relative error", e20, "; the uniform-attention control differs by", _rel(z[f"{s}/flow20_uniform"], z[f"{s}/flow20"]))
        assert e20 <= 1e-4, (s, e20)
        assert _rel(z[f"{s}/flow20_uniform"], z[f"{s}/flow20"]) >= 100 * 1e-4        # a wrong attention could not pass the line above
        up = (f12 if d == "12" else f21).cpu().numpy()
        step = int(z[f"{s}/flow_up_step"])                  # the fixture keeps every step-th row and column
        up = up[::step, ::step]
        ref_up = z[f"{s}/flow_up"]
        assert up.shape == ref_up.shape
        err = float(np.abs(up - ref_up).max())
        print(s, "flow_up max abs error px", err)
        assert err <= 1e-3, (s, err)
    # NDC output: the same flow / (W, H) * 2
    n12, _ = estimator.pair(img1, img2)
    torch.testing.assert_close(n12, f12 / torch.tensor([W, H], dtype=torch.float32, device=DEV) * 2, rtol=0, atol=1e-6)


def test_estimator_deterministic_and_encodes_each_key_once(golden):
    from slam.optical_flow import GmaFlow, gma_recipe_state_dict
    est = GmaFlow(gma_recipe_state_dict(int(golden["seed"])), DEV)
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
    assert est.encoder_runs == 7 and est.pairs == 5 and all(torch.equal(u, v) for u, v in zip(x1, y2))
    est.forget(0)
    with pytest.raises(KeyError):
        est.pair(None, b, key_i=0, key_j=1)


def test_estimator_refuses_graph_capture(golden):
    from slam.optical_flow import GmaFlow, gma_recipe_state_dict
    est = GmaFlow(gma_recipe_state_dict(int(golden["seed"])), DEV)
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


def test_memory_guard_on_device(golden):
    from slam.optical_flow import GmaFlow, attention_bytes, gma_recipe_state_dict
    est = GmaFlow(gma_recipe_state_dict(int(golden["seed"])), DEV, max_attention_bytes=attention_bytes(130, 170) - 1)
    a, b = _pair_images(golden, "a")
    with pytest.raises(ValueError, match="max_attention_bytes"):
        est.pair(a, b)
    assert est.encoder_runs == 0


# ---- a dataset with a GmaFlow --------------------------------------------------------------------------------------------------------
def test_tum_dataset_takes_a_gma_estimator(tmp_path, golden):
    """A TUM-layout sequence of 8 frames at 320 x 240: gt_flow is GmaFlow.pair on the two frames, bit for bit, whole and under the frames'
    motion masks (as the backend masks its targets), and flow_stats counts the pair. The backend consumes gt_flow unchanged
    (test_hip_raft.py runs that path)."""
    from slam.config import apply_cli_overrides, load_config
    from slam.dataset import SyntheticRGBDDataset
    from slam.optical_flow import GmaFlow, gma_recipe_state_dict
    from slam.recorded import load_dataset, write_tum_sequence
    from test_hip_recorded_slam import _write_configs
    src = SyntheticRGBDDataset(num_frames=8, width=320, height=240, seed=1, dynamic=True, dystart=2)
    seq = tmp_path / "data" / "dyn"
    calib = write_tum_sequence(src, str(seq), masks=True)
    cfg = apply_cli_overrides(load_config(_write_configs(tmp_path, seq, calib, {"dystart": 2})), dynamic=True)
    sd = gma_recipe_state_dict(int(golden["seed"]))
    est = GmaFlow(sd, DEV)
    ds = load_dataset(cfg, DEV, flow=est)
    assert hasattr(ds, "gt_flow") and len(ds) == 8
    f01, valid = ds.gt_flow(0, 1)
    f10, _ = ds.gt_flow(1, 0)
    assert tuple(f01.shape) == (240, 320, 2) and bool(valid.all())
    st = ds.flow_stats
    assert st["pairs"] == est.pairs == 1 and np.isfinite(st["ms_per_pair"]) and st["ms_per_pair"] > 0, st
    i0, _, _, m0 = ds[0]
    i1, _, _, m1 = ds[1]
    fresh = GmaFlow(sd, DEV)
    g01, g10 = fresh.pair(i0, i1)
    assert torch.equal(f01, g01) and torch.equal(f10, g10)
    assert torch.equal(f01.permute(2, 0, 1) * m0, g01.permute(2, 0, 1) * m0) and torch.equal(f10.permute(2, 0, 1) * m1, g10.permute(2, 0, 1) * m1)
    assert bool(torch.isfinite(f01).all()) and float(f01.abs().max()) > 0
    ds.close()
