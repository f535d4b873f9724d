"""The fp64 references of tests/test_hip_small_kernels_fp64.py (tests/fp64_references.py, oracle/loss_oracle.py evaluated in fp64) against
what was recorded from the reference under tests/golden/: the GPU tests then compare the kernels with the right thing."""
import os

import numpy as np
import pytest
import torch

import util
import fp64_references as ref64

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "golden_node_losses.npz"))
FX = np.load(os.path.join(GOLDEN, "golden_loss.npz"), allow_pickle=False)


def _dense(Nv, K=10):
    nn_idx = torch.zeros((Nv, K), dtype=torch.int64)
    keep = torch.zeros((Nv, K), dtype=torch.bool)
    nn_idx[G["conn_ii"], G["conn_nn"]] = torch.as_tensor(G["conn_jj"])
    keep[G["conn_ii"], G["conn_nn"]] = True
    return nn_idx, keep


def test_fp64_svd_rotations_reproduce_the_recorded_rotations():
    for a, b in (("rot_S", "rot_R"), ("rot_S_random", "rot_R_random")):
        R = ref64.svd_rotations64(torch.tensor(G[a]))
        assert R.dtype == torch.float64
        np.testing.assert_allclose(R.numpy(), G[b], atol=2e-5)
    assert int(G["rot_n_reflections"]) > 0                       # the recorded set exercises the flip


def test_fp64_arap_program_reproduces_the_recorded_error_and_gradient():
    seq = torch.tensor(G["arap_nodes_seq"]).double()[None].requires_grad_(True)
    nn_idx, keep = _dense(seq.shape[2])
    err = ref64.arap_reference64(seq, nn_idx[None], keep[None])
    err.sum().backward()
    assert err.shape == (1,) and abs(float(err.detach()) - float(G["arap_error"])) <= 2e-5 * abs(float(G["arap_error"]))
    np.testing.assert_allclose(seq.grad[0].numpy(), G["arap_grad"], rtol=2e-4, atol=2e-6)
    # the cross-covariances the rotations are fitted to are the recorded ones too (sample 2 against the rest pose)
    S, unchanged = ref64.arap_covariances64(ref64.arap_edges64(seq.detach(), nn_idx[None], keep[None]), keep[None])
    assert not bool(unchanged.any())
    np.testing.assert_allclose(S[0, 1].numpy(), G["rot_S"], rtol=1e-5, atol=1e-7)


def test_fp64_elastic_program_reproduces_the_recorded_value_and_gradient():
    nodes = torch.tensor(G["warp_nodes"]).double()
    d = ((nodes[:, None] - nodes[None]) ** 2).sum(-1)
    nn_dist, nn_idx = torch.topk(d, 3, dim=-1, largest=False, sorted=True)
    radius, nw = torch.exp(torch.tensor(G["warp_radius_raw"]).double()), torch.sigmoid(torch.tensor(G["warp_weight_raw"]).double())
    w = torch.exp(-nn_dist / (2 * radius[nn_idx] ** 2)) * nw[nn_idx][..., 0] + 1e-7
    w = w / w.sum(-1, keepdim=True)
    amp = torch.tensor(G["motion_amp"]).double().requires_grad_(True)
    t = torch.tensor(np.asarray(G["elastic_t"], np.float32)).double()[None, :, None]
    nodes_t = nodes[:, None, :] + amp[:, None, :] * torch.sin(9.0 * t + torch.tensor(G["motion_phase"]).double()[:, None, :])
    val = ref64.elastic_reference64(nodes_t, w[:, 1:], nn_idx[:, 1:])
    val.backward()
    assert abs(float(val.detach()) - float(G["elastic_value"])) <= 1e-4 * abs(float(G["elastic_value"]))
    np.testing.assert_allclose(amp.grad.numpy(), G["elastic_grad_amp"], rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize("name", [str(c) for c in FX["ssim_cases"]])
def test_ssim_reference_in_fp64_reproduces_the_recorded_values(name):
    from oracle.loss_oracle import ssim_reference

    img1 = torch.tensor(FX[f"{name}/img1"]).double().requires_grad_(True)
    img2 = torch.tensor(FX[f"{name}/img2"]).double()
    mk = torch.tensor(FX[f"{name}/mask"]) if FX[f"{name}/mask"].size else None
    v = ssim_reference(img1, img2, mk)
    v.backward()
    assert v.dtype == torch.float64
    assert abs(float(v) - float(FX[f"{name}/value"])) < 1e-6
    assert util.rel_l1(img1.grad.numpy(), FX[f"{name}/g_img1"]) < 1e-5


def test_fp64_edge_intensity_reproduces_the_recorded_edge_mask():
    S = np.load(os.path.join(GOLDEN, "golden_slam.npz"))
    inten = ref64.edge_intensity64(torch.tensor(S["gradmask_image"]))
    flat = inten.reshape(-1)
    median = torch.sort(flat)[0][(flat.numel() - 1) // 2]
    assert np.array_equal((inten > median * 1.1)[None].numpy(), S["gradmask_mask"])


@pytest.mark.parametrize("weights", [False, True])
def test_fp64_exposure_terms_sum_to_the_gradient_of_the_loss_program(weights):
    """weighted_l1_exposure_terms64 (written from the loss's definition) against autograd through oracle/loss_oracle.py in fp64 -- the
    program that reproduces the reference's recorded loss values: the terms add up to dL/d(exposure_a) and dL/d(exposure_b)."""
    from oracle.loss_oracle import weighted_l1_loss_reference
    g = torch.Generator().manual_seed(5)
    H, W = 9, 13
    R = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    image, depth, gt_image, gt_depth = R(3, H, W), R(1, H, W), R(3, H, W), R(1, H, W)
    w_rgb, opacity = (R(1, H, W), R(1, H, W)) if weights else (None, None)
    a = torch.tensor([0.03], dtype=torch.float64, requires_grad=True)
    b = torch.tensor([-0.01], dtype=torch.float64, requires_grad=True)
    weighted_l1_loss_reference(image, depth, gt_image, gt_depth, w_rgb=w_rgb, exposure_a=a, exposure_b=b, alpha=0.9, opacity=opacity).backward()
    ta, tb, r = ref64.weighted_l1_exposure_terms64(image, gt_image, w_rgb, 0.03, -0.01, 0.9, opacity=opacity)
    assert ta.dtype == tb.dtype == r.dtype == torch.float64 and ta.shape == tb.shape == r.shape == (3, H, W)
    assert abs(float(ta.sum()) - float(a.grad)) <= 1e-14 and abs(float(tb.sum()) - float(b.grad)) <= 1e-14
    assert float(a.grad) != 0.0 and float(b.grad) != 0.0
