"""The RGB-only (monocular) forms of the tracking and mapping losses against values and gradients recorded from the reference's own
get_loss_tracking_rgb / get_loss_mapping_rgb (tests/golden/make_golden_mono.py -> tests/golden/mono_losses.npz; 12x16, an exposure pair,
a grad mask, pixels under the boundary threshold). CPU: the operands this repository hands the fused kernel -- boundary mask [x grad
mask], a zero depth plane, zero depth weights, alpha = 1 -- with the plain-torch loss expression (oracle/loss_oracle.py) reproduce them.
GPU: slam_losses.get_loss_tracking / get_loss_mapping (the fused kernels) reproduce them. Tolerances: those of tests/test_slam_losses.py."""
import os
import types

import numpy as np
import pytest
import torch

import util  # noqa: F401  (puts the repo and the package on sys.path)

FX = np.load(os.path.join(os.path.dirname(__file__), "golden", "mono_losses.npz"), allow_pickle=False)
TCASES, MCASES = [str(c) for c in FX["tracking_cases"]], [str(c) for c in FX["mapping_cases"]]
CONFIG = {"Training": {"monocular": True, "rgb_boundary_threshold": float(FX["cfg_thr"]), "alpha": float(FX["cfg_alpha"])}}


def _viewpoint(dev):
    a, b = (float(v) for v in FX["exposure"])
    return types.SimpleNamespace(
        original_image=torch.tensor(FX["gt_image"], device=dev), depth=None, grad_mask=torch.tensor(FX["grad_mask"], device=dev),
        exposure_a=torch.nn.Parameter(torch.tensor([a], device=dev)), exposure_b=torch.nn.Parameter(torch.tensor([b], device=dev)),
        motion_mask=torch.tensor(FX["motion_mask"], device=dev), uid=3)


def _inputs(name, dev):
    image = torch.tensor(FX[f"{name}/image"], device=dev, requires_grad=True)
    depth = torch.tensor(FX[f"{name}/depth"], device=dev, requires_grad=True)
    return image, depth


def _check(name, loss, image, depth, vp, tol):
    loss.backward()
    want = float(FX[f"{name}/loss"])
    assert abs(float(loss) - want) < tol * max(1.0, abs(want))
    assert util.rel_l1(image.grad.cpu().numpy(), FX[f"{name}/g_image"]) < tol
    assert depth.grad is None or float(depth.grad.abs().max()) == 0.0            # the reference never touches the depth map
    if FX[f"{name}/g_a"].size:
        assert abs(float(vp.exposure_a.grad) - float(FX[f"{name}/g_a"][0])) < 10 * tol * max(1e-3, abs(float(FX[f"{name}/g_a"][0])))
        assert abs(float(vp.exposure_b.grad) - float(FX[f"{name}/g_b"][0])) < 10 * tol * max(1e-3, abs(float(FX[f"{name}/g_b"][0])))
    else:
        assert vp.exposure_a.grad is None and vp.exposure_b.grad is None


def _tracking_args(name, dev):
    rm_dynamic, use_mask = [bool(v) for v in FX[f"{name}/flags"]]
    return rm_dynamic, torch.tensor(FX["mask"], device=dev) if use_mask else None


@pytest.mark.parametrize("name", TCASES)
def test_tracking_operands_and_expression_reproduce_the_reference_on_cpu(name):
    from slam_losses import tracking_loss_operands
    from oracle.loss_oracle import weighted_l1_loss_reference
    vp = _viewpoint("cpu")
    image, depth = _inputs(name, "cpu")
    rm_dynamic, mask = _tracking_args(name, "cpu")
    gt_image, gt_depth, w_rgb, w_dep, alpha = tracking_loss_operands(CONFIG, vp, torch.device("cpu"), rm_dynamic, mask)
    assert alpha == 1.0 and float(gt_depth.abs().max()) == 0.0 and float(w_dep.abs().max()) == 0.0
    loss = weighted_l1_loss_reference(image, depth, gt_image, gt_depth, w_rgb, w_dep, vp.exposure_a, vp.exposure_b, alpha,
                                      opacity=torch.tensor(FX[f"{name}/opacity"]))
    _check(name, loss, image, depth, vp, 1e-5)


@pytest.mark.parametrize("name", MCASES)
def test_mapping_operands_and_expression_reproduce_the_reference_on_cpu(name):
    from slam_losses import mapping_loss_operands
    from oracle.loss_oracle import weighted_l1_loss_reference
    vp = _viewpoint("cpu")
    image, depth = _inputs(name, "cpu")
    initialization, rm_dynamic = [bool(v) for v in FX[f"{name}/flags"]]
    gt_image, gt_depth, w_rgb, w_dep, alpha = mapping_loss_operands(CONFIG, vp, torch.device("cpu"), rm_dynamic=rm_dynamic)
    assert alpha == 1.0 and float(gt_depth.abs().max()) == 0.0 and float(w_dep.abs().max()) == 0.0
    a, b = (None, None) if initialization else (vp.exposure_a, vp.exposure_b)
    loss = weighted_l1_loss_reference(image, depth, gt_image, gt_depth, w_rgb, w_dep, a, b, alpha)
    _check(name, loss, image, depth, vp, 1e-5)


def test_a_frame_without_depth_has_no_depth_constants():
    from slam_losses import _keyframe_constants
    gt_image, gt_depth, rgb, dep, t_rgb, t_dep = _keyframe_constants(CONFIG, _viewpoint("cpu"), torch.device("cpu"))
    assert gt_depth is None and dep is None and t_dep is None
    assert rgb.shape == (1, 12, 16) and float(rgb[0, :3, :5].max()) == 0.0 and float(rgb.min()) == 0.0 and float(rgb.max()) == 1.0
    assert torch.equal(t_rgb, rgb * torch.tensor(FX["grad_mask"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", TCASES)
def test_fused_monocular_tracking_loss_matches_the_reference(name):
    from slam_losses import get_loss_tracking
    vp = _viewpoint("cuda")
    image, depth = _inputs(name, "cuda")
    rm_dynamic, mask = _tracking_args(name, "cuda")
    loss = get_loss_tracking(CONFIG, image, depth, torch.tensor(FX[f"{name}/opacity"], device="cuda"), vp, rm_dynamic=rm_dynamic, mask=mask)
    _check(name, loss, image, depth, vp, 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MCASES)
def test_fused_monocular_mapping_loss_matches_the_reference(name):
    from slam_losses import get_loss_mapping
    vp = _viewpoint("cuda")
    image, depth = _inputs(name, "cuda")
    initialization, rm_dynamic = [bool(v) for v in FX[f"{name}/flags"]]
    loss = get_loss_mapping(CONFIG, image, depth, vp, None, initialization=initialization, rm_dynamic=rm_dynamic)
    _check(name, loss, image, depth, vp, 2e-5)
