"""Plain fp64 restatements of the small per-iteration operations (rotations of the node graph, ARAP, elastic, the edge intensity, the
exposure-gradient terms of the weighted L1 loss), for the GPU comparisons of tests/test_hip_small_kernels_fp64.py and
tests/test_hip_track_step.py. Test infrastructure only: tests/test_fp64_references.py pins every one of them to the
outputs recorded from the reference under tests/golden/ (the exposure terms: to autograd through oracle/loss_oracle.py, which those
outputs pin), so that the GPU tests compare against the right thing."""
import torch


def svd_rotations64(S):
    """R = V U^T of S = U Sigma V^T in fp64; where det(R) <= 0 the column of U of the smallest singular value is negated first
    (estimate_rotation, utils/deform_utils.py:152-162). [..., 3, 3] -> [..., 3, 3] float64."""
    shape = S.shape
    S = S.detach().to(torch.float64).reshape(-1, 3, 3)
    U, sig, Vh = torch.linalg.svd(S)
    V = Vh.transpose(-1, -2)
    R = V @ U.transpose(-1, -2)
    flip = torch.det(R) <= 0
    if bool(flip.any()):
        idx = torch.nonzero(flip, as_tuple=False).flatten()
        Um = U.clone()
        Um[idx, :, torch.argmin(sig[idx], dim=-1)] *= -1
        R[idx] = V[idx] @ Um[idx].transpose(-1, -2)
    return R.reshape(shape)


def arap_edges64(seq, nn_idx, keep):
    """E[..., t, i, k] = (x_i - x_nn(i,k)) * keep of every sample: seq [V, T, M, 3] float64, nn_idx / keep [V, M, K] -> [V, T, M, K, 3]."""
    V, T, M, _ = seq.shape
    K = nn_idx.shape[-1]
    idx = nn_idx[:, None, :, :, None].expand(V, T, M, K, 3).reshape(V, T, M * K, 3)
    nb = torch.gather(seq, 2, idx).reshape(V, T, M, K, 3)
    return (seq[:, :, :, None, :] - nb) * keep.to(seq.dtype)[:, None, :, :, None]


def arap_covariances64(E, keep):
    """(S, unchanged): S [V, T-1, M, 3, 3] = sum_k E_0[k] keep[k] E_t[k]^T and the reference's rule that zeroes it (some coordinate in which
    no edge of the vertex changed, utils/deform_utils.py:147-149)."""
    E0, Et = E[:, :1], E[:, 1:]
    S = torch.einsum("vtmka,vmk,vtmkb->vtmab", E0.expand_as(Et), keep.to(E.dtype), Et)
    unchanged = (E0 == Et).all(dim=-2).any(dim=-1)
    return S, unchanged


def arap_reference64(seq, nn_idx, keep):
    """cal_arap_error (utils/deform_utils.py:177-205, unit edge weights, no subsampling) per view: seq [V, T, M, 3] float64 (sample 0 is the
    rest pose), nn_idx / keep [V, M, K]. The rotations are constants of the backward pass, as in the reference."""
    E = arap_edges64(seq, nn_idx, keep)
    w = keep.to(seq.dtype)
    with torch.no_grad():
        S, unchanged = arap_covariances64(E.detach(), keep)
        R = svd_rotations64(torch.where(unchanged[..., None, None], torch.zeros_like(S), S))
    stretch = E[:, 1:] - torch.einsum("vtmab,vmkb->vtmka", R, E[:, 0])
    return (w[:, None] * stretch.square().sum(dim=-1)).sum(dim=(1, 2, 3))


def elastic_reference64(nodes_t, nn_weight, nn_idx):
    """ControlNodeWarp.elastic_loss' body (utils/time_utils.py:1160-1165): nodes_t [..., M, T, 3] float64, nn_weight / nn_idx [M, K]."""
    edge_t = (nodes_t[..., nn_idx, :, :] - nodes_t[..., :, None, :, :]).norm(dim=-1)
    var = edge_t.var(dim=-1)
    var = var / (var.detach() + 1e-5)
    return (var * nn_weight).sum(dim=-1).mean(dim=-1)


def edge_intensity64(image, eps=0.01):
    """The gradient magnitude Camera.compute_grad_mask thresholds (utils/camera_utils.py:205-233, utils/slam_utils.py:5-39): channel mean,
    reflect padding, Scharr / 16 both ways, zero where one of the nine taps is not above eps in magnitude. image [3, H, W] -> [H, W] float64."""
    gray = image.to(torch.float64).mean(dim=0, keepdim=True)
    p = torch.nn.functional.pad(gray[None], (1, 1, 1, 1), mode="reflect")[0, 0]
    H, W = gray.shape[-2:]
    tap = lambda dy, dx: p[dy:dy + H, dx:dx + W]
    gv = ((3 * tap(0, 0) + 10 * tap(0, 1) + 3 * tap(0, 2)) - (3 * tap(2, 0) + 10 * tap(2, 1) + 3 * tap(2, 2))) / 16.0
    gh = ((3 * tap(0, 0) + 10 * tap(1, 0) + 3 * tap(2, 0)) - (3 * tap(0, 2) + 10 * tap(1, 2) + 3 * tap(2, 2))) / 16.0
    valid = torch.ones((H, W), dtype=torch.bool)
    for dy in range(3):
        for dx in range(3):
            valid &= tap(dy, dx).abs() > eps
    return torch.sqrt(gv * gv + gh * gh) * valid


def weighted_l1_exposure_terms64(image, gt_image, w_rgb, exposure_a, exposure_b, alpha, opacity=None):
    """Per element of the image, the two terms whose sums are dL/d(exposure_a) and dL/d(exposure_b) of the weighted L1 tracking loss
    (slam_losses.weighted_l1_loss; get_loss_tracking, utils/slam_utils.py:57-62,118-135), from its definition:

        L_rgb = alpha * mean_{3,H,W}( w |r| ),   r = exp(a) I + b - gt,   w = w_rgb (1 if None) * opacity (if given: a constant weight)
        dL/da = sum alpha / (3 N) * w * sign(r) * exp(a) * I            dL/db = sum alpha / (3 N) * w * sign(r)

    (the depth term does not depend on the exposure). image / gt_image [3, H, W], w_rgb / opacity [H, W] or [1, H, W] or None, exposure_a /
    exposure_b floats (0.0 and 0.0 without the pair). Returns (terms_a, terms_b, r), each [3, H, W] float64."""
    I, gt = image.detach().to(torch.float64), gt_image.detach().to(torch.float64)
    _, H, W = I.shape
    w = torch.ones((1, H, W), dtype=torch.float64)
    if w_rgb is not None:
        w = w * w_rgb.detach().to(torch.float64).reshape(1, H, W)
    if opacity is not None:
        w = w * opacity.detach().to(torch.float64).reshape(1, H, W)
    ea = torch.exp(torch.tensor(float(exposure_a), dtype=torch.float64))
    r = ea * I + float(exposure_b) - gt
    dL_dr = float(alpha) / (3.0 * H * W) * w * torch.sign(r)
    return dL_dr * ea * I, dL_dr.expand(3, H, W).clone(), r
