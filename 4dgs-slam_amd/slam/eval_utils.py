"""Trajectory and rendering evaluation -- the counterpart of the reference's ``utils/eval_utils.py``: Horn alignment + ATE
(align :160-200, evaluate_ate :203-219, the evo APE-RMSE of evaluate_evo :106-150), eval_ate (:221-297), eval_rendering (:300-428:
masked PSNR, SSIM, depth L1, and LPIPS when a slam.perceptual.Lpips is given), save_gaussians (:431-440). No evo / wandb / cv2."""
import json
import os

import numpy as np
import torch

import slam_losses
from gaussian_renderer import render


def align(model, data):
    """Horn's closed-form rigid alignment of two 3xn point sets (utils/eval_utils.py:160-200): returns (rot 3x3, trans 3x1,
    per-point translational error after alignment [n])."""
    model, data = np.asarray(model, np.float64), np.asarray(data, np.float64)
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    W = np.zeros((3, 3))
    for c in range(model.shape[1]):
        W += np.outer(mz[:, c], dz[:, c])
    U, _, Vh = np.linalg.svd(W.T)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    trans = data.mean(1, keepdims=True) - rot @ model.mean(1, keepdims=True)
    err = rot @ model + trans - data
    return rot, trans, np.sqrt(np.sum(err * err, 0))


def evaluate_ate(gt_traj, est_traj):
    """utils/eval_utils.py:203-219: mean translational error after aligning the GROUND TRUTH onto the estimate (the reference passes
    (gt, est) into align(model, data)); poses are 4x4 camera-to-world matrices."""
    gt = np.stack([np.asarray(p)[:3, 3] for p in gt_traj]).T
    est = np.stack([np.asarray(p)[:3, 3] for p in est_traj]).T
    _, _, err = align(gt, est)
    return float(err.mean())


def ate_rmse(gt_traj, est_traj):
    """What evaluate_evo reports (:106-128): RMSE of the translation part after aligning the estimate onto the ground truth
    (evo's align_trajectory without scale = the same Horn / Umeyama rigid fit)."""
    gt = np.stack([np.asarray(p)[:3, 3] for p in gt_traj]).T
    est = np.stack([np.asarray(p)[:3, 3] for p in est_traj]).T
    _, _, err = align(est, gt)
    return float(np.sqrt(np.mean(err * err)))


def align_sim3(model, data):
    """Umeyama's similarity fit of two 3xn point sets, data ~ scale * rot @ model + trans -- what evo's align_trajectory(correct_scale=True)
    applies in evaluate_evo (utils/eval_utils.py:112-152) for monocular input. Returns (rot 3x3, trans 3x1, scale, per-point error [n]).
    A model without extent (every point the same) has no scale to fit: scale = 1."""
    model, data = np.asarray(model, np.float64), np.asarray(data, np.float64)
    n = model.shape[1]
    mz = model - model.mean(1, keepdims=True)
    dz = data - data.mean(1, keepdims=True)
    U, D, Vh = np.linalg.svd(dz @ mz.T / n)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vh) < 0:
        S[2, 2] = -1
    rot = U @ S @ Vh
    var = float(np.sum(mz * mz)) / n
    scale = float(np.trace(np.diag(D) @ S)) / var if var > 1e-20 else 1.0            # (1e-10 of the unit of length: rounding of the mean)
    trans = data.mean(1, keepdims=True) - scale * rot @ model.mean(1, keepdims=True)
    err = scale * rot @ model + trans - data
    return rot, trans, scale, np.sqrt(np.sum(err * err, 0))


def ate_sim3(gt_traj, est_traj):
    """(RMSE, mean, scale) of the translation error after the similarity fit of the estimate onto the ground truth."""
    gt = np.stack([np.asarray(p)[:3, 3] for p in gt_traj]).T
    est = np.stack([np.asarray(p)[:3, 3] for p in est_traj]).T
    _, _, scale, err = align_sim3(est, gt)
    return float(np.sqrt(np.mean(err * err))), float(err.mean()), scale


def _pose_c2w(R, T):
    m = np.eye(4)
    m[:3, :3] = R.detach().cpu().numpy()
    m[:3, 3] = T.detach().cpu().numpy()
    return np.linalg.inv(m)


def eval_ate(frames, kf_ids, save_dir=None, iterations=0, final=False, monocular=False):
    """utils/eval_utils.py:221-297 without the plots: trajectory json + ATE. `frames` = {frame id: Camera}. Returns the RMSE; with
    final=True every tracked frame counts (:238-249), otherwise the keyframes. monocular=True: the estimate is fitted onto the ground
    truth with scale (align_sim3; the map of an RGB-only run has no metric scale) and the json also records the fitted `scale`."""
    ids = sorted(frames.keys()) if final else list(kf_ids)
    est = [_pose_c2w(frames[i].R, frames[i].T) for i in ids]
    gt = [_pose_c2w(frames[i].R_gt, frames[i].T_gt) for i in ids]
    if monocular:
        rmse, mean, scale = ate_sim3(gt, est) if len(ids) >= 3 else (0.0, 0.0, 1.0)
        out = {"trj_id": ids, "ate_rmse": rmse, "ate_mean": mean, "scale": scale}
    else:
        out = {"trj_id": ids, "ate_rmse": ate_rmse(gt, est) if len(ids) >= 3 else 0.0, "ate_mean": evaluate_ate(gt, est) if len(ids) >= 3 else 0.0}
    if save_dir:
        plot_dir = os.path.join(save_dir, "plot")
        os.makedirs(plot_dir, exist_ok=True)
        label = "final" if final else "{:04}".format(iterations)
        with open(os.path.join(plot_dir, f"trj_{label}.json"), "w", encoding="utf-8") as f:
            json.dump({**out, "trj_est": [p.tolist() for p in est], "trj_gt": [p.tolist() for p in gt]}, f, indent=1)
    return out["ate_rmse"]


def write_trajectory(frames, stamps, path):
    """The tracked frames' camera-to-world poses as a TUM trajectory file, `stamp tx ty tz qx qy qz qw` per line in frame order (the format
    of recorded.write_tum_lists' groundtruth.txt, which evo and the TUM tools read). `frames` = {frame id: Camera}; stamps[frame id] is the
    frame's time in seconds (None: the frame id). Returns the path."""
    from .recorded import rotation_to_quaternion
    lines = []
    for i in sorted(frames.keys()):
        c2w = _pose_c2w(frames[i].R, frames[i].T)
        stamp = float(stamps[i]) if stamps is not None else float(i)
        lines.append(f"{stamp:.6f} " + " ".join(f"{v:.12f}" for v in (*c2w[:3, 3], *rotation_to_quaternion(c2w[:3, :3]))))
    with open(path, "w") as f:
        f.write("# estimated trajectory (camera to world; no ground truth)\n# timestamp tx ty tz qx qy qz qw\n" + "\n".join(lines) + "\n")
    return path


def psnr(img1, img2):
    """gaussian_splatting/utils/image_utils.py:19-21."""
    mse = ((img1 - img2) ** 2).view(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


@torch.no_grad()
def eval_rendering(frames, gaussians, dataset, save_dir, pipe, background, kf_indices=(), iteration="final", deltas_for=None, interval=1,
                   lpips=None):
    """utils/eval_utils.py:300-428: render every frame at its estimated pose and compare with the sensor image: PSNR over the valid
    pixels (:371-381), SSIM, depth L1 (:383-388). `deltas_for(frame)` -> (dx, ds, dr) supplies the dynamic subset's deformation.
    A frame without sensor depth (monocular input: the dataset hands out None) is scored on every pixel with colour and adds nothing to
    the depth L1; `l1_depth` is None when no frame had depth.
    `lpips` (a slam.perceptual.Lpips): the clamped render against the whole sensor image (:352, :378), scores kept on the device and
    read once after the loop; the result and final_result.json gain `mean_lpips`."""
    psnrs, ssims, depths = [], [], []
    end_idx = len(frames) - 1 if len(frames) > 1 else 1
    lpips_scores = None if lpips is None else torch.empty(len(range(0, end_idx, interval)), dtype=torch.float32, device=lpips.device)
    for idx in range(0, end_idx, interval):
        frame = frames[idx]
        gt_image, gt_depth, _, motion_mask = dataset[idx]
        dx, ds, dr = deltas_for(frame) if deltas_for is not None else (0, 0, 0)
        pkg = render(frame, gaussians, pipe, background, dynamic=False, dx=dx, ds=ds, dr=dr)
        image = torch.clamp(pkg["render"], 0.0, 1.0)
        has_depth = gt_depth is not None
        valid_depth = torch.as_tensor(gt_depth > 0, device=image.device) if has_depth else torch.ones(image.shape[-2:], dtype=torch.bool, device=image.device)
        mask = gt_image > 0
        if deltas_for is None and motion_mask is not None:                        # static map: the moving region is not evaluated (:372-376)
            mask = mask & motion_mask.view(1, *valid_depth.shape) & valid_depth[None]
            valid_depth = valid_depth & motion_mask
        else:
            mask = mask & valid_depth[None]
        psnrs.append(float(psnr(image[mask].unsqueeze(0), gt_image[mask].unsqueeze(0))))
        ssims.append(float(slam_losses.ssim(image, gt_image)))
        if has_depth:
            l1 = torch.abs(torch.as_tensor(gt_depth, device=image.device)[None] - pkg["depth"]) * valid_depth[None]
            depths.append(float(l1.sum() / (valid_depth.sum() + 1e-7)))
        if lpips is not None:
            lpips_scores[len(psnrs) - 1:len(psnrs)] = lpips(image[None], gt_image[None])
    out = {"mean_psnr": float(np.mean(psnrs)), "mean_ssim": float(np.mean(ssims)), "l1_depth": float(np.mean(depths)) if depths else None,
           "frames": len(psnrs)}
    if lpips is not None:
        mean_lpips = float(np.mean(lpips_scores.cpu().numpy().astype(np.float64)))
        out = {"mean_psnr": out["mean_psnr"], "mean_ssim": out["mean_ssim"], "mean_lpips": mean_lpips, "l1_depth": out["l1_depth"],
               "frames": out["frames"]}
    if save_dir:
        d = os.path.join(save_dir, "psnr", str(iteration))
        os.makedirs(d, exist_ok=True)
        json.dump(out, open(os.path.join(d, "final_result.json"), "w", encoding="utf-8"), indent=1)
    return out


def save_gaussians(gaussians, name, iteration, final=False):
    """utils/eval_utils.py:431-440."""
    if name is None:
        return
    path = os.path.join(name, "point_cloud/final" if final else "point_cloud/iteration_{}".format(str(iteration)))
    gaussians.save_ply(os.path.join(path, "point_cloud.ply"))
