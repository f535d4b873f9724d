"""Saving a finished 4D map and opening it again in a process that never ran SLAM.

A saved map is a directory:
  point_cloud/final/point_cloud.ply      the canonical Gaussians (GaussianModel.save_ply: float32, exact)
  deform/iteration_<N>/deform.pth        the node warp's state_dict (DeformModel.save_weights; dynamic maps only)
  map_state.npz                          what the PLY lacks and rendering at a time t reads, as exact arrays: the motion mask of the dynamic
                                         subset; per tracked frame uid, time, fid, estimated R / T, ground-truth R / T, exposure a / b and
                                         the keyframe flag; the projection matrix, intrinsics, background and time_interval
  map.json                               format version, SH degree, isotropic, deform_init, time_interval, the node hyper-parameters the
                                         DeformModel was built with, background, fx fy cx cy width height, pipeline_params -- for reading
                                         by people and for the values that are not floats; every float that must round-trip is in the .npz
load_map() rebuilds a GaussianModel (load_ply), the DeformModel (load_weights), pose-only cameras (no images), the background and
deltas_for(camera) with the semantics of BackEnd._deltas(frame, train=False). Imports without a GPU; device="cpu" works for everything but
rendering (the cameras are then plain pose holders: the matrices the rasterizer reads are formed by a device kernel)."""
import json
import os
import types

import numpy as np
import torch

from .deform_model import DeformModel
from .gaussian_model import GaussianModel

FORMAT_VERSION = 1
PLY = os.path.join("point_cloud", "final", "point_cloud.ply")
STATE, META = "map_state.npz", "map.json"
DEFORM_ITERATION = 0
FRAME_FIELDS = ("frame_uid", "frame_time", "frame_fid", "frame_R", "frame_T", "frame_has_gt", "frame_R_gt", "frame_T_gt", "frame_has_exposure",
                "frame_exposure_a", "frame_exposure_b", "frame_is_keyframe")
STATE_FIELDS = ("gaussians", "motion_mask", "time_interval", "background", "projection_matrix", "intrinsics", "fov") + FRAME_FIELDS


def _host(t, dtype=np.float32):
    return np.ascontiguousarray(torch.as_tensor(t).detach().cpu().numpy()).astype(dtype, copy=False)


def node_hyperparameters(deform_model):
    """The arguments a DeformModel is built with (its node warp's), as plain values."""
    d = deform_model.deform
    return {"K": int(d.K), "node_num": int(d.max_nodes), "d_rot_as_res": bool(d.d_rot_as_res), "local_frame": bool(d.local_frame),
            "D": int(d.network.D), "W": int(d.network.W), "multires": int(d.network.multires), "t_multires": int(d.network.t_multires)}


def deltas_at(gaussians, camera):
    """BackEnd._deltas(camera, train=False) for a model outside any mapping iteration: (d_xyz, d_scaling, d_rotation) of the dynamic subset
    at the camera's time, or (None, None, None) when the map has no initialised node network or no dynamic Gaussians."""
    g = gaussians
    if not (g.deform is not None and g.deform_init and g.dyn_rows().shape[0] > 0):
        return None, None, None
    nodes = g.deform.deform
    with torch.no_grad():
        d = g.deform.step(g.get_dygs_xyz.detach(), nodes.expand_time(camera.fid), iteration=0, feature=None, motion_mask=g.motion_mask,
                          camera_center=camera.camera_center, time_interval=g.time_interval, t_key=camera.time)
    return d["d_xyz"], d["d_scaling"], d["d_rotation"]


def save_map(slam, directory):
    """Write the map of a finished run (slam: a slam.system.SLAM, or any object with its gaussians, frontend.cameras, frontend.kf_indices,
    background, pipeline_params) into `directory`. Returns the directory."""
    g = slam.gaussians
    cameras = slam.frontend.cameras
    if not cameras:
        raise ValueError("save_map: the run has no tracked frame")
    os.makedirs(directory, exist_ok=True)
    g.save_ply(os.path.join(directory, PLY))
    dynamic = g.deform is not None
    if dynamic:
        g.deform.save_weights(directory, DEFORM_ITERATION)
    uids = sorted(cameras.keys())
    first = cameras[uids[0]]
    keyframes = set(int(k) for k in slam.frontend.kf_indices)
    n = len(uids)
    eye, zero3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    frames = {k: [] for k in FRAME_FIELDS}
    run_has_gt = bool(getattr(getattr(slam, "dataset", None), "has_ground_truth", True))  # (a plain video's cameras carry the identity where others carry ground truth)
    for uid in uids:
        c = cameras[uid]
        has_gt = run_has_gt and getattr(c, "R_gt", None) is not None and getattr(c, "T_gt", None) is not None
        has_exp = getattr(c, "exposure_a", None) is not None and getattr(c, "exposure_b", None) is not None
        frames["frame_uid"].append(int(c.uid))
        frames["frame_time"].append(float(c.time))
        frames["frame_fid"].append(_host(c.fid).reshape(()))
        frames["frame_R"].append(_host(c.R))
        frames["frame_T"].append(_host(c.T))
        frames["frame_has_gt"].append(has_gt)
        frames["frame_R_gt"].append(_host(c.R_gt) if has_gt else eye)
        frames["frame_T_gt"].append(_host(c.T_gt) if has_gt else zero3)
        frames["frame_has_exposure"].append(has_exp)
        frames["frame_exposure_a"].append(_host(c.exposure_a).reshape(()) if has_exp else np.float32(0))
        frames["frame_exposure_b"].append(_host(c.exposure_b).reshape(()) if has_exp else np.float32(0))
        frames["frame_is_keyframe"].append(int(c.uid) in keyframes)
    kinds = {"frame_uid": np.int64, "frame_time": np.float64, "frame_has_gt": np.bool_, "frame_has_exposure": np.bool_, "frame_is_keyframe": np.bool_}
    state = {k: np.asarray(v, dtype=kinds.get(k, np.float32)) for k, v in frames.items()}
    assert all(v.shape[0] == n for v in state.values())
    P = int(g.get_xyz.shape[0])
    state.update(gaussians=np.int64(P), motion_mask=_host(g.motion_mask) if P else np.zeros((0, 1), np.float32),
                 time_interval=np.float64(g.time_interval), background=_host(slam.background),
                 projection_matrix=_host(first.projection_matrix),
                 intrinsics=np.asarray([first.fx, first.fy, first.cx, first.cy], np.float64), fov=np.asarray([first.FoVx, first.FoVy], np.float64))
    np.savez(os.path.join(directory, STATE), **state)
    meta = {"format_version": FORMAT_VERSION, "gaussians": P, "frames": n,
            "sh_degree": int(g.max_sh_degree), "active_sh_degree": int(g.active_sh_degree), "isotropic": bool(g.isotropic),
            "dynamic_model": bool(dynamic), "deform_init": bool(g.deform_init), "time_interval": float(g.time_interval),
            "deform_iteration": DEFORM_ITERATION if dynamic else None, "nodes": node_hyperparameters(g.deform) if dynamic else None,
            "background": [float(v) for v in _host(slam.background)],
            "fx": float(first.fx), "fy": float(first.fy), "cx": float(first.cx), "cy": float(first.cy),
            "width": int(first.image_width), "height": int(first.image_height), "pipeline_params": dict(vars(slam.pipeline_params))}
    with open(os.path.join(directory, META), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=1)
    return directory


class HostCamera(types.SimpleNamespace):
    """A loaded frame on the CPU: pose, time, exposure and intrinsics, without the device matrices of slam.camera.Camera."""
    camera_center = None


class LoadedMap:
    """What load_map() returns: `gaussians` (with .deform attached for a dynamic map), `cameras` {uid: camera}, `kf_indices`, `background`,
    `pipeline_params`, `meta` (map.json) and deltas_for(camera)."""

    def __init__(self, gaussians, cameras, kf_indices, background, pipeline_params, meta, device):
        self.gaussians, self.cameras, self.kf_indices = gaussians, cameras, kf_indices
        self.background, self.pipeline_params, self.meta, self.device = background, pipeline_params, meta, device

    @property
    def dynamic(self):
        return self.gaussians.deform is not None and bool(self.gaussians.deform_init)

    def deltas_for(self, camera):
        """(d_xyz, d_scaling, d_rotation) as BackEnd._deltas(camera, train=False) gives them; (None, None, None) for a static map."""
        return deltas_at(self.gaussians, camera)


def _need(path, what=""):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such file{what}")
    return path


def load_map(directory, device="cuda:0"):
    """Open a map written by save_map. An unknown version, a missing file or field, or a Gaussian count that differs between the PLY and
    map_state.npz raises with the file and the field named."""
    device = torch.device(device)
    meta_path = _need(os.path.join(directory, META), " (not a saved map)")
    with open(meta_path, encoding="utf-8") as f:
        meta = json.load(f)
    if meta.get("format_version") != FORMAT_VERSION:
        raise ValueError(f"{meta_path}: format_version is {meta.get('format_version')!r}, this build reads version {FORMAT_VERSION}")
    for field in ("sh_degree", "active_sh_degree", "isotropic", "dynamic_model", "deform_init", "nodes", "width", "height", "pipeline_params"):
        if field not in meta:
            raise KeyError(f"{meta_path}: field {field!r} is missing")
    state_path = _need(os.path.join(directory, STATE))
    with np.load(state_path, allow_pickle=False) as z:
        for field in STATE_FIELDS:
            if field not in z.files:
                raise KeyError(f"{state_path}: field {field!r} is missing")
        st = {k: z[k] for k in STATE_FIELDS}
    ply_path = _need(os.path.join(directory, PLY))

    g = GaussianModel(int(meta["sh_degree"]), config=None, device=device)
    g.load_ply(ply_path)
    g.active_sh_degree = int(meta["active_sh_degree"])
    P = int(g.get_xyz.shape[0])
    if int(st["gaussians"]) != P:
        raise ValueError(f"{ply_path} holds {P} Gaussians, but field 'gaussians' of {state_path} says {int(st['gaussians'])}")
    if bool(meta["isotropic"]) != bool(g.isotropic):
        raise ValueError(f"{meta_path}: field 'isotropic' is {meta['isotropic']!r}, but {ply_path} has {g._scaling.shape[1]} scale column(s)")
    dyn = int(g.dyn_rows().shape[0])
    if st["motion_mask"].shape != (dyn, 1):
        raise ValueError(f"{state_path}: field 'motion_mask' has shape {st['motion_mask'].shape}, but {ply_path} has {dyn} dynamic Gaussians")
    mask = torch.from_numpy(st["motion_mask"]).to(device)
    if not torch.equal(mask, g.motion_mask):
        raise ValueError(f"{state_path}: field 'motion_mask' is not the all-ones mask this build's GaussianModel forms")
    g.time_interval = float(st["time_interval"])
    g.deform_init = bool(meta["deform_init"])
    if meta["dynamic_model"]:
        hp = meta["nodes"]
        g.deform = DeformModel(K=hp["K"], node_num=hp["node_num"], d_rot_as_res=hp["d_rot_as_res"], local_frame=hp["local_frame"], device=device)
        if any(hp[k] != v for k, v in node_hyperparameters(g.deform).items()):
            raise ValueError(f"{meta_path}: field 'nodes' is {hp}, this build forms {node_hyperparameters(g.deform)}")
        g.deform.load_weights(directory, int(meta.get("deform_iteration", -1) if meta.get("deform_iteration") is not None else -1))

    n = int(st["frame_uid"].shape[0])
    for field in FRAME_FIELDS:
        if st[field].shape[0] != n:
            raise ValueError(f"{state_path}: field {field!r} has {st[field].shape[0]} rows, 'frame_uid' has {n}")
    fx, fy, cx, cy = (float(v) for v in st["intrinsics"])
    fovx, fovy = (float(v) for v in st["fov"])
    H, W = int(meta["height"]), int(meta["width"])
    projection = torch.from_numpy(st["projection_matrix"]).to(device)
    cameras = {}
    for i in range(n):
        uid, time = int(st["frame_uid"][i]), float(st["frame_time"][i])
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        gt = np.eye(4, dtype=np.float32)
        gt[:3, :3], gt[:3, 3] = st["frame_R_gt"][i], st["frame_T_gt"][i]
        has_exp = bool(st["frame_has_exposure"][i])
        if device.type == "cuda":
            from .camera import Camera
            cam = Camera(uid, None, None, gt, projection, fx, fy, cx, cy, fovx, fovy, H, W, time, device=device)
            cam.update_RT(st["frame_R"][i], st["frame_T"][i])
            with torch.no_grad():
                cam.exposure_a.copy_(T(st["frame_exposure_a"][i:i + 1]))
                cam.exposure_b.copy_(T(st["frame_exposure_b"][i:i + 1]))
        else:
            cam = HostCamera(uid=uid, R=T(st["frame_R"][i]), T=T(st["frame_T"][i]), R_gt=T(gt[:3, :3]), T_gt=T(gt[:3, 3]), time=time,
                             fx=fx, fy=fy, cx=cx, cy=cy, FoVx=fovx, FoVy=fovy, image_height=H, image_width=W, projection_matrix=projection,
                             exposure_a=T(st["frame_exposure_a"][i:i + 1]), exposure_b=T(st["frame_exposure_b"][i:i + 1]), device=device)
        cam.fid = T(st["frame_fid"][i:i + 1])
        if not bool(st["frame_has_gt"][i]):
            cam.R_gt = cam.T_gt = None
        if not has_exp:                                            # a frame that was not a keyframe was cleaned: it has no exposure
            cam.exposure_a = cam.exposure_b = None
        cameras[uid] = cam
    kf = [int(u) for u, k in zip(st["frame_uid"], st["frame_is_keyframe"]) if k]
    background = torch.from_numpy(st["background"]).to(device)
    return LoadedMap(g, cameras, kf, background, types.SimpleNamespace(**meta["pipeline_params"]), meta, device)
