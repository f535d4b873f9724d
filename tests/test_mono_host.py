"""Host logic of monocular (RGB-only) input: the scale-aligned trajectory error, the covisibility pruning of the back-end, the front-end's
reset rule, the refusal of the dynamic model, and recorded sequences without depth files. No GPU."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


# ---- Sim(3) alignment --------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _frames(gt_c2w, est_c2w):
    """{id: camera stand-in} with the W2C pose pairs eval_ate reads."""
    def w2c(m):
        inv = np.linalg.inv(m)
        return torch.tensor(inv[:3, :3]), torch.tensor(inv[:3, 3])
    frames = {}
    for i, (g, e) in enumerate(zip(gt_c2w, est_c2w)):
        (Rg, Tg), (Re, Te) = w2c(g), w2c(e)
        frames[i] = types.SimpleNamespace(R=Re, T=Te, R_gt=Rg, T_gt=Tg)
    return frames


def _trajectory_pair(scale=2.5):
    rng = np.random.default_rng(3)
    t = np.linspace(0, 1, 12)
    centres = np.stack([0.4 * np.cos(3 * t), 0.2 * t + 0.05 * rng.normal(size=t.size), 0.3 * np.sin(2 * t)], 1)
    Rs, shift = _rotation([0.3, -1.0, 0.5], 0.7), np.array([0.4, -1.1, 2.0])
    gt, est = [], []
    for k, c in enumerate(centres):
        g = np.eye(4)
        g[:3, :3], g[:3, 3] = _rotation([0, 1, 0], 0.05 * k), c
        e = np.eye(4)
        e[:3, :3], e[:3, 3] = Rs @ g[:3, :3], scale * (Rs @ c) + shift          # the estimate: the ground truth scaled, rotated and shifted
        gt.append(g)
        est.append(e)
    return gt, est


def test_monocular_ate_fits_the_scale(tmp_path):
    from slam.eval_utils import align_sim3, eval_ate
    gt, est = _trajectory_pair(2.5)
    frames = _frames(gt, est)
    ate = eval_ate(frames, [], str(tmp_path), 0, final=True, monocular=True)
    assert ate < 1e-9
    doc = json.load(open(os.path.join(str(tmp_path), "plot", "trj_final.json")))
    assert abs(doc["scale"] - 1 / 2.5) < 1e-12 and doc["ate_rmse"] == ate and doc["ate_mean"] < 1e-9
    # the rigid fit of the same pair cannot absorb the scale: centimetres of error on a trajectory of this size
    rigid = eval_ate(frames, [], str(tmp_path), 0, final=True, monocular=False)
    assert rigid > 0.05
    doc = json.load(open(os.path.join(str(tmp_path), "plot", "trj_final.json")))
    assert "scale" not in doc and sorted(doc) == ["ate_mean", "ate_rmse", "trj_est", "trj_gt", "trj_id"]
    # the pieces of the fit
    a = np.stack([m[:3, 3] for m in est]).T
    b = np.stack([m[:3, 3] for m in gt]).T
    rot, trans, scale, err = align_sim3(a, b)
    assert abs(np.linalg.det(rot) - 1) < 1e-12 and float(err.max()) < 1e-9
    np.testing.assert_allclose(scale * rot @ a + trans, b, atol=1e-9)
    # a reflected copy is not matched by a proper rotation; a trajectory without extent has no scale to fit
    assert align_sim3(a * np.array([[1.0], [1.0], [-1.0]]), b)[3].max() > 1e-3
    assert align_sim3(np.repeat(a[:, :1], 12, 1), b)[2] == 1.0


def test_rigid_ate_is_what_it_was():
    """monocular=False: the two figures of the Horn fit, unchanged."""
    from slam.eval_utils import ate_rmse, eval_ate, evaluate_ate
    gt, est = _trajectory_pair(1.0)
    est = [e.copy() for e in est]
    est[3][:3, 3] += [0.01, -0.02, 0.005]
    frames = _frames(gt, est)
    assert abs(eval_ate(frames, [], None, 0, final=True) - ate_rmse(gt, est)) < 1e-12 and ate_rmse(gt, est) > 1e-4
    assert evaluate_ate(gt, est) > 1e-4


# ---- covisibility pruning ----------------------------------------------------------------------------------------------------------
class _Gaussians:
    """The members BackEnd._covisibility_prune touches."""

    def __init__(self, kf_ids):
        self.unique_kfIDs = torch.tensor(kf_ids, dtype=torch.int32)
        self.n_obs = torch.zeros(len(kf_ids), dtype=torch.int32)
        self.get_xyz = torch.zeros(len(kf_ids), 3)
        self.pruned = None

    def prune_points(self, mask):
        self.pruned = mask.clone()
        keep = ~mask
        self.unique_kfIDs, self.n_obs, self.get_xyz = self.unique_kfIDs[keep], self.n_obs[keep], self.get_xyz[keep]


WINDOW = [9, 7, 4, 2]
# eight Gaussians: seeded by keyframe ..., seen from ... of the four window keyframes
KF_IDS = [0, 2, 4, 4, 7, 7, 9, 9]
N_SEEN = [4, 2, 3, 4, 1, 4, 3, 0]


def _backend(monocular, prune_mode, initialized, window_size=4):
    from slam.backend import BackEnd
    cfg = {"Training": {"pose_window": 3, "monocular": monocular, "window_size": window_size, "prune_mode": prune_mode},
           "model_params": {"dynamic_model": False}}
    be = BackEnd(cfg)
    be.gaussians = _Gaussians(KF_IDS)
    be.initialized = initialized
    rows = torch.zeros(len(WINDOW), len(KF_IDS), dtype=torch.int64)
    for j, n in enumerate(N_SEEN):
        rows[:n, j] = 1
    be.occ_aware_visibility = {k: rows[i].clone() for i, k in enumerate(WINDOW)}
    return be, rows


@pytest.mark.parametrize("prune_mode,initialized,want", [
    ("odometry", False, [0, 1, 0, 0, 1, 0, 0, 1]),            # seen from fewer than three keyframes
    ("odometry", True, [0, 1, 0, 0, 1, 0, 0, 1]),
    ("slam", False, [0, 1, 1, 0, 1, 0, 1, 1]),                # seen from at most three, whichever keyframe seeded them
    ("slam", True, [0, 0, 1, 0, 1, 0, 1, 1]),                 # ... and seeded by one of the three newest keyframes (id >= 4)
])
def test_covisibility_pruning_of_a_full_window(prune_mode, initialized, want):
    be, rows = _backend(True, prune_mode, initialized)
    be._window_full_bookkeeping(list(WINDOW))
    want = torch.tensor(want, dtype=torch.bool)
    assert torch.equal(be.gaussians.pruned, want)
    assert be.initialized
    for i, k in enumerate(WINDOW):
        assert torch.equal(be.occ_aware_visibility[k], rows[i][~want])
    assert be.gaussians.n_obs.shape[0] == int((~want).sum())


@pytest.mark.parametrize("prune_mode", ["odometry", "slam"])
def test_rgbd_input_never_prunes_by_covisibility(prune_mode):
    be, rows = _backend(False, prune_mode, True)
    be._window_full_bookkeeping(list(WINDOW))
    assert be.gaussians.pruned is None and be.initialized
    assert torch.equal(be.gaussians.n_obs, torch.tensor(N_SEEN, dtype=torch.int32))
    for i, k in enumerate(WINDOW):
        assert torch.equal(be.occ_aware_visibility[k], rows[i])


def test_a_window_that_is_not_full_is_left_alone():
    be, rows = _backend(True, "slam", False, window_size=5)
    be._window_full_bookkeeping(list(WINDOW))
    assert be.gaussians.pruned is None and not be.initialized


def test_unknown_prune_mode_prunes_nothing():
    be, _ = _backend(True, "keep", False)
    be._window_full_bookkeeping(list(WINDOW))
    assert be.gaussians.pruned is None and be.initialized


# ---- the front-end's reset rule ------------------------------------------------------------------------------------------------------
def _frontend(monocular, initialized, removed):
    from slam.frontend import FrontEnd
    cfg = {"Training": {"monocular": monocular, "kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3,
                        "window_size": 4}, "Results": {}, "model_params": {"dynamic_model": False}}
    fe = FrontEnd(cfg)
    fe.save_results = False
    fe.initialized, fe.reset, fe.current_window = initialized, False, [3, 1, 0]
    calls = []
    fe.add_to_window = lambda cur, vis, occ, window: ([cur] + [k for k in window if k != removed], removed)       # the test double
    fe.add_new_keyframe = lambda *a, **k: calls.append("depth") or "depth map"
    fe.backend = types.SimpleNamespace(handle_keyframe=lambda *a: calls.append("map") or ["keyframe", None, {}, []])
    return fe, calls


@pytest.mark.parametrize("monocular,initialized,removed,resets", [(True, False, 1, True), (True, False, None, False), (True, True, 1, False),
                                                                  (False, False, 1, False)])
def test_a_keyframe_dropped_before_initialisation_resets_a_monocular_run(monocular, initialized, removed, resets):
    fe, calls = _frontend(monocular, initialized, removed)
    viewpoint = types.SimpleNamespace(clean_key=lambda: None)
    fe._insert_keyframe(5, viewpoint, None, {"depth": None, "opacity": None}, 0.5)
    assert fe.reset == resets
    assert calls == ([] if resets else ["depth", "map"])          # a reset seeds and maps nothing: the next frame starts the map over
    assert fe.current_window[0] == 5 and (removed is None or removed not in fe.current_window)


# ---- the dynamic model needs sensor depth -------------------------------------------------------------------------------------------
def test_monocular_input_refuses_the_dynamic_model():
    from slam.system import SLAM, default_config, merge_config
    cfg = merge_config(default_config(), {"Dataset": {"sensor_type": "monocular"}, "model_params": {"dynamic_model": True}})
    with pytest.raises(ValueError) as e:
        SLAM(cfg, types.SimpleNamespace(device="cpu"))
    assert "sensor_type" in str(e.value) and "dynamic_model" in str(e.value)


# ---- recorded sequences without depth files ------------------------------------------------------------------------------------------
def _tum_folder(root, n=3, with_depth=False):
    from slam import recorded
    os.makedirs(os.path.join(root, "rgb"))
    stamps = [recorded.tum_stamp(i) for i in range(n)]
    rng = np.random.default_rng(0)
    for t in stamps:
        Image.fromarray(rng.integers(0, 255, size=(6, 8, 3), dtype=np.uint8)).save(os.path.join(root, "rgb", f"{t}.png"))
    recorded.write_tum_lists(root, stamps, [np.eye(4)] * n)
    if not with_depth:
        os.remove(os.path.join(root, "depth.txt"))
    return stamps


def _tum_config(root, sensor_type, depth_scale=None):
    calib = {"fx": 8.0, "fy": 8.0, "cx": 4.0, "cy": 3.0, "width": 8, "height": 6}
    if depth_scale is not None:
        calib["depth_scale"] = depth_scale
    return {"Dataset": {"type": "tum", "sensor_type": sensor_type, "dataset_path": root, "Calibration": calib}}


def test_tum_folder_without_depth_loads_as_monocular_only(tmp_path):
    from slam import frame_decode, recorded
    root = str(tmp_path / "seq")
    stamps = _tum_folder(root)
    frames = recorded.tum_frames(_tum_config(root, "monocular"))
    assert len(frames) == 3 and frames.depth_paths == [None] * 3
    assert [os.path.basename(p) for p in frames.color_paths] == [f"{t}.png" for t in stamps]
    hf = frame_decode.decode_frame(frames.color_paths[0], frames.depth_paths[0], None, 8, 6, None, False)
    assert hf.depth is None and hf.rgb.shape == (6, 8, 3)
    # any other sensor type needs its depth list, as before; so does a monocular configuration that names a depth_scale
    assert recorded.sequence_has_depth(_tum_config(root, "depth")) and recorded.sequence_has_depth(_tum_config(root, "monocular", 5000.0))
    for cfg in (_tum_config(root, "depth", 5000.0), _tum_config(root, "depth"), _tum_config(root, "monocular", 5000.0)):
        with pytest.raises(FileNotFoundError, match="depth.txt"):
            recorded.tum_frames(cfg)


def test_cofusion_folder_without_depth_loads_as_monocular_only(tmp_path):
    from slam import recorded
    root = str(tmp_path / "seq")
    os.makedirs(os.path.join(root, "colour"))
    for i in range(2):
        Image.fromarray(np.zeros((6, 8, 3), np.uint8)).save(os.path.join(root, "colour", f"Color{i:04d}.png"))
    frames = recorded.parse_cofusion(root, depth=False)
    assert len(frames) == 2 and frames.depth_paths == [None, None]
    with pytest.raises(ValueError, match="depth"):
        recorded.parse_cofusion(root)
