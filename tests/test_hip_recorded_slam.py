"""The SLAM system on recorded sequences (slam/config.py + slam/recorded.py): frames of the synthetic generator written in the TUM and
CoFusion layouts, loaded back through load_config + load_dataset (PIL decode ahead of the loop, gsr_frame_prepare on the device), then
the reduced-schedule static and dynamic runs of tests/test_hip_slam.py on them."""
import os
import sys
import threading

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

QUICK = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "dynamic_map_iters": 60, "network_init_iters": 40, "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 4}


def _write_configs(tmp_path, seq, calibration, training=None):
    """base.yaml under configs/ (named by the leaf relative to an ANCESTOR directory, as the reference's files do) and the leaf."""
    base = {"Dataset": {"type": "tum", "sensor_type": "depth", "pcd_downsample": 32, "pcd_downsample_init": 8},
            "Results": {"save_results": False, "use_gui": False, "eval_rendering": True}, "opt_params": {"densify_from_iter": 100},
            "Training": dict(QUICK)}
    os.makedirs(tmp_path / "configs" / "rgbd", exist_ok=True)
    with open(tmp_path / "configs" / "rgbd" / "base.yaml", "w") as f:
        yaml.safe_dump(base, f)
    leaf = {"inherit_from": "configs/rgbd/base.yaml", "Dataset": {"dataset_path": str(seq), "Calibration": calibration},
            "Training": dict(training or {})}
    os.makedirs(tmp_path / "configs" / "rgbd" / "seq", exist_ok=True)
    path = tmp_path / "configs" / "rgbd" / "seq" / "seq.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(leaf, f)
    return str(path)


def _check_frames(ds, src, idxs):
    for i in idxs:
        image, depth, pose, motion = ds[i]
        c, d, p, m = src[i]
        q = np.rint(c.clamp(0, 1).cpu().numpy().astype(np.float64) * 255)
        assert image.dtype == torch.float32 and image.is_cuda and image.is_contiguous() and image.shape == c.shape
        assert np.array_equal(image.cpu().numpy().view(np.uint32), (q / 255.0).astype(np.float32).view(np.uint32)), i
        u16 = np.rint(np.asarray(d, np.float64) * 5000).astype(np.uint16)
        assert depth.dtype == np.float32 and np.array_equal(depth.view(np.uint32), (u16 / 5000.0).astype(np.float32).view(np.uint32)), i
        assert pose.dtype == p.dtype and pose.is_cuda and float((pose - p).abs().max()) < 1e-6, i
        assert motion.dtype == torch.bool and motion.is_cuda and torch.equal(motion, m), i


def _reader_threads():
    return [t for t in threading.enumerate() if t.name.startswith("frame-decode")]


def test_static_tum_sequence_end_to_end(tmp_path, monkeypatch):
    """test_slam_static_sequence_end_to_end's sequence and schedule, read back from a TUM-layout directory (colour quantised to bytes,
    depth to 1/5000 m). Measured on MI355X, identical over three runs: ATE 9.6 mm, PSNR 34.7 dB, depth L1 16.0 mm; the bars sit ~20 % off."""
    from slam.config import load_config
    from slam.dataset import SyntheticRGBDDataset
    from slam.recorded import TUMDataset, load_dataset, write_tum_sequence
    from slam.system import SLAM
    torch.manual_seed(0)
    src = SyntheticRGBDDataset(num_frames=32, width=320, height=240, seed=0)
    seq = tmp_path / "data" / "seq"
    calib = write_tum_sequence(src, str(seq))
    cfg_path = _write_configs(tmp_path, seq, calib)
    monkeypatch.chdir(tmp_path / "data")                     # the inherit_from resolves against the config's ancestors, not the cwd
    cfg = load_config(cfg_path)
    assert cfg["Training"]["tracking_itr_num"] == 40 and cfg["Training"]["window_size"] == 8
    ds = load_dataset(cfg, "cuda:0")
    assert isinstance(ds, TUMDataset) and len(ds) == 32 and not hasattr(ds, "gt_flow")
    assert (ds.width, ds.height, ds.fx, ds.cy, ds.fovx) == (src.width, src.height, src.fx, src.cy, src.fovx)
    torch.testing.assert_close(ds.projection_matrix, src.projection_matrix)
    _check_frames(ds, src, [0, 1, 17, 31])
    assert _reader_threads()
    ds.close()
    assert not _reader_threads() and ds._reader.pool is None
    torch.manual_seed(0)
    ds = load_dataset(cfg, "cuda:0")
    slam = SLAM(cfg, ds, save_dir=str(tmp_path / "out"))
    res = slam.run()
    st = ds.ingest_stats
    print(res, st)
    assert res["frames"] == 32 and len(res["keyframes"]) >= 4
    assert st["prefetched"] >= 28 and st["decode_ms_mean"] > 0
    assert res["ate_rmse"] < 0.0115, res
    assert res["before_opt"]["mean_psnr"] > 33.7 and res["before_opt"]["l1_depth"] < 0.0195, res
    del slam, ds


def test_dynamic_tum_sequence_with_masks(tmp_path):
    """test_slam_dynamic_sequence_end_to_end's sequence with render_mask/ PNGs written from the synthetic motion masks (no gt_flow: the
    flow term is skipped). Measured on MI355X: ATE 8.4 mm, PSNR 27.4 dB, depth L1 27.5 mm, 663 dynamic Gaussians; bars ~20 % off."""
    from slam.config import apply_cli_overrides, load_config
    from slam.dataset import SyntheticRGBDDataset
    from slam.recorded import load_dataset, write_tum_sequence
    from slam.system import SLAM
    torch.manual_seed(0)
    src = SyntheticRGBDDataset(num_frames=30, width=320, height=240, seed=1, dynamic=True, dystart=6)
    seq = tmp_path / "data" / "dyn"
    calib = write_tum_sequence(src, str(seq), masks=True)
    cfg = apply_cli_overrides(load_config(_write_configs(tmp_path, seq, calib, {"dystart": 6})), dynamic=True)
    ds = load_dataset(cfg, "cuda:0")
    _check_frames(ds, src, [0, 5, 6, 12, 29])
    assert not bool(ds[12][3].all())                         # the moving object is in the mask
    slam = SLAM(cfg, ds)
    res = slam.run()
    g = slam.gaussians
    print(res, ds.ingest_stats, int(g.dygs.sum()))
    assert res["frames"] == 30 and g.deform_init and int(g.dygs.sum()) > 50
    assert res["ate_rmse"] < 0.0101, res
    assert res["before_opt"]["mean_psnr"] > 26.4 and res["before_opt"]["l1_depth"] < 0.033, res


def test_cofusion_frame_loads_equal_to_its_source(tmp_path):
    from slam.dataset import SyntheticRGBDDataset
    from slam.recorded import CoFusionDataset, load_dataset, pose_from_tum, rotation_to_quaternion
    src = SyntheticRGBDDataset(num_frames=2, width=160, height=120, seed=1, dynamic=True, dystart=0)
    root = tmp_path / "car"
    for d in ("colour", "depth", "mask_colour", "trajectories"):
        os.makedirs(root / d)
    lines = []
    for i in range(2):
        c, d, p, m = src[i]
        Image.fromarray(np.rint(c.permute(1, 2, 0).cpu().numpy().astype(np.float64) * 255).astype(np.uint8)).save(root / "colour" / f"Color{i:04d}.png")
        Image.fromarray(np.rint(np.asarray(d, np.float64) * 1000).astype(np.uint16)).save(root / "depth" / f"Depth{i:04d}.png")
        Image.fromarray(np.where(m.cpu().numpy(), 0, 255).astype(np.uint8)).save(root / "mask_colour" / f"Mask{i:04d}.png")
        c2w = np.linalg.inv(p.double().cpu().numpy())
        lines.append(f"{i} " + " ".join(f"{v:.12f}" for v in (*c2w[:3, 3], *rotation_to_quaternion(c2w[:3, :3]))))
    (root / "trajectories" / "gt-cam-0.txt").write_text("\n".join(lines) + "\n")
    cal = {"fx": src.fx, "fy": src.fy, "cx": src.cx, "cy": src.cy, "width": 160, "height": 120, "depth_scale": 1000.0, "start": 1, "end": -1}
    ds = load_dataset({"Dataset": {"type": "CoFusion", "dataset_path": str(root), "Calibration": cal}}, "cuda:0")
    assert isinstance(ds, CoFusionDataset) and len(ds) == 1
    image, depth, pose, motion = ds[0]
    c, d, p, m = src[1]
    q = np.rint(c.cpu().numpy().astype(np.float64) * 255)
    assert np.array_equal(image.cpu().numpy().view(np.uint32), (q / 255.0).astype(np.float32).view(np.uint32))
    u16 = np.rint(np.asarray(d, np.float64) * 1000).astype(np.uint16)
    assert np.array_equal(depth, u16.astype(np.float32) / np.float32(1000.0))
    assert torch.equal(motion, m)
    np.testing.assert_allclose(pose.cpu().numpy(), p.cpu().numpy(), atol=1e-6)
    assert np.abs(pose_from_tum([float(x) for x in lines[1].split()]) - p.double().cpu().numpy()).max() < 1e-6
    ds.close()
