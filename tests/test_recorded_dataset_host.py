"""Host side of the recorded-sequence loaders (slam/config.py, slam/recorded.py): configuration inheritance, TUM / Bonn and CoFusion
path parsing, pose conversion, mask indexing, start / end slicing, the errors, the undistortion map and host decoding. No GPU."""
import os
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import recorded  # noqa: E402
from slam.config import apply_cli_overrides, load_config  # noqa: E402
from slam.system import default_config  # noqa: E402


def _yaml(path, doc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        yaml.safe_dump(doc, f)


# ---- configuration ---------------------------------------------------------------------------------------------------------------
def test_inherit_chain_across_directories(tmp_path, monkeypatch):
    root = tmp_path / "checkout"
    # base <- mid (names base relative to the checkout root: an ANCESTOR of its own directory) <- leaf (names mid relative to itself)
    _yaml(str(root / "configs/rgbd/base_config.yaml"),
          {"Dataset": {"type": "tum", "pcd_downsample": 64, "Calibration": {"fx": 1.0, "fy": 2.0}}, "Training": {"kf_interval": 7, "alpha": 0.5}})
    _yaml(str(root / "configs/rgbd/tum/mid.yaml"),
          {"inherit_from": "configs/rgbd/base_config.yaml", "Dataset": {"Calibration": {"fy": 3.0, "cx": 4.0}}, "Training": {"alpha": 0.6}})
    _yaml(str(root / "runs/seq/leaf.yaml"),
          {"inherit_from": "../../configs/rgbd/tum/mid.yaml", "Dataset": {"dataset_path": "/data/seq"}, "Training": {"alpha": 0.7}})
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    monkeypatch.chdir(elsewhere)
    cfg = load_config(str(root / "runs/seq/leaf.yaml"))
    assert cfg["Dataset"]["Calibration"] == {"fx": 1.0, "fy": 3.0, "cx": 4.0}
    assert cfg["Training"]["alpha"] == 0.7 and cfg["Training"]["kf_interval"] == 7
    assert cfg["Dataset"]["type"] == "tum" and cfg["Dataset"]["pcd_downsample"] == 64 and cfg["Dataset"]["dataset_path"] == "/data/seq"
    d = default_config()
    # keys only this project has (and the reference's keys the files do not set) keep their defaults
    assert cfg["Training"]["window_size"] == d["Training"]["window_size"] and cfg["opt_params"] == d["opt_params"]
    assert "inherit_from" in cfg          # the reference keeps the key too (update_recursive copies it)
    # the path as given wins when it exists from the working directory
    monkeypatch.chdir(root)
    assert load_config("runs/seq/leaf.yaml")["Dataset"]["Calibration"]["fy"] == 3.0


def test_inherit_missing_names_the_path(tmp_path, monkeypatch):
    _yaml(str(tmp_path / "a/leaf.yaml"), {"inherit_from": "configs/nope.yaml"})
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="configs/nope.yaml"):
        load_config(str(tmp_path / "a/leaf.yaml"))


def test_cli_overrides_follow_slam_py():
    cfg = apply_cli_overrides(default_config(), eval=True, dynamic=True)
    r = cfg["Results"]
    assert (r["save_results"], r["use_gui"], r["eval_rendering"], r["use_wandb"]) == (True, False, True, False)
    assert cfg["model_params"]["dynamic_model"] is True
    cfg = default_config()
    cfg["Results"]["use_gui"] = True
    cfg["model_params"]["dynamic_model"] = True
    apply_cli_overrides(cfg)
    assert cfg["Results"]["use_gui"] is True and cfg["model_params"]["dynamic_model"] is False


# ---- TUM / Bonn ------------------------------------------------------------------------------------------------------------------
def _quat_w2c(t, q_xyzw):
    """Direct restatement: R of the normalised quaternion, W2C = [R^T | -R^T t]."""
    x, y, z, w = np.asarray(q_xyzw, np.float64) / np.linalg.norm(q_xyzw)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ np.asarray(t)
    return out


def _gt_motion(ts):
    """A smooth ground-truth trajectory: (t, q_xyzw) at time ts (the quaternion is deliberately not unit length)."""
    a = ts - 100.0
    return np.array([0.3 * a, -0.1 * a, 0.05 + 0.2 * a]), np.array([0.1 * np.sin(a), 0.2 * a, -0.05, 1.3])


def _write_tum(root, n_masks=None):
    """rgb at 30 Hz (rows with comment lines), one extra frame 10 ms after row 3 (dropped by the 32 Hz subsampling), a last frame
    without depth within 0.08 s; depth jittered by a few ms; poses at 100 Hz with the TUM header."""
    os.makedirs(root, exist_ok=True)
    t_rgb = [100.0 + i / 30.0 for i in range(10)]
    t_rgb.insert(4, t_rgb[3] + 0.01)
    t_rgb.append(t_rgb[-1] + 0.15)
    with open(os.path.join(root, "rgb.txt"), "w") as f:
        f.write("# color images\n# file: 'seq.bag'\n# timestamp filename\n")
        for i, t in enumerate(t_rgb):
            f.write(f"{t:.6f} rgb/{t:.6f}.png\n")
            if i == 5:
                f.write("# a comment in the middle\n")
    rng = np.random.default_rng(3)
    t_depth = [t + rng.uniform(-0.006, 0.006) for t in t_rgb[:-1]]
    with open(os.path.join(root, "depth.txt"), "w") as f:
        f.write("# depth maps\n# file: 'seq.bag'\n# timestamp filename\n")
        for t in t_depth:
            f.write(f"{t:.6f} depth/{t:.6f}.png\n")
    t_pose = np.arange(99.9, t_rgb[-1] + 0.2, 0.01)
    with open(os.path.join(root, "groundtruth.txt"), "w") as f:
        f.write("# ground truth trajectory\n# file: 'seq.bag'\n# timestamp tx ty tz qx qy qz qw\n")
        for t in t_pose:
            tr, q = _gt_motion(t)
            f.write(f"{t:.4f} " + " ".join(f"{v:.9f}" for v in (*tr, *q)) + "\n")
    if n_masks:
        os.makedirs(os.path.join(root, "render_mask"))
        for k in range(n_masks):
            Image.fromarray(np.full((2, 2), k, np.uint8)).save(os.path.join(root, "render_mask", f"mask_{k}.png"))
    return t_rgb, t_depth, t_pose


def test_tum_parsing_association_and_poses(tmp_path):
    root = str(tmp_path / "seq")
    t_rgb, t_depth, t_pose = _write_tum(root)
    fl = recorded.parse_tum(root)
    kept_rows = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]           # row 4 is 10 ms after row 3 (< 1/32 s), row 11 has no depth within 0.08 s
    assert len(fl) == len(kept_rows) and fl.mask_paths is None
    for n, i in enumerate(kept_rows):
        assert fl.color_paths[n] == os.path.join(root, f"rgb/{t_rgb[i]:.6f}.png")
        assert fl.depth_paths[n] == os.path.join(root, f"depth/{t_depth[i]:.6f}.png")
        k = int(np.argmin(np.abs(np.round(t_pose, 4) - t_rgb[i])))
        tr, q = _gt_motion(float(f"{t_pose[k]:.4f}"))
        want = _quat_w2c(np.round(tr, 9), np.round(q, 9))
        np.testing.assert_allclose(fl.poses[n], want, rtol=0, atol=1e-12)
    # pose.txt is read when groundtruth.txt is absent; its FIRST line is skipped even when it is data
    os.rename(os.path.join(root, "groundtruth.txt"), os.path.join(root, "pose.txt"))
    lines = open(os.path.join(root, "pose.txt")).read().splitlines()
    open(os.path.join(root, "pose.txt"), "w").write("\n".join(lines[2:]) + "\n")      # first line is now a comment, dropped as the header
    assert len(recorded.parse_tum(root)) == len(kept_rows)
    open(os.path.join(root, "pose.txt"), "w").write("\n".join(lines[3:]) + "\n")      # first line is data and is skipped all the same
    fl2 = recorded.parse_tum(root)
    np.testing.assert_array_equal(fl2.poses, fl.poses)


def test_tum_masks_by_rgb_row_and_slicing(tmp_path):
    root = str(tmp_path / "seq")
    _write_tum(root, n_masks=12)
    fl = recorded.parse_tum(root)
    kept_rows = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10]
    # sorted by the trailing number (mask_10 after mask_9, not after mask_1), indexed by rgb.txt row
    assert fl.mask_paths == [os.path.join(root, "render_mask", f"mask_{i}.png") for i in kept_rows]
    s = fl.sliced(2, 6)
    assert s.color_paths == fl.color_paths[2:6] and s.mask_paths == fl.mask_paths[2:6] and s.depth_paths == fl.depth_paths[2:6]
    np.testing.assert_array_equal(s.poses, fl.poses[2:6])
    assert len(fl.sliced(3, -1)) == len(fl) - 3 and fl.sliced(3, -1).mask_paths == fl.mask_paths[3:]
    with pytest.raises(ValueError, match="masks"):
        _write_tum(str(tmp_path / "short"), n_masks=5)
        recorded.parse_tum(str(tmp_path / "short"))


# ---- CoFusion ----------------------------------------------------------------------------------------------------------------------
def _write_cofusion(root, n=4, traj=True, masks=True):
    for d in ("colour", "depth", "mask_colour", "trajectories"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for k in range(n):
        Image.fromarray(np.full((3, 4, 3), 10 * k, np.uint8)).save(os.path.join(root, "colour", f"Color{k:04d}.png"))
        Image.fromarray(np.full((3, 4), 1000 + k, np.uint16)).save(os.path.join(root, "depth", f"Depth{k:04d}.png"))
        if masks:
            Image.fromarray(np.full((3, 4), 255 * (k % 2), np.uint8)).save(os.path.join(root, "mask_colour", f"Mask{k:04d}.png"))
    if traj:
        with open(os.path.join(root, "trajectories", "gt-cam-0.txt"), "w") as f:
            for k in range(n):
                f.write(f"{k} {0.1 * k} 0.2 {-0.3 * k} 0 {0.1 * k} 0 1\n")


def test_cofusion_listing(tmp_path):
    root = str(tmp_path / "car")
    _write_cofusion(root)
    fl = recorded.parse_cofusion(root)
    assert len(fl) == 4 and fl.depth_float32
    assert fl.color_paths == [os.path.join(root, "colour", f"Color{k:04d}.png") for k in range(4)]
    assert fl.depth_paths == [os.path.join(root, "depth", f"Depth{k:04d}.png") for k in range(4)]
    assert fl.mask_paths == [os.path.join(root, "mask_colour", f"Mask{k:04d}.png") for k in range(4)]
    for k in range(4):
        np.testing.assert_allclose(fl.poses[k], _quat_w2c([0.1 * k, 0.2, -0.3 * k], [0, 0.1 * k, 0, 1]), rtol=0, atol=1e-12)
    s = fl.sliced(1, 3)
    assert s.color_paths == fl.color_paths[1:3] and s.mask_paths == fl.mask_paths[1:3] and s.depth_float32
    root2 = str(tmp_path / "room")
    _write_cofusion(root2, traj=False, masks=False)
    fl2 = recorded.parse_cofusion(root2)
    assert fl2.mask_paths is None and all(np.array_equal(p, np.eye(4)) for p in fl2.poses)


def test_unknown_type_and_exr_errors(tmp_path):
    with pytest.raises(ValueError, match="'tum'.*'CoFusion'"):
        recorded.load_dataset({"Dataset": {"type": "replica"}}, device="cpu")
    root = str(tmp_path / "car")
    _write_cofusion(root)
    os.makedirs(os.path.join(root, "depth_noise"))
    open(os.path.join(root, "depth_noise", "Depth0000.exr"), "wb").close()
    cfg = {"Dataset": {"type": "CoFusion", "dataset_path": root, "Calibration": {"fx": 1, "fy": 1, "cx": 1, "cy": 1, "width": 4, "height": 3,
                                                                                "depth_scale": 1.0}}}
    with pytest.raises(NotImplementedError, match="EXR"):
        recorded.load_dataset(cfg, device="cpu")


# ---- undistortion map, byte table, host decoding ---------------------------------------------------------------------------------
def test_undistort_map_closed_form():
    W, H = 64, 48
    fx, fy, cx, cy = 54.2822841, 54.257687, 31.559352, 23.7756098
    k1, k2, p1, p2, k3 = 0.039903, -0.099343, -0.00073, -0.000144, 0.01
    m = recorded.undistort_map(W, H, fx, fy, cx, cy, k1, k2, p1, p2, k3)
    assert m.shape == (H, W, 2) and m.dtype == np.float32
    for (v, u) in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (17, 29), (24, 31)):
        x, y = (u - cx) / fx, (v - cy) / fy
        r2 = x * x + y * y
        kr = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        mx = fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
        my = fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
        np.testing.assert_allclose(m[v, u].astype(np.float64), [mx, my], rtol=0, atol=4e-6)   # float32 storage of the float64 value
    ident = recorded.undistort_map(W, H, fx, fy, cx, cy)
    v, u = np.mgrid[0:H, 0:W]
    np.testing.assert_allclose(ident[..., 0], u, atol=1e-5)
    np.testing.assert_allclose(ident[..., 1], v, atol=1e-5)
    lut = recorded.byte_lut()
    assert lut.dtype == np.float32 and lut[0] == 0 and lut[255] == 1
    assert np.array_equal(lut, np.array([np.float32(b / 255.0) for b in range(256)], np.float32))


def test_host_decode_depth_dtypes_and_mask(tmp_path):
    root = str(tmp_path / "seq")
    _write_tum(root, n_masks=12)
    fl = recorded.parse_tum(root)
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8)
    dep = rng.integers(0, 65536, (3, 4), dtype=np.uint16)
    msk = rng.integers(0, 256, (3, 4, 3), dtype=np.uint8)           # an RGB mask: converted to L like the reference
    for p in (fl.color_paths[0], fl.depth_paths[0], fl.mask_paths[0]):
        os.makedirs(os.path.dirname(p), exist_ok=True)
    Image.fromarray(rgb).save(fl.color_paths[0])
    Image.fromarray(dep).save(fl.depth_paths[0])
    Image.fromarray(msk).save(fl.mask_paths[0])
    hf = recorded.decode_frame(fl, 0, 4, 3, 5000.0)
    assert np.array_equal(hf.rgb, rgb)
    assert np.array_equal(hf.mask, np.asarray(Image.fromarray(msk).convert("L")))
    assert hf.depth.dtype == np.float32 and np.array_equal(hf.depth, (dep / 5000.0).astype(np.float32))
    fl.depth_float32 = True                                         # CoFusion: float32(depth) / scale in float32
    hf = recorded.decode_frame(fl, 0, 4, 3, 3.0)
    assert np.array_equal(hf.depth, dep.astype(np.float32) / np.float32(3.0))
    with pytest.raises(ValueError, match="calibration says"):
        recorded.decode_frame(fl, 0, 5, 3, 5000.0)
