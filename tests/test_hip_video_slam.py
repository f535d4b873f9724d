"""A plain video as a SLAM input (Dataset.type 'video', slam/recorded.py VideoDataset): the frames of a Motion-JPEG AVI file, or of a folder
of .jpg files, decoded on the device are exactly libjpeg's pictures pushed through the byte table every dataset uses, in any read order; and
the monocular run on such a file needs no ground truth, leaves its trajectory in TUM format and tracks no worse than twice the error of the
same configuration fed from memory."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import util  # noqa: F401  (puts the repo and the package on sys.path)
from test_hip_mono import _NoDepth, _mono_config

pytestmark = pytest.mark.gpu

FRAMES, W, H, FPS, QUALITY = 20, 160, 120, 30.0, 95


def _memory_dataset():
    from slam.dataset import SyntheticRGBDDataset
    return SyntheticRGBDDataset(num_frames=FRAMES, width=W, height=H, seed=0)


@pytest.fixture(scope="module")
def video(tmp_path_factory):
    """The synthetic sequence as clip.avi and as a folder of .jpg files, both written by the device encoder at quality 95; the files' bytes and
    the ground-truth camera-to-world poses the video itself does not carry."""
    from slam import mjpeg
    root = tmp_path_factory.mktemp("video")
    ds = _memory_dataset()
    dev = torch.device("cuda:0")
    frames = [ds[i] for i in range(FRAMES)]
    rgb = torch.stack([torch.round(f[0].clamp(0, 1).permute(1, 2, 0) * 255).to(torch.uint8) for f in frames]).contiguous()
    q = mjpeg.quant_tables(QUALITY)
    scan = torch.zeros((FRAMES, W * H * 3), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(FRAMES, dtype=torch.int32, device=dev)
    mjpeg.jpeg_encode(rgb, torch.from_numpy(q.astype(np.int16)).to(dev), scan, sizes)
    sizes = sizes.cpu().numpy()
    assert (sizes > 0).all()
    files = [mjpeg.jfif_header(W, H, q) + scan[k, :sizes[k]].cpu().numpy().tobytes() + mjpeg.EOI for k in range(FRAMES)]
    avi, folder = str(root / "clip.avi"), str(root / "frames")
    os.makedirs(folder)
    with mjpeg.AviWriter(avi, W, H, FPS) as out:
        for k, data in enumerate(files):
            out.add(data)
            with open(os.path.join(folder, f"{k:05d}.jpg"), "wb") as f:
                f.write(data)
    calibration = {"fx": float(ds.fx), "fy": float(ds.fy), "cx": float(ds.cx), "cy": float(ds.cy), "width": W, "height": H, "distorted": False}
    gt = [np.linalg.inv(f[2].double().cpu().numpy()) for f in frames]
    return {"avi": avi, "folder": folder, "files": files, "calibration": calibration, "gt_c2w": gt, "root": root}


def _config(video, path, **dataset):
    from slam.system import merge_config
    return merge_config(_mono_config(), {"Dataset": {"type": "video", "dataset_path": path, "Calibration": dict(video["calibration"]), **dataset}})


def _expected_image(data):
    """[3, H, W] float32: PIL's decode through the byte table of the datasets (float32(b / 255) computed in double)."""
    from slam.recorded import byte_lut
    rgb = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
    return torch.from_numpy(byte_lut()[rgb]).permute(2, 0, 1).contiguous()


@pytest.mark.parametrize("kind", ["avi", "folder"])
def test_frames_equal_pil_through_the_byte_table(video, kind):
    from slam.recorded import VideoDataset, load_dataset
    ds = load_dataset(_config(video, video[kind]), "cuda:0", prefetch=4)
    try:
        assert isinstance(ds, VideoDataset) and len(ds) == FRAMES and ds.has_ground_truth is False
        assert ds.stamps == [k / FPS if kind == "avi" else float(k) for k in range(FRAMES)]
        in_order = []
        for k in range(FRAMES):
            image, depth, pose, motion = ds[k]
            assert depth is None
            assert torch.equal(pose.cpu(), torch.eye(4))
            assert motion.dtype == torch.bool and bool(motion.all())
            assert torch.equal(image.cpu(), _expected_image(video["files"][k])), k
            in_order.append(image.cpu())
        for k in (13, 2, 19, 0, 7, 7, 18, 3):                            # as evaluation reads: any order, again
            assert torch.equal(ds[k][0].cpu(), in_order[k]), k
        stats = ds.ingest_stats
        assert stats["device_decoded"] >= FRAMES and stats["device_decode_ms_per_frame"] > 0 and stats["device_decode_chunk"] == 4
    finally:
        ds.close()


def test_chunk_of_one_and_start_end(video):
    from slam.recorded import load_dataset
    cfg = _config(video, video["avi"])
    cfg["Dataset"]["Calibration"].update(start=3, end=9)
    ds = load_dataset(cfg, "cuda:0", prefetch=1, max_frames=4)
    try:
        assert len(ds) == 4 and ds.stamps == [k / FPS for k in range(3, 7)]
        for k in (3, 0, 1, 2):
            assert torch.equal(ds[k][0].cpu(), _expected_image(video["files"][3 + k]))
    finally:
        ds.close()


def test_refused_configurations(video):
    from slam.recorded import load_dataset
    with pytest.raises(ValueError, match="needs Dataset.sensor_type 'monocular', got 'depth'"):
        load_dataset(_config(video, video["avi"], sensor_type="depth"), "cuda:0")
    cfg = _config(video, video["avi"])
    cfg["Dataset"]["Calibration"]["width"] = 320
    with pytest.raises(ValueError, match="the video is 160 x 120, the calibration says 320 x 120"):
        load_dataset(cfg, "cuda:0")
    cfg = _config(video, video["folder"])
    cfg["Dataset"]["Calibration"]["height"] = 128
    with pytest.raises(ValueError, match="00000.jpg: the picture is 160 x 120, the calibration says 160 x 128"):
        load_dataset(cfg, "cuda:0")
    with pytest.raises(FileNotFoundError, match="no such video file or folder"):
        load_dataset(_config(video, str(video["root"] / "missing.avi")), "cuda:0")


def _run(config, ds, save_dir=None):
    from slam.system import SLAM
    torch.manual_seed(0)
    slam = SLAM(config, ds, save_dir=save_dir)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)              # the seeding noise, as tests/test_hip_mono.py
    return slam, slam.run()


@pytest.fixture(scope="module")
def memory_run():
    """The same configuration fed from memory with the depth withheld: the monocular path as it was before video input (first frame at the
    ground-truth pose, ATE by eval_ate). Returns its scale-aligned ATE RMSE."""
    _, res = _run(_mono_config(), _NoDepth(_memory_dataset()))
    return float(res["ate_rmse"])


def test_monocular_run_on_the_video_file(video, memory_run, tmp_path):
    """Measured on MI355X: ATE RMSE after the Sim(3) fit 0.018398 m from the video, 0.015644 m from memory (bar: twice the latter, 0.031288 m)."""
    from slam.eval_utils import _pose_c2w, ate_sim3
    from slam.recorded import load_dataset, pose_from_tum
    save_dir = str(tmp_path / "run")
    os.makedirs(save_dir)
    ds = load_dataset(_config(video, video["avi"]), "cuda:0")
    try:
        slam, res = _run(_config(video, video["avi"]), ds, save_dir=save_dir)
    finally:
        ds.close()
    fe = slam.frontend
    assert res["frames"] == FRAMES and res["ate_rmse"] is None and res["ground_truth"] is False
    assert not os.path.exists(os.path.join(save_dir, "plot"))                        # no ATE was computed or written
    est = [_pose_c2w(fe.cameras[i].R, fe.cameras[i].T) for i in sorted(fe.cameras)]
    assert all(np.isfinite(p).all() for p in est)
    assert np.allclose(est[0], np.eye(4), atol=1e-6)                                 # the map's frame is the first camera's
    with open(os.path.join(save_dir, "trajectory.txt")) as f:
        rows = [line.split() for line in f if not line.startswith("#")]
    assert len(rows) == FRAMES and all(len(r) == 8 for r in rows)
    values = np.array([[float(v) for v in r] for r in rows])
    assert np.allclose(values[:, 0], np.arange(FRAMES) / FPS, atol=1e-6)
    assert np.allclose(np.linalg.norm(values[:, 4:], axis=1), 1.0, atol=1e-9)
    back = [np.linalg.inv(pose_from_tum(v)) for v in values]                         # the TUM reader of the other loaders
    assert np.allclose(np.stack(back)[:, :3, 3], np.stack(est)[:, :3, 3], atol=1e-6)
    assert np.allclose(np.stack(back)[:, :3, :3], np.stack(est)[:, :3, :3], atol=1e-6)
    ate = ate_sim3(video["gt_c2w"], back)[0]
    print(f"ATE RMSE after the Sim(3) fit: video {ate:.6f} m, memory {memory_run:.6f} m, bar {2 * memory_run:.6f} m")
    assert ate <= 2 * memory_run, (ate, memory_run)


def test_saved_map_of_a_video_run_has_no_ground_truth(video, tmp_path):
    from slam import map_io
    ds = load_dataset_short(video)
    try:
        cfg = _config(video, video["avi"])
        cfg["Results"]["eval_rendering"] = False
        slam, res = _run(cfg, ds, save_dir=str(tmp_path))
        assert res["ate_rmse"] is None and os.path.isfile(res["trajectory"])
        state = np.load(os.path.join(slam.save_map(), map_io.STATE))
        assert not state["frame_has_gt"].any()
    finally:
        ds.close()


def load_dataset_short(video):
    from slam.recorded import load_dataset
    return load_dataset(_config(video, video["avi"]), "cuda:0", max_frames=5)
