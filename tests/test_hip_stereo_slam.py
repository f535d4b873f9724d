"""Stereo depth in the SLAM loop: a pair rendered by the synthetic generator (slam/dataset.py right_view) matched on the device against
its ground-truth depth, and a short sequence written in the EuRoC layout (recorded.write_euroc_sequence), loaded through load_dataset
(EurocDataset) and run through SLAM, against the same frames with the generator's own depth."""
import os
import sys
import threading

import numpy as np
import pytest
import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu

BASELINE = 0.11
FRAMES = 12


def test_rendered_pair_depth_is_within_one_pixel_of_disparity():
    """320 x 240, baseline 0.11 m. Among the valid pixels that have a ground-truth depth, the median relative depth error stays below
    what ONE pixel of disparity error makes at the scene's median ground-truth disparity d_med: depth = bf / d, so a one-pixel error is a
    relative depth error of 1 / (d_med - 1) (the larger of the two signs). A wrong bf, a wrong sign or a one-pixel shift overshoots this.
    Measured on MI355X: d_med 9.20 px, bar 0.122, median relative error 0.0154, density 0.898 of the pixels with ground truth (0.915 of
    all pixels) with uniqueness 40."""
    from slam import recorded, stereo
    from slam.dataset import SyntheticRGBDDataset
    src = SyntheticRGBDDataset(num_frames=1, width=320, height=240, seed=0)
    color, gt, _, _ = src[0]
    left = torch.tensor(recorded.grey_bytes(color), device=src.device)
    right = torch.tensor(recorded.grey_bytes(src.right_view(0, BASELINE)), device=src.device)
    bf = src.fx * BASELINE
    m = stereo.StereoMatcher(320, 240, bf=bf, device=src.device)
    image, disp, depth = m(left, right)
    torch.cuda.synchronize()
    disp, depth = disp.cpu().numpy(), depth.cpu().numpy()
    assert np.array_equal(image.cpu().numpy()[1], (left.cpu().numpy().astype(np.float64) / 255.0).astype(np.float32))
    assert np.array_equal(depth > 0, disp > 0)
    has_gt = gt > 0
    both = has_gt & (disp > 0)
    d_med = float(np.median(bf / gt[has_gt]))
    bar = 1.0 / (d_med - 1.0)
    rel = np.abs(depth[both] - gt[both]) / gt[both]
    density = both.sum() / has_gt.sum()
    print(f"median gt disparity {d_med:.3f} px, bar {bar:.4f}, median relative depth error {np.median(rel):.4f}, density {density:.4f} "
          f"(of all pixels {float((disp > 0).mean()):.4f})")
    assert d_med > 2.0 and both.sum() > 1000
    assert float(np.median(rel)) < bar


class _GreyWithTrueDepth:
    """The generator's frames as the stereo loader shows them (the grey bytes of the left image, in three channels) with the generator's
    own depth: the run the stereo run is measured against."""

    def __init__(self, src, n):
        self.src, self.num_imgs = src, n
        self.lut = torch.tensor((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32), device=src.device)

    def __getattr__(self, name):
        if name == "gt_flow":
            raise AttributeError(name)
        return getattr(self.src, name)

    def __len__(self):
        return self.num_imgs

    def __getitem__(self, i):
        from slam import recorded
        color, depth, pose, motion = self.src[i]
        grey = self.lut[torch.tensor(recorded.grey_bytes(color), device=self.src.device).long()]
        return grey[None].expand(3, -1, -1).contiguous(), depth, pose, motion


def _config(tmp_path, seq, calibration):
    from test_hip_recorded_slam import QUICK
    base = {"Dataset": {"type": "euroc", "sensor_type": "depth", "pcd_downsample": 32, "pcd_downsample_init": 8},
            "Results": {"save_results": False, "use_gui": False, "eval_rendering": True}, "opt_params": {"densify_from_iter": 100},
            "Training": dict(QUICK)}
    os.makedirs(tmp_path / "configs" / "stereo" / "seq", exist_ok=True)
    with open(tmp_path / "configs" / "stereo" / "base.yaml", "w") as f:
        yaml.safe_dump(base, f)
    path = tmp_path / "configs" / "stereo" / "seq" / "seq.yaml"
    with open(path, "w") as f:
        yaml.safe_dump({"inherit_from": "configs/stereo/base.yaml", "Dataset": {"dataset_path": str(seq), "Calibration": calibration}}, f)
    return str(path)


def test_stereo_sequence_end_to_end(tmp_path):
    """12 frames at 320 x 240 with the quick schedule of test_hip_recorded_slam.py. A1 = ATE of the run on the written stereo sequence (depth
    from the matcher), A0 = ATE of the same frames with the generator's depth and the same grey images; A1 <= K A0 with K = ceil(A1 / A0) + 1
    from one measurement, and K <= 5 by the cap set for this test. Measured on MI355X: A1 = 16.9 mm, A0 = 11.1 mm, ratio 1.53, so K = 3; device
    time 0.79 ms per frame, mean depth density 0.913 ("Stereo depth")."""
    from slam import recorded
    from slam.config import load_config
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM
    K = 3
    src = SyntheticRGBDDataset(num_frames=FRAMES, width=320, height=240, seed=0)
    seq = tmp_path / "data" / "stereo"
    calib = recorded.write_euroc_sequence(src, str(seq), BASELINE)
    cfg = load_config(_config(tmp_path, seq, calib))
    torch.manual_seed(0)
    ds = recorded.load_dataset(cfg, "cuda:0")
    assert isinstance(ds, recorded.EurocDataset) and len(ds) == FRAMES and not hasattr(ds, "gt_flow")
    assert (ds.width, ds.height, ds.fx, ds.cy) == (src.width, src.height, src.fx, src.cy) and ds.bf == pytest.approx(src.fx * BASELINE)
    image, depth, pose, motion = ds[3]
    color, gt, gt_pose, _ = src[3]
    assert image.is_cuda and image.dtype == torch.float32 and image.shape == (3, 240, 320) and bool(motion.all()) and motion.dtype == torch.bool
    assert np.array_equal(image[2].cpu().numpy(), (recorded.grey_bytes(color).astype(np.float64) / 255.0).astype(np.float32))
    assert isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == (240, 320)
    both = (depth > 0) & (gt > 0)
    d_med = float(np.median(ds.bf / gt[gt > 0]))                        # the one-pixel bar of the test above
    assert both.any() and np.median(np.abs(depth[both] - gt[both]) / gt[both]) < 1.0 / (d_med - 1.0)
    assert float((pose - gt_pose).abs().max()) < 1e-5
    slam = SLAM(cfg, ds, save_dir=str(tmp_path / "out"))
    res = slam.run()
    stats = ds.ingest_stats
    a1 = res["ate_rmse"]
    ds.close()
    assert not [t for t in threading.enumerate() if t.name.startswith("frame-decode")] and ds._reader.pool is None
    st = stats["stereo"]
    assert st["frames"] >= FRAMES and st["ms_per_frame"] > 0 and st["num_disparities"] == 64 and st["uniqueness_ratio"] == 40
    assert 0.0 < st["depth_density_mean"] <= 1.0 and st["depth_wait_ms_total"] >= 0
    del slam
    torch.manual_seed(0)
    res0 = SLAM(cfg, _GreyWithTrueDepth(src, FRAMES), save_dir=str(tmp_path / "out0")).run()
    a0 = res0["ate_rmse"]
    print(f"ATE with stereo depth A1 = {a1 * 1e3:.2f} mm, with the generator's depth A0 = {a0 * 1e3:.2f} mm, ratio {a1 / a0:.2f}; stereo {st}")
    assert res["frames"] == FRAMES and res0["frames"] == FRAMES
    assert K <= 5 and a1 <= K * a0, (a1, a0)
