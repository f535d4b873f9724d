"""Host side of the stereo path: the numpy restatement of the matcher (tests/stereo_reference.py) checked against hand-computed cases and
a planted pair, rectify_map, the EuRoC-layout parser and writer and EurocDataset's argument handling (slam/stereo.py, slam/recorded.py).
No GPU."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stereo_reference as ref  # noqa: E402
from slam import recorded, stereo  # noqa: E402


# ---- the reference against hand-computed cases ------------------------------------------------------------------------------------
def test_pure_shift_is_found():
    """right(x) = left(x + k): every valid pixel whose match lies in the right image (x >= k) has d* = k. The stored value is 16 k plus the
    contract's sub-pixel term, at most half a pixel, which is 0 only where S(k - 1) and S(k + 1) are close to equal (about half of these
    pixels; always for k = 0, where no step is taken), so the integer disparity is what is pinned. Left of x = k the true match is outside
    the right image and the few pixels that pass the checks there are not looked at."""
    rng = np.random.default_rng(3)
    H, W = 20, 90
    for k in (0, 7, 31):
        left = rng.integers(0, 256, (H, W), dtype=np.uint8)
        right = rng.integers(0, 256, (H, W), dtype=np.uint8)
        right[:, :W - k] = left[:, k:]
        d16, S = ref.match(left, right)
        region = np.arange(W)[None, :] >= k
        valid = (d16 >= 0) & region
        assert valid.sum() > 0.9 * region.sum() * H, (k, valid.sum())
        assert np.all((d16[valid].astype(np.int64) + 8) // 16 == k), k
        assert np.all(np.abs(d16[valid].astype(np.int64) - 16 * k) <= 8), k
        if k == 0:
            assert np.all(d16[valid] == 0)


HAND_C = np.array([[2, 0, 5], [1, 4, 0], [3, 3, 3]], np.int64)                 # C(p, d) of three pixels on a line, D = 3
# p1 = 1, p2 = 3, walking p0 -> p2:  L = [2 0 5], [2 4 1], [4 4 3];  walking back:  [3 3 3], [1 4 0], [3 1 5]  (in pixel order: [3 1 5],
# [1 4 0], [3 3 3]); the six directions that leave the line at once contribute C each
HAND_FORWARD = np.array([[2, 0, 5], [2, 4, 1], [4, 4, 3]])
HAND_BACKWARD = np.array([[3, 1, 5], [1, 4, 0], [3, 3, 3]])
HAND_S = np.array([[17, 1, 40], [9, 32, 1], [25, 25, 24]])


def test_aggregation_by_hand_on_a_row_and_a_column():
    row = HAND_C[None]                                                           # 1 x 3
    assert np.array_equal(ref.aggregate_direction(row, 1, 0, 1, 3)[0], HAND_FORWARD)
    assert np.array_equal(ref.aggregate_direction(row, -1, 0, 1, 3)[0], HAND_BACKWARD)
    for dx, dy in ((0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)):
        assert np.array_equal(ref.aggregate_direction(row, dx, dy, 1, 3), row)
    assert np.array_equal(ref.aggregate(row, 1, 3)[0], HAND_S)
    col = HAND_C[:, None]                                                        # 3 x 1
    assert np.array_equal(ref.aggregate_direction(col, 0, 1, 1, 3)[:, 0], HAND_FORWARD)
    assert np.array_equal(ref.aggregate_direction(col, 0, -1, 1, 3)[:, 0], HAND_BACKWARD)
    for dx, dy in ((1, 0), (-1, 0), (1, 1), (-1, 1), (1, -1), (-1, -1)):
        assert np.array_equal(ref.aggregate_direction(col, dx, dy, 1, 3), col)
    assert np.array_equal(ref.aggregate(col, 1, 3)[:, 0], HAND_S)


def test_diagonals_restart_at_the_side_borders():
    """On a 2 x 2 image the (1, 1) path through pixel (1, 1) comes from (0, 0); pixels (0, 1) and (1, 0) have no predecessor."""
    C = np.arange(2 * 2 * 3, dtype=np.int64).reshape(2, 2, 3) * 3 % 7
    L = ref.aggregate_direction(C, 1, 1, 1, 3)
    assert np.array_equal(L[0], C[0]) and np.array_equal(L[1, 0], C[1, 0])
    assert np.array_equal(L[1, 1], ref._step(C[1, 1], C[0, 0], 1, 3))
    L = ref.aggregate_direction(C, -1, 1, 1, 3)
    assert np.array_equal(L[0], C[0]) and np.array_equal(L[1, 1], C[1, 1])
    assert np.array_equal(L[1, 0], ref._step(C[1, 0], C[0, 1], 1, 3))


def test_subpixel_division_truncates():
    assert [ref.trunc_div(a, 52) for a in (-358, -52, -51, -1, 0, 51, 52, 358)] == [-6, -1, 0, 0, 0, 0, 1, 6]
    S = np.full((1, 4, 4), 50, np.int64)
    S[0, 3] = [50, 6, 5, 30]              # d* = 2: den = 6 + 30 - 10 = 26, ((6 - 30) 16 + 26) / 52 = -358 / 52 -> -6 (floor would be -7)
    assert ref.select(S, 0, -1)[0, 3] == 32 - 6
    S[0, 3] = [50, 10, 5, 9]              # den = 9, (16 + 9) / 18 -> 1
    assert ref.select(S, 0, -1)[0, 3] == 33
    S[0, 3] = [50, 5, 5, 5]               # first minimum d* = 1: den = max(50 + 5 - 10, 1) = 45, ((50 - 5) 16 + 45) / 90 = 8
    assert ref.select(S, 0, -1)[0, 3] == 16 + 8
    S[0, 3] = [50, 60, 70, 5]             # d* = D - 1: no sub-pixel step
    assert ref.select(S, 0, -1)[0, 3] == 48
    S[0, 1] = [50, 50, 5, 50]             # x - d* < 0
    assert ref.select(S, 0, -1)[0, 1] == -16


def test_selection_rules():
    S = np.full((1, 6, 4), 100, np.int64)
    S[0, 5] = [100, 100, 50, 79]          # 79 is next to d*: not a rival
    assert ref.select(S, 40, -1)[0, 5] >= 0
    S[0, 5] = [83, 100, 50, 100]          # 83 * 60 = 4980 < 5000: a rival two steps away
    assert ref.select(S, 40, -1)[0, 5] == -16
    S[0, 5] = [84, 100, 50, 100]          # 84 * 60 = 5040: not below
    assert ref.select(S, 40, -1)[0, 5] >= 0
    # left-right check: pixel 5 picks d* = 2 -> right pixel 3, whose candidates are S(3, 0), S(4, 1), S(5, 2) = 100, 100, 50 -> dR = 2
    assert ref.select(S, 40, 0)[0, 5] >= 0
    S[0, 3, 0] = 10                        # ... now dR(3) = 0: |0 - 2| > 1
    assert ref.select(S, 40, 1)[0, 5] == -16 and ref.select(S, 40, 2)[0, 5] >= 0 and ref.select(S, 40, -1)[0, 5] >= 0


def test_constant_image_ties_go_to_the_first_minimum():
    img = np.full((9, 70), 128, np.uint8)
    d16, S = ref.match(img, img)
    assert np.all(S[..., 0] == 0) and np.all(d16 == 0)
    assert np.all(ref.depth_from_disparity(d16, 40.0) == 0)
    assert np.all(S[:, :5, 5:] > 0)                                             # C = 62 where x - d < 0


def test_depth_is_one_float32_division():
    d16 = np.array([[-16, 0, 1, 16, 257, 1023 * 16]], np.int16)
    out = ref.depth_from_disparity(d16, 47.90639384423901)
    bf16 = np.float32(47.90639384423901 * 16.0)
    assert out.dtype == np.float32 and out[0, 0] == 0 and out[0, 1] == 0
    assert np.array_equal(out[0, 2:], bf16 / np.array([1, 16, 257, 1023 * 16], np.float32))


@pytest.mark.parametrize("seed", [0, 1])
def test_planted_pair_aggregation_beats_winner_take_all(seed):
    """The paths must help: higher density AND a lower share of valid pixels more than 1 px off than winner-take-all on the raw cost under
    the same selection rules. Values of this reference (seed 0 / 1): matcher density 0.877 / 0.876, bad share 0.0005 / 0.0005; raw cost
    0.521 / 0.561 and 0.022 / 0.017."""
    left, right, truth, evaluated = ref.planted_pair(seed=seed)
    assert left.shape == (48, 112) and evaluated.sum() > 0.8 * evaluated.size
    d_sgm, _ = ref.match(left, right, **ref.DEFAULTS)
    d_wta, _ = ref.match(left, right, aggregated=False, **ref.DEFAULTS)
    (dens, bad), (dens0, bad0) = ref.quality(d_sgm, truth, evaluated), ref.quality(d_wta, truth, evaluated)
    print(f"seed {seed}: matcher density {dens:.4f} bad {bad:.4f}; winner-take-all density {dens0:.4f} bad {bad0:.4f}")
    assert dens > dens0 and bad < bad0


# ---- rectify_map -------------------------------------------------------------------------------------------------------------------
def test_rectify_map_without_rotation_is_undistort_map():
    W, H, fx, fy, cx, cy = 75, 48, 61.3, 60.1, 36.2, 24.9
    dist = (-0.28, 0.07, 2e-4, -3e-4, 0.01)
    K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]
    a = stereo.rectify_map(K, dist, np.eye(3), K, W, H)
    b = recorded.undistort_map(W, H, fx, fy, cx, cy, *dist)
    assert a.dtype == np.float32 and a.shape == (H, W, 2)
    np.testing.assert_array_max_ulp(a, b, maxulp=1)


def test_rectify_map_without_distortion_is_a_homography():
    W, H = 60, 40
    K_raw = np.array([[58.0, 0, 30.5], [0, 57.0, 19.5], [0, 0, 1]])
    K_opt = np.array([[50.0, 0, 29.0], [0, 50.0, 21.0], [0, 0, 1]])
    ax, ay, az = 0.01, -0.02, 0.015
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    Rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    R = Rz @ Ry @ Rx
    m = stereo.rectify_map(K_raw, np.zeros(5), R, K_opt, W, H, dtype=np.float64)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    q = np.stack([u, v, np.ones_like(u)], -1) @ (K_raw @ np.linalg.inv(R) @ np.linalg.inv(K_opt)).T
    assert np.abs(m - q[..., :2] / q[..., 2:]).max() < 1e-9
    assert np.abs(m - np.stack([u, v], -1)).max() > 0.5                          # and it is not the identity


# ---- the EuRoC layout --------------------------------------------------------------------------------------------------------------
STAMPS = [1403636579763555584, 1403636579813555456, 1403636579863555584, 1403636579913555456]
S2 = np.sqrt(0.5)
# csv rows: stamp offset (ns) from a frame, position, quaternion w x y z
POSE_ROWS = [(STAMPS[0] - 2_000_000, (1.0, 2.0, 3.0), (1.0, 0.0, 0.0, 0.0)),          # nearest to frame 0
             (STAMPS[0] + 20_000_000, (9.0, 9.0, 9.0), (0.0, 1.0, 0.0, 0.0)),         # 20 ms from frame 0, 30 ms from frame 1: nobody's nearest
             (STAMPS[1] + 1_000_000, (0.5, -1.0, 2.0), (S2, 0.0, 0.0, S2)),            # frame 1: 90 degrees about z
             (STAMPS[2] - 3_000_000, (-2.0, 0.0, 1.0), (S2, S2, 0.0, 0.0)),            # frame 2: 90 degrees about x
             (STAMPS[3] + 4_000_000, (0.0, 4.0, 0.0), (0.0, 0.0, 2.0, 0.0))]           # frame 3: 180 degrees about y, not normalised
ROTATIONS = {0: np.eye(3), 1: np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), 2: np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]]),
             3: np.array([[-1.0, 0, 0], [0, 1, 0], [0, 0, -1]])}
ROW_OF_FRAME = {0: 0, 1: 2, 2: 3, 3: 4}


def _write_euroc(root, n_right=4, csv=True, shuffle=False):
    for cam, n in (("cam0", 4), ("cam1", n_right)):
        os.makedirs(root / "mav0" / cam / "data")
        order = STAMPS[:n][::-1] if shuffle else STAMPS[:n]
        for k, s in enumerate(order):
            Image.fromarray(np.full((6, 8), 10 * STAMPS.index(s) + (cam == "cam1"), np.uint8)).save(root / "mav0" / cam / "data" / f"{s}.png")
    if csv:
        os.makedirs(root / "mav0" / "state_groundtruth_estimate0")
        lines = ["#timestamp, p_RS_R_x [m], p_RS_R_y [m], p_RS_R_z [m], q_RS_w [], q_RS_x [], q_RS_y [], q_RS_z [], v_RS_R_x [m s^-1]"]
        lines += [",".join([str(t)] + [repr(float(v)) for v in (*p, *q)] + ["0.125"]) for t, p, q in POSE_ROWS]
        (root / "mav0" / "state_groundtruth_estimate0" / "data.csv").write_text("\n".join(lines) + "\n")
    return str(root)


def _expected_w2c(frame, T_i_c0):
    T = np.eye(4)
    T[:3, :3] = ROTATIONS[frame]
    T[:3, 3] = POSE_ROWS[ROW_OF_FRAME[frame]][1]
    return np.linalg.inv(T @ T_i_c0)


def test_parse_euroc_order_association_and_pose_convention(tmp_path):
    root = _write_euroc(tmp_path / "seq", shuffle=True)
    frames = recorded.parse_euroc(root)
    assert len(frames) == 4
    assert [os.path.basename(p) for p in frames.color_paths] == [f"{s}.png" for s in STAMPS]
    assert [os.path.basename(p) for p in frames.right_paths] == [f"{s}.png" for s in STAMPS]
    assert all("cam0" in p for p in frames.color_paths) and all("cam1" in p for p in frames.right_paths)
    default = np.array(recorded.EUROC_T_I_C0)
    assert default.shape == (4, 4) and abs(np.linalg.det(default[:3, :3]) - 1) < 1e-6
    for k in range(4):
        assert np.abs(frames.poses[k] - _expected_w2c(k, default)).max() < 1e-12, k
    own = np.eye(4)
    own[:3, :3] = ROTATIONS[1]
    own[:3, 3] = (0.1, -0.2, 0.3)
    frames = recorded.parse_euroc(root, T_i_c0=own.tolist())
    for k in range(4):
        assert np.abs(frames.poses[k] - _expected_w2c(k, own)).max() < 1e-12, k
    part = frames.sliced(1, -1)
    assert len(part) == 3 and part.right_paths == frames.right_paths[1:] and np.array_equal(part.poses, frames.poses[1:])
    f = recorded.frame_decode.decode_stereo_frame(frames.color_paths[2], frames.right_paths[2], 8, 6)
    assert f.left.dtype == np.uint8 and f.left.shape == (6, 8) and int(f.left[0, 0]) == 20 and int(f.right[0, 0]) == 21
    with pytest.raises(ValueError, match="calibration says"):
        recorded.frame_decode.decode_stereo_frame(frames.color_paths[2], frames.right_paths[2], 6, 8)


def test_parse_euroc_errors(tmp_path):
    with pytest.raises(ValueError, match="4 mav0/cam0/data/\\*.png and 3 mav0/cam1"):
        recorded.parse_euroc(_write_euroc(tmp_path / "unequal", n_right=3))
    with pytest.raises(FileNotFoundError, match="data.csv"):
        recorded.parse_euroc(_write_euroc(tmp_path / "nocsv", csv=False))
    with pytest.raises(ValueError, match="0 mav0/cam0"):
        recorded.parse_euroc(str(tmp_path / "nothing"))


def _config(root, **dataset):
    cam = {"raw": {"fx": 8.0, "fy": 8.0, "cx": 4.0, "cy": 3.0, "k1": 0.0, "k2": 0.0, "p1": 0.0, "p2": 0.0, "k3": 0.0},
           "opt": {"fx": 8.0, "fy": 8.0, "cx": 4.0, "cy": 3.0}, "R": {"data": list(np.eye(3).reshape(-1))}}
    return {"Dataset": dict({"type": "euroc", "dataset_path": root,
                             "Calibration": {"cam0": cam, "cam1": cam, "distorted": False, "width": 8, "height": 6}}, **dataset)}


def test_euroc_dataset_argument_handling(tmp_path):
    root = _write_euroc(tmp_path / "seq")
    assert "euroc" in recorded.SUPPORTED_TYPES
    with pytest.raises(ValueError, match="'euroc' takes no segmenter"):
        recorded.EurocDataset(_config(root), device="cuda:0", segmenter=object())
    with pytest.raises(ValueError, match="'euroc' takes no segmenter"):              # load_dataset dispatches on the type
        recorded.load_dataset(_config(root), "cuda:0", segmenter=object())
    with pytest.raises(ValueError, match="4 mav0/cam0/data/\\*.png and 2 mav0/cam1"):
        recorded.load_dataset(_config(_write_euroc(tmp_path / "unequal", n_right=2)), "cuda:0")
    with pytest.raises(FileNotFoundError, match="data.csv"):
        recorded.load_dataset(_config(_write_euroc(tmp_path / "nocsv", csv=False)), "cuda:0")
    with pytest.raises(ValueError, match="'tum'.*'CoFusion'.*'euroc'"):
        recorded.load_dataset({"Dataset": {"type": "replica"}})


class _Pairs:
    """The part of slam/dataset.py's interface that write_euroc_sequence uses, on the CPU."""
    fx, fy, cx, cy, width, height = 9.5, 9.25, 5.0, 3.5, 10, 7

    def __init__(self, n):
        g = torch.Generator().manual_seed(5)
        self.images = torch.rand((n, 2, 3, 7, 10), generator=g)
        self.poses = []
        for k in range(n):
            a, b = 0.3 * k + 0.1, -0.2 * k
            Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rz @ Rx, (0.1 * k, -0.05 * k, 1.0 + k)
            self.poses.append(torch.tensor(T, dtype=torch.float32))

    def __len__(self):
        return len(self.poses)

    def __getitem__(self, i):
        return self.images[i, 0], np.ones((7, 10), np.float32), self.poses[i], torch.ones((7, 10), dtype=torch.bool)

    def right_view(self, i, baseline):
        return self.images[i, 1]


def test_write_euroc_sequence_round_trip(tmp_path):
    src = _Pairs(4)
    calib = recorded.write_euroc_sequence(src, str(tmp_path / "seq"), baseline=0.11)
    assert calib["bf"] == pytest.approx(9.5 * 0.11) and calib["distorted"] is False and (calib["width"], calib["height"]) == (10, 7)
    assert calib["cam0"]["opt"] == {"fx": 9.5, "fy": 9.25, "cx": 5.0, "cy": 3.5} and calib["cam1"]["raw"]["k1"] == 0.0
    frames = recorded.parse_euroc(str(tmp_path / "seq"), calib["T_i_c0"])
    assert len(frames) == 4
    for k in range(4):
        assert np.abs(frames.poses[k] - src.poses[k].double().numpy()).max() < 1e-6, k
        f = recorded.frame_decode.decode_stereo_frame(frames.color_paths[k], frames.right_paths[k], 10, 7)
        assert np.array_equal(f.left, recorded.grey_bytes(src.images[k, 0])) and np.array_equal(f.right, recorded.grey_bytes(src.images[k, 1]))
        assert os.path.basename(frames.color_paths[k]) == f"{recorded.euroc_stamp(k)}.png"


# ---- the C entry point's argument checks (nothing is launched on a refused call, so no GPU is needed) ------------------------------
def test_entry_point_refuses_bad_arguments_before_any_launch():
    import ctypes
    from diff_gaussian_rasterization import _C
    lib = _C.load_library()
    W, H = 97, 23
    need = lib.gsr_stereo_workspace_size(W, H, 64)
    assert need >= 2 * W * H * 8 + W * H * 64 * 2 and need % 16 == 0
    assert lib.gsr_stereo_workspace_size(W, H, 128) >= 2 * W * H * 8 + W * H * 128 * 2
    assert [lib.gsr_stereo_workspace_size(*a) for a in ((W, H, 96), (0, H, 64), (W, -1, 64), (1 << 15, 1 << 15, 64))] == [0, 0, 0, 0]
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15                   # a non-NULL, 16-byte aligned address; never dereferenced by a refused call
    base = dict(width=W, height=H, D=64, p1=10, p2=120, uniq=40, d12=1, bf=1.0, left=ptr, right=ptr, map_l=None, map_r=None, lut=None,
                rect_l=None, rect_r=None, image=None, disp=ptr, depth=None, cost=None, ws=ptr, ws_bytes=need - 1, stream=None)
    for over, text in (({"D": 96}, r"num_disparities 64 or 128 \(got 96\)"), ({"width": 0}, "width and height must be positive"),
                       ({"p1": 120}, "0 < p1 < p2 <= 2047, got p1 120, p2 120"), ({"p1": 0}, "0 < p1 < p2"), ({"p2": 2048}, "0 < p1 < p2"),
                       ({"uniq": 100}, r"uniqueness_ratio must be in \[0, 99\], got 100"), ({"uniq": -1}, "uniqueness_ratio"),
                       ({"d12": -2}, "disp12_max_diff must be -1"), ({"disp": None}, "must not be NULL"), ({"left": None}, "must not be NULL"),
                       ({"map_l": ptr}, "go together"), ({"map_r": ptr}, "go together"),
                       ({"map_l": ptr, "map_r": ptr}, "left_rect and right_rect must not be NULL when maps are given"),
                       ({"image": ptr}, "image needs lut"), ({"ws": ptr + 8, "ws_bytes": need}, "16-byte aligned"),
                       ({}, rf"hold {need} bytes \(gsr_stereo_workspace_size\), got {need - 1}")):          # one byte short
        with pytest.raises(RuntimeError, match=r"gsr_stereo_depth failed \(code -1\): gsr_stereo_depth: .*" + text):
            lib.gsr_stereo_depth(*dict(base, **over).values())
