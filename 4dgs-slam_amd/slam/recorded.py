"""Recorded RGB-D sequences: the TUM / Bonn and CoFusion loaders of the reference (utils/dataset.py:85-181, 490-660, 677-696, 962-976)
with the interface of slam/dataset.py:

    dataset[idx] -> (image [3,H,W] float32 device, depth [H,W] float32 numpy, pose [4,4] float32 W2C device, motion_mask [H,W] bool device)

Path parsing (``parse_tum`` / ``parse_cofusion``) is separate from decoding and runs without a GPU. PNG decoding stays on the host (PIL,
slam/frame_decode.py) in a background thread that reads ahead of the SLAM loop; the frame is staged in pinned memory, and its upload,
lens undistortion, byte -> float conversion, CHW transpose and motion-mask threshold are one HIP launch on a side stream
(gsr_frame_prepare, include/frame_io.h) that the caller's stream waits for. Given an optical-flow estimator (``flow=``, slam/optical_flow.py
RaftFlow), the dataset has ``gt_flow`` -- RAFT's flow between two frames, as the reference's generate_flow asks it for; without one it has no
``gt_flow`` and the backend skips its flow term, as it does for any dataset that lacks it. Given a segmenter (``segmenter=``,
slam/segmentation.py YoloSeg), every frame runs YOLO on the side stream right after its preparation and the instance masks of the loader's
COCO classes are cleared from its motion mask (slam/segmentation.py dataset_classes: TUM / Bonn person, plus chair with seg_chair, ORed
with the file masks; CoFusion person / clock / teddy bear, and no YOLO when mask files exist); without one, motion masks come only from
mask files.

Stereo sequences in the EuRoC layout (``parse_euroc`` / ``EurocDataset``, the reference's EuRoCParser and StereoDataset,
utils/dataset.py:183-248, 376-487) have no depth files: the two grey images are rectified and matched on the side stream
(gsr_stereo_depth, include/stereo_depth.h, slam/stereo.py) and the depth handed out is bf / disparity.

A plain video (``VideoDataset``, Dataset.type 'video': a Motion-JPEG AVI file or a folder of .jpg files; no counterpart in the reference) has
neither depth nor ground truth: its frames are parsed on the read-ahead thread (slam/jpeg_decode.py) and decoded on the side stream
(gsr_jpeg_decode, include/video_io.h), and ``has_ground_truth`` is False, which the run reads (slam/system.py).

What the reference does and this does not: EXR depth (CoFusion's depth_noise/*.exr raises), and its TUM mask list is not sliced by
Calibration start / end (:691-696) -- here the masks are sliced with the frames."""
import collections
import concurrent.futures
import glob
import math
import os
import re
import time
import weakref

import numpy as np

from . import frame_decode
from .camera import fov_from_focal

MASK_THRESHOLD = 0.01          # utils/dataset.py:346: ToTensor(mask_L) > 0.01 is a moving pixel


# ---- path parsing (host only) ------------------------------------------------------------------------------------------------------
class FrameList:
    """What a sequence is on disk: per kept frame its colour, depth and (optional) mask file and its W2C pose (float64)."""

    def __init__(self, color_paths, depth_paths, poses, mask_paths=None, depth_float32=False):
        self.color_paths, self.depth_paths = list(color_paths), list(depth_paths)
        self.poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        self.mask_paths = list(mask_paths) if mask_paths else None
        self.depth_float32 = depth_float32       # CoFusion divides in float32, TUM in float64 (then casts)

    def __len__(self):
        return len(self.color_paths)

    def sliced(self, start, end):
        """Calibration start / end (end -1 = to the last frame), applied to every per-frame list."""
        n = len(self)
        end = n if end == -1 else end
        return FrameList(self.color_paths[start:end], self.depth_paths[start:end], self.poses[start:end],
                         self.mask_paths[start:end] if self.mask_paths else None, self.depth_float32)


def read_list(path, skiprows=0):
    """np.loadtxt(path, delimiter=" ", dtype=str, skiprows=skiprows): the first skiprows lines are dropped, '#' starts a comment."""
    rows = []
    with open(path, "r") as f:
        for k, line in enumerate(f):
            if k < skiprows:
                continue
            line = line.split("#", 1)[0].strip()
            if line:
                rows.append(line.split())
    return rows


def extract_number(path):
    """The trailing number of a '<...><digits>.png' name (utils/dataset.py:114-122); 0 without one."""
    m = re.search(r"(\d+)(?=\.png$)", path)
    return float(m.group(1)) if m else 0


def quaternion_matrix(q_wxyz):
    """Homogeneous rotation of a (w, x, y, z) quaternion, normalised first (trimesh.transformations.quaternion_matrix)."""
    q = np.asarray(q_wxyz, dtype=np.float64)
    n = float(np.dot(q, q))
    if n < np.finfo(float).eps * 4.0:
        return np.identity(4)
    w, x, y, z = q * math.sqrt(2.0 / n)
    return np.array([[1.0 - y * y - z * z, x * y - z * w, x * z + y * w, 0.0],
                     [x * y + z * w, 1.0 - x * x - z * z, y * z - x * w, 0.0],
                     [x * z - y * w, y * z + x * w, 1.0 - x * x - y * y, 0.0],
                     [0.0, 0.0, 0.0, 1.0]])


def pose_from_tum(vec):
    """W2C from a TUM line's (timestamp tx ty tz qx qy qz qw): inv(T), T = [R(q) | t] with the quaternion rolled to w-first."""
    vec = np.asarray(vec, dtype=np.float64)
    T = quaternion_matrix(np.roll(vec[4:8], 1))
    T[:3, 3] = vec[1:4]
    return np.linalg.inv(T)


def associate_frames(tstamp_image, tstamp_depth, tstamp_pose, max_dt=0.08):
    """TUMParser.associate_frames: per colour frame the nearest depth and pose stamps, both within max_dt."""
    out = []
    for i, t in enumerate(tstamp_image):
        j = int(np.argmin(np.abs(tstamp_depth - t)))
        k = int(np.argmin(np.abs(tstamp_pose - t)))
        if abs(tstamp_depth[j] - t) < max_dt and abs(tstamp_pose[k] - t) < max_dt:
            out.append((i, j, k))
    return out


def sequence_has_depth(config):
    """The reference's ``has_depth`` (utils/dataset.py:303,534): a sequence is read without depth files only when ``Dataset.sensor_type``
    is 'monocular' AND the calibration has no ``depth_scale``; any other configuration needs its depth files, and says so when they are missing."""
    d = config["Dataset"]
    return not (d.get("sensor_type") == "monocular" and "depth_scale" not in d["Calibration"])


def tum_frames(config):
    """The FrameList of a 'tum' configuration: parsed (without depth files for a monocular sequence, sequence_has_depth), then start / end."""
    c = config["Dataset"]["Calibration"]
    return parse_tum(config["Dataset"]["dataset_path"], depth=sequence_has_depth(config)).sliced(int(c.get("start", 0)), int(c.get("end", -1)))


def parse_tum(datapath, frame_rate=32, max_dt=0.08, depth=True):
    """TUMParser (utils/dataset.py:85-181): rgb.txt / depth.txt / groundtruth.txt (else pose.txt, first line skipped), association,
    frame-rate subsampling, W2C poses, and per kept frame the render_mask/*.png at its rgb.txt row (masks sorted by trailing number).
    depth=False (a monocular sequence): depth.txt is not read, a colour frame only needs a pose within max_dt, and every depth path is None."""
    pose_list = None
    for name in ("groundtruth.txt", "pose.txt"):
        if os.path.isfile(os.path.join(datapath, name)):
            pose_list = os.path.join(datapath, name)
            break
    if pose_list is None:
        raise FileNotFoundError(f"{datapath}: neither groundtruth.txt nor pose.txt")
    mask_dir = os.path.join(datapath, "render_mask")
    mask_all = sorted(glob.glob(os.path.join(mask_dir, "*.png")), key=extract_number) if os.path.isdir(mask_dir) else None
    image_data = read_list(os.path.join(datapath, "rgb.txt"))
    depth_data = read_list(os.path.join(datapath, "depth.txt")) if depth else None
    pose_vecs = np.array([[float(x) for x in r] for r in read_list(pose_list, skiprows=1)], dtype=np.float64)
    if depth:
        if not image_data or not depth_data or not len(pose_vecs):
            raise ValueError(f"{datapath}: rgb.txt, depth.txt and the pose file must each list at least one entry")
        tstamp_image = np.array([float(r[0]) for r in image_data])
        tstamp_depth = np.array([float(r[0]) for r in depth_data])
        assoc = associate_frames(tstamp_image, tstamp_depth, pose_vecs[:, 0], max_dt)
        if not assoc:
            raise ValueError(f"{datapath}: no colour frame has a depth frame and a pose within {max_dt} s")
    else:
        if not image_data or not len(pose_vecs):
            raise ValueError(f"{datapath}: rgb.txt and the pose file must each list at least one entry")
        tstamp_image = np.array([float(r[0]) for r in image_data])
        assoc = [(i, None, k) for i, _, k in associate_frames(tstamp_image, tstamp_image, pose_vecs[:, 0], max_dt)]
        if not assoc:
            raise ValueError(f"{datapath}: no colour frame has a pose within {max_dt} s")
    keep = [0]
    for ix in range(1, len(assoc)):
        if tstamp_image[assoc[ix][0]] - tstamp_image[assoc[keep[-1]][0]] > 1.0 / frame_rate:
            keep.append(ix)
    colors, depths, poses, masks = [], [], [], []
    for ix in keep:
        i, j, k = assoc[ix]
        colors.append(os.path.join(datapath, image_data[i][1]))
        depths.append(os.path.join(datapath, depth_data[j][1]) if depth else None)
        poses.append(pose_from_tum(pose_vecs[k]))
        if mask_all is not None:
            if i >= len(mask_all):
                raise ValueError(f"{mask_dir}: {len(mask_all)} masks, but rgb.txt row {i} is a kept frame")
            masks.append(mask_all[i])
    return FrameList(colors, depths, poses, masks if mask_all is not None else None)


def parse_cofusion(datapath, depth=True):
    """CoFusion (utils/dataset.py:490-575): colour/*.png, depth/*.png, mask_colour/*.png, trajectories/gt-cam-0.txt (identity poses
    without it). EXR depth (depth_noise/*.exr) needs an OpenEXR reader this project does not have. depth=False (a monocular sequence):
    the depth folders are not looked at and every depth path is None."""
    colors = sorted(glob.glob(os.path.join(datapath, "colour", "*.png")))
    masks = sorted(glob.glob(os.path.join(datapath, "mask_colour", "*.png")))
    n = len(colors)
    if depth:
        exr = sorted(glob.glob(os.path.join(datapath, "depth_noise", "*.exr")))
        if exr:
            raise NotImplementedError(f"{os.path.join(datapath, 'depth_noise')}: EXR depth is not supported (no OpenEXR reader); "
                                      "provide depth/*.png instead")
        depths = sorted(glob.glob(os.path.join(datapath, "depth", "*.png")))
        if n == 0 or len(depths) < n:
            raise ValueError(f"{datapath}: {n} colour/*.png and {len(depths)} depth/*.png (need at least one frame and a depth per frame)")
    else:
        depths = [None] * n
        if n == 0:
            raise ValueError(f"{datapath}: no colour/*.png")
    traj = os.path.join(datapath, "trajectories", "gt-cam-0.txt")
    if os.path.isfile(traj):
        rows = read_list(traj)
        if len(rows) < n:
            raise ValueError(f"{traj}: {len(rows)} poses for {n} frames")
        poses = [pose_from_tum([float(x) for x in r]) for r in rows[:n]]
    else:
        poses = [np.eye(4) for _ in range(n)]
    return FrameList(colors, depths[:n], poses, masks or None, depth_float32=True)


class StereoFrameList(FrameList):
    """A stereo sequence on disk: per frame the left (cam0) and the right (cam1) image and the W2C pose of the left camera."""

    def __init__(self, left_paths, right_paths, poses):
        super().__init__(left_paths, [], poses)
        self.right_paths = list(right_paths)

    def sliced(self, start, end):
        end = len(self) if end == -1 else end
        return StereoFrameList(self.color_paths[start:end], self.right_paths[start:end], self.poses[start:end])


# utils/dataset.py:217-224: the cam0 extrinsic of the EuRoC rig (body frame <- cam0)
EUROC_T_I_C0 = ((0.0148655429818, -0.999880929698, 0.00414029679422, -0.0216401454975),
                (0.999557249008, 0.0149672133247, 0.025715529948, -0.064676986768),
                (-0.0257744366974, 0.00375618835797, 0.999660727178, 0.00981073058949),
                (0.0, 0.0, 0.0, 1.0))


def parse_euroc(datapath, T_i_c0=None):
    """EuRoCParser (utils/dataset.py:183-248): mav0/cam0/data/*.png and mav0/cam1/data/*.png, sorted and paired by position, and
    mav0/state_groundtruth_estimate0/data.csv (timestamp, p x y z, q w x y z, ...; the first line is a header). Per frame the pose row with
    the nearest time stamp to the left image's file name; W2C = (T_w_i T_i_c0)^-1, T_i_c0 the EuRoC cam0 extrinsic unless given."""
    left = sorted(glob.glob(os.path.join(datapath, "mav0", "cam0", "data", "*.png")))
    right = sorted(glob.glob(os.path.join(datapath, "mav0", "cam1", "data", "*.png")))
    if not left or len(left) != len(right):
        raise ValueError(f"{datapath}: {len(left)} mav0/cam0/data/*.png and {len(right)} mav0/cam1/data/*.png (need at least one frame and "
                         "as many right images as left ones)")
    csv_path = os.path.join(datapath, "mav0", "state_groundtruth_estimate0", "data.csv")
    if not os.path.isfile(csv_path):
        raise FileNotFoundError(f"{csv_path}: a stereo sequence needs its ground-truth poses")
    rows = []
    with open(csv_path, "r") as f:
        for k, line in enumerate(f):
            line = line.strip()
            if k == 0 or not line or line.startswith("#"):
                continue
            rows.append([float(v) for v in line.split(",")[:8]])
    if not rows:
        raise ValueError(f"{csv_path}: no pose rows")
    data = np.array(rows, dtype=np.float64)
    T_i_c0 = np.asarray(EUROC_T_I_C0 if T_i_c0 is None else T_i_c0, dtype=np.float64).reshape(4, 4)
    poses = []
    for path in left:
        stamp = float(os.path.basename(path).split(".")[0])
        row = data[int(np.argmin(np.abs(data[:, 0] - stamp)))]
        T_w_i = quaternion_matrix(row[4:8])
        T_w_i[:3, 3] = row[1:4]
        poses.append(np.linalg.inv(T_w_i @ T_i_c0))
    return StereoFrameList(left, right, poses)


def undistort_map(width, height, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """cv2.initUndistortRectifyMap(K, (k1, k2, p1, p2, k3), R = I, newK = K, (width, height), CV_32FC1) restated in float64, stored as
    float32 [H,W,2] = (map_x, map_y): where the undistorted pixel (u, v) samples the distorted frame."""
    v, u = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
    mx = fx * (x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) + cx
    my = fy * (y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) + cy
    return np.stack([mx, my], -1).astype(np.float32)


def byte_lut():
    """float32(b / 255.0) in double for every byte b: the reference's torch.from_numpy(image / 255.0).to(float32)."""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


# ---- decoding (host) ---------------------------------------------------------------------------------------------------------------
def decode_frame(frames, idx, width, height, depth_scale):
    """PIL decode of frame idx of a FrameList (frame_decode.decode_frame)."""
    return frame_decode.decode_frame(frames.color_paths[idx], frames.depth_paths[idx], frames.mask_paths[idx] if frames.mask_paths else None,
                                     width, height, depth_scale, frames.depth_float32)


class _Reader:
    """Decoding ahead of the consumer in one thread, and a small bounded cache; holds no reference to the dataset object."""

    def __init__(self, tasks, depth, cache, decode=frame_decode.decode_frame):
        self.tasks, self.n, self.depth, self.decode = tasks, len(tasks), depth, decode
        # a thread that runs PIL and numpy only: it never touches the device, so it cannot disturb a graph capture on the caller's thread
        # (a decoding process measured no faster)
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="frame-decode") if depth > 0 else None
        self.pending = {}
        self.cache = collections.OrderedDict()
        self.cache_size = max(1, cache)
        self.stats = {"decode_ms": [], "wait_ms": 0.0, "prefetched": 0, "on_demand": 0, "cached": 0}

    def _decode(self, idx):
        return self.decode(*self.tasks[idx])

    def _done(self, f):
        self.stats["decode_ms"].append(f.decode_ms)
        return f

    def schedule(self, first):
        if self.pool is None:
            return
        for k in range(first, min(first + self.depth, self.n)):
            if k not in self.pending and k not in self.cache:
                self.pending[k] = self.pool.submit(self.decode, *self.tasks[k])

    def get(self, idx):
        t0 = time.perf_counter()
        fut = self.pending.pop(idx, None)
        if idx in self.cache:
            f = self.cache.pop(idx)
            self.stats["cached"] += 1
        elif fut is not None:
            f = self._done(fut.result())
            self.stats["prefetched"] += 1
        else:
            f = self._done(self._decode(idx))
            self.stats["on_demand"] += 1
        self.stats["wait_ms"] += (time.perf_counter() - t0) * 1e3
        self.cache[idx] = f
        while len(self.cache) > self.cache_size:
            self.cache.popitem(last=False)
        for k in [k for k in self.pending if k < idx or k > idx + self.depth]:     # a jump (eval re-reads): drop what is now stale
            if self.pending[k].cancel():
                del self.pending[k]
        self.schedule(idx + 1)
        return f

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True, cancel_futures=True)
            self.pool = None
        self.pending.clear()


# ---- datasets ----------------------------------------------------------------------------------------------------------------------
def check_motion_segmenter(motion_segmenter, flow, has_depth):
    """A flow-and-depth motion segmenter needs both: refuse it, naming what is missing, before anything is read or allocated."""
    if motion_segmenter is None:
        return
    if flow is None:
        raise ValueError("a motion segmenter needs a flow estimator (flow=): it segments from the optical flow between a frame and its partner")
    if not has_depth:
        raise ValueError("a motion segmenter needs sensor depth: a monocular sequence (no depth files) cannot be segmented from flow and depth")


class RecordedRGBDDataset:
    """A recorded sequence with the interface of slam/dataset.py's SyntheticRGBDDataset; ``gt_flow`` only with a flow estimator."""

    FLOW_CACHE_PAIRS = 16          # estimated pairs kept (both directions each; 4.9 MB per pair at 640x480)
    SEG_CACHE_FRAMES = 32          # segmented motion masks kept (0.3 MB each at 640x480): evaluation reads the frames again

    def __init__(self, frames, calibration, device="cuda:0", distorted=False, prefetch=4, max_frames=None, flow=None, segmenter=None,
                 seg_classes=None, motion_segmenter=None):
        import torch
        from .camera import getProjectionMatrix2
        from .pretrained import EventLog
        if max_frames is not None:
            frames = frames.sliced(0, min(int(max_frames), len(frames)))
        if len(frames) == 0:
            raise ValueError("the sequence has no frames (after Calibration start / end)")
        check_motion_segmenter(motion_segmenter, flow, not (frames.depth_paths and frames.depth_paths[0] is None))
        self.frames = frames
        self.device = torch.device(device)
        c = calibration
        self.fx, self.fy, self.cx, self.cy = float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])
        self.width, self.height = int(c["width"]), int(c["height"])
        self.fovx, self.fovy = fov_from_focal(self.fx, self.width), fov_from_focal(self.fy, self.height)
        # (a monocular sequence read without depth files, sequence_has_depth: no scale either, and every frame's depth is None)
        self.depth_scale = None if (frames.depth_paths and frames.depth_paths[0] is None) else float(c["depth_scale"])
        self.num_imgs = len(frames)
        self.dynamic_objects = 0
        self.projection_matrix = getProjectionMatrix2(0.01, 100.0, self.cx, self.cy, self.fx, self.fy, self.width,
                                                      self.height).transpose(0, 1).to(self.device)
        self.poses = torch.tensor(frames.poses, dtype=torch.float32, device=self.device)
        self._lut = torch.tensor(byte_lut(), device=self.device)
        self._map = None
        if distorted:
            m = undistort_map(self.width, self.height, self.fx, self.fy, self.cx, self.cy,
                              *(float(c.get(k, 0.0)) for k in ("k1", "k2", "p1", "p2", "k3")))
            self._map = torch.tensor(m, device=self.device)
        torch.cuda.synchronize(self.device)             # the tables exist before the side stream reads them
        self._side = torch.cuda.Stream(self.device)
        self._reader = _Reader(self._decode_tasks(frames), int(prefetch), cache=int(prefetch) + 4, decode=self._decode)
        self._finalizer = weakref.finalize(self, self._reader.close)
        self._reader.schedule(0)
        self._reader.get(0)                             # the reader is up and frame 0 is decoded before the dataset is handed out
        self._reader.stats.update(wait_ms=0.0, prefetched=0, on_demand=0)
        self._flow = flow
        if flow is not None:
            self._flow_token = object()                 # names this dataset's frames in the estimator's encoder cache
            self._flow_cache = collections.OrderedDict()
            self._flow_log = EventLog(self.device)
            self.gt_flow = self._gt_flow
        self._segmenter = segmenter if seg_classes else None
        self.seg_classes = list(seg_classes) if self._segmenter is not None else None
        self._seg_cache = collections.OrderedDict()   # frame -> its motion mask with the instance masks cleared
        self._seg_log = EventLog(self.device)
        self._motion_segmenter = motion_segmenter     # slam/motion_segmentation.py FlowMotionSegmenter: flow + depth, any class

    _decode = staticmethod(frame_decode.decode_frame)     # what the read-ahead thread runs on one entry of _decode_tasks

    def _decode_tasks(self, frames):
        return [(frames.color_paths[i], frames.depth_paths[i], frames.mask_paths[i] if frames.mask_paths else None, self.width, self.height,
                 self.depth_scale, frames.depth_float32) for i in range(self.num_imgs)]

    def __len__(self):
        return self.num_imgs

    def close(self):
        """Stop the reader thread (also done when the dataset is dropped and at interpreter exit)."""
        self._finalizer()

    @property
    def ingest_stats(self):
        s = self._reader.stats
        d = np.asarray(s["decode_ms"], dtype=np.float64)
        return {"decode_ms_mean": float(d.mean()) if len(d) else None, "decode_ms_p95": float(np.percentile(d, 95)) if len(d) else None,
                "decoded": int(len(d)), "wait_ms_total": s["wait_ms"], "prefetched": s["prefetched"], "on_demand": s["on_demand"],
                "cached": s["cached"], "prefetch_depth": self._reader.depth}

    def _gt_flow(self, idx_from, idx_to):
        """(flow [H,W,2] float32 NDC on the device, valid [H,W] bool): RAFT with image1 = frame idx_from, image2 = frame idx_to, divided by
        (W, H) and times 2 (utils/camera_utils.py:386-417). Both directions of a pair come from one estimator call, in frame order, and are
        kept. `valid` is all true: the reference's forward-backward consistency masks never enter its loss."""
        import torch
        hit = self._flow_cache.get((idx_from, idx_to))
        if hit is None:
            a, b = sorted((int(idx_from), int(idx_to)))
            est = self._flow
            image = lambda i: None if (self._flow_token, i) in est._enc else self._frame_image(i)
            with self._flow_log.timed():
                fab, fba = est.pair(image(a), image(b), key_i=(self._flow_token, a), key_j=(self._flow_token, b))
            valid = torch.ones((self.height, self.width), dtype=torch.bool, device=self.device)
            while len(self._flow_cache) >= 2 * self.FLOW_CACHE_PAIRS:
                self._flow_cache.popitem(last=False)
            self._flow_cache[(a, b)] = (fab, valid)
            self._flow_cache[(b, a)] = (fba, valid)
            hit = self._flow_cache[(idx_from, idx_to)]
        return hit

    @property
    def flow_stats(self):
        """Pairs estimated and the device ms per pair (None without an estimator)."""
        if self._flow is None:
            return None
        t = self._flow_log.summary()
        return {"pairs": t["calls"], "ms_per_pair": t["ms_per_item"], "ms_first": t["ms_first"], "ms_rest_mean": t["ms_per_item_rest"]}

    @property
    def segmentation_stats(self):
        """Frames segmented and the device ms per frame (network + post-processing; None without a segmenter)."""
        if self._segmenter is None:
            return None
        t = self._seg_log.summary()
        return {"frames": t["calls"], "classes": self.seg_classes, "ms_per_frame": t["ms_per_item"], "ms_first": t["ms_first"],
                "ms_rest_mean": t["ms_per_item_rest"]}

    @property
    def motion_segmentation_stats(self):
        """Frames segmented from flow and depth, the device ms per frame of the fit and of the cleaning, the mean moving share and the mean
        final cutoff (None without a motion segmenter). The flow pair each frame needs is counted in flow_stats, not here."""
        return None if self._motion_segmenter is None else self._motion_segmenter.stats

    def _segment_motion(self, idx, hf, motion):
        """motion &= ~(what frame idx's flow to its partner frame cannot be explained by one camera motion), in place on the caller's
        stream. The partner is `gap` frames back, or ahead for the first frames; a one-frame sequence keeps its mask."""
        import torch
        gap = self._motion_segmenter.gap
        j = idx - gap if idx >= gap else min(idx + gap, self.num_imgs - 1)
        if j == idx:
            return
        flow_ij, flow_ji = self._gt_flow(idx, j)[0], self._gt_flow(j, idx)[0]
        main = torch.cuda.current_stream(self.device)
        depth_h = torch.from_numpy(np.ascontiguousarray(hf.depth, dtype=np.float32)).pin_memory()
        with torch.cuda.stream(self._side):
            depth = depth_h.to(self.device, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(self._side)
        main.wait_event(ready)
        depth.record_stream(main)
        self._motion_segmenter.segment(flow_ij, depth, (self.fx, self.fy, self.cx, self.cy), flow_ji=flow_ji, motion=motion, stream=main)

    def _frame_image(self, idx):
        """Frame idx's image [3,H,W] without moving the read-ahead window (a keyframe the flow term needs again); never segmented."""
        if not 0 <= idx < self.num_imgs:
            raise IndexError(f"frame {idx} of a {self.num_imgs}-frame sequence")
        hf = self._reader.cache.get(idx)
        if hf is None:
            hf = self._reader._decode(idx)
        return self._prepare(hf)[0]

    def __getitem__(self, idx):
        if not 0 <= idx < self.num_imgs:
            raise IndexError(f"frame {idx} of a {self.num_imgs}-frame sequence")
        hf = self._reader.get(idx)
        if self._segmenter is None and self._motion_segmenter is None:
            image, motion = self._prepare(hf)
            return image, hf.depth, self.poses[idx].clone(), motion
        hit = self._seg_cache.get(idx)
        image, motion = self._prepare(hf, segment=hit is None and self._segmenter is not None)
        if hit is None:
            if self._motion_segmenter is not None:      # after the file mask and the instance masks: known movers stay out of the fit
                self._segment_motion(idx, hf, motion)
            self._seg_cache[idx] = motion
            while len(self._seg_cache) > self.SEG_CACHE_FRAMES:
                self._seg_cache.popitem(last=False)
        else:
            self._seg_cache.move_to_end(idx)
            motion = hit
        return image, hf.depth, self.poses[idx].clone(), motion.clone()

    def _prepare(self, hf, segment=False):
        import torch
        from . import frame_io
        H, W, dev = self.height, self.width, self.device
        main = torch.cuda.current_stream(dev)
        # pinned staging on this thread (the decoding thread never touches the device); the host allocator keeps a block until the
        # copy that reads it has completed
        rgb_h = torch.from_numpy(hf.rgb).pin_memory()
        mask_h = None if hf.mask is None else torch.from_numpy(hf.mask).pin_memory()
        with torch.cuda.stream(self._side):
            rgb = rgb_h.to(dev, non_blocking=True)
            mask = None if mask_h is None else mask_h.to(dev, non_blocking=True)
            image = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            motion = torch.empty((H, W), dtype=torch.bool, device=dev)
            frame_io.frame_prepare(rgb, self._map, self._lut, mask, MASK_THRESHOLD, image, motion, self._side)
            if segment:                                 # YOLO on the prepared frame; motion &= ~(instance masks), in place
                with self._seg_log.timed(self._side):
                    self._segmenter(image, self.seg_classes, motion=motion)
            ready = torch.cuda.Event()
            ready.record(self._side)
        main.wait_event(ready)
        image.record_stream(main)                       # allocated on the side stream, used (and freed) on the caller's
        motion.record_stream(main)
        return image, motion


class TUMDataset(RecordedRGBDDataset):
    """TUM RGB-D and Bonn (utils/dataset.py:677-696): Dataset.type 'tum'; Bonn calibrations are distorted."""

    def __init__(self, config, device="cuda:0", prefetch=4, max_frames=None, flow=None, segmenter=None, motion_segmenter=None):
        from .segmentation import dataset_classes
        check_motion_segmenter(motion_segmenter, flow, sequence_has_depth(config))
        c = config["Dataset"]["Calibration"]
        frames = tum_frames(config)
        super().__init__(frames, c, device, distorted=bool(c.get("distorted", False)), prefetch=prefetch, max_frames=max_frames, flow=flow,
                         segmenter=segmenter, seg_classes=dataset_classes("tum", config["Dataset"], bool(frames.mask_paths)),
                         motion_segmenter=motion_segmenter)


class CoFusionDataset(RecordedRGBDDataset):
    """CoFusion (utils/dataset.py:490-660): Dataset.type 'CoFusion'; never undistorted, depth divided in float32."""

    def __init__(self, config, device="cuda:0", prefetch=4, max_frames=None, flow=None, segmenter=None, motion_segmenter=None):
        from .segmentation import dataset_classes
        c, d = config["Dataset"]["Calibration"], config["Dataset"]
        has_depth = sequence_has_depth(config)
        check_motion_segmenter(motion_segmenter, flow, has_depth)
        frames = parse_cofusion(d["dataset_path"], depth=has_depth).sliced(int(c.get("start", 0)), int(c.get("end", -1)))
        if d.get("seg_teddy", False) or d.get("seg_clock", False):           # :545-547, after the slicing
            frames.color_paths = sorted(frames.color_paths, key=extract_number)
            if has_depth:
                frames.depth_paths = sorted(frames.depth_paths, key=extract_number)
        super().__init__(frames, c, device, distorted=False, prefetch=prefetch, max_frames=max_frames, flow=flow, segmenter=segmenter,
                         seg_classes=dataset_classes("CoFusion", d, bool(frames.mask_paths)), motion_segmenter=motion_segmenter)


class EurocDataset(RecordedRGBDDataset):
    """Stereo sequences in the EuRoC layout (utils/dataset.py:376-487, 710-718): Dataset.type 'euroc'. Calibration has ``cam0`` / ``cam1``,
    each with ``raw`` (fx fy cx cy k1 k2 p1 p2 k3), ``opt`` (fx fy cx cy of the rectified camera) and ``R`` {data: 9 numbers}; ``distorted``
    (rectify, or take the images as they are), ``width``, ``height``, ``bf`` (baseline x focal length, default the reference's constant)
    and an optional ``T_i_c0``. Dataset.stereo may set the matcher's num_disparities, p1, p2, uniqueness_ratio and disp12_max_diff
    (slam/stereo.py StereoMatcher). The image handed out is the rectified left picture, grey in three channels; the depth is bf / disparity,
    0 where the matcher found no match; every pixel is static."""

    def __init__(self, config, device="cuda:0", prefetch=4, max_frames=None, flow=None, segmenter=None):
        import torch
        from .stereo import REFERENCE_BF, StereoMatcher, rectify_map
        from .pretrained import EventLog
        if segmenter is not None:
            raise ValueError("Dataset.type 'euroc' takes no segmenter: the reference names no classes to segment for its stereo sequences")
        d, c = config["Dataset"], config["Dataset"]["Calibration"]
        frames = parse_euroc(d["dataset_path"], c.get("T_i_c0")).sliced(int(c.get("start", 0)), int(c.get("end", -1)))
        opt = c["cam0"]["opt"]
        flat = {"fx": opt["fx"], "fy": opt["fy"], "cx": opt["cx"], "cy": opt["cy"], "width": c["width"], "height": c["height"], "depth_scale": 1.0}
        super().__init__(frames, flat, device, distorted=False, prefetch=prefetch, max_frames=max_frames, flow=flow)
        self.bf = float(c.get("bf", REFERENCE_BF))
        self.matcher = StereoMatcher(self.width, self.height, bf=self.bf, device=self.device, **dict(d.get("stereo") or {}))
        self._maps = None
        if bool(c.get("distorted", False)):
            K = lambda p: [[p["fx"], 0.0, p["cx"]], [0.0, p["fy"], p["cy"]], [0.0, 0.0, 1.0]]
            self._maps = tuple(torch.tensor(rectify_map(K(c[cam]["raw"]), [c[cam]["raw"].get(k, 0.0) for k in ("k1", "k2", "p1", "p2", "k3")],
                                                        c[cam]["R"]["data"], K(c[cam]["opt"]), self.width, self.height), device=self.device)
                               for cam in ("cam0", "cam1"))
        torch.cuda.synchronize(self.device)             # the maps and the matcher's table exist before the side stream reads them
        self._motion = torch.ones((self.height, self.width), dtype=torch.bool, device=self.device)
        self._stereo_log = EventLog(self.device)
        self._depth_wait_ms, self._valid_share = 0.0, []

    _decode = staticmethod(frame_decode.decode_stereo_frame)

    def _decode_tasks(self, frames):
        return [(frames.color_paths[i], frames.right_paths[i], self.width, self.height) for i in range(self.num_imgs)]

    @property
    def stereo_stats(self):
        """Frames matched, the device ms per frame (rectify + match + depth), the host ms spent waiting for the depth copies, and the mean
        share of pixels with a depth."""
        t = self._stereo_log.summary()
        return {"frames": t["calls"], **self.matcher.params, "ms_per_frame": t["ms_per_item"], "ms_first": t["ms_first"],
                "ms_rest_mean": t["ms_per_item_rest"], "depth_wait_ms_total": self._depth_wait_ms,
                "depth_density_mean": float(np.mean(self._valid_share)) if self._valid_share else None}

    @property
    def ingest_stats(self):
        return dict(super().ingest_stats, stereo=self.stereo_stats)

    def __getitem__(self, idx):
        if not 0 <= idx < self.num_imgs:
            raise IndexError(f"frame {idx} of a {self.num_imgs}-frame sequence")
        image, depth_h, done = self._prepare(self._reader.get(idx), host_depth=True)
        t0 = time.perf_counter()
        done.synchronize()                              # the interface hands out a host array: wait for the copy into pinned memory
        self._depth_wait_ms += (time.perf_counter() - t0) * 1e3
        depth = depth_h.numpy().copy()
        self._valid_share.append(float((depth > 0).mean()))
        return image, depth, self.poses[idx].clone(), self._motion.clone()

    def _prepare(self, hf, segment=False, host_depth=False):
        """(image, pinned host depth, event) -- rectify, match and bf / disparity on the side stream, then the copy of the depth to pinned
        memory; the caller's stream waits for the image. Without host_depth only the image matters (a keyframe the flow term reads again)."""
        import torch
        dev = self.device
        main = torch.cuda.current_stream(dev)
        left_h, right_h = torch.from_numpy(hf.left).pin_memory(), torch.from_numpy(hf.right).pin_memory()
        depth_h = done = None
        with torch.cuda.stream(self._side):
            left, right = left_h.to(dev, non_blocking=True), right_h.to(dev, non_blocking=True)
            with self._stereo_log.timed(self._side):
                image, _, depth = self.matcher(left, right, maps=self._maps, stream=self._side)
            if host_depth:
                depth_h = torch.empty((self.height, self.width), dtype=torch.float32).pin_memory()
                depth_h.copy_(depth, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
        main.wait_event(done)
        image.record_stream(main)
        return image, depth_h, done


class VideoDataset:
    """A plain video, with no ground truth beside it: Dataset.type 'video'. ``Dataset.dataset_path`` is a Motion-JPEG AVI file or a folder
    of .jpg / .jpeg files (slam/jpeg_decode.py AviIndex, JpegFolder); Calibration as for 'tum' (fx fy cx cy width height, distorted and
    k1 k2 p1 p2 k3, start / end); Dataset.sensor_type must be 'monocular'. The read-ahead thread reads and parses the frames' headers; the
    pictures are decoded on the device, on the side stream, `prefetch` consecutive frames per call (mjpeg.jpeg_decode, include/video_io.h
    gsr_jpeg_decode), and kept as bytes in a bounded cache because evaluation reads frames again in any order. Each picture then goes through
    gsr_frame_prepare like every other dataset's. A frame is (image, None, identity, all-static mask): there is no depth and no ground truth
    (``has_ground_truth`` is False). ``stamps`` are the frames' times in seconds (frame index / frame rate; the index for a folder)."""

    DECODED_CACHE_FRAMES = 32      # decoded byte pictures kept on the device (0.9 MB each at 640x480)
    has_ground_truth = False

    def __init__(self, config, device="cuda:0", prefetch=4, max_frames=None, flow=None, segmenter=None, motion_segmenter=None):
        import torch
        from . import jpeg_decode
        from .camera import getProjectionMatrix2
        from .pretrained import EventLog
        d, c = config["Dataset"], config["Dataset"]["Calibration"]
        if d.get("sensor_type") != "monocular":
            raise ValueError(f"Dataset.type 'video' needs Dataset.sensor_type 'monocular', got {d.get('sensor_type')!r}: a video file has no depth")
        for name, given in (("flow estimator", flow), ("segmenter", segmenter), ("motion segmenter", motion_segmenter)):
            if given is not None:
                raise ValueError(f"Dataset.type 'video' takes no {name}: the static monocular run is what a plain video feeds")
        self.device = torch.device(device)
        self.fx, self.fy, self.cx, self.cy = float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"])
        self.width, self.height = int(c["width"]), int(c["height"])
        self.fovx, self.fovy = fov_from_focal(self.fx, self.width), fov_from_focal(self.fy, self.height)
        self.depth_scale = None
        self.source = jpeg_decode.open_source(d["dataset_path"])
        info = self.source.info
        if "width" in info and (info["width"], info["height"]) != (self.width, self.height):
            raise ValueError(f"{d['dataset_path']}: the video is {info['width']} x {info['height']}, the calibration says {self.width} x {self.height}")
        start, end = int(c.get("start", 0)), int(c.get("end", -1))
        ids = list(range(len(self.source)))[start:len(self.source) if end == -1 else end]
        if max_frames is not None:
            ids = ids[:int(max_frames)]
        if not ids:
            raise ValueError(f"{d['dataset_path']}: the sequence has no frames (after Calibration start / end)")
        self._ids = ids
        self.num_imgs = len(ids)
        self.stamps = [float(self.source.time(k)) for k in ids]
        self.dynamic_objects = 0
        self.projection_matrix = getProjectionMatrix2(0.01, 100.0, self.cx, self.cy, self.fx, self.fy, self.width,
                                                      self.height).transpose(0, 1).to(self.device)
        self.poses = torch.eye(4, dtype=torch.float32, device=self.device).repeat(self.num_imgs, 1, 1)
        self._lut = torch.tensor(byte_lut(), device=self.device)
        self._map = None
        if bool(c.get("distorted", False)):
            m = undistort_map(self.width, self.height, self.fx, self.fy, self.cx, self.cy,
                              *(float(c.get(k, 0.0)) for k in ("k1", "k2", "p1", "p2", "k3")))
            self._map = torch.tensor(m, device=self.device)
        torch.cuda.synchronize(self.device)             # the tables exist before the side stream reads them
        self._side = torch.cuda.Stream(self.device)
        self.chunk = max(1, int(prefetch))
        self._decoded = collections.OrderedDict()       # frame -> (rgb8 [H, W, 3] on the device, its call's host status, position, event)
        self._decode_log = EventLog(self.device)
        self._workspace = None
        tasks = [(self.source, k, self.width, self.height) for k in ids]
        self._reader = _Reader(tasks, int(prefetch), cache=2 * self.chunk + 4, decode=jpeg_decode.read_frame)
        self._finalizer = weakref.finalize(self, self._reader.close)
        self._reader.schedule(0)
        self._reader.get(0)                             # the reader is up and frame 0 is parsed before the dataset is handed out
        self._reader.stats.update(wait_ms=0.0, prefetched=0, on_demand=0)

    def __len__(self):
        return self.num_imgs

    def close(self):
        """Stop the reader thread (also done when the dataset is dropped and at interpreter exit)."""
        self._finalizer()

    @property
    def ingest_stats(self):
        s = self._reader.stats
        d = np.asarray(s["decode_ms"], dtype=np.float64)
        t = self._decode_log.summary()
        return {"decode_ms_mean": float(d.mean()) if len(d) else None, "decode_ms_p95": float(np.percentile(d, 95)) if len(d) else None,
                "decoded": int(len(d)), "wait_ms_total": s["wait_ms"], "prefetched": s["prefetched"], "on_demand": s["on_demand"],
                "cached": s["cached"], "prefetch_depth": self._reader.depth, "device_decode_ms_per_frame": t["ms_per_item"],
                "device_decode_calls": t["calls"], "device_decoded": t["items"], "device_decode_chunk": self.chunk}

    def _decode_chunk(self, idx):
        """Decode frame idx and the frames behind it that are not decoded yet, up to `chunk`, of its sampling, in one call on the side stream."""
        import torch
        from . import jpeg_decode, mjpeg
        dev, H, W = self.device, self.height, self.width
        parsed = [self._reader.get(idx)]
        for k in range(idx + 1, min(idx + self.chunk, self.num_imgs)):
            if k in self._decoded:
                break
            f = self._reader.get(k)
            if f.sampling != parsed[0].sampling:
                break
            parsed.append(f)
        p = jpeg_decode.pack(parsed)
        n = len(parsed)
        host = {k: torch.from_numpy(p[k].view(np.int16) if k == "qtables" else np.ascontiguousarray(p[k])).pin_memory()
                for k in ("scans", "offsets", "qtables", "huffman", "descriptors")}
        status_h = torch.empty(n, dtype=torch.int32).pin_memory()
        with torch.cuda.stream(self._side):
            t = {k: v.to(dev, non_blocking=True) for k, v in host.items()}
            rgb8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            status = torch.empty(n, dtype=torch.int32, device=dev)
            need = mjpeg.jpeg_decode_workspace_size(n, W, H, p["sampling"], p["max_intervals"])
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)          # (used on the side stream only)
            with self._decode_log.timed(self._side, count=n):
                mjpeg.jpeg_decode(t["scans"], t["offsets"], t["qtables"], t["huffman"], t["descriptors"], rgb8, status, p["sampling"],
                                  p["max_intervals"], None, self._workspace, self._side)
            status_h.copy_(status, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self._side)
        for j in range(n):
            self._decoded[idx + j] = (rgb8[j], status_h, j, done)
        while len(self._decoded) > max(self.DECODED_CACHE_FRAMES, self.chunk):
            self._decoded.popitem(last=False)

    def _picture(self, idx):
        """Frame idx as bytes [H, W, 3] on the device, decoded on the side stream (which the caller must still wait for)."""
        if idx not in self._decoded:
            self._decode_chunk(idx)
        self._decoded.move_to_end(idx)
        rgb8, status_h, j, done = self._decoded[idx]
        done.synchronize()                              # the status is read on the host: a damaged frame is refused, not shown
        if int(status_h[j]) != 0:
            raise ValueError(f"{self.source.name(self._ids[idx])}: the entropy-coded data cannot be decoded (GSR_JPEG status {int(status_h[j])}, "
                             "include/video_io.h)")
        return rgb8

    def __getitem__(self, idx):
        import torch
        from . import frame_io
        if not 0 <= idx < self.num_imgs:
            raise IndexError(f"frame {idx} of a {self.num_imgs}-frame sequence")
        H, W, dev = self.height, self.width, self.device
        rgb8 = self._picture(idx)
        main = torch.cuda.current_stream(dev)
        with torch.cuda.stream(self._side):
            image = torch.empty((3, H, W), dtype=torch.float32, device=dev)
            motion = torch.empty((H, W), dtype=torch.bool, device=dev)
            frame_io.frame_prepare(rgb8, self._map, self._lut, None, MASK_THRESHOLD, image, motion, self._side)
            ready = torch.cuda.Event()
            ready.record(self._side)
        main.wait_event(ready)
        image.record_stream(main)                       # allocated on the side stream, used (and freed) on the caller's
        motion.record_stream(main)
        return image, None, self.poses[idx].clone(), motion


SUPPORTED_TYPES = ("tum", "CoFusion", "euroc", "video")


def load_dataset(config, device="cuda:0", prefetch=4, max_frames=None, flow=None, segmenter=None, motion_segmenter=None):
    """utils/dataset.py:962-976 for the recorded types this project reads: 'tum' (TUM, Bonn), 'CoFusion', 'euroc' (stereo) and 'video' (a
    Motion-JPEG AVI file or a folder of JPEG files without ground truth, decoded on the device: VideoDataset). flow: an optical-flow
    estimator (slam/optical_flow.py RaftFlow) that gives the dataset gt_flow, or None. segmenter: a YOLO instance segmenter
    (slam/segmentation.py YoloSeg) whose masks of the loader's classes are cleared from the motion masks, or None. motion_segmenter: a
    class-agnostic segmenter from flow and depth (slam/motion_segmentation.py FlowMotionSegmenter; needs flow and an RGB-D type), or None."""
    kind = config["Dataset"].get("type")
    if kind == "tum":
        return TUMDataset(config, device, prefetch=prefetch, max_frames=max_frames, flow=flow, segmenter=segmenter, motion_segmenter=motion_segmenter)
    if kind == "CoFusion":
        return CoFusionDataset(config, device, prefetch=prefetch, max_frames=max_frames, flow=flow, segmenter=segmenter,
                               motion_segmenter=motion_segmenter)
    if kind == "euroc":
        if motion_segmenter is not None:
            raise ValueError("Dataset.type 'euroc' takes no motion segmenter: segmenting stereo sequences from flow is not supported")
        return EurocDataset(config, device, prefetch=prefetch, max_frames=max_frames, flow=flow, segmenter=segmenter)
    if kind == "video":
        return VideoDataset(config, device, prefetch=prefetch, max_frames=max_frames, flow=flow, segmenter=segmenter, motion_segmenter=motion_segmenter)
    raise ValueError(f"unknown dataset type {kind!r}: the supported types are 'tum' (TUM RGB-D, Bonn), 'CoFusion', 'euroc' (stereo) and "
                     "'video' (a Motion-JPEG AVI file or a folder of JPEG files, no ground truth)")


# ---- writing a sequence (tests, measurements, exporting the synthetic generator) --------------------------------------------------
def rotation_to_quaternion(R):
    """(qx, qy, qz, qw) of a rotation matrix (Shepperd's method, float64)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * math.sqrt(tr + 1.0)
        w, x, y, z = 0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        w, x, y, z = (R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * math.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        w, x, y, z = (R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s
    else:
        s = 2.0 * math.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        w, x, y, z = (R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s
    return np.array([x, y, z, w])


def tum_stamp(i, t0=1000.0, hz=30.0):
    """The time stamp of frame i of a written sequence, as the six-decimal text its files and lists are named by."""
    return f"{t0 + i / hz:.6f}"


def write_tum_lists(root, stamps, c2w_poses, origin="written from an in-memory dataset"):
    """rgb.txt, depth.txt and groundtruth.txt (C2W as tx ty tz qx qy qz qw) of a sequence whose images are rgb/<stamp>.png, depth/<stamp>.png."""
    rgb_lines = [f"{t} rgb/{t}.png" for t in stamps]
    depth_lines = [f"{t} depth/{t}.png" for t in stamps]
    pose_lines = [f"{t} " + " ".join(f"{v:.12f}" for v in (*c2w[:3, 3], *rotation_to_quaternion(c2w[:3, :3]))) for t, c2w in zip(stamps, c2w_poses)]
    for name, header, lines in (("rgb.txt", f"# color images\n# file: {origin}\n# timestamp filename\n", rgb_lines),
                                ("depth.txt", f"# depth maps\n# file: {origin}\n# timestamp filename\n", depth_lines),
                                ("groundtruth.txt", f"# ground truth trajectory\n# file: {origin}\n"
                                                    "# timestamp tx ty tz qx qy qz qw\n", pose_lines)):
        with open(os.path.join(root, name), "w") as f:
            f.write(header + "\n".join(lines) + "\n")


def write_tum_sequence(dataset, root, masks=False, t0=1000.0, hz=30.0):
    """Write the frames of an in-memory dataset (slam/dataset.py interface) in the TUM layout: rgb/*.png = round(colour * 255),
    depth/*.png = round(depth * 5000) as 16-bit, groundtruth.txt (C2W as tx ty tz qx qy qz qw) and, with masks=True, render_mask/*.png
    (255 on moving pixels). Returns the Calibration block of a config for it."""
    from PIL import Image
    for d in ("rgb", "depth") + (("render_mask",) if masks else ()):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    stamps, c2ws = [], []
    for i in range(len(dataset)):
        color, depth, pose, motion = dataset[i]
        t = tum_stamp(i, t0, hz)
        c = np.rint(color.clamp(0, 1).permute(1, 2, 0).cpu().numpy().astype(np.float64) * 255).astype(np.uint8)
        Image.fromarray(c).save(os.path.join(root, "rgb", f"{t}.png"))
        Image.fromarray(np.rint(np.asarray(depth, np.float64) * 5000).astype(np.uint16)).save(os.path.join(root, "depth", f"{t}.png"))
        if masks:
            Image.fromarray(np.where(motion.cpu().numpy(), 0, 255).astype(np.uint8)).save(os.path.join(root, "render_mask", f"mask_{i}.png"))
        stamps.append(t)
        c2ws.append(np.linalg.inv(pose.double().cpu().numpy()))
    write_tum_lists(root, stamps, c2ws)
    return {"fx": float(dataset.fx), "fy": float(dataset.fy), "cx": float(dataset.cx), "cy": float(dataset.cy), "k1": 0.0, "k2": 0.0, "p1": 0.0,
            "p2": 0.0, "k3": 0.0, "distorted": False, "width": int(dataset.width), "height": int(dataset.height), "depth_scale": 5000.0}


def euroc_stamp(i, t0=1000.0, hz=30.0):
    """The nanosecond time stamp of frame i of a written stereo sequence: what its images are named by and its csv rows start with."""
    return int(round((t0 + i / hz) * 1e9))


def grey_bytes(color):
    """8-bit luma (ITU-R BT.601 weights, rounded) of a [3, H, W] colour image in [0, 1]."""
    c = color.clamp(0, 1).double().cpu().numpy()
    return np.rint((0.299 * c[0] + 0.587 * c[1] + 0.114 * c[2]) * 255).astype(np.uint8)


def write_euroc_sequence(dataset, root, baseline, t0=1000.0, hz=30.0):
    """Write the frames of an in-memory dataset that has ``right_view`` (slam/dataset.py) as a rectified stereo sequence in the EuRoC
    layout: mav0/cam0/data/<ns>.png and mav0/cam1/data/<ns>.png (8-bit grey), mav0/state_groundtruth_estimate0/data.csv with the left
    camera's C2W pose as the body pose (so the Calibration carries T_i_c0 = identity). Returns the Calibration block of a config for it:
    both cameras with the dataset's intrinsics, no distortion, R = I, bf = fx * baseline."""
    from PIL import Image
    dirs = {k: os.path.join(root, "mav0", k, "data") for k in ("cam0", "cam1")}
    gt_dir = os.path.join(root, "mav0", "state_groundtruth_estimate0")
    for d in (*dirs.values(), gt_dir):
        os.makedirs(d, exist_ok=True)
    lines = ["#timestamp, p_RS_R_x [m], p_RS_R_y [m], p_RS_R_z [m], q_RS_w [], q_RS_x [], q_RS_y [], q_RS_z []"]
    for i in range(len(dataset)):
        color, _, pose, _ = dataset[i]
        stamp = euroc_stamp(i, t0, hz)
        Image.fromarray(grey_bytes(color)).save(os.path.join(dirs["cam0"], f"{stamp}.png"))
        Image.fromarray(grey_bytes(dataset.right_view(i, baseline))).save(os.path.join(dirs["cam1"], f"{stamp}.png"))
        c2w = np.linalg.inv(pose.double().cpu().numpy())
        x, y, z, w = rotation_to_quaternion(c2w[:3, :3])
        lines.append(",".join([str(stamp)] + [f"{v:.12f}" for v in (*c2w[:3, 3], w, x, y, z)]))
    with open(os.path.join(gt_dir, "data.csv"), "w") as f:
        f.write("\n".join(lines) + "\n")
    k = {"fx": float(dataset.fx), "fy": float(dataset.fy), "cx": float(dataset.cx), "cy": float(dataset.cy)}
    cam = {"raw": dict(k, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0), "opt": dict(k), "R": {"data": [float(v) for v in np.eye(3).reshape(-1)]}}
    return {"cam0": cam, "cam1": {"raw": dict(cam["raw"]), "opt": dict(k), "R": {"data": list(cam["R"]["data"])}}, "distorted": False,
            "width": int(dataset.width), "height": int(dataset.height), "bf": float(dataset.fx) * float(baseline),
            "T_i_c0": [[float(v) for v in row] for row in np.eye(4)]}
