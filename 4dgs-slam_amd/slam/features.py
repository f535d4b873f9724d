"""The relative pose of two frames from matched binary features: the wide-baseline step between place recognition (the ferns of
slam/relocalise.py) and the dense alignment (slam/odometry.py), whose reach is its basin of convergence. The checked ctypes binding of
include/feature_matching.h (gsr_feat_extract: FAST-9 corners and rotated BRIEF descriptors in a fixed slot layout; gsr_feat_match: the mutual
ratio-tested Hamming match; gsr_feat_pose: three-point RANSAC, a point-to-point refinement and a gate; gsr_feat_pose_pnp: the same from
the 3D points of the first frame and the pixels of the second alone, for a second frame without depth; csrc/gs_features.h) and what is
built from them:

  pattern_tables        the direction table and the rotated point pairs, built on the host from a seed
  feature_seed_options  the ``Training.feature_seed`` block
  FeatureSeeder         features(image, mask) and pose(a, depth_a, b, depth_b) for frames of one size, everything on the device; with
                        ``solver: pnp`` depth_b is never touched and may be None (a monocular frame)

Relocaliser._seed (slam/relocalise.py) and LoopCloser.verify (slam/loop_closure.py) start the dense alignment at the pose found here when
the block is on. The reference has no counterpart. tests/features_reference.py and tests/pnp_reference.py restate the kernels in numpy.
No CPU path.

Limits: nothing here has been run on real images. One scale only (no pyramid). The PnP solver follows one root of the three-point
problem, the one next to the first frame's ranges (no complete P3P), and its pose is coarser than the 3D-3D one: a start for the dense
alignment, not a replacement for it (Feature seed)."""
import math

import numpy as np
import torch

from diff_gaussian_rasterization import _C

from .camera import frame_tensors
from .options import check_gate, read_block, to_floats

I32 = (torch.int32,)
I8 = (torch.int8,)
MASK = (torch.uint8, torch.bool)
STATS = ("keypoints_a", "keypoints_b", "pairs", "winner", "winner_inliers", "inliers", "accepted", "zero7")
MAX_SLOTS, MAX_HYPOTHESES, BINS, PAIRS, WORDS = 4096, 1024, 32, 256, 8
MIN_AREA = 0.05                                # metres: the height of a sampled triangle below which its frame is too poorly held


# ---- the three calls -----------------------------------------------------------------------------------------------------------------
def slot_count(width, height, cell, per_cell):
    """The slots of a frame; 0 outside the ranges of gsr_feat_extract."""
    return int(_C.load_library().gsr_feat_slots(int(width), int(height), int(cell), int(per_cell)))


def extract(image, mask, cell, per_cell, threshold, directions, pattern, keypoints, descriptors, workspace=None, stream=None):
    """One call of gsr_feat_extract. image float32 [3, H, W]; mask None or uint8 / bool [H, W] (0 = no corner there); directions int32 [32, 2]
    and pattern int8 [32, 256, 4] on the device (pattern_tables); keypoints int32 [slots, 4] rows (x, y, score, bin) and descriptors int32
    [slots, 8] (the bits of the uint32 words) are written. The library checks the ranges and raises RuntimeError with its text."""
    _C._require_device(image, "image")
    if image.dim() != 3 or image.shape[0] != 3:
        raise RuntimeError(f"image must be [3, H, W], got {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    slots = int(keypoints.shape[0])
    args = [_C.dev_ptr(image, "image", _C.F32, (3, H, W)), _C.dev_ptr(mask, "mask", MASK, (H, W))]
    tables = [_C.dev_ptr(directions, "directions", I32, (BINS, 2)), _C.dev_ptr(pattern, "pattern", I8, (BINS, PAIRS, 4))]
    lib = _C.load_library()
    want = int(lib.gsr_feat_slots(W, H, int(cell), int(per_cell)))
    if want and slots != want:
        raise RuntimeError(f"keypoints must hold {want} slots, got {tuple(keypoints.shape)}")
    outs = [_C.dev_ptr(keypoints, "keypoints", I32, (slots, 4)), _C.dev_ptr(descriptors, "descriptors", I32, (slots, WORDS))]
    workspace = _C.workspace(workspace, int(lib.gsr_feat_extract_workspace_size(W, H)) if workspace is None else 0, image.device)
    with torch.cuda.device(image.device):
        lib.gsr_feat_extract(W, H, *args, int(cell), int(per_cell), int(threshold), *tables, *outs, workspace.data_ptr() or None,
                             int(workspace.numel()), _C.stream_handle(stream, image.device))


def match(keypoints_a, descriptors_a, keypoints_b, descriptors_b, max_distance, ratio_eighths, matches, workspace=None, stream=None):
    """One call of gsr_feat_match: matches int32 [slots_a, 2] is written, rows (b, d) or (-1, d)."""
    _C._require_device(keypoints_a, "keypoints_a")
    A, B, dev = int(keypoints_a.shape[0]), int(keypoints_b.shape[0]), keypoints_a.device
    args = [A, _C.dev_ptr(keypoints_a, "keypoints_a", I32, (A, 4)), _C.dev_ptr(descriptors_a, "descriptors_a", I32, (A, WORDS)),
            B, _C.dev_ptr(keypoints_b, "keypoints_b", I32, (B, 4)), _C.dev_ptr(descriptors_b, "descriptors_b", I32, (B, WORDS))]
    lib = _C.load_library()
    workspace = _C.workspace(workspace, int(lib.gsr_feat_match_workspace_size(A, B)) if workspace is None else 0, dev)
    with torch.cuda.device(dev):
        lib.gsr_feat_match(*args, int(max_distance), int(ratio_eighths), _C.dev_ptr(matches, "matches", I32, (A, 2)),
                           workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, dev))


def pose(keypoints_a, depth_a, keypoints_b, depth_b, matches, K_a, K_b, T, stats, seed=0, hypotheses=256, min_area=MIN_AREA, tau_px=2.0,
         tau_depth=0.05, refine_iters=3, min_matches=12, min_inliers=8, min_share=0.5, max_translation=1.5, max_rotation=math.radians(45.0),
         counts=None, workspace=None, stream=None):
    """One call of gsr_feat_pose. depth_a, depth_b float32 [H, W]; K_a, K_b float32 [4] = (fx, fy, cx, cy) on the device; max_rotation in
    radians. T float32 [4, 4], stats int32 [8] (STATS) and, if given, counts int32 [hypotheses] are written."""
    _C._require_device(depth_a, "depth_a")
    H, W = int(depth_a.shape[0]), int(depth_a.shape[1])
    A, B, dev = int(keypoints_a.shape[0]), int(keypoints_b.shape[0]), depth_a.device
    args = [W, H, A, _C.dev_ptr(keypoints_a, "keypoints_a", I32, (A, 4)), _C.dev_ptr(depth_a, "depth_a", _C.F32, (H, W)),
            B, _C.dev_ptr(keypoints_b, "keypoints_b", I32, (B, 4)), _C.dev_ptr(depth_b, "depth_b", _C.F32, (H, W)),
            _C.dev_ptr(matches, "matches", I32, (A, 2)), _C.dev_ptr(K_a, "K_a", _C.F32, (4,)), _C.dev_ptr(K_b, "K_b", _C.F32, (4,))]
    outs = [_C.dev_ptr(T, "T", _C.F32, (4, 4)), _C.dev_ptr(stats, "stats", I32, (len(STATS),)),
            _C.dev_ptr(counts, "counts", I32, (int(hypotheses),))]
    lib = _C.load_library()
    workspace = _C.workspace(workspace, int(lib.gsr_feat_pose_workspace_size(A, int(hypotheses))) if workspace is None else 0, dev)
    with torch.cuda.device(dev):
        lib.gsr_feat_pose(*args, int(seed) & 0xFFFFFFFF, int(hypotheses), float(min_area), float(tau_px), float(tau_depth), int(refine_iters),
                          int(min_matches), int(min_inliers), float(min_share), float(max_translation), float(max_rotation), *outs,
                          workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, dev))


def pose_pnp(keypoints_a, depth_a, keypoints_b, matches, K_a, K_b, T, stats, seed=0, hypotheses=256, min_area=MIN_AREA, tau_px=2.0,
             refine_iters=3, min_matches=12, min_inliers=8, min_share=0.5, max_translation=1.5, max_rotation=math.radians(45.0), counts=None,
             workspace=None, stream=None):
    """One call of gsr_feat_pose_pnp: pose() from the depth of frame A and the pixels of frame B; no depth of B and no tau_depth. The
    frame size is depth_a's."""
    _C._require_device(depth_a, "depth_a")
    H, W = int(depth_a.shape[0]), int(depth_a.shape[1])
    A, B, dev = int(keypoints_a.shape[0]), int(keypoints_b.shape[0]), depth_a.device
    args = [W, H, A, _C.dev_ptr(keypoints_a, "keypoints_a", I32, (A, 4)), _C.dev_ptr(depth_a, "depth_a", _C.F32, (H, W)),
            B, _C.dev_ptr(keypoints_b, "keypoints_b", I32, (B, 4)), _C.dev_ptr(matches, "matches", I32, (A, 2)),
            _C.dev_ptr(K_a, "K_a", _C.F32, (4,)), _C.dev_ptr(K_b, "K_b", _C.F32, (4,))]
    outs = [_C.dev_ptr(T, "T", _C.F32, (4, 4)), _C.dev_ptr(stats, "stats", I32, (len(STATS),)),
            _C.dev_ptr(counts, "counts", I32, (int(hypotheses),))]
    lib = _C.load_library()
    workspace = _C.workspace(workspace, int(lib.gsr_feat_pose_pnp_workspace_size(A, int(hypotheses))) if workspace is None else 0, dev)
    with torch.cuda.device(dev):
        lib.gsr_feat_pose_pnp(*args, int(seed) & 0xFFFFFFFF, int(hypotheses), float(min_area), float(tau_px), int(refine_iters),
                              int(min_matches), int(min_inliers), float(min_share), float(max_translation), float(max_rotation), *outs,
                              workspace.data_ptr() or None, int(workspace.numel()), _C.stream_handle(stream, dev))


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def pattern_tables(seed):
    """(directions int32 [32, 2], pattern int8 [32, 256, 4]) on the host. directions[k] = round(256 cos, 256 sin) of 2 pi k / 32. The 256
    point pairs of bin 0 come from np.random.default_rng(seed): normal with sigma 31 / 5 (Calonder et al., "BRIEF"), redrawn until inside
    radius 15; bin k holds them rotated by 2 pi k / 32 and rounded, so every entry lies in [-16, 16]. The same seed gives the same bytes."""
    angles = 2.0 * np.pi * np.arange(BINS) / BINS
    directions = np.stack([np.rint(256.0 * np.cos(angles)), np.rint(256.0 * np.sin(angles))], axis=1).astype(np.int32)
    rng = np.random.default_rng(int(seed))
    points = np.empty((0, 2))
    while len(points) < 2 * PAIRS:
        draw = rng.normal(0.0, 31.0 / 5.0, size=(4 * PAIRS, 2))
        points = np.concatenate([points, draw[np.hypot(draw[:, 0], draw[:, 1]) <= 15.0]])
    points = points[:2 * PAIRS].reshape(PAIRS, 2, 2)                   # [pair, a / b, x / y]
    c, s = np.cos(angles)[:, None, None], np.sin(angles)[:, None, None]
    x, y = points[None, :, :, 0], points[None, :, :, 1]
    rotated = np.stack([c * x - s * y, s * x + c * y], axis=-1)        # [bin, pair, a / b, x / y]
    return directions, np.rint(rotated).astype(np.int8).reshape(BINS, PAIRS, 4)


# ---- options -------------------------------------------------------------------------------------------------------------------------
# cell 32 with 4 per cell gives 1200 slots at 640 x 480; the thresholds of the match and of the pose are those of the prototype the stage
# was specified from; the gate lies between what the analytic scene's true pairs gave (20 or more pairs, shares of 0.8 and more) and what
# unrelated textures gave (at most 9 pairs and 1 inlier): DESIGN.md section 8, Feature seed
FEATURE_SEED_DEFAULTS = {"enabled": False, "threshold": 20, "cell": 32, "per_cell": 4, "seed": 0, "max_distance": 64, "ratio_eighths": 6,
                         "hypotheses": 256, "tau_px": 2.0, "tau_depth": 0.05, "min_matches": 12, "min_inliers": 8, "min_share": 0.5,
                         "refine_iters": 3, "max_translation": 1.5, "max_rotation": 45.0, "solver": "points"}
SOLVERS = ("points", "pnp")


def feature_seed_options(training):
    """The ``Training.feature_seed`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys, values the
    kernels cannot take and the runs the stage cannot serve are refused here, before the run starts. max_translation is in metres,
    max_rotation in degrees: the gate of the feature pose AND of the dense alignment that starts from it. solver: "points" (both frames'
    depths, gsr_feat_pose) or "pnp" (the first frame's depth and the second frame's pixels, gsr_feat_pose_pnp: the one that serves
    monocular input); "pnp" has no depth test and ignores tau_depth."""
    name = "Training.feature_seed"
    opt = read_block(training, "feature_seed", FEATURE_SEED_DEFAULTS)
    if opt is None:
        return None
    if opt["solver"] not in SOLVERS:
        raise ValueError(f"{name}.solver must be one of {list(SOLVERS)}, got {opt['solver']!r}")
    if training.get("monocular", False) and opt["solver"] != "pnp":
        raise ValueError(f"{name} cannot be used with monocular input: a frame has no depth to back-project its keypoints with, and a pose "
                         "from 2D-3D matches (PnP) is not part of this stage unless solver is 'pnp'")
    if not any((training.get(k) or {}).get("enabled", False) for k in ("relocalisation", "loop_closure")):
        raise ValueError(f"{name} needs Training.relocalisation or Training.loop_closure enabled: it seeds their alignments and would do "
                         "nothing by itself")
    ranges = {"threshold": (0, 255), "cell": (8, 64), "per_cell": (1, 8), "seed": (0, 2 ** 32 - 1), "max_distance": (0, 256),
              "ratio_eighths": (0, 8), "hypotheses": (1, MAX_HYPOTHESES), "min_matches": (0, MAX_SLOTS), "min_inliers": (3, MAX_SLOTS),
              "refine_iters": (0, 16)}
    for key, (lo, hi) in ranges.items():
        if isinstance(opt[key], bool) or (isinstance(opt[key], float) and not opt[key].is_integer()):
            raise ValueError(f"{name}.{key} must be an integer, got {opt[key]!r}")
        opt[key] = int(opt[key])
        if not lo <= opt[key] <= hi:
            raise ValueError(f"{name}.{key} must be in [{lo}, {hi}], got {opt[key]}")
    to_floats(opt, name, ("tau_px", "tau_depth", "min_share", "max_translation", "max_rotation"))
    for key in ("tau_px", "tau_depth"):
        if not 0.0 <= opt[key] < math.inf:
            raise ValueError(f"{name}.{key} must be finite and not negative, got {opt[key]}")
    if not 0.0 <= opt["min_share"] <= 1.0:
        raise ValueError(f"{name}.min_share must be in [0, 1], got {opt['min_share']}")
    check_gate(opt, name, ("max_translation", "max_rotation"))
    if not opt["max_translation"] < math.inf:
        raise ValueError(f"{name}.max_translation must be finite, got {opt['max_translation']}")
    return opt


def default_options(**overrides):
    """The enabled block with its defaults (tools, tests): feature_seed_options of a run with relocalisation on."""
    return feature_seed_options({"relocalisation": {"enabled": True}, "feature_seed": {"enabled": True, **overrides}})


# ---- the stage -----------------------------------------------------------------------------------------------------------------------
def gated(T, flag, seed_accepted, max_translation, max_rotation):
    """The narrower gate of an alignment that ran with the wider one, on the device: where the feature pose was refused (seed_accepted,
    a device scalar, is 0) the alignment started where it starts without this stage, and what it found counts only within max_translation
    (metres) and max_rotation (degrees) -- the gate is the last thing the alignment decides, so T and flag are then what the narrow
    alignment gives. Returns (T or the identity, flag or 0)."""
    R, t = T[:3, :3].to(torch.float64), T[:3, 3].to(torch.float64)
    ax = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    angle = torch.atan2(0.5 * torch.linalg.norm(ax), 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
    keep = (seed_accepted > 0) | ((torch.linalg.norm(t) <= float(max_translation)) & (angle <= math.radians(float(max_rotation))))
    return torch.where(keep, T, torch.eye(4, dtype=T.dtype, device=T.device)), flag * keep.to(flag.dtype)


class FeatureSeeder:
    """Features and poses for frames of one size. size = (width, height); K = (fx, fy, cx, cy) of both frames; options:
    feature_seed_options(...).

        a = seeder.features(image_a, mask_a)                 # (keypoints int32 [slots, 4], descriptors int32 [slots, 8]) on the device
        T, stats = seeder.pose(a, depth_a, b, depth_b)       # T [4, 4] float32: P_b = T P_a, the identity where the gate refused; STATS
        a = seeder.cached(frame_id, image, mask)             # features(), kept per frame id: a keyframe is extracted once

    Nothing is read from the device; stats[6] is the accepted flag for whoever reads something anyway. The tables, the workspaces and the
    match buffer are allocated once."""

    def __init__(self, size, K, options, device):
        self.width, self.height, self.options, self.device = int(size[0]), int(size[1]), options, torch.device(device)
        self.slots = slot_count(self.width, self.height, options["cell"], options["per_cell"])
        if self.slots == 0:
            raise ValueError(f"Training.feature_seed: a {self.width} x {self.height} frame with cell {options['cell']} and per_cell "
                             f"{options['per_cell']} has more than {MAX_SLOTS} slots (or is outside what gsr_feat_extract takes)")
        directions, pattern = pattern_tables(options["seed"])
        self.directions, self.pattern = torch.from_numpy(directions).to(self.device), torch.from_numpy(pattern).to(self.device)
        self.K = torch.tensor([float(v) for v in K], dtype=torch.float32, device=self.device)
        lib = _C.load_library()
        sizes = (lib.gsr_feat_extract_workspace_size(self.width, self.height), lib.gsr_feat_match_workspace_size(self.slots, self.slots),
                 lib.gsr_feat_pose_workspace_size(self.slots, options["hypotheses"]),
                 lib.gsr_feat_pose_pnp_workspace_size(self.slots, options["hypotheses"]))
        self._workspace = torch.empty(max(int(s) for s in sizes), dtype=torch.uint8, device=self.device)
        self._matches = torch.empty((self.slots, 2), dtype=torch.int32, device=self.device)
        self._cache = {}
        self.tried = 0
        self._accepted = torch.zeros((), dtype=torch.int32, device=self.device)        # summed on the device, read by summary() alone

    def features(self, image, mask=None):
        image, _, mask = frame_tensors(image, None, mask, self.device)
        opt = self.options
        keypoints = torch.empty((self.slots, 4), dtype=torch.int32, device=self.device)
        descriptors = torch.empty((self.slots, WORDS), dtype=torch.int32, device=self.device)
        extract(image, mask, opt["cell"], opt["per_cell"], opt["threshold"], self.directions, self.pattern, keypoints, descriptors, self._workspace)
        return keypoints, descriptors

    def cached(self, key, image, mask=None):
        if key not in self._cache:
            self._cache[key] = self.features(image, mask)
        return self._cache[key]

    def forget(self):
        self._cache = {}

    def pose(self, a, depth_a, b, depth_b=None, counts=None):
        """The pose of frame b against frame a. With ``solver: pnp`` depth_b is never touched; with "points" it is required."""
        opt = self.options
        pnp = opt["solver"] == "pnp"
        if depth_b is None and not pnp:
            raise ValueError("FeatureSeeder.pose: the second frame has no depth; Training.feature_seed.solver must be 'pnp' for such a frame")
        plane = lambda d: torch.as_tensor(d).detach().to(device=self.device, dtype=torch.float32).reshape(self.height, self.width).contiguous()
        depth_a, depth_b = plane(depth_a), None if pnp else plane(depth_b)
        match(a[0], a[1], b[0], b[1], opt["max_distance"], opt["ratio_eighths"], self._matches, self._workspace)
        T = torch.empty((4, 4), dtype=torch.float32, device=self.device)
        stats = torch.empty(len(STATS), dtype=torch.int32, device=self.device)
        gate = dict(seed=opt["seed"], hypotheses=opt["hypotheses"], tau_px=opt["tau_px"], refine_iters=opt["refine_iters"],
                    min_matches=opt["min_matches"], min_inliers=opt["min_inliers"], min_share=opt["min_share"],
                    max_translation=opt["max_translation"], max_rotation=math.radians(opt["max_rotation"]), counts=counts,
                    workspace=self._workspace)
        if pnp:
            pose_pnp(a[0], depth_a, b[0], self._matches, self.K, self.K, T, stats, **gate)
        else:
            pose(a[0], depth_a, b[0], depth_b, self._matches, self.K, self.K, T, stats, tau_depth=opt["tau_depth"], **gate)
        self.tried += 1
        self._accepted += stats[6]
        return T, stats

    def summary(self):
        """{"feature_seeds_tried", "feature_seeds_accepted"}: the one host read, at the end of a run."""
        return {"feature_seeds_tried": self.tried, "feature_seeds_accepted": int(self._accepted)}
