"""Tracking front-end for RGB-D, stereo and monocular input, single process -- the role of the reference's ``utils/slam_frontend.py``
FrontEnd in its ``single_thread: True`` schedule (the front-end hands every keyframe to the back-end and waits for it, :664-666). The public methods
keep the reference's names and meaning (add_new_keyframe :128-187, initialize :189-207, tracking :335-470, is_keyframe :472-499,
add_to_window :501-562, run :603-833) so that code written against it keeps working; the GUI / wandb / queue plumbing does not exist
here, the back-end is called directly.

How a frame is processed:

  track      the pose is optimised against the static Gaussians by ``slam/tracking_graph.TrackingGraph`` -- render (fused prologue,
             static rows gathered inside the kernels, Gaussians DETACHED so that the backward pass runs pose-only) -> fused tracking
             loss -> backward -> ONE camera-step launch (Adam on pose + exposure, update_pose, matrices) -- either replayed as a
             captured hipGraph (``Training.tracking_graph``) or called eagerly; the host only polls the convergence latch every
             ``converge_check_every`` iterations (the reference synchronises every iteration, :440);
  judge      only with ``Training.relocalisation``: the rendering at the tracked pose is scored against the frame (one launch, ONE host
             transfer of eight ints); a refused frame is lost and is looked for among the keyframes (``slam/relocalise.py``); one that is
             not found keeps the previous pose and is passed over;
  decide    one device-side statistics vector per frame (visibility overlap with the newest keyframe, distance to it) decides
             whether the frame becomes a keyframe (``slam/keyframes.py``; ONE host transfer per frame);
  insert     the window update is computed on the device and read back as two indices; the back-end maps the new keyframe.
"""
import math
import struct
import time

import torch

from gaussian_renderer import render

from . import keyframes as kf
from .camera import Camera
from .eval_utils import eval_ate, save_gaussians
from .relocalise import KeyframeIndex, Relocaliser, relocalisation_options, score, verdict


@torch.no_grad()
def render_without_grad(viewpoint, gaussians, pipe, background):
    return render(viewpoint, gaussians, pipe, background, dynamic=False)


def lower_median(x):
    """torch.median's value (the lower of the two middle elements) through a sort: Tensor.median() takes ~3 ms for an image on this
    stack, the sort 0.1 ms."""
    flat = x.reshape(-1)
    if flat.numel() == 0:
        return flat.median()                      # nan + the reference's behaviour on empty input
    return torch.sort(flat)[0][(flat.numel() - 1) // 2]


def get_median_depth(depth, opacity=None, mask=None, return_std=False):
    """utils/slam_utils.py:367-378."""
    depth = depth.detach().clone()
    valid = depth > 0
    if opacity is not None:
        valid = torch.logical_and(valid, opacity.detach() > 0.95)
    if mask is not None:
        valid = torch.logical_and(valid, mask)
    valid_depth = depth[valid]
    if return_std:
        return lower_median(valid_depth), valid_depth.std(), valid
    return lower_median(valid_depth)


MONO_SWEEP_DEFAULTS = {"enabled": False, "partners": 3, "near": 0.25, "p1": 10, "p2": 120, "uniqueness_ratio": 40, "min_span_px": 8}


def mono_sweep_options(training):
    """The ``Training.mono_sweep`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys and values the
    sweep cannot take are refused here, before the run starts."""
    block = training.get("mono_sweep")
    if not block or not block.get("enabled", False):
        return None
    unknown = sorted(set(block) - set(MONO_SWEEP_DEFAULTS))
    if unknown:
        raise ValueError(f"Training.mono_sweep: unknown keys {unknown} (known: {sorted(MONO_SWEEP_DEFAULTS)})")
    opt = dict(MONO_SWEEP_DEFAULTS, **block)
    opt = {"enabled": True, "near": float(opt["near"]), **{k: int(opt[k]) for k in ("partners", "p1", "p2", "uniqueness_ratio", "min_span_px")}}
    if not 1 <= opt["partners"] <= 4:
        raise ValueError(f"Training.mono_sweep.partners must be 1 to 4, got {opt['partners']}")
    if not (0.0 < opt["near"] <= 1.0):
        raise ValueError(f"Training.mono_sweep.near must be in (0, 1] (the nearest swept depth as a share of the median), got {opt['near']}")
    if not (0 < opt["p1"] < opt["p2"] <= 2047) or not 0 <= opt["uniqueness_ratio"] <= 99 or opt["min_span_px"] < 0:
        raise ValueError("Training.mono_sweep needs 0 < p1 < p2 <= 2047, 0 <= uniqueness_ratio <= 99 and min_span_px >= 0, got "
                         f"p1 {opt['p1']}, p2 {opt['p2']}, uniqueness_ratio {opt['uniqueness_ratio']}, min_span_px {opt['min_span_px']}")
    return opt


def merge_sweep_depth(sweep_depth, sweep_valid, gt_img, rgb_boundary_threshold, fallback):
    """The seed depth of a swept keyframe: the sweep's where it is valid and the pixel passes the RGB boundary threshold, else the fallback."""
    use = sweep_valid & (gt_img.sum(dim=0) > rgb_boundary_threshold)
    return torch.where(use, sweep_depth, fallback)


POSE_PRIOR_DEFAULTS = {"enabled": False, "levels": 3, "iters": [5, 7, 10], "nu": 5.0, "sigma_init": 0.1, "sigma_min": 1e-3, "min_share": 0.3,
                       "max_last_step": 1e-2, "max_translation": 0.5, "max_rotation": 20.0, "depth_min": 0.0, "depth_max": 1e6,
                       "constant_velocity": False}


def pose_prior_options(training):
    """The ``Training.pose_prior`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys and values the
    alignment cannot take are refused here, before the run starts. max_translation is in metres (monocular input: map units), max_rotation
    in degrees; iters lists the passes per level, finest first."""
    block = training.get("pose_prior")
    if not block or not block.get("enabled", False):
        return None
    unknown = sorted(set(block) - set(POSE_PRIOR_DEFAULTS))
    if unknown:
        raise ValueError(f"Training.pose_prior: unknown keys {unknown} (known: {sorted(POSE_PRIOR_DEFAULTS)})")
    opt = dict(POSE_PRIOR_DEFAULTS, **block)
    opt["enabled"], opt["constant_velocity"], opt["levels"] = True, bool(opt["constant_velocity"]), int(opt["levels"])
    if not 1 <= opt["levels"] <= 6:
        raise ValueError(f"Training.pose_prior.levels must be 1 to 6, got {opt['levels']}")
    if "iters" not in block and opt["levels"] != POSE_PRIOR_DEFAULTS["levels"]:
        raise ValueError(f"Training.pose_prior.iters must be given with levels = {opt['levels']}: one count per level, finest first")
    if isinstance(opt["iters"], (str, bytes)) or not hasattr(opt["iters"], "__len__"):
        raise ValueError(f"Training.pose_prior.iters must be a list of {opt['levels']} pass counts, finest first, got {opt['iters']!r}")
    opt["iters"] = [int(v) for v in opt["iters"]]
    if len(opt["iters"]) != opt["levels"] or not all(0 <= v <= 64 for v in opt["iters"]):
        raise ValueError(f"Training.pose_prior.iters must hold {opt['levels']} pass counts in [0, 64], finest first, got {opt['iters']}")
    for key in ("nu", "sigma_init", "sigma_min", "min_share", "max_last_step", "max_translation", "max_rotation", "depth_min", "depth_max"):
        opt[key] = float(opt[key])
        if math.isnan(opt[key]):
            raise ValueError(f"Training.pose_prior.{key} must be a number, got nan")
    for key in ("nu", "sigma_init", "sigma_min"):
        if not (0.0 < opt[key] < math.inf):
            raise ValueError(f"Training.pose_prior.{key} must be positive and finite, got {opt[key]}")
    if not 0.0 <= opt["min_share"] <= 1.0:
        raise ValueError(f"Training.pose_prior.min_share must be in [0, 1], got {opt['min_share']}")
    for key in ("max_last_step", "max_translation", "max_rotation"):
        if opt[key] < 0.0:
            raise ValueError(f"Training.pose_prior.{key} must not be negative, got {opt[key]}")
    if opt["max_rotation"] > 180.0:
        raise ValueError(f"Training.pose_prior.max_rotation is in degrees and must not exceed 180, got {opt['max_rotation']}")
    if not 0.0 <= opt["depth_min"] <= opt["depth_max"]:
        raise ValueError(f"Training.pose_prior needs 0 <= depth_min <= depth_max, got {opt['depth_min']} and {opt['depth_max']}")
    return opt


def compose_pose(T, R_prev, t_prev):
    """The world-to-camera pose T W2C_prev of the current frame from the relative motion T [4, 4] (previous camera -> current camera) and the
    previous frame's world-to-camera R [3, 3], t [3]: R = T_R R_prev, t = T_R t_prev + T_t. Tensor operations only."""
    T_R = T[:3, :3].to(R_prev.dtype)
    return T_R @ R_prev, T_R @ t_prev + T[:3, 3].to(t_prev.dtype)


class FrontEnd:
    MIN_KEYFRAME_GAP = 5          # a keyframe at the latest every five frames (utils/slam_frontend.py:739)

    def __init__(self, config: dict):
        training, self.config = config["Training"], config
        self.monocular, self.dynamic_model = training.get("monocular", False), config["model_params"]["dynamic_model"]
        self.converge_check_every = int(training.get("converge_check_every", 5))
        self.use_tracking_graph = bool(training.get("tracking_graph", False))     # slam/tracking_graph.py
        self.device = torch.device("cuda", 0)
        # wired by slam/system.py
        self.background = self.pipeline_params = self.backend = self.dataset = self.gaussians = None
        # map / trajectory state (the attribute names are the reference's: the back-end and the evaluation read them)
        self.cameras, self.kf_indices, self.current_window, self.occ_aware_visibility = {}, [], [], {}
        self.initialized, self.reset = False, True
        self.median_depth, self.use_every_n_frames, self.iteration_count = 1.0, 1, 0
        self.dynamic_objects = self.dystart = 0
        # bookkeeping
        self._tracker = None
        self.graph_stats = {"captures": 0, "replayed_frames": 0, "eager_frames": 0, "overflow_redos": 0}
        self.log = []
        self.init_done_at = None
        self.resets = 0                    # monocular input: how often the map was started over (a failed initialisation)
        self.mono_sweep = mono_sweep_options(training)      # None: a monocular keyframe is seeded the reference's way alone
        self._sweeper, self._sweep_events, self._sweep_shares = None, [], []
        self.pose_prior = pose_prior_options(training)      # None: a frame's tracking starts at the previous frame's pose, as in the reference
        self._odometry = self._prior_motion = None
        self.relocalisation = relocalisation_options(training)      # None: a frame is never judged lost, as in the reference
        self._reloc_index = self._relocaliser = None
        self._reloc_events, self._reloc_stats = [], {"scored": 0, "lost": 0, "relocalised": 0}

    def set_hyperparams(self):
        """:115-126."""
        r, t = self.config["Results"], self.config["Training"]
        self.save_dir, self.save_results = r.get("save_dir"), r.get("save_results", False)
        self.save_trj, self.save_trj_kf_intv = r.get("save_trj", False), r.get("save_trj_kf_intv", 5)
        self.tracking_itr_num, self.kf_interval = t["tracking_itr_num"], t["kf_interval"]
        self.window_size, self.single_thread = t["window_size"], t.get("single_thread", True)

    @property
    def thresholds(self):
        return kf.KeyframeThresholds.from_config(self.config)

    # ---- keyframe depth (:128-187) ---------------------------------------------------------------------------------------
    def add_new_keyframe(self, frame_idx, depth=None, opacity=None, init=False):
        self.kf_indices += [frame_idx]
        viewpoint = self.cameras[frame_idx]
        gt_img = viewpoint.original_image.to(self.device)
        if self.monocular:
            return self._monocular_seed_depth(gt_img, depth, opacity)
        usable = gt_img.sum(dim=0) > self.config["Training"]["rgb_boundary_threshold"]
        if self.dynamic_model and viewpoint.motion_mask is not None:
            usable = usable & viewpoint.motion_mask                       # :185-186: seed the static map from static pixels only
        return viewpoint.depth_device() * usable                          # :180-181 (no host round trip, unlike x[mask] = 0)

    def _monocular_seed_depth(self, gt_img, depth, opacity):
        """:133-174, the use_inv_depth = False arm. The noise comes from the model's generator (tests pin it). First keyframe (no rendering
        yet): 2 + 0.3 noise as three torch launches. Later keyframes: gsr_mono_keyframe_depth (keyframes.mono_keyframe_depth) on the tracked
        frame's rendered depth and opacity; the result stays on the device and feeds gsr_seed_from_rgbd. Fewer than two valid pixels (the
        reference raises or seeds NaN): the kernel returns zeros, nothing is seeded, and the map is started over at the next frame -- the
        count is the one host read of this branch, taken after the kernel is queued."""
        H, W = int(gt_img.shape[-2]), int(gt_img.shape[-1])
        noise = torch.randn((H, W), device=gt_img.device, generator=self.backend.gaussians.generator)
        threshold = self.config["Training"]["rgb_boundary_threshold"]
        if depth is None:
            return (2.0 + 0.3 * noise) * (gt_img.sum(dim=0) > threshold)
        seed_depth, stats = kf.mono_keyframe_depth(depth, opacity, gt_img, threshold, noise)
        if self.mono_sweep is None:
            n_valid = int(stats.view(torch.int32)[2])
        else:                                                 # the same one host read, all three words of it
            median, _, n_valid = stats.view(torch.int32).tolist()
            median = struct.unpack("<f", struct.pack("<i", median))[0]
        if n_valid < 2:
            self.reset = True
            self.log.append(("reset", "no valid depth to seed a keyframe from"))
        elif self.mono_sweep is not None:
            seed_depth = self._sweep_seed_depth(gt_img, seed_depth, median, threshold)
        return seed_depth

    def _sweep_seed_depth(self, gt_img, fallback, median, threshold):
        """``Training.mono_sweep``: the new keyframe's depth from a plane sweep (slam/sweep.py, include/multiview_depth.h) against the most
        recent `partners` keyframes of the window under their tracked poses, inverse depth 0 .. 1 / (near * median) in 63 steps. Where the
        sweep is valid and the pixel passes the RGB boundary threshold its depth is the seed; everywhere else the fallback stands. Nothing
        is read by the host: the valid share is kept on the device and the time in events until the run's summary asks (sweep_summary)."""
        opt = self.mono_sweep
        newest = self.cameras[self.current_window[0]]
        partners = [self.cameras[k] for k in self.current_window[1:1 + opt["partners"]] if self.cameras[k].original_image is not None]
        if not partners or not (median > 0.0 and median < float("inf")):
            return fallback
        if self._sweeper is None:
            from .sweep import PlaneSweep, relative_transforms
            self._sweeper = PlaneSweep(p1=opt["p1"], p2=opt["p2"], uniqueness_ratio=opt["uniqueness_ratio"], min_span_px=opt["min_span_px"],
                                       device=gt_img.device)
            self._relative_transforms = relative_transforms
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        swept = self._sweeper.sweep(gt_img, [cam.original_image for cam in partners], (newest.fx, newest.fy, newest.cx, newest.cy),
                                    self._relative_transforms(newest, partners), 0.0, 1.0 / (opt["near"] * median * 63.0))
        end.record()
        self._sweep_events.append((begin, end))
        self._sweep_shares.append(swept["valid"].float().mean())
        return merge_sweep_depth(swept["depth"], swept["valid"], gt_img, threshold, fallback)

    def sweep_summary(self):
        """The `sweep` block of the run result (None with the option off): keyframes swept, their mean valid share, device ms per keyframe."""
        if self.mono_sweep is None:
            return None
        n = len(self._sweep_events)
        if n == 0:
            return {"keyframes": 0, "valid_share": 0.0, "device_ms_per_keyframe": 0.0}
        torch.cuda.synchronize(self.device)
        ms = sum(a.elapsed_time(b) for a, b in self._sweep_events)
        return {"keyframes": n, "valid_share": float(torch.stack(self._sweep_shares).mean()), "device_ms_per_keyframe": ms / n}

    # ---- Training.pose_prior: the start of a frame's tracking from dense frame-to-frame alignment (slam/odometry.py) -------------------
    def _prior_keep(self, viewpoint, render_pkg=None):
        """Keep `viewpoint` as the frame the next one is aligned against. Its depth: the sensor's (RGB-D) or the matcher's (stereo); for
        monocular input the depth of `render_pkg` where its opacity is above 0.5 (None: the map does not exist yet, nothing is kept)."""
        if self._odometry is None:
            from .odometry import DenseOdometry
            options = {k: v for k, v in self.pose_prior.items() if k not in ("enabled", "constant_velocity")}
            self._odometry = DenseOdometry(viewpoint.image_width, viewpoint.image_height, (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy),
                                           device=self.device, **options)
        if self.monocular:
            depth = None if render_pkg is None else render_pkg["depth"].detach() * (render_pkg["opacity"].detach() > 0.5)
        else:
            depth = viewpoint.depth_device()
        if depth is None:
            self._odometry.drop()
            return
        mask = viewpoint.motion_mask if self.dynamic_model else None
        self._odometry.keep(viewpoint.original_image, depth, mask)

    def _prior_start(self, viewpoint, previous):
        """Move `viewpoint` from the previous frame's pose W2C_prev to T W2C_prev, T the aligned motion (identity where the gate refused it:
        the reference's start). Device tensors throughout; the host reads nothing."""
        T_init = self._prior_motion if self.pose_prior["constant_velocity"] else None
        T, _ = self._odometry.align(viewpoint.original_image, T_init)
        self._prior_motion = T
        viewpoint.update_RT(*compose_pose(T, previous.R, previous.T))

    def odometry_summary(self):
        """The `odometry` block of the run result (None with the option off): frames aligned, the accepted share, the mean inlier share,
        device ms per frame."""
        if self.pose_prior is None:
            return None
        if self._odometry is None:
            return {"frames": 0, "accepted_share": 0.0, "inlier_share": 0.0, "device_ms_per_frame": 0.0}
        return self._odometry.summary()

    def initialize(self, frame_idx, viewpoint):
        """:189-207."""
        self.kf_indices, self.iteration_count, self.occ_aware_visibility, self.current_window = [], 0, {}, []
        self.initialized, self.reset = not self.monocular, False
        viewpoint.update_RT(viewpoint.R_gt, viewpoint.T_gt)               # first frame at the ground-truth pose
        if self.pose_prior is not None:                                   # a map that starts (over) drops the kept frame
            self._prior_motion = None
            self._prior_keep(viewpoint)
        if self.relocalisation is not None:                               # a map that starts (over) forgets the places of the old one
            if self._reloc_index is None:
                self._reloc_index = KeyframeIndex.from_options(self.relocalisation, self.device)
            self._reloc_index.clear()
            self._reloc_add(frame_idx, viewpoint)
        seed_depth = self.add_new_keyframe(frame_idx, init=True)
        self.sync_backend(self.backend.handle_init(frame_idx, viewpoint, seed_depth))

    # ---- tracking (:335-470) -------------------------------------------------------------------------------------------
    def _tracker_for_current_map(self, viewpoint):
        """The TrackingGraph of the current map version (its static slot, the detached Gaussians and -- if asked for -- the captured
        graph); rebuilt whenever the back-end replaced the model's tensors."""
        from .tracking_graph import TrackingGraph
        if self._tracker is None or self._tracker.version != TrackingGraph.model_version(self.gaussians):
            self._tracker = TrackingGraph(self.gaussians, self.pipeline_params, self.background, self.config, viewpoint)
            if self.use_tracking_graph:
                self._tracker.load(viewpoint)
                self._tracker.capture()
                self.graph_stats["captures"] += 1
        return self._tracker

    def tracking(self, frame_idx, viewpoint, last_keyframe_idx=None):
        previous = self.cameras[frame_idx - self.use_every_n_frames]
        viewpoint.update_RT(previous.R, previous.T)
        if self._odometry is not None and self._odometry.has_previous:
            self._prior_start(viewpoint, previous)
        pkg = self._optimise_pose(viewpoint)
        self.median_depth = get_median_depth(pkg["depth"], pkg["opacity"])        # :461
        render_pkg = render_without_grad(viewpoint, self.gaussians, self.pipeline_params, self.background)
        if self.pose_prior is not None:
            self._prior_keep(viewpoint, render_pkg)
        return render_pkg

    def _optimise_pose(self, viewpoint):
        """The pose (and exposure) of `viewpoint` optimised against the map from where it stands; returns the last iteration's render."""
        tracker = self._tracker_for_current_map(viewpoint)
        tracker.load(viewpoint)
        replayed = False
        if self.use_tracking_graph:
            _, replayed = tracker.run(self.tracking_itr_num, self.converge_check_every)
            self.graph_stats["replayed_frames" if replayed else "overflow_redos"] += 1
            if not replayed:
                tracker.load(viewpoint)          # the frame outgrew the captured graph's binning buffer: start over, eagerly
        if replayed:
            pkg = tracker.pkg                    # the captured iteration's static outputs: the last replay's render
        else:                                    # eager: the same iteration, launch by launch
            self.graph_stats["eager_frames"] += 1
            for it in range(self.tracking_itr_num):
                pkg = tracker.iteration()
                if (it + 1) % self.converge_check_every == 0 and tracker.cam.converged():
                    break
        tracker.store(viewpoint)
        return pkg

    # ---- Training.relocalisation: is the tracked frame lost, and if so where is it (slam/relocalise.py) -------------------------------
    def _reloc_mask(self, viewpoint):
        return viewpoint.motion_mask if self.dynamic_model else None

    def _reloc_add(self, frame_idx, viewpoint):
        """The new keyframe's real frame into the place index: one encode into the next row of the device database."""
        self._reloc_index.add(frame_idx, viewpoint.original_image, viewpoint.depth_device(), self._reloc_mask(viewpoint))

    def _reloc_track_from(self, viewpoint):
        pkg = self._optimise_pose(viewpoint)
        self.median_depth = get_median_depth(pkg["depth"], pkg["opacity"])
        return render_without_grad(viewpoint, self.gaussians, self.pipeline_params, self.background)

    def _found(self, frame_idx, viewpoint, render_pkg):
        """Judge the tracked frame by the rendering tracking() returned: one gsr_reloc_score launch and ONE host read, its eight counts.
        Accepted: (True, render_pkg), nothing else happens. Refused: the frame is lost and Relocaliser.localise looks for it among the
        keyframes; found there: ("relocalised", frame, keyframe, candidates tried) is logged and the rendering at the new pose returned.
        Not found: ("lost", frame) is logged, the frame gets the previous frame's pose and (False, None) tells run() to pass it over."""
        opt = self.relocalisation
        mask = self._reloc_mask(viewpoint)
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        counts = score(render_pkg, viewpoint, opt["tau_colour"], opt["tau_depth"], mask)
        end.record()
        self._reloc_events.append((begin, end))
        self._reloc_stats["scored"] += 1
        if verdict(counts.tolist(), opt)["accepted"]:
            return True, render_pkg
        if self._relocaliser is None:
            render_at = lambda camera: render_without_grad(camera, self.gaussians, self.pipeline_params, self.background)
            self._relocaliser = Relocaliser(self._reloc_index, self.cameras, render_at, self._reloc_track_from,
                                            (viewpoint.image_width, viewpoint.image_height), (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy),
                                            opt)
        previous = self.cameras[frame_idx - self.use_every_n_frames]
        viewpoint.update_RT(previous.R, previous.T)                        # what a refusal leaves the frame with
        found = self._relocaliser.localise(viewpoint, mask)
        if not found["accepted"]:
            self._reloc_stats["lost"] += 1
            self.log.append(("lost", frame_idx))
            if self._odometry is not None:
                self._odometry.drop()                                         # the next frame is not aligned against a frame without a pose
            return False, None
        self._reloc_stats["relocalised"] += 1
        self.log.append(("relocalised", frame_idx, found["keyframe"], found["candidates_tried"]))
        render_pkg = render_without_grad(viewpoint, self.gaussians, self.pipeline_params, self.background)
        if self.pose_prior is not None:
            self._prior_keep(viewpoint, render_pkg)
        return True, render_pkg

    def relocalisation_summary(self):
        """The `relocalisation` block of the run result (None with the option off): frames scored, lost, relocalised, device ms per score."""
        if self.relocalisation is None:
            return None
        n = len(self._reloc_events)
        ms = 0.0
        if n:
            torch.cuda.synchronize(self.device)
            ms = sum(a.elapsed_time(b) for a, b in self._reloc_events) / n
        return {**self._reloc_stats, "device_ms_per_score": ms}

    # ---- keyframe management (:472-562): the decisions of the reference, computed by slam/keyframes.py -------------------------
    def is_keyframe(self, cur_frame_idx, last_keyframe_idx, cur_frame_visibility_filter, occ_aware_visibility):
        stats = kf.frame_statistics(self.cameras[cur_frame_idx], self.cameras[last_keyframe_idx], cur_frame_visibility_filter,
                                    occ_aware_visibility[last_keyframe_idx])
        return bool(kf.keyframe_decision(stats, self.median_depth, self.thresholds))

    def add_to_window(self, cur_frame_idx, cur_frame_visibility_filter, occ_aware_visibility, window):
        thr = self.thresholds
        old = list(window)
        cutoff = thr.cutoff if self.initialized else 0.4                  # :523-529
        drop = kf.window_evictions(self.cameras[cur_frame_idx], [self.cameras[k] for k in old], cur_frame_visibility_filter,
                                   kf.visibility_matrix(occ_aware_visibility, old, cur_frame_visibility_filter), cutoff, thr.window_size)
        low, crowded = (int(v) for v in drop.tolist())                    # the one host transfer of the window update
        gone = [old[j] for j in (low, crowded) if j >= 0]
        removed = gone[-1] if gone else None
        return [cur_frame_idx] + [k for k in old if k not in gone], removed

    def sync_backend(self, data):
        """:582-590 (single process: the Gaussians are shared, not cloned)."""
        _, self.gaussians, self.occ_aware_visibility, poses = data[:4]
        for frame, R, T in poses:
            self.cameras[frame].update_RT(R.clone(), T.clone())

    def cleanup(self, frame_idx):
        self.cameras[frame_idx].clean()

    # ---- main loop (:603-833, single-thread schedule) ----------------------------------------------------------------------
    def _wants_keyframe(self, cur_frame_idx, newest_kf, frames_since_kf, visibility):
        """Keyframe decision of one tracked frame; returns (decision, overlap ratio for the log or None)."""
        stats = kf.frame_statistics(self.cameras[cur_frame_idx], self.cameras[newest_kf], visibility, self.occ_aware_visibility[newest_kf])
        by_motion = kf.keyframe_decision(stats, self.median_depth, self.thresholds)
        iou, by_motion = torch.stack([stats[0], by_motion.to(stats.dtype)]).tolist()                  # the one host transfer of the decision
        by_motion = by_motion > 0.5
        due = frames_since_kf >= self.kf_interval
        reported = None
        if len(self.current_window) < self.window_size:                   # while the window fills up only the overlap counts (:716-728)
            wanted, reported = due and iou < self.thresholds.overlap, iou
        else:
            wanted = by_motion
        if self.single_thread:
            wanted = due and wanted
        forced = cur_frame_idx - newest_kf >= self.MIN_KEYFRAME_GAP or cur_frame_idx == self.dystart
        new_object = self.dataset.dynamic_objects > self.dynamic_objects and cur_frame_idx > 0
        return bool(wanted or forced or new_object), reported

    def _insert_keyframe(self, cur_frame_idx, viewpoint, visibility, render_pkg, overlap):
        self.current_window, removed = self.add_to_window(cur_frame_idx, visibility, self.occ_aware_visibility, self.current_window)
        if self.monocular and not self.initialized and removed is not None:       # :771-776: the next frame starts the map over
            self.reset = True
            self.log.append(("reset", cur_frame_idx, "keyframes lack the overlap to initialise the map"))
            return
        depth_map = self.add_new_keyframe(cur_frame_idx, depth=render_pkg["depth"], opacity=render_pkg["opacity"], init=False)
        if self.reset:                                                            # no valid depth to seed from (_monocular_seed_depth)
            return
        if self.relocalisation is not None:
            self._reloc_add(cur_frame_idx, viewpoint)
        self.sync_backend(self.backend.handle_keyframe(cur_frame_idx, viewpoint, self.current_window, depth_map, True, False))
        self.log.append(("keyframe", cur_frame_idx, overlap))
        viewpoint.clean_key()
        if self.save_results and self.save_trj and len(self.kf_indices) % self.save_trj_kf_intv == 0:
            eval_ate(self.cameras, self.kf_indices, self.save_dir, cur_frame_idx, monocular=self.monocular)

    def run(self, max_frames=None):
        n_frames = len(self.dataset) if max_frames is None else min(max_frames, len(self.dataset))
        previous_kf = 0                                   # the window's newest keyframe as of the previous frame
        for cur_frame_idx in range(n_frames):
            viewpoint = Camera.init_from_dataset(self.dataset, cur_frame_idx, self.dataset.projection_matrix)
            viewpoint.compute_grad_mask(self.config)
            self.cameras[cur_frame_idx] = viewpoint
            if self.reset:                                # first frame (monocular input: or a failed initialisation): build the map from it
                self.resets += 1 if cur_frame_idx > 0 else 0
                self.initialize(cur_frame_idx, viewpoint)
                self.current_window += [cur_frame_idx]
                previous_kf = cur_frame_idx
                torch.cuda.synchronize(self.device)
                self.init_done_at = time.perf_counter()   # map initialisation (hundreds of iterations on one frame) is reported apart
                continue
            self.initialized = self.initialized or len(self.current_window) == self.window_size
            render_pkg = self.tracking(cur_frame_idx, viewpoint, previous_kf)
            if self.relocalisation is not None and self.initialized:
                found, render_pkg = self._found(cur_frame_idx, viewpoint, render_pkg)
                if not found:                             # lost: it keeps the previous frame's pose and is no keyframe
                    self.cleanup(cur_frame_idx)
                    self.dynamic_objects = self.dataset.dynamic_objects
                    continue
            frames_since_kf = cur_frame_idx - previous_kf
            previous_kf = newest_kf = self.current_window[0]
            visibility = (render_pkg["n_touched"] > 0).long()
            wanted, overlap = self._wants_keyframe(cur_frame_idx, newest_kf, frames_since_kf, visibility)
            if wanted:
                self._insert_keyframe(cur_frame_idx, viewpoint, visibility, render_pkg, overlap)
            if not wanted or self.reset:                  # (a frame whose insertion ended in a reset is no keyframe: it keeps its pose only)
                self.cleanup(cur_frame_idx)
            self.dynamic_objects = self.dataset.dynamic_objects
        if self.save_results and self.save_dir:
            eval_ate(self.cameras, self.kf_indices, self.save_dir, 0, final=True, monocular=self.monocular)
            save_gaussians(self.gaussians, self.save_dir, "final", final=True)
