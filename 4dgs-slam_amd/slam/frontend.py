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

What the reference does not have is one object of ``slam/stages.py`` per option, None when its ``Training`` block is absent or off:
``mono_sweep`` (a monocular keyframe's seed depth), ``pose_prior`` (where tracking starts), ``relocalisation`` (the judge step) and
``loop_closure`` (a new keyframe is tied to old keyframes that saw the same place; poses and map are corrected before the back-end maps
it). This file calls them by name and keeps what couples them: the log, and the prior's kept frame when a frame is lost or relocalised or
a loop is closed.
"""
import struct
import time
import weakref

import torch

from gaussian_renderer import render

from . import keyframes as kf
from .camera import Camera
from .eval_utils import eval_ate, save_gaussians
from .relocalise import relocalisation_options
from .stages import (LoopClosure, PosePrior, Relocalisation, SweepSeeding, feature_seed_options, loop_closure_options, mono_sweep_options, pose_prior_options,
                     pose_prior_terms_options)


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
        # the optional stages (slam/stages.py), each None when its block is absent or off: a monocular keyframe is then seeded the reference's
        # way alone, a frame's tracking starts at the previous frame's pose and no frame is ever judged lost, as in the reference
        sweep, prior, reloc = mono_sweep_options(training), pose_prior_options(training), relocalisation_options(training)
        self.mono_sweep = sweep and SweepSeeding(sweep)
        terms = pose_prior_terms_options(training)                         # refused without pose_prior
        self.pose_prior = prior and PosePrior(prior, self.monocular, self.dynamic_model, terms)
        seed = feature_seed_options(training)                               # refused without a stage to seed, and for monocular runs unless its solver is pnp
        self.relocalisation = reloc and Relocalisation(reloc, self.dynamic_model, seed)
        loops = loop_closure_options(training, self.dynamic_model)          # refused for monocular, dynamic and spherical-harmonics runs
        self.loop_closure = loops and LoopClosure(loops, seed)

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
            seed_depth = self.mono_sweep.seed_depth(gt_img, seed_depth, median, threshold, [self.cameras[k] for k in self.current_window])
        return seed_depth

    def initialize(self, frame_idx, viewpoint):
        """:189-207."""
        self.kf_indices, self.iteration_count, self.occ_aware_visibility, self.current_window = [], 0, {}, []
        self.initialized, self.reset = not self.monocular, False
        if getattr(self.dataset, "has_ground_truth", True):
            viewpoint.update_RT(viewpoint.R_gt, viewpoint.T_gt)           # first frame at the ground-truth pose
        else:                                                             # no ground truth (a plain video): the map's frame is the first camera's
            viewpoint.update_RT(torch.eye(3, device=viewpoint.R.device), torch.zeros(3, device=viewpoint.R.device))
        if self.pose_prior is not None:                                   # a map that starts (over) drops the kept frame
            self.pose_prior.restart(viewpoint)
        if self.relocalisation is not None:                               # a map that starts (over) forgets the places of the old one
            # (the stage keeps the two calls for the run: through a weak reference, or this object -- streams, events and captured graphs --
            # would be freed by the cycle collector alone, whenever it next runs, be that in the middle of a later run's graph capture)
            me = weakref.proxy(self)
            self.relocalisation.restart(frame_idx, viewpoint, self.cameras, lambda c: me._render_at(c), lambda v: me._track_and_render(v))
        if self.loop_closure is not None:                                 # a map that starts (over) starts its pose graph over; node 0 is this frame
            me = weakref.proxy(self)
            self.loop_closure.restart(frame_idx, viewpoint, self.cameras, lambda: me.gaussians,
                                      self.relocalisation.index if self.relocalisation is not None else None, self.backend.shard.world)
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
        if self.pose_prior is not None:
            self.pose_prior.start(viewpoint, previous)
        render_pkg = self._track_and_render(viewpoint)
        if self.pose_prior is not None:
            self.pose_prior.keep(viewpoint, render_pkg)
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
            pkg = tracker.run_eager(self.tracking_itr_num, self.converge_check_every)
        tracker.store(viewpoint)
        return pkg

    @torch.no_grad()
    def _render_at(self, camera):
        return render(camera, self.gaussians, self.pipeline_params, self.background, dynamic=False)

    def _track_and_render(self, viewpoint):
        """Track `viewpoint` from where it stands (the median depth is the last tracking iteration's, :461) and render the map there."""
        pkg = self._optimise_pose(viewpoint)
        self.median_depth = get_median_depth(pkg["depth"], pkg["opacity"])
        return self._render_at(viewpoint)

    def _found(self, frame_idx, viewpoint, render_pkg):
        """Judge the tracked frame by the rendering tracking() returned (Relocaliser.judge: ONE host read, the eight counts). Accepted:
        (True, render_pkg). Found again among the keyframes: ("relocalised", frame, keyframe, candidates tried) is logged and the rendering
        at the new pose returned. Not found: ("lost", frame) is logged, the frame has the previous one's pose and run() passes it over."""
        previous = self.cameras[frame_idx - self.use_every_n_frames]
        found = self.relocalisation.judge(viewpoint, render_pkg, (previous.R, previous.T))
        if not found["accepted"]:
            self.log.append(("lost", frame_idx))
            if self.pose_prior is not None:
                self.pose_prior.drop()                                        # the next frame is not aligned against a frame without a pose
            return False, None
        if found["keyframe"] is not None:
            self.log.append(("relocalised", frame_idx, found["keyframe"], found["candidates_tried"]))
            render_pkg = self._render_at(viewpoint)
            if self.pose_prior is not None:
                self.pose_prior.keep(viewpoint, render_pkg)
        return True, render_pkg

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
            self.relocalisation.add(cur_frame_idx, viewpoint)
        if self.loop_closure is not None:                                         # the keyframe is a node before the back-end seeds from its pose
            closed = self.loop_closure.on_keyframe(cur_frame_idx, viewpoint)
            if closed is not None and closed["applied"]:
                self.log.append(("loop_closed", cur_frame_idx, closed["keyframes"], closed["translation"], closed["rotation"]))
                if self.pose_prior is not None:
                    self.pose_prior.drop()                                        # as after a relocalised frame: poses moved under the kept frame
        if self.pose_prior is not None:                                           # (aligning against keyframes: this one from now on)
            self.pose_prior.keyframe(viewpoint, render_pkg)
        self.sync_backend(self.backend.handle_keyframe(cur_frame_idx, viewpoint, self.current_window, depth_map, True, False))
        self.log.append(("keyframe", cur_frame_idx, overlap))
        viewpoint.clean_key()
        if self.save_results and self.save_trj and len(self.kf_indices) % self.save_trj_kf_intv == 0 and getattr(self.dataset, "has_ground_truth", True):
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
        if self.save_results and self.save_dir and getattr(self.dataset, "has_ground_truth", True):      # (no ATE without ground truth)
            eval_ate(self.cameras, self.kf_indices, self.save_dir, 0, final=True, monocular=self.monocular)
            save_gaussians(self.gaussians, self.save_dir, "final", final=True)
