"""A run of STATIC mapping iterations as hipGraph replays (utils/slam_backend.py:1013-1224 is the loop being replaced):

    [schedule row -> keyframe slots] -> multi-view render (window keyframes + 2 random ones) -> fused mapping loss per view ->
    isotropic regulariser -> ONE backward -> densification statistics -> Adam on the six Gaussian groups -> gradient reset -> camera steps

Eager, that is ~55 launches driven by Python and autograd: 1.0-1.6 ms of wall time for 0.5 ms of device time at SLAM sizes. Captured, the host
issues one ``graph.replay()`` per iteration. What makes the iteration capturable (beyond what slam/tracking_graph.py already needed -- the
rasterizer's lazy mode, cameras in persistent device buffers, a camera step with its Adam counter on the device):

  * the two RANDOM keyframes of an iteration (:1031-1037) are rendered through two persistent *slots*: a slot is a camera object plus
    ground-truth / loss-weight images of its own, filled inside the graph by ``gsr_slot_gather`` from a device table of the candidate
    keyframes' buffer addresses and an index read from device memory -- which keyframes an iteration draws is an index write, not a capture;
  * everything that depends on the iteration NUMBER -- those indices, Adam's bias corrections, the position learning rate (GM:492-505) -- is a
    row of a device-side schedule written once per run; ``gsr_schedule_advance`` copies row ``counter`` into the "current" block the other
    kernels read and bumps the counter (include/slam_map.h), ``gsr_adam_step_scheduled`` reads its coefficients there (include/slam_losses.h);
  * the iterations that densify or reset opacities (every ``gaussian_update_every`` / ``gaussian_reset`` iterations: slam/schedule.py's
    mapping_rule, which also measures the runs) replace the model's tensors: they run eagerly (BackEnd._map_static_iteration) and end a
    run; the next run captures again.

The host draws the random keyframes for the whole run up front -- the same ``torch.randperm`` calls in the same order as the eager loop -- and
``iteration()`` is ONE code path: executed directly for the warm-up iterations of a run, captured once, then replayed. Results are
bit-identical to the eager loop (tests/test_hip_slam.py). Warm-up, capture, replays and undo are slam/graph_run.py's: a replayed forward pass
that outgrows its (generously sized) binning buffer is detected after the run through the sticky overflow counters, the run is then undone
from a snapshot (``state_tensors()``) and repeated eagerly; so is the rest of a run whose capture fails."""
import torch

import slam_losses

from . import keyframe_slots
from .schedule import Schedule, adam_rows, camera_gradients, densification_statistics, gaussian_state, window_state, xyz_lr_rule

N_INDEX_WORDS = 2            # random keyframes per iteration (utils/slam_backend.py:1031-1037)
# head room of the binning buffers a captured iteration lays out (gsr_set_option, see include/gs_rasterizer.h): the longest tile list may
# grow 4x during the replays
CAPTURE_OPTIONS = {"cap_margin_permille": 500, "cap_tile_margin_permille": 3000}
# initialize_map's runs: the instance count of the ONE view being fitted grew 1.82x inside a 99-iteration run right after the opacity reset
# (104 438 -> 190 427 instances at iteration 501 of the config #4 stand-in; 1.5x was the margin, 97 iterations were redone): 3x here
INIT_CAPTURE_OPTIONS = dict(CAPTURE_OPTIONS, cap_margin_permille=2000)


class MappingGraph:
    """One run of plain static mapping iterations of ``backend`` over ``current_window`` (see the module docstring)."""

    def __init__(self, backend, current_window, viewpoint_stack, candidates, draws, iteration_count0):
        be = self.backend = backend
        g = be.gaussians
        self.current_window, self.window, self.candidates = list(current_window), list(viewpoint_stack), list(candidates)
        self.draws = [list(d)[:N_INDEX_WORDS] for d in draws]
        self.rows = len(self.draws)
        dev = self.device = self.window[0].device
        self.n_slots = min(N_INDEX_WORDS, len(self.candidates))
        proto = self.window[0]
        H, W = int(proto.image_height), int(proto.image_width)
        self.pixels = H * W
        cfg = be.config
        # ---- slots: a camera + ground truth / weights each ------------------------------------------------------------------------------
        self.slots = [keyframe_slots.blank_camera(proto, -1 - s, dev) for s in range(self.n_slots)]
        self.slot_ops = [keyframe_slots.slot_buffers(H, W, dev) for _ in range(self.n_slots)]
        store = be.keyframe_operands
        self.window_ops = [store.get(cfg, v, dev, rm_dynamic=True, dynamic=False) for v in self.window]
        self.alpha = self.window_ops[0][4]
        # ---- the candidates' buffer addresses, one gsr_keyframe_entry per candidate, in device memory ----------------------------------------
        self._keep = [store.get(cfg, v, dev, rm_dynamic=True, dynamic=False) for v in self.candidates]
        self.kf_table = keyframe_slots.upload_rows(keyframe_slots.address_rows(self.candidates, [ops[:4] for ops in self._keep]), torch.int64, dev)
        self.slot_dst = keyframe_slots.entries(list(zip(self.slots, self.slot_ops)))
        # ---- the schedule: per iteration [index 0, index 1 | (step size, 1 / sqrt(bias correction 2)) per parameter tensor] -------------------
        self.todo = g.optimizer.scheduled_segments()
        if self.todo is None:
            raise RuntimeError("MappingGraph: the optimizer state does not fit the fused scheduled step (run one eager iteration first)")
        self.schedule = Schedule(self.rows, dev, index_words=self.draws, adam=adam_rows(g.optimizer, self.todo, self.rows, xyz_lr_rule(g, iteration_count0)))
        self.slot_index = self.schedule.indices(self.n_slots)
        self.pkgs = None

    # ---- the iteration (one code path: run directly, or captured and replayed) ---------------------------------------------------------------
    def iteration(self):
        be, g, dev = self.backend, self.backend.gaussians, self.device
        self.pkgs = None            # (the previous iteration's autograd graph dies here, not while the next one is being built)
        self.schedule.advance()
        keyframe_slots.gather(self.n_slots, self.kf_table, self.slot_index, self.slot_dst, self.pixels, dev)
        views = self.window + self.slots
        ops = list(self.window_ops) + [o + (self.alpha,) for o in self.slot_ops]
        rendered = be._render_many(views, [(None, None, None)] * len(views))
        # (every term a root of ONE backward pass with the gradient 1 instead of a sum nobody reads: see DynamicMapping.iteration)
        terms = [slam_losses.weighted_l1_loss(pkg["render"], pkg["depth"], gt_image, gt_depth, w_rgb, w_dep, viewpoint.exposure_a, viewpoint.exposure_b,
                                              alpha, compute_value=False)
                 for viewpoint, pkg, (gt_image, gt_depth, w_rgb, w_dep, alpha) in zip(views, rendered, ops)]
        terms.append(be._isotropic_loss())
        torch.autograd.backward(terms, [be.unit_gradient(dev)] * len(terms))
        with torch.no_grad():
            for pkg in rendered:
                be._view_stats(pkg)
            g.optimizer.step_scheduled(self.todo, self.schedule.coefficients_ptr())
            g.optimizer.zero_grad(set_to_none=True)
            be._pose_updates(self.window, self.current_window)
            be._clear_camera_grads(self.slots)
        self.pkgs = rendered
        return rendered

    # ---- for slam/graph_run.py -------------------------------------------------------------------------------------------------------
    def state_tensors(self):
        g = self.backend.gaussians
        return gaussian_state(g.optimizer, [p for _, p in self.todo], self.todo) + densification_statistics(g) + [self.schedule.counter] + window_state(self.window)

    def discard(self):
        for v in self.window:
            v.refresh_matrices()
        self.backend.gaussians.optimizer.zero_grad(set_to_none=True)
        self.backend._clear_camera_grads(self.window + self.slots)


class InitGraph:
    """A run of plain iterations of BackEnd.initialize_map (utils/slam_backend.py:237-296: one view, the mapping loss without exposure, Adam
    on the Gaussians; no camera step, no regulariser, a constant learning rate) as hipGraph replays: the single-view counterpart of
    MappingGraph. The schedule rows only carry Adam's coefficients. ``iteration()`` is one code path -- executed directly for the warm-up,
    captured once, replayed; iterations that densify or reset opacities stay in initialize_map's eager loop and end a run."""

    def __init__(self, backend, viewpoint, rm_dynamic, rows):
        be = self.backend = backend
        g = be.gaussians
        self.viewpoint, self.rows = viewpoint, int(rows)
        dev = self.device = viewpoint.device
        self.ops = be.keyframe_operands.get(be.config, viewpoint, dev, rm_dynamic=rm_dynamic, dynamic=False)
        self.todo = g.optimizer.scheduled_segments()
        if self.todo is None:
            raise RuntimeError("InitGraph: the optimizer state does not fit the fused scheduled step (run one eager iteration first)")
        self.schedule = Schedule(self.rows, dev, adam=adam_rows(g.optimizer, self.todo, self.rows))
        self.pkg = None

    def iteration(self):
        be, g, v = self.backend, self.backend.gaussians, self.viewpoint
        self.pkg = None
        self.schedule.advance()
        pkg = be._render(v, (None, None, None))
        gt_image, gt_depth, w_rgb, w_dep, alpha = self.ops
        loss = slam_losses.weighted_l1_loss(pkg["render"], pkg["depth"], gt_image, gt_depth, w_rgb, w_dep, None, None, alpha, compute_value=False)
        loss.backward()
        with torch.no_grad():
            be._view_stats(pkg)
            g.optimizer.step_scheduled(self.todo, self.schedule.coefficients_ptr())
            g.optimizer.zero_grad(set_to_none=True)
        # (the view's camera parameters keep accumulating their gradients, as in the eager loop and in the reference, whose initialize_map
        # never clears them: in place, into the tensors the warm-up iterations left -- which is why the snapshot covers them)
        self.pkg = pkg
        return pkg

    def state_tensors(self):
        g = self.backend.gaussians
        return gaussian_state(g.optimizer, [p for _, p in self.todo], self.todo) + densification_statistics(g) + [self.schedule.counter] + camera_gradients(self.viewpoint)

    def discard(self):
        """(the view's camera gradients are part of the snapshot: they accumulate across the loop on purpose, see iteration())"""
        self.backend.gaussians.optimizer.zero_grad(set_to_none=True)
