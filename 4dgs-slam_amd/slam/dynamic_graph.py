"""The DYNAMIC mapping call (utils/slam_backend.py:306-774, BackEnd.map with the control-node network) in a fixed layout, its runs of plain
iterations as hipGraph replays (second half; slam/mapping_graph.py is the static counterpart).

A dynamic iteration is: node network on ~100 time samples -> node blend at the views' times -> two regularisers on the random samples ->
multi-view render (window views + 2 random keyframes) -> fused mapping losses -> 2 flow renders per view + flow losses -> ONE backward ->
statistics -> camera steps -> Adam on the network (and, in the second half of the call, on the Gaussians). Eager: ~370 launches from Python
and autograd, 6.4 ms of wall time for 5.0 ms of device time (profiles/r04_mapping_iteration_launches_dynamic.json).

What the host decides per iteration in the reference -- and what therefore had to move into device memory before an iteration could be
recorded once and replayed:

  * which two RANDOM keyframes are rendered (:344-349): two persistent *slots* (camera + ground truth + loss weights, filled by
    gsr_slot_gather from a device table of the candidates' buffer addresses, slam/keyframe_slots.py) -- plus, here, the slot's TIME, its
    flow PARTNER (the closest earlier keyframe, :299-304,:479-509: a second slot camera) and the pair's flow targets (six image planes,
    moved by a second gather through the same entry point), and the partner's time;
  * the random TIME SAMPLES of the two regularisers (:517-519,:646-648; 12 per window view, 10 per random keyframe): drawn on the host
    for a whole run up front -- the same torch.rand calls in the same order as iteration by iteration -- and stored as a row of the
    device-side schedule next to the slot indices and Adam's coefficients (gsr_schedule_advance copies row `counter` into the block the
    iteration reads);
  * the ORDER of the network's batch: the eager loop (BackEnd.map's body, kept for sharded runs and test doubles) names time samples by
    their host value, sorts and merges them; here the layout is fixed -- [the window views' and their partners' times, merged and sorted
    once per call | slot 0's time, its partner's | slot 1's ... | the samples, view by view in drawing order] -- and consumers address
    rows by position (ControlNodes.begin_iteration_indexed / regularisers_indexed). Same terms, summed in another order.

``iteration()`` is ONE code path: executed directly -- every iteration when ``Training.mapping_graph`` is off, the warm-up iterations of a
run, the iterations that densify or reset opacities (those replace the model's tensors: they end a run; WHICH they are is
slam/schedule.mapping_rule's, how long the run before them its plain_run, WHAT they do BackEnd._maintain) -- or captured once and replayed.
Direct and replayed iterations are bit-identical (tests/test_hip_slam.py). The call's two halves (:350-355: the loss weights double on the
moving pixels in the first half; :337-338,:765-770: the Gaussians only step in the second) are different graphs: a run never crosses the
boundary. Warm-up, capture, replays and undo are slam/graph_run.py's: a replayed forward pass that outgrows its binning buffer is detected
after the run (sticky overflow counters), the run is then undone from a snapshot (``state_tensors()``) and repeated directly; so is the rest
of a run whose capture fails."""
import os

import torch

import control_nodes
import slam_losses

from . import graph_run, keyframe_slots
from .camera import Camera
from .deform_model import draw_loss_times, time_key
from .mapping_graph import N_INDEX_WORDS
from .schedule import (Schedule, adam_rows, camera_gradients, catch_up, densification_statistics, gaussian_state, init_rule, mapping_rule, network_state,
                       plain_run, window_state, xyz_lr_rule)

# Head room of the binning buffers a captured iteration lays out (include/gs_rasterizer.h): while the node network trains alone (first half
# of a call) the moving object's Gaussians can swell and pile up for a few iterations -- measured: instance counts +10 %, the longest tile
# list x 2-4 -- and every overflow costs the whole run (undone, repeated directly).
CAPTURE_MARGIN_PERMILLE, CAPTURE_TILE_MARGIN_PERMILLE = (int(v) for v in os.environ.get("GSR_DYN_MARGINS", "2000,7000").split(","))
# the slots of an iteration's two random keyframes (and their flow renders) show another keyframe on every replay: the instance count at
# capture says little about the next draw (flow slot: 7 042 at capture, > 25 000 later = the 3x margin overrun, 99 iterations redone in the
# config #4 stand-in, 39 of 400 in the census) -- a floor in instances (~70 B each: 9 MB per view) instead of a ratio alone
CAPTURE_FLOOR_INSTANCES = int(os.environ.get("GSR_DYN_CAP_FLOOR", "131072"))
CAPTURE_OPTIONS = {"cap_margin_permille": CAPTURE_MARGIN_PERMILLE, "cap_tile_margin_permille": CAPTURE_TILE_MARGIN_PERMILLE,
                   "cap_floor": CAPTURE_FLOOR_INSTANCES}
FLOW_CLIPS = os.environ.get("GSR_FLOW_CLIPS", "1") != "0"      # render the flow images only where the flow loss reads them (gsr_view.flow_clip)
WINDOW_SAMPLES, EXTRA_SAMPLES = (4, 8), (2, 8)        # (ARAP, elastic) time samples per window view / per random keyframe (:517-519,:646-648)


_region = torch.autograd.profiler.record_function          # names a part of the iteration for the profiler (tools/mapping_iteration_launches.py)


def _planes(f6):          # a [6, H, W] flow-target tensor as the four planes gsr_slot_gather moves (gt_image[3], gt_depth, w_rgb, w_depth)
    return f6[0:3], f6[3:4], f6[4:5], f6[5:6]


def eligible(be, views, candidates):
    """Can this map() call run in the fixed layout? (Else BackEnd.map's eager body takes it: sharded runs, test doubles, monocular input,
    fewer than three nodes, keyframes without a motion mask.)"""
    g, t = be.gaussians, be.config["Training"]
    if not t.get("dynamic_fixed_layout", True) or be.shard.active or be.loss_values or t.get("monocular", False):
        return False
    if not str(be.device).startswith("cuda") or g.deform is None or not g.deform_init or g.get_xyz.shape[0] == 0:
        return False
    if g.deform.deform.node_num < 3 or g.dyn_rows().shape[0] == 0 or not getattr(g.optimizer, "_fused_acc", False):
        return False
    return all(isinstance(v, Camera) and v.depth is not None and v.motion_mask is not None for v in list(views) + list(candidates))


def phase(i, iters, warm):
    """Of iteration i of a map(iters) call: (the loss weights double on the moving pixels, :350-355; the Gaussians take part, :337-338,:765-770)"""
    return (i < iters / 2, i > warm)


def plain_rows(be, i, iters, warm):
    """How many iterations from i on make one run: of i's phase and, while the Gaussians step -- iteration_count advances then only, i's
    own count is iteration_count + 1 --, none that densifies or resets opacities. 0: iteration i is such a one."""
    ph = phase(i, iters, warm)
    count = be.iteration_count + (1 if ph[1] else 0)
    return plain_run(i, iters, lambda k: phase(k, iters, warm) != ph or (ph[1] and mapping_rule(be, count + (k - i)) is not None))


class _Run:
    """`rows` consecutive iterations of one phase: their schedule in device memory."""
    __slots__ = ("i0", "rows", "dyn", "stepping", "with_flow", "flow_weight", "layout", "tables", "todo", "schedule", "count0", "draws")


class DynamicMapping:
    """One BackEnd.map(current_window, iters, dynamic_network=True) call (see the module docstring)."""

    def __init__(self, backend, current_window, views, positions, candidates, iters, warm):
        be = self.be = backend
        self.g = be.gaussians
        self.nodes = self.g.deform.deform
        self.current_window, self.views, self.positions, self.candidates = list(current_window), list(views), list(positions), list(candidates)
        self.iters, self.warm = int(iters), int(warm)
        dev = self.device = self.views[0].device
        proto = self.views[0]
        self.H, self.W = int(proto.image_height), int(proto.image_width)
        self.pixels = self.H * self.W
        t = be.config["Training"]
        self.flow_weights = {True: float(t["flow_loss"]), False: float(t.get("flow_loss_fine", t["flow_loss"]))}
        self.has_flow_data = hasattr(be.dataset, "gt_flow")
        self.n_slots = min(N_INDEX_WORDS, len(self.candidates))
        any_flow = self.has_flow_data and max(self.flow_weights.values()) > 0
        self.slots = [keyframe_slots.blank_camera(proto, -1 - s, dev) for s in range(self.n_slots)]
        self.slot_ops = [keyframe_slots.slot_buffers(self.H, self.W, dev) for _ in range(self.n_slots)]
        self.partner_slots = [keyframe_slots.blank_camera(proto, -101 - s, dev) for s in range(self.n_slots)] if any_flow else []
        self.partner_flow = [torch.zeros((6, self.H, self.W), device=dev) for _ in range(self.n_slots)] if any_flow else []
        self.slot_dst = keyframe_slots.entries(list(zip(self.slots, self.slot_ops)))
        self.partner_dst = keyframe_slots.entries([(c, _planes(f)) for c, f in zip(self.partner_slots, self.partner_flow)])
        self._zero6 = None
        self.slot_clips = torch.zeros((max(1, self.n_slots), 8), dtype=torch.int32, device=dev)       # per slot: its rectangle, its partner's
        self._layouts, self._tables, self._window_ops = {}, {}, {}
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.run, self.pkgs = None, None
        self.stats = graph_run.stats(be, "dynamic_graph")
        self.stats.setdefault("special", 0)

    # ---- per-call constants --------------------------------------------------------------------------------------------------------------
    def phase(self, i):
        return phase(i, self.iters, self.warm)

    def with_flow(self, dyn):
        return self.has_flow_data and self.flow_weights[dyn] > 0

    def partner_of(self, v):
        """The keyframe the flow terms of `v` are formed with (:299-304,:479-509), or None."""
        closest = self.be.find_closest_keyframe(v.uid)
        if closest is None:
            return None
        other = self.be.viewpoints[closest]
        return other if (v.motion_mask is not None and other.motion_mask is not None) else None

    def layout(self, with_flow):
        hit = self._layouts.get(with_flow)
        if hit is None:
            store, ds = self.be.flow_targets, self.be.dataset          # (keyframe_slots.FlowTargets: the eager body reads the same tensors)
            partners = [self.partner_of(v) if with_flow else None for v in self.views]
            keys = sorted({time_key(v.time) for v in self.views} | {time_key(p.time) for p in partners if p is not None})
            index = {k: i for i, k in enumerate(keys)}
            epf = 2 if with_flow else 1                        # batch entries per slot: its time (and its partner's)
            n_w = len(keys)
            hit = self._layouts[with_flow] = {
                "partners": partners, "n_w": n_w, "epf": epf, "n_full": n_w + self.n_slots * epf,
                "view_idx": [index[time_key(v.time)] for v in self.views] + [n_w + e * epf for e in range(self.n_slots)],
                "partner_idx": [None if p is None else index[time_key(p.time)] for p in partners],
                "flow6": [None if p is None else store.get(ds, v, p) for v, p in zip(self.views, partners)],
                "clips": [None if p is None else (store.clip(v), store.clip(p)) for v, p in zip(self.views, partners)],
                "wtimes": torch.tensor(keys, dtype=torch.float32).to(self.device)}
        return hit

    def tables(self, dyn, with_flow):
        """Per candidate keyframe, in device memory: the addresses gsr_slot_gather copies from (camera + loss operands; partner camera + flow
        targets) and the (own, partner) times."""
        hit = self._tables.get((dyn, with_flow))
        if hit is None:
            be, dev = self.be, self.device
            store, cfg = be.keyframe_operands, be.config
            ops, partners, flows, times, clip_rows = [], [], [], [], []
            for c in self.candidates:
                ops.append(store.get(cfg, c, dev, rm_dynamic=False, dynamic=dyn))
                if with_flow:
                    p = self.partner_of(c)
                    if p is None:               # no earlier keyframe: the candidate stands in for its partner with an all-zero target and mask --
                        p = c                   # both flow terms and their gradients are exactly zero
                        if self._zero6 is None:
                            self._zero6 = torch.zeros((6, self.H, self.W), device=dev)
                        f6 = self._zero6
                    else:
                        f6 = be.flow_targets.get(be.dataset, c, p)
                    partners.append(p)
                    flows.append(f6)
                    times.append([time_key(c.time), time_key(p.time)])
                    # (rows 2 c and 2 c + 1: the rectangles the two flow images of the pair are read in; the stand-in pair reads nothing)
                    clip_rows += [be.flow_targets.clip(c), be.flow_targets.clip(p)] if p is not c else [torch.zeros(4, dtype=torch.int32, device=dev)] * 2
                else:
                    times.append([time_key(c.time)])
            up = keyframe_slots.upload_rows
            hit = self._tables[(dyn, with_flow)] = {
                "keep": ops + flows, "kf": up(keyframe_slots.address_rows(self.candidates, [o[:4] for o in ops]), torch.int64, dev),
                "partner": up(keyframe_slots.address_rows(partners, [_planes(f) for f in flows]), torch.int64, dev), "times": up(times, torch.float32, dev),
                "clips": torch.stack(clip_rows).reshape(len(self.candidates), 8) if clip_rows else None}
        return hit

    # ---- a run's schedule -------------------------------------------------------------------------------------------------------------------
    def make_run(self, i0, rows, phase):
        """Draw what the iterations i0 .. i0 + rows - 1 draw, in their order (:344-349 torch.randperm for the random keyframes, then per view
        the regularisers' torch.rand calls, deform_model.draw_loss_times), and lay it out as the run's device-side schedule."""
        be, g = self.be, self.g
        r = _Run()
        r.i0, r.rows, (r.dyn, r.stepping) = i0, rows, phase
        r.with_flow = self.with_flow(r.dyn)
        r.flow_weight = self.flow_weights[r.dyn]
        r.layout, r.tables = self.layout(r.with_flow), self.tables(r.dyn, r.with_flow)
        t = be.config["Training"]
        ti = g.time_interval
        arap_delta = float(t.get("delta", 5)) * ti                                    # :325,:518
        nv = len(self.views)
        r.draws = []
        for _ in range(rows):
            extra_idx = [int(c) for c in torch.randperm(len(self.candidates))[:2]]
            samples = []
            for k, v in enumerate(self.views + [self.candidates[c] for c in extra_idx]):
                window = k < nv
                plan = draw_loss_times(v.time, arap_delta if window else 5 * ti, WINDOW_SAMPLES[0] if window else EXTRA_SAMPLES[0], 5 * ti)
                samples += [time_key(x) for x in plan["arap"] + plan["elastic"]]
            r.draws.append((extra_idx, samples))
        r.todo = g.optimizer.scheduled_segments() if r.stepping else None
        r.count0 = be.iteration_count
        r.schedule = Schedule(rows, self.device, index_words=[d[0] for d in r.draws], samples=[d[1] for d in r.draws], counter=self.counter,
                              adam=adam_rows(g.optimizer, r.todo, rows, xyz_lr_rule(g, r.count0)) if r.todo else None)
        self.counter.zero_()
        self.run = r
        return r

    # ---- the iteration (one code path: run directly, or captured and replayed) ---------------------------------------------------------------
    def iteration(self, special=None):
        """`special` (direct execution only): {"last": bool} for an iteration that may densify / reset opacities -- it decides that on the
        host like the eager loop and takes a plain optimizer step (the model's tensors may have been replaced)."""
        be, g, nodes, r, dev = self.be, self.g, self.nodes, self.run, self.device
        lay, tab = r.layout, r.tables
        self.pkgs = None            # (the previous iteration's autograd graph dies here, not while the next one is being built)
        r.schedule.advance()
        slot_index = r.schedule.indices(self.n_slots)
        keyframe_slots.gather(self.n_slots, tab["kf"], slot_index, self.slot_dst, self.pixels, dev)
        if r.with_flow:
            keyframe_slots.gather(self.n_slots, tab["partner"], slot_index, self.partner_dst, self.pixels, dev)
        # ---- the iteration's time samples, in the fixed layout ------------------------------------------------------------------------------
        # (the _region ranges only name the iteration's parts for tools/mapping_iteration_launches.py; no effect on the work)
        with _region("gsr.network"):
            parts = [lay["wtimes"]]
            if self.n_slots:
                parts.append(tab["times"].index_select(0, slot_index.long()).reshape(-1))
            parts.append(r.schedule.samples())
            it = nodes.begin_iteration_indexed(torch.cat(parts), lay["n_full"], blend=(g.get_dygs_xyz.detach(), g.motion_mask))
        nv, ne = len(self.views), self.n_slots
        with _region("gsr.regularisers"):
            loss_network = nodes.regularisers_indexed(it, nv, ne, be._regulariser_weights(nv, ne), WINDOW_SAMPLES, EXTRA_SAMPLES)
        views = self.views + self.slots
        # Who reads which row of the warp's output: every view's render its own sample (d_xyz, d_scaling, d_rotation); a flow pair (view sample
        # i, partner sample j) reads i whole + j's d_xyz for "this keyframe -> the earlier one", and j whole + i's d_xyz for the way back. All
        # readers are outputs of ONE node (control_nodes.fan_out) whose backward adds a row's gradients in one launch for all rows.
        plan = []

        def reader(i, whole):
            pos = {"x": len(plan)}
            plan.append((0, i))
            if whole:
                pos["s"], pos["r"] = len(plan), len(plan) + 1
                plan.extend([(2, i), (1, i)])
            return pos

        render_readers = [reader(i, True) for i in lay["view_idx"]]
        flow_readers = {}
        if r.with_flow:
            for k in range(len(views)):
                if k < nv and lay["partners"][k] is None:
                    continue
                i = lay["view_idx"][k]
                j = lay["partner_idx"][k] if k < nv else i + 1
                flow_readers[k] = (reader(i, True), reader(j, False), reader(j, True), reader(i, False))
        fan = control_nodes.fan_out(it["blended_stacked"], plan)
        deltas = [(fan[p["x"]], fan[p["s"]], fan[p["r"]]) for p in render_readers]
        cfg = be.config
        ops = self._window_ops.get(r.dyn)          # (held by the call: a captured iteration points at these buffers)
        if ops is None:
            ops = self._window_ops[r.dyn] = [be.keyframe_operands.get(cfg, v, dev, rm_dynamic=False, dynamic=r.dyn) for v in self.views]
        ops = ops + [o + (ops[0][4],) for o in self.slot_ops]
        with _region("gsr.render"):
            rendered = be._render_many(views, deltas)
        # The iteration's loss is a sum of terms whose VALUE nobody reads (the fused losses leave it uninitialised): instead of adding them up --
        # a launch per term -- every term is a root of ONE backward pass with the gradient 1 (be.unit_gradient): the same gradients, exactly
        terms = [loss_network]
        with _region("gsr.losses"):
            for v, pkg, (gt_image, gt_depth, w_rgb, w_dep, alpha) in zip(views, rendered, ops):
                terms.append(slam_losses.weighted_l1_loss(pkg["render"], pkg["depth"], gt_image, gt_depth, w_rgb, w_dep, v.exposure_a,
                                                          v.exposure_b, alpha, compute_value=False))
        if r.with_flow:
            from gaussian_renderer import render_flow_views
            requests, pairs, clips = [], [], []
            if self.n_slots and tab["clips"] is not None:
                torch.index_select(tab["clips"], 0, slot_index.long(), out=self.slot_clips[:self.n_slots])
            for k, v in enumerate(views):
                if k < nv:
                    other, f6 = lay["partners"][k], lay["flow6"][k]
                    if other is None:
                        continue
                    clips += list(lay["clips"][k])
                else:
                    other, f6 = self.partner_slots[k - nv], self.partner_flow[k - nv]
                    clips += [self.slot_clips[k - nv, 0:4], self.slot_clips[k - nv, 4:8]]
                a1, b1, a2, b2 = flow_readers[k]
                requests += [(v, other, fan[a1["x"]], fan[b1["x"]], fan[a1["r"]], fan[a1["s"]]),      # this keyframe -> the earlier one,
                             (other, v, fan[a2["x"]], fan[b2["x"]], fan[a2["r"]], fan[a2["s"]])]      # and back
                pairs.append(keyframe_slots.FlowTargets.pair_operands(f6))
            if requests:
                with _region("gsr.flow_render"):
                    flows = render_flow_views(g, requests, clips=clips if FLOW_CLIPS else None)
                if FLOW_CLIPS and be.config["Training"].get("flow_clip_check") and not torch.cuda.is_current_stream_capturing():
                    self._check_flow_clips(requests, pairs, clips, flows)          # TEST facility: the same terms without the clips
                with _region("gsr.flow_losses"):
                    for k, (t_back, m1, t_fwd, m2) in enumerate(pairs):
                        terms.append(slam_losses.masked_l1(r.flow_weight, [(flows[2 * k]["render"], t_back, m1), (flows[2 * k + 1]["render"], t_fwd, m2)],
                                                           channels=2, compute_value=False))          # (nobody reads the value: eligible() excludes loss_values)
        with _region("gsr.isotropic"):
            terms.append(be._isotropic_loss())
        torch.autograd.backward(terms, [be.unit_gradient(dev)] * len(terms))
        with _region("gsr.end_iteration"):
            nodes.end_iteration()
        with torch.no_grad(), _region("gsr.updates"):
            if special is not None and special.get("last"):           # (before a densification changes the row count, like the eager loop)
                be._publish_visibility(self.current_window, {k: rendered[k]["n_touched"] for k in range(nv)}, n_views=nv)
            for pkg in rendered:
                be._view_stats(pkg)
            split = be._maintain(be.iteration_count, rendered, enabled=special is not None and r.stepping)
            be._pose_updates(self.views, self.current_window, positions=self.positions)
            be._clear_camera_grads(self.slots + self.partner_slots)
            g.deform.optimizer.step()
            g.deform.optimizer.zero_grad(set_to_none=True)
            if r.stepping:                                                    # :765-770
                if special is None:
                    g.optimizer.step_scheduled(r.todo, r.schedule.coefficients_ptr())
                else:
                    g.optimizer.step()
                    g.update_learning_rate(be.iteration_count)
            g.optimizer.zero_grad(set_to_none=True)
        self.pkgs = rendered
        return split

    def _check_flow_clips(self, requests, pairs, clips, flows):
        """TEST facility (Training.flow_clip_check): render the iteration's flow images again WITHOUT the clips and record, in
        backend.flow_clip_checks, whether the masked images are equal, how far the gradients of the flow loss are apart (relative to their
        largest entry) and how many Gaussians each variant rasterized."""
        from gaussian_renderer import render_flow_views
        be, g, r = self.be, self.g, self.run

        def grads_of(cl):
            fl = render_flow_views(g, requests, clips=cl)
            loss = 0.0
            for k, (t_back, m1, t_fwd, m2) in enumerate(pairs):
                loss = loss + slam_losses.masked_l1(r.flow_weight, [(fl[2 * k]["render"], t_back, m1), (fl[2 * k + 1]["render"], t_fwd, m2)], channels=2)
            leaves = [g._xyz] + [t for rq in requests for t in rq[2:]]
            out = torch.autograd.grad(loss, leaves, allow_unused=True)
            g.optimizer.zero_grad(set_to_none=True)
            return fl, out
        _, ga = grads_of(clips)
        ref, gb = grads_of(None)
        rel = 0.0
        for x, y in zip(ga, gb):
            if x is not None and y is not None and float(y.abs().max()) > 0:
                rel = max(rel, float((x - y).abs().max() / y.abs().max()))
        same = True
        with torch.no_grad():
            for k, (t_back, m1, t_fwd, m2) in enumerate(pairs):
                for j, m in ((2 * k, m1), (2 * k + 1, m2)):
                    same = same and torch.equal(flows[j]["render"][:2] * m, ref[j]["render"][:2] * m)
            drawn = (sum(int((f["radii"] > 0).sum()) for f in flows), sum(int((f["radii"] > 0).sum()) for f in ref))
        be.flow_clip_checks.append({"masked_images_equal": same, "gradient_rel_diff": rel, "gaussians_drawn": drawn})

    # ---- executing a run ---------------------------------------------------------------------------------------------------------------
    def direct(self, n):
        for _ in range(n):
            self.iteration()
        self.stats["direct"] += n

    # ---- for slam/graph_run.py -------------------------------------------------------------------------------------------------------
    def state_tensors(self):
        g = self.g
        return (gaussian_state(g.optimizer, [p for grp in g.optimizer.param_groups for p in grp["params"]], self.run.todo)
                + network_state(g.deform.optimizer) + densification_statistics(g) + [self.counter] + window_state(self.views))

    def discard(self):
        for v in self.views:
            v.refresh_matrices()
        self.g.optimizer.zero_grad(set_to_none=True)
        self.g.deform.optimizer.zero_grad(set_to_none=True)
        self.be._clear_camera_grads(self.views + self.slots + self.partner_slots)

    def run_rows(self, rows):
        """A run of plain iterations: replays of one captured iteration when the run is long enough and graphs are on; directly executed,
        what the graph did not do."""
        be, r = self.be, self.run
        done = 0
        if (be._graphs_enabled() and rows >= be.graph_min_run and not graph_run.broken(be, "dynamic_graph")
                and (not r.stepping or r.todo is not None)):
            # (TEST facility, Training.graph_test_shrink_permille: lay the captured buffers out too small, so that replays overflow)
            options = dict(CAPTURE_OPTIONS, cap_test_shrink_permille=int(be.config["Training"].get("graph_test_shrink_permille", 0)))
            done = graph_run.replay_run(be, self, rows, min(be.dynamic_graph_warmup, rows), kind="dynamic_graph", options=options)
        self.direct(rows - done)
        catch_up(be, r.todo, rows, counts_iterations=r.stepping)

    def execute(self):
        """All iterations of the call. Returns gaussian_split of the last one (:336,:745)."""
        be, g = self.be, self.g
        i, split = 0, False
        nv = len(self.views)
        while i < self.iters:
            ph = self.phase(i)
            stepping = ph[1]
            rows = plain_rows(be, i, self.iters, self.warm)
            if rows == 0 or (stepping and g.optimizer.scheduled_segments() is None):          # special, or no Adam moments yet
                if stepping:
                    be.iteration_count += 1                                      # :337-338
                be.last_sent += 1
                self.make_run(i, 1, ph)
                split = self.iteration(special={"last": i == self.iters - 1})
                self.stats["special"] += 1
                i += 1
                continue
            self.make_run(i, rows, ph)
            self.run_rows(rows)
            split = False
            i += rows
            if i == self.iters:
                with torch.no_grad():
                    be._publish_visibility(self.current_window, {k: self.pkgs[k]["n_touched"] for k in range(nv)}, n_views=nv)
        self.run, self.pkgs = None, None
        return split


class NetworkInit:
    """BackEnd.initialize_network's loop (utils/slam_backend.py:160-234: the node network fitted on ONE view -- network, blend, render, the
    mapping loss without exposure, backward, Adam on the network) in the indexed layout (one time sample, every head), its iterations after the
    first -- which may densify -- as hipGraph replays (slam/graph_run.py). ``iteration()`` is one code path, executed directly or captured and
    replayed."""

    def __init__(self, backend, viewpoint):
        be = self.be = backend
        self.g, self.viewpoint = be.gaussians, viewpoint
        self.nodes = self.g.deform.deform
        dev = self.device = viewpoint.device
        self.ops = be.keyframe_operands.get(be.config, viewpoint, dev, rm_dynamic=False, dynamic=False)
        self.time = torch.tensor([time_key(viewpoint.time)], dtype=torch.float32).to(dev)
        self.pkg = None
        self.stats = graph_run.stats(be, "network_init_graph")

    @staticmethod
    def eligible(be, viewpoint, update_gaussians):
        g, t = be.gaussians, be.config["Training"]
        return (t.get("dynamic_fixed_layout", True) and not update_gaussians and not be.shard.active and not be.loss_values and not t.get("monocular", False)
                and str(be.device).startswith("cuda") and isinstance(viewpoint, Camera) and viewpoint.depth is not None and g.deform_init
                and g.deform.deform.node_num >= 1 and g.dyn_rows().shape[0] > 0 and getattr(g.optimizer, "_fused_acc", False))

    def iteration(self, densify=False):
        be, g, nodes, v = self.be, self.g, self.nodes, self.viewpoint
        self.pkg = None
        it = nodes.begin_iteration_indexed(self.time, 1, blend=(g.get_dygs_xyz.detach(), g.motion_mask))
        rows = it["blended"]
        pkg = be._render(v, (rows[0][0], rows[2][0], rows[1][0]))
        gt_image, gt_depth, w_rgb, w_dep, alpha = self.ops
        slam_losses.weighted_l1_loss(pkg["render"], pkg["depth"], gt_image, gt_depth, w_rgb, w_dep, None, None, alpha, compute_value=False).backward()
        nodes.end_iteration()
        with torch.no_grad():
            be._view_stats(pkg)
            be._maintain_init(densify)                                            # :209-215 (iteration 0 with the shipped schedule)
            g.deform.optimizer.step()
            g.deform.optimizer.zero_grad(set_to_none=True)
            g.optimizer.zero_grad(set_to_none=True)
        # (the view's camera parameters keep accumulating their gradients, as in the reference: see mapping_graph.InitGraph)
        self.pkg = pkg
        return pkg

    def state_tensors(self):
        return network_state(self.g.deform.optimizer) + densification_statistics(self.g) + camera_gradients(self.viewpoint)

    def discard(self):
        """(the view's camera gradients are part of the snapshot: they accumulate across the loop on purpose, see iteration())"""
        self.g.optimizer.zero_grad(set_to_none=True)
        self.g.deform.optimizer.zero_grad(set_to_none=True)

    def run(self, iterations):
        """All iterations of the loop; returns the last render package."""
        be = self.be
        i = 0
        while i < iterations:
            rows = plain_run(i, iterations, lambda k: init_rule(be, k)[0])
            if rows == 0:
                self.iteration(densify=True)
                self.stats["direct"] += 1
                i += 1
                continue
            done = 0
            if be._graphs_enabled() and rows >= be.graph_min_run and not graph_run.broken(be, "network_init_graph"):
                done = graph_run.replay_run(be, self, rows, min(be.dynamic_graph_warmup, rows), kind="network_init_graph", options=CAPTURE_OPTIONS)
            else:
                self.stats["direct"] += rows
            for _ in range(rows - done):
                self.iteration()
            i += rows
        return self.pkg
