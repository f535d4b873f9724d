"""The device-side schedule of a run of graph-replayed mapping iterations (slam/mapping_graph.py, slam/dynamic_graph.py): what depends on
the iteration NUMBER is a row ``[index words | Adam coefficients | float samples]`` (any block may be empty) of a table written once per run;
``gsr_schedule_advance`` (include/slam_map.h) copies row ``counter`` into the ``current`` block the iteration reads and bumps the counter.
The runners draw and hand the results over. Also here: what the host owes a run afterwards, and the pieces of the runners' snapshots.

And the HOST rule of what an iteration number does -- densify, reset opacities, or nothing ("plain") -- with the one splitter that measures a
run of plain iterations by it. Those iterations replace the model's tensors, so they run eagerly and end a run: the eager bodies
(slam/backend.py) and the runners' splitters (backend.py, slam/dynamic_graph.py) all ask mapping_rule / init_rule / plain_run and nobody
else writes the expressions out."""
import numpy as np
import torch

from diff_gaussian_rasterization import _C


def mapping_rule(backend, count):
    """What the mapping iteration whose iteration_count is `count` does to the model before its step (utils/slam_backend.py:722-745,
    :1185-1206): "densify", "reset" (the opacities of the Gaussians no view saw) or None; where both hold it densifies. The three periods
    are read from the back-end when asked."""
    if count % backend.gaussian_update_every == backend.gaussian_update_offset:
        return "densify"
    return "reset" if count % backend.gaussian_reset == 0 else None


def init_rule(backend, m, count=None):
    """(densify, reset opacities) of iteration `m` of an initialisation call (utils/slam_backend.py:217,:277-287); `count`: the
    iteration_count of that iteration, None for a loop that never resets (initialize_network). Both can hold: densify runs first."""
    return m % backend.init_gaussian_update == 0, count is not None and (count == backend.init_gaussian_reset or count == backend.opt_params.densify_from_iter)


def plain_run(start, stop, is_special):
    """The number of consecutive k in [start, stop) from `start` on for which is_special(k) is false."""
    n = 0
    while start + n < stop and not is_special(start + n):
        n += 1
    return n


def xyz_lr_rule(gaussians, count0):
    """lr_of of map_static / map: update_learning_rate(iteration_count) ran after the previous step (GM:492-505) -- from row 1 on, for xyz."""
    return lambda group, j: gaussians.xyz_lr_at(count0 + j) if j > 0 and group.get("name") == "xyz" else group["lr"]


def adam_rows(optimizer, todo, rows, lr_of=None):
    """(step size, 1 / sqrt(bias correction 2)) per tensor of `todo` (scheduled_segments) for the next `rows` steps, float32 [rows, 2 * len(todo)].
    lr_of(group, j): row j's rate (default group["lr"]), handed over as a Python float: coefficients() rounds to fp32 itself, like step()."""
    out = np.zeros((rows, 2 * len(todo)), dtype=np.float32)
    for j in range(rows):
        for k, (group, p) in enumerate(todo):
            lr = group["lr"] if lr_of is None else lr_of(group, j)
            out[j, 2 * k], out[j, 2 * k + 1] = optimizer.coefficients(lr, group["betas"], int(optimizer.state[p]["step"]) + j + 1)
    return out


class Schedule:
    def __init__(self, rows, device, index_words=None, adam=None, samples=None, counter=None):
        """`counter`: an int32 [1] device tensor the caller shares among its runs and zeroes per run; default: a fresh one."""
        table, self.coef_lo, self.samples_lo = self.pack(rows, index_words, adam, samples)
        self.rows, self.row_words, self.device = int(rows), int(table.shape[1]), device
        self.table = torch.from_numpy(table.view(np.int32)).pin_memory().to(device, non_blocking=True)
        self.counter = torch.zeros(1, dtype=torch.int32, device=device) if counter is None else counter
        self.current = torch.zeros(self.row_words, dtype=torch.int32, device=device)

    @staticmethod
    def pack(rows, index_words=None, adam=None, samples=None):
        """Host only: (uint32 [rows, row_words] table, word offset of the Adam block, of the samples); floats as their fp32 bits."""
        blocks = [np.ascontiguousarray([] if b is None else b, dtype=dt) for b, dt in ((index_words, np.uint32), (adam, np.float32), (samples, np.float32))]
        blocks = [b.reshape(rows, b.size // rows).view(np.uint32) for b in blocks]
        return np.concatenate(blocks, axis=1), blocks[0].shape[1], blocks[0].shape[1] + blocks[1].shape[1]

    def advance(self):
        with torch.cuda.device(self.device):
            _C.load_library().gsr_schedule_advance(self.counter.data_ptr(), self.table.data_ptr(), self.row_words, self.rows, self.current.data_ptr(),
                                                   _C._stream(self.device))

    def indices(self, n):
        return self.current[:n]

    def coefficients_ptr(self):
        """Device address of the current row's Adam block (FusedAdam.step_scheduled)."""
        return self.current.data_ptr() + 4 * self.coef_lo

    def samples(self):
        return self.current.view(torch.float32)[self.samples_lo:]


def catch_up(backend, todo, n, *, counts_iterations=True, sent=True, learning_rate=True):
    """Host-side state after `n` graph iterations: what n eager iterations would have left. `counts_iterations`: the Gaussians stepped
    (iteration_count, Adam's step counts of `todo`, and -- `learning_rate` -- the position learning rate of the new count)."""
    if sent:
        backend.last_sent += n
    if counts_iterations and n:
        backend.iteration_count += n
        backend.gaussians.optimizer.advance_steps(todo, n)
        if learning_rate:
            backend.gaussians.update_learning_rate(backend.iteration_count)


def gaussian_state(optimizer, params, todo):
    """Snapshot pieces (state_tensors() of the runners): `params`, each runner's own list, plus Adam's moments of `todo` (None: no step)."""
    return list(params) + [optimizer.state[p][k] for _, p in (todo or ()) for k in ("exp_avg", "exp_avg_sq")]


def network_state(optimizer):
    """Every parameter of the node network's optimizer with every tensor of its state."""
    return [t for grp in optimizer.param_groups for p in grp["params"]
            for t in [p] + [s for s in optimizer.state.get(p, {}).values() if torch.is_tensor(s)]]


def densification_statistics(g):
    return [g.xyz_gradient_accum, g.denom, g.max_radii2D]


def window_state(views):
    return [t for v in views for t in (v._R, v._T, v._adam, v._converged, v.exposure_a, v.exposure_b, v.cam_rot_delta, v.cam_trans_delta)]


def camera_gradients(v):
    """What one view's camera parameters have accumulated (the init runners never clear it: slam/mapping_graph.InitGraph)."""
    return [p.grad for p in (v.cam_rot_delta, v.cam_trans_delta, v.exposure_a, v.exposure_b) if p is not None and p.grad is not None]
