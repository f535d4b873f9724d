"""Loop closure: constraints between keyframes that see the same place, a pose graph over the keyframes, and a rigid correction of the map
that follows the corrected keyframes. The checked ctypes binding of include/loop_closure.h (gsr_pose_graph_solve: damped Gauss-Newton with
block-Jacobi preconditioned conjugate gradients in one workgroup; gsr_map_correct: every Gaussian moved with the keyframe that seeded it;
csrc/gs_loop.h) and what is built from them:

  PoseGraph      the keyframe ids in insertion order and the edges (odometry, loop) on the device
  LoopCloser     on_keyframe(): candidates of the place index (slam/relocalise.py KeyframeIndex) older than min_gap keyframes, each verified
                 by a two-way dense alignment of the REAL frames (slam/odometry.py); accepted ones become loop edges; solve(): one
                 gsr_pose_graph_solve and, where the largest correction exceeds min_correction, gsr_map_correct on the model and
                 X <- X D_k^-1 on every camera of the run; close_all(): the same for every keyframe of a finished run, then one solve()

The front-end's stage is slam/stages.py LoopClosure (``Training.loop_closure``). The reference has no counterpart.
tests/pose_graph_reference.py restates the two calls in float64 numpy. No CPU path.

Limits: nothing here has been run on real images or on a trajectory that drifted by itself. RGB-D and stereo input with a static map only:
monocular drift includes scale (that needs Sim(3)), a deformation field lives in world coordinates and cannot be moved piecewise, and
spherical harmonics of degree 1 and higher would need rotating. Adam's moments are not moved with the Gaussians (include/loop_closure.h)."""
import bisect
import math

import torch

from diff_gaussian_rasterization import _C

from .pretrained import EventLog
from .relocalise import KeyframeIndex

I32, F64 = (torch.int32,), (torch.float64,)
STATS = ("initial_cost", "final_cost", "outer_iterations", "last_step", "edges_used", "edges_skipped", "max_translation", "max_rotation")
MAX_NODES, MAX_EDGES = 4096, 65536


# ---- the two calls -------------------------------------------------------------------------------------------------------------------
def pose_graph_workspace_size(nodes, edges):
    return int(_C.load_library().gsr_pose_graph_workspace_size(int(nodes), int(edges)))


def pose_graph_solve(poses, fixed, edge_nodes, edge_Z, edge_weights, edges, outer_iters, cg_iters, lam, step_tol, D, stats, workspace=None,
                     stream=None):
    """One call of gsr_pose_graph_solve. poses float64 [N, 12] (read and overwritten); fixed int32 [N]; the first `edges` rows of edge_nodes
    int32 [>= edges, 2], edge_Z float64 [>= edges, 12] and edge_weights float64 [>= edges, 2] (all three None with edges == 0); D float32
    [N, 12] and stats float64 [8] (STATS) are written. The library checks the ranges and raises RuntimeError with its text."""
    _C._require_device(poses, "poses")
    if poses.dim() != 2 or poses.shape[1] != 12:
        raise RuntimeError(f"poses must be [N, 12], got {tuple(poses.shape)}")
    N, E, dev = int(poses.shape[0]), int(edges), poses.device
    for name, t, width in (("edge_nodes", edge_nodes, 2), ("edge_Z", edge_Z, 12), ("edge_weights", edge_weights, 2)):
        if t is not None and (t.dim() != 2 or t.shape[0] < E or t.shape[1] != width):
            raise RuntimeError(f"{name} must be [>= {E}, {width}], got {tuple(t.shape)}")
    args = [_C.dev_ptr(poses, "poses", F64), _C.dev_ptr(fixed, "fixed", I32, (N,)), _C.dev_ptr(edge_nodes, "edge_nodes", I32),
            _C.dev_ptr(edge_Z, "edge_Z", F64), _C.dev_ptr(edge_weights, "edge_weights", F64)]
    outs = [_C.dev_ptr(D, "D", _C.F32, (N, 12)), _C.dev_ptr(stats, "stats", F64, (len(STATS),))]
    lib = _C.load_library()
    workspace = _C.workspace(workspace, int(lib.gsr_pose_graph_workspace_size(N, E)) if workspace is None else 0, dev)
    with torch.cuda.device(dev):
        lib.gsr_pose_graph_solve(N, E, *args, int(outer_iters), int(cg_iters), float(lam), float(step_tol), *outs, workspace.data_ptr() or None,
                                 int(workspace.numel()), _C.stream_handle(stream, dev))


def map_correct(xyz, rotation, kf_id, slot_of_frame, D, quat_workspace=None, stream=None):
    """One call of gsr_map_correct, in place on xyz float32 [P, 3] and rotation float32 [P, 4]. kf_id int32 [P]; slot_of_frame int32
    [frames] (None: no frame has a slot); D float32 [N, 12]; quat_workspace None or float32 [N, 4]."""
    _C._require_device(D, "D")
    if D.dim() != 2 or D.shape[1] != 12:
        raise RuntimeError(f"D must be [N, 12], got {tuple(D.shape)}")
    P, N, dev = int(xyz.shape[0]), int(D.shape[0]), D.device
    frames = 0 if slot_of_frame is None else int(slot_of_frame.shape[0])
    if quat_workspace is None:
        quat_workspace = torch.empty((N, 4), dtype=torch.float32, device=dev)
    args = [_C.dev_ptr(xyz, "xyz", _C.F32, (P, 3)), _C.dev_ptr(rotation, "rotation", _C.F32, (P, 4)), _C.dev_ptr(kf_id, "kf_id", I32, (P,))]
    table = _C.dev_ptr(slot_of_frame, "slot_of_frame", I32, (frames,))
    with torch.cuda.device(dev):
        _C.load_library().gsr_map_correct(P, *(a or None for a in args), frames, table or None, N, _C.dev_ptr(D, "D", _C.F32, (N, 12)),
                                          _C.dev_ptr(quat_workspace, "quat_workspace", _C.F32, (N, 4)), _C.stream_handle(stream, dev))


# ---- small device-side pose algebra (float64 [4, 4]); nothing here reads the device ---------------------------------------------------
def pose44(R, t):
    T = torch.eye(4, dtype=torch.float64, device=R.device)
    T[:3, :3], T[:3, 3] = R.detach().to(torch.float64), t.detach().to(torch.float64)
    return T


def inverse44(T):
    out = torch.eye(4, dtype=T.dtype, device=T.device)
    Rt = T[:3, :3].transpose(0, 1)
    out[:3, :3], out[:3, 3] = Rt, -(Rt @ T[:3, 3])
    return out


def motion_size(T):
    """(|rho|, angle in radians) of Log(T) as one device tensor [2]: the header's Log, its branch away from pi (a rotation near pi is far
    beyond any gate this is compared with and comes out large either way)."""
    R, t = T[:3, :3], T[:3, 3]
    ax = torch.stack([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    c = (0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)).clamp(-1.0, 1.0)
    s = 0.5 * torch.linalg.norm(ax)
    a = torch.atan2(s, c)
    small = a < 1e-5
    safe = torch.where(small, torch.ones_like(a), a)
    theta = torch.where(small, 0.5 * ax, (safe / (2.0 * torch.where(small, torch.ones_like(s), s))) * ax)
    G = torch.where(small, torch.full_like(a, 1.0 / 12.0), (1.0 - 0.5 * safe * torch.cos(0.5 * safe) / torch.sin(0.5 * safe)) / (safe * safe))
    W = torch.zeros((3, 3), dtype=T.dtype, device=T.device)
    W[0, 1], W[0, 2], W[1, 0], W[1, 2], W[2, 0], W[2, 1] = -theta[2], theta[1], theta[2], -theta[0], -theta[1], theta[0]
    rho = t - 0.5 * (W @ t) + G * (W @ (W @ t))
    return torch.stack([torch.linalg.norm(rho), a])


def correction_node(frame, ids):
    """The node whose correction a frame takes: its own for a keyframe; for any other frame the last keyframe at or before it; None for a
    frame before the first keyframe. ids: the keyframe ids in insertion order, ascending."""
    k = bisect.bisect_right(ids, frame) - 1
    return k if k >= 0 else None


# ---- the graph -------------------------------------------------------------------------------------------------------------------------
class PoseGraph:
    """Keyframe ids in insertion order (the node of an id is its position) and the edges on the device: edge_nodes int32 [capacity, 2],
    edge_Z float64 [capacity, 12], edge_weights float64 [capacity, 2], the first `edges` rows in use (they double when full). `loops`
    lists the loop edges as (old id, new id). Adding an edge reads nothing from the device."""

    def __init__(self, device, capacity=64):
        self.device = torch.device(device)
        self.ids, self.node, self.loops, self.edges = [], {}, [], 0
        self.edge_nodes = torch.zeros((capacity, 2), dtype=torch.int32, device=self.device)
        self.edge_Z = torch.zeros((capacity, 12), dtype=torch.float64, device=self.device)
        self.edge_weights = torch.zeros((capacity, 2), dtype=torch.float64, device=self.device)

    def clear(self):
        self.ids, self.node, self.loops, self.edges = [], {}, [], 0

    def add_node(self, frame_id):
        if len(self.ids) == MAX_NODES:
            raise RuntimeError(f"PoseGraph: more than {MAX_NODES} keyframes")
        self.node[frame_id] = len(self.ids)
        self.ids.append(frame_id)

    def _add(self, i, j, Z, weights):
        if self.edges == MAX_EDGES:
            raise RuntimeError(f"PoseGraph: more than {MAX_EDGES} edges")
        if self.edges == self.edge_nodes.shape[0]:
            for name in ("edge_nodes", "edge_Z", "edge_weights"):
                old = getattr(self, name)
                grown = torch.zeros((2 * old.shape[0], old.shape[1]), dtype=old.dtype, device=self.device)
                grown[:old.shape[0]] = old
                setattr(self, name, grown)
        n = self.edges
        self.edge_nodes[n] = torch.tensor([self.node[i], self.node[j]], dtype=torch.int32)
        self.edge_Z[n] = Z.detach().to(device=self.device, dtype=torch.float64)[:3, :4].reshape(12)
        self.edge_weights[n] = torch.tensor([float(weights[0]), float(weights[1])], dtype=torch.float64)
        self.edges = n + 1

    def add_odometry_edge(self, i, j, cameras, weights):
        """The edge (i, j) whose Z is the current estimate X_j X_i^-1 of the cameras' poses (device arithmetic, float64)."""
        a, b = cameras[i], cameras[j]
        self._add(i, j, pose44(b.R, b.T) @ inverse44(pose44(a.R, a.T)), weights)

    def add_loop_edge(self, i, j, Z, weights):
        """The verified constraint X_j ~ Z X_i between the old keyframe i and the new one j; Z [4, 4] on the device."""
        self._add(i, j, Z, weights)
        self.loops.append((i, j))


# ---- the loop closer -------------------------------------------------------------------------------------------------------------------
class LoopCloser:
    """options: slam.stages.loop_closure_options(...); cameras: {frame id: Camera} of the run (keyframes keep their image and depth);
    get_gaussians: a callable returning the run's GaussianModel as it is now (the back-end may replace it); size = (width, height), K =
    (fx, fy, cx, cy); index: a KeyframeIndex another stage fills with every keyframe (relocalisation), or None to own one; feature_seed:
    slam.features.feature_seed_options(...) or None -- with it verify() starts at the pose of matched features (slam/features.py) where
    that is accepted, and the alignment may then move as far as that block's gate allows."""

    def __init__(self, options, cameras, get_gaussians, size, K, device, index=None, feature_seed=None):
        from .odometry import DenseOdometry
        self.options, self.cameras, self.get_gaussians, self.device = options, cameras, get_gaussians, torch.device(device)
        self.shared_index = index is not None
        self.index = index if self.shared_index else KeyframeIndex.from_options(options, self.device)
        self.graph = PoseGraph(self.device)
        self.stats = {"keyframes_queried": 0, "candidates_verified": 0, "edges_accepted": 0, "solves": 0, "corrections_applied": 0,
                      "max_correction_m": 0.0, "max_correction_deg": 0.0}
        self.seeder = None
        gate = (options["max_translation"], options["max_rotation"])
        if feature_seed is not None:
            from .features import FeatureSeeder
            self.seeder = FeatureSeeder(size, K, feature_seed, self.device)
            gate = (max(gate[0], feature_seed["max_translation"]), max(gate[1], feature_seed["max_rotation"]))
            self.stats.update(feature_seeds_tried=0, feature_seeds_accepted=0)
        self.odometry = DenseOdometry(size[0], size[1], K, levels=options["levels"], iters=options["iters"], max_translation=gate[0],
                                      max_rotation=gate[1], device=self.device, affine=True, geometric_weight=options["geometric_weight"])
        self.verify_log, self.solve_log = EventLog(self.device), EventLog(self.device)
        self.last_solve = None

    @property
    def gaussians(self):
        return self.get_gaussians()

    def clear(self):
        self.graph.clear()
        if not self.shared_index:
            self.index.clear()
        if self.seeder is not None:
            self.seeder.forget()

    # ---- verification ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def verify(self, a, b):
        """Two-way dense alignment of the real frames of the keyframes a (old) and b (new), frame ids: forward keep(a), align(b) from
        X_b X_a^-1 gives T_ab; backward keep(b), align(a) from T_ab^-1 gives T_ba. Accepted when both gates accept and Log(T_ba T_ab) is
        below `consistency`. ONE host read: the two flags and the size of the inconsistency, together. Returns (accepted, T_ab [4, 4] float32
        on the device, {"forward", "backward", "translation" in metres, "rotation" in degrees}). With the feature seed on, verify_seeded()."""
        if self.seeder is not None:
            return self.verify_seeded(a, b)
        ca, cb = self.cameras[a], self.cameras[b]
        with self.verify_log.timed():
            start = (pose44(cb.R, cb.T) @ inverse44(pose44(ca.R, ca.T))).to(torch.float32)
            self.odometry.keep(ca.original_image, ca.depth_device(), None)
            T_ab, s_ab = self.odometry.align(cb.original_image, start, depth=cb.depth_device())
            self.odometry.keep(cb.original_image, cb.depth_device(), None)
            T_ba, s_ba = self.odometry.align(ca.original_image, inverse44(T_ab.to(torch.float64)).to(torch.float32), depth=ca.depth_device())
            size = motion_size(T_ba.to(torch.float64) @ T_ab.to(torch.float64))
            packed = torch.cat([s_ab[:1], s_ba[:1], size])
        forward, backward, metres, radians = packed.tolist()
        degrees = math.degrees(radians)
        ok = forward > 0.5 and backward > 0.5 and metres <= self.options["consistency"][0] and degrees <= self.options["consistency"][1]
        self.stats["candidates_verified"] += 1
        return ok, T_ab, {"forward": forward > 0.5, "backward": backward > 0.5, "translation": metres, "rotation": degrees}

    @torch.no_grad()
    def verify_seeded(self, a, b):
        """verify() with the feature seed: the keypoints of the two real frames (kept per frame id) are matched and posed; an accepted pose
        replaces X_b X_a^-1 as the start of the forward alignment. The two alignments run with the wider of the two gates; where the seed
        was refused their own, narrower gate is applied afterwards on the device (features.gated), which is what verify() decides for
        that pair. The two-way test decides as before. Still ONE host read, the seed's flag packed into it; the dictionary gains "seeded"."""
        from .features import gated
        ca, cb = self.cameras[a], self.cameras[b]
        opt = self.options
        with self.verify_log.timed():
            seed, seed_stats = self.seeder.pose(self.seeder.cached(a, ca.original_image), ca.depth_device(),
                                                self.seeder.cached(b, cb.original_image), cb.depth_device())
            seeded = seed_stats[6]
            start = (pose44(cb.R, cb.T) @ inverse44(pose44(ca.R, ca.T))).to(torch.float32)
            start = torch.where(seeded > 0, seed, start)
            self.odometry.keep(ca.original_image, ca.depth_device(), None)
            T_ab, s_ab = self.odometry.align(cb.original_image, start, depth=cb.depth_device())
            T_ab, f_ab = gated(T_ab, s_ab[0], seeded, opt["max_translation"], opt["max_rotation"])
            self.odometry.keep(cb.original_image, cb.depth_device(), None)
            T_ba, s_ba = self.odometry.align(ca.original_image, inverse44(T_ab.to(torch.float64)).to(torch.float32), depth=ca.depth_device())
            T_ba, f_ba = gated(T_ba, s_ba[0], seeded, opt["max_translation"], opt["max_rotation"])
            size = motion_size(T_ba.to(torch.float64) @ T_ab.to(torch.float64))
            packed = torch.cat([torch.stack([f_ab, f_ba]), size, seeded.to(torch.float64).reshape(1)])
        forward, backward, metres, radians, seeded = packed.tolist()
        degrees = math.degrees(radians)
        ok = forward > 0.5 and backward > 0.5 and metres <= opt["consistency"][0] and degrees <= opt["consistency"][1]
        self.stats["candidates_verified"] += 1
        self.stats["feature_seeds_tried"] += 1
        self.stats["feature_seeds_accepted"] += int(seeded > 0.5)
        return ok, T_ab, {"forward": forward > 0.5, "backward": backward > 0.5, "translation": metres, "rotation": degrees,
                          "seeded": seeded > 0.5}

    def _candidates(self, viewpoint, rows):
        """The rows of the index among its first `rows` whose code is close enough to the frame's: ONE host read, the topk pairs."""
        opt = self.options
        self.stats["keyframes_queried"] += 1
        if rows <= 0:
            return []
        best, _ = self.index.query(viewpoint.original_image, viewpoint.depth_device(), None, opt["topk"], rows=rows)
        limit = opt["max_code_distance"] * self.index.ferns
        return [row for row, distance in best.tolist() if row >= 0 and distance <= limit]

    def _link(self, frame_id, viewpoint, rows):
        """Node, odometry edge and verified loop edges of one keyframe; returns the old keyframes it was tied to."""
        opt, graph = self.options, self.graph
        previous = graph.ids[-1] if graph.ids else None
        graph.add_node(frame_id)
        if previous is not None:
            graph.add_odometry_edge(previous, frame_id, self.cameras, opt["odometry_weights"])
        tied = []
        for row in self._candidates(viewpoint, rows):
            old = self.index.ids[row]
            if old not in graph.node or old == frame_id:
                continue
            ok, T_ab, _ = self.verify(old, frame_id)
            if ok:
                graph.add_loop_edge(old, frame_id, T_ab, opt["loop_weights"])
                self.stats["edges_accepted"] += 1
                tied.append(old)
        return tied

    def on_keyframe(self, frame_id, viewpoint):
        """The new keyframe becomes a node; the index is searched over the rows older than min_gap keyframes; every candidate is verified;
        accepted ones become loop edges and, if there is one, solve() runs. With a shared index the keyframe is its newest row already; an
        owned index gets it here, after the search. Returns None, or solve()'s dictionary extended by "keyframes": the old ones tied to."""
        node = len(self.graph.ids)
        tied = self._link(frame_id, viewpoint, node - self.options["min_gap"])
        if not self.shared_index:
            self.index.add(frame_id, viewpoint.original_image, viewpoint.depth_device(), None)
        if not tied:
            return None
        return {**self.solve(), "keyframes": tied}

    def close_all(self, kf_ids):
        """For a finished run: graph and (owned) index are rebuilt from the keyframes `kf_ids` in insertion order, each searched and verified
        as on_keyframe does, then ONE solve(). Returns its dictionary extended by "keyframes": (old, new) of every loop edge."""
        if self.shared_index:                                  # the run's own index holds every keyframe already: search a private one
            self.index, self.shared_index = KeyframeIndex.from_options(self.options, self.device), False
        self.clear()
        for frame_id in kf_ids:
            viewpoint = self.cameras[frame_id]
            self._link(frame_id, viewpoint, len(self.graph.ids) - self.options["min_gap"])
            self.index.add(frame_id, viewpoint.original_image, viewpoint.depth_device(), None)
        return {**self.solve(), "keyframes": list(self.graph.loops)}

    # ---- the solve and the correction -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def solve(self):
        """Upload the keyframe poses, one gsr_pose_graph_solve with node 0 fixed, ONE host read (stats); where the largest correction exceeds
        min_correction (metres or degrees) it is applied: gsr_map_correct on the model, X <- X D_k^-1 on every camera. Otherwise nothing
        is touched. Returns {"applied", "translation" (m), "rotation" (deg), "stats": {STATS}}."""
        opt, graph = self.options, self.graph
        N = len(graph.ids)
        cams = [self.cameras[k] for k in graph.ids]
        R = torch.stack([c.R.detach() for c in cams]).to(torch.float64)
        t = torch.stack([c.T.detach() for c in cams]).to(torch.float64)
        poses = torch.cat([R, t[:, :, None]], dim=2).reshape(N, 12).contiguous()
        fixed = torch.zeros(N, dtype=torch.int32, device=self.device)
        fixed[0] = 1
        D = torch.empty((N, 12), dtype=torch.float32, device=self.device)
        stats = torch.empty(len(STATS), dtype=torch.float64, device=self.device)
        with self.solve_log.timed():
            pose_graph_solve(poses, fixed, graph.edge_nodes, graph.edge_Z, graph.edge_weights, graph.edges, opt["outer_iters"], opt["cg_iters"],
                             opt["lambda"], opt["step_tolerance"], D, stats)
        values = dict(zip(STATS, stats.tolist()))
        metres, degrees = values["max_translation"], math.degrees(values["max_rotation"])
        self.stats["solves"] += 1
        applied = metres > opt["min_correction"][0] or degrees > opt["min_correction"][1]
        if applied:
            self.apply(poses, D)
            self.stats["corrections_applied"] += 1
            self.stats["max_correction_m"] = max(self.stats["max_correction_m"], metres)
            self.stats["max_correction_deg"] = max(self.stats["max_correction_deg"], degrees)
        self.last_solve = {"applied": bool(applied), "translation": metres, "rotation": degrees, "stats": values}
        return self.last_solve

    @torch.no_grad()
    def apply(self, poses, D):
        """The correction D [N, 12] of the graph's nodes on the map and on every camera: a keyframe gets the solver's pose, any other frame
        X <- X D_k^-1 with k = correction_node(frame). In place everywhere: no tensor of the model or of a camera is replaced."""
        ids = self.graph.ids
        table = torch.full((max(ids) + 1,), -1, dtype=torch.int32)
        table[torch.tensor(ids, dtype=torch.long)] = torch.arange(len(ids), dtype=torch.int32)
        g = self.gaussians
        map_correct(g._xyz.data, g._rotation.data, g.unique_kfIDs, table.to(self.device), D)
        X = poses.reshape(-1, 3, 4).to(torch.float32)
        Dm = D.reshape(-1, 3, 4)
        for frame, camera in self.cameras.items():
            k = self.graph.node.get(frame)
            if k is not None:
                camera.update_RT(X[k, :, :3], X[k, :, 3])
                continue
            k = correction_node(frame, ids)
            if k is None:
                continue
            R = camera.R.detach() @ Dm[k, :, :3].transpose(0, 1)             # X D^-1 = [R R_D^T | t - R R_D^T t_D]
            camera.update_RT(R, camera.T.detach() - R @ Dm[k, :, 3])

    def summary(self):
        """The `loop_closure` block of the run result."""
        return {**self.stats, "device_ms_per_verify": self.verify_log.summary()["ms_per_item"] or 0.0,
                "device_ms_per_solve": self.solve_log.summary()["ms_per_item"] or 0.0}
