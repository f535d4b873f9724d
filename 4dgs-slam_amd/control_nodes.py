"""SC-GS control-node warp on the MI355X library (include/control_nodes.h) -- the per-Gaussian half of the reference's
utils/time_utils.py ControlNodeWarp: `knn_points` (the pytorch3d.ops routine the reference imports, which has no ROCm build),
`cal_nn_weight` (:981-1011) and `node_blend`, the body of ControlNodeWarp.forward (:1192-1258) after the node MLP.

The node MLP stays in torch (O(nodes) library GEMMs).  Everything else -- the K nearest nodes, exp / sigmoid of the raw node
radius / weight (:893-898), quaternion_to_matrix of the local rotations (:115-133,1207-1208), the RBF weights, the blend, and all
of their chain rules -- is one HIP launch forward and three backward.  There is no CPU path."""
import ctypes
from collections import namedtuple

import torch

from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization._abi import (GSR_BLEND_MAX_K, GSR_KNN_MAX_DIM, GSR_KNN_MAX_K, GSR_NODE_RADIUS_IS_LOG,
                                              GSR_NODE_WEIGHT_IS_LOGIT, gsr_multi_add_item, gsr_node_blend)

MAX_K, MAX_DIM, BLEND_MAX_K = GSR_KNN_MAX_K, GSR_KNN_MAX_DIM, GSR_BLEND_MAX_K
_KNN = namedtuple("KNN", "dists idx knn")
_lib = _C.load_library          # the declared library under its former name


def _f32(t, name, shape=None):
    _C._require_device(t, name)
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be fp32, got {t.dtype}")
    if shape is not None and t.shape != shape:
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.detach().contiguous()


def knn_points(p1, p2, lengths1=None, lengths2=None, K: int = 1, version: int = -1, return_nn: bool = False, return_sorted: bool = True):
    """pytorch3d.ops.knn_points for equal-length batches: p1 [B, N, D], p2 [B, M, D] -> (dists [B, N, K] squared, idx [B, N, K]
    int64, knn [B, N, K, D] or None).  No gradient flows through dists (the reference only uses detached inputs here)."""
    if lengths1 is not None or lengths2 is not None:
        raise NotImplementedError("knn_points: ragged batches (lengths1 / lengths2) are not used by the reference and not implemented")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError(f"knn_points expects p1 [B, N, D] and p2 [B, M, D], got {tuple(p1.shape)} and {tuple(p2.shape)}")
    B, N, D = p1.shape
    if not (1 <= K <= MAX_K) or not (1 <= D <= MAX_DIM):
        raise ValueError(f"knn_points: K = {K}, D = {D} outside 1..32")
    a, b = _f32(p1, "p1"), _f32(p2, "p2")
    dists = torch.empty((B, N, K), dtype=torch.float32, device=a.device)
    idx = torch.empty((B, N, K), dtype=torch.int64, device=a.device)
    lib = _C.load_library()
    with torch.cuda.device(a.device):
        lib.gsr_knn_points_batch(B, N, b.shape[1], D, K, a.data_ptr(), b.data_ptr(), dists.data_ptr(), idx.data_ptr(), _C._stream(a.device))
    knn = None
    if return_nn:
        knn = torch.gather(p2[:, None].expand(-1, N, -1, -1), 2, idx[..., None].expand(-1, -1, -1, D))
    return _KNN(dists, idx, knn)


class _FanOut(torch.autograd.Function):
    """outputs[k] = stacked[plan[k][0]][plan[k][1]] (aliases: no copy); backward: every row of every stacked tensor's gradient = the sum of the
    gradients of its readers, all rows in ONE launch (gsr_multi_add)."""

    @staticmethod
    def forward(ctx, plan, *stacked):
        ctx.plan, ctx.shapes = plan, [tuple(t.shape) for t in stacked]
        ctx.set_materialize_grads(False)
        return tuple(stacked[a].detach()[i] for a, i in plan)

    @staticmethod
    def backward(ctx, *grads):
        plan, shapes = ctx.plan, ctx.shapes
        dev = next(g for g in grads if g is not None).device if any(g is not None for g in grads) else None
        if dev is None:
            return (None,) + (None,) * len(shapes)
        outs = [torch.empty(shape, dtype=torch.float32, device=dev) for shape in shapes]
        readers, keep = {}, []
        for (a, i), g in zip(plan, grads):
            if g is None:
                continue
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.to(torch.float32).contiguous()
            keep.append(g)
            readers.setdefault((a, i), []).append(g)
        rows = [(a, i) for a, shape in enumerate(shapes) for i in range(shape[0])]
        lib = _C.load_library()
        with torch.cuda.device(dev):
            for lo in range(0, len(rows), 64):
                part = rows[lo:lo + 64]
                items = (gsr_multi_add_item * len(part))()
                for it, (a, i) in zip(items, part):
                    srcs = readers.get((a, i), [])
                    if len(srcs) > 4:                     # (more readers than a launch item carries: fold the rest first)
                        extra = srcs[3]
                        for g in srcs[4:]:
                            extra = extra + g
                        keep.append(extra)
                        srcs = srcs[:3] + [extra]
                    it.dst, it.count = outs[a][i].data_ptr(), int(outs[a][i].numel())
                    for k in range(4):
                        it.src[k] = srcs[k].data_ptr() if k < len(srcs) else None
                lib.gsr_multi_add(len(part), items, _C._stream(dev))
        return (None,) + tuple(outs)


def fan_out(stacked, plan):
    """Rows of stacked tensors for SEVERAL readers each: returns [stacked[a][i] for (a, i) in plan] (the same row may appear many times) as one
    autograd node whose backward pass adds the readers' gradients of all rows in one launch and hands back whole stacked gradients -- instead
    of an unbind per tensor, a pairwise addition per extra reader and a re-stacking (32 + 3 launches of tiny kernels per dynamic mapping
    iteration, slam/dynamic_graph.py). stacked: fp32 device tensors [S, ...]; rows nobody reads get zero gradients."""
    for t in stacked:
        _C._require_device(t, "stacked")
    return list(_FanOut.apply(tuple((int(a), int(i)) for a, i in plan), *[t.contiguous() for t in stacked]))


class IndexSets:
    """S index sets idx [S, E] (int64, values in [0, Nv)) together with their reverse lists (gsr_index_csr): what gather_rows needs to
    run its backward pass as an ORDERED segment sum. Build it once per index array, use it for every gather through that array."""

    def __init__(self, idx, n_targets):
        _C._require_device(idx, "idx")
        if idx.dtype != torch.int64 or idx.dim() != 2:
            raise ValueError("IndexSets: idx must be an int64 [S, E] device tensor")
        self.idx = idx.contiguous()
        self.S, self.E, self.Nv = int(idx.shape[0]), int(idx.shape[1]), int(n_targets)
        lib = _C.load_library()
        self.csr = torch.empty((int(lib.gsr_index_csr_workspace_size(self.S, self.E, self.Nv)),), dtype=torch.uint8, device=idx.device)
        with torch.cuda.device(idx.device):
            lib.gsr_index_csr(self.S, self.E, self.Nv, self.idx.data_ptr(), self.csr.data_ptr(), _C._stream(idx.device))


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, sets, set_of_b):
        # table [B, Nv, C]; out[b, e, :] = table[b, idx[set_of_b[b], e], :]
        B, Nv, Cn = table.shape
        idx = sets.idx if set_of_b is None else sets.idx.index_select(0, getattr(set_of_b, "_gsr_long", None) if hasattr(set_of_b, "_gsr_long") else set_of_b.long())
        idx = idx if idx.shape[0] == B else idx.expand(B, -1)
        ctx.sets, ctx.set_of_b, ctx.shape = sets, set_of_b, (B, Nv, Cn)
        return torch.gather(table, 1, idx[:, :, None].expand(-1, -1, Cn))

    @staticmethod
    def backward(ctx, g):
        sets, (B, Nv, Cn) = ctx.sets, ctx.shape
        g = g.to(torch.float32).contiguous()
        out = torch.empty((B, Nv, Cn), dtype=torch.float32, device=g.device)
        lib = _C.load_library()
        sob = None if ctx.set_of_b is None else ctx.set_of_b.to(torch.int32).contiguous()
        with torch.cuda.device(g.device):
            lib.gsr_segment_sum(B, sets.S, sets.E, Cn, Nv, g.data_ptr(), sets.csr.data_ptr(), None if sob is None else sob.data_ptr(), out.data_ptr(),
                                _C._stream(g.device))
        return out, None, None


def gather_rows(table, sets: IndexSets, set_of_b=None):
    """out[b, e, :] = table[b, idx[s, e], :] with s = set_of_b[b] (int tensor [B]; None: the one set, or one set per batch element when
    S == B) -- torch.gather's values, but a BACKWARD pass that adds the incoming rows of a target in a fixed order (gsr_segment_sum) instead of
    torch's scatter_add with float atomics: bit-reproducible gradients. table [B, Nv, C] fp32 on the device."""
    if table.dim() != 3 or table.shape[1] != sets.Nv:
        raise ValueError(f"gather_rows: table {tuple(table.shape)} does not match the index sets ({sets.Nv} targets)")
    if set_of_b is None and sets.S not in (1, table.shape[0]):
        raise ValueError("gather_rows: give set_of_b when the number of index sets is neither 1 nor the batch size")
    if set_of_b is None and sets.S == table.shape[0] and sets.S > 1:
        set_of_b = torch.arange(sets.S, device=table.device, dtype=torch.int32)
    return _GatherRows.apply(table, sets, set_of_b)


def node_embedding(nodes, times, n_freq_x, n_freq_t):
    """[n * M, 3 (1 + 2 Fx) + 1 + 2 Ft]: the node network's input for every (time sample, node) pair in one launch (gsr_node_embedding,
    include/control_nodes.h). nodes [M, 3] and times [n] fp32 on the device; no gradient (node positions are detached, times are data)."""
    _C._require_device(nodes, "nodes")
    nodes, times = _f32(nodes, "nodes"), _f32(times.reshape(-1), "times")
    if nodes.dim() != 2 or nodes.shape[1] < 3:
        raise ValueError(f"node_embedding expects nodes [M, >=3], got {tuple(nodes.shape)}")
    n, M = int(times.shape[0]), int(nodes.shape[0])
    out = torch.empty((n * M, 3 * (1 + 2 * n_freq_x) + 1 + 2 * n_freq_t), dtype=torch.float32, device=nodes.device)
    lib = _C.load_library()
    ws = torch.empty((int(lib.gsr_node_embedding_workspace_size(n, M, int(n_freq_x), int(n_freq_t))),), dtype=torch.uint8, device=nodes.device)
    with torch.cuda.device(nodes.device):
        lib.gsr_node_embedding(n, M, int(n_freq_x), int(n_freq_t), nodes.data_ptr(), int(nodes.shape[1]), times.data_ptr(), out.data_ptr(), ws.data_ptr(),
                               _C._stream(nodes.device))
    return out


RELU_BIAS_COLS = (64, 128, 256, 512, 1024)


def relu_backward_bias(dY, Y):
    """(G, dbias) of a layer y = relu(x W^T + b): G = dY * (Y > 0) and dbias = G.sum(0), in one pass over dY and Y (gsr_relu_backward_bias,
    include/control_nodes.h) with the column sums formed in a fixed order. dY, Y [rows, cols] fp32 on the device, cols in RELU_BIAS_COLS."""
    _C._require_device(dY, "dY")
    if dY.dim() != 2 or dY.shape != Y.shape or dY.dtype != torch.float32 or Y.dtype != torch.float32 or int(dY.shape[1]) not in RELU_BIAS_COLS:
        raise ValueError(f"relu_backward_bias expects two fp32 [rows, cols] tensors with cols in {RELU_BIAS_COLS}, got {tuple(dY.shape)} and {tuple(Y.shape)}")
    dY, Y = dY.contiguous(), Y.contiguous()
    rows, cols = int(dY.shape[0]), int(dY.shape[1])
    G = torch.empty_like(dY)
    db = torch.empty((cols,), dtype=torch.float32, device=dY.device)
    lib = _C.load_library()
    ws = torch.empty((max(16, int(lib.gsr_relu_backward_bias_workspace_size(rows, cols))),), dtype=torch.uint8, device=dY.device)
    with torch.cuda.device(dY.device):
        lib.gsr_relu_backward_bias(rows, cols, dY.data_ptr(), Y.data_ptr(), G.data_ptr(), db.data_ptr(), ws.data_ptr(), _C._stream(dY.device))
    return G, db


def quaternion_to_matrix(q):
    """utils/time_utils.py:115-133: real part first; the 2 / |q|^2 factor normalises."""
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


RADIUS_IS_LOG, WEIGHT_IS_LOGIT = GSR_NODE_RADIUS_IS_LOG, GSR_NODE_WEIGHT_IS_LOGIT
# the node attributes of a blend, and their first columns in the packed layout's one [B, m, 14] matrix
_ATTRS = (("node_trans", 3), ("node_rot", 4), ("node_scale", 3), ("local_rotation", 4))
ATTR_COLS = (0, 3, 7, 10)


def _flat(t):
    return None if t is None else t.reshape(-1)


def _blend_inputs(layout, x, motion_mask, nodes, node_radius, node_weight, attrs):
    """The inputs of a blend as contiguous fp32 device tensors with their shapes checked: (shared, attrs, n, m, B). layout "single": attrs
    are node_trans [m, 3], node_rot [m, 4], node_scale [m, 3], local_rotation [m, 4] | None, or nothing at all (weights only); "batch": the
    same four with a leading axis B; "packed": one matrix [B, m, 14]."""
    x, nodes = _f32(x, "x"), _f32(nodes, "nodes")
    if x.dim() != 2 or x.shape[1] != 3 or nodes.dim() != 2 or nodes.shape[1] < 3:
        raise ValueError(f"node blend expects x [N, 3] and nodes [M, >=3], got {tuple(x.shape)} and {tuple(nodes.shape)}")
    n, m = x.shape[0], nodes.shape[0]
    motion_mask = None if motion_mask is None else _f32(motion_mask, "motion_mask")
    if motion_mask is not None and motion_mask.numel() != n:
        raise ValueError(f"motion_mask must have one value per Gaussian ({n}), got {tuple(motion_mask.shape)}")
    node_radius = _f32(node_radius, "node_radius").reshape(-1)
    node_weight = None if node_weight is None else _f32(node_weight, "node_weight").reshape(-1)
    if node_radius.numel() != m or (node_weight is not None and node_weight.numel() != m):
        raise ValueError("node_radius / node_weight must have one value per node")
    if not attrs or attrs[0] is None:                     # weights only
        attrs = [None] * len(attrs)
    lead = ()
    if layout != "single":
        if attrs[0] is None or attrs[0].dim() != 3:
            raise ValueError(f"node blend ({layout}) expects node attributes [B, M, .], got {getattr(attrs[0], 'shape', None)}")
        lead = (attrs[0].shape[0],)
    spec = (("attrs", 14),) if layout == "packed" else _ATTRS
    attrs = [None if t is None else _f32(t, name, (*lead, m, c)) for t, (name, c) in zip(attrs, spec)]
    shared = dict(x=x, motion_mask=motion_mask, nodes=nodes, node_radius=node_radius, node_weight=node_weight)
    return shared, attrs, n, m, (lead[0] if lead else 1)


def _attr_ptrs(tensors, packed):
    """Where the four attributes (or their gradients) start: column ranges of the one matrix, or the four tensors' own (None: absent)."""
    if packed:
        return [tensors[0].data_ptr() + 4 * c for c in ATTR_COLS]
    return [t.data_ptr() if t is not None else None for t in tensors] + [None] * (4 - len(tensors))


def _descriptor(scalars, shared, attrs):
    """gsr_node_blend of a call, for its forward and its backward stage (the tensors behind the pointers: `shared` and `attrs`, kept by the caller)."""
    a = gsr_node_blend(**scalars)
    for k, t in shared.items():
        setattr(a, k, t.data_ptr() if t is not None else None)
    a.node_trans, a.node_rot, a.node_scale, a.node_local_rotation = _attr_ptrs(attrs, scalars["attr_stride"] != 0)
    return a


class _NodeBlend(torch.autograd.Function):
    """The SC-GS node blend for every layout of the node attributes (see _blend_inputs). "single": one blend, outputs (nn_weight, nn_dist, nn_idx,
    d_xyz, d_rotation, d_scaling). "batch" / "packed": B blends of the same Gaussians and nodes with B sets of attributes in one launch per stage
    -- the views and flow partners of one mapping iteration --, outputs d_xyz [B, n, 3], d_rotation [B, n, 4], d_scaling [B, n, 3]; packed: the
    node network's heads as its single head layer produces them (gsr_node_blend.attr_stride / grad_stride), no per-attribute copies on the way in
    and one [B, m, 14] gradient on the way out. Gradients to node_radius, node_weight and the attributes; x and nodes are constants of the op
    (detached in the reference)."""

    @staticmethod
    def forward(ctx, layout, x, motion_mask, nodes, node_radius, node_weight, K, rot_as_residual, raw, *attrs):
        if not 1 <= K <= BLEND_MAX_K:
            raise ValueError(f"node blend: K = {K} outside 1..{BLEND_MAX_K}")
        flags = (RADIUS_IS_LOG | WEIGHT_IS_LOGIT) if raw else 0
        ctx.n_attrs, ctx.glue_args, glue = len(attrs), None, _C._glue
        ctx.set_materialize_grads(False)
        if layout == "single" and glue is not None and hasattr(glue, "node_blend_forward"):      # native host glue (csrc/torch_glue.cpp): ~10x less host time
            _C._require_device(x, "x")
            det = lambda t: None if t is None else t.detach()
            trans, rot, scale, local = attrs or (None,) * 4
            ctx.glue_args = (x.detach(), det(motion_mask), nodes.detach(), node_radius.detach(), det(node_weight), det(trans), det(rot), det(scale),
                             det(local) if trans is not None else None, int(K), bool(rot_as_residual), flags)
            try:
                w, dist, idx, *outs = glue.node_blend_forward(*ctx.glue_args, _C._stream(x.device))
            except RuntimeError as e:
                raise ValueError(str(e)) from e
        else:
            shared, attrs, n, m, B = _blend_inputs(layout, x, motion_mask, nodes, node_radius, node_weight, attrs)
            packed, blend = layout == "packed", bool(attrs) and attrs[0] is not None
            scalars = dict(n=n, m=m, K=K, local_frame=int(packed or (blend and attrs[3] is not None)), rot_as_residual=int(bool(rot_as_residual)),
                           node_stride=shared["nodes"].shape[1], flags=flags, attr_stride=14 if packed else 0, grad_stride=14 if packed else 0)
            a = _descriptor(scalars, shared, attrs)
            dev, lead = shared["x"].device, () if layout == "single" else (B,)
            w = torch.empty((n, K), dtype=torch.float32, device=dev)
            dist = torch.empty((n, K), dtype=torch.float32, device=dev)
            idx = torch.empty((n, K), dtype=torch.int64, device=dev)
            outs = [torch.empty((*lead, n, c) if blend else (0, c), dtype=torch.float32, device=dev) for c in (3, 4, 3)]
            with torch.cuda.device(dev):
                _C.load_library().gsr_node_blend_forward_batch(ctypes.byref(a), B, w.data_ptr(), dist.data_ptr(), idx.data_ptr(),
                                                               *([o.data_ptr() for o in outs] if blend else (None, None, None)), _C._stream(dev))
            ctx.call = a, shared, attrs, B                # (shared and attrs: the tensors the descriptor points to)
        # (w, dist, idx are OUTPUTS: kept through save_for_backward -- as plain attributes of ctx they form a reference cycle output ->
        # grad_fn -> ctx -> output that only the cyclic collector breaks, and the whole upstream graph, the network's AccumulateGrad
        # nodes included, lingers until then)
        ctx.save_for_backward(w, dist, idx)
        if layout != "single":                            # (B sets of attributes share one nn_weight: the library takes its cotangent for a single blend only)
            return tuple(outs)
        ctx.mark_non_differentiable(dist, idx)
        return (w, dist, idx, *outs)

    @staticmethod
    def backward(ctx, *grads):
        g_w, (g_xyz, g_rot, g_scale) = grads[0] if len(grads) == 6 else None, grads[-3:]
        w, dist, idx = ctx.saved_tensors
        dev = w.device
        cot = lambda g: None if g is None or not g.numel() else g.to(torch.float32).contiguous()
        cots = [cot(g) for g in (g_xyz, g_rot, g_scale, g_w)]
        if ctx.glue_args is not None:
            g_radius, g_weight, *g_attrs = _C._glue.node_blend_backward(*ctx.glue_args, w, dist, idx, cots[3], *cots[:3], _C._stream(dev))
        else:
            a, shared, attrs, B = ctx.call
            n, m = a.n, a.m
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
            rows = (B, m) if B > 1 else (m,)
            g_radius, g_weight = new(*rows), new(*rows) if shared["node_weight"] is not None else None
            g_attrs = [None if t is None else new(*t.shape) for t in attrs]
            lib = _C.load_library()
            ws = torch.empty((lib.gsr_node_blend_workspace_size_batch(n, m, B),), dtype=torch.uint8, device=dev)
            p = lambda t: t.data_ptr() if t is not None else None
            with torch.cuda.device(dev):
                lib.gsr_node_blend_backward_batch(ctypes.byref(a), B, w.data_ptr(), dist.data_ptr(), idx.data_ptr(), *[p(g) for g in cots],
                                                  *_attr_ptrs(g_attrs, a.grad_stride != 0), p(g_radius), p(g_weight), ws.data_ptr(), _C._stream(dev))
            if B > 1:                                     # radius / weight are shared by the B blends: their gradient is the sum of the rows
                g_radius, g_weight = g_radius.sum(0), None if g_weight is None else g_weight.sum(0)
        # inputs: layout, x, motion_mask, nodes, node_radius, node_weight, K, residual, raw, *attrs
        return (None, None, None, None, g_radius, g_weight, None, None, None, *g_attrs[:ctx.n_attrs])


def cal_nn_weight(x, nodes, node_radius, node_weight=None, K: int = 3, raw: bool = True):
    """ControlNodeWarp.cal_nn_weight (:981-1011, gs_kernel=True).  raw=True (default): node_radius / node_weight are the module's RAW
    parameters _node_radius [M] / _node_weight [M, 1] and exp / sigmoid (:893-898) happen in the kernel; raw=False: they are the
    activated properties.  node_weight None: with_node_weight False.  Returns (nn_weight [N, K], nn_dist [N, K], nn_idx [N, K] int64)
    with gradients to node_radius / node_weight."""
    return _NodeBlend.apply("single", x, None, nodes, node_radius.reshape(-1), _flat(node_weight), K, True, raw)[:3]


def node_blend(x, motion_mask, nodes, node_radius, node_weight, node_trans, node_rot, node_scale, local_rotation=None, K: int = 3,
               d_rot_as_res: bool = True, raw: bool = True):
    """The body of ControlNodeWarp.forward (:1199-1258) after node_deform: blends the K nearest nodes' predictions
    node_trans = node_attrs['d_xyz'], node_rot = node_attrs['d_rotation'], node_scale = node_attrs['d_scaling'].
    local_rotation [M, 4] (node_attrs['local_rotation'], :1207) selects the local-frame translation; None = the global one.
    raw: see cal_nn_weight.  Returns {'d_xyz', 'd_rotation', 'd_scaling', 'nn_weight', 'nn_dist', 'nn_idx'}."""
    w, dist, idx, d_xyz, d_rot, d_scale = _NodeBlend.apply("single", x, motion_mask, nodes, node_radius.reshape(-1), _flat(node_weight), K, d_rot_as_res,
                                                           raw, node_trans, node_rot, node_scale, local_rotation)
    return {"d_xyz": d_xyz, "d_rotation": d_rot, "d_scaling": d_scale, "nn_weight": w, "nn_dist": dist, "nn_idx": idx}


def node_blend_batch(x, motion_mask, nodes, node_radius, node_weight, node_trans, node_rot, node_scale, local_rotation=None, K: int = 3,
                     d_rot_as_res: bool = True, raw: bool = True):
    """node_blend for B sets of node attributes at once: node_trans [B, M, 3], node_rot [B, M, 4], node_scale [B, M, 3], local_rotation
    [B, M, 4] | None -> (d_xyz [B, N, 3], d_rotation [B, N, 4], d_scaling [B, N, 3]). Values and gradients are those of B node_blend calls
    (the radius / weight gradients are their sum)."""
    return _NodeBlend.apply("batch", x, motion_mask, nodes, node_radius.reshape(-1), _flat(node_weight), K, d_rot_as_res, raw, node_trans, node_rot,
                            node_scale, local_rotation)


def node_blend_batch_packed(x, motion_mask, nodes, node_radius, node_weight, attrs, K: int = 3, d_rot_as_res: bool = True, raw: bool = True):
    """node_blend_batch (local frame) with the node attributes as one matrix attrs [B, M, 14] = [d_xyz | d_rotation | d_scaling |
    local_rotation]: same values and gradients, no copies of the four column ranges and one gradient matrix."""
    return _NodeBlend.apply("packed", x, motion_mask, nodes, node_radius.reshape(-1), _flat(node_weight), K, d_rot_as_res, raw, attrs)
