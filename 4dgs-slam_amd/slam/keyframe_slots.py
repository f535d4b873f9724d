"""Keyframe slots of the graph-replayed iterations (slam/mapping_graph.py, dynamic_graph.py, tracking_graph.py) and the per-keyframe
operands they are filled from. A slot is a blank camera plus persistent ground-truth / loss-weight images; which keyframe a replay shows
in it is an index in device memory: ``gsr_slot_gather`` (include/slam_map.h) copies candidate ``index[s]`` of a device table of buffer
addresses -- nine per candidate, a ``gsr_keyframe_entry`` -- into the buffers of slot s, named by a host array of the same struct."""
import ctypes as C

import torch

from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization._abi import gsr_keyframe_entry
import slam_losses

from .camera import Camera


def device_store_budget(device, fraction, floor_bytes=256 << 20):
    """Bytes a per-keyframe store may hold on `device`: `fraction` of the memory that is free right now (never less than floor_bytes)."""
    try:
        free, _total = torch.cuda.mem_get_info(device)
    except Exception:
        return floor_bytes
    return max(int(free * fraction), floor_bytes)


class KeyframeOperands:
    """Per keyframe: the constant operands of its mapping loss (ground truth, weights), held so that their device addresses stay valid for
    the graphs that point at them (slam_losses keeps only a bounded cache).

    One entry per keyframe: the ground-truth image and depth ONCE, the loss weights per (rm_dynamic, dynamic) flag variant (a weight pair is
    2.4 MB at 640x480, the ground truth 4.9 MB -- three variants used to hold three copies of it once slam_losses' constants cache had
    evicted the keyframe). The store is bounded by BYTES -- BUDGET_FRACTION of the device memory free at its first use, least recently used
    keyframe first -- and follows Camera.clean() through slam_losses.drop_keyframe_constants. What is dropped is formed again on demand; a
    graph that still points at an entry's buffers holds the tensors itself."""

    BUDGET_FRACTION = 0.05

    def __init__(self):
        self._held = {}                 # id(viewpoint) -> [viewpoint, gt_image, gt_depth, {(rm_dynamic, dynamic): (w_rgb, w_depth, alpha)}, bytes]
        self._bytes, self._budget = 0, None
        slam_losses.on_drop_keyframe_constants(self.drop)

    @staticmethod
    def _nbytes(*tensors):
        return sum(t.numel() * t.element_size() for t in tensors if isinstance(t, torch.Tensor))

    def get(self, config, viewpoint, device, rm_dynamic=True, dynamic=False):
        """(gt_image, gt_depth, w_rgb, w_depth, alpha) of slam_losses.mapping_loss_operands, computed once per (keyframe, flags) and held:
        a keyframe's ground truth and masks never change. The eager loop's get_loss_mapping forms the same values."""
        flags = (bool(rm_dynamic), bool(dynamic))
        ent = self._held.get(id(viewpoint))
        if ent is not None and ent[0] is not viewpoint:     # the id was recycled by another object
            self.drop(ent[0])
            ent = None
        if ent is not None and flags in ent[3]:
            self._held[id(viewpoint)] = self._held.pop(id(viewpoint))           # (most recently used last)
            w = ent[3][flags]
            return ent[1], ent[2], w[0], w[1], w[2]
        gt_image, gt_depth, w_rgb, w_dep, alpha = slam_losses.mapping_loss_operands(config, viewpoint, device, rm_dynamic=rm_dynamic, dynamic=dynamic)
        if ent is None:
            ent = self._held[id(viewpoint)] = [viewpoint, gt_image, gt_depth, {}, self._nbytes(gt_image, gt_depth)]
            self._bytes += ent[4]
        else:
            self._held[id(viewpoint)] = self._held.pop(id(viewpoint))
        ent[3][flags] = (w_rgb, w_dep, alpha)
        extra = self._nbytes(w_rgb, w_dep)
        ent[4] += extra
        self._bytes += extra
        if self._budget is None:
            self._budget = device_store_budget(device, self.BUDGET_FRACTION)
        while self._bytes > self._budget and len(self._held) > 1:          # least recently used first, never the entry just returned
            oldest = next(iter(self._held))
            self._bytes -= self._held.pop(oldest)[4]
        return ent[1], ent[2], w_rgb, w_dep, alpha

    def drop(self, viewpoint=None):
        if viewpoint is None:
            self._held.clear()
            self._bytes = 0
        else:
            ent = self._held.pop(id(viewpoint), None)
            if ent is not None:
                self._bytes -= ent[4]

    def held_bytes(self):
        return self._bytes


class FlowTargets:
    """Per keyframe pair (a keyframe and the closest earlier one: the partner never changes) the constants of its two flow terms, per
    keyframe the tile rectangle of its moving pixels: ONE store for both bodies of BackEnd.map (the fixed layout's tables point at the
    tensors, the eager body reads slices of them). Bounded by count and by bytes, oldest first; what is dropped is formed again on demand
    from the dataset's cached flows; a running call holds what its tables point at."""

    BUDGET_FRACTION = 0.03      # at most this share of the device memory free when the first target is formed
    MAX_PAIRS = 512             # ~7 MB each at 640x480

    def __init__(self):
        self.targets, self.clips, self._budget = {}, {}, None          # (uid, partner's uid) -> [6, H, W]; uid -> int32 [4]

    def clear(self):
        self.targets, self.clips = {}, {}

    def get(self, dataset, v, other):
        """ONE [6, H, W] tensor: planes 0-1 the flow v -> other on v's moving pixels, 2 their mask, 3 the mask of `other`, 4-5 the flow
        other -> v on other's moving pixels (utils/slam_backend.py:486-488,:503-505 mask both sides of the difference by ~motion_mask; with a
        0 / 1 mask: the masked target minus the masked rendering). The plane order is the one gsr_slot_gather moves as (gt_image[3],
        gt_depth, w_rgb, w_depth); the operands of slam_losses.masked_l1 are the slices ``pair_operands`` names."""
        hit = self.targets.get((v.uid, other.uid))
        if hit is None:
            m1 = (~v.motion_mask).to(torch.float32)[None]
            m2 = (~other.motion_mask).to(torch.float32)[None]
            back = dataset.gt_flow(v.uid, other.uid)[0].permute(2, 0, 1) * m1
            fwd = dataset.gt_flow(other.uid, v.uid)[0].permute(2, 0, 1) * m2
            hit = torch.cat([back, m1, m2, fwd], 0).to(torch.float32).contiguous()
            if self._budget is None:
                self._budget = device_store_budget(hit.device, self.BUDGET_FRACTION)
            each = hit.numel() * hit.element_size()
            while self.targets and (len(self.targets) >= self.MAX_PAIRS or (len(self.targets) + 1) * each > self._budget):
                self.targets.pop(next(iter(self.targets)))
            self.targets[(v.uid, other.uid)] = hit
        return hit

    @staticmethod
    def pair_operands(f6):
        """(target, mask) of "this keyframe -> the earlier one", then of the way back."""
        return f6[0:2], f6[2:3], f6[4:6], f6[3:4]

    def clip(self, v):
        """The tile rectangle [x0, y0, x1, y1) (16-pixel tiles) around keyframe v's MOVING pixels -- all its flow loss reads of the flow image
        rendered from v -- as an int32 [4] device tensor (gsr_view.flow_clip); one host read per keyframe, kept."""
        hit = self.clips.get(v.uid)
        if hit is None:
            moving = ~v.motion_mask
            ys, xs = moving.any(dim=1).nonzero().flatten(), moving.any(dim=0).nonzero().flatten()
            rect = [0, 0, 0, 0] if ys.numel() == 0 else [int(xs[0]) // 16, int(ys[0]) // 16, int(xs[-1]) // 16 + 1, int(ys[-1]) // 16 + 1]
            while len(self.clips) >= 4 * self.MAX_PAIRS:
                self.clips.pop(next(iter(self.clips)))
            hit = self.clips[v.uid] = torch.tensor(rect, dtype=torch.int32).to(moving.device)
        return hit


def blank_camera(proto, uid, device):
    """A camera with the intrinsics of `proto` and nothing else: pose, matrices and exposure are written on the device."""
    return Camera(uid, None, None, torch.eye(4), proto.projection_matrix, proto.fx, proto.fy, proto.cx, proto.cy, proto.FoVx, proto.FoVy,
                  int(proto.image_height), int(proto.image_width), 0.0, None, device=device)


def slot_buffers(H, W, device):
    """(ground-truth image, ground-truth depth, rgb weights, depth weights) of one slot."""
    return tuple(torch.zeros((c, H, W), device=device) for c in (3, 1, 1, 1))


def entries(pairs):
    """The host array of destinations gsr_slot_gather takes, from (slot camera, its four image buffers) pairs; None without pairs."""
    rows = address_rows([cam for cam, _ in pairs], [ops for _, ops in pairs])
    return (gsr_keyframe_entry * len(rows))(*(gsr_keyframe_entry(*row) for row in rows)) if rows else None


def address_rows(cameras, planes):
    """Per camera the nine addresses of a gsr_keyframe_entry, in field order: matrices, centre, exposure, then its four image `planes`."""
    if any(t.dtype != torch.float32 or not t.is_contiguous() for ops in planes for t in ops):
        raise RuntimeError("keyframe slots: loss operands must be contiguous float32 tensors")
    return [[t.data_ptr() for t in (v.world_view_transform, v.full_proj_transform, v.camera_center, v.exposure_a, v.exposure_b, *ops)]
            for v, ops in zip(cameras, planes)]


def upload_rows(rows, dtype, device):
    """A host table into device memory through a pinned copy; None for an empty one."""
    return torch.tensor(rows, dtype=dtype).pin_memory().to(device, non_blocking=True) if rows else None


def gather(n_slots, table, index, dst, pixels, device):
    """Fill the slots `dst` (entries()) from the candidates index[0 .. n_slots) of the device `table` (address_rows, uploaded as int64)."""
    if n_slots:
        with torch.cuda.device(device):
            _C.load_library().gsr_slot_gather(n_slots, C.cast(table.data_ptr(), C.POINTER(gsr_keyframe_entry)), index.data_ptr(), dst, pixels,
                                              _C._stream(device))
