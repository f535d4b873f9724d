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
