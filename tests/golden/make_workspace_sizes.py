#!/usr/bin/env python
"""What every workspace size query of the C ABI returns over a small table of arguments: workspace_sizes.json.

The file was written by running this script at the commit BEFORE the layouts of gs_capi.hip moved into one layout function each (one Carver);
tests/test_workspace_sizes.py holds the library of the current tree against it: no query may return more than it did then, the sizes that
tests and headers pin return exactly the same, and none drops to 0. The size queries are host functions: no GPU is needed.

Per query the table holds zero and invalid arguments, one element, one below / at / above each rounding boundary of its regions (256 bytes,
or 16 for the workspaces whose entry point receives a byte count) and one production size.

  python tests/golden/make_workspace_sizes.py      (re)writes tests/golden/workspace_sizes.json from the library of this checkout
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "4dgs-slam_amd"))
from diff_gaussian_rasterization import _C, _abi  # noqa: E402

# queries whose value a test or a header pins: they must not change at all
EXACT = ("gsr_track_workspace_size", "gsr_mono_keyframe_depth_workspace_size", "gsr_lpips_workspace_size", "gsr_relu_backward_bias_workspace_size",
         "gsr_stereo_workspace_size", "gsr_flow_rigid_fit_workspace_size", "gsr_motion_mask_clean_workspace_size")

_SIZES = [0, -1, 1, 63, 64, 65, 4352, 100000]
_FRAMES = [(0, 1), (-1, 5), (1, 1), (15, 1), (16, 1), (17, 1), (17, 9), (17, 16), (640, 480)]
_ITEMS = [(24, 20), (256, 64)]
_FIELD = [[8, 8, 8, 4]]                                           # a HexPlane field: per level (rx, ry, rz, rt)
_FIELD2 = [[64, 64, 64, 25], [128, 128, 128, 50]]

# query -> argument lists (plain JSON values; `call` below turns the structured ones into ctypes)
TABLE = {
    "gsr_ssim_workspace_size": [(0, 0, 0), (0, 9, 3), (-1, 9, 3), (1, 1, 1), (17, 9, 3), (144, 112, 1), (128, 128, 1), (208, 80, 1), (640, 480, 3)],
    "gsr_dense_chain_workspace_size": [(0, 256, 1), (33, 0, 1), (33, 256, 0), (33, 256, -1), (1, 1, 1), (1, 256, 1), (32, 256, 8), (33, 256, 8),
                                       (64, 256, 8), (33, 63, 2), (33, 64, 2), (33, 65, 2), (65, 63, 3), (33, 256, 9), (200000, 256, 8)],
    "gsr_dense_wgrad_workspace_size": [(0, 24, 20), (70, 0, 20), (70, 24, 0), (-5, 3, 3), (1, 1, 1), (70, 24, 20), (70, 8, 8), (128, 64, 1),
                                       (129, 64, 1), (200000, 256, 64)],
    "gsr_dense_wgrad_many_workspace_size": [(70, _ITEMS), (0, _ITEMS), (-1, _ITEMS), (70, []), (1, [(1, 1)]), (70, [(24, 20)] * 13),
                                            (70, [(0, 4)]), (200000, [(256, 64), (256, 256), (64, 256)])],
    "gsr_node_blend_workspace_size": [(0, 1), (1, 1), (65, 0), (65, 3), (127, 3), (128, 3), (129, 3), (100000, 512)],
    "gsr_node_blend_workspace_size_batch": [(65, 3, 0), (65, 3, -1), (0, 3, 1), (1, 1, 1), (65, 3, 1), (65, 3, 2), (16, 3, 1), (128, 600, 2),
                                            (1000, 512, 12), (100000, 512, 4)],
    "gsr_index_csr_workspace_size": [(0, 0, 0), (1, 0, 1), (1, 1, 1), (2, 37, 5), (1, 511, 4), (1, 512, 4), (1, 513, 4), (63, 10, 3), (64, 10, 3),
                                     (65, 10, 3), (7, 5120, 512), (1, 10240, 512), (1, 10241, 512), (1, 400000, 512)],
    "gsr_seed_workspace_size": [(n,) for n in _SIZES],
    "gsr_knn_workspace_size": [(n,) for n in _SIZES],
    "gsr_track_workspace_size": _FRAMES,
    "gsr_mono_keyframe_depth_workspace_size": [(0, 0), (-1, 4), (1, 1), (3, 5), (480, 640)],
    "gsr_yolo_workspace_size": [(a,) for a in (0, -1, 1, 15, 16, 17, 63, 64, 65, 8192, 8193)],
    "gsr_views_scratch_size": [(0, 65, 4, 3), (-1, 65, 4, 3), (3, 0, 4, 3), (1, 1, 1, 3), (1, 63, 1, 3), (1, 64, 1, 3), (1, 65, 1, 3), (3, 65, 4, 3),
                               (2, 65, 1, 1), (12, 100000, 4, 3)],
    "gsr_jpeg_workspace_size": [(0, 16, 16), (1, 0, 16), (1, 1, 1), (1, 16, 16), (1, 17, 16), (3, 17, 9), (3, 640, 480), (1, 65536, 16)],
    "gsr_stereo_workspace_size": [(0, 1, 64), (1, 1, 64), (17, 9, 64), (17, 9, 128), (17, 9, 32), (640, 480, 128)],
    "gsr_flow_rigid_fit_workspace_size": _FRAMES,
    "gsr_motion_mask_clean_workspace_size": _FRAMES,
    # (field levels or None, feat_dim, channels_last, n, "hex_ordered"); the views query: + V
    "gsr_hexplane_backward_workspace_size": [(None, 32, 1, 65, 0)] + [(_FIELD, 32, cl, n, o) for o in (0, 1) for cl, n in
                                                                        ((0, 65), (1, 0), (1, 1), (1, 63), (1, 64), (1, 65))] +
                                            [(_FIELD2, 32, 1, 20000, 0), (_FIELD2, 32, 1, 20000, 1), ([[2048, 8, 8, 4]], 32, 1, 65, 0)],
    "gsr_hexplane_backward_views_workspace_size": [(_FIELD, 32, 1, n, o, v) for o in (0, 1) for n, v in ((0, 2), (1, 1), (64, 2), (65, 3))] +
                                                  [(_FIELD2, 32, 1, 20000, 1, 4)],
    # not carved by the host (one region at the caller's base), listed because tests pin them exactly: (batch, [(c, h, w), ...]); (rows, cols)
    "gsr_lpips_workspace_size": [(0, [(64, 17, 9)]), (1, []), (1, [(64, 17, 9), (128, 8, 4)]), (2, [(64, 64, 64), (192, 31, 31), (384, 15, 15)])],
    "gsr_relu_backward_bias_workspace_size": [(0, 256), (1, 64), (64, 256), (65, 256), (50000, 256)],
}


def _field(levels, feat_dim, channels_last):
    if levels is None:
        return None
    f = _abi.gsr_hexplane_field(num_levels=len(levels), feat_dim=feat_dim, channels_last=channels_last)
    for lv, res in zip(f.levels, levels):
        lv.res[:] = res
    return ctypes.byref(f)


def call(lib, query, args):
    """The query's value for one row of TABLE."""
    fn = getattr(lib, query)
    if query == "gsr_dense_wgrad_many_workspace_size":
        M, items = args
        arr = (_abi.gsr_dense_wgrad_item * max(len(items), 1))(*[_abi.gsr_dense_wgrad_item(ldg=n, ldx=k, lddw=k, N=n, K=k) for n, k in items])
        return int(fn(M, len(items), arr))
    if query == "gsr_lpips_workspace_size":
        batch, levels = args
        chw = (ctypes.c_int * max(3 * len(levels), 1))(*[v for lv in levels for v in lv])
        return int(fn(batch, len(levels), chw))
    if query.startswith("gsr_hexplane"):
        levels, feat_dim, channels_last, n, ordered = args[:5]
        before = lib.gsr_set_option(b"hex_ordered", ordered)
        try:
            return int(fn(_field(levels, feat_dim, channels_last), n, *args[5:]))
        finally:
            lib.gsr_set_option(b"hex_ordered", before)
    return int(fn(*args))


def rows(lib):
    return [{"query": q, "args": json.loads(json.dumps(a)), "bytes": call(lib, q, a)} for q, table in TABLE.items() for a in table]


if __name__ == "__main__":
    out = os.path.join(HERE, "workspace_sizes.json")
    with open(out, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows(_C.load_library())) + "\n]\n")
    print("wrote", out)
