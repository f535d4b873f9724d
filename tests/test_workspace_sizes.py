"""The workspace size queries against what they returned before each workspace got one layout function (tests/golden/workspace_sizes.json,
written by tests/golden/make_workspace_sizes.py at that commit): never larger, never down to 0, and unchanged where a test or a header pins
the value. Host code only: the library loads and answers size queries without a device."""
import importlib.util
import json
import os

import pytest

from diff_gaussian_rasterization import _C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_workspace_sizes", os.path.join(GOLDEN, "make_workspace_sizes.py"))
table = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(table)

with open(os.path.join(GOLDEN, "workspace_sizes.json")) as _fh:
    BEFORE = json.load(_fh)


def test_the_golden_file_covers_the_whole_table():
    assert [(r["query"], r["args"]) for r in BEFORE] == [(q, json.loads(json.dumps(a))) for q, rows in table.TABLE.items() for a in rows]


@pytest.mark.parametrize("query", list(table.TABLE))
def test_size_query_never_grows_and_pinned_sizes_stay_exact(query):
    lib = _C.load_library()
    for row in (r for r in BEFORE if r["query"] == query):
        now, before = table.call(lib, query, row["args"]), row["bytes"]
        print(query, row["args"], "before", before, "now", now)
        assert now <= before, (query, row["args"])
        assert now > 0 or before == 0, (query, row["args"])
        if query in table.EXACT:
            assert now == before, (query, row["args"])


def test_orientation_values_of_the_earlier_layouts():
    """The handful of values the layouts were read against by hand."""
    want = {("gsr_ssim_workspace_size", (17, 9, 3)): 5788, ("gsr_dense_chain_workspace_size", (33, 256, 8)): 18688,
            ("gsr_dense_wgrad_workspace_size", (70, 24, 20)): 2176, ("gsr_node_blend_workspace_size_batch", (65, 3, 1)): 25856,
            ("gsr_index_csr_workspace_size", (2, 37, 5)): 3328, ("gsr_seed_workspace_size", (65,)): 4372,
            ("gsr_track_workspace_size", (17, 16)): 4400, ("gsr_mono_keyframe_depth_workspace_size", (3, 5)): 2140,
            ("gsr_yolo_workspace_size", (65,)): 5392, ("gsr_yolo_workspace_size", (8193,)): 0, ("gsr_views_scratch_size", (3, 65, 4, 3)): 18964}
    have = {(r["query"], json.dumps(r["args"])): r["bytes"] for r in BEFORE}
    for (query, args), value in want.items():
        assert have[query, json.dumps(list(args))] == value, (query, args)
