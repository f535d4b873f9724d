"""Host-side checks of the relocaliser (slam/relocalise.py, include/relocalisation.h): the numpy restatement of the three kernels
(tests/reloc_reference.py) on cases small enough to work out by hand, the fern table, the ``Training.relocalisation`` options and the
verdict. No GPU needed."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reloc_reference as ref  # noqa: E402
from slam import relocalise  # noqa: E402


# ---- the restatement, by hand -----------------------------------------------------------------------------------------------------------
def test_quantisation_by_hand():
    v = np.array([-1.0, 0.0, 0.5 / 255, 0.49 / 255, 100 / 255, 1.0, 7.0, np.nan, np.inf, -np.inf], np.float32)
    assert ref.quant(v).tolist() == [0, 0, 1, 0, 100, 255, 255, 0, 255, 0]
    assert [int(ref.quant(np.float32(k / 255))) for k in range(256)] == list(range(256))
    d = np.array([0.0, -1.0, np.nan, np.inf, -np.inf, 0.0004, 0.0005, 1.0, 65.5344, 65.535, 70.0, 3e38], np.float32)
    #                                     inf * scale >= 65535 clamps; 0.0004 * 1000 + 0.5 = 0.9 -> 0: invalid after all
    assert ref.depth_quant(d, None, 1000.0).tolist() == [0, 0, 0, 0, 0, 0, 1, 1000, 65534, 65535, 65535, 65535]
    assert ref.depth_quant(d, np.zeros(12, np.uint8), 1000.0).tolist() == [0] * 12
    assert relocalise.quantise_depth(0.3, 1000.0) == 300 and relocalise.quantise_depth(6.0, 1000.0) == 6000
    assert relocalise.quantise_depth(70.0, 1000.0) == 65535


def test_encode_on_a_four_by_four_frame_by_hand():
    # 4 x 4, a 2 x 2 grid: cell 0 is the upper left 2 x 2 block, cell 1 the upper right, cell 2 the lower left, cell 3 the lower right
    image = np.zeros((3, 4, 4), np.float32)
    image[0, :2, :2] = np.array([[10, 20], [30, 40]], np.float32) / 255          # cell 0: S_R = 100, n = 4
    image[1, :2, :2] = 25 / 255                                                  #         S_G = 100
    image[2, :2, :2] = 1.0                                                       #         S_B = 1020
    image[:, 2:, 2:] = 0.5                                                       # cell 3: masked out entirely below
    depth = np.zeros((4, 4), np.float32)
    depth[:2, :2] = [[1.0, 2.0], [np.nan, 0.0]]                                  # cell 0: S_D = 3000, n_D = 2
    mask = np.ones((4, 4), np.uint8)
    mask[2:, 2:] = 0
    sums = ref.cell_sums(image, depth, mask, 2, 2, 1000.0)
    assert sums.tolist() == [[100, 100, 1020, 4, 3000, 2], [0, 0, 0, 4, 0, 0], [0, 0, 0, 4, 0, 0], [0, 0, 0, 0, 0, 0]]
    table = np.array([[0, 25, 25, 25, 1500],         # S_R = 100 == 25 * 4: 0; S_G likewise: 0; S_B = 1020 > 100: 1; S_D = 3000 == 1500 * 2: 0
                      [0, 24, 24, 255, 1499],        # 100 > 96: 1, 1; 1020 == 255 * 4: 0; 3000 > 2998: 1
                      [3, 0, 0, 0, 0],               # the empty cell: every bit 0, although 0 > 0 * 0 is false anyway ...
                      [3, -1, -1, -1, -1],           # ... and 0 > -1 * 0 as well: n = 0 decides
                      [1, -1, 0, 0, 0],              # cell 1: n = 4, S = 0: 0 > -4: 1; 0 > 0: 0, 0; no depth: n_D = 0: 0
                      [4, 25, 25, 25, 1500],         # 4 % 4 = cell 0 again
                      [-1, 0, 0, 0, 0],              # (unsigned)-1 % 4 = 4294967295 % 4 = 3: the empty cell
                      [-3, 24, 24, 255, 1499]],      # (unsigned)-3 % 4 = 4294967293 % 4 = 1: sums 0 against positive thresholds: 0
                     np.int32)
    nibbles = ref.bits_from_sums(sums, table)
    assert nibbles.tolist() == [0b0100, 0b1011, 0, 0, 0b0001, 0b0100, 0, 0]
    code = ref.encode(image, depth, mask, 2, 2, table, 1000.0)
    assert code.dtype == np.uint32 and code.tolist() == [0x004100B4]
    assert ref.unpack(code).tolist() == nibbles.tolist()
    # no depth: every depth bit is 0, the others stay
    assert ref.unpack(ref.encode(image, None, mask, 2, 2, table, 1000.0)).tolist() == [0b0100, 0b0011, 0, 0, 0b0001, 0b0100, 0, 0]
    # S == t n gives 0, S == t n + 1 gives 1
    flat = np.full((3, 4, 4), 7 / 255, np.float32)
    one_more = flat.copy()
    one_more[0, 0, 0] = 8 / 255
    t = np.array([[0, 7, 7, 7, 0]] * 8, np.int32)
    assert ref.unpack(ref.encode(flat, None, None, 1, 1, t, 1.0))[0] == 0 and ref.unpack(ref.encode(one_more, None, None, 1, 1, t, 1.0))[0] == 0b0001


def test_cells_of_an_uneven_grid_cover_every_pixel_once():
    image = np.ones((3, 7, 10), np.float32)
    sums = ref.cell_sums(image, None, None, 3, 2, 1.0)
    # x: [0, 3) [3, 6) [6, 10); y: [0, 3) [3, 7)
    assert sums[:, 3].tolist() == [9, 9, 12, 12, 12, 16] and sums[:, 3].sum() == 70 and (sums[:, 0] == 255 * sums[:, 3]).all()


def test_search_by_hand_and_the_order_of_ties():
    F = 8
    query = ref.pack([1, 2, 3, 4, 5, 6, 7, 8])
    rows = [ref.pack([1, 2, 3, 4, 5, 6, 7, 8]),            # 0: equal
            ref.pack([0, 2, 3, 4, 5, 6, 7, 0]),            # 1: two ferns differ
            ref.pack([9, 10, 11, 12, 13, 14, 15, 0]),      # 2: the depth bit alone in seven ferns; fern 7 loses its depth bit too
            ref.pack([0, 2, 3, 4, 5, 6, 0, 8]),            # 3: two ferns differ: ties with row 1, comes after it
            ref.pack([1, 2, 3, 4, 5, 6, 7, 8])]            # 4: equal: ties with row 0, comes after it
    db = np.stack(rows)
    distance, best = ref.search(db, query, 0xF, 4, F)
    assert distance.tolist() == [0, 2, 8, 2, 0] and best.tolist() == [[0, 0], [4, 0], [1, 2], [3, 2]]
    distance, best = ref.search(db, query, 0x7, 16, F)
    assert distance.tolist() == [0, 1, 0, 2, 0]                      # row 1's fern 7 differs from the query's in the depth bit alone
    assert best.tolist() == [[0, 0], [2, 0], [4, 0], [1, 1], [3, 2]] + [[-1, 9]] * 11
    distance, best = ref.search(np.zeros((0, 1), np.uint32), query, 0xF, 2, F)
    assert distance.shape == (0,) and best.tolist() == [[-1, 9], [-1, 9]]


def test_score_by_hand():
    render = np.zeros((3, 2, 4), np.float32)
    image = np.zeros((3, 2, 4), np.float32)
    image[:, 0, 0] = [10 / 255, 10 / 255, 10 / 255]        # colour difference 30: exactly tau
    image[:, 0, 1] = [10 / 255, 10 / 255, 11 / 255]        # 31: one past it
    opacity = np.full((2, 4), 0.9, np.float32)
    opacity[0, 2] = 0.5                                    # exactly 0.5: not considered
    mask = np.ones((2, 4), np.uint8)
    mask[1, 3] = 0
    rdepth = np.full((2, 4), 2.0, np.float32)
    depth = np.array([[2.0, 2.2, 2.0, np.nan], [1.9, np.inf, 0.0, 2.0]], np.float32)
    # masked 7; considered 6 (0.5 is out); colour: all but (0, 1): 5; depth valid among the considered: (0,0) (0,1) (1,0): 3;
    # |2 - 2| <= 0.2: yes; |2 - 2.2| = 0.2 (float32: 0.20000005) <= 0.1 * 2.2: yes (0.22); |2 - 1.9| <= 0.19: yes
    assert ref.score(render, rdepth, opacity, image, depth, mask, 30, 0.1).tolist() == [7, 6, 5, 3, 3, 0, 0, 0]
    assert ref.score(render, rdepth, opacity, image, depth, mask, 30, 0.05).tolist() == [7, 6, 5, 3, 1, 0, 0, 0]
    assert ref.score(render, rdepth, opacity, image, None, None, 31, 0.05).tolist() == [8, 7, 7, 0, 0, 0, 0, 0]


# ---- the fern table -------------------------------------------------------------------------------------------------------------------------
def test_fern_table_is_reproducible_and_in_range():
    a = relocalise.fern_table(512, 40, 30, 0, 0.3, 6.0, 1000.0)
    b = relocalise.fern_table(512, 40, 30, 0, 0.3, 6.0, 1000.0)
    c = relocalise.fern_table(512, 40, 30, 1, 0.3, 6.0, 1000.0)
    assert a.dtype == np.int32 and a.shape == (512, 5) and a.tobytes() == b.tobytes() and a.tobytes() != c.tobytes()
    assert a[:, 0].min() >= 0 and a[:, 0].max() < 1200 and len(set(a[:, 0].tolist())) > 300
    assert a[:, 1:4].min() >= 32 and a[:, 1:4].max() < 224
    assert a[:, 4].min() >= 300 and a[:, 4].max() <= 6000
    small = relocalise.fern_table(8, 1, 1, 3, 1.0, 1.0, 1000.0)
    assert small.shape == (8, 5) and (small[:, 0] == 0).all() and (small[:, 4] == 1000).all()
    with pytest.raises(ValueError, match="must be in order"):
        relocalise.fern_table(8, 1, 1, 0, 2.0, 1.0, 1000.0)


# ---- options --------------------------------------------------------------------------------------------------------------------------------
def test_relocalisation_options_defaults_and_refusals():
    opts = relocalise.relocalisation_options
    assert opts({}) is None and opts({"relocalisation": {}}) is None and opts({"relocalisation": {"enabled": False, "ferns": 7}}) is None
    got = opts({"relocalisation": {"enabled": True}})
    assert got == {"enabled": True, "ferns": 512, "grid": [40, 30], "seed": 0, "topk": 4, "depth_scale": 1000.0, "depth_lo": 0.3, "depth_hi": 6.0,
                   "tau_colour": 48, "tau_depth": 0.05, "min_score": 0.72, "min_coverage": 0.5, "levels": 4, "iters": [5, 7, 10, 10],
                   "max_translation": 1.0, "max_rotation": 30.0}
    assert opts({"relocalisation": {"enabled": True, "levels": 2}})["iters"] == [5, 7]              # one count per level
    assert opts({"relocalisation": {"enabled": True, "levels": 2, "iters": [1, 2]}})["iters"] == [1, 2]
    assert relocalise.default_options(topk=2)["topk"] == 2
    for block, text in (({"fern": 8}, "unknown keys \\['fern'\\]"),
                        ({"ferns": 12}, "relocalisation.ferns must be a multiple of 8"),
                        ({"ferns": 0}, "relocalisation.ferns"),
                        ({"ferns": 4096}, "relocalisation.ferns"),
                        ({"grid": [100, 41]}, "relocalisation.grid .* at most 4096 cells"),
                        ({"grid": [0, 4]}, "relocalisation.grid"),
                        ({"grid": 40}, "relocalisation.grid"),
                        ({"topk": 0}, "relocalisation.topk must be 1 to 16"),
                        ({"topk": 17}, "relocalisation.topk must be 1 to 16"),
                        ({"iters": [5, 7, 10]}, "relocalisation.iters must hold 4 pass counts"),
                        ({"levels": 3, "iters": [5, 7, 10, 10]}, "relocalisation.iters must hold 3 pass counts"),
                        ({"iters": [5, 7, 10, 65]}, "relocalisation.iters"),
                        ({"levels": 7}, "relocalisation.levels"),
                        ({"tau_depth": math.nan}, "relocalisation.tau_depth must be a number"),
                        ({"min_score": math.nan}, "relocalisation.min_score must be a number"),
                        ({"min_coverage": math.nan}, "relocalisation.min_coverage must be a number"),
                        ({"tau_colour": math.nan}, "relocalisation.tau_colour must be an integer"),
                        ({"tau_colour": 766}, "relocalisation.tau_colour"),
                        ({"tau_depth": -0.1}, "relocalisation.tau_depth"),
                        ({"min_score": 1.5}, "relocalisation.min_score"),
                        ({"depth_scale": 0.0}, "relocalisation.depth_scale"),
                        ({"depth_scale": math.inf}, "relocalisation.depth_scale"),
                        ({"depth_lo": 6.0, "depth_hi": 0.3}, "depth_lo < depth_hi"),
                        ({"max_rotation": 181.0}, "relocalisation.max_rotation"),
                        ({"max_translation": -1.0}, "relocalisation.max_translation")):
        with pytest.raises(ValueError, match=text):
            opts({"relocalisation": dict({"enabled": True}, **block)})


def test_the_front_end_reads_the_block_once_and_is_inert_without_it():
    from slam.frontend import FrontEnd
    from slam.system import default_config, merge_config
    off = FrontEnd(default_config())
    assert off.relocalisation is None
    on = FrontEnd(merge_config(default_config(), {"Training": {"relocalisation": {"enabled": True, "topk": 2}}}))
    assert on.relocalisation.options["topk"] == 2 and on.relocalisation.index is None              # the index is built with the map, on the device
    assert on.relocalisation.summary() == {"scored": 0, "lost": 0, "relocalised": 0, "device_ms_per_score": 0.0}
    with pytest.raises(ValueError, match="relocalisation.topk"):
        FrontEnd(merge_config(default_config(), {"Training": {"relocalisation": {"enabled": True, "topk": 17}}}))


def test_a_front_end_whose_stage_has_started_is_freed_without_the_cycle_collector(monkeypatch):
    """The relocaliser is handed two calls into the front-end. A front-end that could only be freed by the cycle collector would have its
    streams, events and captured graphs destroyed whenever that next runs -- in the middle of a later run's graph capture, for instance."""
    import gc
    import weakref
    from slam import stages
    from slam.frontend import FrontEnd
    from slam.system import default_config, merge_config
    built = []
    monkeypatch.setattr(stages, "Relocaliser", lambda *args: built.append(args) or types.SimpleNamespace())
    monkeypatch.setattr(stages.KeyframeIndex, "from_options", lambda opt, device: types.SimpleNamespace(clear=lambda: None, add=lambda *a: None))
    frame = types.SimpleNamespace(R_gt=torch.eye(3), T_gt=torch.zeros(3), original_image=torch.ones(3, 2, 2), motion_mask=None, device="cpu",
                                  image_width=2, image_height=2, fx=1.0, fy=1.0, cx=1.0, cy=1.0, update_RT=lambda R, T: None,
                                  depth_device=lambda: torch.ones(2, 2))
    gc.disable()
    try:
        fe = FrontEnd(merge_config(default_config(), {"Training": {"relocalisation": {"enabled": True}}}))
        fe.device, fe.cameras[0] = "cpu", frame
        fe.backend = types.SimpleNamespace(handle_init=lambda *a: (None, None, {}, []))
        fe._render_at, fe._track_and_render = (lambda camera: ("rendered at", camera)), (lambda viewpoint: ("tracked", viewpoint))
        fe.initialize(0, frame)
        (index, cameras, render_at, track_from, size, K, options, log), = built
        assert cameras is fe.cameras and render_at(frame) == ("rendered at", frame) and track_from(frame) == ("tracked", frame)
        assert size == (2, 2) and K == (1.0, 1.0, 1.0, 1.0) and options is fe.relocalisation.options and log is fe.relocalisation.log
        gone = weakref.ref(fe)
        del fe
        assert gone() is None
    finally:
        gc.enable()


# ---- the verdict ----------------------------------------------------------------------------------------------------------------------------
def test_verdict_shares_and_every_zero_denominator():
    opt = relocalise.default_options(min_score=0.6, min_coverage=0.5)
    v = relocalise.verdict([100, 80, 60, 40, 30, 0, 0, 0], opt)
    assert v == {"accepted": True, "coverage": 0.8, "colour_share": 0.75, "depth_share": 0.75}
    assert relocalise.verdict([100, 50, 30, 40, 24, 0, 0, 0], opt)["accepted"]                          # each share exactly at its bar
    assert not relocalise.verdict([100, 49, 49, 40, 40, 0, 0, 0], opt)["accepted"]                      # coverage
    assert not relocalise.verdict([100, 80, 47, 40, 40, 0, 0, 0], opt)["accepted"]                      # colour
    assert not relocalise.verdict([100, 80, 80, 40, 23, 0, 0, 0], opt)["accepted"]                      # depth
    no_depth = relocalise.verdict([100, 80, 60, 0, 0, 0, 0, 0], opt)                                    # no depth to judge: colour decides
    assert no_depth["accepted"] and no_depth["depth_share"] is None
    nothing = relocalise.verdict([0, 0, 0, 0, 0, 0, 0, 0], opt)                                         # every pixel masked out
    assert nothing == {"accepted": False, "coverage": 0.0, "colour_share": 0.0, "depth_share": None}
    unseen = relocalise.verdict([100, 0, 0, 0, 0, 0, 0, 0], opt)                                        # the map covers no pixel
    assert unseen == {"accepted": False, "coverage": 0.0, "colour_share": 0.0, "depth_share": None}
    lenient = dict(opt, min_coverage=0.0, min_score=0.0)
    assert not relocalise.verdict([0, 0, 0, 0, 0, 0, 0, 0], lenient)["accepted"]                        # refused, never a division error
    assert not relocalise.verdict([100, 0, 0, 0, 0, 0, 0, 0], lenient)["accepted"]
    assert relocalise.verdict([100, 1, 0, 1, 0, 0, 0, 0], lenient)["accepted"]


# ---- judge and recover: the one path of a live run and of a saved map ---------------------------------------------------------------------------
ACCEPT, REFUSE = [100, 80, 80, 0, 0, 0, 0, 0], [100, 0, 0, 0, 0, 0, 0, 0]
NUDGE = 0.125                          # what the tracking double adds to the translation and to the exposure gain


class _Index:
    """Stands in for KeyframeIndex: three keyframes, a fixed answer, and a count of the queries."""
    device = "cpu"

    def __init__(self, best):
        self.ids, self.best, self.queries = [10, 20, 30], best, 0

    def query(self, image, depth=None, mask=None, topk=4):
        self.queries += 1
        return torch.tensor(self.best, dtype=torch.int32), None


class _Aligner:
    """Stands in for DenseOdometry: every alignment is refused, so a seeded pose is the candidate keyframe's."""

    def __init__(self, *args, **kwargs):
        pass

    def keep(self, image, depth=None, mask=None):
        pass

    def align(self, image, T_init=None):
        return torch.eye(4), None


def _frame(seed):
    g = torch.Generator().manual_seed(seed)
    cam = types.SimpleNamespace(R=torch.linalg.qr(torch.randn(3, 3, generator=g))[0], T=torch.randn(3, generator=g), original_image=torch.zeros(3, 2, 2),
                                exposure_a=torch.tensor([0.25]), exposure_b=torch.tensor([-0.5]), depth_device=lambda: None)
    cam.update_RT = lambda R, T: (setattr(cam, "R", R.clone()), setattr(cam, "T", T.clone()))
    return cam


def _judge(monkeypatch, verdicts, best, fallback_is_entry=False):
    """Relocaliser.judge of a tracked frame among doubles; the scores are `verdicts` in order. Returns (result, frame, what it was on entry,
    fallback pose, keyframes, index)."""
    from slam import odometry
    monkeypatch.setattr(odometry, "DenseOdometry", _Aligner)
    script = [torch.tensor(c, dtype=torch.int32) for c in verdicts]
    monkeypatch.setattr(relocalise, "score", lambda pkg, viewpoint, tau_colour, tau_depth, mask=None: script.pop(0))
    keyframes, index = {k: _frame(k) for k in (10, 20, 30)}, _Index(best)
    blank = {"render": torch.zeros(3, 2, 2), "depth": torch.ones(1, 2, 2), "opacity": torch.ones(1, 2, 2)}

    def track_from(viewpoint):
        viewpoint.update_RT(viewpoint.R, viewpoint.T + NUDGE)
        viewpoint.exposure_a += NUDGE
        return blank

    reloc = relocalise.Relocaliser(index, keyframes, lambda camera: blank, track_from, (2, 2), (1.0, 1.0, 1.0, 1.0), relocalise.default_options())
    frame = _frame(1)
    fallback = (frame.R.clone(), frame.T.clone()) if fallback_is_entry else (_frame(2).R, _frame(2).T)
    entry = tuple(t.clone() for t in (frame.R, frame.T, frame.exposure_a, frame.exposure_b))
    out = reloc.judge(frame, blank, fallback)
    assert not script                                                         # one score per verdict: nothing is judged twice or skipped
    return out, frame, entry, fallback, keyframes, index


def test_judge_accepts_a_tracked_frame_without_asking_the_index(monkeypatch):
    out, frame, entry, _, _, index = _judge(monkeypatch, [ACCEPT], [[0, 1], [-1, 9]])
    assert out["accepted"] and out["keyframe"] is None and out["candidates_tried"] == 0 and out["counts"] == ACCEPT
    assert index.queries == 0
    assert all(torch.equal(a, b) for a, b in zip((frame.R, frame.T, frame.exposure_a, frame.exposure_b), entry))     # it stays where tracking put it


def test_judge_finds_a_refused_frame_at_the_second_candidate(monkeypatch):
    out, frame, _, _, keyframes, index = _judge(monkeypatch, [REFUSE, REFUSE, ACCEPT], [[2, 3], [0, 5], [1, 7], [-1, 9]])
    assert out["accepted"] and out["keyframe"] == 10 and out["candidates_tried"] == 2 and out["distance"] == 5 and index.queries == 1
    # the pose is the second candidate's (row 0, keyframe 10), tracked once from there -- not the first candidate's, not the fallback
    assert torch.equal(frame.R, keyframes[10].R) and torch.equal(frame.T, keyframes[10].T + NUDGE)


@pytest.mark.parametrize("fallback_is_entry", [True, False])
def test_judge_leaves_a_frame_that_is_not_found_as_it_came(monkeypatch, fallback_is_entry):
    """Refused at the tracked pose and at both candidates: the frame has the fallback pose (here once the pose it came with, once another)
    and the exposure it came with, bit for bit, although the tracking double moved both at every candidate."""
    out, frame, entry, fallback, _, index = _judge(monkeypatch, [REFUSE, REFUSE, REFUSE], [[2, 3], [0, 5], [-1, 9], [-1, 9]], fallback_is_entry)
    assert not out["accepted"] and out["keyframe"] is None and out["candidates_tried"] == 2 and index.queries == 1
    assert torch.equal(frame.R, fallback[0]) and torch.equal(frame.T, fallback[1])
    assert torch.equal(frame.exposure_a, entry[2]) and torch.equal(frame.exposure_b, entry[3])
    if fallback_is_entry:
        assert torch.equal(frame.R, entry[0]) and torch.equal(frame.T, entry[1])
