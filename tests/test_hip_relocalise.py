"""The relocaliser on the device (include/relocalisation.h, csrc/gs_reloc.h, slam/relocalise.py): the three kernels bit for bit against the
numpy restatement (tests/reloc_reference.py) at edge sizes and inputs, determinism, guard bytes, refusals; then end to end on the synthetic
sequence: localisation in a saved map, refusals, a run with the option on that loses nothing, a kidnapped run, and lost-then-found."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import reloc_reference as ref  # noqa: E402
from slam import relocalise  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
ENCODE_SHAPES = [(8, 8, 8, 8, 8), (33, 21, 5, 4, 24), (320, 240, 40, 30, 512), (161, 97, 40, 30, 1000)]


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _words(a):
    """uint32 numpy -> int32 device tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint32).view(np.int32)).cuda()


def _guarded(n, dtype=torch.int32):
    """(the whole buffer, its first n entries): four guard entries follow the output"""
    buf = torch.full((n + 4,), GUARD, dtype=dtype, device="cuda")
    return buf, buf[:n]


def _guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


# ---- encode -------------------------------------------------------------------------------------------------------------------------------
def _frame(W, H, seed, kind):
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    depth = rng.uniform(0.3, 6.0, (H, W)).astype(np.float32)
    mask = None
    flat = depth.reshape(-1)
    if kind != "clean":
        for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -1.0, 65.535, 70.0, 3e38, 0.0004)):       # past the clamp: d * 1000 >= 65535
            flat[(7 * k + 3) % flat.size::max(1, flat.size // 5)] = v
    if kind == "no_depth":
        depth = None
    if kind == "masked":
        mask = (rng.uniform(size=(H, W)) < 0.8).astype(np.uint8)
        mask[:H // 2, W // 3:] = 0                                                                     # whole cells without a pixel
    if kind == "bool_mask":
        mask = rng.uniform(size=(H, W)) < 0.5
    if kind == "wild_image":
        wild = image.reshape(-1)
        wild[::7], wild[3::11], wild[5::13], wild[1::17], wild[2::19] = -0.25, 1.5, np.nan, np.inf, -np.inf
    return image, depth, mask


def _table(F, grid_w, grid_h, seed, wild_cells=False):
    table = relocalise.fern_table(F, grid_w, grid_h, seed, 0.3, 6.0, 1000.0)
    if wild_cells:                                                                                     # the modulo: negative and far out of range
        rng = np.random.default_rng(seed + 1)
        table[:, 0] = rng.integers(-2 ** 31, 2 ** 31, size=F)
        table[0, 0], table[1, 0], table[2, 0] = -1, -2 ** 31, 2 ** 31 - 1
    return table


def _encode(image, depth, mask, grid_w, grid_h, table, depth_scale=1000.0):
    F = table.shape[0]
    buf, code = _guarded(F // 8)
    relocalise.encode(_dev(image), _dev(depth), _dev(mask), (grid_w, grid_h), _dev(table), depth_scale, code)
    torch.cuda.synchronize()
    assert _guard_ok(buf, F // 8)
    return code.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", ["depth", "no_depth", "masked", "bool_mask", "wild_image", "wild_cells"])
@pytest.mark.parametrize("W,H,grid_w,grid_h,F", ENCODE_SHAPES)
def test_encode_equals_the_restatement_bit_for_bit(W, H, grid_w, grid_h, F, kind):
    image, depth, mask = _frame(W, H, W + H, kind)
    table = _table(F, grid_w, grid_h, F, wild_cells=kind == "wild_cells")
    want = ref.encode(image, depth, mask, grid_w, grid_h, table, 1000.0)
    got = _encode(image, depth, mask, grid_w, grid_h, table)
    assert got.tobytes() == want.tobytes()
    nibbles = ref.unpack(want)
    assert (nibbles != 0).any() and (nibbles != 15).any()               # the case says something: bits of both values
    if depth is None:
        assert (nibbles & 8 == 0).all()
    again = _encode(image, depth, mask, grid_w, grid_h, table)
    assert again.tobytes() == got.tobytes()


@pytest.mark.parametrize("W,H,grid_w,grid_h,F", ENCODE_SHAPES)
def test_encode_of_a_constant_image_turns_exactly_at_its_value(W, H, grid_w, grid_h, F):
    k = 100
    image = np.full((3, H, W), k / 255, np.float32)
    depth = np.full((H, W), 1.5, np.float32)                             # dq = 1500 everywhere
    table = _table(F, grid_w, grid_h, 5)
    for t, bit in ((k - 1, 1), (k, 0), (k + 1, 0)):                      # S = k n: S > (k - 1) n, not S > k n
        table[:, 1:4] = t
        table[:, 4] = 1500 + (t - k)
        got = ref.unpack(_encode(image, depth, None, grid_w, grid_h, table))
        assert (got == (15 if bit else 0)).all()
        assert got.tolist() == ref.unpack(ref.encode(image, depth, None, grid_w, grid_h, table, 1000.0)).tolist()


# ---- search -------------------------------------------------------------------------------------------------------------------------------
def _database(K, F, seed):
    """Random codes with few distinct distances (many ties), duplicates of row 0 among them; the query is row 0 with two ferns changed."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 16, size=F)
    nibbles = np.tile(base, (K, 1))
    change = rng.uniform(size=(K, F)) < rng.uniform(0, 0.5, size=(K, 1))
    nibbles = np.where(change, rng.integers(0, 16, size=(K, F)), nibbles)
    if K > 2:
        nibbles[K // 2] = nibbles[0]
        nibbles[K - 1] = nibbles[0]
    query = base.copy()
    query[:2] ^= 5
    db = np.stack([ref.pack(r) for r in nibbles]) if K else np.zeros((0, F // 8), np.uint32)
    return db, ref.pack(query)


def _search(db, query, F, nibble_mask, topk, rows=None):
    K = db.shape[0] if rows is None else rows
    dbuf, distance = _guarded(K)
    bbuf, best = _guarded(2 * topk)
    best = best.view(topk, 2)
    relocalise.search(_words(db) if db.shape[0] else None, K, _words(query), F, nibble_mask, topk, distance if K else None, best)
    torch.cuda.synchronize()
    assert _guard_ok(dbuf, K) and _guard_ok(bbuf, 2 * topk)
    return distance.cpu().numpy(), best.cpu().numpy()


@pytest.mark.parametrize("F", [8, 24, 512])
def test_search_equals_the_restatement_with_ties_to_the_lower_index(F):
    for K in (0, 1, 2, 63, 64, 65, 1000):
        db, query = _database(K, F, K + F)
        for topk in (1, 4, 16):                                          # topk > K among them
            for nibble_mask in (0xF, 0x7):
                want_d, want_b = ref.search(db, query, nibble_mask, topk, F)
                got_d, got_b = _search(db, query, F, nibble_mask, topk)
                assert got_d.tobytes() == want_d.tobytes(), (K, topk, nibble_mask)
                assert got_b.tobytes() == want_b.tobytes(), (K, topk, nibble_mask, got_b, want_b)
                assert (got_b[K:] == [-1, F + 1]).all()
        if K > 2:                                                        # the duplicates of row 0, lower index first
            distance, best = _search(db, db[0], F, 0xF, 16)
            equal = [k for k in range(K) if distance[k] == 0]
            assert equal[0] == 0 and K // 2 in equal and K - 1 in equal and best[:len(equal), 0].tolist() == equal[:16]
            again = _search(db, query, F, 0xF, 16)
            assert again[0].tobytes() == ref.search(db, query, 0xF, 16, F)[0].tobytes()


def test_search_without_the_depth_bit_and_over_a_part_of_the_database():
    F = 24
    rng = np.random.default_rng(3)
    base = rng.integers(0, 8, size=F)
    db = np.stack([ref.pack(base | (rng.integers(0, 2, size=F) << 3)) for _ in range(5)] + [ref.pack(base ^ 1)])
    distance, best = _search(db, ref.pack(base), F, 0x7, 4)
    assert distance.tolist() == [0, 0, 0, 0, 0, F] and best.tolist() == [[0, 0], [1, 0], [2, 0], [3, 0]]
    distance, _ = _search(db, ref.pack(base | 8), F, 0x8, 1)             # the depth bit alone
    assert distance.tolist() == [int(((ref.unpack(r) & 8) == 0).sum()) for r in db]
    distance, best = _search(db, ref.pack(base ^ 1), F, 0xF, 2, rows=3)  # the first three rows only: row 5 is not looked at
    assert distance.shape == (3,) and (best[:, 0] < 3).all() and (best[:, 0] >= 0).all()


def test_encode_into_a_database_row_and_the_index():
    W, H, F = 161, 97, 1000
    index = relocalise.KeyframeIndex(F, (40, 30), 0, 0.3, 6.0, 1000.0, "cuda:0", capacity=2)
    frames = [_frame(W, H, s, "depth" if s % 2 else "clean") for s in range(5)]
    for s, (image, depth, mask) in enumerate(frames):
        index.add(100 + s, _dev(image), _dev(depth), None)                # grows twice: 2 -> 4 -> 8 rows
    assert len(index) == 5 and index.ids == [100, 101, 102, 103, 104] and index.database.shape[0] == 8
    torch.cuda.synchronize()
    rows = index.database[:5].cpu().numpy().view(np.uint32)
    for s, (image, depth, mask) in enumerate(frames):                    # straight into the row = encode, then copy
        assert rows[s].tobytes() == _encode(image, depth, None, 40, 30, index.table_host).tobytes()
    assert index.table_host.tobytes() == relocalise.fern_table(F, 40, 30, 0, 0.3, 6.0, 1000.0).tobytes()
    image, depth, _ = frames[3]
    best, distance = index.query(_dev(image), _dev(depth), None, 4)
    assert best.is_cuda and distance.is_cuda and best[0].tolist() == [3, 0]
    want_d, want_b = ref.search(rows, rows[3], 0xF, 4, F)
    assert best.cpu().numpy().tobytes() == want_b.tobytes() and distance.cpu().numpy().tobytes() == want_d.tobytes()
    best, _ = index.query(_dev(image), None, None, 2)                    # a frame without depth is compared on its colour bits
    assert best[0].tolist() == [3, 0]
    index.clear()
    assert len(index) == 0
    best, distance = index.query(_dev(image), _dev(depth), None, 3)
    assert best.tolist() == [[-1, F + 1]] * 3 and distance.numel() == 0


# ---- score --------------------------------------------------------------------------------------------------------------------------------
def _score_case(W, H, seed):
    rng = np.random.default_rng(seed)
    image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    q = np.round(image * 255)
    step = rng.integers(-12, 13, size=(3, H, W))                           # |dR| + |dG| + |dB| spreads around tau = 16: many exactly at it
    render = (np.clip(q + step, 0, 255) / 255).astype(np.float32)
    image = (q / 255).astype(np.float32)
    opacity = rng.uniform(0, 1, (H, W)).astype(np.float32)
    opacity.reshape(-1)[::5] = 0.5                                         # exactly 0.5: not considered
    opacity.reshape(-1)[1::9] = np.nan
    depth = rng.uniform(0.3, 6.0, (H, W)).astype(np.float32)
    rdepth = (depth * rng.uniform(0.9, 1.1, (H, W))).astype(np.float32)
    rdepth.reshape(-1)[2::7] = (depth.reshape(-1)[2::7] * np.float32(1.05)).astype(np.float32)        # near tau_depth = 0.05 from either side
    rdepth.reshape(-1)[3::31] = np.nan
    for k, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -2.0)):
        depth.reshape(-1)[(4 + k)::23] = v
    mask = (rng.uniform(size=(H, W)) < 0.7).astype(np.uint8)
    image[:, 0, 2], render[:, 0, 2] = np.float32(100 / 255), (np.array([116, 100, 100]) / 255).astype(np.float32)       # one pixel exactly at 16 for sure
    opacity[0, 2], mask[0, 2] = 0.9, 1
    return render, rdepth, opacity, image, depth, mask


def _score(render, rdepth, opacity, image, depth, mask, tau_colour, tau_depth):
    buf, counts = _guarded(8)
    relocalise.score_counts(_dev(render), _dev(rdepth), _dev(opacity), _dev(image), _dev(depth), _dev(mask), tau_colour, tau_depth, counts)
    torch.cuda.synchronize()
    assert _guard_ok(buf, 8)
    return counts.cpu().numpy()


@pytest.mark.parametrize("with_depth,with_mask", [(True, True), (False, True), (True, False), (False, False)])
@pytest.mark.parametrize("W,H", [(8, 8), (33, 21), (320, 240)])
def test_score_equals_the_restatement(W, H, with_depth, with_mask):
    render, rdepth, opacity, image, depth, mask = _score_case(W, H, W)
    depth, mask = depth if with_depth else None, mask if with_mask else None
    for tau_colour, tau_depth in ((16, 0.05), (0, 0.0), (765, 10.0)):
        want = ref.score(render, rdepth, opacity, image, depth, mask, tau_colour, tau_depth)
        got = _score(render, rdepth, opacity, image, depth, mask, tau_colour, tau_depth)
        assert got.tolist() == want.tolist(), (tau_colour, tau_depth)
        assert _score(render, rdepth, opacity, image, depth, mask, tau_colour, tau_depth).tobytes() == got.tobytes()
    want = ref.score(render, rdepth, opacity, image, depth, mask, 16, 0.05)
    assert want[0] == (W * H if mask is None else int(mask.sum())) and 0 < want[2] < want[1] < want[0] and (want[5:] == 0).all()
    if with_depth:
        assert 0 < want[4] < want[3] < want[1]
        exact = ref.score(render, rdepth, opacity, image, depth, mask, 15, 0.05)
        assert exact[2] < want[2]                                          # pixels exactly at tau_colour = 16 exist and count
    else:
        assert want[3] == want[4] == 0


def test_score_through_a_render_package_applies_the_exposure():
    import types
    W, H = 33, 21
    render, rdepth, opacity, image, depth, mask = _score_case(W, H, 9)
    pkg = {"render": _dev(render), "depth": _dev(rdepth)[None], "opacity": _dev(opacity)[None]}
    frame = types.SimpleNamespace(original_image=_dev(image), depth_device=lambda: _dev(depth), exposure_a=None, exposure_b=None)
    got = relocalise.score(pkg, frame, 16, 0.05, _dev(mask))
    assert got.is_cuda and got.tolist() == ref.score(render, rdepth, opacity, image, depth, mask, 16, 0.05).tolist()
    frame.exposure_a, frame.exposure_b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    assert relocalise.score(pkg, frame, 16, 0.05, _dev(mask)).tolist() == got.tolist()                # a = b = 0 changes no value
    frame.exposure_a, frame.exposure_b = torch.tensor([0.1], device="cuda"), torch.tensor([-0.02], device="cuda")
    exposed = (torch.exp(frame.exposure_a) * pkg["render"] + frame.exposure_b).cpu().numpy()
    want = ref.score(exposed, rdepth, opacity, image, depth, mask, 16, 0.05)
    assert relocalise.score(pkg, frame, 16, 0.05, _dev(mask)).tolist() == want.tolist() and want[2] != got[2].item()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_with_text_and_touch_nothing():
    W, H, gw, gh, F = 33, 21, 5, 4, 24
    image, depth, mask = _frame(W, H, 1, "masked")
    table = _dev(_table(F, gw, gh, 0))
    need = relocalise.encode_workspace_size(gw, gh)
    assert need >= gw * gh * 6 * 4 and relocalise.encode_workspace_size(0, 4) == 0 and relocalise.encode_workspace_size(64, 65) == 0
    assert relocalise.encode_workspace_size(64, 64) > 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    code = torch.full((F // 8,), GUARD, dtype=torch.int32, device="cuda")
    enc = lambda **kw: relocalise.encode(kw.get("image", _dev(image)), _dev(depth), _dev(mask), kw.get("grid", (gw, gh)), kw.get("table", table),
                                         kw.get("depth_scale", 1000.0), kw.get("code", code), kw.get("workspace", ws))
    with pytest.raises(RuntimeError, match="gsr_reloc_encode: workspace must be 16-byte aligned and hold %d bytes \\(gsr_reloc_encode_workspace_size\\)" % need):
        enc(workspace=ws[:need - 16])
    for grid in ((0, 4), (5, 0), (34, 4), (5, 22)):
        with pytest.raises(RuntimeError, match="gsr_reloc_encode: 1 <= grid_w <= width, 1 <= grid_h <= height and grid_w \\* grid_h <= 4096"):
            enc(grid=grid, workspace=torch.full((1 << 17,), 0x5A, dtype=torch.uint8, device="cuda"))
    big = torch.zeros((3, 80, 80), device="cuda")
    with pytest.raises(RuntimeError, match="grid_w \\* grid_h <= 4096"):
        relocalise.encode(big, None, None, (80, 52), table, 1000.0, code, torch.zeros(1 << 17, dtype=torch.uint8, device="cuda"))
    for bad_F in (0, 4, 2056):
        with pytest.raises(RuntimeError, match="gsr_reloc_encode: ferns must be a multiple of 8 in \\[8, 2048\\], got %d" % bad_F):
            enc(table=torch.zeros((bad_F, 5), dtype=torch.int32, device="cuda"), code=torch.full((bad_F // 8,), GUARD, dtype=torch.int32, device="cuda"))
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="gsr_reloc_encode: depth_scale must be positive and finite"):
            enc(depth_scale=scale)
    lib = relocalise._C.load_library()
    with pytest.raises(RuntimeError, match="gsr_reloc_encode: width and height must be at least 1 and width \\* height below 2\\^23"):
        lib.gsr_reloc_encode(4096, 2048, _dev(image).data_ptr(), None, None, gw, gh, F, table.data_ptr(), 1000.0, code.data_ptr(), ws.data_ptr(), need, None)
    with pytest.raises(RuntimeError, match="gsr_reloc_encode: image, fern_table, code and workspace must not be NULL"):
        lib.gsr_reloc_encode(W, H, None, None, None, gw, gh, F, table.data_ptr(), 1000.0, code.data_ptr(), ws.data_ptr(), need, None)
    with pytest.raises(RuntimeError, match="depth must be a contiguous float32 device tensor of shape \\(21, 33\\)"):
        relocalise.encode(_dev(image), _dev(depth).double(), None, (gw, gh), table, 1000.0, code, ws)
    torch.cuda.synchronize()
    assert bool((code == GUARD).all()) and bool((ws == 0x5A).all())
    enc()                                                                                              # exactly enough
    torch.cuda.synchronize()
    assert code.cpu().numpy().view(np.uint32).tobytes() == ref.encode(image, depth, mask, gw, gh, table.cpu().numpy(), 1000.0).tobytes()

    db, query = _database(5, F, 0)
    distance = torch.full((5,), GUARD, dtype=torch.int32, device="cuda")
    best = torch.full((4, 2), GUARD, dtype=torch.int32, device="cuda")
    call = lambda rows=5, ferns=F, nibble_mask=0xF, topk=4, database=_words(db): lib.gsr_reloc_search(
        rows, ferns, None if database is None else database.data_ptr(), _words(query).data_ptr(), nibble_mask, topk, distance.data_ptr(), best.data_ptr(), None)
    for kw, text in ((dict(rows=-1), "rows must be in \\[0, 2\\^20\\], got -1"), (dict(rows=(1 << 20) + 1), "rows must be in \\[0, 2\\^20\\]"),
                     (dict(ferns=12), "ferns must be a multiple of 8 in \\[8, 2048\\], got 12"), (dict(ferns=4096), "ferns must be a multiple of 8"),
                     (dict(nibble_mask=0), "nibble_mask must be in \\[1, 15\\], got 0"), (dict(nibble_mask=16), "nibble_mask must be in \\[1, 15\\]"),
                     (dict(topk=0), "topk must be in \\[1, 16\\], got 0"), (dict(topk=17), "topk must be in \\[1, 16\\], got 17"),
                     (dict(database=None), "database, query and distance must not be NULL when rows > 0")):
        with pytest.raises(RuntimeError, match="gsr_reloc_search: " + text):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((distance == GUARD).all()) and bool((best == GUARD).all())

    render, rdepth, opacity, image, depth, mask = _score_case(W, H, 2)
    counts = torch.full((8,), GUARD, dtype=torch.int32, device="cuda")
    for tau_colour, tau_depth, text in ((-1, 0.05, "tau_colour must be in \\[0, 765\\], got -1"), (766, 0.05, "tau_colour must be in \\[0, 765\\], got 766"),
                                        (48, -0.1, "tau_depth must be finite and not negative"), (48, float("nan"), "tau_depth must be finite"),
                                        (48, float("inf"), "tau_depth must be finite")):
        with pytest.raises(RuntimeError, match="gsr_reloc_score: " + text):
            relocalise.score_counts(_dev(render), _dev(rdepth), _dev(opacity), _dev(image), _dev(depth), _dev(mask), tau_colour, tau_depth, counts)
    with pytest.raises(RuntimeError, match="gsr_reloc_score: render, render_depth, opacity, image and counts must not be NULL"):
        lib.gsr_reloc_score(W, H, _dev(render).data_ptr(), None, _dev(opacity).data_ptr(), _dev(image).data_ptr(), None, None, 48, 0.05, counts.data_ptr(), None)
    with pytest.raises(RuntimeError, match="gsr_reloc_score: width and height must be at least 1"):
        lib.gsr_reloc_score(0, H, _dev(render).data_ptr(), _dev(rdepth).data_ptr(), _dev(opacity).data_ptr(), _dev(image).data_ptr(), None, None, 48, 0.05,
                            counts.data_ptr(), None)
    with pytest.raises(RuntimeError, match="opacity must be a contiguous float32 device tensor of shape \\(21, 33\\)"):
        relocalise.score_counts(_dev(render), _dev(rdepth), _dev(opacity)[None], _dev(image), None, None, 48, 0.05, counts)
    torch.cuda.synchronize()
    assert bool((counts == GUARD).all())


# ---- end to end on the synthetic sequence --------------------------------------------------------------------------------------------------
# ATE as the project reports it (slam/eval_utils.py ate_rmse): the RMSE of the camera centres' distances after ONE rigid fit of the estimate
# onto the ground truth. The fit is made over `fit` (for a run: all of its frames, the fit eval_ate(final=True) makes) and the error is taken
# over `ids`, a stretch of them: a fit over the ten frames after a jump alone would fit most of a wrong pose away, and no fit at all would
# measure the run's constant offset (35 - 50 mm here, the same before and after the jump) instead of what the jump did.
# the synthetic demo's dataset and options at its small size (tools/run_slam_demo.py, static_*_graph)
FRAMES, WIDTH, HEIGHT = 40, 320, 240
TRAINING = {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": 60, "static_map_iters": 30,
            "gaussian_update_every": 60, "gaussian_update_offset": 20, "tracking_graph": True}
FAR_R, FAR_T = torch.eye(3), torch.tensor([5.0, -4.0, 6.0])                 # a start pose metres away from the room


def _slam(dataset, training_addition):
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    cfg = merge_config(default_config(), {"Training": TRAINING, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 150}, "Results": {"eval_rendering": False}})
    cfg = merge_config(cfg, {"Training": training_addition})
    slam = SLAM(cfg, dataset)
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    return slam.run(), slam


def _centre(R, T):
    return (-R.detach().double().cpu().numpy().T @ T.detach().double().cpu().numpy())


def _ate(cameras, ids, poses=None, fit=None):
    """RMSE over `ids` after the rigid fit over `fit` (default: `ids`); poses {id: (R, T)} overrides the cameras' estimates."""
    from slam.eval_utils import align
    fit = list(ids) if fit is None else list(fit)
    est = lambda i: _centre(*(poses[i] if poses is not None else (cameras[i].R, cameras[i].T)))
    gt = lambda i: _centre(cameras[i].R_gt, cameras[i].T_gt)
    rot, trans, _ = align(np.stack([est(i) for i in fit]).T, np.stack([gt(i) for i in fit]).T)
    err = [np.linalg.norm(rot @ est(i) + trans[:, 0] - gt(i)) for i in ids]
    return float(np.sqrt(np.mean(np.square(err))))


class Replay:
    """A dataset that replays frames of another in a given order; None in the order is a frame of uniform noise (image and depth)."""

    def __init__(self, base, order):
        self.base, self.order, self.num_imgs = base, list(order), len(order)
        self._noise = torch.Generator(device="cpu").manual_seed(11)

    def __len__(self):
        return self.num_imgs

    def __getattr__(self, name):
        return getattr(self.base, name)

    def __getitem__(self, i):
        k = self.order[i]
        if k is not None:
            return self.base[k]
        _, depth, pose, motion = self.base[0]
        image = torch.rand((3, self.base.height, self.base.width), generator=self._noise).to(self.base.device)
        noise_depth = (0.3 + 5.7 * torch.rand((self.base.height, self.base.width), generator=self._noise)).numpy()
        return image, noise_depth.astype(np.asarray(depth).dtype), pose, motion


def _dataset(**more):
    from slam.dataset import SyntheticRGBDDataset
    return SyntheticRGBDDataset(num_frames=FRAMES, width=WIDTH, height=HEIGHT, seed=0, **more)


@pytest.fixture(scope="module")
def plain_run():
    """The one plain run (option absent) of the module: (result, slam, dataset)."""
    ds = _dataset()
    result, slam = _slam(ds, {})
    return result, slam, ds


@pytest.fixture(scope="module")
def localiser(plain_run, tmp_path_factory):
    from slam.map_io import load_map
    _, slam, ds = plain_run
    directory = str(tmp_path_factory.mktemp("reloc") / "map")
    slam.save_map(directory)
    before = {k: v.detach().clone() for k, v in (("xyz", slam.gaussians.get_xyz), ("opacity", slam.gaussians._opacity))}
    loaded = load_map(directory)
    return relocalise.MapLocaliser(loaded, slam.config), loaded, before


def test_end_to_end_every_frame_is_found_again_in_the_saved_map(plain_run, localiser):
    _, slam, ds = plain_run
    loc, loaded, _ = localiser
    cameras, keyframes = slam.frontend.cameras, set(slam.frontend.kf_indices)
    others = [i for i in sorted(cameras) if i not in keyframes]
    assert len(loc.index) == len(keyframes) and len(others) >= 20
    poses, found = {}, []
    for i in others:
        viewpoint = loc.camera(ds, i)
        viewpoint.update_RT(FAR_R, FAR_T)
        out = loc.localise(viewpoint)
        found.append(out)
        poses[i] = (viewpoint.R.detach().clone(), viewpoint.T.detach().clone())
    run_ate, loc_ate = _ate(cameras, others), _ate(cameras, others, poses)
    tried = [o["candidates_tried"] for o in found]
    print(f"saved map: {len(others)} non-keyframes, accepted {sum(o['accepted'] for o in found)}, candidates tried {np.bincount(tried).tolist()}, "
          f"ATE of the run {run_ate * 1000:.2f} mm, of the localised poses {loc_ate * 1000:.2f} mm, ratio {loc_ate / run_ate:.2f}")
    # measured on an MI355X: 32 of 32 accepted, each at its first candidate; ATE of the run's own poses over these frames 3.35 mm, of the
    # localised poses 0.88 mm (ratio 0.26; without any fit 21.79 and 21.55 mm). The bar: at most twice the run's own, for a different start
    # pose under the same optimiser and the same convergence test.
    assert all(o["accepted"] for o in found)
    assert all(o["keyframe"] in keyframes and o["distance"] is not None and len(o["counts"]) == 8 for o in found)
    assert loc_ate <= 2.0 * run_ate


def test_end_to_end_noise_and_black_frames_are_refused_and_keep_their_pose(plain_run, localiser):
    _, slam, ds = plain_run
    loc, loaded, before = localiser
    viewpoint = loc.camera(Replay(ds, [None] + list(range(1, FRAMES))), 0)
    black = loc.camera(ds, 3)
    black.original_image = torch.zeros_like(black.original_image)
    black.depth, black._depth_dev = np.zeros_like(black.depth), None
    black.compute_grad_mask(loc.config)
    for frame in (viewpoint, black):
        frame.update_RT(FAR_R, FAR_T)
        out = loc.localise(frame)
        print("refused:", out)
        assert out["accepted"] is False and out["keyframe"] is None and out["candidates_tried"] >= 1
        assert torch.equal(frame.R.cpu(), FAR_R) and torch.equal(frame.T.cpu(), FAR_T)
    assert torch.equal(loaded.gaussians.get_xyz, before["xyz"]) and torch.equal(loaded.gaussians._opacity, before["opacity"])     # the map is not touched


def test_end_to_end_a_dynamic_map_is_refused():
    import types
    fake = types.SimpleNamespace(dynamic=True)
    with pytest.raises(ValueError, match="the map is dynamic"):
        relocalise.MapLocaliser(fake)


def test_end_to_end_follow_tracks_a_stretch_of_the_sequence(plain_run, localiser):
    _, slam, ds = plain_run
    loc, _, _ = localiser
    out = loc.follow(ds, list(range(10, 16)))
    print("follow:", out["status"], "ATE", out["ate_rmse"])
    assert out["status"][0] == "localised" and all(s in ("tracked", "relocalised") for s in out["status"][1:])
    assert tuple(out["poses"].shape) == (6, 4, 4) and out["ate_rmse"] is not None and out["ate_rmse"] < 0.05


def test_end_to_end_the_option_on_changes_no_pose_when_nothing_is_lost(plain_run):
    off, slam_off, _ = plain_run
    on, slam_on = _slam(_dataset(), {"relocalisation": {"enabled": True}})
    events = [e[0] for e in slam_on.frontend.log]
    print("option on:", on["relocalisation"], "keyframes", on["keyframes"])
    assert "relocalisation" not in off and slam_off.frontend.relocalisation is None
    assert "lost" not in events and "relocalised" not in events
    assert on["keyframes"] == off["keyframes"] and on["relocalisation"]["scored"] == FRAMES - 1
    assert on["relocalisation"]["lost"] == on["relocalisation"]["relocalised"] == 0 and on["relocalisation"]["device_ms_per_score"] > 0.0        # measured: 0.15 ms
    assert len(slam_on.frontend.relocalisation.index) == len(on["keyframes"])
    for i in sorted(slam_off.frontend.cameras):
        a, b = slam_off.frontend.cameras[i], slam_on.frontend.cameras[i]
        assert torch.equal(a.R, b.R) and torch.equal(a.T, b.T), i


# the kidnapped sequence: frames 0 .. 24, then the camera is back at frame 5 and goes on to 14
KIDNAP = dict(step=0.02, rot_step=0.012)
JUMP_AT, ORDER = 25, list(range(25)) + list(range(5, 15))


@pytest.fixture(scope="module")
def kidnapped_off():
    ds = Replay(_dataset(**KIDNAP), ORDER)
    return _slam(ds, {})


def test_end_to_end_a_kidnapped_camera_is_found_again(kidnapped_off):
    off, slam_off = kidnapped_off
    on, slam_on = _slam(Replay(_dataset(**KIDNAP), ORDER), {"relocalisation": {"enabled": True}})
    before, after = list(range(1, JUMP_AT)), list(range(JUMP_AT, len(ORDER)))
    every = list(range(len(ORDER)))
    off_after = _ate(slam_off.frontend.cameras, after, fit=every)
    on_before, on_after = _ate(slam_on.frontend.cameras, before, fit=every), _ate(slam_on.frontend.cameras, after, fit=every)
    events = [e for e in slam_on.frontend.log if e[0] in ("lost", "relocalised")]
    print(f"kidnapped: off post-jump {off_after * 1000:.1f} mm; on pre-jump {on_before * 1000:.2f} mm, post-jump {on_after * 1000:.2f} mm; "
          f"off / on {off_after / on_after:.1f}; events {events}; {on['relocalisation']}")
    # measured on an MI355X: option off, post-jump 136.0 mm; option on, pre-jump 9.11 mm, post-jump 4.97 mm; off / on 27.4. (Without any fit:
    # 182.2, 47.96, 49.51 mm and 3.7 -- each run's constant offset is in both figures; 26 other step / rot_step pairs gave 1.3 to 4.9.)
    assert [e[:2] for e in events] == [("relocalised", JUMP_AT)]
    assert on_after <= 2.0 * on_before
    assert off_after >= 5.0 * on_after


def test_end_to_end_lost_on_noise_then_found():
    order = ORDER[:JUMP_AT] + [None, None] + ORDER[JUMP_AT:]
    on, slam_on = _slam(Replay(_dataset(**KIDNAP), order), {"relocalisation": {"enabled": True}})
    fe = slam_on.frontend
    events = [e for e in fe.log if e[0] in ("lost", "relocalised")]
    print("lost, then found:", events, on["relocalisation"])
    assert [e[:2] for e in events] == [("lost", JUMP_AT), ("lost", JUMP_AT + 1), ("relocalised", JUMP_AT + 2)]
    for i in (JUMP_AT, JUMP_AT + 1):
        assert i not in fe.kf_indices and torch.equal(fe.cameras[i].R, fe.cameras[JUMP_AT - 1].R) and torch.equal(fe.cameras[i].T, fe.cameras[JUMP_AT - 1].T)
    after, found = list(range(JUMP_AT + 2, len(order))), [i for i in range(len(order)) if i not in (JUMP_AT, JUMP_AT + 1)]
    pre, post = _ate(fe.cameras, list(range(1, JUMP_AT)), fit=found), _ate(fe.cameras, after, fit=found)
    print(f"lost, then found: ATE before the jump {pre * 1000:.2f} mm, after the two lost frames {post * 1000:.2f} mm")
    assert post <= 2.0 * pre                                              # measured on an MI355X: 4.97 mm after, 9.11 mm before
    assert on["relocalisation"]["lost"] == 2 and on["relocalisation"]["relocalised"] == 1
