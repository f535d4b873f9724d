"""The HIP post-processing of the YOLO segmenter (include/segmentation.h, csrc/gs_yolo.h) against the fp64 restatement of ultralytics'
decode, NMS and process_mask (tests/yolo_reference.py) on seeded head tensors with planted detections; YoloSeg's network (a seeded
stand-in of yolov9e-seg's topology, slam/yolo_stand_in.py) against the unfused reference; and the recorded dataset's motion masks with a
segmenter."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import segmentation as seg  # noqa: E402
import yolo_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STRIDES = [8.0, 16.0, 32.0]


def _grid(H, W):
    return [(H // 8, W // 8), (H // 16, W // 16), (H // 32, W // 32)]


def _heads(H, W, plants, seed=0, nc=80, nm=32):
    """Head tensors [64 + nc, h, w] / [nm, h, w] per level: background class logits -6 (never a candidate), random DFL logits and
    coefficients; each plant (level, y, x, class, class logit, (l, t, r, b) in cells) gets that class logit and near one-hot DFL bins,
    so its box is the anchor centre -+ (l, t, r, b) cells (IoUs of the planted layouts stay far from 0.7)."""
    g = torch.Generator().manual_seed(seed)
    heads = []
    for lh, lw in _grid(H, W):
        h = torch.randn((64 + nc, lh, lw), generator=g)
        h[64:] = -6.0
        heads.append([h, torch.randn((nm, lh, lw), generator=g)])
    for l, y, x, c, logit, ltrb in plants:
        h = heads[l][0]
        h[:64, y, x] = 0.0
        for k, d in enumerate(ltrb):
            h[k * 16 + d, y, x] = 12.0
        h[64 + c, y, x] = logit
    proto = torch.randn((nm, H // 4, W // 4), generator=g)
    return [(h.to(DEV).contiguous(), c.to(DEV).contiguous()) for h, c in heads], proto.to(DEV).contiguous()


def _plants_general(seed=1):
    """40 clusters of 1-4 anchors in a row (1-cell shifts: IoU 0.6 at d = 2, 0.85 at d = 6) in the lower half of the image, classes 0, 56
    and 3 (not requested); in the upper half, the same box in classes 0 and 56 (anchors 810 and 811: both survive, the class offset keeps
    them apart), and an anchor whose best class 3 is outside the set while its class 0 is above conf (anchor 5005: dropped)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(40):
        l = int(rng.integers(0, 3))
        lh, lw = _grid(480, 640)[l]
        y, x = int(rng.integers(lh // 2, lh)), int(rng.integers(0, lw - 4))
        c = int(rng.choice([0, 56, 3]))
        d = int(rng.choice([2, 6])) if l < 2 else 2
        for k in range(int(rng.integers(1, 5))):
            out.append((l, y, x + k, c, float(rng.uniform(-0.5, 4.0)), (d, d, d, d)))
    out.append((0, 10, 10, 0, 2.0, (6, 6, 6, 6)))
    out.append((0, 10, 11, 56, 2.5, (7, 6, 5, 6)))
    out.append((1, 5, 5, 3, 3.0, (2, 2, 2, 2)))
    out.append((1, 5, 5, 0, 1.0, (2, 2, 2, 2)))
    return out


def _by_anchor(rows):
    return {int(r[6]): r for r in rows.tolist()}


def _check_dets(res, heads, proto, classes, max_det=300):
    rrows, rcoef = ref.detections(heads, STRIDES, classes, max_det=max_det)
    n = int(res.counts[0])
    rows = res.dets[:n].double().cpu()
    assert n == len(rrows), (n, len(rrows))
    got, want = _by_anchor(rows[:, :7]), _by_anchor(rrows)
    assert set(got) == set(want)                                                   # the kept sets are identical
    for a, w in want.items():
        g = got[a]
        assert g[5] == w[5]
        np.testing.assert_allclose(g[:5], w[:5], rtol=1e-5, atol=1e-3)
    order = [(-r[4], r[6]) for r in rows.tolist()]
    assert order == sorted(order)                                                  # score descending, anchor ascending
    rc = {int(r[6]): c for r, c in zip(rrows.tolist(), rcoef)}
    for r in rows:
        assert torch.equal(r[7:].float(), rc[int(r[6])].float().cpu())             # the coefficients of the kept anchors, copied
    return rrows, rcoef


def _check_mask(mask, rrows, rcoef, proto, shape):
    want, lg = ref.union_mask(rrows, rcoef, proto, shape)
    # ambiguous: a logit within 1e-4 of 0 but not 0 (exact zeros are the crop's and must agree)
    amb = ((lg.abs() < 1e-4) & (lg != 0)).any(0) if len(lg) else torch.zeros(shape, dtype=torch.bool, device=proto.device)
    diff = (mask.bool() != want) & ~amb
    assert int(diff.sum()) == 0, int(diff.sum())
    return want


def test_detect_and_masks_against_the_reference():
    heads, proto = _heads(480, 640, _plants_general())
    motion = torch.rand((480, 640), device=DEV) > 0.1
    before = motion.clone()
    res = seg.postprocess(heads, proto, [0, 56], STRIDES, motion)
    assert int(res.counts[1]) > int(res.counts[0]) > 20
    rrows, rcoef = _check_dets(res, heads, proto, [0, 56])
    assert {0.0, 56.0} == set(rrows[:, 5].tolist())
    kept = set(_by_anchor(res.dets[:int(res.counts[0]), :7].cpu()))
    assert {810, 811} <= kept and 5005 not in kept
    want = _check_mask(res.mask, rrows, rcoef, proto, (480, 640))
    assert want.any()
    assert torch.equal(motion, before & ~res.mask.bool())                        # motion &= ~yolo, in place
    # the mask kernel alone, on the reference's detections
    dets = torch.cat((rrows, rcoef.cpu()), 1).float().to(DEV).contiguous()
    counts = torch.tensor([len(rrows), 0, 0], dtype=torch.int32, device=DEV)
    _check_mask(seg.masks_from_dets(dets, counts, proto), rrows, rcoef, proto, (480, 640))


def test_zero_candidates():
    heads, proto = _heads(480, 640, [])
    motion = torch.ones((480, 640), dtype=torch.bool, device=DEV)
    res = seg.postprocess(heads, proto, [0], STRIDES, motion)
    assert res.counts.tolist() == [0, 0, 0]
    assert not res.mask.any() and motion.all()


def test_more_than_max_det_in_one_class_and_score_ties():
    # 600 anchors of class 0 on level 0, boxes one cell wide on each side (1-cell neighbours: IoU 1/3, all survive NMS); scores come in
    # tied groups of 8
    plants = [(0, y, x, 0, 1.0 + 0.05 * ((y * 80 + x) // 8 % 40), (1, 1, 1, 1)) for y in range(0, 60, 2) for x in range(0, 80, 4)]
    plants = plants[:600] + [(1, 3, 3, 56, 2.0, (2, 2, 2, 2))]
    heads, proto = _heads(480, 640, plants, seed=5)
    res = seg.postprocess(heads, proto, [0, 56], STRIDES)
    assert int(res.counts[2]) == 601 and int(res.counts[0]) == 301                 # max_det per class: 300 of class 0, and the class 56 one
    rrows, rcoef = _check_dets(res, heads, proto, [0, 56])
    _check_mask(res.mask, rrows, rcoef, proto, (480, 640))


def test_postprocess_is_bitwise_repeatable_and_never_syncs():
    heads, proto = _heads(480, 640, _plants_general(7), seed=7)
    a = seg.postprocess(heads, proto, [0, 56], STRIDES)
    torch.cuda.synchronize()
    ws = {}
    seg.postprocess(heads, proto, [0, 56], STRIDES, workspaces=ws)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b = seg.postprocess(heads, proto, [0, 56], STRIDES, workspaces=ws)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a.mask, b.mask) and torch.equal(a.counts, b.counts)
    n = int(a.counts[0])
    assert torch.equal(a.dets[:n].view(torch.int32), b.dets[:n].view(torch.int32))


@pytest.fixture(scope="module")
def stand_in(tmp_path_factory):
    from slam import yolo_stand_in
    path = yolo_stand_in.write_checkpoint(str(tmp_path_factory.mktemp("yolo") / "stand_in.pt"), width=16, cls_bias=-1.5)
    return path


def test_network_against_the_unfused_reference(stand_in):
    ck = seg.load_checkpoint(stand_in)
    y = seg.YoloSeg.from_checkpoint(stand_in, DEV)
    assert seg.YoloSeg.from_checkpoint(stand_in, DEV) is y                        # loaded once per process
    g = torch.Generator().manual_seed(11)
    img = torch.rand((3, 480, 640), generator=g).to(DEV)
    heads, proto = y.forward(img)
    rheads, rproto = ref.network(ck["model"], img)
    for (h, c), (rh, rc) in zip(heads, rheads):
        assert float((h.double() - rh).abs().max()) <= 1e-4 * float(rh.abs().max())
        assert float((c.double() - rc).abs().max()) <= 1e-4 * float(rc.abs().max())
    assert float((proto.double() - rproto).abs().max()) <= 1e-4 * float(rproto.abs().max())
    # the seeded network's class scores are flat (float32 ties among neighbours): compare with float32-rounded reference scores, and
    # put conf in the widest gap among the top 16-256 scores; the two most frequent argmax classes
    best, j = ref.decode(heads, STRIDES, fp32_scores=True)[1].max(1)
    s = best.sort(descending=True).values
    k = 16 + int((s[15:255] - s[16:256]).argmax())
    assert float(s[k - 1] - s[k]) > 1e-6
    conf = float((s[k - 1] + s[k]) / 2)
    top = torch.bincount(j[best > conf], minlength=80).argsort(descending=True)[:2].tolist()
    y2 = seg.YoloSeg(ck["model"], DEV, conf=conf)
    res = y2.postprocess(heads, proto, top)
    rrows, rcoef = ref.detections(heads, STRIDES, top, conf=conf, fp32_scores=True)
    n = int(res.counts[0])
    assert n == len(rrows) > 0 and set(_by_anchor(res.dets[:n, :7].cpu())) == set(_by_anchor(rrows))
    _check_mask(res.mask, rrows, rcoef, proto, (480, 640))
    # two calls on the image: bitwise-identical masks
    m1 = y2(img, top).mask.clone()
    m2 = y2(img, top).mask
    assert torch.equal(m1, m2)


def test_capture_and_sizes_raise(stand_in):
    y = seg.YoloSeg.from_checkpoint(stand_in, DEV)
    with pytest.raises(ValueError, match="multiples of 32"):
        y.forward(torch.zeros((3, 240, 320), device=DEV))
    heads, proto = _heads(480, 640, [])
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(graph, stream=s):
                y.postprocess(heads, proto, [0])


class _FixedSegmenter:
    """A segmenter whose network output is fixed: the dataset's hook with given head tensors."""

    def __init__(self, heads, proto):
        self.heads, self.proto, self.calls = heads, proto, []

    def __call__(self, image, classes, motion=None):
        self.calls.append(list(classes))
        return seg.postprocess(self.heads, self.proto, classes, STRIDES, motion)


@pytest.mark.parametrize("file_masks", [False, True])
def test_tum_dataset_motion_masks(tmp_path, file_masks):
    from slam.dataset import SyntheticRGBDDataset
    from slam.recorded import load_dataset, write_tum_sequence
    H, W = 256, 320
    src = SyntheticRGBDDataset(num_frames=4, width=W, height=H, seed=1, dynamic=True, dystart=1)
    seq = tmp_path / "seq"
    calib = write_tum_sequence(src, str(seq), masks=file_masks)
    rng = np.random.default_rng(2)
    plants = [(int(rng.integers(0, 2)), int(rng.integers(0, 8)), int(rng.integers(0, 10)), int(rng.choice([0, 56])), 2.0,
               (2, 2, 2, 2)) for _ in range(6)]
    heads, proto = _heads(H, W, plants, seed=3)
    fixed = _FixedSegmenter(heads, proto)
    cfg = {"Dataset": {"type": "tum", "dataset_path": str(seq), "Calibration": calib, "seg_chair": False}}
    plain = load_dataset(cfg, DEV)
    ds = load_dataset(cfg, DEV, segmenter=fixed)
    assert ds.seg_classes == [0, 56]
    rrows, rcoef = ref.detections(heads, STRIDES, [0, 56])
    union, lg = ref.union_mask(rrows, rcoef, proto, (H, W))
    amb = ((lg.abs() < 1e-4) & (lg != 0)).any(0)                                 # ambiguous pixels, as in _check_mask
    assert union.any()
    for i in (0, 2, 3, 2):
        image, _, _, motion = ds[i]
        image0, _, _, motion0 = plain[i]
        _, _, _, m_src = src[i]
        file_moving = ~m_src if file_masks else torch.zeros_like(union)
        assert torch.equal(image, image0)
        assert torch.equal(motion0, ~file_moving)                                  # without a segmenter: the file masks alone
        assert torch.equal(motion[~amb], (~(union | file_moving))[~amb]), i
    assert len(fixed.calls) == 3                                                   # frame 2 read again: from the cache
    assert ds._frame_image(1) is not None and len(fixed.calls) == 3                # the flow path never segments
    st = ds.segmentation_stats
    assert st["frames"] == 3 and st["ms_per_frame"] > 0
    assert plain.segmentation_stats is None
    ds.close()
    plain.close()


def test_dynamic_slam_run_with_a_segmenter(tmp_path, stand_in):
    from slam.config import apply_cli_overrides
    from slam.dataset import SyntheticRGBDDataset
    from slam.recorded import load_dataset, write_tum_sequence
    from slam.system import SLAM, default_config
    torch.manual_seed(0)
    src = SyntheticRGBDDataset(num_frames=12, width=320, height=256, seed=1, dynamic=True, dystart=4)
    seq = tmp_path / "dyn"
    calib = write_tum_sequence(src, str(seq), masks=True)
    cfg = default_config()
    cfg["Dataset"].update({"type": "tum", "dataset_path": str(seq), "Calibration": calib})
    cfg["Training"].update({"init_itr_num": 100, "init_gaussian_update": 50, "init_gaussian_reset": 60, "tracking_itr_num": 20,
                            "static_map_iters": 10, "dynamic_map_iters": 20, "network_init_iters": 20, "gaussian_update_every": 60,
                            "gaussian_update_offset": 20, "kf_interval": 4, "dystart": 4})
    cfg["Results"].update({"save_results": False, "use_gui": False})
    cfg = apply_cli_overrides(cfg, dynamic=True)
    y = seg.YoloSeg.from_checkpoint(stand_in, DEV)
    ds = load_dataset(cfg, DEV, segmenter=y)
    res = SLAM(cfg, ds).run()
    assert res["frames"] == 12 and np.isfinite(res["ate_rmse"])
    assert ds.segmentation_stats["frames"] >= 12
    ds.close()
