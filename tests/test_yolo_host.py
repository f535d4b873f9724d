"""Host-side checks of the YOLO segmenter (slam/segmentation.py): loading an ultralytics-style checkpoint without ultralytics (fp16 to fp32,
the layer graph from `f`), refusing foreign globals and unknown module types, the size rule, the loaders' class sets, the fp64 reference
(tests/yolo_reference.py) on hand-made NMS cases, its vectorised NMS against the scalar statement, its max_dets rule and its two
input-quality measures, and tools/run_slam.py's --yolo-weights. No GPU needed."""
import io
import os
import pickle
import sys
import zipfile

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import segmentation as seg  # noqa: E402
from slam import yolo_stand_in  # noqa: E402
import yolo_reference as ref  # noqa: E402


@pytest.fixture(scope="module")
def ckpt_path(tmp_path_factory):
    return yolo_stand_in.write_checkpoint(str(tmp_path_factory.mktemp("yolo") / "stand_in.pt"), width=16)


def test_checkpoint_loads_without_ultralytics(ckpt_path):
    assert not any(k == "ultralytics" or k.startswith("ultralytics.") for k in sys.modules)      # the fake modules are gone
    ck = seg.load_checkpoint(ckpt_path)
    assert ck["ema"] is None
    model = ck["model"]
    assert isinstance(model, seg.Stub) and model.path == "ultralytics.nn.tasks.SegmentationModel"
    layers = list(seg.children(seg.child(model, "model")).values())
    assert len(layers) == 43
    assert [seg.kind(m) for m in layers[:3]] == ["Silence", "Conv", "Conv"]
    assert layers[16].f == [10, 11, 12, 13, 14, -1] and layers[42].f == [35, 38, 41]
    w = layers[1]._modules["conv"]._parameters["weight"]
    assert w.dtype == torch.float16                                   # stored half, as a stripped ultralytics checkpoint is
    y = seg.YoloSeg(model, "cpu")
    assert y.nc == 80 and y.nm == 32 and y.stride == [8.0, 16.0, 32.0]
    assert y.save == {0, 1, 3, 5, 7, 9, 10, 11, 12, 13, 14, 22, 25, 29, 32, 35, 38, 41}
    conv = y.layers[1][2]
    assert conv.w.dtype == torch.float32 and conv.b is not None       # BatchNorm folded into a biased fp32 convolution


def test_loaded_network_matches_the_unfused_reference_on_cpu(ckpt_path):
    ck = seg.load_checkpoint(ckpt_path)
    y = seg.YoloSeg(ck["model"], "cpu")
    g = torch.Generator().manual_seed(3)
    img = torch.rand((3, 64, 96), generator=g)
    heads, proto = y.forward(img)
    rheads, rproto = ref.network(ck["model"], img)
    for (h, c), (rh, rc) in zip(heads, rheads):
        assert h.shape == rh.shape and c.shape == rc.shape
        assert float((h.double() - rh).abs().max()) <= 1e-4 * float(rh.abs().max())
        assert float((c.double() - rc).abs().max()) <= 1e-4 * float(rc.abs().max())
    assert float((proto.double() - rproto).abs().max()) <= 1e-4 * float(rproto.abs().max())


def _with_pickle(tmp_path, obj_pickle):
    """A torch zip checkpoint whose data.pkl is the given bytes."""
    buf = io.BytesIO()
    torch.save({"a": 1}, buf)
    src = zipfile.ZipFile(io.BytesIO(buf.getvalue()))
    path = tmp_path / "evil.pt"
    with zipfile.ZipFile(path, "w") as dst:
        for info in src.infolist():
            data = obj_pickle if info.filename.endswith("data.pkl") else src.read(info)
            dst.writestr(info, data)
    return str(path)


def test_foreign_global_is_refused(tmp_path):
    payload = b"cos\nsystem\n(S'echo pwned'\ntR."                     # os.system('echo pwned')
    with pytest.raises(pickle.UnpicklingError, match=r"os\.system|posix\.system"):
        seg.load_checkpoint(_with_pickle(tmp_path, payload))
    payload = b"cbuiltins\neval\n(S'1'\ntR."
    with pytest.raises(pickle.UnpicklingError, match=r"builtins\.eval"):
        seg.load_checkpoint(_with_pickle(tmp_path, payload))


def test_unknown_module_type_is_named(tmp_path):
    model, U = yolo_stand_in.build_model(width=32, n=1)
    C2f = type("C2f", (torch.nn.Module,), {"__module__": "ultralytics.nn.modules.block", "__qualname__": "C2f"})
    bad = C2f()
    bad.f, bad.i = -1, 5
    model.model[5] = bad
    U = dict(U, C2f=C2f)
    path = str(tmp_path / "c2f.pt")
    with yolo_stand_in.registered(U):
        torch.save({"model": model, "ema": None}, path)
    with pytest.raises(ValueError, match=r"ultralytics\.nn\.modules\.block\.C2f"):
        seg.YoloSeg.from_checkpoint(path, "cpu")


def test_sizes_not_multiple_of_32_raise(ckpt_path):
    y = seg.YoloSeg(seg.load_checkpoint(ckpt_path)["model"], "cpu")
    for h, w in ((480, 630), (470, 640), (100, 96)):
        with pytest.raises(ValueError, match="multiples of 32"):
            y.forward(torch.zeros((3, h, w)))
    seg.check_size(480, 640)


def test_class_sets_per_loader():
    dc = seg.dataset_classes
    assert dc("tum", {}, False) == [0]
    assert dc("tum", {"seg_chair": False}, False) == [0, 56]          # presence, not value (utils/dataset.py:315)
    assert dc("tum", {"seg_chair": True}, True) == [0, 56]            # TUM ORs its file masks with YOLO
    assert dc("CoFusion", {}, False) == [0]
    assert dc("CoFusion", {"seg_clock": True, "seg_teddy": True}, False) == [0, 74, 77]
    assert dc("CoFusion", {"seg_clock": False, "seg_teddy": True}, False) == [0, 77]
    assert dc("CoFusion", {"seg_clock": True, "seg_teddy": True}, True) is None     # mask_colour/*.png: no YOLO
    with pytest.raises(ValueError):
        dc("replica", {}, False)


# ---- the fp64 reference on hand-made cases ------------------------------------------------------------------------------------------
def _case(boxes, scores):
    """xywh boxes [n, 4], class scores [n, nc] as the decode would give them; zero coefficients."""
    b = torch.tensor(boxes, dtype=torch.float64)
    s = torch.tensor(scores, dtype=torch.float64)
    return b, s, torch.zeros((len(b), 32), dtype=torch.float64)


def _iou_pair(iou):
    """Two 10 x 10 boxes side by side whose IoU is `iou`: overlap o with o / (200 - o) = iou."""
    o = 200 * iou / (1 + iou)
    shift = 10 * (1 - o / 100)
    return [[50, 50, 10, 10], [50 + shift, 50, 10, 10]]


def test_reference_iou_threshold():
    above = _case(_iou_pair(0.7 + 1e-6), [[0.9, 0.0], [0.8, 0.0]])
    rows, _ = ref.non_max_suppression(*above, cls_id=0)
    assert rows[:, 6].tolist() == [0.0]                               # IoU just above 0.7: suppressed
    below = _case(_iou_pair(0.7 - 1e-6), [[0.9, 0.0], [0.8, 0.0]])
    rows, _ = ref.non_max_suppression(*below, cls_id=0)
    assert rows[:, 6].tolist() == [0.0, 1.0]                          # just below: both kept


def test_reference_same_box_in_two_classes_survives():
    b, s, c = _case([[50, 50, 10, 10], [50, 50, 10, 10]], [[0.9, 0.1], [0.1, 0.8]])
    r0, _ = ref.non_max_suppression(b, s, c, 0)
    r1, _ = ref.non_max_suppression(b, s, c, 1)
    assert r0[:, 6].tolist() == [0.0] and r1[:, 6].tolist() == [1.0]


def test_reference_best_class_outside_the_set_is_dropped():
    # anchor 0: class 1 is best (0.9) while class 0 (0.6) also exceeds conf; asking for class 0 drops it
    b, s, c = _case([[50, 50, 10, 10], [150, 50, 10, 10]], [[0.6, 0.9], [0.7, 0.1]])
    rows, _ = ref.non_max_suppression(b, s, c, 0)
    assert rows[:, 6].tolist() == [1.0]


def test_reference_score_exactly_at_conf_is_dropped():
    b, s, c = _case([[50, 50, 10, 10], [150, 50, 10, 10]], [[0.25, 0.0], [0.2500001, 0.0]])
    rows, _ = ref.non_max_suppression(b, s, c, 0)
    assert rows[:, 6].tolist() == [1.0]


def test_reference_max_det_and_score_ties():
    boxes = [[20 * (k % 30) + 10, 20 * (k // 30) + 10, 8, 8] for k in range(320)]      # 320 disjoint boxes of one class
    scores = [[0.5, 0.0] for _ in range(320)]                                           # all tied
    rows, _ = ref.non_max_suppression(*_case(boxes, scores), cls_id=0)
    assert rows[:, 6].tolist() == [float(k) for k in range(300)]                        # ties by anchor, cut at max_det


def _nms_inputs():
    """name -> (xyxy boxes [n, 4], scores [n]) with n <= 300, so that the scalar nms() stays fast."""
    g = torch.Generator().manual_seed(0)
    out = {}
    xy = torch.rand((300, 2), generator=g, dtype=torch.float64) * 100
    wh = torch.rand((300, 2), generator=g, dtype=torch.float64) * 40 + 5
    out["random"] = (torch.cat((xy, xy + wh), 1), torch.rand(300, generator=g, dtype=torch.float64))
    # dense: jittered copies of 12 boxes, so that most IoUs are high and survivors suppress in long runs
    base = out["random"][0][:12].repeat(25, 1) + torch.rand((300, 4), generator=g, dtype=torch.float64) * 4
    out["random dense"] = (base, torch.rand(300, generator=g, dtype=torch.float64))
    out["identical"] = (torch.tensor([[10.0, 20.0, 50.0, 70.0]], dtype=torch.float64).repeat(200, 1),
                        torch.rand(200, generator=g, dtype=torch.float64))
    k = torch.arange(256, dtype=torch.float64)
    x, y = (k % 16) * 20, (k // 16) * 20
    out["disjoint"] = (torch.stack((x, y, x + 20, y + 20), 1), torch.rand(256, generator=g, dtype=torch.float64))     # edges touch: IoU 0
    for d in (2, 6):                                       # 1-cell shifts of a box of half-width d cells: IoU 0.6 and 0.846 next door
        x = torch.arange(300, dtype=torch.float64) * 8
        b = torch.stack((x - 8 * d, torch.zeros(300, dtype=torch.float64), x + 8 * d, torch.full((300,), 16.0 * d, dtype=torch.float64)), 1)
        out[f"chain d={d} descending"] = (b, torch.linspace(0.9, 0.3, 300, dtype=torch.float64))
        out[f"chain d={d} random"] = (b, torch.rand(300, generator=g, dtype=torch.float64))
    out["tied scores"] = (out["random dense"][0], torch.randint(0, 4, (300,), generator=g).double() / 8 + 0.3)
    out["all tied"] = (out["chain d=6 random"][0], torch.full((300,), 0.5, dtype=torch.float64))
    out["empty"] = (torch.zeros((0, 4), dtype=torch.float64), torch.zeros(0, dtype=torch.float64))
    out["one"] = (out["random"][0][:1], out["random"][1][:1])
    return out


@pytest.mark.parametrize("name", sorted(_nms_inputs()))
def test_reference_vectorised_nms_equals_the_scalar_statement(name):
    boxes, scores = _nms_inputs()[name]
    for thr in (0.7, 0.45):
        want = ref.nms(boxes, scores, thr)
        assert ref.nms_vectorised(boxes, scores, thr) == want
        if name == "identical":
            assert len(want) == 1
        if name == "disjoint":
            assert len(want) == len(boxes)
        if name == "chain d=6 descending" and thr == 0.7:
            assert want == list(range(0, 300, 3))          # shifts 1 and 2 (IoU 0.846, 0.714) go, shift 3 (0.6) stays
        if name == "all tied" and thr == 0.7:
            assert want == list(range(0, 300, 3))          # ties are visited by lower index


def _tiny_heads(cands, nc=2, width=8):
    """One level of 1 x width anchors (stride 8), background class logits -6; cands: anchor -> (class, logit). Every box is its own
    cell (l, t, r, b = 0, 0, 1, 1 by near one-hot DFL bins), so nothing is suppressed."""
    h = torch.zeros((64 + nc, 1, width))
    h[64:] = -6.0
    for k, d in enumerate((0, 0, 1, 1)):
        h[k * 16 + d] = 12.0
    for a, (c, logit) in cands.items():
        h[64 + c, 0, a] = logit
    return [(h, torch.arange(3.0 * width).reshape(3, 1, width))]


def test_reference_max_dets_rule():
    # global order: a0 (class 0) a5 (1) a1 (0) a6 (1) a2 (0) a3 (0) a7 (1) a4 (0)
    heads = _tiny_heads({0: (0, 3.0), 1: (0, 2.0), 2: (0, 1.0), 3: (0, 0.5), 4: (0, 0.0), 5: (1, 2.5), 6: (1, 1.5), 7: (1, 0.2)})

    def anchors(**kw):
        rows, coef, counts = ref.detections(heads, [8.0], [0, 1], counts=True, **kw)
        assert counts == (len(rows), 8, 8) and torch.equal(coef[:, 0], rows[:, 6])      # coefficient 0 of anchor a is a
        return [int(a) for a in rows[:, 6]]

    assert anchors() == [0, 1, 2, 3, 4, 5, 6, 7]                                        # per class, concatenated
    assert anchors(max_det=3) == [0, 1, 2, 5, 6, 7]
    assert anchors(max_det=3, max_dets=6) == [0, 1, 2, 5, 6, 7]                         # max_dets not binding: as without it
    assert anchors(max_det=3, max_dets=4) == [0, 1, 5, 6]                               # the first four of the global order
    assert anchors(max_det=3, max_dets=5) == [0, 1, 2, 5, 6]
    assert anchors(max_det=2, max_dets=5) == [0, 1, 5, 6]                               # a2 is over its class's max_det: never counted
    assert anchors(max_det=1, max_dets=2) == [0, 5]
    assert anchors(max_det=5, max_dets=1) == [0]
    rows, _ = ref.detections(heads, [8.0], [1], max_dets=2)
    assert [int(a) for a in rows[:, 6]] == [5, 6]


def test_reference_input_quality_measures():
    a, b = [0.0, 0.0, 10.0, 10.0], [5.0, 0.0, 15.0, 10.0]                               # IoU 50 / 150
    assert ref.min_iou_margin([a, b], [0, 0], 0.7) == pytest.approx(0.7 - 1 / 3, abs=1e-15)
    assert ref.min_iou_margin([a, b], [0, 0], 0.3) == pytest.approx(1 / 3 - 0.3, abs=1e-15)
    assert ref.min_iou_margin([a, b], [0, 1], 0.7) == float("inf")                      # no pair of equal class
    assert ref.min_iou_margin([a], [0], 0.7) == float("inf") and ref.min_iou_margin([], [], 0.7) == float("inf")
    c = [0.0, 0.0, 10.0, 10.5]                                                          # IoU with a: 100 / 105; with b: 50 / 155
    assert ref.min_iou_margin([a, b, c], [0, 0, 0], 0.7) == pytest.approx(100 / 105 - 0.7, abs=1e-15)
    assert ref.min_iou_margin([a, b, c], [0, 0, 1], 0.7) == pytest.approx(0.7 - 1 / 3, abs=1e-15)
    assert ref.min_iou_margin([a, b, a], [0, 1, 1], 0.7) == pytest.approx(0.7 - 1 / 3, abs=1e-15)      # a and a differ in class
    assert ref.min_iou_margin([a, a], [3, 3], 0.7) == pytest.approx(0.3, abs=1e-15)
    z = [3.0, 3.0, 3.0, 9.0]                                                            # zero area: IoU 0 with everything, itself included
    assert ref.min_iou_margin([z, z], [0, 0], 0.7) == pytest.approx(0.7, abs=1e-15)
    many = torch.tensor([a, b, c] * 400, dtype=torch.float64)                           # more than one block of rows
    many[1100] = torch.tensor([0.0, 0.0, 10.0, 14.0])                                   # IoU with a: 100 / 140 = 0.714
    assert ref.min_iou_margin(many, torch.zeros(1200), 0.7) == pytest.approx(100 / 140 - 0.7, abs=1e-15)

    assert ref.min_score_gap([0.9, 0.5, 0.5, 0.26]) == pytest.approx(0.01, abs=1e-15)   # to conf; the tie is no gap
    assert ref.min_score_gap([0.9, 0.5, 0.5, 0.6, 0.26], conf=0.1) == pytest.approx(0.1, abs=1e-15)
    assert ref.min_score_gap([0.9, 0.9 - 1e-6, 0.5]) == pytest.approx(1e-6, abs=1e-15)
    assert ref.min_score_gap([0.5, 0.5]) == pytest.approx(0.25, abs=1e-15)
    assert ref.min_score_gap([0.2], conf=0.25) == pytest.approx(0.05, abs=1e-15)
    assert ref.min_score_gap([]) == float("inf")


def test_run_slam_yolo_flag(tmp_path):
    import run_slam
    args = run_slam.parse_args(["--config", "x.yaml"])
    assert args.yolo_weights is None
    w = tmp_path / "w.pt"
    w.write_bytes(b"")
    args = run_slam.parse_args(["--config", "x.yaml", "--yolo-weights", str(w)])
    assert args.yolo_weights == str(w) and not args.dynamic           # YOLO serves static runs too: the reference always loads it
    with pytest.raises(SystemExit):
        run_slam.parse_args(["--config", "x.yaml", "--yolo-weights", str(tmp_path / "missing.pt")])
