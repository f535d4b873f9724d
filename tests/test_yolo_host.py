"""Host-side checks of the YOLO segmenter (slam/segmentation.py): loading an ultralytics-style checkpoint without ultralytics (fp16 to fp32,
the layer graph from `f`), refusing foreign globals and unknown module types, the size rule, the loaders' class sets, the fp64 reference
(tests/yolo_reference.py) on hand-made NMS cases, and tools/run_slam.py's --yolo-weights. No GPU needed."""
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
