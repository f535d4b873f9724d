"""Seeded stand-in YOLOv9-seg checkpoints (no real checkpoint is needed to build, test or time the segmenter).

``write_checkpoint`` pickles a model the way an ultralytics checkpoint holds one: a SegmentationModel whose ``model`` is a Sequential of
layers with ``f`` / ``i`` / ``type`` attributes, built from modules whose classes carry the ``ultralytics.nn.modules.*`` names. Those
classes are plain torch.nn.Module subclasses made here and placed in sys.modules only while the file is written. The topology is that of
the public yolov9e-seg.yaml (Silence, Conv, RepNCSPELAN4, ADown, CBLinear, CBFuse, SPPELAN, Upsample, Concat, Segment); ``width``
divides every channel count, so width=1 is yolov9e-seg's size and width=16 a network small enough for tests. Weights are seeded
(per module, in build order); BatchNorm statistics are non-trivial so that folding them matters. The weights carry no meaning."""
import contextlib
import sys
import types

import torch
import torch.nn as nn

_MODULES = {"Conv": "conv", "Concat": "conv", "RepConvN": "block", "RepBottleneck": "block", "RepCSP": "block", "RepNCSPELAN4": "block",
            "ADown": "block", "SPPELAN": "block", "CBLinear": "block", "CBFuse": "block", "Silence": "block", "DFL": "block", "Proto": "block",
            "Segment": "head", "SegmentationModel": None}


def fake_classes():
    """name -> an nn.Module subclass whose __module__ / __qualname__ are ultralytics' for that name."""
    out = {}
    for name, sub in _MODULES.items():
        module = "ultralytics.nn.tasks" if sub is None else f"ultralytics.nn.modules.{sub}"
        out[name] = type(name, (nn.Module,), {"__module__": module, "__qualname__": name})
    return out


@contextlib.contextmanager
def registered(classes):
    """Place the fake classes' modules (and their parent packages) in sys.modules for pickling; remove them afterwards."""
    added = []
    for cls in classes.values():
        parts = cls.__module__.split(".")
        for k in range(1, len(parts) + 1):
            name = ".".join(parts[:k])
            if name not in sys.modules:
                sys.modules[name] = types.ModuleType(name)
                added.append(name)
        setattr(sys.modules[cls.__module__], cls.__qualname__, cls)
    try:
        yield
    finally:
        for name in added:
            sys.modules.pop(name, None)


class _Builder:
    def __init__(self, U, seed):
        self.U = U
        self.g = torch.Generator().manual_seed(seed)

    def _u(self, shape, lo, hi):
        return torch.rand(shape, generator=self.g) * (hi - lo) + lo

    def conv(self, c1, c2, k=1, s=1, p=None, g=1, act=True):
        m = self.U["Conv"]()
        m.conv = nn.Conv2d(c1, c2, k, s, k // 2 if p is None else p, groups=g, bias=False)
        b = (1.0 / (c1 // g * k * k)) ** 0.5
        m.conv.weight.data = self._u(m.conv.weight.shape, -b, b)
        m.bn = nn.BatchNorm2d(c2, eps=1e-3)
        m.bn.weight.data = self._u((c2,), 0.8, 1.2)
        m.bn.bias.data = self._u((c2,), -0.1, 0.1)
        m.bn.running_mean = self._u((c2,), -0.1, 0.1)
        m.bn.running_var = self._u((c2,), 0.5, 1.5)
        m.act = nn.SiLU() if act else nn.Identity()
        return m

    def conv2d(self, c1, c2, k=1, bias_value=None):
        m = nn.Conv2d(c1, c2, k, 1, k // 2, bias=True)
        b = (1.0 / (c1 * k * k)) ** 0.5
        m.weight.data = self._u(m.weight.shape, -b, b)
        m.bias.data = self._u((c2,), -b, b) if bias_value is None else torch.full((c2,), float(bias_value))
        return m

    def repconvn(self, c1, c2):
        m = self.U["RepConvN"]()
        m.act = nn.SiLU()
        m.bn = None
        m.conv1 = self.conv(c1, c2, 3, 1, 1, act=False)
        m.conv2 = self.conv(c1, c2, 1, 1, 0, act=False)
        return m

    def repbottleneck(self, c1, c2, shortcut=True):
        m = self.U["RepBottleneck"]()
        m.cv1 = self.repconvn(c1, c2)
        m.cv2 = self.conv(c2, c2, 3, 1)
        m.add = shortcut and c1 == c2
        return m

    def repcsp(self, c1, c2, n=1):
        m = self.U["RepCSP"]()
        c_ = int(c2 * 0.5)
        m.cv1, m.cv2, m.cv3 = self.conv(c1, c_), self.conv(c1, c_), self.conv(2 * c_, c2)
        m.m = nn.Sequential(*(self.repbottleneck(c_, c_) for _ in range(n)))
        return m

    def elan(self, c1, c2, c3, c4, n=1):
        m = self.U["RepNCSPELAN4"]()
        m.c = c3 // 2
        m.cv1 = self.conv(c1, c3, 1, 1)
        m.cv2 = nn.Sequential(self.repcsp(c3 // 2, c4, n), self.conv(c4, c4, 3, 1))
        m.cv3 = nn.Sequential(self.repcsp(c4, c4, n), self.conv(c4, c4, 3, 1))
        m.cv4 = self.conv(c3 + 2 * c4, c2, 1, 1)
        return m

    def adown(self, c1, c2):
        m = self.U["ADown"]()
        m.c = c2 // 2
        m.cv1 = self.conv(c1 // 2, m.c, 3, 2, 1)
        m.cv2 = self.conv(c1 // 2, m.c, 1, 1, 0)
        return m

    def sppelan(self, c1, c2, c3, k=5):
        m = self.U["SPPELAN"]()
        m.c = c3
        m.cv1 = self.conv(c1, c3, 1, 1)
        m.cv2, m.cv3, m.cv4 = (nn.MaxPool2d(kernel_size=k, stride=1, padding=k // 2) for _ in range(3))
        m.cv5 = self.conv(4 * c3, c2, 1, 1)
        return m

    def cblinear(self, c1, c2s):
        m = self.U["CBLinear"]()
        m.c2s = list(c2s)
        m.conv = self.conv2d(c1, sum(c2s), 1)
        return m

    def cbfuse(self, idx):
        m = self.U["CBFuse"]()
        m.idx = list(idx)
        return m

    def concat(self, d=1):
        m = self.U["Concat"]()
        m.d = d
        return m

    def segment(self, nc, nm, npr, ch, cls_bias):
        m = self.U["Segment"]()
        m.nc, m.nl, m.reg_max, m.nm, m.npr = nc, len(ch), 16, nm, npr
        m.no = nc + m.reg_max * 4
        m.stride = torch.tensor([8.0, 16.0, 32.0][:len(ch)])
        c2, c3, c4 = max((16, ch[0] // 4, m.reg_max * 4)), max(ch[0], min(nc, 100)), max(ch[0] // 4, nm)
        m.cv2 = nn.ModuleList(nn.Sequential(self.conv(x, c2, 3), self.conv(c2, c2, 3), self.conv2d(c2, 4 * m.reg_max, 1)) for x in ch)
        m.cv3 = nn.ModuleList(nn.Sequential(self.conv(x, c3, 3), self.conv(c3, c3, 3), self.conv2d(c3, nc, 1, cls_bias)) for x in ch)
        dfl = self.U["DFL"]()
        dfl.conv = nn.Conv2d(16, 1, 1, bias=False).requires_grad_(False)
        dfl.conv.weight.data[:] = torch.arange(16, dtype=torch.float).view(1, 16, 1, 1)
        dfl.c1 = 16
        m.dfl = dfl
        proto = self.U["Proto"]()
        proto.cv1 = self.conv(ch[0], npr, 3)
        proto.upsample = nn.ConvTranspose2d(npr, npr, 2, 2, 0, bias=True)
        b = (1.0 / (npr * 4)) ** 0.5
        proto.upsample.weight.data = self._u(proto.upsample.weight.shape, -b, b)
        proto.upsample.bias.data = self._u((npr,), -b, b)
        proto.cv2 = self.conv(npr, npr, 3)
        proto.cv3 = self.conv(npr, nm)
        m.proto = proto
        m.cv4 = nn.ModuleList(nn.Sequential(self.conv(x, c4, 3), self.conv(c4, c4, 3), self.conv2d(c4, nm, 1)) for x in ch)
        return m


def build_model(width=16, nc=80, nm=32, n=2, seed=0, cls_bias=-2.0):
    """The stand-in SegmentationModel (float32, eval mode): yolov9e-seg.yaml's layers with every channel count divided by `width`
    and `n` repeats in each RepCSP. cls_bias: the class convolutions' bias (a low value keeps most anchors below conf)."""
    U = fake_classes()
    B = _Builder(U, seed)
    c = lambda v: max(2, v // width)
    layers = []

    def add(f, mod):
        mod.f, mod.i, mod.type = f, len(layers), f"{type(mod).__module__}.{type(mod).__name__}"
        layers.append(mod)

    add(-1, U["Silence"]())                                                     # 0
    add(-1, B.conv(3, c(64), 3, 2))                                             # 1  P1/2
    add(-1, B.conv(c(64), c(128), 3, 2))                                        # 2  P2/4
    add(-1, B.elan(c(128), c(256), c(128), c(64), n))                           # 3
    add(-1, B.adown(c(256), c(256)))                                            # 4  P3/8
    add(-1, B.elan(c(256), c(512), c(256), c(128), n))                          # 5
    add(-1, B.adown(c(512), c(512)))                                            # 6  P4/16
    add(-1, B.elan(c(512), c(1024), c(512), c(256), n))                         # 7
    add(-1, B.adown(c(1024), c(1024)))                                          # 8  P5/32
    add(-1, B.elan(c(1024), c(1024), c(512), c(256), n))                        # 9
    add(1, B.cblinear(c(64), [c(64)]))                                          # 10
    add(3, B.cblinear(c(256), [c(64), c(128)]))                                 # 11
    add(5, B.cblinear(c(512), [c(64), c(128), c(256)]))                         # 12
    add(7, B.cblinear(c(1024), [c(64), c(128), c(256), c(512)]))                # 13
    add(9, B.cblinear(c(1024), [c(64), c(128), c(256), c(512), c(1024)]))       # 14
    add(0, B.conv(3, c(64), 3, 2))                                              # 15 P1/2
    add([10, 11, 12, 13, 14, -1], B.cbfuse([0, 0, 0, 0, 0]))                    # 16
    add(-1, B.conv(c(64), c(128), 3, 2))                                        # 17 P2/4
    add([11, 12, 13, 14, -1], B.cbfuse([1, 1, 1, 1]))                           # 18
    add(-1, B.elan(c(128), c(256), c(128), c(64), n))                           # 19
    add(-1, B.adown(c(256), c(256)))                                            # 20 P3/8
    add([12, 13, 14, -1], B.cbfuse([2, 2, 2]))                                  # 21
    add(-1, B.elan(c(256), c(512), c(256), c(128), n))                          # 22
    add(-1, B.adown(c(512), c(512)))                                            # 23 P4/16
    add([13, 14, -1], B.cbfuse([3, 3]))                                         # 24
    add(-1, B.elan(c(512), c(1024), c(512), c(256), n))                         # 25
    add(-1, B.adown(c(1024), c(1024)))                                          # 26 P5/32
    add([14, -1], B.cbfuse([4]))                                                # 27
    add(-1, B.elan(c(1024), c(1024), c(512), c(256), n))                        # 28
    add(-1, B.sppelan(c(1024), c(512), c(256)))                                 # 29
    add(-1, nn.Upsample(None, 2, "nearest"))                                    # 30
    add([-1, 25], B.concat(1))                                                  # 31
    add(-1, B.elan(c(1024) + c(512), c(512), c(512), c(256), n))                # 32
    add(-1, nn.Upsample(None, 2, "nearest"))                                    # 33
    add([-1, 22], B.concat(1))                                                  # 34
    add(-1, B.elan(c(512) + c(512), c(256), c(256), c(128), n))                 # 35
    add(-1, B.adown(c(256), c(256)))                                            # 36
    add([-1, 32], B.concat(1))                                                  # 37
    add(-1, B.elan(c(256) + c(512), c(512), c(512), c(256), n))                 # 38
    add(-1, B.adown(c(512), c(512)))                                            # 39
    add([-1, 29], B.concat(1))                                                  # 40
    add(-1, B.elan(c(512) + c(512), c(512), c(1024), c(512), n))                # 41
    add([35, 38, 41], B.segment(nc, nm, c(256), [c(256), c(512), c(512)], cls_bias))   # 42
    model = U["SegmentationModel"]()
    model.model = nn.Sequential(*layers)
    model.save = sorted({j for m in layers for j in ([m.f] if isinstance(m.f, int) else m.f) if j != -1})
    model.stride = torch.tensor([8.0, 16.0, 32.0])
    model.names = {k: str(k) for k in range(nc)}
    model.yaml = {"nc": nc, "stand_in": True}
    return model.eval(), U


def write_checkpoint(path, half=True, **kw):
    """torch.save an ultralytics-style checkpoint dict ({'model': the half-precision model, 'ema': None, ...}) of build_model(**kw)."""
    model, U = build_model(**kw)
    if half:
        model = model.half()
    ckpt = {"date": "stand-in", "version": "stand-in", "model": model, "ema": None, "updates": None, "optimizer": None,
            "train_args": {"imgsz": 640}, "train_metrics": {"metrics/mAP50(B)": 0.0}}
    with registered(U):
        torch.save(ckpt, path)
    return path
