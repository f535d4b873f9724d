"""Instance segmentation of moving people and objects: the YOLO-seg model the reference runs on every recorded frame
(slam.py:80 loads pretrained/yolov9e-seg.pt; utils/dataset.py:340-373, 612-650 OR the instance masks of chosen COCO classes into the
frame's motion mask), in inference only and without ultralytics.

The checkpoint is read by a restricted unpickler: every ``ultralytics.*`` and ``torch.nn.modules.*`` class becomes an inert stub that
keeps its pickled attributes, tensors are rebuilt by torch, and any other global (``os.system`` and the like) is refused. The layer graph
is rebuilt from each layer's ``f`` / ``i`` attributes and every hyper-parameter from the child modules' own attributes; BatchNorm is
folded into the convolutions at load time (in float64, stored as float32) and the network runs on torch.nn.functional (MIOpen) in fp32.

The post-processing is HIP (include/segmentation.h, csrc/gs_yolo.h): DFL decode, per-class greedy NMS with max_det per class, and the
masks' crop, bilinear upsampling and threshold, folded into the motion mask in place, in five launches with no host round trip."""
import ctypes as C
import io
import pickle
from typing import NamedTuple

import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization._abi import GSR_YOLO_DET_HEAD, GSR_YOLO_MAX_ANCHORS, GSR_YOLO_MAX_LEVELS, GSR_YOLO_REG_MAX
from . import pretrained

CONF, IOU, MAX_DET = 0.25, 0.7, 300          # ultralytics predictor defaults
PERSON, CHAIR, CLOCK, TEDDY_BEAR = 0, 56, 74, 77


# ---- the restricted unpickler --------------------------------------------------------------------------------------------------------
class Stub:
    """An inert stand-in for a pickled ultralytics or torch.nn class: it keeps the pickled state as attributes and has no behaviour."""

    path = "?"

    def __init__(self, *args, **kwargs):           # a stubbed callable reached through REDUCE: keep the arguments, run nothing
        self.__dict__["_args"] = args

    def __setstate__(self, state):
        if isinstance(state, tuple) and len(state) == 2 and (state[0] is None or isinstance(state[0], dict)):
            state = {**(state[0] or {}), **(state[1] or {})}
        if isinstance(state, dict):
            self.__dict__.update(state)
        else:
            self.__dict__["_state"] = state

    def __repr__(self):
        return f"<stub {self.path}>"


_stubs = {}


def _stub(module, name):
    path = f"{module}.{name}"
    cls = _stubs.get(path)
    if cls is None:
        cls = _stubs[path] = type(name, (Stub,), {"path": path})
    return cls


_ALLOWED = {
    ("torch._utils", "_rebuild_tensor_v2"), ("torch._utils", "_rebuild_parameter"), ("torch._utils", "_rebuild_parameter_with_state"),
    ("collections", "OrderedDict"), ("builtins", "set"), ("builtins", "frozenset"), ("__builtin__", "set"), ("__builtin__", "frozenset"),
    ("torch", "Size"), ("torch", "device"),
    ("_codecs", "encode"), ("numpy", "dtype"), ("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
}


class _Unpickler(pickle.Unpickler):
    def find_class(self, module, name):
        if module == "ultralytics" or module.startswith("ultralytics.") or module.startswith("torch.nn.modules."):
            return _stub(module, name)
        if (module, name) in _ALLOWED or (module == "torch" and isinstance(getattr(torch, name, None), torch.dtype)):
            return super().find_class(module, name)
        raise pickle.UnpicklingError(f"refusing the global {module}.{name}: a YOLO checkpoint holds only ultralytics / torch.nn modules, "
                                     "tensors and plain data")


class _RestrictedPickle:
    """The pickle_module torch.load reads with: torch's own wrapper derives from this Unpickler (storages stay torch's)."""
    Unpickler = _Unpickler
    __name__ = "restricted_pickle"

    @staticmethod
    def load(f, **kw):
        return _Unpickler(f, **kw).load()


def load_checkpoint(path):
    """The checkpoint's dict, with every module a Stub. Never imports ultralytics."""
    with open(path, "rb") as f:
        data = f.read()
    return torch.load(io.BytesIO(data), map_location="cpu", pickle_module=_RestrictedPickle, weights_only=False)


# ---- the module graph ----------------------------------------------------------------------------------------------------------------
def kind(m):
    return type(m).__name__


def children(m):
    return m.__dict__.get("_modules") or {}


def child(m, name):
    c = children(m).get(name)
    if c is None:
        raise ValueError(f"{kind(m)} has no child module {name!r}")
    return c


def tensor(m, name, required=True):
    for table in ("_parameters", "_buffers"):
        t = (m.__dict__.get(table) or {}).get(name)
        if t is not None:
            return t.detach().float()
    t = m.__dict__.get(name)
    if isinstance(t, torch.Tensor):
        return t.detach().float()
    if required:
        raise ValueError(f"{kind(m)} has no tensor {name!r}")
    return None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class _ConvOp:
    """One convolution (a Conv2d / ConvTranspose2d, with a BatchNorm folded in) and its activation, as F.conv2d arguments."""

    def __init__(self, conv, bn, act, device, transposed=False):
        w, b = tensor(conv, "weight").double(), tensor(conv, "bias", required=False)
        b = None if b is None else b.double()
        if bn is not None:
            s = tensor(bn, "weight").double() / torch.sqrt(tensor(bn, "running_var").double() + float(bn.eps))
            shift = tensor(bn, "bias").double() - tensor(bn, "running_mean").double() * s
            w = w * s.view(-1, 1, 1, 1)
            b = shift if b is None else b * s + shift
        self.w = w.float().to(device).contiguous()
        self.b = None if b is None else b.float().to(device).contiguous()
        self.stride, self.dilation, self.groups = _pair(conv.stride), _pair(getattr(conv, "dilation", 1)), int(getattr(conv, "groups", 1))
        self.padding = conv.padding if isinstance(conv.padding, str) else _pair(conv.padding)
        self.transposed = transposed
        self.output_padding = _pair(getattr(conv, "output_padding", 0))
        if act is None or kind(act) == "Identity":
            self.act = None
        elif kind(act) == "SiLU":
            self.act = F.silu
        else:
            raise ValueError(f"unsupported activation {act.path if isinstance(act, Stub) else kind(act)}")

    def __call__(self, x, act=True):
        if self.transposed:
            y = F.conv_transpose2d(x, self.w, self.b, self.stride, self.padding, self.output_padding, self.groups, self.dilation)
        else:
            y = F.conv2d(x, self.w, self.b, self.stride, self.padding, self.dilation, self.groups)
        return self.act(y) if act and self.act is not None else y


def compile_module(m, device):
    """A callable for module m (a Stub) and everything under it; an unknown type raises and names it."""
    k = kind(m)
    sub = lambda name: compile_module(child(m, name), device)
    if k == "Conv":
        c = children(m)
        return _ConvOp(c["conv"], c.get("bn"), c.get("act"), device)
    if k in ("Conv2d",):
        return _ConvOp(m, None, None, device)
    if k in ("Sequential", "ModuleList"):
        fns = [compile_module(c, device) for c in children(m).values()]

        def seq(x):
            for fn in fns:
                x = fn(x)
            return x
        return seq
    if k == "Silence":
        return lambda x: x
    if k == "RepConvN":
        c1, c2, a = sub("conv1"), sub("conv2"), children(m).get("act")      # SiLU(conv3x3(x) + conv1x1(x)), no identity branch
        if a is not None and kind(a) not in ("Identity", "SiLU"):
            raise ValueError(f"unsupported activation {a.path}")
        if children(m).get("bn") is not None:
            raise ValueError("RepConvN with an identity BatchNorm branch is not supported")
        if a is None or kind(a) == "Identity":
            return lambda x: c1(x) + c2(x)
        return lambda x: F.silu(c1(x) + c2(x))
    if k == "RepBottleneck":
        cv1, cv2, add = sub("cv1"), sub("cv2"), bool(m.add)
        return lambda x: x + cv2(cv1(x)) if add else cv2(cv1(x))
    if k == "RepCSP":
        cv1, cv2, cv3, mm = sub("cv1"), sub("cv2"), sub("cv3"), sub("m")
        return lambda x: cv3(torch.cat((mm(cv1(x)), cv2(x)), 1))
    if k == "RepNCSPELAN4":
        cv1, cv2, cv3, cv4 = sub("cv1"), sub("cv2"), sub("cv3"), sub("cv4")

        def elan(x):
            y = list(cv1(x).chunk(2, 1))
            y.append(cv2(y[-1]))
            y.append(cv3(y[-1]))
            return cv4(torch.cat(y, 1))
        return elan
    if k == "ADown":
        cv1, cv2 = sub("cv1"), sub("cv2")

        def adown(x):
            x = F.avg_pool2d(x, 2, 1, 0, False, True)
            x1, x2 = x.chunk(2, 1)
            return torch.cat((cv1(x1), cv2(F.max_pool2d(x2, 3, 2, 1))), 1)
        return adown
    if k == "MaxPool2d":
        ks, st, pd, dl, ceil = m.kernel_size, m.stride, m.padding, getattr(m, "dilation", 1), bool(getattr(m, "ceil_mode", False))
        return lambda x: F.max_pool2d(x, ks, st, pd, dl, ceil)
    if k == "SPPELAN":
        cv1, pools, cv5 = sub("cv1"), [sub(n) for n in ("cv2", "cv3", "cv4")], sub("cv5")

        def sppelan(x):
            y = [cv1(x)]
            for p in pools:
                y.append(p(y[-1]))
            return cv5(torch.cat(y, 1))
        return sppelan
    if k == "CBLinear":
        conv, c2s = _ConvOp(child(m, "conv"), None, None, device), [int(c) for c in m.c2s]
        return lambda x: conv(x).split(c2s, dim=1)
    if k == "CBFuse":
        idx = [int(i) for i in m.idx]

        def cbfuse(xs):
            size = xs[-1].shape[2:]
            res = [F.interpolate(x[idx[i]], size=size, mode="nearest") for i, x in enumerate(xs[:-1])]
            return torch.sum(torch.stack(res + xs[-1:]), dim=0)
        return cbfuse
    if k == "Concat":
        d = int(m.d)
        return lambda xs: torch.cat(xs, d)
    if k == "Upsample":
        size, scale, mode = m.size, m.scale_factor, m.mode
        if mode != "nearest":
            raise ValueError(f"Upsample mode {mode!r} is not supported (only 'nearest')")
        return lambda x: F.interpolate(x, size=size, scale_factor=scale, mode="nearest")
    if k == "Proto":
        cv1, cv2, cv3 = sub("cv1"), sub("cv2"), sub("cv3")
        up = _ConvOp(child(m, "upsample"), None, None, device, transposed=True)
        return lambda x: cv3(cv2(up(cv1(x))))
    if k == "Segment":
        return _SegmentHead(m, device)
    raise ValueError(f"unsupported module type {m.path if isinstance(m, Stub) else k!r}: the YOLO loader knows Silence, Conv, RepConvN, "
                     "RepBottleneck, RepCSP, RepNCSPELAN4, ADown, SPPELAN, CBLinear, CBFuse, Concat, Upsample and Segment")


class _SegmentHead:
    """Segment's raw outputs: per level (Detect's cat(cv2, cv3) [64 + nc, h, w], cv4 [nm, h, w]) and the protos [nm, H/4, W/4]."""

    def __init__(self, m, device):
        self.nc, self.nm, self.nl = int(m.nc), int(m.nm), int(m.nl)
        if int(getattr(m, "reg_max", GSR_YOLO_REG_MAX)) != GSR_YOLO_REG_MAX:
            raise ValueError(f"Segment.reg_max is {m.reg_max}; only {GSR_YOLO_REG_MAX} is supported")
        if not 1 <= self.nl <= GSR_YOLO_MAX_LEVELS:
            raise ValueError(f"Segment has {self.nl} levels; 1 to {GSR_YOLO_MAX_LEVELS} are supported")
        dfl = children(m).get("dfl")
        if dfl is not None and kind(dfl) == "DFL":
            w = tensor(child(dfl, "conv"), "weight").flatten()
            if not torch.equal(w, torch.arange(GSR_YOLO_REG_MAX, dtype=torch.float32)):
                raise ValueError("Segment.dfl's weights are not 0 .. 15: the decode assumes the fixed DFL expectation")
        self.stride = [float(s) for s in tensor(m, "stride").flatten()]
        if len(self.stride) != self.nl or min(self.stride) <= 0:
            raise ValueError(f"Segment.stride {self.stride} does not give a positive stride per level (was the model built?)")
        self.proto = compile_module(child(m, "proto"), device)
        self.cv2 = [compile_module(c, device) for c in children(child(m, "cv2")).values()]
        self.cv3 = [compile_module(c, device) for c in children(child(m, "cv3")).values()]
        self.cv4 = [compile_module(c, device) for c in children(child(m, "cv4")).values()]

    def __call__(self, xs):
        proto = self.proto(xs[0])[0].contiguous()
        heads = [(torch.cat((self.cv2[l](xs[l]), self.cv3[l](xs[l])), 1)[0].contiguous(), self.cv4[l](xs[l])[0].contiguous())
                 for l in range(self.nl)]
        return heads, proto


class Segmentation(NamedTuple):
    mask: torch.Tensor            # [H, W] uint8: the union of the kept instance masks
    dets: torch.Tensor            # [max_det * len(classes), 7 + nm]: x1 y1 x2 y2 score class anchor coefficients (rows past counts[0] unused)
    counts: torch.Tensor          # int32 [3]: detections, candidates, NMS survivors before max_det


def check_size(height, width):
    if height % 32 or width % 32 or height <= 0 or width <= 0:
        raise ValueError(f"a {width}x{height} image: YOLO takes a tensor source as it is, so both sides must be multiples of 32 "
                         "(letterboxing other sizes is not supported)")


class YoloSeg:
    """A YOLO instance-segmentation model on one device: ``seg(image, classes, motion)`` runs the network on a [3, H, W] image in [0, 1]
    and folds the union of the instance masks of the requested COCO classes into ``motion`` (motion &= ~yolo)."""

    _loaded = {}                  # pretrained.load_once: a checkpoint is read once per process

    def __init__(self, model, device="cuda:0", conf=CONF, iou=IOU, max_det=MAX_DET):
        self.device = torch.device(device)
        self.conf, self.iou, self.max_det = float(conf), float(iou), int(max_det)
        layers = list(children(child(model, "model")).values())
        if not layers:
            raise ValueError("the model has no layers")
        self.layers, refs = [], set()
        for n, layer in enumerate(layers):
            f, i = layer.f, int(getattr(layer, "i", n))
            if i != n:
                raise ValueError(f"layer {n} says it is layer {i}")
            for j in ([f] if isinstance(f, int) else list(f)):
                if j != -1:
                    refs.add(j if j >= 0 else n + j)
            self.layers.append((f if isinstance(f, int) else [int(j) for j in f], i, compile_module(layer, self.device)))
        self.save = refs
        head = self.layers[-1][2]
        if not isinstance(head, _SegmentHead):
            raise ValueError(f"the last layer is {kind(layers[-1])}, not a Segment head")
        self.head = head
        self.nc, self.nm, self.stride = head.nc, head.nm, head.stride
        self._ws = {}
        self.frames = 0

    @classmethod
    def from_checkpoint(cls, path, device="cuda:0", **kw):
        def build(path):
            ckpt = load_checkpoint(path)
            if not isinstance(ckpt, dict):
                raise ValueError(f"{path}: expected an ultralytics checkpoint dict, got {type(ckpt).__name__}")
            model = ckpt.get("ema") or ckpt.get("model")
            if model is None:
                raise ValueError(f"{path}: the checkpoint has neither 'ema' nor 'model'")
            return cls(model, device, **kw)
        return pretrained.load_once(cls._loaded, [path], device, None, build)

    @torch.no_grad()
    def forward(self, image):
        """The network on one image [3, H, W] float in [0, 1]: (per level (head [64 + nc, h, w], coef [nm, h, w]), proto [nm, H/4, W/4])."""
        pretrained.refuse_capture("YoloSeg.forward", "segment frames before capture")
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"expected a [3, H, W] image, got {tuple(image.shape)}")
        check_size(int(image.shape[1]), int(image.shape[2]))
        x = image.to(self.device, torch.float32)[None]
        y = []
        with pretrained.deterministic_convolutions():
            for f, i, fn in self.layers:
                if f != -1:
                    x = y[f] if isinstance(f, int) else [x if j == -1 else y[j] for j in f]
                x = fn(x)
                y.append(x if i in self.save else None)
        return x

    @torch.no_grad()
    def postprocess(self, head_outputs, proto, classes, motion=None):
        """The HIP post-processing of given head tensors: per level (head [64 + nc, h, w], coef [nm, h, w]) and proto [nm, H/4, W/4].
        classes: COCO ids. motion: [H, W] bool on the device, cleared where the union is set (in place), or None."""
        return postprocess(head_outputs, proto, classes, self.stride, motion, self.conf, self.iou, self.max_det, self._ws)

    def __call__(self, image, classes, motion=None):
        heads, proto = self.forward(image)
        out = self.postprocess(heads, proto, classes, motion)
        self.frames += 1
        return out


def postprocess(head_outputs, proto, classes, strides, motion=None, conf=CONF, iou=IOU, max_det=MAX_DET, workspaces=None):
    """The functional form of YoloSeg.postprocess (strides: the level strides in pixels)."""
    pretrained.refuse_capture("yolo postprocess", "segment frames before capture")
    classes = sorted({int(c) for c in classes})
    nl = len(head_outputs)
    if not classes or nl != len(strides) or not 1 <= nl <= GSR_YOLO_MAX_LEVELS:
        raise ValueError(f"need at least one class and one stride per level ({nl} levels, {len(strides)} strides)")
    nm, ph, pw = (int(s) for s in proto.shape)
    H, W = 4 * ph, 4 * pw
    check_size(H, W)
    _C.dev_ptr(proto, "proto", _C.F32)
    nc = int(head_outputs[0][0].shape[0]) - 4 * GSR_YOLO_REG_MAX
    hw, heads, coefs = [], [], []
    for l, (h, c) in enumerate(head_outputs):
        _, lh, lw = (int(s) for s in h.shape)
        heads.append(_C.dev_ptr(h, f"head[{l}]", _C.F32, (4 * GSR_YOLO_REG_MAX + nc, lh, lw)))
        coefs.append(_C.dev_ptr(c, f"coef[{l}]", _C.F32, (nm, lh, lw)))
        hw += [lh, lw]
    anchors = sum(hw[2 * l] * hw[2 * l + 1] for l in range(nl))
    if anchors > GSR_YOLO_MAX_ANCHORS:
        raise ValueError(f"{anchors} anchors: at most {GSR_YOLO_MAX_ANCHORS} are supported")
    dev = proto.device
    L = _C.load_library()
    ws = pretrained.workspace(workspaces, (anchors, dev), L.gsr_yolo_workspace_size(anchors), dev)
    max_dets = max_det * len(classes)
    dets = torch.empty((max_dets, GSR_YOLO_DET_HEAD + nm), dtype=torch.float32, device=dev)
    counts = torch.empty(3, dtype=torch.int32, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    if motion is not None:
        _C._require_device(motion, "motion")
        if motion.dtype not in (torch.bool, torch.uint8) or not motion.is_contiguous() or tuple(motion.shape) != (H, W):
            raise RuntimeError(f"motion must be a contiguous bool [{H}, {W}] device tensor, got {motion.dtype} {tuple(motion.shape)}")
    with torch.cuda.device(dev):
        s = _C._stream(dev)
        L.gsr_yolo_detect(nl, (C.c_int * (2 * nl))(*hw), (C.c_float * nl)(*[float(x) for x in strides]), (C.c_void_p * nl)(*heads),
                          (C.c_void_p * nl)(*coefs), nc, nm, (C.c_int * len(classes))(*classes), len(classes), float(conf), float(iou),
                          int(max_det), ws.data_ptr(), dets.data_ptr(), max_dets, counts.data_ptr(), s)
        L.gsr_yolo_masks(max_dets, dets.data_ptr(), counts.data_ptr(), nm, proto.data_ptr(), ph, pw, H, W, mask.data_ptr(),
                         None if motion is None else motion.data_ptr(), s)
    return Segmentation(mask, dets, counts)


def masks_from_dets(dets, counts, proto, motion=None):
    """gsr_yolo_masks alone: the union of the instance masks of given detection rows (dets [n, 7 + nm], counts int32 [>= 1] on the device)."""
    nm, ph, pw = (int(s) for s in proto.shape)
    H, W = 4 * ph, 4 * pw
    check_size(H, W)
    _C.dev_ptr(proto, "proto", _C.F32)
    _C.dev_ptr(dets, "dets", _C.F32, (int(dets.shape[0]), GSR_YOLO_DET_HEAD + nm))
    mask = torch.empty((H, W), dtype=torch.uint8, device=proto.device)
    with torch.cuda.device(proto.device):
        _C.load_library().gsr_yolo_masks(int(dets.shape[0]), dets.data_ptr(), counts.data_ptr(), nm, proto.data_ptr(), ph, pw, H, W,
                                          mask.data_ptr(), None if motion is None else motion.data_ptr(), _C._stream(proto.device))
    return mask


# ---- which classes a dataset segments (utils/dataset.py:315, 340-373, 536-547, 612-650) --------------------------------------------
def dataset_classes(kind_name, dataset_config, has_mask_files):
    """The COCO classes the reference's loader of this kind segments, or None when it runs no YOLO. 'tum' (TUM, Bonn): person, plus
    chair when the key seg_chair is present (whatever its value); the file masks are ORed in as well. 'CoFusion': no YOLO when
    mask_colour/*.png exist; otherwise person, plus clock if seg_clock and teddy bear if seg_teddy are true."""
    d = dataset_config
    if kind_name == "tum":
        return [PERSON] + ([CHAIR] if "seg_chair" in d else [])
    if kind_name == "CoFusion":
        if has_mask_files:
            return None
        return [PERSON] + ([CLOCK] if d.get("seg_clock", False) else []) + ([TEDDY_BEAR] if d.get("seg_teddy", False) else [])
    raise ValueError(f"unknown dataset type {kind_name!r}")
