"""The perceptual image metric of the rendering evaluation: LPIPS v0.1 (Zhang et al., CVPR 2018), AlexNet variant, as the reference
calls it (utils/eval_utils.py:314-318, 378: LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True)), in inference only
and without lpips, torchmetrics or torchvision.

For images x, y [B, 3, H, W] in [0, 1]: u = 2 v - 1, the scaling layer (u - shift) / scale, AlexNet's `features` with a tap after each of
its five ReLUs; per tap and pixel both feature vectors are unit-normalised over the channels, the squared difference is weighted by the
non-negative `lin` weights and summed over the channels, then averaged over the tap's pixels; the score is the sum of the five means.

The LPIPS-specific part is HIP (include/perceptual.h, csrc/gs_lpips.h): both images of every pair go into one network batch in one
launch, and the five taps of all pairs are reduced in one launch plus a small one that adds the per-block sums in index order, with no
float atomics and no host round trip. The convolutions, ReLU and max-pool are torch.nn.functional (MIOpen) in fp32. With device="cpu"
the same network runs with a torch stand-in for the two kernels (the host tests); on a GPU there is no such path.

Weights: a torchvision AlexNet state_dict and the LPIPS linear layers, both plain tensor dictionaries; ``recipe_state_dicts`` gives
seeded stand-ins of the same shapes for building and testing without the published files."""
import collections
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C
from diff_gaussian_rasterization._abi import GSR_LPIPS_NORM_LPIPS, GSR_LPIPS_NORM_TORCHMETRICS
from . import pretrained

SHIFT = (-.030, -.088, -.188)                           # LPIPS' ScalingLayer
SCALE = (.458, .448, .450)
# AlexNet.features' convolutions: (index in `features`, out channels, in channels, kernel, stride, padding, max-pool 3x3/2 before it)
CONVS = ((0, 64, 3, 11, 4, 2, False), (3, 192, 64, 5, 1, 2, True), (6, 384, 192, 3, 1, 1, True), (8, 256, 384, 3, 1, 1, False),
         (10, 256, 256, 3, 1, 1, False))
CHANNELS = tuple(c[1] for c in CONVS)
NORMS = {"torchmetrics": GSR_LPIPS_NORM_TORCHMETRICS,   # f / sqrt(1e-8 + sum f^2)
         "lpips": GSR_LPIPS_NORM_LPIPS}                 # f / (sqrt(sum f^2) + 1e-10)
MIN_SIDE = 67                                           # the third tap then still has 3 x 3 pixels


# ---- the parameter tables ------------------------------------------------------------------------------------------------------------
def param_shapes():
    """(AlexNet entries, linear-layer entries): name -> shape, in state_dict order. AlexNet's `classifier.*` is not part of the metric."""
    alex = collections.OrderedDict()
    for idx, cout, cin, k, _, _, _ in CONVS:
        alex[f"features.{idx}.weight"] = (cout, cin, k, k)
        alex[f"features.{idx}.bias"] = (cout,)
    lin = collections.OrderedDict((f"lin{l}.model.1.weight", (1, c, 1, 1)) for l, c in enumerate(CHANNELS))
    return alex, lin


def recipe_state_dicts(seed=0):
    """Seeded stand-in weights (no checkpoint needed to build or test): per entry a generator pretrained.entry_rng(seed, name);
    He-scaled convolutions N(0, 2 / fan_in), biases N(0, 0.1^2), linear weights U[0, 0.5). Scores from them are well-behaved distances
    but carry no perceptual meaning."""
    alex_shapes, lin_shapes = param_shapes()
    alex, lin = collections.OrderedDict(), collections.OrderedDict()
    for name, shape in alex_shapes.items():
        rng = pretrained.entry_rng(seed, name)
        v = rng.standard_normal(shape) * (math.sqrt(2.0 / (shape[1] * shape[2] * shape[3])) if len(shape) == 4 else 0.1)
        alex[name] = torch.from_numpy(v.astype(np.float32))
    for name, shape in lin_shapes.items():
        lin[name] = torch.from_numpy(pretrained.entry_rng(seed, name).uniform(0.0, 0.5, shape).astype(np.float32))
    return alex, lin


def check_state_dicts(alexnet_sd, lin_sd):
    """Strip DataParallel's `module.` prefix, drop AlexNet's `classifier.*`, and check both dictionaries against param_shapes(): a missing,
    extra or misshapen entry raises and names it, and so does a negative linear weight (the metric is not a distance then). Returns the
    stripped pair."""
    alex = pretrained.strip_module_prefix(alexnet_sd, "AlexNet checkpoint")
    alex = {k: v for k, v in alex.items() if not k.startswith("classifier.")}
    lin = pretrained.strip_module_prefix(lin_sd, "LPIPS linear-layer checkpoint")
    alex_shapes, lin_shapes = param_shapes()
    pretrained.check_entries(alex, alex_shapes, "AlexNet checkpoint")
    pretrained.check_entries(lin, lin_shapes, "LPIPS linear-layer checkpoint")
    for k in lin_shapes:
        if not bool((lin[k] >= 0).all()):
            raise ValueError(f"LPIPS linear-layer checkpoint entry {k!r} has a negative weight (min {float(lin[k].min()):g})")
    return alex, lin


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def tap_sizes(height, width):
    """(h, w) of the five taps for an H x W image."""
    def side(n):
        n1 = (n + 2 * 2 - 11) // 4 + 1
        n2 = (n1 - 3) // 2 + 1
        n3 = (n2 - 3) // 2 + 1
        return n1, n2, n3
    hs, ws = side(height), side(width)
    return [(hs[0], ws[0]), (hs[1], ws[1])] + [(hs[2], ws[2])] * 3


def check_size(height, width):
    if height < MIN_SIDE or width < MIN_SIDE:
        raise ValueError(f"a {width}x{height} image: LPIPS needs both sides to be at least {MIN_SIDE} (the deepest taps would have fewer "
                         "than 3 x 3 pixels)")


# ---- kernels (ctypes binding of include/perceptual.h) ---------------------------------------------------------------------------------
def prepare(x, y):
    """gsr_lpips_prepare: x, y [B, 3, H, W] in [0, 1] -> the network batch [2B, 3, H, W] (x's rows, then y's), scaled. One launch."""
    B, _, H, W = (int(s) for s in x.shape)
    _C.dev_ptr(x, "x", _C.F32, (B, 3, H, W))
    _C.dev_ptr(y, "y", _C.F32, (B, 3, H, W))
    out = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _C.load_library().gsr_lpips_prepare(B, H, W, x.data_ptr(), y.data_ptr(), out.data_ptr(), _C._stream(x.device))
    return out


def distance(feats, lins, norm="torchmetrics", workspaces=None):
    """gsr_lpips_distance on given taps: feats[l] [2B, C_l, h_l, w_l] (rows 0 .. B-1 against rows B .. 2B-1), lins[l] [C_l].
    Returns (per-tap means [B, levels], scores [B]) on the device."""
    if len(feats) != len(lins) or not feats:
        raise ValueError(f"{len(feats)} taps and {len(lins)} linear layers")
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
    B = int(feats[0].shape[0]) // 2
    chw = []
    for l, (f, w) in enumerate(zip(feats, lins)):
        n, c, h, wd = (int(s) for s in f.shape)
        _C.dev_ptr(f, f"feats[{l}]", _C.F32, (2 * B, c, h, wd))
        _C.dev_ptr(w, f"lins[{l}]", _C.F32, (c,))
        chw += [c, h, wd]
    nl, dev = len(feats), feats[0].device
    L = _C.load_library()
    chw_c = (C.c_int * len(chw))(*chw)
    ws = pretrained.workspace(workspaces, (B, tuple(chw), dev), L.gsr_lpips_workspace_size(B, nl, chw_c), dev)
    taps = torch.empty((B, nl), dtype=torch.float32, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.gsr_lpips_distance(B, nl, chw_c, (C.c_void_p * nl)(*[f.data_ptr() for f in feats]), (C.c_void_p * nl)(*[w.data_ptr() for w in lins]),
                             NORMS[norm], ws.data_ptr(), taps.data_ptr(), scores.data_ptr(), _C._stream(dev))
    return taps, scores


# ---- the torch stand-ins of the two kernels (device="cpu" only) ---------------------------------------------------------------------
def prepare_torch(x, y):
    shift, scale = (torch.tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (SHIFT, SCALE))
    return (2 * torch.cat((x, y)) - 1 - shift) / scale


def distance_torch(feats, lins, norm="torchmetrics"):
    B = int(feats[0].shape[0]) // 2
    taps = []
    for f, w in zip(feats, lins):
        s = (f * f).sum(1, keepdim=True)
        n = f / (torch.sqrt(s) + 1e-10) if NORMS[norm] == GSR_LPIPS_NORM_LPIPS else f / torch.sqrt(1e-8 + s)
        d = n[:B] - n[B:]
        taps.append((d * d * w.view(1, -1, 1, 1)).sum(1).mean((1, 2)))
    taps = torch.stack(taps, 1)
    return taps, taps.sum(1)


# ---- the metric ----------------------------------------------------------------------------------------------------------------------
class Lpips:
    """LPIPS (AlexNet) on one device: ``lpips(x, y)`` scores image pairs [B, 3, H, W] in [0, 1] and returns [B] on the device."""

    _loaded = {}                  # pretrained.load_once: the checkpoints are read once per process

    def __init__(self, alexnet_state_dict, lin_state_dict, device="cuda:0", norm="torchmetrics"):
        if norm not in NORMS:
            raise ValueError(f"norm must be one of {sorted(NORMS)}, got {norm!r}")
        alex, lin = check_state_dicts(alexnet_state_dict, lin_state_dict)
        self.device, self.norm = torch.device(device), norm
        to = lambda t: t.detach().to(self.device, torch.float32).contiguous()
        self.convs = [(to(alex[f"features.{idx}.weight"]), to(alex[f"features.{idx}.bias"]), stride, pad, pool)
                      for idx, _, _, _, stride, pad, pool in CONVS]
        self.lins = [to(lin[f"lin{l}.model.1.weight"]).reshape(-1) for l in range(len(CHANNELS))]
        self._ws = {}
        self._log = pretrained.EventLog(self.device)
        self.pairs = 0

    @classmethod
    def from_checkpoints(cls, alexnet_path, lin_path, device="cuda:0", norm="torchmetrics"):
        build = lambda *paths: cls(*(torch.load(p, map_location="cpu", weights_only=True) for p in paths), device, norm)
        return pretrained.load_once(cls._loaded, (alexnet_path, lin_path), device, norm, build)

    def features(self, batch):
        """The five taps of the scaled network batch [N, 3, H, W]."""
        taps, x = [], batch
        for w, b, stride, pad, pool in self.convs:
            if pool:
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w, b, stride, pad))
            taps.append(x)
        return taps

    @torch.no_grad()
    def forward(self, x, y, taps=False):
        """The scores [B] of the pairs (x[b], y[b]), on the device and without a host synchronisation; with taps=True also the per-tap
        means [B, 5]."""
        if x.dim() != 4 or x.shape[1] != 3 or x.shape != y.shape:
            raise ValueError(f"expected two [B, 3, H, W] batches of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
        check_size(int(x.shape[2]), int(x.shape[3]))
        x, y = (t.to(self.device, torch.float32).contiguous() for t in (x, y))
        if self.device.type == "cpu":
            means, scores = distance_torch(self.features(prepare_torch(x, y)), self.lins, self.norm)
        else:
            pretrained.refuse_capture("Lpips.forward", "score images outside capture")
            with self._log.timed(count=int(x.shape[0])):
                with pretrained.deterministic_convolutions():
                    feats = [f.contiguous() for f in self.features(prepare(x, y))]
                means, scores = distance(feats, self.lins, self.norm, self._ws)
        self.pairs += int(x.shape[0])
        return (scores, means) if taps else scores

    __call__ = forward

    @property
    def stats(self):
        """Pairs scored and the device ms per pair (network + kernels), from device events around every call. Waits for the last call."""
        t = self._log.summary()
        return {"pairs": self.pairs, "calls": t["calls"], "norm": self.norm, "ms_per_pair": t["ms_per_item"],
                "ms_first_call": t["ms_first"], "ms_per_pair_rest": t["ms_per_item_rest"]}
