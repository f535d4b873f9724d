"""Optical flow for the dynamic mapping's flow term: RAFT (Teed & Deng, ECCV 2020) in the configuration the reference calls
(utils/camera_utils.py:368-417 generate_flow: RAFT-basic, 20 iterations, test mode, 'sintel' padding), in inference only.

The RAFT-specific hot path is HIP (include/optical_flow.h, csrc/gs_raft.h): the all-pairs correlation pyramid of both directions from
one product on the matrix cores, the 9x9 window lookup of every iteration, and the convex upsampling with the unpad crop and the NDC
scaling. The convolutions of the two encoders and of the update block are torch.nn.functional.conv2d (MIOpen) in fp32.

The network is written here as functions over a flat parameter table whose names and shapes are those of the reference's RAFT
state_dict (179 entries), so the published raft-things.pth loads unchanged. ``RaftFlow.pair`` computes both directions of a pair with
one correlation product and the two directions batched through the update block; each image's encoder outputs are cached (bounded,
by the caller's key), so a keyframe that appears in two pairs is encoded once.

``GmaFlow`` is the reference's second estimator, GMA (Jiang et al., ICCV 2021; GMA/network.py RAFTGMA as utils/camera_utils.py:372-373
would call it: one head, content-only attention): RAFT plus an attention over all low-resolution pixels of image 1's context features,
computed once per pair, with which every iteration aggregates the motion features globally (motion + gamma * attn @ to_v(motion)) as a
third input of the GRU. The attention and the aggregation are HIP (csrc/gs_gma.h); everything else is RaftFlow's code, which GmaFlow
parametrises by its parameter table and two hooks."""
import collections
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import _C
from . import pretrained

LEVELS, RADIUS, HDIM, CDIM, ITERS = 4, 4, 128, 128, 20
CORR_CHANNELS = LEVELS * (2 * RADIUS + 1) ** 2          # 324
MASK_CHANNELS = 9 * 64                                  # 576
NORM_EPS = 1e-5                                         # nn.InstanceNorm2d / nn.BatchNorm2d defaults


# ---- the parameter table -------------------------------------------------------------------------------------------------------------
def _norm_entries(name, ch, norm):
    if norm == "batch":
        return [(f"{name}.weight", (ch,)), (f"{name}.bias", (ch,)), (f"{name}.running_mean", (ch,)), (f"{name}.running_var", (ch,)),
                (f"{name}.num_batches_tracked", ())]
    return []                                           # instance norm without affine parameters or running statistics


def _conv_entries(name, cout, cin, kh, kw=None):
    return [(f"{name}.weight", (cout, cin, kh, kh if kw is None else kw)), (f"{name}.bias", (cout,))]


def _encoder_entries(prefix, norm, out_dim):
    """BasicEncoder: 7x7/2 stem (64), three stages of two residual blocks (64, 96/2, 128/2), 1x1 head; in state_dict order (the stem's
    norm before its convolution; a block's convolutions, its norms, then its projection shortcut, whose norm is registered both as norm3
    and as downsample.1)."""
    e = _norm_entries(f"{prefix}.norm1", 64, norm) + _conv_entries(f"{prefix}.conv1", 64, 3, 7)
    cin = 64
    for s, (ch, stride) in enumerate(((64, 1), (96, 2), (128, 2)), start=1):
        for b in range(2):
            blk = f"{prefix}.layer{s}.{b}"
            st = stride if b == 0 else 1
            e += _conv_entries(f"{blk}.conv1", ch, cin, 3) + _conv_entries(f"{blk}.conv2", ch, ch, 3)
            e += _norm_entries(f"{blk}.norm1", ch, norm) + _norm_entries(f"{blk}.norm2", ch, norm)
            if st != 1:
                e += _norm_entries(f"{blk}.norm3", ch, norm)
                e += _conv_entries(f"{blk}.downsample.0", ch, cin, 1) + _norm_entries(f"{blk}.downsample.1", ch, norm)
            cin = ch
    return e + _conv_entries(f"{prefix}.conv2", out_dim, 128, 1)


def _entries(gru_extra):
    """RAFT-basic's entries; the GRU's input is hidden + context + motion (+ gru_extra: GMA's aggregated motion) channels wide."""
    u = "update_block"
    e = _encoder_entries("fnet", "instance", 256) + _encoder_entries("cnet", "batch", HDIM + CDIM)
    e += (_conv_entries(f"{u}.encoder.convc1", 256, CORR_CHANNELS, 1) + _conv_entries(f"{u}.encoder.convc2", 192, 256, 3)
          + _conv_entries(f"{u}.encoder.convf1", 128, 2, 7) + _conv_entries(f"{u}.encoder.convf2", 64, 128, 3)
          + _conv_entries(f"{u}.encoder.conv", 128 - 2, 64 + 192, 3))
    for d, (kh, kw) in (("1", (1, 5)), ("2", (5, 1))):
        for g in "zrq":
            e += _conv_entries(f"{u}.gru.conv{g}{d}", HDIM, HDIM + 128 + HDIM + gru_extra, kh, kw)
    e += _conv_entries(f"{u}.flow_head.conv1", 256, HDIM, 3) + _conv_entries(f"{u}.flow_head.conv2", 2, 256, 3)
    e += _conv_entries(f"{u}.mask.0", 256, 128, 3) + _conv_entries(f"{u}.mask.2", MASK_CHANNELS, 256, 1)
    return e


def param_shapes():
    """name -> shape of every entry of RAFT-basic's state_dict, in its order."""
    return collections.OrderedDict(_entries(0))


GMA_MAX_POS = 160                                       # RAFTGMA's Attention(max_pos_size=160): the size of the unused pos_emb tables
GMA_QK_GAIN = 105.0                                     # gma_recipe_state_dict: see there


def gma_param_shapes():
    """name -> shape of every entry of RAFTGMA's state_dict (GMA/network.py), in its order: RAFT-basic's names with a GRU 128 channels
    wider, then the aggregator (gamma before to_v: a module's own parameters precede its children's) and the attention. The pos_emb
    entries are in every GMA checkpoint but unused (position_only and position_and_content are hard-coded off)."""
    e = _entries(128)
    e += [("update_block.aggregator.gamma", (1,)), ("update_block.aggregator.to_v.weight", (128, 128, 1, 1)),
          ("att.to_qk.weight", (2 * CDIM, CDIM, 1, 1)), ("att.pos_emb.rel_ind", (GMA_MAX_POS, GMA_MAX_POS)),
          ("att.pos_emb.rel_height.weight", (2 * GMA_MAX_POS - 1, CDIM)), ("att.pos_emb.rel_width.weight", (2 * GMA_MAX_POS - 1, CDIM))]
    return collections.OrderedDict(e)


def recipe_state_dict(seed=0):
    """Seeded stand-in weights (no checkpoint needed to build or test): per entry a generator pretrained.entry_rng(seed, name);
    conv weights U(+-sqrt(1 / fan_in)), norm weights U(0.8, 1.2), other vectors U(+-0.05), running_mean U(+-0.1), running_var
    U(0.5, 1.5), num_batches_tracked 0. Flows from them are finite and mostly inside the image, but carry no meaning."""
    return _recipe(param_shapes(), seed)


def _recipe(shapes, seed):
    out = collections.OrderedDict()
    for name, shape in shapes.items():
        rng = pretrained.entry_rng(seed, name)
        if name.endswith("num_batches_tracked"):
            out[name] = torch.tensor(0, dtype=torch.int64)
            continue
        if len(shape) == 4:
            b = math.sqrt(1.0 / (shape[1] * shape[2] * shape[3]))
            v = rng.uniform(-b, b, shape)
        elif name.endswith("running_mean"):
            v = rng.uniform(-0.1, 0.1, shape)
        elif name.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif name.endswith(".weight"):
            v = rng.uniform(0.8, 1.2, shape)
        else:
            v = rng.uniform(-0.05, 0.05, shape)
        out[name] = torch.from_numpy(v.astype(np.float32))
    return out


def gma_recipe_state_dict(seed=0):
    """recipe_state_dict's rules for gma_param_shapes(), with two exceptions without which the stand-in would exercise nothing:
    aggregator.gamma ~ U(0.5, 1.5) (the module initialises it to 0, which switches the aggregation off), and att.to_qk.weight is its
    U(+-sqrt(1 / 128)) draw times GMA_QK_GAIN: with the plain draw every attention row is uniform to three digits; with the gain the
    reference's rows on the fixture images are peaked but not one-hot (mean row entropy / log N in [0.3, 0.8]; tests/golden/
    make_golden_gma.py asserts it). pos_emb.rel_ind is the module's own index table."""
    out = _recipe(gma_param_shapes(), seed)
    out["update_block.aggregator.gamma"] = torch.from_numpy(
        pretrained.entry_rng(seed, "update_block.aggregator.gamma").uniform(0.5, 1.5, (1,)).astype(np.float32))
    out["att.to_qk.weight"] = out["att.to_qk.weight"] * GMA_QK_GAIN
    r = torch.arange(GMA_MAX_POS)
    out["att.pos_emb.rel_ind"] = r.view(1, -1) - r.view(-1, 1) + GMA_MAX_POS - 1
    return out


def check_state_dict(sd):
    """Strip DataParallel's `module.` prefix and check the entries against param_shapes(): a missing, extra or misshapen entry raises
    and names it. Returns the stripped dict."""
    sd = pretrained.strip_module_prefix(sd, "RAFT checkpoint")
    if any(".conv3." in k for k in sd) or tuple(getattr(sd.get("update_block.encoder.convc1.weight"), "shape", ())) == (96, 196, 1, 1):
        raise ValueError("this is a RAFT-small checkpoint; only RAFT-basic (raft-things.pth and its kind) is supported")
    pretrained.check_entries(sd, param_shapes(), "RAFT checkpoint")
    return sd


def check_gma_state_dict(sd):
    """check_state_dict for a GMA checkpoint (gma-things.pth and its kind) against gma_param_shapes(), the unused pos_emb entries
    included. A RAFT-basic checkpoint raises with a message that says so."""
    sd = pretrained.strip_module_prefix(sd, "GMA checkpoint")
    if not any(k.startswith(("att.", "update_block.aggregator.")) for k in sd) and "update_block.gru.convz1.weight" in sd:
        raise ValueError("this is a RAFT checkpoint (it has no attention or aggregator entries), not a GMA one: load it with RaftFlow "
                         "(tools/run_slam.py --raft-weights)")
    pretrained.check_entries(sd, gma_param_shapes(), "GMA checkpoint")
    return sd


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def pad_amounts(height, width):
    """InputPadder 'sintel' mode (RAFT/utils/utils.py): replicate padding to a multiple of 8, split evenly with the odd pixel after.
    Returns (left, right, top, bottom)."""
    ph = ((height // 8 + 1) * 8 - height) % 8
    pw = ((width // 8 + 1) * 8 - width) % 8
    return pw // 2, pw - pw // 2, ph // 2, ph - ph // 2


def check_size(height, width):
    """Every pyramid level needs at least 2 x 2 cells: bilinear_sampler divides by (H - 1) and (W - 1) of each level, so a level of
    height or width 1 yields NaN in the reference. Raises ValueError below that (padded size under 128 in either direction)."""
    l, r, t, b = pad_amounts(height, width)
    hp, wp = height + t + b, width + l + r
    if hp // 64 < 2 or wp // 64 < 2:
        raise ValueError(f"a {width}x{height} image pads to {wp}x{hp}: RAFT needs a padded size of at least 128x128 "
                         f"(the coarsest correlation level would have a side of 1)")
    return hp, wp


def attention_bytes(height, width, batch=2):
    """The bytes of GMA's attention for `batch` directions of a height x width image: batch * N^2 * 4 with N the low-resolution pixel
    count of the padded image."""
    l, r, t, b = pad_amounts(height, width)
    n = ((height + t + b) // 8) * ((width + l + r) // 8)
    return batch * n * n * 4


# ---- kernels (ctypes binding of include/optical_flow.h) -------------------------------------------------------------------------------
def level_sizes(h, w):
    out = []
    for _ in range(LEVELS):
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


def corr_pyramid(fmap1, fmap2, both=True):
    """The correlation pyramid of fmaps [D, h, w]: a list of LEVELS tensors [2 (or 1), h*w, h_l, w_l]; index 0 is 1->2 (row: a pixel of
    image 1, grid: image 2), index 1 is 2->1. One launch of the product for both directions, one per pooled level."""
    D, h, w = (int(s) for s in fmap1.shape)
    _C.dev_ptr(fmap1, "fmap1", _C.F32, (D, h, w))
    _C.dev_ptr(fmap2, "fmap2", _C.F32, (D, h, w))
    nd = 2 if both else 1
    levels = [torch.empty((nd, h * w, hl, wl), dtype=torch.float32, device=fmap1.device) for hl, wl in level_sizes(h, w)]
    p12 = (C.c_void_p * LEVELS)(*[t[0].data_ptr() for t in levels])
    p21 = (C.c_void_p * LEVELS)(*[t[1].data_ptr() for t in levels]) if both else None
    with torch.cuda.device(fmap1.device):
        _C.load_library().gsr_raft_corr_pyramid(D, h, w, fmap1.data_ptr(), fmap2.data_ptr(), p12, p21, _C._stream(fmap1.device))
    return levels


def corr_lookup(levels, coords, out=None):
    """CorrBlock.__call__: coords [B, 2, h, w] (B = the pyramid's direction count) -> [B, 324, h, w]."""
    B, _, h, w = (int(s) for s in coords.shape)
    if B != int(levels[0].shape[0]) or tuple(levels[0].shape[1:]) != (h * w, h, w):
        raise RuntimeError(f"coords {tuple(coords.shape)} do not match the pyramid {tuple(levels[0].shape)}")
    _C.dev_ptr(coords, "coords", _C.F32, (B, 2, h, w))
    for t in levels:
        _C.dev_ptr(t, "pyramid level", _C.F32)
    if out is None:
        out = torch.empty((B, CORR_CHANNELS, h, w), dtype=torch.float32, device=coords.device)
    _C.dev_ptr(out, "out", _C.F32, (B, CORR_CHANNELS, h, w))
    ptrs = (C.c_void_p * (B * LEVELS))(*[levels[l][b].data_ptr() for b in range(B) for l in range(LEVELS)])
    with torch.cuda.device(coords.device):
        _C.load_library().gsr_raft_corr_lookup(B, h, w, ptrs, coords.data_ptr(), out.data_ptr(), _C._stream(coords.device))
    return out


def upsample(flow, mask, pad, out_hw, ndc=True):
    """RAFT.upsample_flow + InputPadder.unpad (+ flow / (W, H) * 2 with ndc): flow [B, 2, h, w], mask [B, 576, h, w], pad = (left, right,
    top, bottom), out_hw = (H, W) unpadded -> [B, H, W, 2]."""
    B, _, h, w = (int(s) for s in flow.shape)
    H, W = (int(s) for s in out_hw)
    _C.dev_ptr(flow, "flow", _C.F32, (B, 2, h, w))
    _C.dev_ptr(mask, "mask", _C.F32, (B, MASK_CHANNELS, h, w))
    out = torch.empty((B, H, W, 2), dtype=torch.float32, device=flow.device)
    with torch.cuda.device(flow.device):
        _C.load_library().gsr_raft_upsample(B, h, w, flow.data_ptr(), mask.data_ptr(), int(pad[0]), int(pad[2]), W, H, int(bool(ndc)),
                                            out.data_ptr(), _C._stream(flow.device))
    return out


def gma_attention(q, k, scale, out=None):
    """GMA's attention: q, k [B, D, h, w] (B = 1 or 2) -> softmax_j(sum_c (scale q[b, c, i]) k[b, c, j]) as [B, N, N], N = h * w."""
    B, D, h, w = (int(s) for s in q.shape)
    _C.dev_ptr(q, "q", _C.F32, (B, D, h, w))
    _C.dev_ptr(k, "k", _C.F32, (B, D, h, w))
    N = h * w
    if out is None:
        out = torch.empty((B, N, N), dtype=torch.float32, device=q.device)
    _C.dev_ptr(out, "attn", _C.F32, (B, N, N))
    with torch.cuda.device(q.device):
        _C.load_library().gsr_gma_attention(B, D, h, w, q.data_ptr(), k.data_ptr(), float(scale), out.data_ptr(), _C._stream(q.device))
    return out


def gma_aggregate(attn, v, x, gamma, out=None):
    """GMA's aggregation: x + gamma * (attn @ v over the pixels); attn [B, N, N], v and x [B, D, h, w] -> [B, D, h, w]."""
    B, D, h, w = (int(s) for s in x.shape)
    _C.dev_ptr(attn, "attn", _C.F32, (B, h * w, h * w))
    _C.dev_ptr(v, "v", _C.F32, (B, D, h, w))
    _C.dev_ptr(x, "x", _C.F32, (B, D, h, w))
    if out is None:
        out = torch.empty_like(x)
    _C.dev_ptr(out, "out", _C.F32, (B, D, h, w))
    with torch.cuda.device(x.device):
        _C.load_library().gsr_gma_aggregate(B, D, h, w, attn.data_ptr(), v.data_ptr(), x.data_ptr(), float(gamma), out.data_ptr(),
                                            _C._stream(x.device))
    return out


# ---- the network ---------------------------------------------------------------------------------------------------------------------
class RaftFlow:
    """RAFT-basic inference (hidden = context = 128, 4 levels, radius 4, 20 iterations) on one device."""

    _loaded = {}                  # pretrained.load_once: a checkpoint is read once per process
    _check = staticmethod(check_state_dict)

    def __init__(self, state_dict, device="cuda:0", cache_frames=8):
        sd = self._check(state_dict)
        self.device = torch.device(device)
        # the projection shortcut's norm is one module under two names; loading a state_dict leaves it with downsample.1's values
        self.p = {k: v.detach().to(self.device, torch.float32 if v.is_floating_point() else v.dtype).contiguous() for k, v in sd.items()}
        self.cache_frames = max(2, int(cache_frames))
        self._enc = collections.OrderedDict()     # key -> (fmap [256,h,w], net [128,h,w], inp [128,h,w]) of one padded image
        self.encoder_runs = 0
        self.pairs = 0

    @classmethod
    def from_checkpoint(cls, path, device="cuda:0", **kw):
        def build(path):
            sd = torch.load(path, map_location="cpu", weights_only=True)
            return cls(pretrained.strip_module_prefix(sd, path), device, **kw)
        return pretrained.load_once(cls._loaded, [path], device, None, build)

    # -- encoders
    def _norm(self, x, name, kind):
        if kind == "instance":
            return F.instance_norm(x, eps=NORM_EPS)
        p = self.p
        return F.batch_norm(x, p[name + ".running_mean"], p[name + ".running_var"], p[name + ".weight"], p[name + ".bias"], False, 0.0, NORM_EPS)

    def _conv(self, x, name, stride=1, padding=0):
        return F.conv2d(x, self.p[name + ".weight"], self.p[name + ".bias"], stride, padding)

    def _encoder(self, x, prefix, kind):
        x = F.relu(self._norm(self._conv(x, f"{prefix}.conv1", 2, 3), f"{prefix}.norm1", kind))
        for s, stride in ((1, 1), (2, 2), (3, 2)):
            for b in range(2):
                blk = f"{prefix}.layer{s}.{b}"
                st = stride if b == 0 else 1
                y = F.relu(self._norm(self._conv(x, f"{blk}.conv1", st, 1), f"{blk}.norm1", kind))
                y = F.relu(self._norm(self._conv(y, f"{blk}.conv2", 1, 1), f"{blk}.norm2", kind))
                if st != 1:
                    x = self._norm(self._conv(x, f"{blk}.downsample.0", st, 0), f"{blk}.downsample.1", kind)
                x = F.relu(x + y)
        return self._conv(x, f"{prefix}.conv2")

    def _prepare(self, image):
        """generate_flow's input: image * 255 (the float keyframe image), replicate-padded ('sintel'), then RAFT's 2 (x / 255) - 1."""
        if image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"expected a [3, H, W] image, got {tuple(image.shape)}")
        H, W = int(image.shape[1]), int(image.shape[2])
        check_size(H, W)
        self._admit(H, W)
        x = image.to(self.device, torch.float32)[None] * 255
        x = F.pad(x, list(pad_amounts(H, W)), mode="replicate")
        return 2 * (x / 255.0) - 1.0

    def encode(self, image, key=None):
        """(fmap, net, inp, (H, W)) of one image, from the cache when `key` was encoded before (then `image` may be None)."""
        if key is not None and key in self._enc:
            self._enc.move_to_end(key)
            return self._enc[key]
        if image is None:
            raise KeyError(f"no image given and {key!r} is not in the encoder cache")
        x = self._prepare(image)
        fmap = self._encoder(x, "fnet", "instance")[0].contiguous()
        net, inp = torch.split(self._encoder(x, "cnet", "batch")[0], [HDIM, CDIM], dim=0)
        hit = (fmap, torch.tanh(net).contiguous(), torch.relu(inp).contiguous(), (int(image.shape[1]), int(image.shape[2])))
        self.encoder_runs += 1
        if key is not None:
            self._enc[key] = hit
            while len(self._enc) > self.cache_frames:
                self._enc.popitem(last=False)
        return hit

    def forget(self, key):
        self._enc.pop(key, None)

    # -- what GmaFlow adds: nothing here
    def _admit(self, H, W):
        """Called with an image's size before anything is allocated for it."""

    def _attention(self, inp, trace):
        """Per pair, from the stacked context features inp [2, 128, h, w]: what _motion_inputs receives in every iteration."""
        return None

    def _motion_inputs(self, motion, attention, trace):
        """The motion features' part of the GRU's input, as a tuple of [B, *, h, w] tensors."""
        return (motion,)

    # -- update block
    def _update(self, net, inp, corr, flow, with_mask, attention=None, trace=None):
        u = "update_block"
        c = F.relu(self._conv(corr, f"{u}.encoder.convc1"))
        c = F.relu(self._conv(c, f"{u}.encoder.convc2", 1, 1))
        f = F.relu(self._conv(flow, f"{u}.encoder.convf1", 1, 3))
        f = F.relu(self._conv(f, f"{u}.encoder.convf2", 1, 1))
        motion = torch.cat([F.relu(self._conv(torch.cat([c, f], 1), f"{u}.encoder.conv", 1, 1)), flow], 1)
        x = torch.cat([inp, *self._motion_inputs(motion, attention, trace)], 1)
        h = net
        for d, pad in (("1", (0, 2)), ("2", (2, 0))):          # the separable GRU: a 1x5 pass, then a 5x1 pass
            hx = torch.cat([h, x], 1)
            z = torch.sigmoid(self._conv(hx, f"{u}.gru.convz{d}", 1, pad))
            r = torch.sigmoid(self._conv(hx, f"{u}.gru.convr{d}", 1, pad))
            q = torch.tanh(self._conv(torch.cat([r * h, x], 1), f"{u}.gru.convq{d}", 1, pad))
            h = (1 - z) * h + z * q
        delta = self._conv(F.relu(self._conv(h, f"{u}.flow_head.conv1", 1, 1)), f"{u}.flow_head.conv2", 1, 1)
        mask = .25 * self._conv(F.relu(self._conv(h, f"{u}.mask.0", 1, 1)), f"{u}.mask.2") if with_mask else None
        return h, mask, delta

    # -- a pair
    @torch.no_grad()
    def pair(self, image_i, image_j, key_i=None, key_j=None, iters=ITERS, ndc=True, trace=None):
        """RAFT(image1 = image_i, image2 = image_j) and RAFT(image1 = image_j, image2 = image_i): (flow_ij, flow_ji), each [H, W, 2] float32
        on the device, in NDC units (flow / (W, H) * 2, utils/camera_utils.py:412-413) or pixels with ndc=False. Images: [3, H, W] float
        in [0, 1]; an image may be None when its key is in the encoder cache. key_i / key_j name the images for that cache (None: not
        cached). `trace`, a dict, receives the intermediates."""
        pretrained.refuse_capture("RaftFlow.pair", "estimate flows before capture (dynamic_graph fills its flow planes during table setup)")
        with pretrained.deterministic_convolutions():          # the flow targets are cached by pair
            return self._pair(image_i, image_j, key_i, key_j, iters, ndc, trace)

    def _pair(self, image_i, image_j, key_i, key_j, iters, ndc, trace):
        f_i, net_i, inp_i, (H, W) = self.encode(image_i, key_i)
        f_j, net_j, inp_j, hw_j = self.encode(image_j, key_j)
        if hw_j != (H, W):
            raise ValueError(f"the two images differ in size: {W}x{H} vs {hw_j[1]}x{hw_j[0]}")
        pad = pad_amounts(H, W)
        _, h, w = (int(s) for s in f_i.shape)
        levels = corr_pyramid(f_i, f_j, both=True)             # [0]: i -> j, [1]: j -> i
        net = torch.stack([net_i, net_j])
        inp = torch.stack([inp_i, inp_j])
        ys, xs = torch.meshgrid(torch.arange(h, device=self.device), torch.arange(w, device=self.device), indexing="ij")
        coords0 = torch.stack([xs, ys]).float()[None].expand(2, 2, h, w).contiguous()
        coords1 = coords0.clone()
        corr = torch.empty((2, CORR_CHANNELS, h, w), dtype=torch.float32, device=self.device)
        attention = self._attention(inp, trace)
        if trace is not None:
            trace.update(fmap_i=f_i, fmap_j=f_j, net_i=net_i, inp_i=inp_i, net_j=net_j, inp_j=inp_j, pyramid=levels)
        mask = None
        for it in range(iters):
            corr_lookup(levels, coords1, corr)
            flow = coords1 - coords0
            net, mask, delta = self._update(net, inp, corr, flow, it == iters - 1, attention, trace if it == 0 else None)
            coords1 = coords1 + delta
            if trace is not None and it == 0:
                trace.update(corr1=corr.clone(), flow1=(coords1 - coords0).clone())
        flow = (coords1 - coords0).contiguous()
        if trace is not None:
            trace["flow_low"] = flow
        up = upsample(flow, mask.contiguous(), pad, (H, W), ndc=ndc)
        self.pairs += 1
        return up[0], up[1]


class GmaFlow(RaftFlow):
    """GMA inference (RAFT-basic plus one-head content attention and global motion aggregation, 20 iterations) on one device: RaftFlow's
    interface and behaviour (pair, encode, forget, from_checkpoint, the encoder cache and its counters) with a GMA checkpoint. The
    attention of a pair, [2, N, N] float32, is computed once from the cached context features and lives for that pair only; a pair whose
    attention would exceed max_attention_bytes raises ValueError before anything is allocated for it."""

    _loaded = {}
    _check = staticmethod(check_gma_state_dict)

    def __init__(self, state_dict, device="cuda:0", cache_frames=8, max_attention_bytes=2 << 30):
        super().__init__(state_dict, device, cache_frames)
        self.max_attention_bytes = int(max_attention_bytes)
        sd = pretrained.strip_module_prefix(state_dict, "GMA checkpoint")
        self.gamma = float(sd["update_block.aggregator.gamma"].detach().reshape(-1)[0])    # read on the host, once: no sync per pair
        self.scale = float(CDIM) ** -0.5                                                    # Attention.scale = dim_head ** -0.5

    def _admit(self, H, W):
        need = attention_bytes(H, W)
        if need > self.max_attention_bytes:
            l, r, t, b = pad_amounts(H, W)
            n = ((H + t + b) // 8) * ((W + l + r) // 8)
            raise ValueError(f"GMA's attention for a {W}x{H} image is 2 x {n} x {n} float32 = {need} bytes, more than max_attention_bytes = "
                             f"{self.max_attention_bytes}")

    def _attention(self, inp, trace):
        qk = F.conv2d(inp, self.p["att.to_qk.weight"])
        attn = gma_attention(qk[:, :CDIM].contiguous(), qk[:, CDIM:].contiguous(), self.scale)
        if trace is not None:
            trace["attention"] = attn
        return attn

    def _motion_inputs(self, motion, attention, trace):
        v = F.conv2d(motion, self.p["update_block.aggregator.to_v.weight"])
        glob = gma_aggregate(attention, v, motion.contiguous(), self.gamma)
        if trace is not None:
            trace["motion_global"] = glob
        return (motion, glob)
