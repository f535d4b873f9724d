"""The size query is enough: every entry point whose workspace the host carves stays inside `*_workspace_size` bytes.

The workspace is a slice [lead, lead + size) of a uint8 buffer of lead + size + 65536 bytes filled with 0xA5. After the call every byte before
and after the slice must still be 0xA5, and the outputs must equal, bit for bit, those of the same call on a fresh 256-byte aligned workspace
of size + 4096 bytes. (An overrun at these sizes lands in the owned tail: a wrong layout fails the assertion, it cannot fault.) lead is
256 + 16 for the entry points that align the base themselves, so their base is off its alignment, and 256 for the rest."""
import ctypes
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from diff_gaussian_rasterization import _C, _abi  # noqa: E402
from slam import perceptual, segmentation  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL, TAIL = 0xA5, 65536
ANY_BASE, ALIGNED_BASE = 256 + 16, 256            # lead bytes: the entry point aligns the base itself / takes it as it is
CSR_REG_TRIP = 512                                # csrc/gs_nodes.h: sets of up to 20 trips take the packed route


def _rand(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(DEV).contiguous()


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _check(size, lead, run):
    """run(workspace) -> output tensors. Guarded slice against a fresh workspace."""
    size = int(size)
    assert size > 0
    buf = torch.full((lead + size + TAIL,), FILL, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    got = run(buf[lead:lead + size])
    torch.cuda.synchronize()
    assert bool((buf[:lead] == FILL).all()), "bytes before the workspace were written"
    assert bool((buf[lead + size:] == FILL).all()), "bytes behind the workspace were written"
    fresh = torch.zeros(size + 4096, dtype=torch.uint8, device=DEV)
    assert fresh.data_ptr() % 256 == 0
    want = run(fresh)
    torch.cuda.synchronize()
    assert len(got) == len(want) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(_bits(g), _bits(w)), f"output {k} differs from the call on a fresh workspace"


def _stream():
    return _C._stream(torch.device(DEV))


@pytest.mark.parametrize("M,N,K", [(70, 24, 20), (1, 1, 1)])
def test_dense_wgrad(M, N, K):
    lib = _C.load_library()
    G, X = _rand(M, N, seed=1), _rand(M, K, seed=2)

    def run(ws):
        dW = torch.empty((N, K), dtype=torch.float32, device=DEV)
        lib.gsr_dense_wgrad(M, N, K, G.data_ptr(), N, None, 0, X.data_ptr(), K, dW.data_ptr(), K, ws.data_ptr(), _stream())
        return [dW]

    _check(lib.gsr_dense_wgrad_workspace_size(M, N, K), ANY_BASE, run)


def test_dense_wgrad_many():
    lib = _C.load_library()
    M, shapes = 70, [(24, 20), (256, 64)]
    pairs = [(_rand(M, n, seed=3 + i), _rand(M, k, seed=13 + i)) for i, (n, k) in enumerate(shapes)]

    def items(outs):
        arr = (_abi.gsr_dense_wgrad_item * len(shapes))()
        for it, (G, X), o, (n, k) in zip(arr, pairs, outs, shapes):
            it.G, it.X, it.dW, it.ldg, it.ldx, it.lddw, it.N, it.K = G.data_ptr(), X.data_ptr(), o.data_ptr() if o is not None else None, n, k, k, n, k
        return arr

    def run(ws):
        outs = [torch.empty((n, k), dtype=torch.float32, device=DEV) for n, k in shapes]
        lib.gsr_dense_wgrad_many(M, len(shapes), items(outs), ws.data_ptr(), _stream())
        return outs

    _check(lib.gsr_dense_wgrad_many_workspace_size(M, len(shapes), items([None] * len(shapes))), ANY_BASE, run)


@pytest.mark.parametrize("E", [37, 20 * CSR_REG_TRIP, 20 * CSR_REG_TRIP + 1])       # the packed route up to 20 trips, the plain one above
def test_index_csr_and_segment_sum(E):
    lib = _C.load_library()
    S, Nv, B, C = 2, 5, 3, 4
    idx = torch.randint(0, Nv, (S, E), generator=torch.Generator().manual_seed(E)).to(DEV).contiguous()
    g = _rand(B, E, C, seed=E)
    set_of_b = torch.tensor([0, 1, 1], dtype=torch.int32, device=DEV)

    def run(ws):
        out = torch.empty((B, Nv, C), dtype=torch.float32, device=DEV)
        lib.gsr_index_csr(S, E, Nv, idx.data_ptr(), ws.data_ptr(), _stream())
        lib.gsr_segment_sum(B, S, E, C, Nv, g.data_ptr(), ws.data_ptr(), set_of_b.data_ptr(), out.data_ptr(), _stream())
        return [out]

    _check(lib.gsr_index_csr_workspace_size(S, E, Nv), ANY_BASE, run)


def test_seed_from_rgbd():
    lib = _C.load_library()
    n, W, H = 65, 17, 16
    gen = torch.Generator().manual_seed(7)
    pix = torch.randperm(W * H, generator=gen)[:n].sort()[0].to(torch.int32).to(DEV)
    depth = (1.0 + torch.rand((H, W), generator=gen)).to(DEV)
    image = torch.rand((3, H, W), generator=gen).to(DEV)
    zero = torch.zeros(1, device=DEV)                                  # exposure a, b
    R, T = torch.eye(3, device=DEV).contiguous(), torch.zeros(3, device=DEV)

    def run(ws):
        outs = [torch.empty((n, w), dtype=torch.float32, device=DEV) for w in (3, 3, 3, 4, 1)]      # xyz, features_dc, log_scales, rotations, opacity
        lib.gsr_seed_from_rgbd(n, pix.data_ptr(), W, H, depth.data_ptr(), image.data_ptr(), zero.data_ptr(), zero.data_ptr(), 20.0, 20.0, 8.5, 8.0,
                               R.data_ptr(), T.data_ptr(), 0.05, 3, *[o.data_ptr() for o in outs], ws.data_ptr(), _stream())
        return outs

    _check(lib.gsr_seed_workspace_size(n), ANY_BASE, run)


def test_ssim_forward_and_backward():
    lib = _C.load_library()
    W, H, Cn = 17, 9, 3
    a, b = _rand(Cn, H, W, seed=1).sigmoid().contiguous(), _rand(Cn, H, W, seed=2).sigmoid().contiguous()
    mask = (torch.rand((H, W), generator=torch.Generator().manual_seed(3)) > 0.3).to(torch.uint8).to(DEV)
    upstream = torch.ones((), dtype=torch.float32, device=DEV)

    def run(ws):
        mean = torch.empty((), dtype=torch.float32, device=DEV)
        grad = torch.empty((Cn, H, W), dtype=torch.float32, device=DEV)
        lib.gsr_ssim_forward(W, H, Cn, a.data_ptr(), b.data_ptr(), mask.data_ptr(), mean.data_ptr(), ws.data_ptr(), _stream())
        lib.gsr_ssim_backward(W, H, Cn, a.data_ptr(), b.data_ptr(), mask.data_ptr(), upstream.data_ptr(), grad.data_ptr(), ws.data_ptr(), _stream())
        return [mean, grad]

    _check(lib.gsr_ssim_workspace_size(W, H, Cn), ALIGNED_BASE, run)


def _through_cache(call):
    """call(workspaces) -> outputs, for a wrapper that keeps its workspace in the dict `workspaces`: the key and the size it asks for are
    learned from a first call, then the guarded slice (or the fresh buffer) is put under that key."""
    cache = {}
    call(cache)
    torch.cuda.synchronize()
    (key, first), = cache.items()

    def run(ws):
        cache[key] = ws
        return call(cache)

    return int(first.numel()), run


def test_yolo_detect():
    from test_hip_yolo import STRIDES, _heads, _plants_general
    heads, proto = _heads(480, 640, _plants_general(7), seed=7)

    def call(workspaces):
        res = segmentation.postprocess(heads, proto, [0, 56], STRIDES, workspaces=workspaces)
        n = int(res.counts[0])
        return [res.mask, res.counts, res.dets[:n]]

    size, run = _through_cache(call)
    assert size == _C.load_library().gsr_yolo_workspace_size(80 * 60 + 40 * 30 + 20 * 15)
    _check(size, ALIGNED_BASE, run)


def test_lpips_distance():
    from test_hip_lpips import _features, _lins
    feats, lins = _features(77, 131, 1, 1e-2, seed=5), _lins()
    size, run = _through_cache(lambda workspaces: list(perceptual.distance(feats, lins, "lpips", workspaces)))
    chw = [v for f in feats for v in f.shape[1:]]
    assert size == _C.load_library().gsr_lpips_workspace_size(1, len(feats), (ctypes.c_int * len(chw))(*chw))
    _check(size, ALIGNED_BASE, run)
