"""The device's deflate encoder (include/video_io.h gsr_png_encode, csrc/gs_png.h) and the lossless playback built on it
(Playback.write(device_png=True), tools/play_map.py --device-png). The decoders are the oracle: zlib's inflate must give back the numpy
filtered bytes exactly and end at the stream's end, PIL must read the assembled file as the input pixels, and no stream may pass
gsr_png_stream_bound. Where the contract fixes the tokens, a small inflate of the test's own (tests/png_reference.py parse) reads them out of
the device's stream and holds them against the numpy statement of the rule.

Compressed size, measured on an MI355X against len(zlib.compress(filtered, 1)) on three seeded 320 x 240 pictures (filter Up): see SIZE_RATIO
below; each is asserted with 10 % on top, since the device's bytes are deterministic but another machine's zlib build may differ."""
import io
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_reference as ref
from util import REPO

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
FILTER = {"none": 0, "up": 2}
# device bytes / zlib level 1 bytes, measured (DESIGN.md section 8 has the table)
SIZE_RATIO = {"clean": 0.9241, "noisy": 0.8157, "depth": 1.0889}


def _seg():
    from slam import png_device
    return png_device.SEGMENT


def _kind(pic):
    return 0 if pic.dtype == np.uint8 else 1


def _encode(pics, filter_name, tail=4096):
    """(streams [bytes per view], bound) from ONE call on the stacked pictures; the bytes behind every stream and behind the buffer stay
    untouched."""
    from slam import png_device
    dev = torch.device("cuda:0")
    a = np.stack(pics)
    kind = _kind(pics[0])
    V, H, W = a.shape[:3]
    pixels = torch.from_numpy(a.view(np.int16) if kind else a).to(dev)
    bound = png_device.png_stream_bound(W, H, kind)
    flat = torch.full((V * bound + tail,), SENTINEL, dtype=torch.uint8, device=dev)
    out = flat[:V * bound].view(V, bound)
    sizes = torch.full((V,), -7, dtype=torch.int32, device=dev)
    assert png_device.png_encode(pixels, out, sizes, filter_name) == kind
    torch.cuda.synchronize()
    sizes, host = sizes.cpu().numpy(), flat.cpu().numpy()
    assert (sizes >= 2 + 5 + 9).all() and (sizes <= bound).all(), (sizes, bound)
    for v in range(V):
        assert (host[v * bound + sizes[v]:(v + 1) * bound] == SENTINEL).all(), v
    assert (host[V * bound:] == SENTINEL).all()
    return [host[v * bound:v * bound + sizes[v]].tobytes() for v in range(V)], bound


def _check(pic, filter_name, stream, bound):
    """The three things every case is held to. Returns the filtered bytes."""
    from slam import png
    raw = ref.filtered(pic, FILTER[filter_name]).tobytes()
    d = zlib.decompressobj()
    got = d.decompress(stream)
    assert got == raw, next((i for i in range(min(len(got), len(raw))) if got[i] != raw[i]), (len(got), len(raw)))
    assert d.eof and d.unused_data == b""
    H, W = pic.shape[:2]
    with Image.open(io.BytesIO(png.assemble(W, H, _kind(pic), stream))) as im:
        assert np.array_equal(np.array(im).astype(pic.dtype), pic)
    assert len(stream) <= bound
    return raw


def _segments(raw):
    seg = _seg()
    return [np.frombuffer(raw[g:g + seg], np.uint8) for g in range(0, len(raw), seg)]


def _check_tokens(raw, stream, D):
    """Every dynamic block's tokens are the rule's tokens of its own segment; the blocks alternate with empty stored blocks; returns them."""
    blocks = ref.parse(stream)
    segs = _segments(raw)
    assert len(blocks) == 2 * len(segs) + 1
    assert blocks[-1] == {"type": "stored", "final": True, "tokens": [("stored", 0)], "bytes": 0}
    for k, s in enumerate(segs):
        b, sync = blocks[2 * k], blocks[2 * k + 1]
        assert sync["type"] == "stored" and sync["bytes"] == 0 and not sync["final"] and not b["final"] and b["bytes"] == len(s)
        if b["type"] == "dynamic":
            want = [t if t[0] == "lit" else t + (D,) for t in ref.tokens(s, D)]
            assert b["tokens"] == want, (k, next(i for i in range(len(want)) if b["tokens"][i] != want[i]))
            assert b["max_length"] <= 15 and b["max_cl_length"] <= 7
            matches = any(t[0] == "match" for t in want)
            assert b["distance_lengths"] == ([0] * (D - 1) + [1] if matches else [0])
    return blocks


def _random_picture(rng, W, H, kind):
    """Flat stretches, smooth stretches and noise in one picture."""
    if kind == 0:
        a = np.full((H, W, 3), (10, 200, 90), np.uint8)
        noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        a = np.full((H, W), 0x1234, np.uint16)
        noise = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    pick = rng.random((H, W)) < 0.15
    a[pick] = noise[pick]
    return a


def _shape_for(n, D):
    """(W, H) with H * (W * D + 1) == n, of the factorisations the one with H nearest 64; None when there is none."""
    fits = [H for H in range(1, n + 1) if n % H == 0 and (n // H - 1) % D == 0 and n // H > 1]
    if not fits:
        return None
    H = min(fits, key=lambda h: abs(h - 64))
    return (n // H - 1) // D, H


def _from_filtered_row(f, kind):
    """The one-row picture whose filtered bytes (filter None) are f: f[0] == 0, then W * D bytes."""
    body = np.asarray(f[1:], np.uint8)
    if kind == 0:
        return body.reshape(1, -1, 3)
    return body.reshape(1, -1, 2).astype(np.uint16) @ np.array([256, 1], np.uint16)


def _fresh(f, D, k=1):
    """A byte that does not repeat at distance D when appended to f."""
    return (f[-D] + k) % 256 if len(f) >= D else (17 * len(f) + 1) % 256


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("filter_name", ["none", "up"])
def test_smallest_pictures(kind, filter_name):
    rng = np.random.default_rng(1)
    for W, H in [(1, 1), (2, 3), (5, 2), (7, 3)]:                       # 7: rows of 22 and 15 bytes, no multiple of 4
        pic = _random_picture(rng, W, H, kind)
        streams, bound = _encode([pic], filter_name)
        _check(pic, filter_name, streams[0], bound)


@pytest.mark.parametrize("filter_name", ["none", "up"])
@pytest.mark.parametrize("extra", [-1, 0, 1, "two"])
def test_segment_edges(extra, filter_name):
    seg = _seg()
    n = 2 * seg + 1 if extra == "two" else seg + extra
    done = 0
    for kind, D in ((0, 3), (1, 2)):
        shape = _shape_for(n, D)
        if shape is None:                                               # (a power of two has no odd row: 16-bit grey cannot be n = SEG)
            continue
        W, H = shape
        assert H * (W * D + 1) == n
        rng = np.random.default_rng(n + kind)
        flat = np.full((H, W, 3), 77, np.uint8) if kind == 0 else np.full((H, W), 0x4D4D, np.uint16)
        for pic in (flat, _random_picture(rng, W, H, kind)):
            streams, bound = _encode([pic], filter_name)
            raw = _check(pic, filter_name, streams[0], bound)
            blocks = _check_tokens(raw, streams[0], D)
            assert len(blocks) == 2 * -(-n // seg) + 1
        # the flat picture repeats across every segment edge: the run restarts there, with D literals
        if filter_name == "none" and extra == "two":
            second = ref.parse(_encode([flat], filter_name)[0][0])[2]["tokens"]
            assert all(t[0] == "lit" for t in second[:D]) and second[D][0] == "match"
        done += 1
    assert done >= 1


@pytest.mark.parametrize("kind", [0, 1])
def test_match_lengths(kind):
    D = 3 if kind == 0 else 2
    runs = [2, 3, 257, 258, 259, 260, 261, 516, 517]
    f = [0]
    for L in runs:
        for k in range(D):
            f.append(_fresh(f, D, 1 + k))
        for _ in range(L):
            f.append(f[-D])
    f.append(_fresh(f, D))
    while (len(f) - 1) % D:
        f.append(_fresh(f, D))
    pic = _from_filtered_row(f, kind)
    raw = ref.filtered(pic, 0).tobytes()
    assert list(raw) == f
    assert ref.remainders(f, D) == [2, 3, 257, 258, 1, 2, 3, 258, 1]                    # remainders of 1 and 2 occur
    want = ref.tokens(f, D)
    assert [t[1] for t in want if t[0] == "match"] == [3, 257, 258, 258, 258, 258, 3, 258, 258, 258, 258]
    streams, bound = _encode([pic], "none")
    assert _check(pic, "none", streams[0], bound) == raw
    blocks = _check_tokens(raw, streams[0], D)
    assert blocks[0]["type"] == "dynamic"


def test_length_limiting():
    """Literals that never repeat, with Fibonacci frequencies over 17 values: the unconstrained Huffman tree is deeper than 15."""
    fib = [1, 1]                                                        # the two ones are the row's filter byte and the end-of-block symbol
    while len(fib) < 19:
        fib.append(fib[-1] + fib[-2])
    left = {10 + 3 * i: c for i, c in enumerate(fib[2:])}               # 17 values, 2 .. 4181 times
    left[max(left)] += 1                                                # 10943 + 1 bytes: a whole number of pixels
    f = [0]
    while any(left.values()):
        v = max((c, s) for s, c in left.items() if c and (len(f) < 3 or s != f[-3]))[1]
        f.append(v)
        left[v] -= 1
    assert len(f) == 10945 and len(f) < _seg()
    pic = _from_filtered_row(f, 0)
    raw = ref.filtered(pic, 0).tobytes()
    want = ref.tokens(f, 3)
    assert all(t[0] == "lit" for t in want)
    histogram = np.bincount(np.frombuffer(raw, np.uint8), minlength=257)
    histogram[256] = 1                                                  # end of block
    assert ref.huffman_depth(histogram) > 15
    streams, bound = _encode([pic], "none")
    _check(pic, "none", streams[0], bound)
    blocks = _check_tokens(raw, streams[0], 3)
    assert blocks[0]["type"] == "dynamic" and blocks[0]["max_length"] == 15


@pytest.mark.parametrize("filter_name", ["none", "up"])
def test_degenerate_alphabets(filter_name):
    zero = np.zeros((9, 40, 3), np.uint8)
    zero16 = np.zeros((9, 40), np.uint16)
    constant = np.full((9, 40, 3), (3, 141, 59), np.uint8)
    f = [0] + [(5, 9, 14)[(i // 3) % 3] for i in range(3 * 200)]        # three values in threes: no byte equals the one three back
    never = _from_filtered_row(f, 0)                                    # no byte repeats: no match, one distance code of zero bits
    assert all(t[0] == "lit" for t in ref.tokens(f, 3))
    for pic in (zero, zero16, constant, never):
        D = 2 if pic.dtype == np.uint16 else 3
        streams, bound = _encode([pic], filter_name)
        raw = _check(pic, filter_name, streams[0], bound)
        blocks = _check_tokens(raw, streams[0], D)
        assert blocks[0]["type"] == "dynamic"
        if pic is never and filter_name == "none":
            assert blocks[0]["distance_lengths"] == [0] and all(t[0] == "lit" for t in blocks[0]["tokens"])


@pytest.mark.parametrize("kind", [0, 1])
def test_stored_fallback(kind):
    rng = np.random.default_rng(7)
    W, H = 120, 100                                                     # three segments
    pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if kind == 0 else rng.integers(0, 65536, (H, W), dtype=np.uint16)
    streams, bound = _encode([pic], "none")
    raw = _check(pic, "none", streams[0], bound)
    assert len(raw) <= len(streams[0]) <= bound
    blocks = ref.parse(streams[0])
    assert [b["type"] for b in blocks[0:-1:2]] == ["stored"] * -(-len(raw) // _seg())


def test_run_coding_is_alive():
    pic = np.zeros((64, 64, 3), np.uint8)
    streams, bound = _encode([pic], "up")
    raw = _check(pic, "up", streams[0], bound)
    print(f"64 x 64 zeros: {len(streams[0])} bytes of {len(raw)}")
    assert len(streams[0]) <= len(raw) // 20                            # codes alone cannot go below n / 8


def test_adler32_over_many_segments():
    pic = np.full((480, 640, 3), 255, np.uint8)
    streams, bound = _encode([pic], "none")
    raw = _check(pic, "none", streams[0], bound)
    assert streams[0][-4:] == zlib.adler32(raw).to_bytes(4, "big") and len(raw) > 50 * _seg()


def _scene(seed, W=640, H=480):
    """A procedural picture that is different for every seed: shading, a flat background, an edge."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.stack([128 + 100 * np.sin(xx / (40 + seed) + yy / 90), 128 + 100 * np.cos(xx / 55 - yy / (35 + seed)), (xx + 2 * yy + 30 * seed) / 8 % 256], -1)
    a[yy > H * 0.7 + 20 * np.sin(xx / 50)] = (30 + seed, 60, 90)
    return a.astype(np.uint8)


def test_batches_equal_single_calls_and_calls_repeat():
    for kind in (0, 1):
        rng = np.random.default_rng(kind)
        pics = [_random_picture(rng, 150, 131, kind), _scene(2, 150, 131) if kind == 0 else (_scene(2, 150, 131)[..., 0].astype(np.uint16) * 200),
                _random_picture(rng, 150, 131, kind)]
        batch, bound = _encode(pics, "up")
        again, _ = _encode(pics, "up")
        assert again == batch
        assert len(set(batch)) == 3
        for v, pic in enumerate(pics):
            _check(pic, "up", batch[v], bound)
            assert _encode([pic], "up")[0][0] == batch[v], v


def test_twelve_views_at_640x480():
    pics = [_scene(v) for v in range(12)]
    streams, bound = _encode(pics, "up")
    for v in (0, 5, 11):
        _check(pics[v], "up", streams[v], bound)
    for v in range(12):
        assert zlib.decompress(streams[v]) == ref.filtered(pics[v], 2).tobytes(), v


def test_sixteen_bit_byte_order():
    from slam import png
    pic = np.array([[0x0102, 0xFF00], [0x0001, 0x8000]], np.uint16)
    streams, bound = _encode([pic], "none")
    assert zlib.decompress(streams[0]) == bytes([0, 1, 2, 0xFF, 0, 0, 0, 1, 0x80, 0])
    with Image.open(io.BytesIO(png.assemble(2, 2, 1, streams[0]))) as im:
        assert int(np.array(im)[0, 0]) == 258 and np.array_equal(np.array(im).astype(np.uint16), pic)


def test_bad_arguments_name_the_argument_and_enqueue_nothing():
    from diff_gaussian_rasterization import _C
    from slam import png_device
    dev = "cuda:0"
    lib = _C.load_library()
    V, H, W = 2, 20, 24
    rgb = torch.zeros((V, H, W, 3), dtype=torch.uint8, device=dev)
    grey = torch.zeros((V, H, W), dtype=torch.int16, device=dev)
    bound = png_device.png_stream_bound(W, H, 0)
    need = png_device.png_workspace_size(V, W, H, 0)
    assert bound == 2 + H * (W * 3 + 1) + 10 + 9 and need > 0
    out = torch.full((V, bound), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((V,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match="pixels must be"):
        png_device.png_encode(rgb.float(), out, sizes)
    with pytest.raises(RuntimeError, match="pixels must be"):
        png_device.png_encode(rgb[..., :2], out, sizes)
    with pytest.raises(RuntimeError, match="pixels must be"):
        png_device.png_encode(rgb[:, :, ::2], out, sizes)
    with pytest.raises(RuntimeError, match="filter must be"):
        png_device.png_encode(rgb, out, sizes, "paeth")
    with pytest.raises(RuntimeError, match="out is on 'cpu'"):
        png_device.png_encode(rgb, out.cpu(), sizes)
    with pytest.raises(RuntimeError, match="out must hold"):
        png_device.png_encode(rgb, out[:, :bound - 1].contiguous(), sizes)
    with pytest.raises(RuntimeError, match="out must be"):
        png_device.png_encode(rgb, torch.cat([out, out], 1)[:, ::2], sizes)
    with pytest.raises(RuntimeError, match="sizes must be"):
        png_device.png_encode(rgb, out, sizes[:1])
    with pytest.raises(RuntimeError, match="sizes must be"):
        png_device.png_encode(rgb, out, sizes.long())
    with pytest.raises(RuntimeError, match="workspace must be"):
        png_device.png_encode(rgb, out, sizes, workspace=ws[:need - 1])
    # the C entry point: the error code, the argument's name in the text
    code = r"gsr_png_encode failed \(code -\d+\): gsr_png_encode: "
    good = dict(views=V, width=W, height=H, kind=0, filter=2, pixels=rgb.data_ptr(), out=out.data_ptr(), out_stride=bound, sizes=sizes.data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=need, stream=None)

    def call(**change):
        a = {**good, **change}
        return lib.gsr_png_encode(*[a[k] for k in good])

    for change, text in [({"kind": 2}, "kind"), ({"kind": -1}, "kind"), ({"filter": 1}, "filter"), ({"filter": 3}, "filter"), ({"filter": -2}, "filter"),
                         ({"views": 0}, "views"), ({"width": 0}, "width"), ({"height": -4}, "height"),
                         ({"pixels": None}, "pixels must not be NULL"), ({"out": None}, "out must not be NULL"),
                         ({"sizes": None}, "sizes must not be NULL"), ({"workspace": None}, "workspace must not be NULL"),
                         ({"out_stride": bound - 1}, "out_stride"), ({"out_stride": 0}, "out_stride"),
                         ({"workspace_bytes": need - 1}, "workspace must be 16-byte aligned and hold"),
                         ({"workspace": ws.data_ptr() + 1}, "workspace must be 16-byte aligned")]:
        with pytest.raises(RuntimeError, match=code + ".*" + text):
            call(**change)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (sizes == -7).all()
    assert call() == 0
    png_device.png_encode(grey, out, sizes, "none", ws[:need])          # (the 16-bit kind needs no more than the RGB one)
    torch.cuda.synchronize()
    assert (sizes > 0).all()


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------
def _size_inputs():
    rng = np.random.default_rng(11)
    clean = _scene(1, 320, 240)
    noisy = np.clip(clean.astype(np.float64) + rng.normal(0.0, 1.0, clean.shape), 0, 255).round().astype(np.uint8)
    yy, xx = np.mgrid[0:240, 0:320].astype(np.float64)
    depth = 5000.0 * (1.5 + 0.004 * xx + 0.002 * yy + 0.3 * np.sin(xx / 45) * np.cos(yy / 60))
    depth[(xx - 200) ** 2 + (yy - 90) ** 2 < 50 ** 2] = 5000.0 * 0.9                    # an object in front, flat to the camera
    return {"clean": clean, "noisy": noisy, "depth": depth.astype(np.uint16)}


@pytest.mark.parametrize("name", ["clean", "noisy", "depth"])
def test_compressed_size_against_zlib_level_1(name):
    pic = _size_inputs()[name]
    streams, bound = _encode([pic], "up")
    raw = _check(pic, "up", streams[0], bound)
    theirs = len(zlib.compress(raw, 1))
    ratio = len(streams[0]) / theirs
    print(f"{name}: device {len(streams[0])} bytes, zlib level 1 {theirs} bytes, ratio {ratio:.4f} (of {len(raw)} filtered bytes)")
    assert ratio <= SIZE_RATIO[name] * 1.10


# ---- playback ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static_map(tmp_path_factory):
    """A static 14-frame synthetic SLAM run at the sizes and schedule of tests/test_hip_mjpeg.py, saved."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "dynamic_map_iters": 60, "network_init_iters": 40, "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 4}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 100}, "model_params": {"dynamic_model": False}})
    torch.manual_seed(0)
    slam = SLAM(cfg, SyntheticRGBDDataset(num_frames=14, width=320, height=240, seed=0, dynamic=False, dystart=None))
    slam.run()
    return slam.save_map(str(tmp_path_factory.mktemp("static") / "map"))


def _read(path):
    with Image.open(path) as im:
        return np.array(im)


def test_write_with_device_png_leaves_the_files_of_the_host_route(static_map, tmp_path):
    """14 tracked poses: a full chunk of 12 and a partial one of 2, through the ring of slots."""
    from slam.map_io import load_map
    from slam.playback import Playback, tracked
    loaded = load_map(static_map, "cuda:0")
    poses, times = tracked(loaded)
    assert len(times) == 14
    pb = Playback(loaded)
    host, device = str(tmp_path / "host"), str(tmp_path / "device")
    a = pb.write(poses, times, host, depth16=True)
    b = pb.write(poses, times, device, depth16=True, device_png=True)
    assert "encode_ms" not in a and b["encode_ms"] > 0 and b["frames"] == 14 and b["fps"] > 0 and b["writer_wait_s"] >= 0
    assert {k: v for k, v in b.items() if k in ("frames", "calibration")} == {k: v for k, v in a.items() if k in ("frames", "calibration")}
    assert sorted(os.listdir(device)) == sorted(os.listdir(host)) == ["depth", "depth.txt", "depth_vis", "groundtruth.txt", "rgb", "rgb.txt"]
    total = 0
    for kind, dtype, mode in (("rgb", np.uint8, "RGB"), ("depth_vis", np.uint8, "RGB"), ("depth", np.uint16, None)):
        names = sorted(os.listdir(os.path.join(host, kind)))
        assert sorted(os.listdir(os.path.join(device, kind))) == names and len(names) == 14
        for n in names:
            mine, theirs = _read(os.path.join(device, kind, n)), _read(os.path.join(host, kind, n))
            assert mine.shape == theirs.shape and np.array_equal(mine, theirs), (kind, n)
            assert mine.shape == ((240, 320, 3) if mode else (240, 320))
            total += os.path.getsize(os.path.join(device, kind, n))
    assert b["bytes"] == total
    assert float(_read(os.path.join(device, "rgb", names[3])).std()) > 10 and int(_read(os.path.join(device, "depth", names[3])).max()) > 1000
    for name in ("rgb.txt", "depth.txt", "groundtruth.txt"):
        assert open(os.path.join(device, name)).read() == open(os.path.join(host, name)).read(), name
    # files=False writes nothing and still encodes; without the optional outputs nothing else is written; png_level has no meaning here
    none = str(tmp_path / "none")
    c = pb.write(poses[:3], times[:3], none, files=False, device_png=True)
    assert not os.path.exists(none) and c["bytes"] > 0 and c["encode_ms"] > 0
    plain = str(tmp_path / "plain")
    pb.write(poses[:3], times[:3], plain, depth_colour=False, png_filter="none", device_png=True)
    assert sorted(os.listdir(plain)) == ["rgb"] and len(os.listdir(os.path.join(plain, "rgb"))) == 3
    for n in os.listdir(os.path.join(plain, "rgb")):
        assert np.array_equal(_read(os.path.join(plain, "rgb", n)), _read(os.path.join(host, "rgb", n)))
    with pytest.raises(ValueError, match="png_level"):
        pb.write(poses[:3], times[:3], plain, png_level=6, device_png=True)
    with pytest.raises(ValueError, match="png_filter"):
        pb.write(poses[:3], times[:3], plain, png_filter="paeth", device_png=True)


def test_play_map_tool_writes_device_png_from_a_fresh_process(static_map, tmp_path):
    out = str(tmp_path / "played")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "play_map.py"), "--map", static_map, "--path", "resample:5", "--out", out,
                        "--device-png", "--depth16"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["device_png"] is True and line["frames"] == 5 and line["bytes"] > 0 and line["encode_ms"] > 0 and line["fps"] > 0
    assert sorted(os.listdir(out)) == ["depth", "depth.txt", "depth_vis", "groundtruth.txt", "rgb", "rgb.txt"]
    for kind, shape in (("rgb", (240, 320, 3)), ("depth_vis", (240, 320, 3)), ("depth", (240, 320))):
        names = os.listdir(os.path.join(out, kind))
        assert len(names) == 5 and all(_read(os.path.join(out, kind, n)).shape == shape for n in names)
