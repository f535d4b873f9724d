"""The host side of the device's PNG route: png.assemble frames a zlib stream as a file PIL reads, the two pure size functions of
include/video_io.h (gsr_png_workspace_size, gsr_png_stream_bound) follow the closed form the header states, and the host restatement of
the token rule and the small inflate of tests/png_reference.py hold against zlib. Needs the built library but no GPU."""
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_reference as ref


def _pictures():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, (7, 11, 3), dtype=np.uint8), rng.integers(0, 65536, (5, 9), dtype=np.uint16),
            np.full((1, 1, 3), 200, np.uint8), np.array([[0x0102]], np.uint16)]


@pytest.mark.parametrize("filter_name", ["none", "up"])
def test_assemble_frames_a_zlib_stream_as_the_file_encode_writes(filter_name):
    from slam import png
    for a in _pictures():
        kind = 0 if a.dtype == np.uint8 else 1
        H, W = a.shape[:2]
        raw = ref.filtered(a, png.FILTERS[filter_name])
        stream = zlib.compress(raw.tobytes(), 1)
        data = png.assemble(W, H, kind, stream)
        assert data == png.encode(a, filter_name, 1)                                    # the same stream gives the same file
        with Image.open(io.BytesIO(data)) as im:
            assert np.array_equal(np.array(im).astype(a.dtype), a)
        # the chunk layout, byte by byte: signature | IHDR | IDAT | IEND, each length + type + data + CRC-32 of type + data
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        at, seen = 8, []
        while at < len(data):
            n, name = struct.unpack(">I4s", data[at:at + 8])
            body = data[at + 8:at + 8 + n]
            assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(name + body) & 0xFFFFFFFF
            seen.append((name, body))
            at += 12 + n
        assert at == len(data) and [s[0] for s in seen] == [b"IHDR", b"IDAT", b"IEND"]
        assert seen[0][1] == struct.pack(">IIBBBBB", W, H, 8 if kind == 0 else 16, 2 if kind == 0 else 0, 0, 0, 0)
        assert seen[1][1] == stream and seen[2][1] == b""
    with pytest.raises(ValueError, match="kind"):
        png.assemble(4, 4, 2, b"")
    with pytest.raises(ValueError, match="empty"):
        png.assemble(0, 4, 0, b"")


def _closed_form(W, H, kind, seg):
    n = H * (W * (3 if kind == 0 else 2) + 1)
    return 2 + n + 10 * -(-n // seg) + 9


def test_size_functions_follow_the_closed_form_and_refuse_what_is_out_of_range():
    from diff_gaussian_rasterization import _abi
    from slam import png_device
    seg = png_device.SEGMENT
    assert seg == _abi.GSR_PNG_SEGMENT and 1024 <= seg <= 65535
    for kind in (0, 1):
        for W, H in [(1, 1), (2, 3), (5, 2), (341, 16), (640, 480), (1920, 1080), (seg, 1), (1, seg + 1)]:
            assert png_device.png_stream_bound(W, H, kind) == _closed_form(W, H, kind, seg), (W, H, kind)
            assert png_device.png_workspace_size(1, W, H, kind) > 0
    # outside the range: 0
    for W, H, kind in [(0, 4, 0), (4, 0, 0), (-1, 4, 1), (4, 4, 2), (4, 4, -1), (2 ** 30, 2 ** 30, 0), (65535, 65535, 0), (2 ** 31 - 1, 1, 0)]:
        assert png_device.png_stream_bound(W, H, kind) == 0, (W, H, kind)
        assert png_device.png_workspace_size(1, W, H, kind) == 0, (W, H, kind)
    assert png_device.png_workspace_size(0, 4, 4, 0) == 0 and png_device.png_workspace_size(65536, 4, 4, 0) == 0
    assert png_device.png_workspace_size(65535, 4, 4, 0) > 0
    # the largest picture whose bound stays below 2^31 is taken, the next is not
    H = (2 ** 31 - 1) // 4
    while _closed_form(1, H, 0, seg) > 2 ** 31 - 1:
        H -= 1
    assert png_device.png_stream_bound(1, H, 0) == _closed_form(1, H, 0, seg) and png_device.png_stream_bound(1, H + 1, 0) == 0


def test_size_functions_are_monotone_in_every_argument():
    from slam import png_device
    sizes = [1, 2, 3, 5, 85, 341, 342, 640, 2340, 5461, 5462]
    for kind in (0, 1):
        for fixed in (1, 7, 480):
            b = [png_device.png_stream_bound(w, fixed, kind) for w in sizes]
            assert b == sorted(b) and len(set(b)) == len(b)
            b = [png_device.png_stream_bound(fixed, h, kind) for h in sizes]
            assert b == sorted(b) and len(set(b)) == len(b)
            w = [png_device.png_workspace_size(3, s, fixed, kind) for s in sizes]
            assert w == sorted(w)
            w = [png_device.png_workspace_size(3, fixed, s, kind) for s in sizes]
            assert w == sorted(w)
        v = [png_device.png_workspace_size(views, 64, 48, kind) for views in (1, 2, 3, 12, 100)]
        assert v == sorted(v) and len(set(v)) == len(v)
    for W, H in [(1, 1), (64, 48), (640, 480)]:                                         # three bytes a pixel take no less than two
        assert png_device.png_stream_bound(W, H, 0) >= png_device.png_stream_bound(W, H, 1)
        assert png_device.png_workspace_size(2, W, H, 0) >= png_device.png_workspace_size(2, W, H, 1)


def test_the_token_rule_and_the_small_inflate_hold_against_zlib():
    """tokens(): runs of 1 and 2 stay literals, 3 .. 258 are one match, longer runs are cut at 258 from their start; parse() reads zlib's
    own streams (dynamic and stored blocks) into tokens whose lengths add up to the input."""
    D = 3
    b = np.arange(40, dtype=np.uint8).repeat(1)
    assert ref.tokens(b, D) == [("lit", int(v)) for v in b]
    zeros = np.zeros(3 + 258 + 2, np.uint8)                                             # three bytes that cannot repeat, then a run of 260
    assert ref.tokens(zeros, D) == [("lit", 0)] * 3 + [("match", 258)] + [("lit", 0)] * 2 and ref.remainders(zeros, D) == [2]
    assert ref.tokens(np.zeros(3 + 261, np.uint8), D)[3:] == [("match", 258), ("match", 3)]
    assert ref.tokens(np.zeros(2 + 2, np.uint8), 2) == [("lit", 0)] * 4
    smooth = (np.arange(30000) // 7 % 251).astype(np.uint8)
    for data, level in ((smooth, 6), (smooth, 0)):
        blocks = ref.parse(zlib.compress(data.tobytes(), level))
        assert sum(bl["bytes"] for bl in blocks) == len(data) and blocks[-1]["final"]
    assert ref.huffman_depth([1, 1, 2, 3, 5, 8]) == 5 and ref.huffman_depth([4, 4, 4, 4]) == 2
