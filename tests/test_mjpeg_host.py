"""The host side of the Motion-JPEG output (slam/mjpeg.py) and the numpy statement of the encoder (tests/jpeg_reference.py), without a GPU:
the tables against the ones PIL's libjpeg writes, the statement's files decoded by PIL and measured against PIL's own encoder, and the AVI
container read back. No video tool is installed here, so the container is checked structurally and frame by frame through PIL."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_reference as ref
from slam import mjpeg

QUALITIES = (50, 90, 100)
PSNR_MARGIN_DB = 0.25          # against PIL at the same quality and subsampling: covers libjpeg's integer DCT and its chroma rounding


def _pil_jpeg(rgb, quality):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
    return b.getvalue()


def _decode(data):
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        assert im.format == "JPEG"
        return np.array(im.convert("RGB"))


def _segments(data):
    """[(marker, payload)] up to and including SOS."""
    out, i = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[i] == 0xFF
        marker, length = data[i + 1], struct.unpack_from(">H", data, i + 2)[0]
        out.append((marker, data[i + 4:i + 2 + length]))
        if marker == 0xDA:
            return out
        i += 2 + length


@pytest.mark.parametrize("quality", [1, 25, 50, 75, 90, 95, 100])
def test_tables_equal_the_ones_pil_writes(quality):
    segs = _segments(_pil_jpeg(ref.smooth_picture(32, 32), quality))
    dqt, dht = {}, {}
    for marker, payload in segs:
        j = 0
        while marker == 0xDB and j < len(payload):
            assert payload[j] >> 4 == 0                                            # 8-bit entries
            dqt[payload[j] & 15] = list(payload[j + 1:j + 65])
            j += 65
        while marker == 0xC4 and j < len(payload):
            counts = list(payload[j + 1:j + 17])
            dht[payload[j]] = (counts, list(payload[j + 17:j + 17 + sum(counts)]))
            j += 17 + sum(counts)
    q = mjpeg.quant_tables(quality)
    assert q.shape == (2, 64) and q.dtype == np.uint16
    assert dqt == {0: q[0].tolist(), 1: q[1].tolist()}
    h = mjpeg.huffman_tables()
    assert dht == {0x00: tuple(h["dc0"]), 0x10: tuple(h["ac0"]), 0x01: tuple(h["dc1"]), 0x11: tuple(h["ac1"])}
    # and the whole header is the one libjpeg writes for this size and quality
    assert mjpeg.jfif_header(32, 32, q) == _pil_jpeg(ref.smooth_picture(32, 32), quality)[:len(mjpeg.jfif_header(32, 32, q))]


@pytest.mark.parametrize("bad", [0, 101, -3, 50.0, None, True])
def test_quality_outside_1_to_100_is_refused(bad):
    with pytest.raises(ValueError, match="quality"):
        mjpeg.quant_tables(bad)


def test_header_layout():
    q = mjpeg.quant_tables(90)
    segs = _segments(mjpeg.jfif_header(131, 77, q))
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert segs[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    assert segs[3][1] == struct.pack(">BHHB", 8, 77, 131, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert [p[0] for m, p in segs if m == 0xC4] == [0x00, 0x10, 0x01, 0x11]
    with pytest.raises(ValueError, match="qtables"):
        mjpeg.jfif_header(16, 16, np.zeros((2, 64), np.uint16))


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 33), (131, 77)])
@pytest.mark.parametrize("quality", QUALITIES)
def test_statement_decodes_and_matches_pils_encoder(size, quality):
    W, H = size
    pic = ref.adversarial_picture(H, W)
    mine = _decode(ref.encode(pic, quality))
    theirs = _decode(_pil_jpeg(pic, quality))
    assert mine.shape == (H, W, 3)
    a, b = ref.psnr(mine, pic), ref.psnr(theirs, pic)
    print(f"{W}x{H} Q{quality}: statement {a:.3f} dB, PIL {b:.3f} dB")
    assert a >= b - PSNR_MARGIN_DB


def test_statement_at_131x77_is_adversarial_and_of_pils_size():
    pic = ref.adversarial_picture(77, 131)
    events = {}
    for quality in QUALITIES:
        e = {}
        data = ref.encode(pic, quality, events=e)
        events[quality] = e
        theirs = len(_pil_jpeg(pic, quality))
        print(f"Q{quality}: {len(data)} bytes, PIL {theirs}, {e}")
        assert abs(len(data) - theirs) <= 0.10 * theirs
    assert events[100]["dc_category_max"] == 11                                    # a DC step of 2040
    assert events[50]["zrl"] + events[90]["zrl"] >= 1
    assert all(e["stuffed"] >= 1 for e in events.values())
    scan = ref.entropy_code(ref.coefficients(pic, mjpeg.quant_tables(100)))
    assert scan.count(b"\xff\x00") >= 1 and b"\xff" not in scan.replace(b"\xff\x00", b"")


def test_entropy_coder_pads_with_ones_and_stuffs_the_padded_byte():
    # one MCU of zeros: six blocks of (DC category 0, EOB): 4 x (2 + 4) + 2 x (2 + 2) = 32 bits, no padding
    zero = np.zeros((1, 1, 6, 64), np.int16)
    assert len(ref.entropy_code(zero)) == 4
    # a DC of -1024 then +1016 steps through category 11; the codes end inside a byte, which is filled with 1-bits
    c = zero.copy()
    c[0, 0, 0, 0], c[0, 0, 1, 0] = -1024, 1016
    e = {}
    out = ref.entropy_code(c, e)
    assert e["dc_category_max"] == 11 and out[-1] & 1 == 1


# ---- container ---------------------------------------------------------------------------------------------------------------------
def _frames():
    pics = [ref.smooth_picture(24, 40, seed=s) for s in range(3)]
    frames = [ref.encode(p, 90) for p in pics]
    if len(frames[1]) % 2 == 0:                                                    # one frame of odd length: a byte behind EOI is legal
        frames[1] += b"\0"
    assert len(frames[1]) % 2 == 1
    return pics, frames


def test_avi_round_trip_and_header_fields(tmp_path):
    pics, frames = _frames()
    path = str(tmp_path / "clip.avi")
    w = mjpeg.AviWriter(path, 40, 24, 29.97)
    for f in frames:
        w.add(f)
    w.close()
    w.close()                                                                      # idempotent
    with pytest.raises(ValueError, match="closed"):
        w.add(frames[0])
    info, back = mjpeg.read_avi(path)
    assert back == frames
    assert info["width"] == 40 and info["height"] == 24 and info["frames"] == 3 and info["length"] == 3 and info["streams"] == 1
    assert info["flags"] == 0x10 and info["type"] == b"vids" and info["handler"] == b"MJPG" and info["compression"] == b"MJPG"
    assert info["scale"] == 1000 and info["rate"] == 29970 and abs(info["fps"] - 29.97) < 1e-9
    assert info["bitmap_size"] == 40 and info["bit_count"] == 24 and info["planes"] == 1
    assert info["bitmap_width"] == 40 and info["bitmap_height"] == 24
    for pic, f in zip(pics, back):
        assert _decode(f).shape == pic.shape and ref.psnr(_decode(f), pic) > 30
    # the structure, byte by byte
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    assert data[12:16] == b"LIST" and data[20:24] == b"hdrl" and data[24:28] == b"avih" and struct.unpack_from("<I", data, 28)[0] == 56
    assert data[88:92] == b"LIST" and data[96:100] == b"strl" and data[100:104] == b"strh" and struct.unpack_from("<I", data, 104)[0] == 56
    assert data[164:168] == b"strf" and struct.unpack_from("<I", data, 168)[0] == 40
    assert data[212:216] == b"LIST" and data[220:224] == b"movi"
    movi = struct.unpack_from("<I", data, 216)[0]
    assert movi == 4 + sum(8 + len(f) + (len(f) & 1) for f in frames)              # odd frames are padded to even length
    at = 224
    for k, f in enumerate(frames):
        assert data[at:at + 4] == b"00dc" and struct.unpack_from("<I", data, at + 4)[0] == len(f) and at % 2 == 0
        at += 8 + len(f) + (len(f) & 1)
    assert data[at:at + 4] == b"idx1" and struct.unpack_from("<I", data, at + 4)[0] == 48 and at + 8 + 48 == len(data)
    entries = [struct.unpack_from("<4sIII", data, at + 8 + 16 * k) for k in range(3)]
    offsets = [4 + sum(8 + len(g) + (len(g) & 1) for g in frames[:k]) for k in range(3)]                  # from the 'movi' fourcc
    assert entries == [(b"00dc", 0x10, o, len(f)) for o, f in zip(offsets, frames)]


def test_read_avi_notices_an_index_that_disagrees_with_movi(tmp_path):
    _, frames = _frames()
    path = str(tmp_path / "clip.avi")
    with mjpeg.AviWriter(path, 40, 24, 30) as w:
        for f in frames:
            w.add(f)
    data = bytearray(open(path, "rb").read())
    at = data.rindex(b"idx1") + 8 + 16 + 8                                         # the second entry's offset
    data[at:at + 4] = struct.pack("<I", struct.unpack_from("<I", data, at)[0] + 2)
    bad = str(tmp_path / "bad.avi")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(ValueError, match="disagree"):
        mjpeg.read_avi(bad)


def test_avi_size_guard_closes_the_file_validly(tmp_path, monkeypatch):
    _, frames = _frames()
    path = str(tmp_path / "full.avi")
    monkeypatch.setattr(mjpeg, "AVI_LIMIT", mjpeg.AviWriter.HEADER + 2 * (8 + len(frames[0]) + (len(frames[0]) & 1) + 16) + 8 + 40)
    w = mjpeg.AviWriter(path, 40, 24, 30)
    w.add(frames[0])
    w.add(frames[0])
    with pytest.raises(ValueError, match="split"):
        w.add(frames[2])
    info, back = mjpeg.read_avi(path)                                              # closed by the refused add, and valid
    assert info["frames"] == 2 and back == [frames[0], frames[0]]
    import os
    assert os.path.getsize(path) <= mjpeg.AVI_LIMIT
