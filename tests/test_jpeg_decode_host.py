"""The JPEG decoder's arithmetic contract (include/video_io.h gsr_jpeg_decode) on the CPU: the integer numpy restatement
(tests/jpeg_decode_reference.py) equals libjpeg, through PIL, in every byte for every sampling the host parser (slam/jpeg_decode.py) accepts;
what the parser does not accept it refuses with its reason; the tables it hands the device decode what the restatement decodes; the AVI
index reads frames back by offset. No GPU."""
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_decode_cases as cases
import jpeg_decode_reference as ref
import jpeg_reference as enc

CASES = [(v, H, W, q) for v in cases.VARIANTS for (H, W) in cases.SIZES for q in cases.QUALITIES]


@pytest.mark.parametrize("variant", list(cases.VARIANTS))
def test_restatement_equals_pil_in_every_byte(variant):
    from slam import jpeg_decode
    for H, W in cases.SIZES:
        for q in cases.QUALITIES:
            data = cases.jpeg_file(variant, H, W, q)
            parsed = jpeg_decode.parse_frame(data, f"{variant} {W}x{H} q{q}", W, H)          # the parser accepts it ...
            rgb, _, status = ref.decode(data)
            want = cases.pil_rgb(data)
            assert status == ref.OK
            assert rgb.shape == want.shape == (parsed.height, parsed.width, 3)
            assert np.array_equal(rgb, want), f"{variant} {W}x{H} q{q}: {int((rgb != want).sum())} bytes differ"     # ... so it must be exact


def test_smooth_pictures_too():
    for variant in cases.VARIANTS:
        data = cases.jpeg_file(variant, 37, 53, 75, "smooth", 3)
        assert np.array_equal(ref.decode(data)[0], cases.pil_rgb(data)), variant


def test_variants_are_what_they_claim():
    """The files exercise what they are meant to: samplings, restart intervals, custom tables."""
    from diff_gaussian_rasterization import _abi
    from slam import jpeg_decode
    want = {"ours": _abi.GSR_JPEG_420, "pil": _abi.GSR_JPEG_420, "422": _abi.GSR_JPEG_422, "444": _abi.GSR_JPEG_444, "grey": _abi.GSR_JPEG_GREY}
    for variant, sampling in want.items():
        assert jpeg_decode.parse_frame(cases.jpeg_file(variant, 37, 53, 75)).sampling == sampling
    blocks = jpeg_decode.parse_frame(cases.jpeg_file("restart_blocks", 37, 53, 75))
    rows = jpeg_decode.parse_frame(cases.jpeg_file("restart_rows", 37, 53, 75))
    assert (blocks.restart_interval, blocks.intervals) == (1, 3 * 4) and (rows.restart_interval, rows.intervals) == (4, 3)
    assert not np.array_equal(jpeg_decode.parse_frame(cases.jpeg_file("optimize", 37, 53, 75)).huffman, jpeg_decode.default_huffman())
    assert np.array_equal(jpeg_decode.parse_frame(cases.jpeg_file("ours", 37, 53, 75)).huffman, jpeg_decode.default_huffman())


@pytest.mark.parametrize("H,W", cases.SIZES)
def test_coefficients_of_our_own_files(H, W):
    from slam import mjpeg
    for q in cases.QUALITIES:
        _, coef, status = ref.decode(cases.jpeg_file("ours", H, W, q))
        assert status == ref.OK
        assert np.array_equal(coef, enc.coefficients(cases.picture(H, W), mjpeg.quant_tables(q)))


def test_missing_dht_means_annex_k():
    from slam import jpeg_decode
    data = cases.jpeg_file("pil", 37, 53, 75)
    bare = cases.strip_dht(data)
    assert len(bare) < len(data) and b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")]
    assert np.array_equal(ref.decode(bare)[0], cases.pil_rgb(data))
    assert np.array_equal(jpeg_decode.parse_frame(bare).huffman, jpeg_decode.parse_frame(data).huffman)


def _device_table_symbol(table, bits):
    """Decodes one symbol from a '0101..' string with the kernel's table form, as the kernel does; (symbol, length)."""
    peek = int((bits + "0" * 16)[:16], 2)
    for length in range(1, 17):
        if peek < table[length - 1]:
            idx = (int(table[16 + length - 1]) + (peek >> (16 - length))) & 255
            return (int(table[32 + idx // 4]) >> (8 * (idx % 4))) & 0xFF, length
    return None, 0


def test_device_huffman_tables_decode_every_code():
    """Every code of the Annex K tables and of PIL's optimised tables decodes to its symbol through limit / offset / symbols."""
    from slam import jpeg_decode, mjpeg
    tables = list(mjpeg.huffman_tables().values()) + list(ref.parse(cases.jpeg_file("optimize", 131, 77, 95))["huffman"].values())
    for table in tables:
        dev = jpeg_decode.device_huffman(table)
        for symbol, (code, length) in mjpeg.huffman_codes(table).items():
            assert _device_table_symbol(dev, format(code, f"0{length}b")) == (symbol, length)
        assert _device_table_symbol(dev, "1" * 16)[0] is None             # the all-ones code is never assigned
    with pytest.raises(ValueError, match="more codes of 1 bits than there are"):
        jpeg_decode.device_huffman(([3] + [0] * 15, [0, 1, 2]))


def test_parser_output_matches_the_restatement():
    from slam import jpeg_decode
    for variant in cases.VARIANTS:
        data = cases.jpeg_file(variant, 37, 53, 30)
        parsed, p = jpeg_decode.parse_frame(data), ref.parse(data)
        assert parsed.scan == p["scan"][:-2] and p["scan"][-2:] == b"\xff\xd9"
        for k, c in enumerate(p["components"]):
            assert np.array_equal(parsed.qtables[k], p["qtables"][c[2]])
            assert (parsed.descriptor[1 + k], parsed.descriptor[4 + k]) == (c[3], c[4])
        assert parsed.descriptor[0] == p["restart_interval"]


REFUSED = [
    ("progressive", lambda: _pil(progressive=True), "progressive file .SOF2.; only baseline"),
    ("size", lambda: cases.jpeg_file("pil", 37, 53, 75), "the picture is 53 x 37, the calibration says 64 x 48"),
    ("truncated header", lambda: cases.jpeg_file("pil", 37, 53, 75)[:100], "the header is truncated"),
    ("4:4:0", lambda: cases.with_luminance_sampling(cases.jpeg_file("422", 37, 53, 75), 1, 2), "luminance sampling 1 x 2: only grey, 4:4:4, 4:2:2"),
    ("4:1:1", lambda: cases.with_luminance_sampling(cases.jpeg_file("422", 37, 53, 75), 4, 1), "luminance sampling 4 x 1: only grey"),
    ("not jpeg", lambda: b"RIFF" + bytes(40), "not a JPEG file"),
    ("cmyk", lambda: _pil(mode="CMYK"), "4 components"),
]


def _pil(mode="RGB", **options):
    out = io.BytesIO()
    Image.fromarray(cases.picture(37, 53)).convert(mode).save(out, "JPEG", **options)
    return out.getvalue()


@pytest.mark.parametrize("name,make,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_parser_refuses_with_the_reason(name, make, text):
    from slam import jpeg_decode
    size = (64, 48) if name == "size" else (None, None)
    with pytest.raises(ValueError, match=f"clip.avi frame 7: .*{text}"):
        jpeg_decode.parse_frame(make(), "clip.avi frame 7", *size)


def test_avi_index_reads_every_frame_by_offset(tmp_path):
    from slam import jpeg_decode, mjpeg
    files = [cases.jpeg_file("ours", 16, 17, q) for q in cases.QUALITIES] + [cases.jpeg_file("pil", 16, 17, 75)]
    path = str(tmp_path / "clip.avi")
    with mjpeg.AviWriter(path, 17, 16, 12.5) as avi:
        for data in files:
            avi.add(data)
    index = jpeg_decode.open_source(path)
    assert isinstance(index, jpeg_decode.AviIndex) and len(index) == len(files)
    assert (index.info["width"], index.info["height"], index.info["fps"]) == (17, 16, 12.5)
    for k in (3, 0, 2, 1):                                               # any order
        assert index.read(k) == files[k]
    assert index.read(1) == mjpeg.read_avi(path)[1][1]
    assert index.time(2) == 2 / 12.5
    with open(path, "r+b") as f:                                          # a file cut inside its last frame
        f.truncate(index.entries[-1][0] + 3)
    with pytest.raises(ValueError, match="runs past its parent"):
        jpeg_decode.AviIndex(path)


def test_folder_source_sorts_by_name(tmp_path):
    from slam import jpeg_decode
    for name, q in (("b.jpeg", 75), ("a.jpg", 30), ("c.JPG", 95), ("notes.txt", 30)):
        (tmp_path / name).write_bytes(cases.jpeg_file("pil", 16, 17, q))
    src = jpeg_decode.open_source(str(tmp_path))
    assert [os.path.basename(src.name(k)) for k in range(len(src))] == ["a.jpg", "b.jpeg", "c.JPG"]
    assert src.read(0) == cases.jpeg_file("pil", 16, 17, 30) and src.time(2) == 2.0
    with pytest.raises(FileNotFoundError):
        jpeg_decode.open_source(str(tmp_path / "missing.avi"))


def test_pack_joins_a_chunk():
    from slam import jpeg_decode
    frames = [jpeg_decode.parse_frame(cases.jpeg_file(v, 37, 53, 75)) for v in ("ours", "optimize", "restart_rows")]
    p = jpeg_decode.pack(frames)
    assert p["offsets"].tolist() == np.cumsum([0] + [len(f.scan) for f in frames]).tolist() and p["max_intervals"] == 3
    assert p["scans"].tobytes() == b"".join(f.scan for f in frames)
    assert p["qtables"].shape == (3, 3, 64) and p["huffman"].shape == (3, 4, 96) and p["descriptors"].shape == (3, 8)
    with pytest.raises(ValueError, match="one call decodes one size and sampling"):
        jpeg_decode.pack(frames + [jpeg_decode.parse_frame(cases.jpeg_file("444", 37, 53, 75))])
