"""The device's JPEG decoder (include/video_io.h gsr_jpeg_decode, csrc/gs_jpeg_decode.h) against the integer numpy statement of its
arithmetic (tests/jpeg_decode_reference.py) and against libjpeg through PIL. Everything is integer work, so every comparison is equality:
pictures, coefficients and status codes, on whole files and on damaged ones. Every output and the workspace sit between guard bytes."""
import functools

import numpy as np
import pytest
import torch

import jpeg_decode_cases as cases
import jpeg_decode_reference as ref

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0xA5
SIZES = cases.SIZES + [(48, 64)]
FOUR_TWO_ZERO = ["ours", "pil", "optimize", "restart_blocks", "restart_rows"]


def _guarded(nbytes, dev):
    """(flat uint8 buffer of sentinels, the view of its middle `nbytes`)."""
    flat = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    return flat, flat[GUARD:GUARD + nbytes]


def _guards_intact(flat):
    f = flat.cpu().numpy()
    return bool((f[:GUARD] == SENTINEL).all() and (f[-GUARD:] == SENTINEL).all())


def _decode(frames, want_coefficients=True, stream=None):
    """(rgb [F, H, W, 3], status [F], coefficients or None, all guards intact) of one call on a list of ParsedFrame."""
    from slam import jpeg_decode, mjpeg
    dev = torch.device("cuda:0")
    p = jpeg_decode.pack(frames)
    F, W, H, sampling = len(frames), p["width"], p["height"], p["sampling"]
    rows, cols = jpeg_decode.mcu_grid(W, H, sampling)
    bpm = jpeg_decode.BLOCKS_PER_MCU[sampling]
    inputs = {k: torch.from_numpy(p[k].view(np.int16) if k == "qtables" else p[k].copy()).to(dev) for k in ("scans", "offsets", "qtables", "huffman", "descriptors")}
    rgb_flat, rgb = _guarded(F * H * W * 3, dev)
    st_flat, st = _guarded(F * 4, dev)
    need = mjpeg.jpeg_decode_workspace_size(F, W, H, sampling, p["max_intervals"])
    ws_flat, ws = _guarded(need, dev)
    flats = [rgb_flat, st_flat, ws_flat]
    coef = None
    if want_coefficients:
        co_flat, co = _guarded(F * rows * cols * bpm * 64 * 2, dev)
        flats.append(co_flat)
        coef = co.view(torch.int16).view(F, rows, cols, bpm, 64)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
    mjpeg.jpeg_decode(inputs["scans"], inputs["offsets"], inputs["qtables"], inputs["huffman"], inputs["descriptors"], rgb.view(F, H, W, 3),
                      st.view(torch.int32), sampling, p["max_intervals"], coef, ws, stream)
    torch.cuda.synchronize()
    return (rgb.view(F, H, W, 3).cpu().numpy(), st.view(torch.int32).cpu().numpy(), None if coef is None else coef.cpu().numpy(),
            all(_guards_intact(f) for f in flats))


@functools.lru_cache(maxsize=None)
def _statement(variant, H, W, quality):
    """(file bytes, the statement's rgb, coefficients, status, PIL's rgb), computed once."""
    data = cases.jpeg_file(variant, H, W, quality)
    rgb, coef, status = ref.decode(data)
    return data, rgb, coef, status, cases.pil_rgb(data)


def _statement_of_scan(data, scan):
    """The statement's (rgb, coefficients, status) of a file whose entropy-coded segment is replaced by `scan`."""
    p = ref.parse(data)
    p["scan"] = scan
    coef, status = ref.decode_coefficients(p)
    return ref.to_rgb(p, ref.component_planes(p, coef)), coef, status


def _parsed(data):
    from slam import jpeg_decode
    return jpeg_decode.parse_frame(data)


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("variant", list(cases.VARIANTS))
def test_equals_the_statement_and_pil(variant, H, W):
    """Three qualities (three sets of quantisation tables and, for "optimize", of Huffman tables) in one call."""
    want = [_statement(variant, H, W, q) for q in cases.QUALITIES]
    rgb, status, coef, intact = _decode([_parsed(w[0]) for w in want])
    assert intact
    assert status.tolist() == [0, 0, 0]
    for k, (_, want_rgb, want_coef, want_status, pil) in enumerate(want):
        assert want_status == 0
        assert np.array_equal(coef[k], want_coef), f"frame {k}: {int((coef[k] != want_coef).sum())} coefficients differ"
        assert np.array_equal(rgb[k], want_rgb), f"frame {k}: {int((rgb[k] != want_rgb).sum())} bytes differ from the statement"
        assert np.array_equal(rgb[k], pil), f"frame {k}: {int((rgb[k] != pil).sum())} bytes differ from PIL"


@pytest.mark.parametrize("count", [1, 2, 65])
def test_frame_counts_with_mixed_tables_and_restart_intervals(count):
    """16 x 16 pictures; 65 is more frames than a wave has lanes. Variants and qualities cycle, so one call mixes Annex K and custom Huffman
    tables, three quantisation tables and frames with and without restart markers."""
    want = [_statement(FOUR_TWO_ZERO[k % 5], 16, 16, cases.QUALITIES[k % 3]) for k in range(count)]
    rgb, status, coef, intact = _decode([_parsed(w[0]) for w in want])
    assert intact and not status.any()
    for k, (_, want_rgb, want_coef, _, pil) in enumerate(want):
        assert np.array_equal(coef[k], want_coef) and np.array_equal(rgb[k], want_rgb) and np.array_equal(rgb[k], pil), k


def test_mixed_restart_intervals_at_a_size_with_several_mcu_rows():
    want = [_statement(v, 37, 53, 75) for v in FOUR_TWO_ZERO]
    rgb, status, coef, intact = _decode([_parsed(w[0]) for w in want])
    assert intact and not status.any()
    for k, (_, want_rgb, want_coef, _, pil) in enumerate(want):
        assert np.array_equal(coef[k], want_coef) and np.array_equal(rgb[k], want_rgb) and np.array_equal(rgb[k], pil), k


def test_without_coefficients_twice_and_on_a_side_stream():
    want = [_statement(v, 131, 77, 95) for v in ("pil", "restart_rows")]
    frames = [_parsed(w[0]) for w in want]
    first = _decode(frames)
    plain = _decode(frames, want_coefficients=False)
    again = _decode(frames)
    side = _decode(frames, stream=torch.cuda.Stream(torch.device("cuda:0")))
    for rgb, status, coef, intact in (first, plain, again, side):
        assert intact and not status.any()
        assert all(np.array_equal(rgb[k], w[4]) for k, w in enumerate(want))
    assert plain[2] is None
    assert np.array_equal(first[2], again[2]) and np.array_equal(first[2], side[2]) and np.array_equal(first[2][0], want[0][2])


def test_round_trip_with_the_device_encoder():
    """A file of the device encoder decodes to the coefficients the encoder reported."""
    from slam import mjpeg
    dev = torch.device("cuda:0")
    H, W, quality = 37, 53, 90
    pics = [cases.picture(H, W, "adversarial", 1), cases.picture(H, W, "smooth", 2)]
    q = mjpeg.quant_tables(quality)
    rows, cols = mjpeg.mcu_grid(W, H)
    scan = torch.zeros((2, 65536), dtype=torch.uint8, device=dev)
    sizes = torch.zeros(2, dtype=torch.int32, device=dev)
    coef = torch.zeros((2, rows, cols, 6, 64), dtype=torch.int16, device=dev)
    mjpeg.jpeg_encode(torch.from_numpy(np.stack(pics)).to(dev), torch.from_numpy(q.astype(np.int16)).to(dev), scan, sizes, coef)
    files = [mjpeg.jfif_header(W, H, q) + scan[k, :int(sizes[k])].cpu().numpy().tobytes() + mjpeg.EOI for k in range(2)]
    rgb, status, back, intact = _decode([_parsed(f) for f in files])
    assert intact and not status.any()
    assert np.array_equal(back, coef.cpu().numpy())
    assert all(np.array_equal(rgb[k], cases.pil_rgb(files[k])) for k in range(2))


def _damaged(variant, change):
    """One call of three frames whose middle one has its scan changed; checks the neighbours and the guards, and the damaged frame against
    the statement. Returns the damaged frame's status."""
    data, _, _, _, pil = _statement(variant, 37, 53, 75)
    frames = [_parsed(data) for _ in range(3)]
    frames[1].scan = change(frames[1].scan)
    want_rgb, want_coef, want_status = _statement_of_scan(data, frames[1].scan)
    rgb, status, coef, intact = _decode(frames)
    assert intact
    assert status[0] == 0 and status[2] == 0 and np.array_equal(rgb[0], pil) and np.array_equal(rgb[2], pil)
    assert status[1] == want_status
    assert np.array_equal(coef[1], want_coef) and np.array_equal(rgb[1], want_rgb)
    return int(status[1])


@pytest.mark.parametrize("variant", ["pil", "optimize", "restart_rows", "422", "grey"])
def test_a_cut_scan_is_refused_cleanly(variant):
    n = len(_parsed(cases.jpeg_file(variant, 37, 53, 75)).scan)
    for cut in (0, 1, n // 3, n // 2, n - 1):
        assert _damaged(variant, lambda s, cut=cut: s[:cut]) != 0, cut
    if variant == "restart_rows":                                      # cut inside a restart marker, and right behind one
        at = _parsed(cases.jpeg_file(variant, 37, 53, 75)).scan.index(b"\xff\xd0")
        assert _damaged(variant, lambda s: s[:at + 1]) != 0
        assert _damaged(variant, lambda s: s[:at + 2]) != 0


def _flip(scan, bit):
    out = bytearray(scan)
    out[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(out)


@pytest.mark.parametrize("variant", ["pil", "restart_rows"])
def test_a_flipped_bit_is_refused_cleanly(variant):
    """The first few bit positions (of a fixed pseudo-random order) whose flip the statement cannot decode either."""
    data = cases.jpeg_file(variant, 37, 53, 75)
    scan = _parsed(data).scan
    order = np.random.default_rng(5).permutation(len(scan) * 8)
    bad = [int(b) for b in order[:60] if _statement_of_scan(data, _flip(scan, int(b)))[2] != 0][:4]
    assert len(bad) == 4
    codes = {_damaged(variant, lambda s, b=b: _flip(s, b)) for b in bad}
    assert 0 not in codes


def test_restart_markers_out_of_sequence():
    def swap(scan):                                                    # RST0 <-> RST1
        a, b = scan.index(b"\xff\xd0"), scan.index(b"\xff\xd1")
        out = bytearray(scan)
        out[a + 1], out[b + 1] = 0xD1, 0xD0
        return bytes(out)

    from diff_gaussian_rasterization import _abi
    assert _damaged("restart_rows", swap) == _abi.GSR_JPEG_BAD_RESTART
    assert _damaged("restart_rows", lambda s: s.replace(b"\xff\xd1", b"", 1)) == _abi.GSR_JPEG_BAD_RESTART      # a marker is missing
    assert _damaged("pil", lambda s: s[:40] + b"\xff\xd0" + s[40:]) == _abi.GSR_JPEG_BAD_RESTART                  # a marker too many


def test_refused_arguments_write_nothing():
    from slam import jpeg_decode, mjpeg
    dev = torch.device("cuda:0")
    data = cases.jpeg_file("pil", 16, 17, 75)
    frames = [_parsed(data), _parsed(data)]
    p = jpeg_decode.pack(frames)
    t = {k: torch.from_numpy(p[k].view(np.int16) if k == "qtables" else p[k].copy()).to(dev) for k in ("scans", "offsets", "qtables", "huffman", "descriptors")}
    rgb = torch.full((2, 16, 17, 3), SENTINEL, dtype=torch.uint8, device=dev)
    status = torch.full((2,), -7, dtype=torch.int32, device=dev)
    coef = torch.full((2, 1, 2, 6, 64), 12345, dtype=torch.int16, device=dev)

    def call(sampling=p["sampling"], max_intervals=1, workspace=None, **over):
        a = {**t, "rgb8": rgb, "status": status, "coefficients": coef, **over}
        mjpeg.jpeg_decode(a["scans"], a["offsets"], a["qtables"], a["huffman"], a["descriptors"], a["rgb8"], a["status"], sampling, max_intervals,
                          a["coefficients"], workspace)

    refused = [
        (dict(rgb8=rgb.cpu()), "rgb8 is on 'cpu'"),
        (dict(rgb8=rgb[..., :2]), r"rgb8 must be \[F, H, W, 3\]"),
        (dict(scans=t["scans"].view(1, -1)), r"scans must be \[bytes\]"),
        (dict(scans=t["scans"].cpu()), "scans is on 'cpu'"),
        (dict(offsets=t["offsets"][:2]), r"offsets must be a contiguous torch.int64 device tensor of shape \(3,\)"),
        (dict(offsets=t["offsets"].to(torch.int32)), "offsets must be a contiguous torch.int64"),
        (dict(qtables=t["qtables"][:, :2]), r"qtables must be .* of shape \(2, 3, 64\)"),
        (dict(huffman=t["huffman"][:, :, :95]), r"huffman must be .* of shape \(2, 4, 96\)"),
        (dict(descriptors=t["descriptors"].to(torch.int64)), "descriptors must be a contiguous torch.int32"),
        (dict(status=status[:1]), r"status must be .* of shape \(2,\)"),
        (dict(coefficients=coef[:, :, :, :4]), r"coefficients must be .* of shape \(2, 1, 2, 6, 64\)"),
        (dict(sampling=4), "sampling must be GSR_JPEG_GREY"),
        (dict(sampling=None), "sampling must be GSR_JPEG_GREY"),
        (dict(max_intervals=0), "max_intervals 0 are outside what gsr_jpeg_decode takes"),
        (dict(max_intervals=3), "max_intervals 3 are outside what gsr_jpeg_decode takes"),
        (dict(workspace=torch.zeros(64, dtype=torch.uint8, device=dev)), "workspace must be a contiguous uint8 device tensor of at least"),
    ]
    for over, text in refused:
        with pytest.raises(RuntimeError, match=text):
            call(**over)
    lib_ws = torch.zeros(mjpeg.jpeg_decode_workspace_size(2, 17, 16, p["sampling"], 1) + 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="gsr_jpeg_decode: workspace must be 16-byte aligned"):
        call(workspace=lib_ws[1:])
    assert mjpeg.jpeg_decode_workspace_size(2, 17, 16, 7, 1) == 0 and mjpeg.jpeg_decode_workspace_size(0, 17, 16, 3, 1) == 0
    torch.cuda.synchronize()
    assert (rgb == SENTINEL).all() and (status == -7).all() and (coef == 12345).all()
    call()                                                            # and the same arguments, unchanged, decode
    torch.cuda.synchronize()
    assert np.array_equal(rgb[1].cpu().numpy(), cases.pil_rgb(data)) and not status.any()
