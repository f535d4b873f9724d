"""Motion-JPEG output: the tables and headers of baseline JPEG (ITU-T T.81: 8 bit, three components, 4:2:0, the Annex K tables), the checked
ctypes binding of include/video_io.h (gsr_jpeg_encode: colour conversion, DCT, quantisation and Huffman coding on the device, csrc/gs_jpeg.h)
and a plain RIFF AVI 1.0 container for the frames (AviWriter, read_avi). The host runs no compressor: a file is jfif_header() + the device's
entropy-coded segment + EOI. tests/jpeg_reference.py restates the encoder's arithmetic in numpy. jpeg_decode is the binding of the inverse
(gsr_jpeg_decode, csrc/gs_jpeg_decode.h): pictures from entropy-coded segments and the tables slam/jpeg_decode.py parses out of the headers;
tests/jpeg_decode_reference.py restates its arithmetic."""
import struct

import numpy as np
import torch

from diff_gaussian_rasterization import _C

# zigzag position -> natural (row-major, row = vertical frequency) index of an 8 x 8 block (T.81 figure 5)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
# T.81 Annex K.1 (luminance) and K.2 (chrominance), natural order
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# T.81 Annex K.3 - K.6: (number of codes of length 1 .. 16, the symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))


def _rows(first, last, lo=1, hi=10):
    return [h << 4 | l for h in range(first, last + 1) for l in range(lo, hi + 1)]


AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
            0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a] + _rows(4, 7, 3) + _rows(8, 8, 3) + _rows(9, 13, 2) +
           _rows(14, 15, 1))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
              0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
              0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a] + _rows(4, 7, 3) + _rows(8, 15, 2))

EOI = b"\xff\xd9"
AVI_LIMIT = 2 ** 31 - 1                                            # AVI 1.0: one RIFF chunk, 32-bit sizes that every reader takes as signed


def quant_tables(quality):
    """The two quantisation tables (luminance, chrominance) as uint16 [2, 64] in zigzag order: Annex K.1 / K.2 scaled by libjpeg's quality
    rule, s = 5000 / Q below 50 and 200 - 2 Q from 50, q = clamp((base * s + 50) div 100, 1, 255)."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer from 1 to 100, got {quality!r}")
    q = int(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * s + 50) // 100, 1, 255)[ZIGZAG] for base in (K1, K2)]).astype(np.uint16)


def huffman_tables():
    """The Annex K.3 - K.6 tables: {"dc0", "ac0", "dc1", "ac1"} -> (counts of the code lengths 1 .. 16, symbols in code order)."""
    return {"dc0": DC_LUMA, "ac0": AC_LUMA, "dc1": DC_CHROMA, "ac1": AC_CHROMA}


def huffman_codes(table):
    """{symbol: (code, length)} of one (counts, symbols) table (T.81 Annex C)."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jfif_header(width, height, qtables):
    """Everything of a JPEG file before the entropy-coded segment: SOI, APP0 "JFIF" 1.01 (units 0, density 1:1), two 8-bit DQT, SOF0 (Y 2 x 2
    on table 0, Cb and Cr 1 x 1 on table 1), four DHT (DC0, AC0, DC1, AC1), SOS."""
    q = np.asarray(qtables)
    if q.shape != (2, 64) or q.min() < 1 or q.max() > 255:
        raise ValueError("qtables must be [2, 64] with entries from 1 to 255 (quant_tables())")
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise ValueError(f"a JPEG frame is 1 .. 65535 pixels wide and high, got {width} x {height}")
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for t in range(2):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in q[t]))
    out += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    h = huffman_tables()
    for ident, name in ((0x00, "dc0"), (0x10, "ac0"), (0x01, "dc1"), (0x11, "ac1")):
        out += _segment(0xC4, bytes([ident]) + bytes(h[name][0]) + bytes(h[name][1]))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def mcu_grid(width, height):
    """(rows, columns) of 16 x 16 MCUs."""
    return (height + 15) // 16, (width + 15) // 16


def jpeg_workspace_size(views, width, height):
    return int(_C.load_library().gsr_jpeg_workspace_size(views, width, height))


_U16 =(torch.int16, getattr(torch, "uint16", torch.int16))


def jpeg_encode(rgb8, qtables, scan, sizes, coefficients=None, workspace=None, stream=None):
    """Baseline JPEG entropy-coded segments of V views, on the device (include/video_io.h gsr_jpeg_encode). rgb8 uint8 [V, H, W, 3] as
    frame_io.frame_export writes it; qtables 16-bit integers [2, 64] in zigzag order (quant_tables()); scan uint8 [V, capacity]: view v's
    segment, byte-stuffed and padded, from scan[v, 0]; sizes int32 [V]: the bytes written, or -(bytes needed) for a view that does not fit its
    capacity (nothing is written beyond it); coefficients None or int16 [V, mcu rows, mcu columns, 6, 64]: the quantised coefficients in scan
    order, zigzag; workspace None (allocated here) or uint8 [>= jpeg_workspace_size(V, W, H)]. stream: a torch stream (default: the current
    stream of rgb8's device). A file is jfif_header(W, H, qtables) + scan[v, :sizes[v]] + EOI."""
    _C._require_device(rgb8, "rgb8")
    if rgb8.dim() != 4 or rgb8.shape[3] != 3:
        raise RuntimeError(f"rgb8 must be [V, H, W, 3], got {tuple(rgb8.shape)}")
    V, H, W, _ = (int(v) for v in rgb8.shape)
    _C._require_device(scan, "scan")
    if scan.dim() != 2:
        raise RuntimeError(f"scan must be [V, capacity], got {tuple(scan.shape)}")
    rows, cols = mcu_grid(W, H)
    _dev = _C.dev_ptr
    args = [_dev(rgb8,"rgb8", (torch.uint8,), (V, H, W, 3)), _dev(qtables, "qtables", _U16, (2, 64)),
            _dev(scan, "scan", (torch.uint8,), (V, scan.shape[1])), int(scan.shape[1]), _dev(sizes, "sizes", (torch.int32,), (V,)),
            None if coefficients is None else _dev(coefficients, "coefficients", (torch.int16,), (V, rows, cols, 6, 64))]
    lib = _C.load_library()
    need = int(lib.gsr_jpeg_workspace_size(V, W, H))
    if need == 0:
        raise RuntimeError(f"rgb8: {V} views of {W} x {H} are outside what gsr_jpeg_encode takes")
    workspace = _C.workspace(workspace, need, rgb8.device)
    with torch.cuda.device(rgb8.device):
        lib.gsr_jpeg_encode(V, W, H, *args, workspace.data_ptr(), int(workspace.numel()), _C.stream_handle(stream, rgb8.device))


_BLOCKS_PER_MCU, _MCU_SIZE = (1, 3, 4, 6), ((8, 8), (8, 8), (16, 8), (16, 16))     # by GSR_JPEG_GREY, _444, _422, _420; (wide, high)
_I16 = (torch.int16, getattr(torch, "uint16", torch.int16))


def jpeg_decode_workspace_size(frames, width, height, sampling, max_intervals=1):
    return int(_C.load_library().gsr_jpeg_decode_workspace_size(frames, width, height, sampling, max_intervals))


def jpeg_decode(scans, offsets, qtables, huffman, descriptors, rgb8, status, sampling, max_intervals=1, coefficients=None, workspace=None,
                stream=None):
    """Baseline JPEG pictures from their entropy-coded segments, on the device (include/video_io.h gsr_jpeg_decode): the inverse of
    jpeg_encode in libjpeg's arithmetic. The inputs are slam.jpeg_decode.pack()'s arrays as device tensors: scans uint8 [bytes]; offsets
    int64 [F + 1]; qtables 16-bit [F, 3, 64] (per component, natural order); huffman int32 [F, 4, 96]; descriptors int32 [F, 8]. rgb8 uint8
    [F, H, W, 3] and status int32 [F] (a GSR_JPEG_* code, 0 = decoded) are written. sampling: GSR_JPEG_GREY / _444 / _422 / _420;
    max_intervals: the most restart intervals of any frame (pack()["max_intervals"]). coefficients None or int16 [F, mcu rows, mcu columns,
    blocks per MCU, 64]: the quantised coefficients in scan order, zigzag. workspace None (allocated here) or uint8
    [>= jpeg_decode_workspace_size(...)]. stream: a torch stream (default: the current stream of rgb8's device)."""
    _C._require_device(rgb8, "rgb8")
    if rgb8.dim() != 4 or rgb8.shape[3] != 3:
        raise RuntimeError(f"rgb8 must be [F, H, W, 3], got {tuple(rgb8.shape)}")
    F, H, W, _ = (int(v) for v in rgb8.shape)
    if isinstance(sampling, bool) or not isinstance(sampling, (int, np.integer)) or not 0 <= int(sampling) <= 3:
        raise RuntimeError(f"sampling must be GSR_JPEG_GREY (0), _444 (1), _422 (2) or _420 (3), got {sampling!r}")
    sampling = int(sampling)
    _C._require_device(scans, "scans")
    if scans.dim() != 1:
        raise RuntimeError(f"scans must be [bytes], got {tuple(scans.shape)}")
    mw, mh = _MCU_SIZE[sampling]
    rows, cols = -(-H // mh), -(-W // mw)
    _dev = _C.dev_ptr
    args = [_dev(scans, "scans", (torch.uint8,), (scans.shape[0],)), _dev(offsets, "offsets", (torch.int64,), (F + 1,)), int(scans.shape[0]),
            _dev(qtables, "qtables", _I16, (F, 3, 64)), _dev(huffman, "huffman", (torch.int32,), (F, 4, 96)),
            _dev(descriptors, "descriptors", (torch.int32,), (F, 8)), _dev(rgb8, "rgb8", (torch.uint8,), (F, H, W, 3)),
            _dev(status, "status", (torch.int32,), (F,)),
            None if coefficients is None else _dev(coefficients, "coefficients", (torch.int16,), (F, rows, cols, _BLOCKS_PER_MCU[sampling], 64))]
    lib = _C.load_library()
    need = int(lib.gsr_jpeg_decode_workspace_size(F, W, H, sampling, int(max_intervals)))
    if need == 0:
        raise RuntimeError(f"rgb8: {F} frames of {W} x {H} with max_intervals {max_intervals} are outside what gsr_jpeg_decode takes "
                           f"(max_intervals from 1 to the {rows * cols} MCUs of a frame)")
    workspace = _C.workspace(workspace, need, rgb8.device)
    with torch.cuda.device(rgb8.device):
        lib.gsr_jpeg_decode(F, W, H, sampling, int(max_intervals), *args, workspace.data_ptr(), int(workspace.numel()),
                            _C.stream_handle(stream, rgb8.device))


# ---- container ---------------------------------------------------------------------------------------------------------------------
class AviWriter:
    """A Motion-JPEG file in plain RIFF AVI 1.0: RIFF 'AVI ' { LIST 'hdrl' { avih, LIST 'strl' { strh, strf } }, LIST 'movi' { 00dc ... },
    idx1 }. add(jpeg_bytes) appends one frame (a whole JPEG file); close() writes the index and patches the totals. The file stays below
    2^31 - 1 bytes: an add() that would cross that closes the file validly and raises ValueError."""
    HEADER = 12 + (12 + (8 + 56) + (12 + (8 + 56) + (8 + 40))) + 12             # up to and including 'movi'

    def __init__(self, path, width, height, fps):
        if not (width >= 1 and height >= 1 and fps > 0):
            raise ValueError(f"AviWriter needs a positive size and rate, got {width} x {height} at {fps}")
        self.path, self.width, self.height, self.fps = path, int(width), int(height), float(fps)
        self.index, self.largest, self.closed = [], 0, False
        self.f = open(path, "wb")
        self.f.write(self._header())
        self.size = self.HEADER

    def _header(self):
        n, w, h = len(self.index), self.width, self.height
        rate = int(round(self.fps * 1000))
        movi = 4 + sum(8 + s + (s & 1) for _, s in self.index)
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), min(int(self.largest * self.fps), 0xFFFFFFFF), 0, 0x10, n, 0, 1, self.largest, w, h, 0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHH8I4h", 0, 0, 0, 0, 1000, rate, 0, n, self.largest, 0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + 56 + 8 + 40) + b"strl" + b"strh" + struct.pack("<I", 56) + strh + b"strf" + struct.pack("<I", 40) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + 56 + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", 56) + avih + strl
        riff = 4 + len(hdrl) + 8 + movi + 8 + 16 * n
        out = b"RIFF" + struct.pack("<I", riff) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", movi) + b"movi"
        assert len(out) == self.HEADER and len(strh) == 56 and len(avih) == 56
        return out

    def add(self, jpeg_bytes):
        if self.closed:
            raise ValueError(f"{self.path} is closed")
        s = len(jpeg_bytes)
        if self.size + 8 + s + (s & 1) + 8 + 16 * (len(self.index) + 1) > AVI_LIMIT:
            self.close()
            raise ValueError(f"{self.path}: frame {len(self.index)} would take the file past {AVI_LIMIT} bytes, the limit of AVI 1.0; it was closed "
                             f"with {len(self.index)} frames: split the path into several files")
        self.f.write(b"00dc" + struct.pack("<I", s))
        self.f.write(jpeg_bytes)
        if s & 1:
            self.f.write(b"\0")
        self.index.append((self.size - (self.HEADER - 4), s))                # offset of the chunk from the 'movi' fourcc
        self.size += 8 + s + (s & 1)
        self.largest = max(self.largest, s)

    def close(self):
        if self.closed:
            return
        self.closed = True
        try:
            self.f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
            self.f.write(b"".join(b"00dc" + struct.pack("<III", 0x10, off, s) for off, s in self.index))
            self.size += 8 + 16 * len(self.index)
            self.f.seek(0)
            self.f.write(self._header())
        finally:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_avi(path):
    """(info, frames) of a file AviWriter wrote (or any AVI 1.0 file with one video stream and an idx1): info = {"width", "height", "fps",
    "frames", "handler", "compression", "scale", "rate", "flags"}, frames = the bytes of every 00dc chunk, read through the index and checked
    against a walk of 'movi' (ValueError when they disagree or the structure is broken)."""
    with open(path, "rb") as f:
        data = f.read()

    def chunks(lo, hi):
        while lo + 8 <= hi:
            four, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
            if lo + 8 + size > hi:
                raise ValueError(f"{path}: chunk {four!r} at {lo} runs past its parent")
            yield four, lo + 8, size
            lo += 8 + size + (size & 1)

    if data[:4] != b"RIFF" or data[8:12] != b"AVI " or struct.unpack_from("<I", data, 4)[0] + 8 != len(data):
        raise ValueError(f"{path}: not a RIFF AVI file of its own length")
    info, movi, idx = {}, None, None
    for four, at, size in chunks(12, len(data)):
        if four == b"LIST" and data[at:at + 4] == b"hdrl":
            for f2, a2, s2 in chunks(at + 4, at + size):
                if f2 == b"avih":
                    v = struct.unpack_from("<14I", data, a2)
                    info.update(us_per_frame=v[0], flags=v[3], frames=v[4], streams=v[6], width=v[8], height=v[9])
                elif f2 == b"LIST" and data[a2:a2 + 4] == b"strl":
                    for f3, a3, s3 in chunks(a2 + 4, a2 + s2):
                        if f3 == b"strh":
                            scale, rate, _, length = struct.unpack_from("<4I", data, a3 + 20)
                            info.update(type=data[a3:a3 + 4], handler=data[a3 + 4:a3 + 8], scale=scale, rate=rate, length=length, fps=rate / scale)
                        elif f3 == b"strf":
                            v = struct.unpack_from("<IiiHH4sI", data, a3)
                            info.update(bitmap_size=v[0], bitmap_width=v[1], bitmap_height=v[2], planes=v[3], bit_count=v[4], compression=v[5])
        elif four == b"LIST" and data[at:at + 4] == b"movi":
            movi = (at, size)
        elif four == b"idx1":
            idx = (at, size)
    if movi is None or idx is None or "fps" not in info or "width" not in info:
        raise ValueError(f"{path}: hdrl, movi or idx1 is missing")
    walked = [(a - 8 - movi[0], s) for four, a, s in chunks(movi[0] + 4, movi[0] + movi[1]) if four == b"00dc"]
    indexed = []
    for k in range(idx[1] // 16):
        four, flags, off, s = struct.unpack_from("<4sIII", data, idx[0] + 16 * k)
        if four != b"00dc" or flags != 0x10:
            raise ValueError(f"{path}: index entry {k} is {four!r} with flags {flags:#x}")
        indexed.append((off, s))
    if indexed != walked or len(indexed) != info["frames"] or info["length"] != info["frames"]:
        raise ValueError(f"{path}: the index ({len(indexed)} entries), the movi list ({len(walked)} chunks) and the headers ({info['frames']} frames) disagree")
    return info, [data[movi[0] + off + 8:movi[0] + off + 8 + s] for off, s in indexed]
