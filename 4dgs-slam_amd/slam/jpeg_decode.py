"""The host side of Motion-JPEG input: where the frames of a video are (AviIndex over a RIFF AVI file, JpegFolder over a directory of .jpg
files), the marker parser that turns one frame's bytes into what the device decoder takes (parse_frame: SOI .. SOS of baseline JPEG), and
pack(), which joins a chunk of parsed frames into the arrays of one mjpeg.jpeg_decode call (include/video_io.h gsr_jpeg_decode). No device
call here: this runs on a dataset's read-ahead thread, like frame_decode.py. Everything that is not an 8-bit baseline file of one scan in an
accepted sampling is refused with a ValueError that names the frame and the reason; nothing is decoded approximately."""
import os
import struct
import time

import numpy as np

from diff_gaussian_rasterization import _abi
from slam import mjpeg

# (components, luminance sampling) -> GSR_JPEG_*: the samplings whose restated arithmetic (tests/jpeg_decode_reference.py) equals libjpeg's
# in every byte (tests/test_jpeg_decode_host.py); the chroma components are always 1 x 1
SAMPLINGS = {(1, (1, 1)): _abi.GSR_JPEG_GREY, (3, (1, 1)): _abi.GSR_JPEG_444, (3, (2, 1)): _abi.GSR_JPEG_422, (3, (2, 2)): _abi.GSR_JPEG_420}
SAMPLING_NAMES = {_abi.GSR_JPEG_GREY: "grey", _abi.GSR_JPEG_444: "4:4:4", _abi.GSR_JPEG_422: "4:2:2", _abi.GSR_JPEG_420: "4:2:0"}
MCU_SIZE = {_abi.GSR_JPEG_GREY: (8, 8), _abi.GSR_JPEG_444: (8, 8), _abi.GSR_JPEG_422: (16, 8), _abi.GSR_JPEG_420: (16, 16)}     # (wide, high)
BLOCKS_PER_MCU = {_abi.GSR_JPEG_GREY: 1, _abi.GSR_JPEG_444: 3, _abi.GSR_JPEG_422: 4, _abi.GSR_JPEG_420: 6}
HUFF_WORDS, DESC_WORDS = 96, 8
_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential", 0xC6: "differential progressive",
              0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential", 0xCA: "arithmetic-coded progressive",
              0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential sequential", 0xCE: "arithmetic-coded differential progressive",
              0xCF: "arithmetic-coded differential lossless"}


def mcu_grid(width, height, sampling):
    """(rows, columns) of MCUs."""
    w, h = MCU_SIZE[sampling]
    return -(-height // h), -(-width // w)


def device_huffman(table, where="a Huffman table", dc=False):
    """int32 [96] of one (counts of the code lengths 1 .. 16, symbols in code order) table, the form the kernel decodes from: limit[16], one
    past the largest code of each length shifted left to 16 bits (the previous limit where no code has that length); offset[16], the index
    of the length's first symbol minus its first code; the 256 symbols, four to a word."""
    counts, symbols = list(table[0]), list(table[1])
    if len(counts) != 16 or sum(counts) != len(symbols) or len(symbols) > 256:
        raise ValueError(f"{where}: {sum(counts)} codes counted, {len(symbols)} symbols")
    if dc and any(s > 15 for s in symbols):
        raise ValueError(f"{where}: a DC category above 15")
    out = np.zeros(HUFF_WORDS, np.int32)
    code, k, limit = 0, 0, 0
    for length in range(1, 17):
        out[16 + length - 1] = k - code
        code, k = code + counts[length - 1], k + counts[length - 1]
        if code > 1 << length:
            raise ValueError(f"{where}: more codes of {length} bits than there are")
        if counts[length - 1]:
            limit = code << (16 - length)
        out[length - 1] = limit
        code <<= 1
    vals = np.zeros(256, np.uint8)
    vals[:len(symbols)] = symbols
    out[32:] = vals.view("<u4").astype(np.int64).astype(np.uint32).view(np.int32)
    return out


_DEFAULT_HUFFMAN = None


def default_huffman():
    """int32 [4, 96]: the Annex K tables (DC 0, DC 1, AC 0, AC 1), for frames without DHT."""
    global _DEFAULT_HUFFMAN
    if _DEFAULT_HUFFMAN is None:
        h = mjpeg.huffman_tables()
        _DEFAULT_HUFFMAN = np.stack([device_huffman(h["dc0"], dc=True), device_huffman(h["dc1"], dc=True), device_huffman(h["ac0"]), device_huffman(h["ac1"])])
    return _DEFAULT_HUFFMAN


class ParsedFrame:
    """One frame, ready for pack(): width, height, sampling (GSR_JPEG_*), scan (bytes of the entropy-coded segment), qtables uint16 [3, 64]
    (per component, natural order), huffman int32 [4, 96], descriptor int32 [8], restart_interval, intervals (restart intervals)."""
    __slots__ = ("width", "height", "sampling", "scan", "qtables", "huffman", "descriptor", "restart_interval", "intervals", "decode_ms")


def parse_frame(data, where="frame", width=None, height=None):
    """ParsedFrame of the bytes of one JPEG file. width / height, when given, are what the calibration says. ValueError with `where` and the
    reason for everything the device decoder does not take."""
    def refuse(reason):
        raise ValueError(f"{where}: {reason}")

    if len(data) < 4 or data[:2] != b"\xff\xd8":
        refuse("not a JPEG file (no SOI marker)")
    qt, huff, ri, frame, at = {}, {}, 0, None, 2
    while True:
        while at < len(data) and data[at] == 0xFF and at + 1 < len(data) and data[at + 1] == 0xFF:
            at += 1                                                  # fill bytes
        if at + 4 > len(data):
            refuse("the header is truncated (the file ends before SOS)")
        if data[at] != 0xFF:
            refuse(f"no marker at byte {at}")
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        if marker == 0xD9:
            refuse("EOI before any scan")
        body = data[at + 4:at + 2 + length]
        if length < 2 or len(body) != length - 2:
            refuse(f"the header is truncated (segment {marker:#04x} at byte {at} runs past the end)")
        at += 2 + length
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    refuse("a 16-bit quantisation table")
                if len(body) < 65 or (body[0] & 15) > 3:
                    refuse("a malformed DQT segment")
                qt[body[0] & 15] = np.frombuffer(body[1:65], np.uint8).astype(np.uint16)
                body = body[65:]
        elif marker == 0xC4:
            while body:
                if len(body) < 17:
                    refuse("a malformed DHT segment")
                cls, ident, counts = body[0] >> 4, body[0] & 15, list(body[1:17])
                n = sum(counts)
                if cls > 1 or ident > 1 or len(body) < 17 + n:
                    refuse(f"a malformed DHT segment or a table id above 1 (class {cls}, id {ident}): baseline has two tables per class")
                huff[(cls, ident)] = device_huffman((counts, list(body[17:17 + n])), f"{where}: Huffman table {cls}/{ident}", dc=cls == 0)
                body = body[17 + n:]
        elif marker == 0xDD:
            if len(body) != 2:
                refuse("a malformed DRI segment")
            ri = struct.unpack(">H", body)[0]
        elif marker == 0xC0:
            if frame is not None:
                refuse("two frame headers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                refuse("a malformed SOF0 segment")
            precision, h, w, n = struct.unpack_from(">BHHB", body)
            if precision != 8:
                refuse(f"{precision}-bit samples; only 8 bit is decoded")
            if n not in (1, 3):
                refuse(f"{n} components; 1 (grey) and 3 (Y Cb Cr) are decoded")
            if w < 1 or h < 1:
                refuse(f"a size of {w} x {h}")
            frame = (w, h, [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(n)])
        elif marker in _SOF_NAMES:
            refuse(f"a {_SOF_NAMES[marker]} file (SOF{marker - 0xC0}" + (", 12 bit" if marker == 0xC1 and body[:1] == b"\x0c" else "") +
                   "); only baseline sequential JPEG (SOF0) is decoded")
        elif marker == 0xCC:
            refuse("arithmetic coding conditioning (DAC); only Huffman coding is decoded")
        elif marker == 0xDA:
            break
    if frame is None:
        refuse("SOS before SOF0")
    w, h, comps = frame
    n = len(comps)
    if (width is not None and w != int(width)) or (height is not None and h != int(height)):
        refuse(f"the picture is {w} x {h}, the calibration says {width} x {height}")
    if not body or body[0] != n or len(body) != 4 + 2 * n:
        refuse(f"a scan of {body[0] if body else 0} of the {n} components: several scans are not decoded")
    if tuple(body[1 + 2 * n:]) != (0, 63, 0):
        refuse("a scan with spectral selection or successive approximation (Ss, Se, Ah/Al other than 0, 63, 0)")
    if [body[1 + 2 * k] for k in range(n)] != [c[0] for c in comps]:
        refuse("the scan's components are not the frame's, in order")
    lum = (comps[0][1], comps[0][2]) if n == 3 else (1, 1)           # a single component is not interleaved: its factors do not matter
    if n == 3 and any((c[1], c[2]) != (1, 1) for c in comps[1:]):
        refuse(f"chroma sampling factors {[(c[1], c[2]) for c in comps[1:]]}; only 1 x 1 chroma is decoded")
    if (n, lum) not in SAMPLINGS:
        refuse(f"luminance sampling {lum[0]} x {lum[1]}: only grey, 4:4:4, 4:2:2 (2 x 1) and 4:2:0 (2 x 2) are decoded, the samplings whose "
               "arithmetic has been checked against libjpeg byte for byte")
    out = ParsedFrame()
    out.width, out.height, out.sampling, out.restart_interval = w, h, SAMPLINGS[(n, lum)], ri
    out.qtables = np.ones((3, 64), np.uint16)
    out.descriptor = np.zeros(DESC_WORDS, np.int32)
    out.descriptor[0] = ri
    if not huff:
        out.huffman = default_huffman()                              # AVI producers routinely leave the tables out
    else:
        out.huffman = np.zeros((4, HUFF_WORDS), np.int32)
        for (cls, ident), t in huff.items():
            out.huffman[2 * cls + ident] = t
    natural = np.argsort(mjpeg.ZIGZAG)
    for k, (_, _, _, tq) in enumerate(comps):
        td, ta = body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15
        if tq not in qt:
            refuse(f"component {k} uses quantisation table {tq}, which the file does not define")
        if td > 1 or ta > 1 or (huff and ((0, td) not in huff or (1, ta) not in huff)):
            refuse(f"component {k} uses Huffman tables {td} / {ta}, which the file does not define")
        out.qtables[k] = qt[tq][natural]
        out.descriptor[1 + k], out.descriptor[4 + k] = td, ta
    end = data.rfind(b"\xff\xd9", at)
    out.scan = data[at:end if end >= 0 else len(data)]
    rows, cols = mcu_grid(w, h, out.sampling)
    out.intervals = -(-rows * cols // ri) if 0 < ri < rows * cols else 1
    return out


def read_frame(source, k, width=None, height=None):
    """Frame k of a source, read and parsed (what a dataset's read-ahead thread runs); decode_ms is the host time it took."""
    t0 = time.perf_counter()
    out = parse_frame(source.read(k), source.name(k), width, height)
    out.decode_ms = (time.perf_counter() - t0) * 1e3
    return out


def pack(frames):
    """The host arrays of one device call for a list of ParsedFrame of one size and sampling: {"scans" uint8 [total], "offsets" int64
    [n + 1], "qtables" uint16 [n, 3, 64], "huffman" int32 [n, 4, 96], "descriptors" int32 [n, 8], "max_intervals", "width", "height", "sampling"}."""
    first = frames[0]
    for k, f in enumerate(frames):
        if (f.width, f.height, f.sampling) != (first.width, first.height, first.sampling):
            raise ValueError(f"frame {k} of the chunk is {f.width} x {f.height} {SAMPLING_NAMES[f.sampling]}, the first is {first.width} x {first.height} "
                             f"{SAMPLING_NAMES[first.sampling]}: one call decodes one size and sampling")
    sizes = [len(f.scan) for f in frames]
    return {"scans": np.frombuffer(b"".join(f.scan for f in frames) or b"\0", np.uint8).copy(), "offsets": np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
            "qtables": np.stack([f.qtables for f in frames]), "huffman": np.stack([f.huffman for f in frames]),
            "descriptors": np.stack([f.descriptor for f in frames]), "max_intervals": max(f.intervals for f in frames),
            "width": first.width, "height": first.height, "sampling": first.sampling}


# ---- frame sources -----------------------------------------------------------------------------------------------------------------------
class AviIndex:
    """The video frames of a RIFF AVI 1.0 file (one video stream, as AviWriter and the common Motion-JPEG producers write it): the chunk walk
    reads headers only, keeps (offset, size) of every '00dc' / '00db' chunk, and read(k) fetches one frame's bytes by offset. The file is
    never held in memory. info = {"width", "height", "fps", "frames", "handler", "compression"}."""

    def __init__(self, path):
        self.path, self.info, self.entries = path, {}, []
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(12)
            if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
                raise ValueError(f"{path}: not a RIFF AVI file")
            end = min(size, 8 + struct.unpack_from("<I", head, 4)[0])
            self._walk(f, 12, end, 0)
        if "fps" not in self.info or "width" not in self.info:
            raise ValueError(f"{path}: no avih / strh header of a video stream")
        if self.info.get("compression", b"MJPG").upper() not in (b"MJPG", b"JPEG") or self.info.get("handler", b"MJPG").upper() not in (b"MJPG", b"JPEG", b"\0\0\0\0"):
            raise ValueError(f"{path}: the video stream is {self.info.get('compression')!r} / {self.info.get('handler')!r}; only Motion-JPEG is decoded")
        self.info["frames"] = len(self.entries)

    def _walk(self, f, lo, hi, depth):
        while lo + 8 <= hi:
            f.seek(lo)
            four, size = struct.unpack("<4sI", f.read(8))
            if lo + 8 + size > hi:
                raise ValueError(f"{self.path}: chunk {four!r} at {lo} runs past its parent")
            if four == b"LIST":
                kind = f.read(4)
                if kind in (b"hdrl", b"strl", b"movi") and depth < 4:
                    self._walk(f, lo + 12, lo + 8 + size, depth + 1)
                elif kind == b"rec " and depth < 4:
                    self._walk(f, lo + 12, lo + 8 + size, depth + 1)
            elif four == b"avih":
                v = struct.unpack("<14I", f.read(56))
                self.info.update(us_per_frame=v[0], width=v[8], height=v[9])
            elif four == b"strh":
                b = f.read(36)
                if b[:4] == b"vids" and "fps" not in self.info:
                    scale, rate = struct.unpack_from("<2I", b, 20)
                    if scale == 0 or rate == 0:
                        raise ValueError(f"{self.path}: a video stream without a frame rate")
                    self.info.update(handler=b[4:8], scale=scale, rate=rate, fps=rate / scale)
            elif four == b"strf" and "compression" not in self.info and "fps" in self.info:
                self.info["compression"] = struct.unpack("<IiiHH4s", f.read(20))[5]
            elif four[2:] in (b"dc", b"db") and four[:2] == b"00" and size > 0:
                self.entries.append((lo + 8, size))
            lo += 8 + size + (size & 1)

    def __len__(self):
        return len(self.entries)

    def name(self, k):
        return f"{self.path} frame {k}"

    def time(self, k):
        return k / self.info["fps"]

    def read(self, k):
        off, size = self.entries[k]
        with open(self.path, "rb") as f:
            f.seek(off)
            data = f.read(size)
        if len(data) != size:
            raise ValueError(f"{self.name(k)}: the file ends inside the frame")
        return data


class JpegFolder:
    """The .jpg / .jpeg files of a directory, sorted by name; the time of a frame is its index."""

    def __init__(self, path):
        self.path = path
        self.files = sorted(n for n in os.listdir(path) if n.lower().endswith((".jpg", ".jpeg")))
        if not self.files:
            raise ValueError(f"{path}: no .jpg or .jpeg file")
        self.info = {"fps": 1.0, "frames": len(self.files)}

    def __len__(self):
        return len(self.files)

    def name(self, k):
        return os.path.join(self.path, self.files[k])

    def time(self, k):
        return float(k)

    def read(self, k):
        with open(self.name(k), "rb") as f:
            return f.read()


def open_source(path):
    """AviIndex for a file, JpegFolder for a directory."""
    if os.path.isdir(path):
        return JpegFolder(path)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path}: no such video file or folder of JPEG files")
    return AviIndex(path)
