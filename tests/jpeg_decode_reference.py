"""The arithmetic of the device's JPEG decoder (include/video_io.h gsr_jpeg_decode, csrc/gs_jpeg_decode.h), restated in integer numpy:
baseline sequential JPEG (ITU-T T.81), 8 bit, one scan; the arithmetic is libjpeg's default one, so the picture equals PIL's byte for byte.
Not a test itself: tests/test_jpeg_decode_host.py holds it against PIL, tests/test_hip_jpeg_decode.py holds the device against it. It shares
no code with slam/jpeg_decode.py: the marker parser and the Huffman decoder here are its own.

  parse       SOI .. SOS: DQT (8 bit), SOF0, DHT, DRI; a file without DHT gets the Annex K tables
  entropy     bit-serial Huffman decoding (T.81 Annex F.2.2): per block the DC difference and the AC (run, size) pairs, 0x00 after 0xFF
              dropped, DC prediction per component, reset at every restart marker; coefficients in zigzag order
  dequantise  coefficient * table entry
  transform   jidctint.c "slow integer": 13-bit constants, columns with (x + 2^10) >> 11, rows with (x + 2^17) >> 18, + 128, clamp to 0 .. 255
  chroma      2 x 2: s = 3 * (this row) + (the nearer neighbouring row); even columns (3 s[x] + s[x-1] + 8) >> 4, odd columns
              (3 s[x] + s[x+1] + 7) >> 4; 2 x 1: even (3 c[x] + c[x-1] + 1) >> 2, odd (3 c[x] + c[x+1] + 2) >> 2. A neighbour outside the real
              chroma plane (ceil(W / 2) x ceil(H / 2), not the block padding) is the edge sample itself. 1 x 1: none
  colour      R = Y + ((F(1.402) Cr + 32768) >> 16), G = Y + ((-F(0.34414) Cb - F(0.71414) Cr + 32768) >> 16), B = Y + ((F(1.772) Cb + 32768) >> 16)
              with F(v) = int(v * 65536 + 0.5), Cb and Cr minus 128, clamp; one component: R = G = B = Y"""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# status of a scan (the device's codes, include/video_io.h)
OK, OUT_OF_BYTES, LONG_CODE, INDEX_PAST_63, RESTART = 0, 1, 2, 3, 4


def _annex_k():
    rows = lambda first, last, lo: [h << 4 | l for h in range(first, last + 1) for l in range(lo, 11)]  # noqa: E731
    dc0 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
    dc1 = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
    ac0 = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
            0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
            0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a] + rows(4, 7, 3) + rows(8, 8, 3) + rows(9, 13, 2) +
           rows(14, 15, 1))
    ac1 = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
           [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
            0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
            0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a] + rows(4, 7, 3) + rows(8, 15, 2))
    return {(0, 0): dc0, (0, 1): dc1, (1, 0): ac0, (1, 1): ac1}


def parse(data):
    """{"width", "height", "components": [(h, v, quantisation table, DC table, AC table)], "qtables": {id: int [64] natural order},
    "huffman": {(class, id): (counts, symbols)}, "restart_interval", "scan": the bytes behind the SOS header} of a baseline file."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    out = {"qtables": {}, "huffman": {}, "restart_interval": 0}
    at = 2
    while True:
        if at + 4 > len(data) or data[at] != 0xFF:
            raise ValueError(f"no marker at byte {at}")
        marker, length = data[at + 1], struct.unpack_from(">H", data, at + 2)[0]
        body = data[at + 4:at + 2 + length]
        if len(body) != length - 2:
            raise ValueError("truncated segment")
        at += 2 + length
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("16-bit quantisation table")
                out["qtables"][body[0] & 15] = np.frombuffer(body[1:65], np.uint8).astype(np.int64)[np.argsort(ZIGZAG)]
                body = body[65:]
        elif marker == 0xC4:
            while body:
                counts = list(body[1:17])
                out["huffman"][(body[0] >> 4, body[0] & 15)] = (counts, list(body[17:17 + sum(counts)]))
                body = body[17 + sum(counts):]
        elif marker == 0xDD:
            out["restart_interval"] = struct.unpack(">H", body)[0]
        elif marker == 0xC0:
            precision, out["height"], out["width"], n = struct.unpack_from(">BHHB", body)
            if precision != 8:
                raise ValueError("not 8 bit")
            frame = [(body[6 + 3 * k], body[7 + 3 * k] >> 4, body[7 + 3 * k] & 15, body[8 + 3 * k]) for k in range(n)]
        elif 0xC1 <= marker <= 0xCF and marker != 0xC8:
            raise ValueError(f"SOF{marker - 0xC0} is not baseline")
        elif marker == 0xDA:
            n = body[0]
            sel = {body[1 + 2 * k]: (body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k in range(n)}
            if n != len(frame) or tuple(body[1 + 2 * n:4 + 2 * n]) != (0, 63, 0):
                raise ValueError("not one sequential scan of all components")
            out["components"] = [(h, v, tq) + sel[ident] for ident, h, v, tq in frame]
            out["scan"] = data[at:]
            if not out["huffman"]:
                out["huffman"] = _annex_k()
            return out


class _BitReader:
    """The bits of one restart interval: 0x00 after 0xFF dropped; a marker ends the data."""

    def __init__(self, data):
        self.data, self.at, self.acc, self.n = data, 0, 0, 0

    def bit(self):
        if self.n == 0:
            if self.at >= len(self.data):
                raise EOFError
            b = self.data[self.at]
            self.at += 1
            if b == 0xFF:
                if self.at >= len(self.data) or self.data[self.at] != 0:
                    self.at = len(self.data)
                    raise EOFError
                self.at += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, count):
        v = 0
        for _ in range(count):
            v = v << 1 | self.bit()
        return v


def _decoder(table):
    """(mincode, maxcode, valptr, symbols) of Annex F.2.2.3, figure F.15."""
    counts, symbols = table
    mincode, maxcode, valptr, code, k = [0] * 17, [-1] * 17, [0] * 17, 0, 0
    for length in range(1, 17):
        if counts[length - 1]:
            valptr[length], mincode[length] = k, code
            k += counts[length - 1]
            code += counts[length - 1]
            maxcode[length] = code - 1
        code <<= 1
    return mincode, maxcode, valptr, symbols


class _Bad(Exception):
    pass


def _symbol(r, dec):
    mincode, maxcode, valptr, symbols = dec
    code = 0
    for length in range(1, 17):
        code = code << 1 | r.bit()
        if code <= maxcode[length]:
            return symbols[valptr[length] + code - mincode[length]]
    raise _Bad(LONG_CODE)


def _extend(v, size):
    return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def split_intervals(scan):
    """The byte ranges between the restart markers of a scan, with each marker's number: [(bytes, number of the marker before, or None)]."""
    a = np.frombuffer(scan, np.uint8)
    at = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] >= 0xD0) & (a[1:] <= 0xD7)) if len(a) > 1 else np.zeros(0, np.int64)
    out, lo, number = [], 0, None
    for p in at:
        out.append((scan[lo:p], number))
        lo, number = int(p) + 2, int(a[p + 1]) & 7
    out.append((scan[lo:], number))
    return out


def decode_coefficients(p):
    """(coefficients int16 [mcu rows, mcu cols, blocks per MCU, 64] zigzag with the DC values, status) of parse()'s result. An interval that
    cannot be decoded keeps what it decoded, zero elsewhere; the status is that of the first such interval."""
    comps = p["components"]
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    if len(comps) == 1:
        comps, hmax, vmax = [(1, 1) + comps[0][2:]], 1, 1
    rows, cols = -(-p["height"] // (8 * vmax)), -(-p["width"] // (8 * hmax))
    order = [k for k, c in enumerate(comps) for _ in range(c[0] * c[1])]
    coef = np.zeros((rows * cols, len(order), 64), np.int16)
    dc = [_decoder(p["huffman"][(0, c[3])]) for c in comps]
    ac = [_decoder(p["huffman"][(1, c[4])]) for c in comps]
    ri = p["restart_interval"] or rows * cols
    count = -(-rows * cols // ri)
    found = split_intervals(p["scan"])
    status = RESTART if len(found) > count else OK
    for k in range(count):
        code = OK
        if k >= len(found) or (k > 0 and found[k][1] != (k - 1) & 7):
            code = RESTART
        else:
            r, pred = _BitReader(found[k][0]), [0] * len(comps)
            try:
                for mcu in range(k * ri, min((k + 1) * ri, rows * cols)):
                    for b, c in enumerate(order):
                        size = _symbol(r, dc[c])
                        if size > 16:
                            raise _Bad(LONG_CODE)
                        pred[c] += _extend(r.bits(size), size)
                        coef[mcu, b, 0] = np.clip(pred[c], -32768, 32767)
                        z = 1
                        while z < 64:
                            rs = _symbol(r, ac[c])
                            run, size = rs >> 4, rs & 15
                            if size == 0:
                                if run != 15:
                                    break
                                z += 16
                                continue
                            z += run
                            if z > 63:
                                raise _Bad(INDEX_PAST_63)
                            coef[mcu, b, z] = _extend(r.bits(size), size)
                            z += 1
                        if z > 64:
                            raise _Bad(INDEX_PAST_63)
            except EOFError:
                code = OUT_OF_BYTES
            except _Bad as e:
                code = e.args[0]
        if status == OK:
            status = code
    return coef.reshape(rows, cols, len(order), 64), status


def idct(block):
    """uint8-range int64 [..., 8, 8] samples of dequantised int64 [..., 8, 8] (row = vertical frequency): jidctint.c."""
    def pass_1d(v, shift):                                          # along the last axis' partner: v[k] are the eight inputs
        z2, z3 = v[2], v[6]
        z1 = (z2 + z3) * 4433
        tmp2, tmp3 = z1 - z3 * 15137, z1 + z2 * 6270
        tmp0, tmp1 = (v[0] + v[4]) << 13, (v[0] - v[4]) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
        z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
        z5 = (z3 + z4) * 9633
        tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
        half = 1 << (shift - 1)
        # the device's sums are 32-bit two's complement: the same value unless a damaged stream's block leaves the bound of video_io.h
        return [((a + half + (1 << 31)) % (1 << 32) - (1 << 31)) >> shift for a in (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                                              tmp10 - tmp3)]

    b = np.asarray(block, np.int64)
    cols = np.stack(pass_1d([b[..., k, :] for k in range(8)], 11), axis=-2)          # columns: over the vertical frequency
    rows = np.stack(pass_1d([cols[..., :, k] for k in range(8)], 18), axis=-1)
    return np.clip(rows + 128, 0, 255)


def component_planes(p, coef):
    """The sample planes [rows * 8 * v, cols * 8 * h] int64 of every component."""
    comps = p["components"] if len(p["components"]) > 1 else [(1, 1) + p["components"][0][2:]]
    rows, cols = coef.shape[:2]
    inverse = np.argsort(ZIGZAG)
    planes, b = [], 0
    for h, v, tq, _, _ in comps:
        c = coef[:, :, b:b + h * v].astype(np.int64)[..., inverse] * p["qtables"][tq]
        s = idct(c.reshape(rows, cols, v, h, 8, 8))
        planes.append(s.transpose(0, 2, 4, 1, 3, 5).reshape(rows * v * 8, cols * h * 8))
        b += h * v
    return planes


def _upsample_h(s, W, three, bias_even, bias_odd, shift):
    """Columns: even (3 s[x] + s[x-1] + bias_even) >> shift, odd (3 s[x] + s[x+1] + bias_odd) >> shift, edge neighbours replicated."""
    left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (three * s + left + bias_even) >> shift
    out[:, 1::2] = (three * s + right + bias_odd) >> shift
    return out[:, :W]


def upsample(plane, h, v, W, H):
    """A chroma plane at full size [H, W]; (h, v) the luminance sampling against it: (1, 1), (2, 1) or (2, 2)."""
    if (h, v) == (1, 1):
        return plane[:H, :W]
    c = plane[:-(-H // v), :-(-W // 2)]                              # the real samples
    if (h, v) == (2, 1):
        return _upsample_h(c, W, 3, 1, 2, 2)
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    return _upsample_h(s[:H], W, 3, 8, 7, 4)


def _fix(v):
    return int(v * 65536 + 0.5)


def to_rgb(p, planes):
    W, H = p["width"], p["height"]
    Y = planes[0][:H, :W]
    if len(planes) == 1:
        return np.repeat(Y[..., None], 3, 2).astype(np.uint8)
    h, v = p["components"][0][:2]
    cb, cr = (upsample(q, h, v, W, H) - 128 for q in planes[1:])
    r = Y + ((_fix(1.402) * cr + 32768) >> 16)
    g = Y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    b = Y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """(rgb uint8 [H, W, 3], coefficients, status) of the bytes of a baseline JPEG file."""
    p = parse(data)
    coef, status = decode_coefficients(p)
    return to_rgb(p, component_planes(p, coef)), coef, status
