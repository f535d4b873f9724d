"""The arithmetic of the device's JPEG encoder (include/video_io.h, csrc/gs_jpeg.h), restated in numpy: baseline sequential JPEG (ITU-T
T.81), 8 bit, three components, 4:2:0, no restart markers. float64 throughout (dtype= switches the floating-point steps for experiments).
Not a test itself: tests/test_mjpeg_host.py holds it against PIL, tests/test_hip_mjpeg.py holds the device against it.

  input      uint8 [H, W, 3] RGB; padded to multiples of 16 by edge replication, pixels first
  colour     Y = 0.299 R + 0.587 G + 0.114 B - 128, Cb = -0.168736 R - 0.331264 G + 0.5 B, Cr = 0.5 R - 0.418688 G - 0.081312 B (no rounding)
  chroma     0.25 * (sum of each 2 x 2)
  transform  F(u, v) = 1/4 C(u) C(v) sum f(x, y) cos((2x+1) u pi / 16) cos((2y+1) v pi / 16), C(0) = 1 / sqrt 2
  quantise   rint(F / q), half to even; the tables of slam.mjpeg.quant_tables
  scan       MCUs row-major, blocks Y00 Y01 Y10 Y11 Cb Cr, zigzag, DC prediction per component through the whole scan, Annex K Huffman tables,
             ZRL for runs above 15, EOB unless coefficient 63 is non-zero, the last byte padded with 1-bits, 0x00 after every 0xFF
  file       slam.mjpeg.jfif_header + scan + EOI"""
import numpy as np

from slam import mjpeg

_X = np.arange(8)
# DCT[u, x] = 1/2 C(u) cos((2x+1) u pi / 16): F = DCT f DCT^T
DCT = 0.5 * np.where(_X[:, None] == 0, 1.0 / np.sqrt(2.0), 1.0) * np.cos((2 * _X[None, :] + 1) * _X[:, None] * np.pi / 16)


def adversarial_picture(H, W, seed=0):
    """uint8 [H, W, 3]: 16 x 16 tiles that cycle through a smooth noisy pattern, black and white 8 x 8 blocks, a one-pixel checkerboard and a
    horizontal ramp. It yields DC steps of 2040, long zero runs (ZRL) and many 0xFF bytes in the scan."""
    rng = np.random.default_rng(seed)
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    y, x = np.mgrid[0:Hp, 0:Wp]
    smooth = 128 + 60 * np.sin(x / 9.0)[..., None] * np.cos(y / 7.0)[..., None] * np.array([1.0, 0.8, -0.9]) + rng.normal(0, 6, (Hp, Wp, 3))
    blocks = np.where(((x // 8 + y // 8) & 1)[..., None] == 1, 255.0, 0.0) * np.ones(3)
    checker = np.where(((x + y) & 1)[..., None] == 1, 255.0, 0.0) * np.ones(3)
    ramp = ((x % 16) * 17.0)[..., None] * np.array([1.0, 0.5, 0.25]) + np.array([0.0, 60.0, 120.0])
    kind = ((x // 16 + y // 16) % 4)[..., None]
    out = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [smooth, blocks, checker, ramp])
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)[:H, :W].copy()


def smooth_picture(H, W, seed=0):
    """uint8 [H, W, 3]: low frequencies plus a little noise, the kind of picture a renderer produces."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 128 + 90 * np.sin(x / 23.0 + seed)[..., None] * np.cos(y / 17.0)[..., None] * np.array([1.0, -0.7, 0.5]) + (x + y)[..., None] * 0.1
    return np.clip(np.rint(base + rng.normal(0, 2, (H, W, 3))), 0, 255).astype(np.uint8)


def planes(rgb, dtype=np.float64):
    """(Y [Hp, Wp], Cb [Hp/2, Wp/2], Cr) of the padded picture."""
    H, W, _ = rgb.shape
    p = np.pad(rgb, ((0, -H % 16), (0, -W % 16), (0, 0)), mode="edge").astype(dtype)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    c = lambda v: dtype(v)  # noqa: E731
    Y = c(0.299) * R + c(0.587) * G + c(0.114) * B - c(128)
    Cb = c(-0.168736) * R - c(0.331264) * G + c(0.5) * B
    Cr = c(0.5) * R - c(0.418688) * G - c(0.081312) * B
    half = lambda a: c(0.25) * (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2])  # noqa: E731
    return Y, half(Cb), half(Cr)


def _blocks(plane):
    """[rows, cols, 8, 8] of a plane whose sides are multiples of 8."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def quotients(rgb, qtables, dtype=np.float64):
    """F / q before rounding as [mcu rows, mcu cols, 6, 64], blocks in scan order, coefficients in zigzag order."""
    q = np.asarray(qtables).astype(dtype)
    d = DCT.astype(dtype)
    Y, Cb, Cr = planes(rgb, dtype)
    F = [np.einsum("uy,rcyx,vx->rcuv", d, _blocks(p), d) for p in (Y, Cb, Cr)]          # [.., vertical frequency, horizontal frequency]
    zz = [f.reshape(f.shape[0], f.shape[1], 64)[..., mjpeg.ZIGZAG] / q[min(i, 1)] for i, f in enumerate(F)]
    y = zz[0]
    return np.stack([y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2], zz[1], zz[2]], axis=2)


def coefficients(rgb, qtables, dtype=np.float64):
    """int16 [mcu rows, mcu cols, 6, 64]: rint(F / q), half to even."""
    return np.rint(quotients(rgb, qtables, dtype)).astype(np.int16)


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.events = {"dc_category_max": 0, "zrl": 0, "stuffed": 0, "largest": 0}

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self._byte((self.acc >> self.n) & 0xFF)
        self.acc &= (1 << self.n) - 1

    def _byte(self, b):
        self.out.append(b)
        if b == 0xFF:
            self.out.append(0)
            self.events["stuffed"] += 1

    def finish(self):
        if self.n:
            self._byte(((self.acc << (8 - self.n)) | ((1 << (8 - self.n)) - 1)) & 0xFF)
        return bytes(self.out)


def _magnitude(v):
    """(category, the category's extra bits) of a non-zero difference or coefficient (T.81 F.1.2.1)."""
    cat = int(abs(v)).bit_length()
    return cat, (v if v > 0 else v - 1) & ((1 << cat) - 1)


def entropy_code(coef, events=None):
    """The entropy-coded segment of coefficients [mcu rows, mcu cols, 6, 64] (zigzag): Huffman coded, padded with 1-bits, byte-stuffed.
    events, when a dict, receives {"dc_category_max", "zrl", "stuffed", "largest"}."""
    h = mjpeg.huffman_tables()
    dc = [mjpeg.huffman_codes(h["dc0"]), mjpeg.huffman_codes(h["dc1"])]
    ac = [mjpeg.huffman_codes(h["ac0"]), mjpeg.huffman_codes(h["ac1"])]
    bits = _Bits()
    pred = [0, 0, 0]
    flat = np.asarray(coef).reshape(-1, 6, 64).astype(np.int64)
    for mcu in flat:
        for k in range(6):
            comp = max(k - 3, 0)
            t = min(comp, 1)
            block = [int(v) for v in mcu[k]]
            diff = block[0] - pred[comp]
            pred[comp] = block[0]
            cat, extra = _magnitude(diff) if diff else (0, 0)
            bits.events["dc_category_max"] = max(bits.events["dc_category_max"], cat)
            bits.put(*dc[t][cat])
            bits.put(extra, cat)
            run = 0
            for z in range(1, 64):
                v = block[z]
                if v == 0:
                    run += 1
                    continue
                bits.events["largest"] = max(bits.events["largest"], abs(v))
                while run > 15:
                    bits.put(*ac[t][0xF0])
                    bits.events["zrl"] += 1
                    run -= 16
                size, extra = _magnitude(v)
                bits.put(*ac[t][run << 4 | size])
                bits.put(extra, size)
                run = 0
            if block[63] == 0:
                bits.put(*ac[t][0x00])
    out = bits.finish()
    if events is not None:
        events.update(bits.events)
    return out


def encode(rgb, quality, dtype=np.float64, events=None):
    """The bytes of the JPEG file of uint8 [H, W, 3]."""
    q = mjpeg.quant_tables(quality)
    H, W, _ = rgb.shape
    return mjpeg.jfif_header(W, H, q) + entropy_code(coefficients(rgb, q, dtype), events) + mjpeg.EOI


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
