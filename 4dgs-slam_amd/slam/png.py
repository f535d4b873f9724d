"""A PNG writer for the two image kinds a playback produces: 8-bit RGB [H, W, 3] and 16-bit grey [H, W] (big-endian on disk). One IDAT chunk
from a single zlib.compress call (which releases the GIL, so a writer thread does not hold up the loop that feeds it), every scanline
with filter 0 (None) or filter 2 (Up, computed for the whole image with one numpy subtraction). assemble() frames a zlib stream that was
made elsewhere (slam/png_device.py: on the device) as the same kind of file. numpy and zlib only."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILTERS = {"none": 0, "up": 2}


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(image, filter="up", level=1):
    """The bytes of a PNG file of `image`: uint8 [H, W, 3] (colour type 2, 8 bit) or uint16 [H, W] (colour type 0, 16 bit)."""
    a = np.asarray(image)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3:
        depth, colour = 8, 2
        rows = np.ascontiguousarray(a).reshape(a.shape[0], a.shape[1] * 3)
    elif a.dtype == np.uint16 and a.ndim == 2:
        depth, colour = 16, 0
        rows = a.astype(">u2").view(np.uint8).reshape(a.shape[0], a.shape[1] * 2)
    else:
        raise ValueError(f"png.encode writes uint8 [H, W, 3] or uint16 [H, W] images, got {a.dtype} {a.shape}")
    if filter not in FILTERS:
        raise ValueError(f"png.encode: filter must be one of {sorted(FILTERS)}, got {filter!r}")
    H, W = int(a.shape[0]), int(a.shape[1])
    if H == 0 or W == 0:
        raise ValueError("png.encode: empty image")
    raw = np.empty((H, rows.shape[1] + 1), np.uint8)
    raw[:, 0] = FILTERS[filter]
    if filter == "up":
        raw[0, 1:] = rows[0]                                # (the row above the first is all zeros)
        np.subtract(rows[1:], rows[:-1], out=raw[1:, 1:])   # modulo 256
    else:
        raw[:, 1:] = rows
    header = struct.pack(">IIBBBBB", W, H, depth, colour, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", header) + _chunk(b"IDAT", zlib.compress(raw, level)) + _chunk(b"IEND", b"")


def assemble(width, height, kind, stream_bytes):
    """The bytes of a PNG file whose one IDAT chunk is `stream_bytes`, a complete zlib stream of the filtered scanlines: kind 0 is 8-bit
    RGB (colour type 2), kind 1 16-bit grey (colour type 0). Signature, IHDR, IDAT, IEND; the CRCs by zlib.crc32."""
    if kind not in (0, 1):
        raise ValueError(f"png.assemble: kind must be 0 (8-bit RGB) or 1 (16-bit grey), got {kind!r}")
    if width < 1 or height < 1:
        raise ValueError(f"png.assemble: empty image ({width} x {height})")
    depth, colour = ((8, 2), (16, 0))[kind]
    header = struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", header) + _chunk(b"IDAT", bytes(stream_bytes)) + _chunk(b"IEND", b"")


def write(path, image, filter="up", level=1):
    with open(path, "wb") as f:
        f.write(encode(image, filter, level))
