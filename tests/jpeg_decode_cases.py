"""The JPEG files the decoder tests share (tests/test_jpeg_decode_host.py, tests/test_hip_jpeg_decode.py): the project's own encoder
statement (tests/jpeg_reference.py) and PIL's encoder in the variants that change what a decoder must do. Not a test itself."""
import functools
import io

import numpy as np
from PIL import Image

import jpeg_reference as enc

SIZES = [(1, 1), (8, 8), (16, 16), (16, 17), (17, 16), (37, 53), (131, 77)]               # (H, W)
QUALITIES = [30, 75, 95]
# name -> (PIL save options, PIL mode); "ours" is jpeg_reference.encode
VARIANTS = {
    "ours": None,
    "pil": ({}, "RGB"),
    "optimize": ({"optimize": True}, "RGB"),                                              # custom Huffman tables
    "restart_blocks": ({"restart_marker_blocks": 1}, "RGB"),                              # a restart interval of one MCU
    "restart_rows": ({"restart_marker_rows": 1}, "RGB"),                                  # ... of one MCU row
    "422": ({"subsampling": 1}, "RGB"),
    "444": ({"subsampling": 0}, "RGB"),
    "grey": ({}, "L"),
}


@functools.lru_cache(maxsize=None)
def picture(H, W, kind="adversarial", seed=0):
    return (enc.adversarial_picture if kind == "adversarial" else enc.smooth_picture)(H, W, seed=seed)


@functools.lru_cache(maxsize=None)
def jpeg_file(variant, H, W, quality, kind="adversarial", seed=0):
    """The bytes of one file."""
    pic = picture(H, W, kind, seed)
    if VARIANTS[variant] is None:
        return enc.encode(pic, quality)
    options, mode = VARIANTS[variant]
    out = io.BytesIO()
    Image.fromarray(pic).convert(mode).save(out, "JPEG", quality=quality, **options)
    return out.getvalue()


def pil_rgb(data):
    """uint8 [H, W, 3]: libjpeg's decode of the file, as PIL hands it out."""
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))


def strip_dht(data):
    """The file without its DHT segments (what many Motion-JPEG producers write)."""
    out, at = bytearray(data[:2]), 2
    while data[at + 1] != 0xDA:
        length = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] != 0xC4:
            out += data[at:at + 2 + length]
        at += 2 + length
    return bytes(out) + data[at:]


def with_luminance_sampling(data, h, v):
    """The file with the luminance sampling factors in its SOF0 replaced (the scan no longer fits it: for header tests only)."""
    at = data.index(b"\xff\xc0")
    return data[:at + 11] + bytes([h << 4 | v]) + data[at + 12:]
