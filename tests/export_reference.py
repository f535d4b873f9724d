"""The rules of gsr_frame_export (include/frame_io.h) stated in numpy, and the adversarial planes the host and the device tests share.
Imported by tests/test_playback_host.py (against numpy's and matplotlib's own arithmetic) and tests/test_hip_playback.py (the kernel)."""
import numpy as np

F = np.float32


def colour_bytes(x):
    """(uint8)(min(max(x, 0), 1) * 255.0f), truncation, NaN -> 0. x float32 [...]."""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        c = np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)       # a NaN fails `x > 0`
    return (c * F(255.0)).astype(np.int32).astype(np.uint8)


def depth_index(d, vmax):
    """Row of the 256-entry table, -1 for NaN: n = d / vmax, (int)(n * 256) clamped to [0, 255], n < 0 -> 0."""
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = (d / F(vmax)) * F(256.0)
        i = np.where(s < 0, 0, np.where(s >= 255, 255, np.nan_to_num(s, nan=0.0, posinf=255.0, neginf=0.0))).astype(np.int32)
    return np.where(np.isnan(s), -1, i)


def depth_colour(d, vmax, lut):
    i = depth_index(d, vmax)
    out = np.asarray(lut, np.uint8)[np.maximum(i, 0)]
    out[i < 0] = 0
    return out


def depth_u16(d, scale):
    """rint(d * scale) (half to even), saturated to [0, 65535]; NaN and negatives -> 0."""
    d = np.asarray(d, F)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(d * F(scale))
        r = np.where(r > 0, np.where(r < 65535, r, F(65535)), F(0))
    return r.astype(np.int64).astype(np.uint16)


def export(colour, depth, lut, vmax, scale):
    """colour [V,3,H,W], depth [V,1,H,W] -> (rgb8 [V,H,W,3], depth_rgb8 [V,H,W,3], depth_u16 [V,H,W])."""
    rgb = np.ascontiguousarray(colour_bytes(colour).transpose(0, 2, 3, 1))
    return rgb, depth_colour(depth[:, 0], vmax, lut), depth_u16(depth[:, 0], scale)


def _neighbours(v):
    v = np.asarray(v, F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))])


SPECIAL = np.array([-1.0, -0.0, 0.0, -1e-30, 1e-30, 1.0, 1.5, 2.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.999999, 254.5 / 255], F)


def adversarial_colour_values():
    """k / 255 and its two float neighbours for every byte k (in float32 and as the float32 nearest the double quotient), plus the specials."""
    k = np.arange(256)
    return np.concatenate([_neighbours(k.astype(F) / F(255.0)), _neighbours((k / 255.0).astype(F)), SPECIAL])


def adversarial_depth_values(vmax, scale):
    """Depths at i * vmax / 256 and their neighbours (table boundaries), (j + 0.5) / scale and neighbours (ties of the 16-bit rounding),
    the 16-bit saturation point and beyond, negatives, infinities and NaN."""
    i = np.arange(258)
    ties = (np.array([0, 1, 2, 3, 4, 5, 100, 101, 1234, 30000, 65533, 65534, 65535, 65536], np.float64) + 0.5) / scale
    edge = np.array([65534, 65535, 65536, 70000, 1e9], np.float64) / scale
    return np.concatenate([_neighbours((i * (vmax / 256.0)).astype(F)), _neighbours(ties.astype(F)), _neighbours(edge.astype(F)),
                           SPECIAL, F(vmax) * SPECIAL[np.isfinite(SPECIAL)]])


def adversarial_planes(V, H, W, vmax, scale, seed=0):
    """colour [V,3,H,W] and depth [V,1,H,W]: the adversarial values first (tiled over the views with a different offset each, so that every
    one meets the vector path and the scalar tail somewhere), random data after."""
    rng = np.random.default_rng(seed)
    cv, dv = adversarial_colour_values(), adversarial_depth_values(vmax, scale)
    colour = rng.uniform(-0.2, 1.2, (V, 3, H, W)).astype(F)
    depth = rng.uniform(-0.5, vmax * 2.5, (V, 1, H, W)).astype(F)
    for v in range(V):
        for c in range(3):
            flat = colour[v, c].reshape(-1)
            n = min(flat.size, cv.size)
            flat[:n] = np.roll(cv, v * 3 + c)[:n]
        flat = depth[v, 0].reshape(-1)
        n = min(flat.size, dv.size)
        flat[:n] = np.roll(dv, v)[:n]
    return colour, depth
