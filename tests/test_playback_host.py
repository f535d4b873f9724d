"""CPU tests of the playback's host parts: the jet table against matplotlib, the numpy statement of the export kernel's rules
(tests/export_reference.py) against numpy's and matplotlib's own arithmetic, the PNG writer against PIL, and the camera paths."""
import io
import types

import numpy as np
import pytest
import torch

import export_reference as ref


def test_jet_lut_equals_matplotlib_for_all_256_rows():
    import matplotlib
    from slam import frame_io
    lut = frame_io.jet_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    want = np.array([matplotlib.colormaps["jet"](i, bytes=True)[:3] for i in range(256)], np.uint8)
    assert np.array_equal(lut, want)


def test_colour_rule_is_numpy_truncation_after_the_clamp():
    x = ref.adversarial_colour_values()
    got = ref.colour_bytes(x)
    finite = ~np.isnan(x)
    assert np.array_equal(got[finite], (np.clip(x[finite], 0, 1) * 255).astype(np.uint8))        # the reference's (image * 255).astype(uint8)
    assert np.all(got[np.isnan(x)] == 0)
    k = np.arange(256)
    exact = (k / 255.0).astype(np.float32)
    assert np.array_equal(ref.colour_bytes(np.nextafter(exact, np.float32(2))), (np.nextafter(exact, np.float32(2)) * np.float32(255)).astype(np.uint8))
    assert ref.colour_bytes(np.float32(1.0)) == 255 and ref.colour_bytes(np.float32(np.inf)) == 255 and ref.colour_bytes(np.float32(-np.inf)) == 0
    assert ref.colour_bytes(np.float32(0.999999)) == 254                                        # truncation, not rounding


@pytest.mark.parametrize("vmax", [6.0, 4.5])
def test_depth_colour_rule_is_matplotlibs_imshow(vmax):
    """vmax = 6 is the reference's. matplotlib divides in double by the double vmax and rounds to float32; the rule divides in float32 by
    float32(vmax). For a vmax that float32 holds exactly the two agree on every input (double rounding of a quotient of two float32 numbers
    is innocuous: 53 >= 2 * 24 + 2 bits); for one it does not hold, such as 3.7, the divisors differ and so can the last bit of n."""
    import matplotlib
    from matplotlib.colors import Normalize
    from slam import frame_io
    d = ref.adversarial_depth_values(vmax, 5000.0)
    got = ref.depth_colour(d, vmax, frame_io.jet_lut())
    with np.errstate(invalid="ignore", over="ignore"):
        want = matplotlib.colormaps["jet"](Normalize(0, vmax)(d), bytes=True)[:, :3]
    assert np.array_equal(got, want)
    i = ref.depth_index(d, vmax)
    assert np.all(i[np.isnan(d)] == -1) and np.all(got[np.isnan(d)] == 0)
    assert np.all(i[d < 0] == 0) and np.all(i[d == np.inf] == 255)
    b = (np.arange(1, 256) * (vmax / 256.0)).astype(np.float32)                                  # table boundaries: every row is reached
    assert set(ref.depth_index(np.concatenate([b, np.nextafter(b, np.float32(0))]), vmax)) == set(range(256))


def test_depth_u16_rule_rounds_half_to_even_and_saturates():
    s = 5000.0
    f = np.float32
    assert list(ref.depth_u16(np.array([0.5, 1.5, 2.5, 3.5], f) / f(1.0), 1.0)) == [0, 2, 2, 4]
    assert list(ref.depth_u16(np.array([65534.4, 65535.0, 65535.5, 65536.0, 1e9, np.inf], f), 1.0)) == [65534, 65535, 65535, 65535, 65535, 65535]
    assert list(ref.depth_u16(np.array([-0.4, -1.0, -np.inf, np.nan, -0.0], f), 1.0)) == [0, 0, 0, 0, 0]
    d = ref.adversarial_depth_values(6.0, s)
    ok = np.isfinite(d)
    want = np.clip(np.rint(d[ok] * f(s)), 0, 65535).astype(np.uint16)
    assert np.array_equal(ref.depth_u16(d, s)[ok], want)
    ties = (np.array([0, 1, 2, 3, 100, 101], np.float64) + 0.5)
    assert list(ref.depth_u16(ties.astype(f), 1.0)) == [0, 2, 2, 4, 100, 102]


def test_export_statement_lays_out_hwc():
    colour, depth = ref.adversarial_planes(2, 7, 9, 6.0, 5000.0)
    from slam import frame_io
    rgb, dvis, d16 = ref.export(colour, depth, frame_io.jet_lut(), 6.0, 5000.0)
    assert rgb.shape == (2, 7, 9, 3) and dvis.shape == (2, 7, 9, 3) and d16.shape == (2, 7, 9) and d16.dtype == np.uint16
    assert rgb[1, 3, 4, 2] == ref.colour_bytes(colour[1, 2, 3, 4])


@pytest.mark.parametrize("size", [(640, 480), (131, 77)])
@pytest.mark.parametrize("filt", ["none", "up"])
def test_png_writer_round_trips_through_pil(size, filt, tmp_path):
    from PIL import Image, ImageFile
    from slam import png
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    W, H = size
    rng = np.random.default_rng(W)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rgb[: H // 2] = (np.arange(W)[None, :, None] + np.arange(H // 2)[:, None, None]).astype(np.uint8)      # smooth half: Up has work to do
    g16 = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    g16[0, :4] = [0, 1, 255, 65535]
    for name, a in (("rgb.png", rgb), ("g16.png", g16)):
        path = str(tmp_path / name)
        png.write(path, a, filter=filt)
        with Image.open(path) as im:
            im.load()                                            # PIL checks every chunk's CRC and the zlib stream here
            assert im.size == (W, H) and im.mode == ("RGB" if a.ndim == 3 else "I;16")
            back = np.array(im)
        assert np.array_equal(back.astype(a.dtype), a)
        with Image.open(io.BytesIO(png.encode(a, filt, level=6))) as im:
            assert np.array_equal(np.array(im).astype(a.dtype), a)
    raw = png.encode(rgb, filt)
    assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw.count(b"IDAT") >= 1 and raw[-8:-4] == b"IEND"
    bad = bytearray(raw)
    bad[-20] ^= 0xFF                                             # a flipped byte in the IDAT payload: its CRC no longer holds
    with pytest.raises(Exception):
        with Image.open(io.BytesIO(bytes(bad))) as im:
            im.load()
    with pytest.raises(ValueError, match="uint8 \\[H, W, 3\\] or uint16"):
        png.encode(np.zeros((4, 4), np.float32))


# ---- camera paths ------------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def _map(n=6, seed=0):
    """A live-SLAM double the way tests/test_slam_host.py builds its cameras: SimpleNamespace poses in a frontend.cameras dict."""
    rng = np.random.default_rng(seed)
    cams = {}
    for k in range(n):
        R = _rot(rng.normal(size=3), 25.0 * k + 3)
        cams[k] = types.SimpleNamespace(uid=k, R=torch.tensor(R, dtype=torch.float32), T=torch.tensor(rng.normal(size=3), dtype=torch.float32),
                                        time=k / (n - 1))
    return types.SimpleNamespace(gaussians=None, frontend=types.SimpleNamespace(cameras=cams, kf_indices=[0]), background=None, pipeline_params=None)


def test_tracked_and_frozen_paths_have_the_promised_lengths_and_constants():
    from slam import playback
    m = _map()
    poses, times = playback.tracked(m)
    assert poses.shape == (6, 4, 4) and poses.dtype == torch.float32 and times == [k / 5 for k in range(6)]
    for k in range(6):
        assert torch.equal(poses[k, :3, :3], m.frontend.cameras[k].R) and torch.equal(poses[k, :3, 3], m.frontend.cameras[k].T)
        assert torch.equal(poses[k, 3], torch.tensor([0.0, 0.0, 0.0, 1.0]))
    p2, t2 = playback.frozen_time(m, 0.25)
    assert torch.equal(p2, poses) and t2 == [0.25] * 6
    p3, t3 = playback.frozen_camera(m, 2, 9)
    assert p3.shape == (9, 4, 4) and all(torch.equal(p, poses[2]) for p in p3)
    assert len(t3) == 9 and t3[0] == 0.0 and t3[-1] == 1.0 and np.allclose(np.diff(t3), 1 / 8)
    for spec, n in (("tracked", 6), ("frozen-time:0.5", 6), ("frozen-camera:1:4", 4), ("resample:17", 17)):
        assert len(playback.parse_path(m, spec)[1]) == n
    for spec in ("orbit", "frozen-time", "frozen-camera:1", "resample:x"):
        with pytest.raises(ValueError, match="camera path"):
            playback.parse_path(m, spec)


@pytest.mark.parametrize("n", [6, 11, 16, 23])
def test_resampled_returns_every_knot_exactly_and_orthonormal_rotations(n):
    from slam import playback
    m = _map()
    knots, knot_times = playback.tracked(m)
    poses, times = playback.resampled(m, n)
    assert poses.shape == (n, 4, 4) and len(times) == n
    assert torch.equal(poses[0], knots[0]) and torch.equal(poses[-1], knots[-1]) and times[0] == knot_times[0] and times[-1] == knot_times[-1]
    at = 0
    for k in range(6):                                           # every knot, in order, bit for bit, with its own time
        while not torch.equal(poses[at], knots[k]):
            at += 1
            assert at < n, f"knot {k} is not among the samples"
        assert times[at] == knot_times[k]
    R = poses[:, :3, :3].double()
    eye = torch.eye(3, dtype=torch.float64)
    assert float((R @ R.transpose(1, 2) - eye).abs().max()) < 1e-6 and float((torch.linalg.det(R) - 1).abs().max()) < 1e-6
    assert all(b >= a for a, b in zip(times, times[1:]))
    # the camera centre moves along the chord between its two knots
    centre = lambda P: -(P[:3, :3].double().T @ P[:3, 3].double())
    C = torch.stack([centre(p) for p in poses])
    K = torch.stack([centre(p) for p in knots])
    total = sum(float((K[k + 1] - K[k]).norm()) for k in range(5))
    assert abs(sum(float((C[i + 1] - C[i]).norm()) for i in range(n - 1)) - total) < 1e-5


def test_resampled_with_fewer_samples_than_knots_keeps_the_ends():
    from slam import playback
    m = _map()
    knots, knot_times = playback.tracked(m)
    poses, times = playback.resampled(m, 4)
    assert poses.shape == (4, 4, 4) and torch.equal(poses[0], knots[0]) and torch.equal(poses[-1], knots[-1])
    assert times[0] == 0.0 and times[-1] == 1.0


def test_slerp_takes_the_shorter_arc():
    from slam import playback
    # two rotations about z, 10 and 350 degrees: the short way passes through 0, not through 180
    P = torch.eye(4).repeat(2, 1, 1)
    P[0, :3, :3] = torch.tensor(_rot((0, 0, 1), 10.0), dtype=torch.float32)
    P[1, :3, :3] = torch.tensor(_rot((0, 0, 1), 350.0), dtype=torch.float32)
    mid = playback.interpolate_poses(P, [0.0, 1.0], 3)[0][1, :3, :3].double()
    assert float((mid - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
    # the same with the second quaternion's sign flipped by hand: q and -q are one rotation
    q0, q1 = playback._quaternion(_rot((0, 0, 1), 10.0)), playback._quaternion(_rot((0, 0, 1), 350.0))
    for a, b in ((q0, q1), (q0, -q1), (-q0, q1)):
        R = playback._rotation(playback.slerp(a, b, 0.5))
        assert np.abs(R - np.eye(3)).max() < 1e-12
    # an (almost) 180 degree step stays a rotation and moves by half the angle
    R = playback._rotation(playback.slerp(playback._quaternion(np.eye(3)), playback._quaternion(_rot((0, 1, 0), 179.0)), 0.5))
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.abs(R - _rot((0, 1, 0), 89.5)).max() < 1e-9
