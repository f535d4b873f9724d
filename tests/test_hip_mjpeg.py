"""The device's JPEG encoder (include/video_io.h gsr_jpeg_encode, csrc/gs_jpeg.h) against the fp64 numpy statement of its arithmetic
(tests/jpeg_reference.py), and the Motion-JPEG playback built on it (Playback.write_video, tools/play_map.py --video).

Coefficients: float32 evaluation of the colour sums and the two 8-term DCT passes carries an absolute error below about 2e-3 on values up to
1024, so a device coefficient may differ from rint(fp64 quotient), by exactly 1, only where that quotient lies within 0.004 of a half-integer;
fewer than 2 % of the coefficients may lie in that band at all. Everything behind the coefficients is integer work and is held byte for byte:
the statement's entropy coder runs on the device's own coefficients."""
import functools
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_reference as ref
from util import REPO

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (1, 1), (131, 77), (320, 240)]
VIEWS = [1, 12]
QUALITIES = [50, 90, 100]
HALF_BAND = 0.004
BAND_SHARE = 0.02
PSNR_MARGIN_DB = 0.25
SENTINEL = 0xA5


def _pictures(W, H, V):
    """The adversarial picture, and for a batch adversarial and smooth pictures in turn, all different."""
    return [ref.adversarial_picture(H, W, seed=v) if v % 2 == 0 else ref.smooth_picture(H, W, seed=v) for v in range(V)]


def _encode(pics, quality, want_coefficients=True, stride=None, tail=0):
    """(sizes [V], scan uint8 [V, stride], coefficients or None, the `tail` bytes behind the last view's capacity) from one call."""
    from slam import mjpeg
    dev = torch.device("cuda:0")
    V, (H, W, _) = len(pics), pics[0].shape
    stride = stride or max(W * H * 3, 65536)
    rgb = torch.from_numpy(np.stack(pics)).to(dev)
    q = torch.from_numpy(mjpeg.quant_tables(quality).astype(np.int16)).to(dev)
    flat = torch.full((V * stride + tail,), SENTINEL, dtype=torch.uint8, device=dev)
    scan = flat[:V * stride].view(V, stride)
    sizes = torch.full((V,), -7, dtype=torch.int32, device=dev)
    rows, cols = mjpeg.mcu_grid(W, H)
    coef = torch.full((V, rows, cols, 6, 64), 12345, dtype=torch.int16, device=dev) if want_coefficients else None
    mjpeg.jpeg_encode(rgb, q, scan, sizes, coef)
    torch.cuda.synchronize()
    return sizes.cpu().numpy(), scan.cpu().numpy(), None if coef is None else coef.cpu().numpy(), flat[V * stride:].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(W, H, V, quality):
    pics = _pictures(W, H, V)
    sizes, scan, coef, _ = _encode(pics, quality)
    return pics, sizes, scan, coef


CASES = [(W, H, V, Q) for (W, H) in SIZES for V in VIEWS for Q in QUALITIES]


@pytest.mark.parametrize("W,H,V,quality", CASES)
def test_coefficients_against_the_fp64_statement(W, H, V, quality):
    from slam import mjpeg
    pics, _, _, coef = _case(W, H, V, quality)
    q = mjpeg.quant_tables(quality)
    for v, pic in enumerate(pics):
        quot = ref.quotients(pic, q)
        want = np.rint(quot)
        off_half = np.abs(np.abs(quot - np.floor(quot)) - 0.5)
        in_band = off_half < HALF_BAND
        diff = coef[v].astype(np.int64) - want.astype(np.int64)
        print(f"{W}x{H} V{V} Q{quality} view {v}: {int((diff != 0).sum())} of {diff.size} differ, {100 * in_band.mean():.3f} % in the band, "
              f"largest |coefficient| {int(np.abs(coef[v]).max())}")
        assert coef[v].shape == want.shape
        assert in_band.mean() < BAND_SHARE
        assert np.abs(diff).max() <= 1
        assert not (diff != 0)[~in_band].any(), float(off_half[diff != 0].max())


@pytest.mark.parametrize("W,H,V,quality", CASES)
def test_scan_bytes_equal_the_statements_entropy_coder_on_the_device_coefficients(W, H, V, quality):
    pics, sizes, scan, coef = _case(W, H, V, quality)
    seen = {"dc_category_max": 0, "zrl": 0, "stuffed": 0}
    for v in range(V):
        e = {}
        want = ref.entropy_code(coef[v], e)
        seen = {k: max(seen[k], e[k]) for k in seen}
        assert sizes[v] == len(want), (v, int(sizes[v]), len(want))
        got = scan[v, :sizes[v]].tobytes()
        assert got == want, (v, next(i for i in range(len(want)) if got[i] != want[i]))
        assert (scan[v, sizes[v]:] == SENTINEL).all()
    if (W, H) in ((131, 77), (320, 240)):                            # the inputs stay adversarial: category 11, ZRL, stuffing
        assert seen["stuffed"] >= 1
        if quality == 100:
            assert seen["dc_category_max"] == 11
        if quality == 90:
            assert seen["zrl"] >= 1


def test_the_adversarial_inputs_reach_zrl_on_the_device():
    zrl = 0
    for quality in (50, 90):
        e = {}
        ref.entropy_code(_case(131, 77, 1, quality)[3][0], e)
        zrl += e["zrl"]
    assert zrl >= 1


@pytest.mark.parametrize("W,H,quality", [(W, H, Q) for (W, H) in SIZES for Q in QUALITIES])
def test_batches_equal_single_calls_and_calls_repeat(W, H, quality):
    pics, sizes, scan, coef = _case(W, H, 12, quality)
    again = _encode(pics, quality)
    assert np.array_equal(again[0], sizes) and np.array_equal(again[1], scan) and np.array_equal(again[2], coef)
    plain = _encode(pics, quality, want_coefficients=False)
    assert plain[2] is None and np.array_equal(plain[0], sizes) and np.array_equal(plain[1], scan)
    for v in range(12):
        one = _encode(pics[v:v + 1], quality)
        assert one[0][0] == sizes[v] and np.array_equal(one[1][0], scan[v]) and np.array_equal(one[2][0], coef[v]), v


@pytest.mark.parametrize("quality", QUALITIES)
def test_a_view_that_does_not_fit_reports_its_size_and_writes_nothing_beyond_its_capacity(quality):
    W, H = 131, 77
    noise = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    pics = [ref.smooth_picture(H, W, seed=1), noise, np.full((H, W, 3), 90, np.uint8), ref.adversarial_picture(H, W, seed=4)]      # four very different sizes
    sizes, scan, coef, _ = _encode(pics, quality)
    need = [len(ref.entropy_code(coef[v])) for v in range(4)]
    assert sizes.tolist() == need
    order = sorted(need)
    stride = (order[1] + order[2]) // 2                              # two views fit, two do not
    assert order[1] <= stride < order[2]
    small = _encode(pics, quality, stride=stride, tail=4096)
    assert small[0].tolist() == [n if n <= stride else -n for n in need]
    for v in range(4):
        if need[v] <= stride:
            assert np.array_equal(small[1][v, :need[v]], scan[v, :need[v]]) and (small[1][v, need[v]:] == SENTINEL).all()
    assert (small[3] == SENTINEL).all()
    assert np.array_equal(small[2], coef)


@pytest.mark.parametrize("W,H,V,quality", CASES)
def test_files_decode_in_pil_as_well_as_pils_own(W, H, V, quality):
    from slam import mjpeg
    pics, sizes, scan, _ = _case(W, H, V, quality)
    header = mjpeg.jfif_header(W, H, mjpeg.quant_tables(quality))
    for v in range(0, V, 5):
        with Image.open(io.BytesIO(header + scan[v, :sizes[v]].tobytes() + mjpeg.EOI)) as im:
            mine = np.array(im.convert("RGB"))
        assert mine.shape == (H, W, 3)
        b = io.BytesIO()
        Image.fromarray(pics[v]).save(b, "JPEG", quality=quality, subsampling=2, optimize=False)
        theirs = np.array(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
        a, p = ref.psnr(mine, pics[v]), ref.psnr(theirs, pics[v])
        print(f"{W}x{H} Q{quality} view {v}: device {a:.3f} dB, PIL {p:.3f} dB")
        assert a >= p - PSNR_MARGIN_DB


def test_bad_arguments_name_the_argument_and_enqueue_nothing():
    from slam import mjpeg
    dev = "cuda:0"
    rgb = torch.zeros((2, 20, 24, 3), dtype=torch.uint8, device=dev)
    q = torch.from_numpy(mjpeg.quant_tables(90).astype(np.int16)).to(dev)
    scan = torch.full((2, 4096), SENTINEL, dtype=torch.uint8, device=dev)
    sizes = torch.full((2,), -7, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="quality"):
        mjpeg.quant_tables(0)
    with pytest.raises(RuntimeError, match="rgb8 must be"):
        mjpeg.jpeg_encode(rgb.float(), q, scan, sizes)
    with pytest.raises(RuntimeError, match="rgb8 must be"):
        mjpeg.jpeg_encode(rgb[..., :2], q, scan, sizes)
    with pytest.raises(RuntimeError, match="qtables must be"):
        mjpeg.jpeg_encode(rgb, q.float(), scan, sizes)
    with pytest.raises(RuntimeError, match="sizes must be"):
        mjpeg.jpeg_encode(rgb, q, scan, sizes[:1])
    with pytest.raises(RuntimeError, match="scan is on 'cpu'"):
        mjpeg.jpeg_encode(rgb, q, scan.cpu(), sizes)
    with pytest.raises(RuntimeError, match="scan must be"):
        mjpeg.jpeg_encode(rgb, q, scan[:, ::2], sizes)
    with pytest.raises(RuntimeError, match="coefficients must be"):
        mjpeg.jpeg_encode(rgb, q, scan, sizes, torch.zeros((2, 2, 2, 6, 63), dtype=torch.int16, device=dev))
    need = mjpeg.jpeg_workspace_size(2, 24, 20)
    assert need > 0 and mjpeg.jpeg_workspace_size(0, 24, 20) == 0
    with pytest.raises(RuntimeError, match="workspace must be"):
        mjpeg.jpeg_encode(rgb, q, scan, sizes, workspace=torch.empty(need - 1, dtype=torch.uint8, device=dev))
    # the C entry point refuses what the wrapper cannot see: a workspace off its alignment
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="gsr_jpeg_encode.*16-byte aligned"):
        mjpeg.jpeg_encode(rgb, q, scan, sizes, workspace=ws[1:])
    torch.cuda.synchronize()
    assert (scan == SENTINEL).all() and (sizes == -7).all()
    mjpeg.jpeg_encode(rgb, q, scan, sizes, workspace=ws[:need])
    torch.cuda.synchronize()
    assert (sizes > 0).all()


# ---- playback ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static_map(tmp_path_factory):
    """A static 14-frame synthetic SLAM run at the sizes and schedule of tests/test_hip_playback.py, saved."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "dynamic_map_iters": 60, "network_init_iters": 40, "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 4}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 100}, "model_params": {"dynamic_model": False}})
    torch.manual_seed(0)
    slam = SLAM(cfg, SyntheticRGBDDataset(num_frames=14, width=320, height=240, seed=0, dynamic=False, dystart=None))
    slam.run()
    return slam.save_map(str(tmp_path_factory.mktemp("static") / "map"))


def _decode(data):
    with Image.open(io.BytesIO(data)) as im:
        assert im.format == "JPEG"
        return np.array(im.convert("RGB"))


def test_write_video_writes_motion_jpeg_files_of_the_rendered_frames(static_map, tmp_path):
    from slam import frame_io, mjpeg
    from slam.map_io import load_map
    from slam.playback import Playback, resampled
    loaded = load_map(static_map, "cuda:0")
    poses, times = resampled(loaded, 12)
    pb = Playback(loaded)
    out = str(tmp_path / "video")
    res = pb.write_video(poses, times, out, fps=25.0, quality=90)
    assert sorted(os.listdir(out)) == ["depth_vis.avi", "rgb.avi"] and res["files"] == [os.path.join(out, "rgb.avi"), os.path.join(out, "depth_vis.avi")]
    assert res["frames"] == 12 and res["fps"] > 0 and res["writer_wait_s"] >= 0 and res["encode_ms"] > 0 and res["export_ms"] > 0
    colour, depth, _ = pb.render(poses, times)
    lut = torch.from_numpy(frame_io.jet_lut().copy()).cuda()
    rgb = torch.empty((12, 240, 320, 3), dtype=torch.uint8, device="cuda")
    vis = torch.empty_like(rgb)
    frame_io.frame_export(colour, depth, lut, 6.0, 5000.0, rgb, vis)
    want = {"rgb": rgb.cpu().numpy(), "depth_vis": vis.cpu().numpy()}
    total = 0
    for kind in ("rgb", "depth_vis"):
        info, frames = mjpeg.read_avi(os.path.join(out, kind + ".avi"))
        assert len(frames) == 12 and info["frames"] == 12 and (info["width"], info["height"]) == (320, 240) and info["fps"] == 25.0
        total += sum(len(f) for f in frames)
        for i, f in enumerate(frames):
            got = _decode(f)
            assert got.shape == (240, 320, 3)
            b = io.BytesIO()
            Image.fromarray(want[kind][i]).save(b, "JPEG", quality=90, subsampling=2, optimize=False)
            a, p = ref.psnr(got, want[kind][i]), ref.psnr(_decode(b.getvalue()), want[kind][i])
            assert a >= p - PSNR_MARGIN_DB, (kind, i, a, p)
    assert res["bytes"] == total
    assert float(want["rgb"].std()) > 10                                            # (pictures, not blanks)
    # without the depth pictures only rgb.avi is written; files=False writes nothing
    out2 = str(tmp_path / "plain")
    res2 = pb.write_video(poses[:3], times[:3], out2, depth_colour=False)
    assert os.listdir(out2) == ["rgb.avi"] and len(mjpeg.read_avi(os.path.join(out2, "rgb.avi"))[1]) == 3 and res2["files"] == [os.path.join(out2, "rgb.avi")]
    out3 = str(tmp_path / "none")
    res3 = pb.write_video(poses[:3], times[:3], out3, files=False)
    assert not os.path.exists(out3) and res3["files"] == [] and res3["bytes"] > 0
    # a frame that does not fit its capacity: the files are closed validly, then the error names the frame and its size
    out4 = str(tmp_path / "tight")
    with pytest.raises(RuntimeError, match=r"frame 0 \(rgb\) needs \d+ bytes"):
        pb.write_video(poses[:3], times[:3], out4, capacity=1000)
    assert mjpeg.read_avi(os.path.join(out4, "rgb.avi"))[0]["frames"] == 0
    with pytest.raises(ValueError, match="quality"):
        pb.write_video(poses[:3], times[:3], out4, quality=0)


def test_write_video_over_two_chunks_equals_direct_encodes_of_the_same_renders(static_map, tmp_path):
    """14 tracked poses: a full chunk of 12 and a partial one of 2, through the ring of slots; every frame of both files is, byte for byte,
    header + gsr_jpeg_encode(gsr_frame_export(render)) + EOI."""
    from slam import frame_io, mjpeg
    from slam.map_io import load_map
    from slam.playback import Playback, tracked
    loaded = load_map(static_map, "cuda:0")
    poses, times = tracked(loaded)
    assert len(times) == 14
    pb = Playback(loaded)
    out = str(tmp_path / "two_chunks")
    res = pb.write_video(poses, times, out, quality=75)
    colour, depth, _ = pb.render(poses, times)
    lut = torch.from_numpy(frame_io.jet_lut().copy()).cuda()
    rgb = torch.empty((14, 240, 320, 3), dtype=torch.uint8, device="cuda")
    vis = torch.empty_like(rgb)
    frame_io.frame_export(colour, depth, lut, 6.0, 5000.0, rgb, vis)
    qt = mjpeg.quant_tables(75)
    header = mjpeg.jfif_header(320, 240, qt)
    q = torch.from_numpy(qt.astype(np.int16)).cuda()
    total = 0
    for kind, pictures in (("rgb", rgb), ("depth_vis", vis)):
        scan = torch.empty((14, 320 * 240 * 3), dtype=torch.uint8, device="cuda")
        sizes = torch.empty((14,), dtype=torch.int32, device="cuda")
        mjpeg.jpeg_encode(pictures, q, scan, sizes)
        scan, sizes = scan.cpu().numpy(), sizes.cpu().numpy()
        info, frames = mjpeg.read_avi(os.path.join(out, kind + ".avi"))
        assert info["frames"] == 14 and info["fps"] == 30.0
        for i, f in enumerate(frames):
            assert f == header + scan[i, :sizes[i]].tobytes() + mjpeg.EOI, (kind, i)
        total += sum(len(f) for f in frames)
    assert res["bytes"] == total and res["frames"] == 14


def test_play_map_tool_writes_video_from_a_fresh_process(static_map, tmp_path):
    from slam import mjpeg
    out = str(tmp_path / "played")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "play_map.py"), "--map", static_map, "--path", "resample:5", "--out", out,
                        "--video", "--fps", "24", "--quality", "75"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["video"] is True and line["frames"] == 5 and line["bytes"] > 0 and line["encode_ms"] > 0 and line["fps"] > 0
    assert sorted(os.listdir(out)) == ["depth_vis.avi", "rgb.avi"]
    info, frames = mjpeg.read_avi(os.path.join(out, "rgb.avi"))
    assert info["fps"] == 24.0 and len(frames) == 5 and all(_decode(f).shape == (240, 320, 3) for f in frames)
