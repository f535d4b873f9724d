"""The playback on the device: gsr_frame_export (include/frame_io.h, csrc/gs_frame.h) byte for byte against the numpy statement of its rules
(tests/export_reference.py); a saved and reloaded map rendering bit-identically to the live one; the playback against the evaluation's
route; the written files read back by PIL and by TUMDataset; tools/play_map.py in a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import export_reference as ref
from util import REPO

pytestmark = pytest.mark.gpu

VMAX, SCALE = 6.0, 5000.0

# Playback evaluates the node network once per chunk (ControlNodes.begin_iteration: the dense-layer kernels on all times at once) where the
# evaluation's route evaluates it one time at a time (the library's GEMMs): the same network in a different fp32 summation order, so the
# two are not bit-identical. The figures are the largest absolute differences of the EVALUATION route against itself across these two
# evaluation orders -- per-frame render() with BackEnd._deltas(frame, train=False), outside and inside a begin_iteration batch -- on the
# 30-frame dynamic run below (measured 3.227e-3, 4.821e-3 and 1.144e-4; the test prints them again); Playback must stay within 10 x of each.
# It is in fact bit-identical to the batched order, which the test asserts as well.
EVAL_ORDER_FIGURE = {"colour": 3.23e-3, "depth": 4.83e-3, "opacity": 1.15e-4}


def _export(colour, depth, want_vis=True, want_u16=True):
    from slam import frame_io
    dev = torch.device("cuda:0")
    V, _, H, W = colour.shape
    lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
    rgb = torch.full((V, H, W, 3), 77, dtype=torch.uint8, device=dev)
    vis = torch.full((V, H, W, 3), 77, dtype=torch.uint8, device=dev) if want_vis else None
    u16 = torch.full((V, H, W), 77, dtype=torch.int16, device=dev) if want_u16 else None
    frame_io.frame_export(colour, depth, lut, VMAX, SCALE, rgb, vis, u16)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), None if vis is None else vis.cpu().numpy(), None if u16 is None else u16.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("size", [(640, 480), (131, 77)])
@pytest.mark.parametrize("V", [1, 12])
def test_frame_export_is_byte_exact_against_the_numpy_statement(size, V):
    from slam import frame_io
    W, H = size
    c_np, d_np = ref.adversarial_planes(V, H, W, VMAX, SCALE, seed=V)
    want = ref.export(c_np, d_np, frame_io.jet_lut(), VMAX, SCALE)
    colour, depth = torch.from_numpy(c_np).cuda(), torch.from_numpy(d_np).cuda()
    got = _export(colour, depth)
    for name, g, w in zip(("rgb8", "depth_rgb8", "depth_u16"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, int((g != w).sum()))
    # each optional output NULL in turn: the others are unchanged
    rgb, vis, u16 = _export(colour, depth, want_vis=False)
    assert vis is None and np.array_equal(rgb, want[0]) and np.array_equal(u16, want[2])
    rgb, vis, u16 = _export(colour, depth, want_u16=False)
    assert u16 is None and np.array_equal(rgb, want[0]) and np.array_equal(vis, want[1])
    rgb, vis, u16 = _export(colour, None, want_vis=False, want_u16=False)
    assert np.array_equal(rgb, want[0])
    # V views in one call equal V single calls
    if V > 1:
        for v in (0, 5, V - 1):
            one = _export(colour[v:v + 1], depth[v:v + 1])
            assert all(np.array_equal(o[0], g[v]) for o, g in zip(one, got))
    # views inside a larger block (the multi-view rasterizer's [V, 5, H, W] output): the per-view stride argument
    block = torch.full((V, 5, H, W), float("nan"), device="cuda")
    block[:, :3], block[:, 3:4] = colour, depth
    strided = _export(block[:, :3], block[:, 3:4])
    assert all(np.array_equal(a, b) for a, b in zip(strided, got))


def test_frame_export_rejects_bad_arguments():
    from slam import frame_io
    dev = "cuda:0"
    colour, depth = torch.zeros((2, 3, 8, 12), device=dev), torch.zeros((2, 1, 8, 12), device=dev)
    lut = torch.from_numpy(frame_io.jet_lut().copy()).to(dev)
    rgb = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="without depth"):
        frame_io.frame_export(colour, None, lut, VMAX, SCALE, rgb, torch.zeros_like(rgb))
    with pytest.raises(RuntimeError, match="rgb8 must be"):
        frame_io.frame_export(colour, depth, lut, VMAX, SCALE, rgb[:1])
    with pytest.raises(RuntimeError, match="contiguous views"):
        frame_io.frame_export(colour.transpose(2, 3).contiguous().transpose(2, 3), depth, lut, VMAX, SCALE, rgb)
    with pytest.raises(RuntimeError, match="depth_vmax must be positive"):
        frame_io.frame_export(colour, depth, lut, 0.0, SCALE, rgb, torch.zeros_like(rgb))
    with pytest.raises(RuntimeError, match="device"):
        frame_io.frame_export(colour.cpu(), depth, lut, VMAX, SCALE, rgb)


# ---- maps --------------------------------------------------------------------------------------------------------------------------
def _run(dynamic, frames):
    """A short synthetic SLAM run at the sizes and schedule of tests/test_hip_slam.py's 30-frame dynamic run (_quick_config)."""
    from slam.dataset import SyntheticRGBDDataset
    from slam.system import SLAM, default_config, merge_config
    t = {"init_itr_num": 250, "init_gaussian_update": 100, "init_gaussian_reset": 120, "tracking_itr_num": 40, "static_map_iters": 20,
         "dynamic_map_iters": 60, "network_init_iters": 40, "gaussian_update_every": 60, "gaussian_update_offset": 20, "kf_interval": 4}
    cfg = merge_config(default_config(), {"Training": t, "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 100}, "model_params": {"dynamic_model": dynamic}})
    torch.manual_seed(0)
    ds = SyntheticRGBDDataset(num_frames=frames, width=320, height=240, seed=1 if dynamic else 0, dynamic=dynamic, dystart=6 if dynamic else None)
    slam = SLAM(cfg, ds)
    slam.run()
    return slam


@pytest.fixture(scope="module")
def dynamic_run(tmp_path_factory):
    slam = _run(True, 30)
    assert slam.gaussians.deform_init and int(slam.gaussians.dygs.sum()) > 50
    return slam, slam.save_map(str(tmp_path_factory.mktemp("dynamic") / "map"))


@pytest.fixture(scope="module")
def static_run(tmp_path_factory):
    slam = _run(False, 14)
    return slam, slam.save_map(str(tmp_path_factory.mktemp("static") / "map"))


def _saved_equals_live(slam, directory):
    from slam.map_io import load_map
    from slam.playback import Playback, tracked
    loaded = load_map(directory, "cuda:0")
    assert loaded.gaussians is not slam.gaussians and (loaded.gaussians.deform is None) == (slam.gaussians.deform is None)
    lp, lt = tracked(loaded)
    sp, st = tracked(slam)
    assert torch.equal(lp, sp) and lt == st and len(lt) == len(slam.frontend.cameras)
    live = Playback(slam).render(sp, st)
    back = Playback(loaded).render(lp, lt)
    for name, a, b in zip(("colour", "depth", "opacity"), live, back):
        assert a.shape == b.shape and torch.equal(a, b), name
    assert float(live[0].std()) > 0.05 and float(live[2].mean()) > 0.5          # (pictures, not blanks)
    return loaded, live


def test_saved_dynamic_map_renders_bit_identically_to_the_live_one(dynamic_run):
    slam, directory = dynamic_run
    loaded, _ = _saved_equals_live(slam, directory)
    assert loaded.dynamic and os.path.isfile(os.path.join(directory, "deform", "iteration_0", "deform.pth"))
    # deltas_for has the semantics of BackEnd._deltas(frame, train=False)
    for uid in (0, 7, 29):
        want = slam.backend._deltas(slam.frontend.cameras[uid], train=False)
        got = loaded.deltas_for(loaded.cameras[uid])
        assert all(torch.equal(a, b) for a, b in zip(want, got))
    # the loaded cameras' device matrices are the live ones
    for uid, c in slam.frontend.cameras.items():
        d = loaded.cameras[uid]
        assert torch.equal(c.world_view_transform, d.world_view_transform) and torch.equal(c.full_proj_transform, d.full_proj_transform)
        assert torch.equal(c.camera_center, d.camera_center)


def test_saved_static_map_renders_bit_identically_to_the_live_one(static_run):
    slam, directory = static_run
    loaded, _ = _saved_equals_live(slam, directory)
    assert not loaded.dynamic and not os.path.exists(os.path.join(directory, "deform"))
    assert loaded.deltas_for(loaded.cameras[0]) == (None, None, None)


def _evaluation_route(slam, batched):
    """The evaluation's route (eval_utils.eval_rendering): per-frame render() with BackEnd._deltas(frame, train=False). batched: the same
    calls inside ControlNodes.begin_iteration batches of 12 times, so that the node network is evaluated on all of a batch's times at once."""
    from gaussian_renderer import render
    g, be = slam.gaussians, slam.backend
    frames = [slam.frontend.cameras[k] for k in sorted(slam.frontend.cameras)]
    out = []
    with torch.no_grad():
        for lo in range(0, len(frames), 12):
            part = frames[lo:lo + 12]
            if batched:
                g.deform.deform.begin_iteration([f.time for f in part], blend=(g.get_dygs_xyz.detach(), g.motion_mask))
            try:
                for f in part:
                    dx, ds, dr = be._deltas(f, train=False)
                    pkg = render(f, g, slam.pipeline_params, slam.background, dynamic=False, dx=dx, ds=ds, dr=dr)
                    out.append((pkg["render"].clone(), pkg["depth"].clone(), pkg["opacity"].clone()))
            finally:
                if batched:
                    g.deform.deform.end_iteration()
    return [torch.stack(t) for t in zip(*out)]


def test_playback_against_the_evaluation_route(dynamic_run):
    """Figures measured on the MI355X (colour / depth / opacity, largest absolute difference over the 30 frames): see EVAL_ORDER_FIGURE."""
    from slam.playback import Playback, tracked
    slam, _ = dynamic_run
    one_at_a_time = _evaluation_route(slam, batched=False)
    in_batches = _evaluation_route(slam, batched=True)
    play = Playback(slam).render(*tracked(slam))
    names = ("colour", "depth", "opacity")
    order = {n: float((a - b).abs().max()) for n, a, b in zip(names, one_at_a_time, in_batches)}
    diff = {n: float((a - b).abs().max()) for n, a, b in zip(names, one_at_a_time, play)}
    print("evaluation route, one time at a time vs batched:", order)
    print("playback vs evaluation route:", diff)
    for n, a, b in zip(names, in_batches, play):
        assert torch.equal(a, b), n                    # same evaluation order: multi-view and single-view renders are bit-identical
    for n in names:
        assert diff[n] <= 10 * EVAL_ORDER_FIGURE[n], (n, diff[n], EVAL_ORDER_FIGURE[n])


def test_static_playback_equals_the_evaluation_route(static_run):
    from gaussian_renderer import render
    from slam.playback import Playback, tracked
    slam, _ = static_run
    play = Playback(slam).render(*tracked(slam))
    with torch.no_grad():
        for i, k in enumerate(sorted(slam.frontend.cameras)):
            pkg = render(slam.frontend.cameras[k], slam.gaussians, slam.pipeline_params, slam.background, dx=0, ds=0, dr=0)
            assert torch.equal(pkg["render"], play[0][i]) and torch.equal(pkg["depth"], play[1][i]) and torch.equal(pkg["opacity"], play[2][i]), k


# ---- files -------------------------------------------------------------------------------------------------------------------------
def test_written_files_equal_the_device_bytes_and_read_back_as_a_tum_sequence(dynamic_run, tmp_path):
    from PIL import Image
    from slam import frame_io, recorded
    from slam.map_io import load_map
    from slam.playback import Playback, resampled
    from slam.system import default_config, merge_config
    _, directory = dynamic_run
    loaded = load_map(directory, "cuda:0")
    poses, times = resampled(loaded, 12)
    pb = Playback(loaded)
    out = str(tmp_path / "seq")
    res = pb.write(poses, times, out, depth16=True)
    assert res["frames"] == 12 and res["fps"] > 0 and res["writer_wait_s"] >= 0
    colour, depth, _ = pb.render(poses, times)
    lut = torch.from_numpy(frame_io.jet_lut().copy()).cuda()
    rgb = torch.empty((12, 240, 320, 3), dtype=torch.uint8, device="cuda")
    vis, u16 = torch.empty_like(rgb), torch.empty((12, 240, 320), dtype=torch.int16, device="cuda")
    frame_io.frame_export(colour, depth, lut, 6.0, 5000.0, rgb, vis, u16)
    rgb, vis, u16 = rgb.cpu().numpy(), vis.cpu().numpy(), u16.cpu().numpy().view(np.uint16)
    assert np.array_equal(rgb, ref.export(colour.cpu().numpy(), depth.cpu().numpy(), frame_io.jet_lut(), 6.0, 5000.0)[0])
    stamps = [recorded.tum_stamp(i) for i in range(12)]
    assert sorted(os.listdir(os.path.join(out, "rgb"))) == [s + ".png" for s in stamps]
    for i, s in enumerate(stamps):
        for kind, want in (("rgb", rgb[i]), ("depth_vis", vis[i]), ("depth", u16[i])):
            with Image.open(os.path.join(out, kind, s + ".png")) as im:
                assert np.array_equal(np.array(im).astype(want.dtype), want), (kind, i)
    assert int(u16.max()) > 1000 and len(np.unique(vis.reshape(-1, 3), axis=0)) > 20
    # the folder is a TUM sequence
    cfg = merge_config(default_config(), {"Dataset": {"type": "tum", "dataset_path": out, "Calibration": res["calibration"]}})
    ds = recorded.TUMDataset(cfg, "cuda:0")
    try:
        assert len(ds) == 12
        table = torch.from_numpy(recorded.byte_lut()).cuda()
        for i in (0, 5, 11):
            image, d, pose, _ = ds[i]
            assert torch.equal(image, table[torch.from_numpy(rgb[i]).cuda().long()].permute(2, 0, 1))
            raw = np.array(Image.open(os.path.join(out, "depth", stamps[i] + ".png")))
            assert np.array_equal(raw, u16[i]) and np.array_equal(np.asarray(d), np.asarray(raw / res["calibration"]["depth_scale"], dtype=np.asarray(d).dtype))
            assert torch.allclose(pose.cpu().float(), poses[i], atol=1e-5)
    finally:
        ds.close()
    # without the optional outputs nothing else is written
    out2 = str(tmp_path / "plain")
    pb.write(poses[:3], times[:3], out2, depth_colour=False)
    assert sorted(os.listdir(out2)) == ["rgb"] and len(os.listdir(os.path.join(out2, "rgb"))) == 3


def test_play_map_tool_prints_one_json_line_from_a_fresh_process(dynamic_run, tmp_path):
    _, directory = dynamic_run
    out = str(tmp_path / "played")
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "play_map.py"), "--map", directory, "--path", "frozen-camera:3:5", "--out", out,
                        "--no-depth-vis"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["frames"] == 5 and line["seconds"] > 0 and line["fps"] > 0 and line["writer_wait_s"] >= 0 and line["dynamic"] is True
    assert sorted(os.listdir(out)) == ["rgb"] and len(os.listdir(os.path.join(out, "rgb"))) == 5
