"""The pose from 2D-3D matches on the device (gsr_feat_pose_pnp of include/feature_matching.h, csrc/gs_features.h, slam/features.py): bit
for bit against the numpy restatement (tests/pnp_reference.py) on the analytic scenes and at the edges of the pair count, what depth it
reads and what it does not, guard words, refusals; then the stage in use with ``solver: pnp``: the seeder end to end and in a graph, the
dense alignment started from the seed, and localisation of RGB-only frames in a saved map."""
import math
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import features_reference as ref  # noqa: E402
import odometry_reference as odo  # noqa: E402
import pnp_reference as pnp  # noqa: E402
from slam import features  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
DIRECTIONS, PATTERN = features.pattern_tables(0)
POSE = dict(seed=0, min_area=features.MIN_AREA, tau_px=2.0, refine_iters=3, min_matches=12, min_inliers=8, min_share=0.5, max_translation=1.5,
            max_rotation=math.radians(45.0))
LOOSE = dict(min_matches=0, min_inliers=3, min_share=0.0)


def _dev(a, dtype=None):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _guarded(n, dtype=torch.int32):
    """(the whole buffer, its first n entries): four guard entries follow the output"""
    buf = torch.full((n + 4,), GUARD, dtype=dtype, device="cuda")
    return buf, buf[:n]


def _guard_ok(buf, n):
    return bool((buf[n:] == GUARD).all())


def _pose(kp_a, depth_a, kp_b, matches, K, hypotheses, **over):
    tbuf, T = _guarded(16, torch.float32)
    sbuf, stats = _guarded(8)
    cbuf, counts = _guarded(hypotheses)
    tbuf[16:] = 7.0
    k = _dev(np.asarray(K, np.float32))
    features.pose_pnp(_dev(kp_a), _dev(depth_a), _dev(kp_b), _dev(matches), k, k, T.view(4, 4), stats, hypotheses=hypotheses, counts=counts,
                      **{**POSE, **over})
    torch.cuda.synchronize()
    assert bool((tbuf[16:] == 7.0).all()) and _guard_ok(sbuf, 8) and _guard_ok(cbuf, hypotheses)
    return T.view(4, 4).cpu().numpy(), stats.cpu().numpy(), counts.cpu().numpy()


def _check(kp_a, depth_a, kp_b, matches, K, hypotheses, **over):
    """counts, the winner and stats equal the restatement bit for bit, T within the header's 2.4e-7 max(1, |entry|); the same bytes twice"""
    want = pnp.pose(kp_a, depth_a, kp_b, matches, K, K, count=hypotheses, **{**POSE, **over})
    T, stats, counts = _pose(kp_a, depth_a, kp_b, matches, K, hypotheses, **over)
    assert counts.tolist() == want["counts"].tolist()
    assert stats.tolist() == want["stats"].tolist()
    assert np.all(np.abs(T.astype(np.float64) - want["T"]) <= 2.4e-7 * np.maximum(1.0, np.abs(want["T"])))
    if stats[6] == 0:
        assert T.tobytes() == np.eye(4, dtype=np.float32).tobytes()      # a refusal returns the identity exactly
    T2, stats2, counts2 = _pose(kp_a, depth_a, kp_b, matches, K, hypotheses, **over)
    assert T2.tobytes() == T.tobytes() and stats2.tobytes() == stats.tobytes() and counts2.tobytes() == counts.tobytes()
    return T, stats, want


_scene_cases = {}


def _scene_case(name, W=160, H=120):
    """keypoints and matches of a scene by the restatement: the pose kernels are tested on their own"""
    if (name, W, H) not in _scene_cases:
        image_a, depth_a, image_b, depth_b, K, T_true = ref.scene(name, W, H)
        a = ref.extract(image_a, None, 16, 3, 20, DIRECTIONS, PATTERN)
        b = ref.extract(image_b, None, 16, 3, 20, DIRECTIONS, PATTERN)
        _scene_cases[(name, W, H)] = (a[0], depth_a, b[0], depth_b, ref.match(*a, *b, 64, 6), K, T_true)
    return _scene_cases[(name, W, H)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hypotheses", [1, 64, 1024])
@pytest.mark.parametrize("W,H", [(160, 120), (161, 97)])
@pytest.mark.parametrize("name", ["wider", "roll", "unrelated"])
def test_pose_on_the_scene_equals_the_restatement(name, W, H, hypotheses):
    kp_a, depth_a, kp_b, _, matches, K, T_true = _scene_case(name, W, H)
    T, stats, want = _check(kp_a, depth_a, kp_b, matches, K, hypotheses)
    if name != "unrelated" and hypotheses >= 64:
        assert stats[6] == 1
        degrees, mm = odo.pose_error(T.astype(np.float64), T_true)
        assert degrees <= 3.0 and mm <= 150.0                            # the bars of tests/test_pnp_host.py
    if name == "unrelated":
        assert stats[6] == 0


_planted = {}


def _planted_pairs():
    """1200 slots at 320 x 240 under the wide motion: B's keypoints on distinct integer pixels, A's where B's points project (candidates
    that project outside A are passed over), A's depth exact there. No depth of B exists. (kp_a, depth_a, kp_b, matches with every slot
    matched to its own, K, T_true)"""
    if not _planted:
        rng = np.random.default_rng(11)
        W, H, n = 320, 240, 1200
        K = tuple(float(np.float32(v)) for v in odo.intrinsics(W, H))
        T_true = ref.MOTIONS["wide"]
        cells = rng.permutation((W // 4) * (H // 4))                     # distinct pixels of B on a 4-pixel lattice
        xb, yb = 4 * (cells % (W // 4)) + 1, 4 * (cells // (W // 4)) + 1
        zb = rng.uniform(1.5, 3.5, len(cells))
        PB = np.stack([(xb - K[2]) * zb / K[0], (yb - K[3]) * zb / K[1], zb], axis=1)
        PA = (PB - T_true[:3, 3]) @ T_true[:3, :3]
        xa = np.rint(K[0] * PA[:, 0] / PA[:, 2] + K[2]).astype(np.int64)
        ya = np.rint(K[1] * PA[:, 1] / PA[:, 2] + K[3]).astype(np.int64)
        take = np.nonzero((xa >= 0) & (xa < W) & (ya >= 0) & (ya < H) & (PA[:, 2] > 0))[0][:n]
        assert len(take) == n
        depth_a = np.full((H, W), 0.0, np.float32)
        depth_a[ya[take], xa[take]] = PA[take, 2]                        # pixels hit twice keep the later depth: a few outliers
        fill = (np.full(n, 30), np.zeros(n, np.int64))
        kp_a, kp_b = np.stack([xa[take], ya[take], *fill], axis=1).astype(np.int32), np.stack([xb[take], yb[take], *fill], axis=1).astype(np.int32)
        matches = np.stack([np.arange(n), np.full(n, 10)], axis=1).astype(np.int32)
        _planted["case"] = (kp_a, depth_a, kp_b, matches, K, T_true)
    return _planted["case"]


@pytest.mark.parametrize("M", [0, 2, 3, 63, 64, 65, 1200])
def test_pose_at_the_edges_of_the_pair_count(M):
    """63, 64, 65: the edges of the 64-lane ballot loop of the hypotheses; 1200 slots cross the 256-thread chunk of the pair list. With
    all 1200 slots, 30 % of B's pixels are replaced by seeded outliers."""
    kp_a, depth_a, kp_b, matches, K, T_true = _planted_pairs()
    matches = matches.copy()
    hit = np.nonzero(matches[:, 0] >= 0)[0]
    if M == 1200:
        rng = np.random.default_rng(12)
        wrong = rng.uniform(size=len(matches)) < 0.3
        matches[wrong, 0] = rng.integers(0, len(matches), size=int(wrong.sum()))
        T, stats, _ = _check(kp_a, depth_a, kp_b, matches, K, 256)
        assert stats[2] == 1200
        assert stats[6] == 1 and stats[5] >= 0.5 * stats[2]
        degrees, mm = odo.pose_error(T.astype(np.float64), T_true)
        assert degrees <= 3.0 and mm <= 150.0
        return
    keep = hit[np.linspace(0, len(hit) - 1, M).astype(int)] if M else hit[:0]       # spread over the slots
    matches[np.setdiff1d(hit, keep), 0] = -1
    _, stats, _ = _check(kp_a, depth_a, kp_b, matches, K, 64, **LOOSE)
    assert stats[2] == M
    if M < 3:
        assert stats[4] == 0 and stats[6] == 0
    if M >= 63:
        assert stats[6] == 1 and stats[5] >= 0.8 * M


def test_pose_reads_the_depth_of_a_alone():
    """A's keypoints on NaN, zero, negative and infinite depth are left out. B has no depth here; where a sensor would have returned holes
    for B (every second matched keypoint), gsr_feat_pose with that depth loses those pairs and this call keeps them."""
    kp_a, depth_a, kp_b, depth_b, matches, K, _ = _scene_case("wider")
    depth_a, holes = depth_a.copy(), depth_b.copy()
    hit = np.nonzero(matches[:, 0] >= 0)[0]
    for k, bad in enumerate((0.0, np.nan, -1.0, np.inf)):
        depth_a[kp_a[hit[k], 1], kp_a[hit[k], 0]] = bad
    lost = hit[4::2]
    holes[kp_b[matches[lost, 0], 1], kp_b[matches[lost, 0], 0]] = np.nan
    _, stats, _ = _check(kp_a, depth_a, kp_b, matches, K, 256)
    assert stats[2] == len(hit) - 4
    k = _dev(np.asarray(K, np.float32))
    T, points_stats = torch.empty((4, 4), device="cuda"), torch.empty(8, dtype=torch.int32, device="cuda")
    features.pose(_dev(kp_a), _dev(depth_a), _dev(kp_b), _dev(holes), _dev(matches), k, k, T, points_stats, **{**POSE, "tau_depth": 0.05})
    print(f"pairs with holes in B: gsr_feat_pose keeps {int(points_stats[2])}, gsr_feat_pose_pnp {int(stats[2])} of {len(hit)} matches")
    assert int(points_stats[2]) == len(hit) - 4 - len(lost) < stats[2]


def test_refusals_leave_the_outputs_untouched():
    kp_a, depth_a, kp_b, _, matches, K, _ = _scene_case("wider")
    tbuf, T = _guarded(16, torch.float32)
    sbuf, stats = _guarded(8)
    cbuf, counts = _guarded(64)
    k = _dev(np.asarray(K, np.float32))
    args = [_dev(kp_a), _dev(depth_a), _dev(kp_b), _dev(matches), k, k, T.view(4, 4), stats]
    small = torch.empty(16, dtype=torch.uint8, device="cuda")
    lib = features._C.load_library()
    need = int(lib.gsr_feat_pose_pnp_workspace_size(len(kp_a), 64))
    assert need > 0 and need == int(lib.gsr_feat_pose_workspace_size(len(kp_a), 64))
    assert lib.gsr_feat_pose_pnp_workspace_size(0, 64) == 0 and lib.gsr_feat_pose_pnp_workspace_size(4097, 64) == 0
    assert lib.gsr_feat_pose_pnp_workspace_size(240, 0) == 0 and lib.gsr_feat_pose_pnp_workspace_size(240, 1025) == 0
    misaligned = torch.empty(need + 32, dtype=torch.uint8, device="cuda")[4:]
    before = tbuf.clone()
    for text, over in (("hypotheses must be in", {"hypotheses": 0}), ("hypotheses must be in", {"hypotheses": 1025}),
                       ("min_area must be positive", {"min_area": 0.0}), ("min_area must be positive", {"min_area": float("inf")}),
                       ("tau_px must be finite and not negative", {"tau_px": -1.0}),
                       ("tau_px must be finite and not negative", {"tau_px": float("nan")}),
                       ("refine_iters must be in", {"refine_iters": 17}), ("refine_iters must be in", {"refine_iters": -1}),
                       ("min_matches must not be negative", {"min_matches": -1}), ("min_inliers must be at least 3", {"min_inliers": 2}),
                       ("min_share must be in", {"min_share": 1.5}), ("min_share must be in", {"min_share": -0.1}),
                       ("max_translation and max_rotation", {"max_rotation": -0.1}),
                       ("max_translation and max_rotation", {"max_translation": float("inf")}),
                       ("workspace must be 16-byte aligned and hold", {"workspace": small}),
                       ("workspace must be 16-byte aligned and hold", {"workspace": misaligned})):
        with pytest.raises(RuntimeError, match="gsr_feat_pose_pnp: " + text):
            features.pose_pnp(*args, **{**POSE, "hypotheses": 64, "counts": None if "hypotheses" in over else counts, **over})
    # null outputs and a size outside the ranges, through the library itself (the binding refuses a missing tensor before the call)
    from diff_gaussian_rasterization._C import stream_handle
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ptr = lambda t: t.data_ptr()
    gate = (0, 64, features.MIN_AREA, 2.0, 3, 12, 8, 0.5, 1.5, 0.7)
    raw = lambda W, H, T_ptr, stats_ptr: lib.gsr_feat_pose_pnp(W, H, len(kp_a), ptr(args[0]), ptr(args[1]), len(kp_b), ptr(args[2]), ptr(args[3]),
                                                               ptr(k), ptr(k), *gate, T_ptr, stats_ptr, ptr(counts), ptr(ws), need,
                                                               stream_handle(None, ws.device))
    for text, call in (("T, stats and workspace must not be NULL", lambda: raw(160, 120, None, ptr(stats))),
                       ("T, stats and workspace must not be NULL", lambda: raw(160, 120, ptr(T), None)),
                       ("width and height must be at least 1", lambda: raw(0, 120, ptr(T), ptr(stats)))):
        with pytest.raises(RuntimeError, match="gsr_feat_pose_pnp: .*" + text):
            call()
    torch.cuda.synchronize()
    assert bool((sbuf == GUARD).all()) and bool((cbuf == GUARD).all()) and torch.equal(tbuf, before)


# ---- the stage object -----------------------------------------------------------------------------------------------------------------------
def test_the_seeder_with_the_pnp_solver_equals_the_restatement_and_replays_in_a_graph():
    image_a, depth_a, image_b, depth_b, K, T_true = ref.scene("wider", 160, 120)
    opt = features.default_options(cell=16, per_cell=3, solver="pnp")
    seeder = features.FeatureSeeder((160, 120), K, opt, "cuda:0")
    ia, ib, da = _dev(image_a), _dev(image_b), _dev(depth_a)
    a, b = seeder.features(ia), seeder.features(ib)
    T, stats = seeder.pose(a, da, b)                                     # a frame without depth
    want_a = ref.extract(image_a, None, 16, 3, 20, DIRECTIONS, PATTERN)
    want_b = ref.extract(image_b, None, 16, 3, 20, DIRECTIONS, PATTERN)
    want = pnp.pose(want_a[0], depth_a, want_b[0], ref.match(*want_a, *want_b, 64, 6), K, K, count=256, **POSE)
    assert stats.tolist() == want["stats"].tolist() and stats[6] == 1
    assert np.all(np.abs(T.cpu().numpy().astype(np.float64) - want["T"]) <= 2.4e-7 * np.maximum(1.0, np.abs(want["T"])))
    degrees, mm = odo.pose_error(T.cpu().numpy().astype(np.float64), T_true)
    assert degrees <= 3.0 and mm <= 150.0
    # nothing of B's depth enters: the true depth and one of NaN give the bytes of none at all
    for depth in (_dev(depth_b), torch.full((120, 160), float("nan"), device="cuda")):
        T2, stats2 = seeder.pose(a, da, b, depth)
        assert torch.equal(T2, T) and torch.equal(stats2, stats)
    assert seeder.summary() == {"feature_seeds_tried": 3, "feature_seeds_accepted": 3}
    points = features.FeatureSeeder((160, 120), K, features.default_options(cell=16, per_cell=3), "cuda:0")
    with pytest.raises(ValueError, match="the second frame has no depth"):
        points.pose(a, da, b, None)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            ga, gb = seeder.features(ia), seeder.features(ib)
            gT, gstats = seeder.pose(ga, da, gb)
    torch.cuda.current_stream().wait_stream(stream)
    gT.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gT, T) and torch.equal(gstats, stats)


def test_the_dense_alignment_converges_from_the_pnp_seed():
    """The alignment LoopCloser.verify runs on the 'wider' pair (26 degrees, 0.97 m; tests/test_hip_features.py) as a frame without depth
    gets it -- the levels and passes of Training.loop_closure, photometric and affine terms alone, no depth of B, the gate of
    Training.feature_seed. From the identity it is refused; from the PnP seed it is accepted, at most twice as far from the truth as
    from the 3D-3D seed of the same pair. Measured on an MI355X: refused from the identity; 0.0313 degrees / 1.453 mm from either seed
    (the seeds themselves: 0.043 degrees / 2.6 mm and 0.512 degrees / 21.8 mm). Without the affine term (what Relocaliser._seed runs) the
    alignment of this analytic pair converges from the identity too, to 0.0311 degrees / 1.462 mm: DESIGN.md section 8, Feature seed."""
    from slam.odometry import DenseOdometry
    from slam.stages import loop_closure_options
    image_a, depth_a, image_b, depth_b, K, T_true = ref.scene("wider", 160, 120)
    loops = loop_closure_options({"loop_closure": {"enabled": True}})
    ia, ib, da, db = _dev(image_a), _dev(image_b), _dev(depth_a), _dev(depth_b)
    seeds = {}
    for solver in ("points", "pnp"):
        opt = features.default_options(cell=16, per_cell=3, solver=solver)
        seeder = features.FeatureSeeder((160, 120), K, opt, "cuda:0")
        seeds[solver], stats = seeder.pose(seeder.features(ia), da, seeder.features(ib), db if solver == "points" else None)
        assert stats[6] == 1
    odometry = DenseOdometry(160, 120, K, levels=loops["levels"], iters=loops["iters"], max_translation=opt["max_translation"],
                             max_rotation=opt["max_rotation"], device="cuda:0", affine=True, geometric_weight=0.0)
    odometry.keep(ia, da, None)
    error = {}
    for start in ("identity", "points", "pnp"):
        T, stats = odometry.align(ib, T_init=seeds.get(start))
        error[start] = (bool(stats[0] > 0.5), *odo.pose_error(T.cpu().numpy().astype(np.float64), T_true))
    seed_error = {k: odo.pose_error(v.cpu().numpy().astype(np.float64), T_true) for k, v in seeds.items()}
    print("alignment of 'wider' from " + "; ".join(f"{k}: accepted {v[0]}, {v[1]:.4f} deg {v[2]:.3f} mm" for k, v in error.items()) +
          "; the seeds themselves: " + "; ".join(f"{k} {v[0]:.4f} deg {v[1]:.3f} mm" for k, v in seed_error.items()))
    assert not error["identity"][0]
    assert error["points"][0] and error["pnp"][0]
    assert error["pnp"][1] <= 2.0 * error["points"][1] and error["pnp"][2] <= 2.0 * error["points"][2]


# ---- the stage in use: RGB-only frames in a saved map -----------------------------------------------------------------------------------------
FRAMES, WIDTH, HEIGHT = 40, 320, 240
TRAINING = {"init_itr_num": 400, "init_gaussian_update": 100, "init_gaussian_reset": 200, "tracking_itr_num": 60, "static_map_iters": 30,
            "gaussian_update_every": 60, "gaussian_update_offset": 20, "tracking_graph": True}
FAR_R, FAR_T = torch.eye(3), torch.tensor([5.0, -4.0, 6.0])


def _dataset(sensor_depth=True):
    from slam.dataset import SyntheticRGBDDataset
    return SyntheticRGBDDataset(num_frames=FRAMES, width=WIDTH, height=HEIGHT, seed=0, texture="blocks", sensor_depth=sensor_depth)


@pytest.fixture(scope="module")
def blocks_map(tmp_path_factory):
    """The one run of the module: the RGB-D run on the blocks room of tests/test_hip_features.py and its saved map: (slam, directory)"""
    from slam.system import SLAM, default_config, merge_config
    torch.manual_seed(0)
    cfg = merge_config(default_config(), {"Training": {**TRAINING, "relocalisation": {"enabled": True}},
                                          "Dataset": {"pcd_downsample": 32, "pcd_downsample_init": 8},
                                          "opt_params": {"densify_from_iter": 150}, "Results": {"eval_rendering": False}})
    slam = SLAM(cfg, _dataset())
    slam.gaussians.generator = torch.Generator(device="cuda").manual_seed(0)
    slam.run()
    directory = str(tmp_path_factory.mktemp("pnp") / "map")
    slam.save_map(directory)
    return slam, directory


def _ate(cameras, ids, poses):
    """RMSE of the camera centres over `ids` after one rigid fit over them; poses {id: (R, T)}"""
    from slam.eval_utils import align
    centre = lambda R, T: -R.detach().double().cpu().numpy().T @ T.detach().double().cpu().numpy()
    est = lambda i: centre(*poses[i])
    gt = lambda i: centre(cameras[i].R_gt, cameras[i].T_gt)
    rot, trans, _ = align(np.stack([est(i) for i in ids]).T, np.stack([gt(i) for i in ids]).T)
    return float(np.sqrt(np.mean([np.linalg.norm(rot @ est(i) + trans[:, 0] - gt(i)) ** 2 for i in ids])))


def _localise_all(blocks_map, monocular, seed_block):
    from slam.map_io import load_map
    from slam.relocalise import MapLocaliser
    from slam.system import merge_config
    slam, directory = blocks_map
    addition = {"Training": {"feature_seed": seed_block, "monocular": monocular}}
    if monocular:
        addition["Dataset"] = {"sensor_type": "monocular"}
    loc = MapLocaliser(load_map(directory), merge_config(slam.config, addition))
    ds = _dataset(sensor_depth=not monocular)
    keyframes = set(slam.frontend.kf_indices)
    others = [i for i in sorted(slam.frontend.cameras) if i not in keyframes]
    poses, found = {}, []
    for i in others:
        viewpoint = loc.camera(ds, i)
        assert (viewpoint.depth is None) == monocular and (viewpoint.depth_device() is None) == monocular
        viewpoint.update_RT(FAR_R, FAR_T)
        found.append(loc.localise(viewpoint))
        poses[i] = (viewpoint.R.detach().clone(), viewpoint.T.detach().clone())
    return loc, others, poses, found


def test_rgb_only_frames_are_found_in_the_saved_map_with_the_pnp_seed(blocks_map):
    """Every non-keyframe of the run, given as an RGB-only frame (no depth, sensor_type monocular) from a pose metres away, is found with
    ``solver: pnp``; some seeds are accepted; the ATE over these frames is at most 1.5 times that of the same localisation without the
    seed, which is the reference here. The share of accepted seeds is printed beside that of the points solver on the RGB-D frames."""
    slam, _ = blocks_map
    cameras = slam.frontend.cameras
    loc, others, poses, found = _localise_all(blocks_map, True, {"enabled": True, "solver": "pnp"})
    seeds = loc.relocaliser.seeder.summary()
    off, _, poses_off, found_off = _localise_all(blocks_map, True, {"enabled": False})
    assert off.relocaliser.seeder is None
    rgbd, _, _, found_rgbd = _localise_all(blocks_map, False, {"enabled": True})
    seeds_rgbd = rgbd.relocaliser.seeder.summary()
    ate, ate_off = _ate(cameras, others, poses), _ate(cameras, others, poses_off)
    share = lambda s: s["feature_seeds_accepted"] / max(1, s["feature_seeds_tried"])
    print(f"saved blocks map, {len(others)} RGB-only frames: found {sum(o['accepted'] for o in found)} with the pnp seed (seeds {seeds}, "
          f"accepted share {share(seeds):.3f}), ATE {ate * 1000:.2f} mm; without the seed found {sum(o['accepted'] for o in found_off)}, ATE "
          f"{ate_off * 1000:.2f} mm; the points solver on the RGB-D frames: found {sum(o['accepted'] for o in found_rgbd)}, seeds {seeds_rgbd}, "
          f"accepted share {share(seeds_rgbd):.3f}")
    assert len(others) >= 20 and all(o["accepted"] for o in found)
    assert seeds["feature_seeds_tried"] >= len(others) and seeds["feature_seeds_accepted"] > 0
    assert ate <= 1.5 * ate_off
