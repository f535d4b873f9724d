"""CPU-side tests of the SLAM-loop host logic against golden vectors produced by the reference's own Python
(tests/golden/make_golden_slam.py): keyframe management, trajectory alignment / ATE, pose algebra, gradient mask, PSNR, median
depth, learning-rate schedule; plus the PLY format round trip. No GPU, no oracle involvement."""
import os
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

G = np.load(os.path.join(REPO, "tests", "golden", "golden_slam.npz"))


def _frontend():
    from slam.frontend import FrontEnd
    cfg = {"Training": {"monocular": False, "kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3,
                        "window_size": 8}, "model_params": {"dynamic_model": False}}
    fe = FrontEnd(cfg)
    fe.cameras = {k: types.SimpleNamespace(R=torch.tensor(G["window_R"][k]), T=torch.tensor(G["window_T"][k]), uid=k) for k in range(12)}
    vis = {k: torch.tensor(G["window_vis"][k]) for k in range(12)}
    return fe, vis


def test_is_keyframe_matches_reference():
    fe, vis = _frontend()
    for cur, last, med, want in G["window_is_keyframe"]:
        fe.median_depth = float(med)
        assert fe.is_keyframe(int(cur), int(last), vis[int(cur)], vis) == bool(want)


def test_add_to_window_matches_reference():
    fe, vis = _frontend()
    for row in G["window_add"]:
        row = [int(v) for v in row]
        init_flag, cur, removed, n = row[:4]
        window = row[4:4 + n]
        rest = row[4 + n + 1:]
        want = rest[:rest.index(-9)] if -9 in rest else rest
        fe.initialized = bool(init_flag)
        w, rem = fe.add_to_window(cur, vis[cur], vis, list(window))
        assert w == want and (rem if rem is not None else -1) == removed


def test_align_and_ate_match_reference():
    from slam.eval_utils import align, ate_rmse, evaluate_ate
    gt, est = G["align_gt"], G["align_est"]
    rot, trans, err = align(gt.T, est.T)
    np.testing.assert_allclose(rot, G["align_rot"], atol=1e-10)
    np.testing.assert_allclose(trans, G["align_trans"], atol=1e-10)
    np.testing.assert_allclose(err, G["align_err"], atol=1e-10)
    mk = lambda p: [np.block([[np.eye(3), q[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]) for q in p]
    assert abs(evaluate_ate(mk(gt), mk(est)) - float(G["align_ate_mean"])) < 1e-12
    # a rigidly moved copy has zero error; the RMSE form is >= the mean form
    assert ate_rmse(mk(gt), mk((G["align_rot"] @ gt.T + G["align_trans"]).T)) < 1e-9
    assert ate_rmse(mk(gt), mk(est)) >= evaluate_ate(mk(gt), mk(est)) - 1e-12


def test_pose_algebra_matches_reference():
    from slam.camera import SE3_exp
    R0 = torch.tensor([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])
    T0 = torch.tensor([0.1, -0.2, 0.3])
    for row in G["pose_cases"]:
        tau = torch.tensor(row[:6], dtype=torch.float32)
        W = torch.eye(4)
        W[:3, :3], W[:3, 3] = R0, T0
        new = SE3_exp(tau) @ W
        np.testing.assert_allclose(new[:3, :3].numpy().ravel(), row[6:15], atol=1e-6)
        np.testing.assert_allclose(new[:3, 3].numpy(), row[15:18], atol=1e-6)
        assert bool(tau.norm() < 1e-4) == bool(row[18])


def test_small_helpers_match_reference():
    from slam.camera import compute_grad_mask
    from slam.eval_utils import psnr
    from slam.frontend import get_median_depth
    from slam.gaussian_model import helper
    m = compute_grad_mask(torch.tensor(G["gradmask_image"]), {"Training": {"edge_threshold": 1.1}, "Dataset": {"type": "tum"}})
    assert np.array_equal(m.numpy(), G["gradmask_mask"])
    a, b = torch.tensor(G["psnr_in"][0]), torch.tensor(G["psnr_in"][1])
    np.testing.assert_allclose(psnr(a, b).numpy(), G["psnr_out"], rtol=1e-6)
    d, o = torch.tensor(G["median_in"][0]), torch.tensor(G["median_in"][1])
    assert abs(float(get_median_depth(d, o)) - float(G["median_out"])) < 1e-7
    for step, lr in G["lr_helper"]:
        assert abs(helper(step, lr_init=0.00096, lr_final=0.0000096, lr_delay_mult=0.01, max_steps=30000) - lr) < 1e-15


def test_ply_round_trip_and_layout(tmp_path):
    from slam.ply_io import read_ply, write_ply
    rng = np.random.default_rng(0)
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2", "opacity", "scale_0", "rot_0", "rot_1", "rot_2", "rot_3", "dygs"]
    data = rng.normal(size=(37, len(names))).astype(np.float32)
    data[:, -1] = rng.uniform(size=37) < 0.3
    path = str(tmp_path / "point_cloud.ply")
    write_ply(path, names, data)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n") + len(b"end_header\n")].decode()
    # the layout plyfile writes for the reference's save_ply: binary little endian, one float property per attribute, in order
    assert header.splitlines()[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    assert [l.split()[-1] for l in header.splitlines() if l.startswith("property float")] == names
    assert len(raw) == len(header) + 37 * len(names) * 4
    n2, d2 = read_ply(path)
    assert n2 == names and np.array_equal(d2, data)
    # ascii variant
    with open(str(tmp_path / "a.ply"), "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty uchar dygs\nend_header\n1.5 1\n-2 0\n")
    n3, d3 = read_ply(str(tmp_path / "a.ply"))
    assert n3 == ["x", "dygs"] and np.allclose(d3, [[1.5, 1], [-2, 0]])
    with pytest.raises(ValueError):
        open(str(tmp_path / "b.ply"), "w").write("not a ply\n")
        read_ply(str(tmp_path / "b.ply"))


def test_slam_map_symbols_and_argument_errors():
    """include/slam_map.h entry points are exported and reject bad arguments without touching a GPU."""
    from diff_gaussian_rasterization import _C
    L = _C.load_library()
    assert L.gsr_seed_workspace_size(1000) > 1000 * 4
    seed = lambda n: L.gsr_seed_from_rgbd(n, None, 4, 4, None, None, None, None, 1.0, 1.0, 0.0, 0.0, None, None, 0.01, 3, *([None] * 7))
    rejected = lambda: pytest.raises(RuntimeError, match=r"failed \(code -\d+\)")
    with rejected():
        seed(-1)
    with rejected():
        seed(5)
    assert seed(0) == 0
    with rejected():
        L.gsr_densify_select(10, None, None, None, 3, None, 0.1, 0.1, 0.1, 0.1, None, None)
    with rejected():
        L.gsr_densify_select(10, None, None, None, 2, None, 0.1, 0.1, 0.1, 0.1, None, None)
    with rejected():
        L.gsr_densify_apply(10, None, None, 1, 0, 0, 0, 40, None, None, None, 3, None, None, None)
    with rejected():
        L.gsr_camera_step_launch(None, None)


@pytest.mark.parametrize("case", ["a", "b"])
def test_keyframe_selection_overlap_matches_reference(case):
    """slam.keyframes.keyframe_selection_overlap (one batched projection of the newest keyframe's depth samples into every older keyframe)
    against the reference's own Camera.keyframe_selection_overlap (utils/camera_utils.py:319-365; tests/golden/make_golden_keyframe_overlap.py):
    the candidate order the permutation sees, and the selection under the same numpy seed. Case b has the newest keyframe at the identity
    pose with a centred principal point: get_pointcloud's duplicate filter then drops all but 32 of 2 741 points -- reproduced."""
    from slam import keyframes as kf
    K = np.load(os.path.join(REPO, "tests", "golden", "golden_keyframe_overlap.npz"))
    ids = [int(i) for i in K[case + "_ids"]]
    cams = {i: types.SimpleNamespace(uid=i, R=torch.tensor(K[case + "_R"][k]), T=torch.tensor(K[case + "_T"][k])) for k, i in enumerate(ids)}
    me = cams[int(K[case + "_self"])]
    me.depth = K[case + "_depth"]
    fx, fy, cx, cy, W, H = K[case + "_intr"]
    intr = (fx, fy, cx, cy, int(W), int(H))
    by_overlap = kf.keyframe_selection_overlap(me, cams, int(K[case + "_time"]), intr, pose_window=-100, permutation=lambda a: a)
    assert by_overlap == [int(v) for v in K[case + "_sorted"]]
    assert 5 not in by_overlap                                   # the keyframe that looks the other way sees nothing
    np.random.seed(int(K[case + "_seed"]))
    assert kf.keyframe_selection_overlap(me, cams, int(K[case + "_time"]), intr, permutation=np.random.permutation) == [int(v) for v in K[case + "_selected"]]
    torch.manual_seed(3)                                         # the default draw: torch's generator, a permutation of the same candidates
    mine = kf.keyframe_selection_overlap(me, cams, int(K[case + "_time"]), intr)
    assert len(mine) == min(5, len(by_overlap)) and set(mine) <= set(by_overlap) and len(set(mine)) == len(mine)
    assert kf.keyframe_selection_overlap(me, cams, 0, intr) == []     # nothing older than `time`
    if case == "b":
        k = ids.index(int(K["b_self"]))
        pts = kf.backprojected_points(torch.tensor(K["b_depth"]), torch.tensor(K["b_R"][k]), torch.tensor(K["b_T"][k]), fx, fy, cx, cy)
        assert pts.shape[0] == 32 and int((K["b_depth"] > 0).sum()) == 2741


def test_network_warmup_schedule_is_pinned():
    """BackEnd.network_warmup(iters) -- the reference's literal 100 for its 200-iteration call (utils/slam_backend.py:337-338,
    :765-770), proportional (an intentional, documented deviation) for shorter schedules, overridable by Training.network_warmup_iters."""
    from slam.backend import BackEnd
    cfg = {"Training": {"pose_window": 3, "monocular": False}, "model_params": {"dynamic_model": True}}
    be = BackEnd(cfg)
    assert [be.network_warmup(n) for n in (1, 10, 80, 199, 200, 300)] == [0, 5, 40, 99, 100, 100]
    cfg["Training"]["network_warmup_iters"] = 7
    assert [be.network_warmup(n) for n in (1, 10, 80, 200)] == [7, 7, 7, 100]        # the reference-length call keeps the reference's literal


def test_overlap_fractions_in_groups_equal_one_batched_projection(monkeypatch):
    """The candidates are projected OVERLAP_GROUP at a time (bounded peak memory): same fractions as one einsum over all of them."""
    from slam import keyframes as kf
    g = torch.Generator().manual_seed(5)
    pts = torch.rand((5000, 3), generator=g) * torch.tensor([4.0, 3.0, 5.0]) - torch.tensor([2.0, 1.5, 0.0])
    K = 37
    ang = torch.rand(K, generator=g) * 0.6 - 0.3
    Rs = torch.stack([torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32) for a in ang.tolist()])
    Ts = torch.rand((K, 3), generator=g) - 0.5
    args = (pts, Rs, Ts, 300.0, 300.0, 160.0, 120.0, 320, 240)
    monkeypatch.setattr(kf, "OVERLAP_GROUP", 1000)
    whole = kf.overlap_fractions(*args)
    for group in (1, 16, 37):
        monkeypatch.setattr(kf, "OVERLAP_GROUP", group)
        part = kf.overlap_fractions(*args)
        assert part.shape == (K,) and torch.equal(part, whole), group
    assert 0.0 < float(whole.mean()) < 1.0


def test_keyframe_operand_store_is_bounded_by_bytes_and_shares_ground_truth(monkeypatch):
    """slam.keyframe_slots.KeyframeOperands: one ground-truth copy per keyframe whatever the flag variant, a byte budget with
    least-recently-used eviction, and Camera.clean()'s hook (slam_losses.drop_keyframe_constants) drops the keyframe's entry."""
    import slam_losses
    from slam import keyframe_slots as mg
    calls = []

    def fake_operands(config, viewpoint, device, rm_dynamic=False, mask=None, dynamic=False):
        calls.append((viewpoint.uid, rm_dynamic, dynamic))
        return (torch.full((3, 4, 4), float(viewpoint.uid)), torch.zeros((1, 4, 4)), torch.full((1, 4, 4), float(rm_dynamic)),
                torch.full((1, 4, 4), float(dynamic)), 0.9)

    monkeypatch.setattr(slam_losses, "mapping_loss_operands", fake_operands)
    monkeypatch.setattr(mg, "device_store_budget", lambda device, fraction, floor_bytes=0: 3 * (4 * 16 * 4 + 2 * 16 * 4) + 10)   # three one-variant keyframes
    store = mg.KeyframeOperands()
    cams = [types.SimpleNamespace(uid=k) for k in range(5)]
    a = store.get({}, cams[0], "cpu", rm_dynamic=True, dynamic=False)
    b = store.get({}, cams[0], "cpu", rm_dynamic=False, dynamic=True)
    assert a[0] is b[0] and a[1] is b[1] and a[2] is not b[2]                  # ground truth once, weights per variant
    assert store.get({}, cams[0], "cpu", rm_dynamic=True, dynamic=False)[2] is a[2] and len(calls) == 2
    assert store.held_bytes() == 4 * 16 * 4 + 2 * (2 * 16 * 4)
    for c in cams[1:4]:
        store.get({}, c, "cpu")
    assert id(cams[0]) not in store._held and store.held_bytes() <= store._budget          # the oldest keyframe went first
    assert store.get({}, cams[0], "cpu", rm_dynamic=True, dynamic=False)[0] is not a[0]    # ... and is formed again on demand
    held = store.held_bytes()
    slam_losses.drop_keyframe_constants(cams[3])                               # what Camera.clean() calls
    assert id(cams[3]) not in store._held and store.held_bytes() < held
    slam_losses.drop_keyframe_constants(None)
    assert store.held_bytes() == 0 and not store._held
