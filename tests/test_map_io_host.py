"""CPU tests of saving and reopening a map (slam/map_io.py, DeformModel.save_weights / load_weights): exact round trips of a static and a
dynamic model built from doubles the way tests/test_slam_host.py builds its cameras, the refusals with the file and field they name, and the
reference's own state_dict names (tests/golden/reference_deform_state.json) through the rename table."""
import json
import os
import types

import numpy as np
import pytest
import torch

from util import REPO


def _model(dynamic, P=57, nodes=23, seed=0, isotropic=False):
    from slam.deform_model import DeformModel
    from slam.gaussian_model import GaussianModel
    gen = torch.Generator().manual_seed(seed)
    R = lambda *s: torch.randn(*s, generator=gen)
    g = GaussianModel(0, config=None, device="cpu")
    g._xyz, g._features_dc, g._features_rest = R(P, 3), R(P, 1, 3), torch.empty(P, 0, 3)
    g._scaling, g._rotation, g._opacity = R(P, 1 if isotropic else 3), R(P, 4), R(P, 1)
    g.isotropic = isotropic
    g.dygs = torch.rand(P, generator=gen) < (0.4 if dynamic else 0.0)
    if dynamic:
        g.deform = DeformModel(K=3, node_num=nodes, device="cpu")
        g.deform.deform.init(g.get_dygs_xyz)                       # fewer points than the node budget or farthest-point sampling: both fine
        with torch.no_grad():
            g.deform.deform._node_weight.copy_(R(g.deform.deform.node_num, 1))
        g.deform_init = True
        g.time_interval = 1 / 7
    return g


def _slam(dynamic, n_frames=7, **kw):
    g = _model(dynamic, **kw)
    gen = torch.Generator().manual_seed(5)
    cams = {}
    projection = torch.randn(4, 4, generator=gen)                 # one sensor: every frame shares it
    for k in range(n_frames):
        q = torch.randn(4, generator=gen)
        w, x, y, z = (q / q.norm()).tolist()
        Rm = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                           [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        kf = k % 3 == 0
        t = k / (n_frames - 1)
        cams[k] = types.SimpleNamespace(uid=k, R=Rm, T=torch.randn(3, generator=gen), R_gt=Rm.clone(), T_gt=torch.randn(3, generator=gen), time=t,
                                        fid=torch.tensor([t], dtype=torch.float32),
                                        exposure_a=torch.randn(1, generator=gen) if kf else None, exposure_b=torch.randn(1, generator=gen) if kf else None,
                                        fx=301.25, fy=299.1, cx=80.3, cy=59.9, FoVx=0.52359877559829887, FoVy=0.4, image_height=120, image_width=160,
                                        projection_matrix=projection)
    return types.SimpleNamespace(gaussians=g, frontend=types.SimpleNamespace(cameras=cams, kf_indices=[0, 3, 6]), background=torch.tensor([1.0, 0.5, 0.25]),
                                 pipeline_params=types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False))


def _assert_same_map(slam, loaded):
    g, h = slam.gaussians, loaded.gaussians
    for name in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity", "dygs", "motion_mask"):
        a, b = getattr(g, name), getattr(h, name)
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.detach(), b.detach()), name
    assert h.isotropic == g.isotropic and h.deform_init == g.deform_init and h.time_interval == g.time_interval
    assert h.max_sh_degree == g.max_sh_degree and h.active_sh_degree == g.active_sh_degree
    assert torch.equal(loaded.background, slam.background) and vars(loaded.pipeline_params) == vars(slam.pipeline_params)
    assert loaded.kf_indices == list(slam.frontend.kf_indices) and sorted(loaded.cameras) == sorted(slam.frontend.cameras)
    for uid, c in slam.frontend.cameras.items():
        d = loaded.cameras[uid]
        for name in ("R", "T", "R_gt", "T_gt", "fid", "projection_matrix"):
            assert torch.equal(getattr(c, name), getattr(d, name)) and getattr(d, name).dtype == torch.float32, (uid, name)
        for name in ("exposure_a", "exposure_b"):
            assert (getattr(c, name) is None) == (getattr(d, name) is None), (uid, name)
            assert getattr(c, name) is None or torch.equal(getattr(c, name), getattr(d, name)), (uid, name)
        for name in ("uid", "time", "fx", "fy", "cx", "cy", "FoVx", "FoVy", "image_height", "image_width"):
            assert getattr(c, name) == getattr(d, name) and type(getattr(c, name)) is type(getattr(d, name)), (uid, name)


def test_static_map_round_trips_exactly(tmp_path):
    from slam.map_io import load_map, save_map
    slam = _slam(False, isotropic=True)
    d = save_map(slam, str(tmp_path / "map"))
    assert sorted(os.listdir(d)) == ["map.json", "map_state.npz", "point_cloud"]                 # no deform/ files for a static map
    loaded = load_map(d, "cpu")
    _assert_same_map(slam, loaded)
    assert loaded.gaussians.deform is None and not loaded.dynamic
    assert loaded.deltas_for(loaded.cameras[0]) == (None, None, None)
    meta = json.load(open(os.path.join(d, "map.json")))
    assert meta["format_version"] == 1 and meta["gaussians"] == 57 and meta["width"] == 160 and meta["fx"] == 301.25 and meta["nodes"] is None


def test_dynamic_map_round_trips_exactly_into_a_fresh_model(tmp_path):
    from slam.map_io import load_map, save_map
    slam = _slam(True)
    live = slam.gaussians.deform.deform
    d = save_map(slam, str(tmp_path / "map"))
    assert os.path.isfile(os.path.join(d, "deform", "iteration_0", "deform.pth"))
    loaded = load_map(d, "cpu")
    _assert_same_map(slam, loaded)
    got = loaded.gaussians.deform.deform
    assert got is not live and got.inited and got.node_num == live.node_num > 0
    a, b = live.state_dict(), got.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for (n, p), (m, q) in zip(live.named_parameters(), got.named_parameters()):
        assert n == m and torch.equal(p, q) and q.requires_grad == p.requires_grad
    meta = json.load(open(os.path.join(d, "map.json")))
    assert meta["nodes"] == {"K": 3, "node_num": 23, "d_rot_as_res": True, "local_frame": True, "D": 8, "W": 256, "multires": 10, "t_multires": 10}
    assert meta["deform_init"] is True and loaded.gaussians.time_interval == 1 / 7


def test_load_weights_resizes_the_node_tensors_of_a_fresh_model_and_takes_the_highest_iteration(tmp_path):
    from slam.deform_model import DeformModel
    src = _model(True).deform
    src.save_weights(str(tmp_path), 3)
    with torch.no_grad():
        src.deform._node_radius.add_(1.0)
    src.save_weights(str(tmp_path), 12)
    fresh = DeformModel(K=3, node_num=23, device="cpu")
    assert fresh.deform.nodes.shape == (0, 3) and fresh.deform._node_radius.shape == (0,) and not fresh.deform.inited
    path = fresh.load_weights(str(tmp_path))
    assert path.endswith(os.path.join("deform", "iteration_12", "deform.pth")) and fresh.deform.inited and fresh.optimizer is None
    assert fresh.deform.nodes.shape == src.deform.nodes.shape and torch.equal(fresh.deform._node_radius, src.deform._node_radius)
    fresh.load_weights(str(tmp_path), 3)
    assert torch.equal(fresh.deform._node_radius + 1.0, src.deform._node_radius)
    fresh.train_setting()                                          # the loaded tensors can be trained again
    assert [g["name"] for g in fresh.optimizer.param_groups] == ["deform", "nodes"]
    with pytest.raises(FileNotFoundError, match="iteration_7"):
        fresh.load_weights(str(tmp_path), 7)
    with pytest.raises(FileNotFoundError, match="no iteration_<N> directory"):
        fresh.load_weights(str(tmp_path / "nowhere"))


def test_load_weights_refuses_missing_extra_and_misshapen_entries_by_name(tmp_path):
    from slam.deform_model import DeformModel, weights_path
    src = _model(True).deform
    good = {k: v.clone() for k, v in src.deform.state_dict().items()}
    path = weights_path(str(tmp_path), 0)
    os.makedirs(os.path.dirname(path))

    def attempt(sd):
        torch.save(sd, path)
        DeformModel(K=3, node_num=23, device="cpu").load_weights(str(tmp_path), 0)

    attempt(good)
    with pytest.raises(KeyError, match=r"deform\.pth lacks 'network\.linear\.3\.bias'"):
        attempt({k: v for k, v in good.items() if k != "network.linear.3.bias"})
    with pytest.raises(KeyError, match=r"deform\.pth has an entry 'network\.surprise\.weight' that the rename table"):
        attempt({**good, "network.surprise.weight": torch.zeros(2)})
    with pytest.raises(ValueError, match=r"deform\.pth entry 'network\.gaussian_warp\.weight' has shape \(3, 255\), expected \(3, 256\)"):
        attempt({**good, "network.gaussian_warp.weight": torch.zeros(3, 255)})
    with pytest.raises(ValueError, match=r"deform\.pth entry '_node_radius' has shape \(5,\), expected \(\d+,\)"):
        attempt({**good, "_node_radius": torch.zeros(5)})
    with pytest.raises(KeyError, match=r"lacks 'nodes'"):
        attempt({k: v for k, v in good.items() if k != "nodes"})
    torch.save([1, 2], path)
    with pytest.raises(ValueError, match="expected a state_dict, got list"):
        DeformModel(K=3, node_num=23, device="cpu").load_weights(str(tmp_path), 0)


def test_reference_state_dict_names_load_through_the_rename_table(tmp_path):
    """The names and shapes the reference's ControlNodeWarp.state_dict() has (recorded by tests/golden/make_reference_deform_state.py; no
    file written by the reference exists to test with), filled with seeded values, load into a fresh model; a name outside the table raises."""
    from slam.deform_model import REFERENCE_NAMES, DeformModel, rename_reference_entries, weights_path
    fixture = json.load(open(os.path.join(REPO, "tests", "golden", "reference_deform_state.json")))
    for case, node_num in (("shipped", 512), ("shipped_64_nodes", 64)):
        entries = fixture[case]["entries"]
        assert ["inited", [], "bool"] in entries and len(entries) == 28
        gen = torch.Generator().manual_seed(1)
        sd = {name: (torch.tensor(True) if dtype == "bool" else torch.randn(*shape, generator=gen)) for name, shape, dtype in entries}
        path = weights_path(str(tmp_path / case), 40)
        os.makedirs(os.path.dirname(path))
        torch.save(sd, path)
        m = DeformModel(K=3, node_num=node_num, device="cpu")
        m.load_weights(str(tmp_path / case))
        mine = m.deform.state_dict()
        assert set(mine) == set(sd) - {"inited"} and m.deform.inited and m.deform.node_num == node_num
        for k, v in mine.items():
            assert torch.equal(v, sd[k]), k
    renamed = rename_reference_entries({"network.color_hash_encoding.params": 0, "inited": 1, "nodes": 2}, "x")
    assert renamed == {"nodes": 2}
    with pytest.raises(KeyError, match="'nodes_extra'.*rename table"):
        rename_reference_entries({"nodes_extra": 0}, "x")
    with pytest.raises(KeyError, match="'network.timenet.0.weight'"):
        rename_reference_entries({"network.timenet.0.weight": 0}, "x")
    assert all(isinstance(a, str) and (b is None or isinstance(b, str)) for a, b in REFERENCE_NAMES)


def test_load_map_refusals_name_the_file_and_the_field(tmp_path):
    from slam.map_io import load_map, save_map
    import shutil
    d = save_map(_slam(True), str(tmp_path / "map"))

    def copy(name):
        c = str(tmp_path / name)
        shutil.copytree(d, c)
        return c

    c = copy("no_json")
    os.remove(os.path.join(c, "map.json"))
    with pytest.raises(FileNotFoundError, match=r"no_json.map\.json: no such file"):
        load_map(c, "cpu")
    c = copy("version")
    meta = json.load(open(os.path.join(c, "map.json")))
    json.dump({**meta, "format_version": 99}, open(os.path.join(c, "map.json"), "w"))
    with pytest.raises(ValueError, match=r"version.map\.json: format_version is 99, this build reads version 1"):
        load_map(c, "cpu")
    c = copy("field")
    json.dump({k: v for k, v in meta.items() if k != "isotropic"}, open(os.path.join(c, "map.json"), "w"))
    with pytest.raises(KeyError, match=r"map\.json: field 'isotropic' is missing"):
        load_map(c, "cpu")
    for missing in ("map_state.npz", os.path.join("point_cloud", "final", "point_cloud.ply"), os.path.join("deform", "iteration_0", "deform.pth")):
        c = copy("missing_" + os.path.basename(missing))
        os.remove(os.path.join(c, missing))
        with pytest.raises(FileNotFoundError, match=os.path.basename(missing).replace(".", r"\.")):
            load_map(c, "cpu")
    c = copy("count")
    other = _slam(True, P=58)
    other.gaussians.save_ply(os.path.join(c, "point_cloud", "final", "point_cloud.ply"))
    with pytest.raises(ValueError, match=r"point_cloud\.ply holds 58 Gaussians, but field 'gaussians' of .*map_state\.npz says 57"):
        load_map(c, "cpu")
    c = copy("state_field")
    st = dict(np.load(os.path.join(c, "map_state.npz")))
    st.pop("frame_exposure_a")
    np.savez(os.path.join(c, "map_state.npz"), **st)
    with pytest.raises(KeyError, match=r"map_state\.npz: field 'frame_exposure_a' is missing"):
        load_map(c, "cpu")
    c = copy("dyn_count")
    st = dict(np.load(os.path.join(c, "map_state.npz")))
    st["motion_mask"] = st["motion_mask"][:-1]
    np.savez(os.path.join(c, "map_state.npz"), **st)
    with pytest.raises(ValueError, match=r"map_state\.npz: field 'motion_mask' has shape"):
        load_map(c, "cpu")


def test_slam_save_map_needs_a_directory():
    from slam.system import SLAM
    stub = types.SimpleNamespace(save_dir=None)
    with pytest.raises(ValueError, match="no directory given"):
        SLAM.save_map(stub)
