"""Host-side checks of the RAFT optical-flow estimator (slam/optical_flow.py): its parameter table against the reference's state_dict
(tests/golden/golden_raft.npz), checkpoint loading and its errors, InputPadder's amounts, the minimum size, and that a recorded dataset
without an estimator has no gt_flow. No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_raft.npz"))


def _golden_shapes(z):
    return {str(k): tuple(int(v) for v in str(s).split(",") if v) for k, s in zip(z["keys"], z["shapes"])}


def test_parameter_table_equals_reference_state_dict(golden):
    from slam.optical_flow import param_shapes
    want = _golden_shapes(golden)
    got = param_shapes()
    assert len(got) == len(want) == 179
    assert list(got) == [str(k) for k in golden["keys"]]          # the same names in the same order
    assert dict(got) == want
    assert sum(int(np.prod(s)) for s in got.values()) == 5261329


def test_recipe_weights_follow_the_recipe():
    import zlib
    from slam.optical_flow import recipe_state_dict
    sd = recipe_state_dict(0)
    w = sd["update_block.gru.convz1.weight"]
    assert float(w.abs().max()) <= np.sqrt(1.0 / (384 * 5)) and w.dtype == torch.float32
    rng = np.random.default_rng([0, zlib.crc32(b"cnet.norm1.running_var")])
    assert np.array_equal(sd["cnet.norm1.running_var"].numpy(), rng.uniform(0.5, 1.5, (64,)).astype(np.float32))
    assert 0.8 <= float(sd["cnet.layer2.0.norm3.weight"].min()) and float(sd["cnet.layer2.0.norm3.weight"].max()) <= 1.2
    assert int(sd["cnet.norm1.num_batches_tracked"]) == 0
    assert not torch.equal(sd["fnet.conv1.bias"], recipe_state_dict(1)["fnet.conv1.bias"])


def test_checkpoint_prefix_and_errors(tmp_path):
    from slam.optical_flow import check_state_dict, recipe_state_dict
    sd = recipe_state_dict(0)
    wrapped = {"module." + k: v for k, v in sd.items()}
    assert list(check_state_dict(wrapped)) == list(sd)
    missing = dict(sd)
    del missing["update_block.mask.2.bias"]
    with pytest.raises(KeyError, match="update_block.mask.2.bias"):
        check_state_dict(missing)
    extra = dict(sd, **{"fnet.extra.weight": torch.zeros(3)})
    with pytest.raises(KeyError, match="fnet.extra.weight"):
        check_state_dict(extra)
    bad = dict(sd, **{"cnet.layer3.0.downsample.0.weight": torch.zeros(128, 96, 3, 3)})
    with pytest.raises(ValueError, match="cnet.layer3.0.downsample.0.weight"):
        check_state_dict(bad)
    small = dict(sd, **{"update_block.encoder.convc1.weight": torch.zeros(96, 196, 1, 1)})
    with pytest.raises(ValueError, match="RAFT-small"):
        check_state_dict(small)
    # a checkpoint on disk, as DataParallel saves it, loads through torch.load(weights_only=True) on the host
    path = tmp_path / "raft-things.pth"
    torch.save(wrapped, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    assert torch.equal(check_state_dict(loaded)["fnet.conv1.weight"], sd["fnet.conv1.weight"])


def test_padding_equals_input_padder(golden):
    from slam.optical_flow import pad_amounts
    for (h, w), ref in zip(golden["pad_sizes"], golden["pad_amounts"]):
        assert list(pad_amounts(int(h), int(w))) == [int(v) for v in ref], (h, w)


@pytest.mark.parametrize("h,w", [(104, 144), (120, 160), (119, 640), (480, 120), (64, 64)])
def test_too_small_sizes_raise(h, w):
    from slam.optical_flow import check_size
    with pytest.raises(ValueError, match="at least 128x128"):
        check_size(h, w)


@pytest.mark.parametrize("h,w", [(128, 128), (127, 640), (121, 170), (130, 170), (480, 640)])
def test_large_enough_sizes_pass(h, w):
    from slam.optical_flow import check_size
    hp, wp = check_size(h, w)
    assert hp % 8 == 0 and wp % 8 == 0 and (hp >> 6) >= 2 and (wp >> 6) >= 2


def test_recorded_dataset_without_flow_has_no_gt_flow():
    import inspect
    from slam.recorded import CoFusionDataset, RecordedRGBDDataset, TUMDataset, load_dataset
    for f in (RecordedRGBDDataset.__init__, TUMDataset.__init__, CoFusionDataset.__init__, load_dataset):
        assert inspect.signature(f).parameters["flow"].default is None
    # gt_flow is an attribute of an instance given an estimator, never of the class: without one hasattr() stays False
    assert not hasattr(RecordedRGBDDataset, "gt_flow") and not hasattr(TUMDataset, "gt_flow")
    ds = RecordedRGBDDataset.__new__(RecordedRGBDDataset)
    assert not hasattr(ds, "gt_flow")


def test_run_slam_ignores_raft_weights_without_dynamic(tmp_path, monkeypatch):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import run_slam
    seen = {}

    def stop(config, *a, **kw):
        seen["flow"] = kw.get("flow")
        raise SystemExit(0)
    monkeypatch.setattr(run_slam, "load_dataset", stop)
    monkeypatch.setattr(run_slam, "load_config", lambda p: {"Dataset": {"dataset_path": "x/y/z"}, "Results": {"save_results": False},
                                                           "Training": {}})
    monkeypatch.setattr(run_slam, "apply_cli_overrides", lambda c, **kw: c)
    with pytest.warns(UserWarning, match="raft-weights"):
        with pytest.raises(SystemExit):
            run_slam.main(["--config", "c.yaml", "--raft-weights", str(tmp_path / "none.pth")])
    assert seen["flow"] is None
