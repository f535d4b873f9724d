"""Host-side checks of the GMA optical-flow estimator (slam/optical_flow.py GmaFlow): its parameter table against the reference's
RAFTGMA state_dict (tests/golden/golden_gma.npz), the stand-in weights, checkpoint checking and the RAFT / GMA mix-ups, the attention
memory guard, and tools/run_slam.py's --gma-weights switch. No GPU needed."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GRU = [f"update_block.gru.conv{g}{d}.weight" for d in "12" for g in "zrq"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "golden_gma.npz"))


def test_parameter_table_equals_reference_state_dict(golden):
    from slam.optical_flow import gma_param_shapes, param_shapes
    want = {str(k): tuple(int(v) for v in str(s).split(",") if v) for k, s in zip(golden["keys"], golden["shapes"])}
    got = gma_param_shapes()
    assert len(got) == len(want) == 185
    assert list(got) == [str(k) for k in golden["keys"]]          # the same names in the same order
    assert dict(got) == want
    raft = param_shapes()
    assert [k for k in got if k in raft] == list(raft)             # RAFT's 179 names, in RAFT's order
    assert sorted(k for k in raft if raft[k] != got[k]) == sorted(GRU)
    for k in GRU:
        assert got[k][1] == raft[k][1] + 128 == 512 and got[k][:1] + got[k][2:] == raft[k][:1] + raft[k][2:]
    assert sorted(set(got) - set(raft)) == sorted(["update_block.aggregator.gamma", "update_block.aggregator.to_v.weight", "att.to_qk.weight",
                                                   "att.pos_emb.rel_ind", "att.pos_emb.rel_height.weight", "att.pos_emb.rel_width.weight"])


def test_recipe_is_deterministic_per_seed_and_switches_aggregation_on(golden):
    import zlib
    from slam.optical_flow import GMA_QK_GAIN, gma_recipe_state_dict, recipe_state_dict
    a, b, c = gma_recipe_state_dict(0), gma_recipe_state_dict(0), gma_recipe_state_dict(1)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["att.to_qk.weight"], c["att.to_qk.weight"]) and not torch.equal(a["fnet.conv1.bias"], c["fnet.conv1.bias"])
    g = float(a["update_block.aggregator.gamma"])
    assert 0.5 <= g <= 1.5 and g != 0.0 and float(c["update_block.aggregator.gamma"]) != g
    # the gain is the fixture's, inside 100..150 (below, every attention row is uniform; above, one-hot), on recipe_state_dict's convolution rule
    assert float(golden["qk_gain"]) == GMA_QK_GAIN and 100 <= GMA_QK_GAIN <= 150
    rng = np.random.default_rng([0, zlib.crc32(b"att.to_qk.weight")])
    plain = torch.from_numpy(rng.uniform(-np.sqrt(1 / 128), np.sqrt(1 / 128), (256, 128, 1, 1)).astype(np.float32))
    assert torch.equal(a["att.to_qk.weight"], plain * GMA_QK_GAIN)
    # entries with RAFT's name and shape are RAFT's stand-in values: a per-entry generator
    raft = recipe_state_dict(0)
    assert torch.equal(a["cnet.conv2.weight"], raft["cnet.conv2.weight"]) and a["update_block.gru.convz1.weight"].shape[1] == 512
    assert a["att.pos_emb.rel_ind"].dtype == torch.int64 and int(a["att.pos_emb.rel_ind"][0, 159]) == 318
    for d in ("12", "21"):
        for n in "ab":
            assert 0.3 <= float(golden[f"{n}/{d}/entropy_ratio"]) <= 0.8


def test_check_gma_state_dict_names_what_is_wrong():
    from slam.optical_flow import check_gma_state_dict, gma_recipe_state_dict, recipe_state_dict
    sd = gma_recipe_state_dict(0)
    assert list(check_gma_state_dict(sd)) == list(sd)
    assert list(check_gma_state_dict({"module." + k: v for k, v in sd.items()})) == list(sd)
    missing = dict(sd)
    del missing["att.pos_emb.rel_width.weight"]                    # unused by the network, but part of every GMA checkpoint
    with pytest.raises(KeyError, match="att.pos_emb.rel_width.weight"):
        check_gma_state_dict(missing)
    with pytest.raises(KeyError, match="update_block.aggregator.project.weight"):
        check_gma_state_dict(dict(sd, **{"update_block.aggregator.project.weight": torch.zeros(128, 128, 1, 1)}))
    with pytest.raises(ValueError, match="update_block.gru.convq2.weight"):
        check_gma_state_dict(dict(sd, **{"update_block.gru.convq2.weight": torch.zeros(128, 384, 5, 1)}))
    with pytest.raises(ValueError, match="att.pos_emb.rel_ind"):
        check_gma_state_dict(dict(sd, **{"att.pos_emb.rel_ind": torch.zeros(100, 100, dtype=torch.int64)}))
    for raft in (recipe_state_dict(0), {"module." + k: v for k, v in recipe_state_dict(0).items()}):
        with pytest.raises(ValueError, match=r"RAFT checkpoint.*RaftFlow.*--raft-weights"):
            check_gma_state_dict(raft)


def test_raft_check_rejects_a_gma_checkpoint():
    from slam.optical_flow import RaftFlow, check_state_dict, gma_recipe_state_dict
    with pytest.raises((KeyError, ValueError), match="update_block.aggregator.gamma|att.to_qk.weight"):
        check_state_dict(gma_recipe_state_dict(0))
    with pytest.raises((KeyError, ValueError)):
        RaftFlow(gma_recipe_state_dict(0), "cpu")


def test_attention_memory_guard_raises_before_any_work():
    from slam.optical_flow import GmaFlow, attention_bytes, gma_recipe_state_dict
    assert attention_bytes(480, 640) == 2 * 4800 * 4800 * 4
    assert attention_bytes(130, 170) == 2 * 374 * 374 * 4           # pads to 136 x 176
    assert attention_bytes(130, 170, batch=1) == 374 * 374 * 4
    est = GmaFlow(gma_recipe_state_dict(0), "cpu", max_attention_bytes=attention_bytes(480, 640) - 1)
    assert est.gamma == float(gma_recipe_state_dict(0)["update_block.aggregator.gamma"]) and isinstance(est.gamma, float)
    img = torch.zeros(3, 480, 640)
    with pytest.raises(ValueError, match=r"640x480.*2 x 4800 x 4800.*184320000.*184319999"):
        est.pair(img, img)
    assert est.encoder_runs == 0 and est.pairs == 0
    assert GmaFlow(gma_recipe_state_dict(0), "cpu").max_attention_bytes == 2 << 30
    GmaFlow(gma_recipe_state_dict(0), "cpu", max_attention_bytes=attention_bytes(480, 640))._admit(480, 640)   # at the limit: admitted


def test_run_slam_rejects_both_checkpoints(tmp_path, capsys):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import run_slam
    with pytest.raises(SystemExit) as e:
        run_slam.main(["--config", "c.yaml", "--dynamic", "--raft-weights", str(tmp_path / "r.pth"), "--gma-weights", str(tmp_path / "g.pth")])
    assert e.value.code == 2                                        # an argparse error
    assert "not allowed with" in capsys.readouterr().err


def test_run_slam_ignores_gma_weights_without_dynamic(tmp_path, monkeypatch):
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
    with pytest.warns(UserWarning, match="gma-weights"):
        with pytest.raises(SystemExit):
            run_slam.main(["--config", "c.yaml", "--gma-weights", str(tmp_path / "none.pth")])
    assert seen["flow"] is None
