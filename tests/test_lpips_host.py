"""Host-side checks of the LPIPS metric (slam/perceptual.py): the checkpoint loader and its refusals, the fp32 network with the torch
stand-in of the two kernels against the fp64 restatement (tests/lpips_reference.py) on the noise ladder, properties of the restatement
itself, the size rule, and tools/run_slam.py's --lpips-weights. No GPU needed."""
import os
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import perceptual  # noqa: E402
import lpips_reference as ref  # noqa: E402

H, W = 195, 227


@pytest.fixture(scope="module")
def weights():
    return perceptual.recipe_state_dicts(0)


@pytest.fixture(scope="module")
def ladder_scores(weights):
    """The restatement's scores of the ladder, both norm forms: {norm: [3 scores]}."""
    base, noisy = ref.ladder(H, W, seed=0)
    return {norm: [float(ref.lpips(*weights, n, base, norm)) for n in noisy] for norm in ("torchmetrics", "lpips")}


def _save(tmp_path, alex, lin, tag=""):
    a, l = str(tmp_path / f"alexnet{tag}.pth"), str(tmp_path / f"lin{tag}.pth")
    torch.save(dict(alex), a)
    torch.save(dict(lin), l)
    return a, l


def test_tables_and_recipe():
    alex, lin = perceptual.param_shapes()
    assert list(alex) == [f"features.{i}.{n}" for i in (0, 3, 6, 8, 10) for n in ("weight", "bias")]
    assert alex["features.0.weight"] == (64, 3, 11, 11) and alex["features.3.weight"] == (192, 64, 5, 5)
    assert [lin[f"lin{l}.model.1.weight"] for l in range(5)] == [(1, c, 1, 1) for c in (64, 192, 384, 256, 256)]
    a0, l0 = perceptual.recipe_state_dicts(0)
    a1, l1 = perceptual.recipe_state_dicts(0)
    a2, _ = perceptual.recipe_state_dicts(1)
    assert all(torch.equal(a0[k], a1[k]) for k in a0) and all(torch.equal(l0[k], l1[k]) for k in l0)
    assert not torch.equal(a0["features.0.weight"], a2["features.0.weight"])
    assert all(tuple(a0[k].shape) == s for k, s in alex.items()) and all(tuple(l0[k].shape) == s for k, s in lin.items())
    assert all(float(v.min()) >= 0 and float(v.max()) < 0.5 for v in l0.values())


def test_checkpoint_round_trip(tmp_path, weights):
    alex, lin = weights
    full = dict(alex)
    full["classifier.1.weight"] = torch.zeros((8, 8))                  # torchvision's AlexNet has a classifier: ignored
    full["classifier.1.bias"] = torch.zeros(8)
    a, l = _save(tmp_path, full, {"module." + k: v for k, v in lin.items()})          # DataParallel's prefix: stripped
    m = perceptual.Lpips.from_checkpoints(a, l, "cpu")
    assert perceptual.Lpips.from_checkpoints(a, l, "cpu") is m                          # read once per process
    assert perceptual.Lpips.from_checkpoints(a, l, "cpu", norm="lpips") is not m
    assert torch.equal(m.convs[1][0], alex["features.3.weight"]) and torch.equal(m.convs[4][1], alex["features.10.bias"])
    assert all(torch.equal(m.lins[k], lin[f"lin{k}.model.1.weight"].reshape(-1)) for k in range(5))


def test_bad_checkpoints_raise_and_name_the_entry(tmp_path, weights):
    alex, lin = weights
    missing = {k: v for k, v in alex.items() if k != "features.6.bias"}
    with pytest.raises(KeyError, match=r"features\.6\.bias"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, missing, lin, "a"), "cpu")
    shaped = dict(alex, **{"features.8.weight": torch.zeros((256, 384, 5, 5))})
    with pytest.raises(ValueError, match=r"features\.8\.weight.*\(256, 384, 5, 5\)"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, shaped, lin, "b"), "cpu")
    unknown = dict(alex, **{"features.12.weight": torch.zeros(3)})
    with pytest.raises(KeyError, match=r"features\.12\.weight"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, unknown, lin, "c"), "cpu")
    no_lin = {k: v for k, v in lin.items() if k != "lin4.model.1.weight"}
    with pytest.raises(KeyError, match=r"lin4\.model\.1\.weight"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, alex, no_lin, "d"), "cpu")
    extra_lin = dict(lin, **{"net.slice1.0.weight": torch.zeros(3)})
    with pytest.raises(KeyError, match=r"net\.slice1\.0\.weight"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, alex, extra_lin, "e"), "cpu")
    neg = lin["lin2.model.1.weight"].clone()
    neg[0, 17, 0, 0] = -0.25
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight.*negative"):
        perceptual.Lpips.from_checkpoints(*_save(tmp_path, alex, dict(lin, **{"lin2.model.1.weight": neg}), "f"), "cpu")
    torch.save([1, 2, 3], str(tmp_path / "list.pth"))
    with pytest.raises(ValueError, match="state_dict"):
        perceptual.Lpips.from_checkpoints(str(tmp_path / "list.pth"), _save(tmp_path, alex, lin, "g")[1], "cpu")
    with pytest.raises(ValueError, match="norm"):
        perceptual.Lpips(alex, lin, "cpu", norm="l2")


@pytest.mark.parametrize("norm", ["torchmetrics", "lpips"])
def test_fp32_network_on_cpu_against_the_restatement(weights, ladder_scores, norm):
    m = perceptual.Lpips(*weights, device="cpu", norm=norm)
    base, noisy = ref.ladder(H, W, seed=0)
    for n, want in zip(noisy, ladder_scores[norm]):
        got = float(m(n, base)[0])
        print(f"{norm}: fp32 {got:.9g} fp64 {want:.9g} rel {abs(got - want) / want:.3g}")
        assert abs(got - want) <= 1e-4 * want
    # a batch of all three rungs scores as the single pairs do
    scores, taps = m.forward(torch.cat(noisy), base.expand(3, -1, -1, -1), taps=True)
    assert scores.shape == (3,) and taps.shape == (3, 5) and m.pairs == 6
    for got, want in zip(scores.tolist(), ladder_scores[norm]):
        assert abs(got - want) <= 1e-4 * want
    assert m.stats["pairs"] == 6 and m.stats["ms_per_pair"] is None       # no device events on the CPU


def test_properties_of_the_restatement(weights, ladder_scores):
    base, noisy = ref.ladder(H, W, seed=0)
    for norm in ("torchmetrics", "lpips"):
        s = ladder_scores[norm]
        assert float(ref.lpips(*weights, noisy[0], noisy[0], norm)) == 0.0                 # d(x, x) == 0 exactly
        assert float(ref.lpips(*weights, base, noisy[0], norm)) == s[0]                    # d(x, y) == d(y, x)
        assert s[0] > s[1] > s[2] > 0                                                      # the score grows along the ladder
    for a, b in zip(ladder_scores["torchmetrics"], ladder_scores["lpips"]):
        assert abs(a - b) <= 1e-6                                                          # the forms differ at near-zero vectors only
    # all-zero feature vectors (ReLU can produce them): both forms stay finite and count them as equal
    f = torch.rand((2, 8, 3, 3), dtype=torch.float64)
    f[:, :, 1, 1] = 0
    for norm in ("torchmetrics", "lpips"):
        means, score = ref.distance([f], [torch.rand(8, dtype=torch.float64)], norm)
        assert torch.isfinite(score).all() and float(score) > 0


def test_tap_sizes_and_size_rule(weights):
    assert perceptual.tap_sizes(480, 640) == [(119, 159), (59, 79), (29, 39), (29, 39), (29, 39)]
    assert perceptual.tap_sizes(67, 67)[2] == (3, 3)
    x = torch.rand((1, 3, 77, 131))
    assert [tuple(t.shape[1:]) for t in ref.features(weights[0], ref.network_input(x, x))] == \
        [(c, h, w) for c, (h, w) in zip(perceptual.CHANNELS, perceptual.tap_sizes(77, 131))]
    m = perceptual.Lpips(*weights, device="cpu")
    assert m(torch.rand((1, 3, 67, 67)), torch.rand((1, 3, 67, 67))).shape == (1,)
    for h, w in ((66, 200), (200, 66), (32, 32)):
        with pytest.raises(ValueError, match="at least 67"):
            m(torch.zeros((1, 3, h, w)), torch.zeros((1, 3, h, w)))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        m(torch.zeros((3, 100, 100)), torch.zeros((3, 100, 100)))
    with pytest.raises(ValueError, match="one shape"):
        m(torch.zeros((1, 3, 100, 100)), torch.zeros((2, 3, 100, 100)))


def test_run_slam_lpips_flag(tmp_path):
    import run_slam
    args = run_slam.parse_args(["--config", "x.yaml"])
    assert args.lpips_weights is None
    a, l = tmp_path / "alexnet.pth", tmp_path / "lin.pth"
    a.write_bytes(b"")
    l.write_bytes(b"")
    args = run_slam.parse_args(["--config", "x.yaml", "--lpips-weights", str(a), str(l)])
    assert args.lpips_weights == [str(a), str(l)] and not args.eval
    with pytest.raises(SystemExit):
        run_slam.parse_args(["--config", "x.yaml", "--lpips-weights", str(a), str(tmp_path / "missing.pth")])
    with pytest.raises(SystemExit):
        run_slam.parse_args(["--config", "x.yaml", "--lpips-weights", str(a)])              # two paths


def test_eval_rendering_and_slam_take_an_lpips():
    import inspect
    from slam.eval_utils import eval_rendering
    from slam.system import SLAM
    assert inspect.signature(eval_rendering).parameters["lpips"].default is None
    assert inspect.signature(SLAM.__init__).parameters["lpips"].default is None
