"""Host side of the plane sweep (include/multiview_depth.h): what the numpy restatement (tests/sweep_reference.py) does on the planted
scene, the front-end's merge rule and noise draw order with the option on, and the parsing of ``Training.mono_sweep``. No GPU."""
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sweep_reference as ref  # noqa: E402

_planted = {}


def _swept(seed):
    """(result of the restatement, truth) on the planted scene with partners right + down: computed once per seed, shared, read-only."""
    if seed not in _planted:
        grey, partners, transforms, truth = ref.planted_scene(("right", "down"), seed=seed)
        out = ref.sweep(grey, partners, ref.PLANTED_K, transforms, ref.PLANTED_W_MIN, ref.PLANTED_W_STEP, **ref.DEFAULTS)
        for a in out.values():
            a.setflags(write=False)
        _planted[seed] = (out, truth, (grey, partners, transforms))
    return _planted[seed]


# ---- the restatement on the planted scene --------------------------------------------------------------------------------------------
def test_planted_geometry_is_what_the_scene_says():
    """A shift of s pixels is hypothesis 2 s: the right partner sees pixel (u, v) of the background at (u - 5, v), the down partner at
    (u, v - 5), and two neighbouring hypotheses share a pixel."""
    vis, xq, yq, _, _, front = ref.project(48, 112, ref.PLANTED_K, ref.planted_transform("right"), 0.0, 1.0 / 32.0)
    assert vis[20, 60].all() and list(xq[20, 60, [0, 10, 11, 40, 63]]) == [60, 55, 55, 40, 29] and (yq[20, 60] == 20).all()
    assert list(vis[20, 3, :9]) == [True] * 8 + [False] and not vis[20, 3, 8:].any()          # u - k / 2 >= -0.5 up to k = 7
    vis, xq, yq, _, _, front = ref.project(48, 112, ref.PLANTED_K, ref.planted_transform("down"), 0.0, 1.0 / 32.0)
    assert list(yq[30, 60, [0, 10, 40]]) == [30, 25, 10] and (xq[30, 60][vis[30, 60]] == 60).all() and not vis[30, 60, 62:].any()
    assert front.all()                                                                        # a sideways partner has every hypothesis in front of it


@pytest.mark.parametrize("seed", [0, 1])
def test_wrong_depths_are_rare_on_the_planted_scene(seed):
    """Of the valid pixels at most 2 % are more than 2 hypotheses (1 px) from the truth, occluded pixels included. The restatement gives
    0.0048 (seed 0) and 0.0028 (seed 1)."""
    out, truth, _ = _swept(seed)
    share, bad = ref.quality(out["index16"], truth)
    print("seed", seed, "valid share", share, "bad share", bad)
    assert bad <= 0.02


@pytest.mark.parametrize("seed,share_is,bad_is", [(0, 0.580, 0.0048), (1, 0.596, 0.0028)])
def test_half_the_planted_scene_is_valid(seed, share_is, bad_is):
    """At least half of all pixels are valid. The restatement gives 0.580 (seed 0) and 0.596 (seed 1), with 0.0048 and 0.0028 of them wrong:
    the figures of the prototype the two conditions were read from, to the digits they were given with. Every pixel of this scene is
    observable (the swept range moves it 31.5 px in both partners)."""
    out, truth, _ = _swept(seed)
    share, bad = ref.quality(out["index16"], truth)
    print("seed", seed, "valid share", share, "bad share", bad, "observable share", float(out["observable"].mean()))
    assert share >= 0.5
    assert abs(share - share_is) < 5e-4 and abs(bad - bad_is) < 5e-5 and out["observable"].all()


def test_observability_asks_for_both_ends_in_front_and_the_span():
    """Hypotheses 0 and 63 in front of one partner and at least min_span_px apart there, whether or not they fall inside its image: in the
    planted scene the span is 31.5 px everywhere, so 31 passes and 32 does not; a partner turned away observes nothing; one of two is enough."""
    _, _, (grey, partners, transforms) = _swept(0)
    args = (ref.PLANTED_K, transforms, ref.PLANTED_W_MIN, ref.PLANTED_W_STEP)
    assert ref.cost_volume(grey, partners, *args, 31)[1].all() and not ref.cost_volume(grey, partners, *args, 32)[1].any()
    away = np.array([-1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, -1, -0.5], np.float32)                      # turned round: X_2 < 0 for every ray
    K = ref.PLANTED_K
    assert not ref.cost_volume(grey, partners[:1], K, away[None], 0.0, 1.0 / 32.0, 0)[1].any()
    assert ref.cost_volume(grey, partners, K, np.stack([away, transforms[1]]), 0.0, 1.0 / 32.0, 8)[1].all()
    # a pixel whose nearest hypothesis leaves both images is observable all the same: the rule is about parallax, not about the image borders
    vis = ref.project(48, 112, K, transforms[0], 0.0, 1.0 / 32.0)[0]
    assert not vis[0, 0, 63] and ref.cost_volume(grey, partners[:1], K, transforms[:1], 0.0, 1.0 / 32.0, 8)[1][0, 0]


def test_aggregation_does_the_work():
    out, truth, (grey, partners, transforms) = _swept(0)
    raw = ref.sweep(grey, partners, ref.PLANTED_K, transforms, ref.PLANTED_W_MIN, ref.PLANTED_W_STEP, aggregated=False, **ref.DEFAULTS)
    (share, bad), (share_raw, bad_raw) = ref.quality(out["index16"], truth), ref.quality(raw["index16"], truth)
    assert share > 1.3 * share_raw and bad < 0.25 * bad_raw
    assert int(out["cost"].max()) <= 2 * 62 and int(out["cost_sum"].max()) <= 8 * (2 * 62 + ref.DEFAULTS["p2"])


def test_depth_is_the_inverse_of_the_swept_inverse_depth():
    out, _, _ = _swept(0)
    valid = out["index16"] >= 0
    assert np.array_equal(out["depth"] == 0, ~valid) and (out["index16"][~valid] == -16).all()
    w = out["index16"][valid].astype(np.float64) / 16.0 / 32.0
    np.testing.assert_allclose(out["depth"][valid], 1.0 / w, rtol=3e-7)
    k = out["index16"][valid] / 16.0
    assert k.min() > 0.5 and k.max() < 62.5                                                   # hypotheses 0 and 63 are never an answer


# ---- the front-end --------------------------------------------------------------------------------------------------------------------
def _config(mono_sweep=None):
    training = {"monocular": True, "kf_translation": 0.08, "kf_min_translation": 0.05, "kf_overlap": 0.9, "kf_cutoff": 0.3, "window_size": 4,
                "rgb_boundary_threshold": 0.01}
    if mono_sweep is not None:
        training["mono_sweep"] = mono_sweep
    return {"Training": training, "Results": {}, "model_params": {"dynamic_model": False}}


def _frontend(monkeypatch, mono_sweep, n_valid=50, H=6, W=8):
    """A FrontEnd on the CPU whose device calls are doubles: mono_keyframe_depth returns 3 + noise and a stats word triple, the sweep
    returns depth 7 with a checkerboard of valid pixels."""
    from slam import frontend
    from slam.pretrained import EventLog
    fe = frontend.FrontEnd(_config(mono_sweep))
    fe.backend = types.SimpleNamespace(gaussians=types.SimpleNamespace(generator=torch.Generator().manual_seed(5)))
    seen = {}

    def mono_keyframe_depth(depth, opacity, gt_img, threshold, noise):
        seen["noise"] = noise.clone()
        stats = torch.tensor(struct.unpack("<3i", struct.pack("<ffi", 2.5, 0.1, n_valid)), dtype=torch.int32).view(torch.float32)
        return 3.0 + noise, stats

    def sweep(ref_image, partner_images, K, transforms, w_min, w_step, stream=None):
        seen["sweep"] = dict(partners=len(partner_images), K=K, transforms=transforms, w_min=w_min, w_step=w_step)
        valid = (torch.arange(H)[:, None] + torch.arange(W)[None, :]) % 2 == 0
        return {"depth": torch.where(valid, 7.0, 0.0), "index16": torch.where(valid, 160, -16).to(torch.int16), "valid": valid}

    monkeypatch.setattr(frontend.kf, "mono_keyframe_depth", mono_keyframe_depth)
    if fe.mono_sweep is not None:
        relative_transforms = lambda newest, partners: ("transforms of", newest.uid, [c.uid for c in partners])
        fe.mono_sweep.sweeper, fe.mono_sweep.log = types.SimpleNamespace(sweep=sweep, relative_transforms=relative_transforms), EventLog("cpu")
    image = torch.full((3, H, W), 0.5)
    image[:, 0, :] = 0.0                                                                       # the first row fails the RGB boundary threshold
    cam = lambda uid, img=image: types.SimpleNamespace(uid=uid, original_image=img, fx=8.0, fy=9.0, cx=4.0, cy=3.0)
    fe.cameras = {k: cam(k) for k in (9, 7, 4, 2, 0)}
    fe.cameras[4].original_image = None                                                        # a keyframe whose image is gone is no partner
    fe.current_window, fe.reset = [9, 7, 4, 2, 0], False
    return fe, seen, image


def test_merge_takes_the_sweep_where_valid_and_coloured_and_keeps_the_noise_draws(monkeypatch):
    off, seen_off, image = _frontend(monkeypatch, None)
    rendered = torch.ones(6, 8)
    seed_off = off._monocular_seed_depth(image, rendered, rendered)
    on, seen_on, _ = _frontend(monkeypatch, {"enabled": True, "near": 0.5})
    seed_on = on._monocular_seed_depth(image, rendered, rendered)
    # the same draws from the model's generator, in the same order, and nothing drawn on top
    assert torch.equal(seen_on["noise"], seen_off["noise"])
    assert torch.equal(on.backend.gaussians.generator.get_state(), off.backend.gaussians.generator.get_state())
    assert torch.equal(seed_off, 3.0 + seen_off["noise"]) and "sweep" not in seen_off
    # the merge: the sweep's depth on the valid checkerboard, except in the dark first row; the fallback everywhere else, bit for bit
    valid = (torch.arange(6)[:, None] + torch.arange(8)[None, :]) % 2 == 0
    use = valid.clone()
    use[0] = False
    assert torch.equal(seed_on[use], torch.full((int(use.sum()),), 7.0)) and torch.equal(seed_on[~use], seed_off[~use]) and use.sum() == 20
    # the call: the three newest window keyframes after the new one that still hold an image, w from the fallback's median
    call = seen_on["sweep"]
    assert call["partners"] == 2 and call["transforms"] == ("transforms of", 9, [7, 2]) and call["K"] == (8.0, 9.0, 4.0, 3.0)
    assert call["w_min"] == 0.0 and call["w_step"] == pytest.approx(1.0 / (0.5 * 2.5 * 63.0), rel=1e-12)
    assert not on.reset and len(on.mono_sweep.shares) == 1 and float(on.mono_sweep.shares[0]) == 0.5


def test_reset_rule_and_first_keyframe_are_unchanged_with_the_option_on(monkeypatch):
    on, seen, image = _frontend(monkeypatch, {"enabled": True}, n_valid=1)
    rendered = torch.ones(6, 8)
    seed = on._monocular_seed_depth(image, rendered, rendered)
    assert on.reset and "sweep" not in seen and torch.equal(seed, 3.0 + seen["noise"])         # fewer than two valid pixels: no sweep, a reset
    on, seen, image = _frontend(monkeypatch, {"enabled": True})
    off, _, _ = _frontend(monkeypatch, None)
    first_on, first_off = on._monocular_seed_depth(image, None, None), off._monocular_seed_depth(image, None, None)
    assert torch.equal(first_on, first_off) and "sweep" not in seen and "noise" not in seen      # the first keyframe has nothing to sweep against
    assert on.mono_sweep.summary() == {"keyframes": 0, "valid_share": 0.0, "device_ms_per_keyframe": 0.0} and off.mono_sweep is None


def test_merge_rule():
    from slam.stages import merge_sweep_depth
    image = torch.tensor([[[0.2, 0.0, 0.2, 0.004]]]).repeat(3, 1, 1)                              # channel sums 0.6, 0, 0.6, 0.012
    got = merge_sweep_depth(torch.tensor([[5.0, 5.0, 0.0, 5.0]]), torch.tensor([[True, True, False, True]]), image, 0.01,
                            torch.tensor([[1.0, 2.0, 3.0, 4.0]]))
    assert got.tolist() == [[5.0, 2.0, 3.0, 5.0]]


# ---- configuration ---------------------------------------------------------------------------------------------------------------------
def test_mono_sweep_block_parses_with_defaults_and_is_off_unless_enabled(tmp_path):
    from slam.frontend import FrontEnd
    from slam.stages import mono_sweep_options
    from slam.system import default_config
    assert "mono_sweep" not in default_config()["Training"]
    for training in ({}, {"mono_sweep": {}}, {"mono_sweep": {"enabled": False, "partners": 2}}, {"mono_sweep": None}):
        assert mono_sweep_options(training) is None
    assert FrontEnd(_config()).mono_sweep is None
    assert mono_sweep_options({"mono_sweep": {"enabled": True}}) == {"enabled": True, "partners": 3, "near": 0.25, "p1": 10, "p2": 120,
                                                                     "uniqueness_ratio": 40, "min_span_px": 8}
    got = FrontEnd(_config({"enabled": True, "partners": 4, "near": 0.5, "p1": 7, "p2": 90, "uniqueness_ratio": 15, "min_span_px": 3})).mono_sweep.options
    assert got == {"enabled": True, "partners": 4, "near": 0.5, "p1": 7, "p2": 90, "uniqueness_ratio": 15, "min_span_px": 3}
    for block, text in (({"partners": 5}, "partners must be 1 to 4"), ({"partners": 0}, "partners must be 1 to 4"), ({"near": 0.0}, "near must be"),
                        ({"p1": 120}, "0 < p1 < p2"), ({"uniqueness_ratio": 100}, "uniqueness_ratio"), ({"min_span_px": -1}, "min_span_px"),
                        ({"hypotheses": 128}, "unknown keys \\['hypotheses'\\]")):
        with pytest.raises(ValueError, match=text):
            mono_sweep_options({"mono_sweep": dict(block, enabled=True)})
    # the YAML key
    from slam.config import load_config
    path = tmp_path / "mono.yaml"
    path.write_text("Dataset:\n  sensor_type: monocular\nTraining:\n  mono_sweep:\n    enabled: true\n    partners: 2\n")
    cfg = load_config(str(path))
    assert mono_sweep_options(cfg["Training"])["partners"] == 2 and cfg["Training"]["kf_interval"] == 5
