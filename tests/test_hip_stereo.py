"""gsr_stereo_depth (include/stereo_depth.h, csrc/gs_stereo.h) against its integer numpy restatement (tests/stereo_reference.py): the
aggregated volume S and disparity16 are equal bit for bit, the depth equals numpy's float32 division bit for bit, at the sizes where the
kernels take another path (odd sizes, W < D, H below the census window, one pixel, two disparities per lane, paths that leave through the
side borders) and at the ends of the parameter ranges."""
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import stereo_reference as ref  # noqa: E402

pytestmark = pytest.mark.gpu

BF = 47.90639384423901
DEV = "cuda:0"


def _random_pair(H, W, seed, shift=9):
    """Random bytes; the upper half of the right image is the left one moved by `shift` (where that fits), so some pixels do match."""
    rng = np.random.default_rng(seed)
    left = rng.integers(0, 256, (H, W), dtype=np.uint8)
    right = rng.integers(0, 256, (H, W), dtype=np.uint8)
    if W > shift:
        right[:H // 2, :W - shift] = left[:H // 2, shift:]
    return left, right


def _planted():
    left, right, _, _ = ref.planted_pair(seed=0)
    return left, right


# name -> (pair, matcher parameters); every name is one parametrised case
CASES = {
    "planted_48x112": (_planted, {}),
    "random_23x97": (lambda: _random_pair(23, 97, 1), {}),
    "random_97x23_W_below_D": (lambda: _random_pair(97, 23, 2), {}),
    "random_5x70_H_below_census": (lambda: _random_pair(5, 70, 3), {}),
    "one_pixel": (lambda: _random_pair(1, 1, 4), {}),
    "random_24x150_D128": (lambda: _random_pair(24, 150, 5, shift=70), {"num_disparities": 128}),
    "constant_9x70": (lambda: (np.full((9, 70), 128, np.uint8),) * 2, {}),
    "p1_1_p2_2047": (_planted, {"p1": 1, "p2": 2047}),
    "p1_10_p2_11": (_planted, {"p1": 10, "p2": 11}),
    "uniqueness_0": (_planted, {"uniqueness_ratio": 0}),
    "uniqueness_99": (_planted, {"uniqueness_ratio": 99}),
    "disp12_off": (_planted, {"disp12_max_diff": -1}),
    "disp12_0": (_planted, {"disp12_max_diff": 0}),
    "planted_D128_p2_2047": (_planted, {"num_disparities": 128, "p2": 2047}),
}
_reference = {}


def _expected(name):
    """(left, right, parameters, disparity16, S) of a case: computed once, shared, read-only."""
    if name not in _reference:
        make, over = CASES[name]
        left, right = make()
        params = dict(ref.DEFAULTS, **over)
        d16, S = ref.match(left, right, **params)
        for a in (left, right, d16, S):
            a.setflags(write=False)
        _reference[name] = (left, right, params, d16, S)
    return _reference[name]


def _run(left, right, params, cost=True, depth=True, image=True, stream=None, **extra):
    from slam import stereo
    H, W = left.shape
    D = params["num_disparities"]
    dev = torch.device(DEV)
    out = {"disparity16": torch.full((H, W), 1234, dtype=torch.int16, device=dev)}
    if cost:
        out["cost_sum"] = torch.full((H, W, D), -1, dtype=torch.int16, device=dev)
    if depth:
        out["depth"] = torch.full((H, W), -7.0, dtype=torch.float32, device=dev)
    if image:
        out["image"] = torch.full((3, H, W), -7.0, dtype=torch.float32, device=dev)
        out["lut"] = torch.tensor((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32), device=dev)
    stereo.stereo_depth(torch.tensor(np.ascontiguousarray(left), device=dev), torch.tensor(np.ascontiguousarray(right), device=dev), bf=BF,
                        stream=stream, **out, **params, **extra)
    (stream or torch.cuda.current_stream(dev)).synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if cost:
        res["cost_sum"] = res["cost_sum"].view(np.uint16)
    return res


def _assert_equal_volume(got, want, name):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        y, x, d = bad[0]
        raise AssertionError(f"{name}: S differs at {len(bad)} of {want.size} entries, first at y {y} x {x} d {d}: {got[y, x, d]} != {want[y, x, d]}; "
                             f"rows touched {np.unique(bad[:, 0])[:8]}, columns {np.unique(bad[:, 1])[:8]}, disparities {np.unique(bad[:, 2])[:8]}")


@pytest.mark.parametrize("name", list(CASES))
def test_volume_disparity_and_depth_equal_the_reference(name):
    left, right, params, d16, S = _expected(name)
    got = _run(left, right, params)
    _assert_equal_volume(got["cost_sum"], S, name)                       # the aggregation ...
    diff = np.argwhere(got["disparity16"] != d16)
    assert len(diff) == 0, (name, len(diff), diff[:5], got["disparity16"][tuple(diff[:5].T)], d16[tuple(diff[:5].T)])      # ... and the selection
    want_depth = ref.depth_from_disparity(d16, BF)
    assert np.array_equal(got["depth"].view(np.uint32), want_depth.view(np.uint32)), name
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    assert np.array_equal(got["image"], np.broadcast_to(lut[left], (3,) + left.shape)), name
    print(name, "valid share", float((d16 >= 0).mean()), "S max", int(S.max()))


def test_optional_outputs_and_repeatability():
    left, right, params, d16, S = _expected("planted_48x112")
    bare = _run(left, right, params, cost=False, depth=False, image=False)
    assert np.array_equal(bare["disparity16"], d16)
    some = _run(left, right, params, cost=False, depth=True, image=False)
    assert np.array_equal(some["disparity16"], d16) and np.array_equal(some["depth"], ref.depth_from_disparity(d16, BF))
    a, b = _run(left, right, params), _run(left, right, params)
    for k in ("disparity16", "cost_sum", "depth", "image"):
        assert a[k].tobytes() == b[k].tobytes(), k
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        c = _run(left, right, params, stream=side)
    for k in ("disparity16", "cost_sum", "depth", "image"):
        assert a[k].tobytes() == c[k].tobytes(), k


def test_matcher_object_keeps_its_workspace():
    from slam import stereo
    left, right, params, d16, _ = _expected("random_23x97")
    m = stereo.StereoMatcher(97, 23, bf=BF, device=DEV, **params)
    l, r = torch.tensor(np.array(left), device=DEV), torch.tensor(np.array(right), device=DEV)
    ws = m._workspace.data_ptr()
    for _ in range(2):
        image, disp, depth = m(l, r)
        assert np.array_equal(disp.cpu().numpy(), d16) and np.array_equal(depth.cpu().numpy(), ref.depth_from_disparity(d16, BF))
        assert image.shape == (3, 23, 97) and image.dtype == torch.float32
    assert m._workspace.data_ptr() == ws and m._workspace.numel() == stereo.stereo_workspace_size(97, 23, 64) > 23 * 97 * 64 * 2
    assert stereo.stereo_workspace_size(97, 23, 96) == 0 and stereo.stereo_workspace_size(0, 23, 64) == 0
    with pytest.raises(ValueError, match="64 or 128"):
        stereo.StereoMatcher(97, 23, num_disparities=96, device=DEV)


def test_rectification_equals_frame_prepare():
    """21 x 33 with distorting maps (taps fall outside the picture along the borders): left_rect / right_rect and image against
    gsr_frame_prepare fed the grey bytes replicated to RGB -- that kernel is pinned to cv2.remap's fixed-point rule -- and the matching
    runs on the rectified bytes."""
    from slam import frame_io, stereo
    H, W = 21, 33
    left, right = _random_pair(H, W, 11, shift=4)
    K = [[30.0, 0, 16.2], [0, 29.0, 10.4], [0, 0, 1]]
    c, s = np.cos(0.02), np.sin(0.02)
    maps_h = (stereo.rectify_map(K, (-0.3, 0.1, 1e-3, -2e-3, 0.0), np.eye(3), [[22.0, 0, 16.2], [0, 22.0, 10.4], [0, 0, 1]], W, H),   # a wider view
              stereo.rectify_map(K, (-0.25, 0.05, 0.0, 1e-3, 0.01), [[c, -s, 0], [s, c, 0], [0, 0, 1]], [[28.0, 0, 16.0], [0, 28.0, 10.0], [0, 0, 1]], W, H))
    dev = torch.device(DEV)
    lut = torch.tensor((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32), device=dev)
    want = []
    for img, m in zip((left, right), maps_h):
        rgb = torch.tensor(np.repeat(img[..., None], 3, -1), device=dev)
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        frame_io.frame_prepare(rgb, torch.tensor(m, device=dev), lut, None, 0.01, out, None)
        want.append(out.cpu().numpy())
    assert np.array_equal(want[0][0], want[0][1]) and np.array_equal(want[0][0], want[0][2])
    rect = torch.full((2, H, W), 77, dtype=torch.uint8, device=dev)
    image = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    disp = torch.empty((H, W), dtype=torch.int16, device=dev)
    stereo.stereo_depth(torch.tensor(left, device=dev), torch.tensor(right, device=dev), disp, image=image, lut=lut,
                        maps=tuple(torch.tensor(m, device=dev) for m in maps_h), left_rect=rect[0], right_rect=rect[1], bf=BF)
    torch.cuda.synchronize()
    lut_h = lut.cpu().numpy()
    rect_h = rect.cpu().numpy()
    assert np.array_equal(image.cpu().numpy(), want[0])
    assert np.array_equal(lut_h[rect_h[0]], want[0][0]) and np.array_equal(lut_h[rect_h[1]], want[1][0])
    outside = (maps_h[0][..., 0] < -1) | (maps_h[0][..., 0] > W) | (maps_h[0][..., 1] < -1) | (maps_h[0][..., 1] > H)
    assert outside.sum() > 50 and np.all(rect_h[0][outside] == 0) and not np.array_equal(rect_h[0], left)      # BORDER_CONSTANT 0 is exercised
    assert np.array_equal(disp.cpu().numpy(), ref.match(rect_h[0], rect_h[1])[0])
    # without maps, rect outputs that are given receive the raw bytes
    rect.fill_(77)
    stereo.stereo_depth(torch.tensor(left, device=dev), torch.tensor(right, device=dev), disp, left_rect=rect[0], right_rect=rect[1], bf=BF)
    torch.cuda.synchronize()
    assert np.array_equal(rect.cpu().numpy(), np.stack([left, right]))


def test_bad_arguments_are_refused_with_text_and_touch_nothing():
    from slam import stereo
    left, right, params, _, _ = _expected("random_23x97")
    H, W = left.shape
    dev = torch.device(DEV)
    l, r = torch.tensor(np.array(left), device=dev), torch.tensor(np.array(right), device=dev)
    disp = torch.full((H, W), 1234, dtype=torch.int16, device=dev)
    depth = torch.full((H, W), -7.0, dtype=torch.float32, device=dev)
    a_map = torch.zeros((H, W, 2), dtype=torch.float32, device=dev)
    rect = torch.zeros((2, H, W), dtype=torch.uint8, device=dev)
    need = stereo.stereo_workspace_size(W, H, 64)
    short = torch.empty(need - 1, dtype=torch.uint8, device=dev)
    image = torch.full((3, H, W), -7.0, dtype=torch.float32, device=dev)
    bad = [({"num_disparities": 96}, "num_disparities 64 or 128 \\(got 96\\)"),
           ({"p1": 120, "p2": 120}, "0 < p1 < p2 <= 2047"),
           ({"p1": 0}, "0 < p1 < p2 <= 2047"),
           ({"p2": 2048}, "0 < p1 < p2 <= 2047"),
           ({"uniqueness_ratio": 100}, "uniqueness_ratio must be in \\[0, 99\\]"),
           ({"uniqueness_ratio": -1}, "uniqueness_ratio must be in \\[0, 99\\]"),
           ({"disp12_max_diff": -2}, "disp12_max_diff must be -1"),
           ({"disparity16": None}, "disparity16 and workspace must not be NULL"),
           ({"maps": (a_map, None), "left_rect": rect[0], "right_rect": rect[1]}, "map_left and map_right go together"),
           ({"maps": (None, a_map), "left_rect": rect[0], "right_rect": rect[1]}, "map_left and map_right go together"),
           ({"maps": (a_map, a_map)}, "left_rect and right_rect must not be NULL when maps are given"),
           ({"image": image}, "image needs lut"),
           ({"workspace": short}, f"hold {need} bytes \\(gsr_stereo_workspace_size\\), got {need - 1}")]
    for over, text in bad:
        kw = dict(disparity16=disp, depth=depth, bf=BF, **params)
        kw.update(over)
        with pytest.raises(RuntimeError, match="gsr_stereo_depth failed \\(code -1\\): gsr_stereo_depth: .*" + text):
            stereo.stereo_depth(l, r, **kw)
    torch.cuda.synchronize()
    assert bool((disp == 1234).all()) and bool((depth == -7.0).all()) and bool((image == -7.0).all()) and not bool(rect.any())
    with pytest.raises(RuntimeError, match="right must be a contiguous torch.uint8 device tensor of shape \\(23, 97\\)"):
        stereo.stereo_depth(l, r[:, :50], disp, bf=BF)
    stereo.stereo_depth(l, r, disp, depth=depth, workspace=torch.empty(need, dtype=torch.uint8, device=dev), bf=BF, **params)      # exactly enough
    torch.cuda.synchronize()
    assert np.array_equal(disp.cpu().numpy(), _expected("random_23x97")[3])
