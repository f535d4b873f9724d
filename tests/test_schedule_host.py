"""Host side of slam/schedule.py and slam/keyframe_slots.py: the packing of a run's schedule table, Adam's coefficient rows and the
candidates' address rows. No GPU."""
import types

import numpy as np
import pytest
import torch

from fused_adam import FusedAdam
from slam import keyframe_slots
from slam.schedule import Schedule, adam_rows, xyz_lr_rule

ROWS = 3
INDEX = [[2, 0], [1, 4000000000], [0, 1]]                                              # (a word above 2^31: stored as uint32)
ADAM = [[0.1 * (j + 1) + 0.01 * k for k in range(4)] for j in range(ROWS)]             # two segments: 4 floats per row
SAMPLES = [[0.5 + 0.125 * j - 0.03 * k for k in range(5)] for j in range(ROWS)]


def _bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("empty", [None, "index", "adam", "samples"])
def test_pack_lays_out_index_words_adam_coefficients_and_samples(empty):
    index, adam, samples = (None if empty == n else b for n, b in (("index", INDEX), ("adam", ADAM), ("samples", SAMPLES)))
    table, coef_lo, samples_lo = Schedule.pack(ROWS, index_words=index, adam=adam, samples=samples)
    n_index, n_adam, n_samples = (0 if b is None else len(b[0]) for b in (index, adam, samples))
    assert table.dtype == np.uint32 and table.shape == (ROWS, n_index + n_adam + n_samples)
    assert (coef_lo, samples_lo) == (n_index, n_index + n_adam)
    for j in range(ROWS):
        want = [np.uint32(w) for w in (index[j] if index else [])] + [_bits(x) for x in (adam[j] if adam else [])]
        want += [_bits(x) for x in (samples[j] if samples else [])]
        assert [int(w) for w in table[j]] == [int(w) for w in want], j


def test_adam_rows_are_the_librarys_coefficients_and_only_xyz_follows_the_schedule():
    rows, count0 = 4, 30
    p_xyz, p_other = torch.zeros(3, requires_grad=True), torch.zeros(2, requires_grad=True)
    opt = FusedAdam([{"params": [p_xyz], "lr": 1.6e-4, "name": "xyz"}, {"params": [p_other], "lr": 2.5e-3, "name": "f_dc", "betas": (0.8, 0.99)}],
                    lr=0.0, eps=1e-15)
    opt.state[p_xyz]["step"], opt.state[p_other]["step"] = torch.tensor(7.0), torch.tensor(0.0)
    todo = [(opt.param_groups[0], p_xyz), (opt.param_groups[1], p_other)]
    rates = {count0 + j: 1.6e-4 * 0.9 ** j for j in range(rows)}
    lr_of = xyz_lr_rule(types.SimpleNamespace(xyz_lr_at=rates.__getitem__), count0)
    got = adam_rows(opt, todo, rows, lr_of)
    assert got.dtype == np.float32 and got.shape == (rows, 4)
    for j in range(rows):
        for k, (group, p) in enumerate(todo):
            lr = rates[count0 + j] if (k == 0 and j > 0) else group["lr"]          # row 0 of xyz: the rate the group holds
            want = FusedAdam.coefficients(lr, group["betas"], int(opt.state[p]["step"]) + j + 1)
            assert [_bits(x) for x in got[j, 2 * k:2 * k + 2]] == [_bits(x) for x in want], (j, k)
    assert _bits(got[0, 0]) == _bits(FusedAdam.coefficients(opt.param_groups[0]["lr"], (0.9, 0.999), 8)[0])
    assert _bits(got[1, 0]) != _bits(FusedAdam.coefficients(opt.param_groups[0]["lr"], (0.9, 0.999), 9)[0])          # (the rule is in force)
    # without lr_of: the constant group["lr"] throughout (initialize_map's runs)
    plain = adam_rows(opt, todo, rows)
    for j in range(rows):
        assert _bits(plain[j, 0]) == _bits(FusedAdam.coefficients(opt.param_groups[0]["lr"], (0.9, 0.999), 8 + j)[0])


def _camera():
    return types.SimpleNamespace(world_view_transform=torch.zeros(4, 4), full_proj_transform=torch.zeros(4, 4), camera_center=torch.zeros(3),
                                 exposure_a=torch.zeros(1), exposure_b=torch.zeros(1))


def test_address_rows_of_plane_views_and_refusal_of_other_layouts():
    H, W = 5, 7
    f6 = torch.zeros(6, H, W)
    cam = _camera()
    planes = (f6[0:3], f6[3:4], f6[4:5], f6[5:6])
    (row,) = keyframe_slots.address_rows([cam], [planes])
    assert row[:5] == [cam.world_view_transform.data_ptr(), cam.full_proj_transform.data_ptr(), cam.camera_center.data_ptr(),
                       cam.exposure_a.data_ptr(), cam.exposure_b.data_ptr()]
    assert row[5:] == [f6.data_ptr() + k * H * W * 4 for k in (0, 3, 4, 5)]
    (entry,) = keyframe_slots.entries([(cam, planes)])                       # a slot's destinations: the same nine addresses, by field
    assert [getattr(entry, name) for name, _ in entry._fields_] == row
    with pytest.raises(RuntimeError):
        keyframe_slots.address_rows([cam], [(f6[0:3], f6[3:4], f6[4:5], torch.zeros(W, H).t()[None])])          # not contiguous
    with pytest.raises(RuntimeError):
        keyframe_slots.address_rows([cam], [(f6[0:3].double(), f6[3:4], f6[4:5], f6[5:6])])                      # float64
    assert keyframe_slots.address_rows([], []) == [] and keyframe_slots.entries([]) is None
