"""Host side of slam/schedule.py and slam/keyframe_slots.py: the packing of a run's schedule table, Adam's coefficient rows and the
candidates' address rows; the rule of which iteration densifies or resets opacities and the splitter of the runs between them. No GPU."""
import itertools
import types

import numpy as np
import pytest
import torch

from fused_adam import FusedAdam
from slam import keyframe_slots
from slam.schedule import Schedule, adam_rows, init_rule, mapping_rule, plain_run, xyz_lr_rule

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


# ---- which iteration densifies or resets opacities, and the runs of plain iterations between such ones ------------------------------------
EVERY, RESET, STARTS, LENGTHS, COUNTS = (3, 4, 30, 150), (4, 7, 2001), (0, 1, 5), (1, 10, 50), (0, 41)


def _grid(every):
    """(offset, reset) for one `every`: offsets below, at and above the period (at or above: the densification never comes)."""
    return itertools.product((0, 2, 12, 50, every), RESET)


def _backend(every, offset, reset, iteration_count=0):
    return types.SimpleNamespace(gaussian_update_every=every, gaussian_update_offset=offset, gaussian_reset=reset, iteration_count=iteration_count)


@pytest.mark.parametrize("every", EVERY)
def test_mapping_rule_is_the_two_expressions_and_densify_wins(every):
    for offset, reset in _grid(every):
        be = _backend(every, offset, reset)
        for count in range(min(2 * every * reset, 5000)):
            densify, reset_now = count % every == offset, count % reset == 0
            got = mapping_rule(be, count)
            assert got == ("densify" if densify else "reset" if reset_now else None), (offset, reset, count)
            assert not (offset >= every and got == "densify"), (offset, count)


def test_mapping_rule_densifies_where_both_expressions_hold_and_reads_the_backend_when_asked():
    be = _backend(4, 2, 7)
    assert 14 % 4 == 2 and 14 % 7 == 0 and mapping_rule(be, 14) == "densify" and mapping_rule(be, 42) == "densify"
    assert mapping_rule(be, 7) == "reset" and mapping_rule(be, 6) == "densify" and mapping_rule(be, 8) is None
    be.gaussian_update_offset = 3                       # (a back-end whose attributes are assigned later, or changed: nothing is frozen)
    assert mapping_rule(be, 14) == "reset" and mapping_rule(be, 7) == "densify"


def test_init_rule_gives_both_halves_and_the_network_loop_reads_only_the_first():
    be = types.SimpleNamespace(init_gaussian_update=20, init_gaussian_reset=21, opt_params=types.SimpleNamespace(densify_from_iter=500))
    # a call that starts at iteration_count = 0: iteration m runs with count m + 1
    assert init_rule(be, 20, 21) == (True, True)                      # both in one iteration (densify runs first)
    assert init_rule(be, 499, 500) == (False, True)                   # count == densify_from_iter alone
    assert init_rule(be, 0, 1) == (True, False) and init_rule(be, 40, 41) == (True, False) and init_rule(be, 7, 8) == (False, False)
    assert init_rule(be, 20) == (True, False) and init_rule(be, 21) == (False, False)          # initialize_network: never resets


@pytest.mark.parametrize("every", EVERY)
def test_plain_runs_and_special_singletons_cover_a_static_call_in_order(every):
    """BackEnd.map_static's splitting, with its predicate -- the rule at iteration_count + (k - it) + 1 -- on a back-end whose counter
    advances with the iterations done, against the rule at each iteration's own count."""
    for (offset, reset), start, length, count0 in itertools.product(_grid(every), STARTS, LENGTHS, COUNTS):
        be, stop = _backend(every, offset, reset, count0), start + length
        special = lambda k: mapping_rule(be, count0 + (k - start) + 1) is not None          # noqa: E731
        it, covered, kinds = start, [], []
        while it < stop:
            run = plain_run(it, stop, lambda k: mapping_rule(be, be.iteration_count + (k - it) + 1) is not None)
            assert 0 <= run <= stop - it
            if run == 0:
                assert special(it), (offset, reset, start, length, it)
            else:
                assert not any(special(k) for k in range(it, it + run)), (offset, reset, start, length, it, run)          # nothing special inside
                assert it + run == stop or special(it + run), (offset, reset, start, length, it, run)                     # maximal
                assert not kinds or kinds[-1] == "special"                                    # (two plain runs never follow each other)
            kinds.append("plain" if run else "special")
            n = max(run, 1)
            covered += range(it, it + n)
            be.iteration_count += n
            it += n
        assert covered == list(range(start, stop)) and be.iteration_count == count0 + length


def test_plain_run_counts_up_to_the_first_special_iteration_or_the_end():
    assert plain_run(3, 3, lambda k: False) == 0 and plain_run(3, 9, lambda k: False) == 6 and plain_run(3, 9, lambda k: True) == 0
    assert plain_run(3, 9, lambda k: k == 7) == 4 and plain_run(7, 9, lambda k: k == 7) == 0 and plain_run(8, 9, lambda k: k == 7) == 1


@pytest.mark.parametrize("every", EVERY)
def test_dynamic_runs_stop_at_the_phase_changes_and_count_only_while_the_gaussians_step(every):
    """slam/dynamic_graph.plain_rows, the splitter of DynamicMapping.execute, walked as execute walks it (iters = 20, warm = 10: the loss
    weights change at i = 10, the Gaussians step from i = 11 on and only then does iteration_count advance, before the iteration's work)."""
    from slam.dynamic_graph import phase, plain_rows
    iters, warm = 20, 10
    assert [phase(i, iters, warm) for i in (0, 9, 10, 11, 19)] == [(True, False), (True, False), (False, False), (False, True), (False, True)]
    for (offset, reset), count0 in itertools.product(_grid(every), COUNTS):
        be = _backend(every, offset, reset, count0)
        count_of = lambda i: count0 + (i - warm)                                              # noqa: E731  (iteration i > warm's own count)
        i, runs, specials = 0, [], []
        while i < iters:
            stepping = phase(i, iters, warm)[1]
            rows = plain_rows(be, i, iters, warm)
            if rows == 0:
                assert stepping and mapping_rule(be, count_of(i)) is not None, (offset, reset, i)
                specials.append(i)
            else:
                runs.append(range(i, i + rows))
                assert len({phase(k, iters, warm) for k in runs[-1]}) == 1
                assert not stepping or all(mapping_rule(be, count_of(k)) is None for k in runs[-1]), (offset, reset, i, rows)
                end = i + rows
                assert (end == iters or phase(end, iters, warm) != phase(i, iters, warm)
                        or (stepping and mapping_rule(be, count_of(end)) is not None)), (offset, reset, i, rows)          # maximal
            n = max(rows, 1)
            if stepping:
                be.iteration_count += n
            else:
                assert be.iteration_count == count0                                           # (no count over the half that does not step)
            i += n
        assert runs[0] == range(0, 10) and runs[1] == range(10, 11)
        assert not any((9 in r and 10 in r) or (10 in r and 11 in r) for r in runs)
        assert sorted([k for r in runs for k in r] + specials) == list(range(iters))
        assert specials == [k for k in range(warm + 1, iters) if mapping_rule(be, count_of(k)) is not None]
        assert be.iteration_count == count0 + iters - warm - 1
