"""slam/schedule.py and slam/keyframe_slots.py on the device: gsr_schedule_advance through Schedule.advance, gsr_slot_gather through a
bank of two slots fed from three candidates. Exact equality only."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_schedule_advance_walks_the_rows_clamps_at_the_last_and_restarts_with_a_zeroed_counter():
    from slam.schedule import Schedule
    rows, rng = 3, np.random.default_rng(0)
    index = rng.integers(0, 2 ** 32, (rows, 2), dtype=np.uint64).astype(np.uint32)
    adam, samples = rng.standard_normal((rows, 8)).astype(np.float32), rng.standard_normal((rows, 60)).astype(np.float32)
    want, coef_lo, samples_lo = Schedule.pack(rows, index, adam, samples)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    sch = Schedule(rows, torch.device(DEV), index_words=index, adam=adam, samples=samples, counter=counter)
    assert sch.row_words == 70 and (sch.coef_lo, sch.samples_lo) == (coef_lo, samples_lo) == (2, 10)       # 70 words: two trips of the 64 lanes
    assert sch.counter is counter and sch.coefficients_ptr() == sch.current.data_ptr() + 4 * 2
    current = lambda: sch.current.cpu().numpy().view(np.uint32)
    for call in range(1, 5):
        sch.advance()
        assert int(counter.item()) == call
        assert np.array_equal(current(), want[min(call, rows) - 1]), call            # the 4th call stays on the last row
    assert np.array_equal(sch.indices(2).cpu().numpy().view(np.uint32), index[2])
    assert np.array_equal(sch.samples().cpu().numpy().view(np.uint32), samples[2].view(np.uint32))
    counter.zero_()
    sch.advance()
    assert int(counter.item()) == 1 and np.array_equal(current(), want[0])
    own = Schedule(rows, torch.device(DEV), adam=adam)                                  # (a counter of its own, one block only)
    own.advance()
    own.advance()
    assert int(own.counter.item()) == 2 and np.array_equal(own.current.cpu().numpy().view(np.uint32), adam[1].view(np.uint32))


def _candidates(n, H, W):
    from slam.camera import Camera, getProjectionMatrix2
    fx, fy, cx, cy = 6.0, 6.5, W / 2, H / 2
    proj = getProjectionMatrix2(0.01, 100.0, cx, cy, fx, fy, W, H).transpose(0, 1)
    cams = []
    for k in range(n):
        cam = Camera(k, None, None, torch.eye(4), proj, fx, fy, cx, cy, 1.0, 0.8, H, W, 0.0, device=DEV)
        a = 0.3 * (k + 1)
        cam.update_RT(torch.tensor([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]), torch.tensor([0.1 * k, -0.2, 1.0 + k]))
        with torch.no_grad():
            cam.exposure_a.fill_(0.01 * (k + 1))
            cam.exposure_b.fill_(-0.02 * (k + 1))
        cams.append(cam)
    return cams


def _assert_camera_copied(slot, cand):
    for name in ("world_view_transform", "full_proj_transform", "camera_center", "exposure_a", "exposure_b"):
        assert torch.equal(getattr(slot, name).detach(), getattr(cand, name).detach()), name


@pytest.mark.parametrize("H, W", [(5, 7), (4, 8)])        # 35 pixels: planes of a [6, H, W] tensor off 16-byte alignment, a tail; 32: float4 copies
def test_slot_gather_fills_own_and_partner_slots_from_the_drawn_candidates(H, W):
    from slam import keyframe_slots as ks
    from slam.schedule import Schedule
    dev, picks = torch.device(DEV), [2, 0]
    torch.manual_seed(H * W)
    cands = _candidates(3, H, W)
    cand_ops = [tuple(torch.rand((c, H, W), device=dev) for c in (3, 1, 1, 1)) for _ in cands]
    cand_f6 = [torch.rand((6, H, W), device=dev) for _ in cands]
    planes = lambda f: (f[0:3], f[3:4], f[4:5], f[5:6])
    slots, partners = ([ks.blank_camera(cands[0], uid0 - s, dev) for s in range(2)] for uid0 in (-1, -101))
    slot_ops, partner_f6 = [ks.slot_buffers(H, W, dev) for _ in slots], [torch.zeros((6, H, W), device=dev) for _ in partners]
    assert [tuple(t.shape) for t in slot_ops[0]] == [(3, H, W), (1, H, W), (1, H, W), (1, H, W)]
    own_table = ks.upload_rows(ks.address_rows(cands, cand_ops), torch.int64, dev)
    partner_table = ks.upload_rows(ks.address_rows(cands[::-1], [planes(f) for f in cand_f6]), torch.int64, dev)      # (partner of k: candidate 2 - k)
    assert tuple(own_table.shape) == tuple(partner_table.shape) == (3, 9)
    sch = Schedule(1, dev, index_words=[picks])
    sch.advance()
    ks.gather(2, own_table, sch.indices(2), ks.entries(list(zip(slots, slot_ops))), H * W, dev)
    ks.gather(2, partner_table, sch.indices(2), ks.entries([(c, planes(f)) for c, f in zip(partners, partner_f6)]), H * W, dev)
    torch.cuda.synchronize(dev)
    for s, k in enumerate(picks):
        _assert_camera_copied(slots[s], cands[k])
        for got, want in zip(slot_ops[s], cand_ops[k]):
            assert torch.equal(got, want), (s, tuple(got.shape))
        _assert_camera_copied(partners[s], cands[2 - k])
        assert torch.equal(partner_f6[s], cand_f6[k]), s


def test_slot_gather_without_slots_launches_nothing():
    from slam import keyframe_slots as ks
    assert ks.gather(0, None, None, None, 35, torch.device(DEV)) is None          # (None tables: any use of them would raise)
    assert ks.upload_rows([], torch.int64, torch.device(DEV)) is None
