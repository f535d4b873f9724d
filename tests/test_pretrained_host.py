"""Host-side checks of what the pretrained networks share (slam/pretrained.py): the state_dict checks and their messages, the seeded
per-entry generator, reading a checkpoint once per process, the capture guard, the cached workspace and the event log. No GPU needed."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "4dgs-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam import pretrained  # noqa: E402

WANT = {"a.weight": (4, 3, 1, 1), "a.bias": (4,)}


def _sd():
    return {k: torch.zeros(s) for k, s in WANT.items()}


def test_strip_module_prefix():
    sd = _sd()
    assert list(pretrained.strip_module_prefix({"module." + k: v for k, v in sd.items()}, "x")) == list(sd)
    assert pretrained.strip_module_prefix(sd, "x") == sd
    with pytest.raises(ValueError, match=r"some file: expected a state_dict, got list"):
        pretrained.strip_module_prefix([1, 2], "some file")


def test_check_entries_names_the_entry():
    pretrained.check_entries(_sd(), WANT, "toy checkpoint")
    missing = _sd()
    del missing["a.bias"]
    with pytest.raises(KeyError, match=r"toy checkpoint lacks 'a\.bias' \(1 missing entries\)"):
        pretrained.check_entries(missing, WANT, "toy checkpoint")
    extra = dict(_sd(), **{"b.weight": torch.zeros(2), "c.weight": torch.zeros(2)})
    with pytest.raises(KeyError, match=r"toy checkpoint has an unexpected entry 'b\.weight' \(2 extra entries\)"):
        pretrained.check_entries(extra, WANT, "toy checkpoint")
    shaped = dict(_sd(), **{"a.weight": torch.zeros((4, 3, 3, 3))})
    with pytest.raises(ValueError, match=r"toy checkpoint entry 'a\.weight' has shape \(4, 3, 3, 3\), expected \(4, 3, 1, 1\)"):
        pretrained.check_entries(shaped, WANT, "toy checkpoint")
    with pytest.raises(ValueError, match=r"'a\.bias' has shape \(\), expected \(4,\)"):
        pretrained.check_entries(dict(_sd(), **{"a.bias": 0.5}), WANT, "toy checkpoint")            # not a tensor


def test_entry_rng_is_the_documented_generator():
    a = pretrained.entry_rng(3, "a.weight").uniform(-1, 1, 8)
    assert np.array_equal(a, np.random.default_rng([3, zlib.crc32(b"a.weight")]).uniform(-1, 1, 8))
    assert not np.array_equal(a, pretrained.entry_rng(3, "a.bias").uniform(-1, 1, 8))
    assert not np.array_equal(a, pretrained.entry_rng(4, "a.weight").uniform(-1, 1, 8))


def test_load_once_builds_once_per_file_state(tmp_path):
    path = tmp_path / "w.pth"
    path.write_bytes(b"one")
    link = tmp_path / "link.pth"
    os.symlink(path, link)
    cache, built = {}, []

    def build(*paths):
        built.append(paths)
        return object()
    a = pretrained.load_once(cache, [str(path)], "cpu", None, build)
    assert pretrained.load_once(cache, [str(path)], "cpu", None, build) is a
    assert pretrained.load_once(cache, [str(link)], "cpu", None, build) is a                       # by real path
    assert built == [(os.path.realpath(path),)]
    assert pretrained.load_once(cache, [str(path)], "cpu", "other", build) is not a                # the extra key counts
    assert pretrained.load_once(cache, [str(path)], "cuda:0", None, build) is not a                # and so does the device
    assert len(built) == 3
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 2_000_000_000))                            # the file changed: read again
    b = pretrained.load_once(cache, [str(path)], "cpu", None, build)
    assert b is not a and len(built) == 4
    assert pretrained.load_once(cache, [str(path)], "cpu", None, build) is b
    with pytest.raises(OSError):
        pretrained.load_once(cache, [str(tmp_path / "missing.pth")], "cpu", None, build)
    with pytest.raises(ValueError, match="bad file"):                                              # a failed build is not kept
        pretrained.load_once({}, [str(path)], "cpu", None, lambda path: (_ for _ in ()).throw(ValueError("bad file")))


def test_refuse_capture_is_silent_outside_capture():
    assert pretrained.refuse_capture("Net.forward", "run it before capture") is None               # and without a device at all


def test_refuse_capture_message(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match=r"Net\.forward was called while the current stream is capturing a graph: run it before capture"):
        pretrained.refuse_capture("Net.forward", "run it before capture")


def test_deterministic_convolutions_sets_and_restores_the_flags():
    before = (torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic)
    with pretrained.deterministic_convolutions():
        assert not torch.backends.cudnn.benchmark and torch.backends.cudnn.deterministic
    assert (torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic) == before


def test_workspace_is_kept_by_key():
    cache = {}
    a = pretrained.workspace(cache, (7, "cpu"), 64, "cpu")
    assert a.dtype == torch.uint8 and a.numel() == 64
    assert pretrained.workspace(cache, (7, "cpu"), 64, "cpu") is a
    b = pretrained.workspace(cache, (8, "cpu"), 32, "cpu")
    assert b is not a and b.numel() == 32 and len(cache) == 2
    c = pretrained.workspace(None, (7, "cpu"), 64, "cpu")                                           # no cache: a fresh buffer each time
    assert c is not a and pretrained.workspace(None, (7, "cpu"), 64, "cpu") is not c


def test_event_log_without_events():
    log = pretrained.EventLog("cpu")
    empty = {"calls": 0, "items": 0, "ms_per_item": None, "ms_first": None, "ms_per_item_rest": None}
    assert log.summary() == empty
    ran = []
    with log.timed(count=3):                                                                        # on the CPU the block runs untimed
        ran.append(1)
    assert ran == [1] and log.summary() == empty
