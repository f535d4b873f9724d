"""What the pretrained networks (slam/optical_flow.py RAFT, slam/segmentation.py YOLO, slam/perceptual.py LPIPS) share around their own
arithmetic: checking a state_dict against a name -> shape table, seeded stand-in weights, reading a checkpoint once per process, refusing
graph capture, deterministic convolutions, a cached workspace and device-event timing. Imports without a GPU or the HIP library."""
import contextlib
import os
import zlib

import numpy as np
import torch


def strip_module_prefix(sd, what):
    """The state_dict without DataParallel's `module.` prefix; anything but a dict raises."""
    if not isinstance(sd, dict):
        raise ValueError(f"{what}: expected a state_dict, got {type(sd).__name__}")
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def check_entries(sd, want, what):
    """sd against the name -> shape table `want`: a missing, extra or misshapen entry raises and names it."""
    missing = [k for k in want if k not in sd]
    if missing:
        raise KeyError(f"{what} lacks {missing[0]!r} ({len(missing)} missing entries)")
    extra = [k for k in sd if k not in want]
    if extra:
        raise KeyError(f"{what} has an unexpected entry {extra[0]!r} ({len(extra)} extra entries)")
    for k, shape in want.items():
        got = tuple(getattr(sd[k], "shape", ()))
        if not isinstance(sd[k], torch.Tensor) or got != shape:
            raise ValueError(f"{what} entry {k!r} has shape {got}, expected {shape}")


def entry_rng(seed, name):
    """The generator of one entry of a seeded stand-in state_dict: independent of the other entries and of their order."""
    return np.random.default_rng([seed, zlib.crc32(name.encode())])


def load_once(cache, paths, device, extra_key, build):
    """build(*real paths) the first time these files (by real path and mtime), device and extra_key are asked for; from `cache` after."""
    paths = tuple(os.path.realpath(p) for p in paths)
    key = (paths, tuple(os.path.getmtime(p) for p in paths), str(torch.device(device)), extra_key)
    if key not in cache:
        cache[key] = build(*paths)
    return cache[key]


def refuse_capture(who, hint):
    """The networks allocate, and their results are cached by the caller: none of them may run while a graph is being captured."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{who} was called while the current stream is capturing a graph: {hint}")


def deterministic_convolutions():
    """Context manager: deterministic MIOpen algorithms without benchmarking, so the same input gives the same bits on every call."""
    return torch.backends.cudnn.flags(enabled=torch.backends.cudnn.enabled, benchmark=False, deterministic=True)


def workspace(cache, key, nbytes, device):
    """A uint8 buffer of nbytes on device, kept in the dict `cache` under key (cache=None: allocated and not kept)."""
    ws = None if cache is None else cache.get(key)
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        if cache is not None:
            cache[key] = ws
    return ws


class EventLog:
    """Device time of repeated calls: ``with log.timed(): ...`` puts an event pair around the block. Nothing is recorded on the CPU."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._events = []             # (start, end, count)

    @contextlib.contextmanager
    def timed(self, stream=None, count=1):
        """Times the block on `stream` (None: the device's current stream) as one call that handled `count` items."""
        if self.device.type == "cpu":
            yield
            return
        stream = torch.cuda.current_stream(self.device) if stream is None else stream
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(stream)
        yield
        end.record(stream)
        self._events.append((start, end, int(count)))

    def summary(self):
        """Calls and items timed, the mean ms per item, the ms of the first call and the mean ms per item of the later calls (None where
        there is no such call). Waits for the last call first: an event pair can be read only once it has completed."""
        if self._events:
            self._events[-1][1].synchronize()
        ms = [s.elapsed_time(e) for s, e, _ in self._events]
        n = sum(c for _, _, c in self._events)
        return {"calls": len(ms), "items": n, "ms_per_item": float(sum(ms) / n) if n else None, "ms_first": ms[0] if ms else None,
                "ms_per_item_rest": float(sum(ms[1:]) / (n - self._events[0][2])) if len(ms) > 1 else None}
