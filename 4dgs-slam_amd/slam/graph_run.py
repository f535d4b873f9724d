"""ONE protocol for the runs of plain mapping iterations that the back-end replays as hipGraphs: static ``map_static`` and
``initialize_map`` (slam/mapping_graph.py), dynamic ``map`` and ``initialize_network`` (slam/dynamic_graph.py).

A run of `rows` iterations: `warm` of them executed directly on the back-end's first graph stream (torch's capture protocol: autograd's
stream bookkeeping must have seen the stream family the capture will use), a snapshot of what a replay may write, ONE iteration captured on
the second stream into the back-end's shared memory pool, `rows - warm` replays, and a look at the sticky overflow counters of every view
slot. When the capture raised or a replay outgrew its binning buffer, the snapshot is restored and the caller finishes the run its own way.

A runner provides:
  * ``device``;
  * ``iteration()`` -- ONE code path: executed directly for the warm-up, captured once, then replayed;
  * ``state_tensors()`` -- every tensor a replay may write (the snapshot);
  * ``discard()`` -- after an undo: camera matrices from the restored poses, no gradient left over from the capture.

What a run needs of the back-end is declared in BackEnd.__init__: the two streams, the pool and the newest graph; the statistics per kind
of run, ``backend.<kind>_stats`` (runs, replays, direct, redone, failed, last_error, capture_ms, overflow_causes; empty until a run of
that kind is first touched); and ``backend._broken_graphs``, the kinds whose capture failed -- that kind's graphs are off from then on (a
failed static capture, kind "graph", also switches off every other kind: BackEnd._graphs_enabled)."""
import contextlib
import gc
import time

import torch

from diff_gaussian_rasterization import _C


def stats(backend, kind):
    st = getattr(backend, f"{kind}_stats")
    if not st:
        st.update(runs=0, replays=0, direct=0, redone=0, failed=0)
    return st


def broken(backend, kind):
    return kind in backend._broken_graphs


def note_failure(backend, kind, error):
    """Count a run that could not use its graph; ``Training.mapping_graph = "strict"`` re-raises."""
    st = stats(backend, kind)
    st["failed"] += 1
    st["last_error"] = f"{type(error).__name__}: {error}"
    if backend.config["Training"].get("mapping_graph") == "strict":
        raise error


@contextlib.contextmanager
def capture_options(**opts):
    """The rasterizer options (gsr_set_option) of a capture, put back however the block is left: they only matter while host code runs --
    replays never consult them. The cycle collector is held off meanwhile: destroying what it finds (an earlier run's streams, events,
    graphs) takes calls that a process must not make while a stream captures, and the runtime aborts on them."""
    before, collecting = {}, gc.isenabled()
    gc.disable()
    try:
        for name, value in opts.items():
            before[name] = _C.set_option(name, value)
        yield
    finally:
        for name, value in before.items():
            _C.set_option(name, value)
        if collecting:
            gc.enable()


def capture(backend, runner, options):
    """One iteration of `runner`, captured. Not through ``torch.cuda.graph``: its __enter__ runs gc.collect() and empties the allocator's
    cache -- tens of milliseconds per capture at SLAM sizes, and every mapping call captures anew (the map's tensors change with every
    keyframe). All captures of a back-end share ONE private memory pool; the previous graph is kept alive until this capture has begun, so
    the pool (and its blocks) survive from capture to capture."""
    dev = runner.device
    s = backend.graph_streams(dev)[1]
    with capture_options(lazy=1, **options):
        s.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            graph.capture_begin(pool=backend.graph_pool(dev))
            try:
                runner.iteration()
            finally:
                graph.capture_end()
    torch.cuda.current_stream(dev).wait_stream(s)
    backend._graph_keepalive = graph             # (drops the previous run's graph: the pool now belongs to this one)
    return graph


def replay_run(backend, runner, rows, warm, *, kind, options):
    """`rows` iterations of `runner` as warm-up + capture + replays (capture `options` on top of the lazy mode). Returns how many
    iterations' effects stand: `rows`, or `warm` when the capture raised or a replay overflowed -- the state is then what the warm-up
    left, and the caller does the rest of the run without the graph."""
    dev = runner.device
    st = stats(backend, kind)
    s = backend.graph_streams(dev)[0]
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(warm):
            runner.iteration()
    torch.cuda.current_stream(dev).wait_stream(s)
    st["direct"] += warm
    if rows <= warm:
        return rows
    # (the directly executed iterations waited for their headers and redid what overflowed themselves)
    overflow0, slots0 = _C.forward_status_views(), _C.debug_view_slots(100)
    with torch.no_grad():
        snap = [(t, t.detach().clone()) for t in runner.state_tensors()]

    def undo():
        with torch.no_grad():
            for t, c in snap:
                t.detach().copy_(c)
            runner.discard()

    try:
        t0 = time.perf_counter()
        graph = capture(backend, runner, options)
        st["capture_ms"] = st.get("capture_ms", 0.0) + (time.perf_counter() - t0) * 1e3
    except Exception as e:        # a capture that fails leaves the warm-up valid: the caller finishes the run, this kind stops capturing
        backend._broken_graphs.add(kind)
        torch.cuda.synchronize(dev)
        undo()
        note_failure(backend, kind, e)
        return warm
    for _ in range(rows - warm):
        graph.replay()
    torch.cuda.current_stream(dev).synchronize()
    if _C.forward_status_views() != overflow0:          # a replayed view outgrew its binning buffer: undo the replays
        # (which slot outgrew what, with the estimates the layout started from: the capture margins are sized from these)
        moved = [dict(slot=k, **{n: a[n] for n in ("R_alloc", "longest_tile", "estimate_R_alloc", "estimate_longest_tile")},
                      captured_estimate_R=b["estimate_R_alloc"], captured_estimate_tile=b["estimate_longest_tile"])
                 for k, (a, b) in enumerate(zip(_C.debug_view_slots(100), slots0)) if a["overflows"] != b["overflows"]]
        st.setdefault("overflow_causes", []).append({"rows": int(rows - warm), "gaussians": int(backend.gaussians.get_xyz.shape[0]), "slots": moved[:6]})
        undo()
        st["redone"] += rows - warm
        return warm
    st["replays"] += rows - warm
    st["runs"] += 1
    return rows
