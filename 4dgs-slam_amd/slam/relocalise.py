"""Relocalisation: recovering a camera whose pose is unknown, in a run or in a saved map. The checked ctypes binding of
include/relocalisation.h (gsr_reloc_encode: the randomised-fern code of a frame, Glocker et al.; gsr_reloc_search: a code against a database
of keyframe codes; gsr_reloc_score: the counts by which a rendering is judged against a frame; csrc/gs_reloc.h) and what is built from them:

  KeyframeIndex   the fern table, a growable device database of keyframe codes and the keyframe ids: place recognition
  score, verdict  does the map rendered at a pose agree with the frame?
  Relocaliser     localise(): candidates of the index in order: render the map at the candidate keyframe, align the frame against that
                  rendering (slam/odometry.py), track from there, accept the first pose the verdict agrees with; judge(): the "am I lost?"
                  test of a tracked frame and, if it is, localise() -- one path for a run (slam/stages.py Relocalisation) and for follow()
  MapLocaliser    the same against a map_io.LoadedMap, whose index is built from renderings at the keyframe poses; follow() tracks a sequence

The reference has no counterpart. tests/reloc_reference.py restates the three kernels in integer numpy. No CPU path.

Limits: nothing here has been run on real images. A relocalised frame is only given a pose; correcting the map when a place is seen again
is the work of slam/loop_closure.py (``Training.loop_closure``, off by default, static RGB-D and stereo runs only). Dynamic saved maps are
refused."""
import math

import numpy as np
import torch

from diff_gaussian_rasterization import _C

from .camera import Camera, compose_pose, frame_tensors, opaque_depth
from .options import check_gate, check_pass_counts, read_block, to_floats
from .pretrained import EventLog

I32 = (torch.int32,)
MASK = (torch.uint8, torch.bool)
COUNTS = ("masked", "considered", "colour_ok", "depth_valid", "depth_ok", "zero5", "zero6", "zero7")
MAX_CELLS, MAX_FERNS, MAX_TOPK = 4096, 2048, 16


# ---- the three calls ---------------------------------------------------------------------------------------------------------------
def encode_workspace_size(grid_w, grid_h):
    return int(_C.load_library().gsr_reloc_encode_workspace_size(int(grid_w), int(grid_h)))


def encode(image, depth, mask, grid, table, depth_scale, code, workspace=None, stream=None):
    """One call of gsr_reloc_encode. image float32 [3, H, W]; depth None or float32 [H, W]; mask None or uint8 / bool [H, W] (0 = exclude);
    grid = (grid_w, grid_h); table int32 [F, 5] on the device; code int32 [F / 8] (the bits of the uint32 words; it may be a row of a
    database). The library checks the ranges and raises RuntimeError with its text."""
    _C._require_device(image, "image")
    if image.dim() != 3 or image.shape[0] != 3:
        raise RuntimeError(f"image must be [3, H, W], got {tuple(image.shape)}")
    H, W = int(image.shape[1]), int(image.shape[2])
    if table.dim() != 2 or table.shape[1] != 5:
        raise RuntimeError(f"table must be [F, 5], got {tuple(table.shape)}")
    F = int(table.shape[0])
    grid_w, grid_h = (int(v) for v in grid)
    args = [_C.dev_ptr(image, "image", _C.F32, (3, H, W)), _C.dev_ptr(depth, "depth", _C.F32, (H, W)), _C.dev_ptr(mask, "mask", MASK, (H, W))]
    table_ptr, code_ptr = _C.dev_ptr(table, "table", I32, (F, 5)), _C.dev_ptr(code, "code", I32, (F // 8,))
    lib = _C.load_library()
    workspace = _C.workspace(workspace, int(lib.gsr_reloc_encode_workspace_size(grid_w, grid_h)) if workspace is None else 0, image.device)
    with torch.cuda.device(image.device):
        lib.gsr_reloc_encode(W, H, *args, grid_w, grid_h, F, table_ptr, float(depth_scale), code_ptr, workspace.data_ptr() or None,
                             int(workspace.numel()), _C.stream_handle(stream, image.device))


def search(database, rows, query, ferns, nibble_mask, topk, distance, best, stream=None):
    """One call of gsr_reloc_search over the first `rows` rows of database int32 [>= rows, F / 8] (None with rows == 0). query int32
    [F / 8]; distance int32 [>= rows] (None with rows == 0) and best int32 [topk, 2], rows (index, distance), are written."""
    rows, F, topk = int(rows), int(ferns), int(topk)
    dev = best.device
    if database is not None and (database.dim() != 2 or database.shape[0] < rows or database.shape[1] != F // 8):
        raise RuntimeError(f"database must be [>= {rows}, {F // 8}], got {tuple(database.shape)}")
    if distance is not None and (distance.dim() != 1 or distance.shape[0] < rows):
        raise RuntimeError(f"distance must hold {rows} entries, got {tuple(distance.shape)}")
    args = [_C.dev_ptr(database, "database", I32), _C.dev_ptr(query, "query", I32, (F // 8,))]
    outs = [_C.dev_ptr(distance, "distance", I32), _C.dev_ptr(best, "best", I32, (topk, 2))]
    with torch.cuda.device(dev):
        _C.load_library().gsr_reloc_search(rows, F, *args, int(nibble_mask), topk, *outs, _C.stream_handle(stream, dev))


def score_counts(render, render_depth, opacity, image, depth, mask, tau_colour, tau_depth, counts, stream=None):
    """One call of gsr_reloc_score: render, image float32 [3, H, W]; render_depth, opacity float32 [H, W]; depth None or float32 [H, W];
    mask None or uint8 / bool [H, W]; counts int32 [8] is written (COUNTS)."""
    _C._require_device(render, "render")
    if render.dim() != 3 or render.shape[0] != 3:
        raise RuntimeError(f"render must be [3, H, W], got {tuple(render.shape)}")
    H, W = int(render.shape[1]), int(render.shape[2])
    args = [_C.dev_ptr(render, "render", _C.F32, (3, H, W)), _C.dev_ptr(render_depth, "render_depth", _C.F32, (H, W)),
            _C.dev_ptr(opacity, "opacity", _C.F32, (H, W)), _C.dev_ptr(image, "image", _C.F32, (3, H, W)),
            _C.dev_ptr(depth, "depth", _C.F32, (H, W)), _C.dev_ptr(mask, "mask", MASK, (H, W))]
    with torch.cuda.device(render.device):
        _C.load_library().gsr_reloc_score(W, H, *args, int(tau_colour), float(tau_depth), _C.dev_ptr(counts, "counts", I32, (len(COUNTS),)),
                                          _C.stream_handle(stream, render.device))


# ---- the fern table ----------------------------------------------------------------------------------------------------------------
def quantise_depth(d, depth_scale):
    """dq of include/relocalisation.h for one host float: float32 operation by operation."""
    s = np.float32(d) * np.float32(depth_scale)
    return 65535 if s >= np.float32(65535.0) else int(s + np.float32(0.5))


def fern_table(ferns, grid_w, grid_h, seed, depth_lo, depth_hi, depth_scale):
    """int32 [ferns, 5] on the host, rows (cell, tR, tG, tB, tD), from np.random.default_rng(seed): cells uniform over the grid, colour
    thresholds uniform in [32, 224), depth thresholds uniform in [dq(depth_lo), dq(depth_hi)]. The same arguments give the same bytes."""
    ferns, cells = int(ferns), int(grid_w) * int(grid_h)
    lo, hi = quantise_depth(depth_lo, depth_scale), quantise_depth(depth_hi, depth_scale)
    if not 0 <= lo <= hi:
        raise ValueError(f"fern_table: depth_lo {depth_lo} and depth_hi {depth_hi} quantise to {lo} and {hi}: they must be in order")
    rng = np.random.default_rng(int(seed))
    table = np.empty((ferns, 5), np.int32)
    table[:, 0] = rng.integers(0, cells, size=ferns)
    table[:, 1:4] = rng.integers(32, 224, size=(ferns, 3))
    table[:, 4] = rng.integers(lo, hi + 1, size=ferns)
    return table


# ---- options -----------------------------------------------------------------------------------------------------------------------
# min_score lies between the colour shares measured on the synthetic sequence: at least 0.82 at the poses a run tracked (against the map as it
# was when the frame was tracked), at most 0.63 at the pose of a keyframe ten or more frames away (Relocalisation)
RELOCALISATION_DEFAULTS = {"enabled": False, "ferns": 512, "grid": [40, 30], "seed": 0, "topk": 4, "depth_scale": 1000.0, "depth_lo": 0.3,
                           "depth_hi": 6.0, "tau_colour": 48, "tau_depth": 0.05, "min_score": 0.72, "min_coverage": 0.5, "levels": 4,
                           "iters": None, "max_translation": 1.0, "max_rotation": 30.0}
DEFAULT_ITERS = (5, 7, 10, 10, 10, 10)         # per level, finest first: the first `levels` of these


def relocalisation_options(training):
    """The ``Training.relocalisation`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys and values
    the kernels or the alignment cannot take are refused here, before the run starts. grid = [grid_w, grid_h]; depth_lo / depth_hi in
    metres; iters lists the alignment's passes per level, finest first (default: one count per level); max_translation in metres,
    max_rotation in degrees: the gate of the alignment against a keyframe's rendering, wider than the frame-to-frame one."""
    name = "Training.relocalisation"
    opt = read_block(training, "relocalisation", RELOCALISATION_DEFAULTS)
    if opt is None:
        return None
    for key in ("ferns", "seed", "topk", "tau_colour", "levels"):
        if isinstance(opt[key], float) and not opt[key].is_integer():
            raise ValueError(f"{name}.{key} must be an integer, got {opt[key]!r}")
        opt[key] = int(opt[key])
    if not 8 <= opt["ferns"] <= MAX_FERNS or opt["ferns"] % 8:
        raise ValueError(f"{name}.ferns must be a multiple of 8 in [8, {MAX_FERNS}], got {opt['ferns']}")
    if isinstance(opt["grid"], (str, bytes)) or not hasattr(opt["grid"], "__len__") or len(opt["grid"]) != 2:
        raise ValueError(f"{name}.grid must be [grid_w, grid_h], got {opt['grid']!r}")
    opt["grid"] = [int(v) for v in opt["grid"]]
    if min(opt["grid"]) < 1 or opt["grid"][0] * opt["grid"][1] > MAX_CELLS:
        raise ValueError(f"{name}.grid must hold two positive counts with at most {MAX_CELLS} cells, got {opt['grid']}")
    if opt["seed"] < 0:
        raise ValueError(f"{name}.seed must not be negative, got {opt['seed']}")
    if not 1 <= opt["topk"] <= MAX_TOPK:
        raise ValueError(f"{name}.topk must be 1 to {MAX_TOPK}, got {opt['topk']}")
    if not 0 <= opt["tau_colour"] <= 765:
        raise ValueError(f"{name}.tau_colour must be in [0, 765], got {opt['tau_colour']}")
    to_floats(opt, name, ("depth_scale", "depth_lo", "depth_hi", "tau_depth", "min_score", "min_coverage", "max_translation", "max_rotation"))
    if not (0.0 < opt["depth_scale"] < math.inf):
        raise ValueError(f"{name}.depth_scale must be positive and finite, got {opt['depth_scale']}")
    if not (0.0 < opt["depth_lo"] < opt["depth_hi"] < math.inf):
        raise ValueError(f"{name} needs 0 < depth_lo < depth_hi, got depth_lo {opt['depth_lo']} and depth_hi {opt['depth_hi']}")
    if not (0.0 <= opt["tau_depth"] < math.inf):
        raise ValueError(f"{name}.tau_depth must be finite and not negative, got {opt['tau_depth']}")
    for key in ("min_score", "min_coverage"):
        if not 0.0 <= opt[key] <= 1.0:
            raise ValueError(f"{name}.{key} must be in [0, 1], got {opt[key]}")
    if not 1 <= opt["levels"] <= 6:
        raise ValueError(f"{name}.levels must be 1 to 6, got {opt['levels']}")
    if opt["iters"] is None:
        opt["iters"] = list(DEFAULT_ITERS[:opt["levels"]])
    check_pass_counts(opt, name)
    check_gate(opt, name, ("max_translation", "max_rotation"))
    return opt


def default_options(**overrides):
    """The enabled block with its defaults (MapLocaliser, tools): relocalisation_options of {"enabled": True, **overrides}."""
    return relocalisation_options({"relocalisation": {"enabled": True, **overrides}})


# ---- place recognition -------------------------------------------------------------------------------------------------------------
class KeyframeIndex:
    """The fern table, the codes of the keyframes added so far (a device database that doubles when it is full) and their ids.

        index.add(frame_id, image, depth, mask)                  # one gsr_reloc_encode straight into the next row
        best, distance = index.query(image, depth, None, topk)   # device tensors: best int32 [topk, 2] rows (row, distance), row -1 = none
        index.ids[row]                                           # the id a row was added under

    query() reads nothing: whoever needs the candidates on the host reads `best`."""

    def __init__(self, ferns=512, grid=(40, 30), seed=0, depth_lo=0.3, depth_hi=6.0, depth_scale=1000.0, device="cuda:0", capacity=64):
        self.ferns, self.grid, self.depth_scale = int(ferns), (int(grid[0]), int(grid[1])), float(depth_scale)
        self.device = torch.device(device)
        self.table_host = fern_table(self.ferns, *self.grid, seed, depth_lo, depth_hi, depth_scale)
        self.table = torch.from_numpy(self.table_host).to(self.device)
        self.words = self.ferns // 8
        self.database = torch.zeros((max(1, int(capacity)), self.words), dtype=torch.int32, device=self.device)
        self.ids = []
        self._query = torch.zeros(self.words, dtype=torch.int32, device=self.device)
        self._workspace = torch.empty(encode_workspace_size(*self.grid), dtype=torch.uint8, device=self.device)

    @classmethod
    def from_options(cls, opt, device):
        return cls(opt["ferns"], opt["grid"], opt["seed"], opt["depth_lo"], opt["depth_hi"], opt["depth_scale"], device)

    def __len__(self):
        return len(self.ids)

    def clear(self):
        self.ids = []

    def add(self, frame_id, image, depth=None, mask=None):
        row = len(self.ids)
        if row == self.database.shape[0]:
            grown = torch.zeros((2 * row, self.words), dtype=torch.int32, device=self.device)
            grown[:row] = self.database
            self.database = grown
        image, depth, mask = frame_tensors(image, depth, mask, self.device)
        encode(image, depth, mask, self.grid, self.table, self.depth_scale, self.database[row], self._workspace)
        self.ids.append(frame_id)

    def query(self, image, depth=None, mask=None, topk=4, nibble_mask=None, rows=None):
        """(best int32 [topk, 2], distance int32 [rows]) on the device. nibble_mask None: 0xF with a depth, 0x7 without (a frame that
        has no depth is compared on its colour bits alone). rows None: every row; otherwise only the first `rows` rows are searched (loop
        closure leaves out the newest keyframes)."""
        image, depth, mask = frame_tensors(image, depth, mask, self.device)
        encode(image, depth, mask, self.grid, self.table, self.depth_scale, self._query, self._workspace)
        rows = len(self.ids) if rows is None else max(0, min(int(rows), len(self.ids)))
        best = torch.empty((int(topk), 2), dtype=torch.int32, device=self.device)
        distance = torch.empty(rows, dtype=torch.int32, device=self.device)
        if nibble_mask is None:
            nibble_mask = 0x7 if depth is None else 0xF
        search(self.database if rows else None, rows, self._query, self.ferns, nibble_mask, topk, distance if rows else None, best)
        return best, distance


# ---- the verdict -------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def score(render_pkg, viewpoint, tau_colour=48, tau_depth=0.05, mask=None):
    """The counts of gsr_reloc_score (int32 [8] on the device, COUNTS) of a rendering against the frame `viewpoint` holds: its image, its
    sensor depth if it has one, `mask` (None: every pixel). Where the frame carries an exposure the rendering is compared as the tracking
    loss compares it, exp(a) * render + b (a = b = 0 leaves every value as it is). One launch and a memset node; the host reads nothing."""
    render = render_pkg["render"].detach()
    a, b = getattr(viewpoint, "exposure_a", None), getattr(viewpoint, "exposure_b", None)
    if a is not None and b is not None:
        render = torch.exp(a.detach()) * render + b.detach()
    dev = render.device
    H, W = int(render.shape[-2]), int(render.shape[-1])
    image, depth, mask = frame_tensors(viewpoint.original_image, viewpoint.depth_device(), mask, dev)
    counts = torch.empty(len(COUNTS), dtype=torch.int32, device=dev)
    score_counts(render.to(torch.float32).contiguous(), render_pkg["depth"].detach().reshape(H, W).contiguous(),
                 render_pkg["opacity"].detach().reshape(H, W).contiguous(), image, depth, mask, tau_colour, tau_depth, counts)
    return counts


def verdict(counts, opt):
    """The decision from the eight counts ON THE HOST (a list of ints): coverage = considered / masked, colour share = colour_ok /
    considered, depth share = depth_ok / depth_valid. Accepted: coverage >= min_coverage, colour share >= min_score, and -- where the frame
    has a depth at a considered pixel -- depth share >= min_score. A zero denominator refuses."""
    masked, considered, colour_ok, depth_valid, depth_ok = (int(v) for v in counts[:5])
    coverage = considered / masked if masked > 0 else 0.0
    colour = colour_ok / considered if considered > 0 else 0.0
    depth = depth_ok / depth_valid if depth_valid > 0 else None
    accepted = (masked > 0 and considered > 0 and coverage >= opt["min_coverage"] and colour >= opt["min_score"]
                and (depth is None or depth >= opt["min_score"]))
    return {"accepted": bool(accepted), "coverage": coverage, "colour_share": colour, "depth_share": depth}


# ---- relocalisation ----------------------------------------------------------------------------------------------------------------
class Relocaliser:
    """Finds the pose of a frame from nothing, against the keyframes of `index`.

    keyframes: {id: camera} -- pose (R, T) and time of every id the index holds; render_at(camera) -> render package of the map at that
    camera; track_from(viewpoint) -> render package: refines viewpoint's pose against the map from where it stands and renders there.
    The two callables keep the class ignorant of whether it serves a live run or a loaded map. size = (width, height), K = (fx, fy, cx,
    cy), opt = relocalisation_options(...); log: an EventLog that times every judge()'s score (default: none is kept). feature_seed:
    slam.features.feature_seed_options(...) or None -- with it the alignment of _seed starts at the pose of matched features
    (slam/features.py) and may move as far as that block's gate allows; static_map: the renderings at the keyframes never change (a loaded
    map), so their features are kept per keyframe id."""

    def __init__(self, index, keyframes, render_at, track_from, size, K, opt, log=None, feature_seed=None, static_map=False):
        from .odometry import DenseOdometry
        self.index, self.keyframes, self.render_at, self.track_from, self.opt = index, keyframes, render_at, track_from, opt
        self.log = EventLog("cpu") if log is None else log
        self.seeder, self.static_map = None, bool(static_map)
        gate = (opt["max_translation"], opt["max_rotation"])
        if feature_seed is not None:
            from .features import FeatureSeeder
            self.seeder = FeatureSeeder(size, K, feature_seed, index.device)
            gate = (max(gate[0], feature_seed["max_translation"]), max(gate[1], feature_seed["max_rotation"]))
        self.odometry = DenseOdometry(size[0], size[1], K, levels=opt["levels"], iters=opt["iters"], max_translation=gate[0],
                                      max_rotation=gate[1], device=index.device)

    @torch.no_grad()
    def _seed(self, viewpoint, keyframe, frame_features=None, key=None):
        """Place `viewpoint` at the keyframe's pose moved by the alignment of its image against the map rendered there; where the
        alignment's gate refuses, T is the identity and the pose is the keyframe's. With the feature seed on (frame_features: the frame's
        keypoints and descriptors) the alignment starts at the feature pose of the rendering and the frame -- the identity where that is
        refused, and then the alignment's own, narrower gate holds (features.gated). The frame's depth is None for a monocular frame, which
        the seeder takes with ``solver: pnp`` alone (it then never touches that depth). Device tensors throughout; nothing is read."""
        pkg = self.render_at(keyframe)
        depth = opaque_depth(pkg["depth"], pkg["opacity"])
        self.odometry.keep(pkg["render"], depth, None)
        if self.seeder is None:
            T, _ = self.odometry.align(viewpoint.original_image)
        else:
            from .features import gated
            there = self.seeder.cached(key, pkg["render"]) if self.static_map else self.seeder.features(pkg["render"])
            start, seed_stats = self.seeder.pose(there, depth, frame_features, viewpoint.depth_device())
            T, stats = self.odometry.align(viewpoint.original_image, T_init=start)
            T, _ = gated(T, stats[0], seed_stats[6], self.opt["max_translation"], self.opt["max_rotation"])
        viewpoint.update_RT(*compose_pose(T, keyframe.R, keyframe.T))

    def judge(self, viewpoint, render_pkg, fallback, mask=None):
        """Is the tracked frame where `render_pkg` shows the map? One gsr_reloc_score launch and ONE host read, its eight counts. Accepted:
        nothing else happens. Refused: the frame gets the pose `fallback` = (R, T) and localise() looks for it among the keyframes. Returns
        localise()'s dictionary: accepted with "keyframe" None: tracked; with a keyframe: relocalised there; not accepted: lost."""
        opt = self.opt
        with self.log.timed():
            counts = score(render_pkg, viewpoint, opt["tau_colour"], opt["tau_depth"], mask)
        counts = counts.tolist()
        if verdict(counts, opt)["accepted"]:
            return {"accepted": True, "keyframe": None, "candidates_tried": 0, "counts": counts, "distance": None}
        viewpoint.update_RT(*fallback)
        return self.localise(viewpoint, mask)

    def localise(self, viewpoint, mask=None):
        """Encode the frame, search the index, and try the candidates in the order of `best`: seed the pose at the candidate (_seed),
        track_from, score the rendering at the result, verdict; the first accepted candidate ends the search. Host reads: `best` once per
        call (the candidates to render), and per candidate the verdict's eight ints -- that is the ONE read per candidate. Returns
        {"accepted", "keyframe" (id or None), "candidates_tried", "counts" (of the last candidate tried, or None), "distance" (of that
        candidate, or None)}; on refusal the frame's pose (and exposure) is what it was on entry."""
        opt = self.opt
        R0, T0 = viewpoint.R.detach().clone(), viewpoint.T.detach().clone()
        exposure0 = [p.detach().clone() for p in (viewpoint.exposure_a, viewpoint.exposure_b)]
        out = {"accepted": False, "keyframe": None, "candidates_tried": 0, "counts": None, "distance": None}
        best, _ = self.index.query(viewpoint.original_image, viewpoint.depth_device(), mask, opt["topk"])
        frame_features = None if self.seeder is None else self.seeder.features(viewpoint.original_image, mask)
        for row, distance in best.tolist():
            if row < 0:
                break
            frame_id = self.index.ids[row]
            self._seed(viewpoint, self.keyframes[frame_id], frame_features, frame_id)
            pkg = self.track_from(viewpoint)
            counts = score(pkg, viewpoint, opt["tau_colour"], opt["tau_depth"], mask).tolist()
            out.update(candidates_tried=out["candidates_tried"] + 1, counts=counts, distance=distance)
            if verdict(counts, opt)["accepted"]:
                out.update(accepted=True, keyframe=frame_id)
                return out
        viewpoint.update_RT(R0, T0)
        with torch.no_grad():
            viewpoint.exposure_a.copy_(exposure0[0])
            viewpoint.exposure_b.copy_(exposure0[1])
        return out


# ---- a saved map -------------------------------------------------------------------------------------------------------------------
class MapLocaliser:
    """Localises frames in a map_io.LoadedMap, which is never modified. The index is built from renderings of the map at its keyframe
    poses and times (a loaded map holds no images), in chunks through Playback.render; their depth is the rendered depth where the opacity
    is above 0.5. config: the run's configuration (default: slam.system.default_config()); its Training.relocalisation block is read
    whether or not it is enabled. A dynamic map is refused."""

    def __init__(self, loaded_map, config=None):
        from .playback import Playback, _w2c
        from .system import default_config
        if loaded_map.dynamic:
            raise ValueError("MapLocaliser: the map is dynamic (its node network is initialised); localisation in dynamic saved maps is not "
                             "supported")
        if not loaded_map.kf_indices:
            raise ValueError("MapLocaliser: the map has no keyframe")
        self.map = loaded_map
        self.config = default_config() if config is None else config
        training = self.config["Training"]
        training.setdefault("monocular", self.config["Dataset"].get("sensor_type") == "monocular")
        self.opt = relocalisation_options({"relocalisation": {**(training.get("relocalisation") or {}), "enabled": True}})
        from .features import feature_seed_options
        self.feature_seed = feature_seed_options({**training, "relocalisation": {"enabled": True}})      # None unless its block is on
        self.device = torch.device(loaded_map.device)
        self.keyframes = {k: loaded_map.cameras[k] for k in loaded_map.kf_indices}
        first = self.keyframes[loaded_map.kf_indices[0]]
        self.size = (int(first.image_width), int(first.image_height))
        self.K = (first.fx, first.fy, first.cx, first.cy)
        self.index = KeyframeIndex.from_options(self.opt, self.device)
        cams = [self.keyframes[k] for k in loaded_map.kf_indices]
        colour, depth, opacity = Playback(loaded_map).render(_w2c(cams), [float(c.time) for c in cams])
        for i, k in enumerate(loaded_map.kf_indices):
            self.index.add(k, colour[i], opaque_depth(depth[i, 0], opacity[i, 0]), None)
        self._tracker = None
        self.relocaliser = Relocaliser(self.index, self.keyframes, self._render_at, self._track_from, self.size, self.K, self.opt,
                                       feature_seed=self.feature_seed, static_map=True)

    @torch.no_grad()
    def _render_at(self, camera):
        from gaussian_renderer import render
        return render(camera, self.map.gaussians, self.map.pipeline_params, self.map.background, dynamic=False)

    def _track_from(self, viewpoint):
        """The front-end's tracking of one frame (TrackingGraph.run_eager) on the loaded Gaussians."""
        from .tracking_graph import TrackingGraph
        training = self.config["Training"]
        if self._tracker is None:
            self._tracker = TrackingGraph(self.map.gaussians, self.map.pipeline_params, self.map.background, self.config, viewpoint)
        self._tracker.load(viewpoint)
        self._tracker.run_eager(int(training["tracking_itr_num"]), int(training.get("converge_check_every", 5)))
        self._tracker.store(viewpoint)
        return self._render_at(viewpoint)

    def camera(self, dataset, idx):
        """The frame `idx` of a dataset as a Camera ready to be localised (its pose is the identity until localise() sets it)."""
        viewpoint = Camera.init_from_dataset(dataset, idx, dataset.projection_matrix)
        viewpoint.compute_grad_mask(self.config)
        return viewpoint

    def localise(self, viewpoint):
        """Relocaliser.localise against the loaded map: the frame's pose on entry does not matter."""
        return self.relocaliser.localise(viewpoint)

    def follow(self, dataset, frames):
        """Tracking only: the first frame is localised from nothing; every later one starts at the previous frame's pose, is tracked and
        scored (one host read), and is relocalised when the verdict refuses it; a frame that stays refused keeps the previous pose. Returns
        {"poses": float32 [N, 4, 4] world-to-camera, "status": per frame "localised" | "tracked" | "relocalised" | "lost", "frames",
        "ate_rmse": against the dataset's ground truth over the frames that are not lost, None without one or with fewer than three}."""
        from .eval_utils import ate_rmse
        poses, status, gts = [], [], []
        previous = None
        for idx in frames:
            viewpoint = self.camera(dataset, idx)
            if previous is None:
                found, state = self.localise(viewpoint), "localised"
            else:
                viewpoint.update_RT(*previous)
                found = self.relocaliser.judge(viewpoint, self._track_from(viewpoint), previous)
                state = "tracked" if found["keyframe"] is None else "relocalised"
            if found["accepted"]:
                previous = (viewpoint.R.detach().clone(), viewpoint.T.detach().clone())
            else:
                state = "lost"
            pose = torch.eye(4)
            pose[:3, :3], pose[:3, 3] = viewpoint.R.detach().cpu(), viewpoint.T.detach().cpu()
            gt = torch.eye(4)
            gt[:3, :3], gt[:3, 3] = viewpoint.R_gt.detach().cpu(), viewpoint.T_gt.detach().cpu()
            poses.append(pose)
            gts.append(gt)
            status.append(state)
            viewpoint.clean()
        kept = [i for i, s in enumerate(status) if s != "lost"]
        ate = None
        if len(kept) >= 3:
            c2w = lambda m: np.linalg.inv(m.numpy().astype(np.float64))
            ate = ate_rmse([c2w(gts[i]) for i in kept], [c2w(poses[i]) for i in kept])
        out = {"poses": torch.stack(poses) if poses else torch.zeros((0, 4, 4)), "status": status, "frames": list(frames), "ate_rmse": ate}
        if self.relocaliser.seeder is not None:
            out.update(self.relocaliser.seeder.summary())
        return out
