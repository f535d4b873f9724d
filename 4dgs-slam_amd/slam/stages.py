"""The optional stages of the front-end, one object each: ``SweepSeeding`` (``Training.mono_sweep``), ``PosePrior`` (``Training.pose_prior``
with ``Training.pose_prior_terms``), ``Relocalisation`` (``Training.relocalisation``) and ``LoopClosure`` (``Training.loop_closure``). Each owns its checked options (``.options``), the device object it builds at its first
use (slam/sweep.py and slam/odometry.py are not imported before that), the device time of its calls and the ``summary()`` a run reports.
What couples two stages (a lost frame drops the prior's kept frame) is left to ``FrontEnd``. Imports without a GPU."""
import torch

from .camera import compose_pose, opaque_depth
from .options import check_gate, check_pass_counts, read_block, to_floats
from .pretrained import EventLog
from .features import feature_seed_options  # noqa: F401  (Training.feature_seed: read here with its neighbours, defined beside its stage object)
from .relocalise import DEFAULT_ITERS, MAX_TOPK, KeyframeIndex, Relocaliser, relocalisation_options


# ---- Training.mono_sweep: a monocular keyframe's seed depth from a plane sweep over the window ---------------------------------------------
MONO_SWEEP_DEFAULTS = {"enabled": False, "partners": 3, "near": 0.25, "p1": 10, "p2": 120, "uniqueness_ratio": 40, "min_span_px": 8}


def mono_sweep_options(training):
    """The ``Training.mono_sweep`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys and values the
    sweep cannot take are refused here, before the run starts."""
    opt = read_block(training, "mono_sweep", MONO_SWEEP_DEFAULTS)
    if opt is None:
        return None
    opt = {"enabled": True, "near": float(opt["near"]), **{k: int(opt[k]) for k in ("partners", "p1", "p2", "uniqueness_ratio", "min_span_px")}}
    if not 1 <= opt["partners"] <= 4:
        raise ValueError(f"Training.mono_sweep.partners must be 1 to 4, got {opt['partners']}")
    if not (0.0 < opt["near"] <= 1.0):
        raise ValueError(f"Training.mono_sweep.near must be in (0, 1] (the nearest swept depth as a share of the median), got {opt['near']}")
    if not (0 < opt["p1"] < opt["p2"] <= 2047) or not 0 <= opt["uniqueness_ratio"] <= 99 or opt["min_span_px"] < 0:
        raise ValueError("Training.mono_sweep needs 0 < p1 < p2 <= 2047, 0 <= uniqueness_ratio <= 99 and min_span_px >= 0, got "
                         f"p1 {opt['p1']}, p2 {opt['p2']}, uniqueness_ratio {opt['uniqueness_ratio']}, min_span_px {opt['min_span_px']}")
    return opt


def merge_sweep_depth(sweep_depth, sweep_valid, gt_img, rgb_boundary_threshold, fallback):
    """The seed depth of a swept keyframe: the sweep's where it is valid and the pixel passes the RGB boundary threshold, else the fallback."""
    use = sweep_valid & (gt_img.sum(dim=0) > rgb_boundary_threshold)
    return torch.where(use, sweep_depth, fallback)


class SweepSeeding:
    def __init__(self, options):
        self.options = options
        self.sweeper = None                   # slam.sweep.PlaneSweep, built at the first keyframe swept
        self.shares, self.log = [], EventLog("cuda")      # per swept keyframe its valid share, a device scalar, and its device time

    def seed_depth(self, gt_img, fallback, median, threshold, window):
        """The new keyframe's depth from a plane sweep (slam/sweep.py, include/multiview_depth.h) against the most recent `partners`
        keyframes of `window` (its cameras, the new keyframe first) under their tracked poses, inverse depth 0 .. 1 / (near * median) in 63
        steps, merged with `fallback` (merge_sweep_depth). Nothing is read by the host: the valid share stays on the device until summary()."""
        opt = self.options
        newest = window[0]
        partners = [cam for cam in window[1:1 + opt["partners"]] if cam.original_image is not None]
        if not partners or not (median > 0.0 and median < float("inf")):
            return fallback
        if self.sweeper is None:
            from .sweep import PlaneSweep
            self.sweeper = PlaneSweep(p1=opt["p1"], p2=opt["p2"], uniqueness_ratio=opt["uniqueness_ratio"], min_span_px=opt["min_span_px"],
                                      device=gt_img.device)
        with self.log.timed():
            swept = self.sweeper.sweep(gt_img, [cam.original_image for cam in partners], (newest.fx, newest.fy, newest.cx, newest.cy),
                                       self.sweeper.relative_transforms(newest, partners), 0.0, 1.0 / (opt["near"] * median * 63.0))
        self.shares.append(swept["valid"].float().mean())
        return merge_sweep_depth(swept["depth"], swept["valid"], gt_img, threshold, fallback)

    def summary(self):
        """The `sweep` block of the run result: keyframes swept, their mean valid share, device ms per keyframe."""
        share = float(torch.stack(self.shares).mean()) if self.shares else 0.0
        return {"keyframes": len(self.shares), "valid_share": share, "device_ms_per_keyframe": self.log.summary()["ms_per_item"] or 0.0}


# ---- Training.pose_prior: the start of a frame's tracking from dense frame-to-frame alignment ----------------------------------------------
POSE_PRIOR_DEFAULTS = {"enabled": False, "levels": 3, "iters": [5, 7, 10], "nu": 5.0, "sigma_init": 0.1, "sigma_min": 1e-3, "min_share": 0.3,
                       "max_last_step": 1e-2, "max_translation": 0.5, "max_rotation": 20.0, "depth_min": 0.0, "depth_max": 1e6,
                       "constant_velocity": False}


def pose_prior_options(training):
    """The ``Training.pose_prior`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys and values the
    alignment cannot take are refused here, before the run starts. max_translation is in metres (monocular input: map units), max_rotation
    in degrees; iters lists the passes per level, finest first."""
    name = "Training.pose_prior"
    opt = read_block(training, "pose_prior", POSE_PRIOR_DEFAULTS)
    if opt is None:
        return None
    opt["constant_velocity"], opt["levels"] = bool(opt["constant_velocity"]), int(opt["levels"])
    if not 1 <= opt["levels"] <= 6:
        raise ValueError(f"{name}.levels must be 1 to 6, got {opt['levels']}")
    if "iters" not in training["pose_prior"] and opt["levels"] != POSE_PRIOR_DEFAULTS["levels"]:
        raise ValueError(f"{name}.iters must be given with levels = {opt['levels']}: one count per level, finest first")
    check_pass_counts(opt, name)
    to_floats(opt, name, ("nu", "sigma_init", "sigma_min", "min_share", "max_last_step", "max_translation", "max_rotation", "depth_min", "depth_max"))
    for key in ("nu", "sigma_init", "sigma_min"):
        if not (0.0 < opt[key] < float("inf")):
            raise ValueError(f"{name}.{key} must be positive and finite, got {opt[key]}")
    if not 0.0 <= opt["min_share"] <= 1.0:
        raise ValueError(f"{name}.min_share must be in [0, 1], got {opt['min_share']}")
    check_gate(opt, name, ("max_last_step", "max_translation", "max_rotation"))
    if not 0.0 <= opt["depth_min"] <= opt["depth_max"]:
        raise ValueError(f"{name} needs 0 <= depth_min <= depth_max, got {opt['depth_min']} and {opt['depth_max']}")
    return opt


# ---- Training.pose_prior_terms: what the alignment of Training.pose_prior models besides brightness constancy ------------------------------
POSE_PRIOR_TERMS_DEFAULTS = {"enabled": False, "affine": True, "geometric_weight": 1.0, "edge_ratio": 0.05, "sigma_depth_init": 0.02,
                             "sigma_depth_min": 1e-4, "max_gain": 0.5, "max_offset": 0.3, "against": "previous"}


def pose_prior_terms_options(training):
    """The ``Training.pose_prior_terms`` block with its defaults filled in, or None when it is absent or not enabled: an affine brightness
    between the two frames (affine), an inverse-depth term against the current frame's depth (geometric_weight > 0; sigma_depth_* in
    1 / metres) and the frame aligned against (against: previous or keyframe). It needs ``Training.pose_prior`` enabled."""
    name = "Training.pose_prior_terms"
    opt = read_block(training, "pose_prior_terms", POSE_PRIOR_TERMS_DEFAULTS)
    if opt is None:
        return None
    if not (training.get("pose_prior") or {}).get("enabled", False):
        raise ValueError(f"{name} is enabled but Training.pose_prior is not: the terms belong to its alignment")
    opt["affine"] = bool(opt["affine"])
    to_floats(opt, name, ("geometric_weight", "edge_ratio", "sigma_depth_init", "sigma_depth_min", "max_gain", "max_offset"))
    for key in ("geometric_weight", "edge_ratio"):
        if not (0.0 <= opt[key] < float("inf")):
            raise ValueError(f"{name}.{key} must be finite and not negative, got {opt[key]}")
    for key in ("sigma_depth_init", "sigma_depth_min"):
        if not (0.0 < opt[key] < float("inf")):
            raise ValueError(f"{name}.{key} must be positive and finite, got {opt[key]}")
    for key in ("max_gain", "max_offset"):
        if opt[key] < 0.0:
            raise ValueError(f"{name}.{key} must not be negative, got {opt[key]}")
    if opt["against"] not in ("previous", "keyframe"):
        raise ValueError(f"{name}.against must be 'previous' or 'keyframe', got {opt['against']!r}")
    if not opt["affine"] and opt["geometric_weight"] == 0.0 and opt["against"] == "previous":
        raise ValueError(f"{name} is enabled with affine off, geometric_weight 0 and against = previous: it would change nothing")
    return opt


class PosePrior:
    def __init__(self, options, monocular, dynamic_model, terms=None):
        self.options, self.monocular, self.dynamic_model, self.terms = options, monocular, dynamic_model, terms
        # slam.odometry.DenseOdometry, built with the first frame that is kept; the last aligned motion, where the next alignment starts
        # with constant_velocity
        self.odometry = self.motion = None
        # terms.against = keyframe: the camera of the kept frame (its pose is read when a frame is aligned, after the back-end moved it)
        self.anchor = None

    @property
    def against_keyframe(self):
        return self.terms is not None and self.terms["against"] == "keyframe"

    def keep(self, viewpoint, render_pkg=None):
        """Keep `viewpoint` as the frame the next one is aligned against. Its depth: the sensor's (RGB-D) or the matcher's (stereo); for
        monocular input the depth of `render_pkg` where its opacity is above 0.5 (None: the map does not exist yet, nothing is kept).
        Against keyframes a frame is kept only while none is: keyframe() and restart() replace the kept one."""
        if self.against_keyframe and self.anchor is not None and self.odometry is not None and self.odometry.has_previous:
            return
        if self.odometry is None:
            from .odometry import DenseOdometry
            options = {k: v for k, v in self.options.items() if k not in ("enabled", "constant_velocity")}
            if self.terms is not None:            # a monocular frame has no depth when it is aligned: photometric and affine alone
                options.update({k: v for k, v in self.terms.items() if k not in ("enabled", "against")})
                options["geometric_weight"] = 0.0 if self.monocular else options["geometric_weight"]
            self.odometry = DenseOdometry(viewpoint.image_width, viewpoint.image_height, (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy),
                                          device=viewpoint.device, **options)
        depth = viewpoint.depth_device()
        if self.monocular:
            depth = None if render_pkg is None else opaque_depth(render_pkg["depth"], render_pkg["opacity"])
        if depth is None:
            self.odometry.drop()
            self.anchor = None
            return
        self.odometry.keep(viewpoint.original_image, depth, viewpoint.motion_mask if self.dynamic_model else None)
        if self.against_keyframe:
            self.anchor, self.motion = viewpoint, None

    def keyframe(self, viewpoint, render_pkg=None):
        """The front-end made `viewpoint` a keyframe: against keyframes it replaces the kept frame, and the next alignment starts at identity."""
        if self.against_keyframe:
            self.anchor = None
            self.keep(viewpoint, render_pkg)

    def restart(self, viewpoint):
        """A map that starts (over): the last motion is forgotten and `viewpoint`, its first frame, replaces the kept frame."""
        self.motion = self.anchor = None
        self.keep(viewpoint)

    def drop(self):
        """The next frame is not aligned against the kept one (a lost frame: it has no pose of its own). A kept keyframe has a pose: it stays."""
        if self.odometry is not None and not self.against_keyframe:
            self.odometry.drop()

    def start(self, viewpoint, previous):
        """Move `viewpoint` from the previous frame's pose W2C_prev to T W2C_prev, T the aligned motion (identity where the gate refused it:
        the reference's start); with no frame kept it stays where it is. Device tensors throughout; the host reads nothing. Against a
        keyframe the alignment starts at the last accepted motion against it and an accepted T moves `viewpoint` to T W2C_keyframe."""
        if self.odometry is None or not self.odometry.has_previous:
            return
        if self.terms is None:
            self.motion, _ = self.odometry.align(viewpoint.original_image, self.motion if self.options["constant_velocity"] else None)
            viewpoint.update_RT(*compose_pose(self.motion, previous.R, previous.T))
            return
        depth = None if self.monocular else viewpoint.depth_device()
        mask = viewpoint.motion_mask if self.dynamic_model and depth is not None else None
        if not self.against_keyframe:
            start = self.motion if self.options["constant_velocity"] else None
            self.motion, _ = self.odometry.align(viewpoint.original_image, start, depth=depth, mask=mask)
            viewpoint.update_RT(*compose_pose(self.motion, previous.R, previous.T))
            return
        T, stats = self.odometry.align(viewpoint.original_image, self.motion, depth=depth, mask=mask)
        accepted = stats[0] > 0.5                                            # stays on the device
        R, t = compose_pose(T, self.anchor.R, self.anchor.T)
        viewpoint.update_RT(torch.where(accepted, R, previous.R.to(R)), torch.where(accepted, t, previous.T.to(t)))
        self.motion = T if self.motion is None else torch.where(accepted, T, self.motion)

    def summary(self):
        """The `odometry` block of the run result: frames aligned, the accepted share, the mean inlier share, device ms per frame. With
        Training.pose_prior_terms on also the mean |alpha| and |beta|, the share of aligned pixels with a depth term, and `against`."""
        if self.odometry is None:
            out = {"frames": 0, "accepted_share": 0.0, "inlier_share": 0.0, "device_ms_per_frame": 0.0}
            if self.terms is not None:
                out.update(mean_abs_alpha=0.0, mean_abs_beta=0.0, depth_term_share=0.0)
        else:
            out = self.odometry.summary()
        if self.terms is not None:
            out["against"] = self.terms["against"]
            if self.monocular:
                out["depth_term"] = "off: a monocular frame has no depth when it is aligned"
        return out


# ---- Training.relocalisation: is the tracked frame lost, and if so where is it ------------------------------------------------------------
class Relocalisation:
    def __init__(self, options, dynamic_model, feature_seed=None):
        self.options, self.dynamic_model, self.feature_seed = options, dynamic_model, feature_seed     # feature_seed_options(...) or None
        self.index = self.relocaliser = None                  # built with the first map, on the device
        self.stats, self.log = {"scored": 0, "lost": 0, "relocalised": 0}, EventLog("cuda")

    def restart(self, frame_idx, viewpoint, cameras, render_at, track_from):
        """A map that starts (over) with the keyframe `viewpoint` forgets the places of the old one. The rest is what Relocaliser works with."""
        if self.index is None:
            self.index = KeyframeIndex.from_options(self.options, viewpoint.device)
            self.relocaliser = Relocaliser(self.index, cameras, render_at, track_from, (viewpoint.image_width, viewpoint.image_height),
                                           (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy), self.options, self.log,
                                           **({} if self.feature_seed is None else {"feature_seed": self.feature_seed}))
        self.index.clear()
        self.add(frame_idx, viewpoint)

    def add(self, frame_idx, viewpoint):
        """The new keyframe's real frame into the place index: one encode into the next row of the device database."""
        self.index.add(frame_idx, viewpoint.original_image, viewpoint.depth_device(), viewpoint.motion_mask if self.dynamic_model else None)

    def judge(self, viewpoint, render_pkg, fallback):
        """Relocaliser.judge of the tracked frame, counted: its result tells accepted, relocalised and lost apart."""
        found = self.relocaliser.judge(viewpoint, render_pkg, fallback, viewpoint.motion_mask if self.dynamic_model else None)
        self.stats["scored"] += 1
        if not found["accepted"]:
            self.stats["lost"] += 1
        elif found["keyframe"] is not None:
            self.stats["relocalised"] += 1
        return found

    def summary(self):
        """The `relocalisation` block of the run result: frames scored, lost, relocalised, device ms per score; with the feature seed on
        also feature_seeds_tried and feature_seeds_accepted."""
        out = {**self.stats, "device_ms_per_score": self.log.summary()["ms_per_item"] or 0.0}
        if self.feature_seed is not None:
            seeder = self.relocaliser and self.relocaliser.seeder
            out.update(seeder.summary() if seeder else {"feature_seeds_tried": 0, "feature_seeds_accepted": 0})
        return out


# ---- Training.loop_closure: tie a keyframe to the old keyframes that saw the same place, and correct poses and map ------------------------
# max_code_distance lies between the code distances measured on the synthetic sequence (step 0.02, rot_step 0.012) of frames one or two apart
# (at most 0.27 of the ferns) and of frames ten or more apart (at least 0.49); consistency between the two-way inconsistency of true pairs
# (at most 1.7 mm and 0.021 degrees) and of an accepted alignment of two different places (234 mm, 7.6 degrees): DESIGN.md section 8, Loop
# closure. The weights have not been measured. The fern keys default to those of Training.relocalisation (None here: "as that block, or its
# defaults")
FERN_KEYS = ("ferns", "grid", "seed", "depth_scale", "depth_lo", "depth_hi")
LOOP_CLOSURE_DEFAULTS = {"enabled": False, **{k: None for k in FERN_KEYS}, "min_gap": 10, "topk": 2, "max_code_distance": 0.38,
                         "consistency": [0.02, 1.0], "min_correction": [0.005, 0.2], "odometry_weights": [1.0, 1.0],
                         "loop_weights": [10.0, 10.0], "outer_iters": 10, "cg_iters": 200, "lambda": 1e-6, "step_tolerance": 1e-9,
                         "levels": 4, "iters": None, "max_translation": 1.0, "max_rotation": 30.0, "geometric_weight": 1.0}


def _pair(opt, name, key, what):
    v = opt[key]
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2:
        raise ValueError(f"{name}.{key} must be [{what}], got {v!r}")
    opt[key] = [float(v[0]), float(v[1])]
    if not all(0.0 <= x < float("inf") for x in opt[key]):
        raise ValueError(f"{name}.{key} must hold two finite numbers that are not negative, got {v!r}")


def loop_closure_options(training, dynamic_model=False, ranks=1):
    """The ``Training.loop_closure`` block with its defaults filled in, or None when it is absent or not enabled. Unknown keys, values the
    kernels or the alignment cannot take, and the runs loop closure cannot serve are refused here, before the run starts. The fern keys
    (ferns, grid, seed, depth_scale, depth_lo, depth_hi) are those of ``Training.relocalisation`` and, with that stage on, must not differ
    from it: the two stages share one place index. consistency and min_correction are [metres, degrees]; the weights are [w_t, w_r];
    max_code_distance is a share of the ferns; iters lists the alignment's passes per level, finest first."""
    name = "Training.loop_closure"
    opt = read_block(training, "loop_closure", LOOP_CLOSURE_DEFAULTS)
    if opt is None:
        return None
    if training.get("monocular", False):
        raise ValueError(f"{name} cannot be used with monocular input: the drift of an RGB-only run includes scale, and correcting that needs "
                         "Sim(3) constraints; this pose graph is SE(3)")
    if dynamic_model:
        raise ValueError(f"{name} cannot be used with model_params.dynamic_model: the deformation field lives in world coordinates and cannot "
                         "be moved piecewise with the keyframes")
    if training.get("spherical_harmonics", False):
        raise ValueError(f"{name} cannot be used with Training.spherical_harmonics: the coefficients of degree 1 and higher would have to be "
                         "rotated with the Gaussians")
    if int(ranks) > 1:
        raise ValueError(f"{name} cannot be used with a sharded back-end of {int(ranks)} ranks: the correction is applied to one copy of the map")
    reloc = relocalisation_options(training)                               # checked by its own rules; None when that stage is off
    given = {k: opt[k] for k in FERN_KEYS if opt[k] is not None}
    ferns = relocalisation_options({"relocalisation": {"enabled": True, **given}}) if reloc is None else reloc
    norm = lambda key, v: [int(x) for x in v] if key == "grid" else float(v)
    for key in FERN_KEYS:
        if reloc is not None and key in given and norm(key, given[key]) != norm(key, reloc[key]):
            raise ValueError(f"{name}.{key} = {given[key]!r} differs from Training.relocalisation.{key} = {reloc[key]!r}: the two stages share one "
                             "place index")
        opt[key] = ferns[key]
    for key in ("min_gap", "topk", "outer_iters", "cg_iters", "levels"):
        if isinstance(opt[key], float) and not opt[key].is_integer():
            raise ValueError(f"{name}.{key} must be an integer, got {opt[key]!r}")
        opt[key] = int(opt[key])
    if opt["min_gap"] < 1:
        raise ValueError(f"{name}.min_gap must be at least 1, got {opt['min_gap']}")
    if not 1 <= opt["topk"] <= MAX_TOPK:
        raise ValueError(f"{name}.topk must be 1 to {MAX_TOPK}, got {opt['topk']}")
    if not 0 <= opt["outer_iters"] <= 1000:
        raise ValueError(f"{name}.outer_iters must be in [0, 1000], got {opt['outer_iters']}")
    if not 1 <= opt["cg_iters"] <= 100000:
        raise ValueError(f"{name}.cg_iters must be in [1, 100000], got {opt['cg_iters']}")
    to_floats(opt, name, ("max_code_distance", "lambda", "step_tolerance", "max_translation", "max_rotation", "geometric_weight"))
    if not 0.0 <= opt["max_code_distance"] <= 1.0:
        raise ValueError(f"{name}.max_code_distance is a share of the ferns and must be in [0, 1], got {opt['max_code_distance']}")
    for key in ("lambda", "step_tolerance"):
        if not 0.0 <= opt[key] < float("inf"):
            raise ValueError(f"{name}.{key} must be finite and not negative, got {opt[key]}")
    if not 0.0 < opt["geometric_weight"] < float("inf"):
        raise ValueError(f"{name}.geometric_weight must be positive and finite (verification aligns colour and depth), got {opt['geometric_weight']}")
    _pair(opt, name, "consistency", "metres, degrees")
    _pair(opt, name, "min_correction", "metres, degrees")
    _pair(opt, name, "odometry_weights", "w_t, w_r")
    _pair(opt, name, "loop_weights", "w_t, w_r")
    for key in ("odometry_weights", "loop_weights"):
        if min(opt[key]) <= 0.0:
            raise ValueError(f"{name}.{key} must be positive, got {opt[key]}")
    if not 1 <= opt["levels"] <= 6:
        raise ValueError(f"{name}.levels must be 1 to 6, got {opt['levels']}")
    if opt["iters"] is None:
        opt["iters"] = list(DEFAULT_ITERS[:opt["levels"]])
    check_pass_counts(opt, name)
    check_gate(opt, name, ("max_translation", "max_rotation"))
    return opt


class LoopClosure:
    def __init__(self, options, feature_seed=None):
        self.options, self.feature_seed = options, feature_seed                                         # feature_seed_options(...) or None
        self.closer = None                                    # slam.loop_closure.LoopCloser, built with the first map, on the device

    def restart(self, frame_idx, viewpoint, cameras, get_gaussians, index=None, ranks=1):
        """A map that starts (over) with the keyframe `viewpoint`: the graph (and an owned index) is emptied; the first keyframe is node 0.
        index: the place index of the relocalisation stage when that is on -- it holds `viewpoint` already -- else None."""
        if int(ranks) > 1:
            raise ValueError(f"Training.loop_closure cannot be used with a sharded back-end of {int(ranks)} ranks: the correction is applied to "
                             "one copy of the map")
        if self.closer is None:
            from .loop_closure import LoopCloser
            self.closer = LoopCloser(self.options, cameras, get_gaussians, (viewpoint.image_width, viewpoint.image_height),
                                     (viewpoint.fx, viewpoint.fy, viewpoint.cx, viewpoint.cy), viewpoint.device, index,
                                     **({} if self.feature_seed is None else {"feature_seed": self.feature_seed}))
        self.closer.clear()
        self.closer.on_keyframe(frame_idx, viewpoint)

    def on_keyframe(self, frame_idx, viewpoint):
        """LoopCloser.on_keyframe of the new keyframe: None, or the dictionary of a solve (its "applied" says whether map and poses moved)."""
        return self.closer.on_keyframe(frame_idx, viewpoint)

    def summary(self):
        """The `loop_closure` block of the run result: keyframes queried, candidates verified, edges accepted, solves, corrections applied,
        the largest correction, device ms per verify and per solve."""
        if self.closer is None:
            seeds = {} if self.feature_seed is None else {"feature_seeds_tried": 0, "feature_seeds_accepted": 0}
            return {"keyframes_queried": 0, "candidates_verified": 0, "edges_accepted": 0, "solves": 0, "corrections_applied": 0,
                    "max_correction_m": 0.0, "max_correction_deg": 0.0, **seeds, "device_ms_per_verify": 0.0, "device_ms_per_solve": 0.0}
        return self.closer.summary()
