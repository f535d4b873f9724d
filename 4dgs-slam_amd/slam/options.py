"""Reading an optional ``Training.<key>`` block (mono_sweep, pose_prior, relocalisation, loop_closure) and the checks more than one of them makes. Every
refusal names the block and the key. Imports without a GPU or the HIP library."""
import math


def read_block(training, key, defaults):
    """The ``Training.<key>`` block over its defaults, or None when it is absent or not enabled. Unknown keys are refused."""
    block = training.get(key)
    if not block or not block.get("enabled", False):
        return None
    unknown = sorted(set(block) - set(defaults))
    if unknown:
        raise ValueError(f"Training.{key}: unknown keys {unknown} (known: {sorted(defaults)})")
    return {**defaults, **block, "enabled": True}


def to_floats(opt, name, keys):
    """opt[key] as a float for every key; NaN is refused."""
    for key in keys:
        opt[key] = float(opt[key])
        if math.isnan(opt[key]):
            raise ValueError(f"{name}.{key} must be a number, got nan")


def check_pass_counts(opt, name):
    """opt["iters"]: a list of opt["levels"] pass counts in [0, 64], finest first."""
    if isinstance(opt["iters"], (str, bytes)) or not hasattr(opt["iters"], "__len__"):
        raise ValueError(f"{name}.iters must be a list of {opt['levels']} pass counts, finest first, got {opt['iters']!r}")
    opt["iters"] = [int(v) for v in opt["iters"]]
    if len(opt["iters"]) != opt["levels"] or not all(0 <= v <= 64 for v in opt["iters"]):
        raise ValueError(f"{name}.iters must hold {opt['levels']} pass counts in [0, 64], finest first, got {opt['iters']}")


def check_gate(opt, name, keys):
    """The alignment's gate (max_translation, max_rotation in degrees, ...): floats that must not be negative, the rotation at most 180."""
    for key in keys:
        if opt[key] < 0.0:
            raise ValueError(f"{name}.{key} must not be negative, got {opt[key]}")
    if opt["max_rotation"] > 180.0:
        raise ValueError(f"{name}.max_rotation is in degrees and must not exceed 180, got {opt['max_rotation']}")
