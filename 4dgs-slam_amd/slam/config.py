"""Configuration files with the reference's YAML structure (utils/config_utils.py): ``yaml.full_load``, a recursive ``inherit_from`` and
``update_recursive`` merging, then merged over ``slam.system.default_config()`` so that keys only this project has keep their defaults.

The reference resolves ``inherit_from`` against the current directory (its files say ``"configs/rgbd/tum/base_config.yaml"``). Here the
path is tried as given, then relative to the including file's directory, then relative to each ancestor of that directory, so a config
of a 4DGS-SLAM checkout loads from any working directory."""
import os

import yaml

from .system import default_config


def update_recursive(dict1, dict2):
    """utils/config_utils.py update_recursive: dict1 is updated in place by dict2 (a dict value merges key by key)."""
    for k, v in dict2.items():
        if k not in dict1:
            dict1[k] = dict()
        if isinstance(v, dict):
            update_recursive(dict1[k], v)
        else:
            dict1[k] = v
    return dict1


def resolve_inherit(inherit_from, including_file):
    """The file an ``inherit_from`` names: as given, then relative to the including file's directory and each of its ancestors."""
    tried = [inherit_from]
    if os.path.isfile(inherit_from):
        return inherit_from
    if not os.path.isabs(inherit_from):
        d = os.path.dirname(os.path.abspath(including_file))
        while True:
            cand = os.path.join(d, inherit_from)
            tried.append(cand)
            if os.path.isfile(cand):
                return cand
            parent = os.path.dirname(d)
            if parent == d:
                break
            d = parent
    raise FileNotFoundError(f"inherit_from {inherit_from!r} in {including_file}: no such file; tried " + ", ".join(tried))


def _load_yaml_chain(path, _seen=()):
    path = os.path.abspath(path)
    if path in _seen:
        raise ValueError(f"inherit_from cycle: {' -> '.join(_seen + (path,))}")
    with open(path, "r") as f:
        cfg_special = yaml.full_load(f) or {}
    inherit_from = cfg_special.get("inherit_from")
    cfg = _load_yaml_chain(resolve_inherit(inherit_from, path), _seen + (path,)) if inherit_from is not None else dict()
    update_recursive(cfg, cfg_special)
    return cfg


def load_config(path):
    """utils/config_utils.py load_config (without default_path), merged over default_config()."""
    return update_recursive(default_config(), _load_yaml_chain(path))


def apply_cli_overrides(config, eval=False, dynamic=False):
    """slam.py:262-276: --eval saves results, turns the GUI off, evaluates the rendering and keeps wandb off; --dynamic sets
    model_params.dynamic_model (it is set either way, as the reference does)."""
    if eval:
        config["Results"]["save_results"] = True
        config["Results"]["use_gui"] = False
        config["Results"]["eval_rendering"] = True
        config["Results"]["use_wandb"] = False
    config["model_params"]["dynamic_model"] = bool(dynamic)
    return config
