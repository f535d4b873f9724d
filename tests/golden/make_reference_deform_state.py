#!/usr/bin/env python
"""Generates tests/golden/reference_deform_state.json: the NAMES and SHAPES of the state_dict() of the reference's own ControlNodeWarp
(utils/time_utils.py:788-1300, imported from /root/reference in the authoring container) as slam.py builds it for the shipped flags
(gaussian_splatting/scene/deform_model.py:20-30, arguments/__init__.py:107-125) -- what a deform.pth written by the reference's
DeformModel.save_weights holds. Names and shapes only: no values, no code. pytorch3d is stubbed as in make_golden_control_nodes.py (no
routine of it runs while the module is built)."""
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")


def _module(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


p3 = _module("pytorch3d")
p3.__path__ = []
p3.ops = _module("pytorch3d.ops", knn_points=None, ball_query=None)
p3.io = _module("pytorch3d.io", load_ply=None)
p3.loss = _module("pytorch3d.loss")
p3.loss.__path__ = []
_module("pytorch3d.loss.mesh_laplacian_smoothing", cot_laplacian=None)
torch.nn.Module.cuda = lambda self, *a, **k: self            # the reference hard-codes .cuda() (time_utils.py:822)
torch.Tensor.cuda = lambda self, *a, **k: self
import utils.time_utils as T                                   # noqa: E402

out = {}
for case, kw in (("shipped", dict(is_blender=False, node_num=512, K=3, local_frame=True, d_rot_as_res=True, hyper_dim=0)),
                 ("shipped_64_nodes", dict(is_blender=False, node_num=64, K=3, local_frame=True, d_rot_as_res=True, hyper_dim=0))):
    w = T.ControlNodeWarp(**kw)
    out[case] = {"arguments": kw, "entries": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in w.state_dict().items()]}
with open(os.path.join(HERE, "reference_deform_state.json"), "w") as f:
    json.dump(out, f, indent=1)
print({c: len(v["entries"]) for c, v in out.items()})
