#!/usr/bin/env python
"""Generates tests/golden/mono_losses.npz by calling the reference's OWN utils/slam_utils.py get_loss_tracking / get_loss_mapping with
``Training.monocular = True`` (they dispatch to get_loss_tracking_rgb / get_loss_mapping_rgb) on seeded CPU tensors. The reference tree
is found through the environment variable REFERENCE_ROOT (authoring container only). Fixtures are data only: inputs, the loss value and
autograd gradients w.r.t. the image and the exposure parameters (the depth map takes no part: its gradient is None in the reference)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["REFERENCE_ROOT"])
torch.Tensor.cuda = lambda self, *a, **k: self          # the reference calls .cuda() on the ground-truth image
import utils.slam_utils as ref                            # noqa: E402

H, W = 12, 16
rng = np.random.default_rng(11)
config = {"Training": {"monocular": True, "rgb_boundary_threshold": 0.01, "alpha": 0.9}}
out = {"H": H, "W": W, "cfg_thr": 0.01, "cfg_alpha": 0.9, "exposure": np.array([0.07, -0.03], np.float32)}
gt_image = rng.uniform(0, 1, size=(3, H, W)).astype(np.float32)
gt_image[:, :3, :5] = 0.0                                 # below the rgb boundary threshold
grad_mask = rng.uniform(size=(1, H, W)) > 0.4
motion = rng.uniform(size=(H, W)) > 0.3
mask = rng.uniform(size=(H, W)) > 0.5
out.update(gt_image=gt_image, grad_mask=grad_mask, motion_mask=motion, mask=mask)


def viewpoint():
    a = torch.nn.Parameter(torch.tensor([0.07]))
    b = torch.nn.Parameter(torch.tensor([-0.03]))
    return types.SimpleNamespace(original_image=torch.tensor(gt_image), depth=None, exposure_a=a, exposure_b=b, motion_mask=torch.tensor(motion),
                                 grad_mask=torch.tensor(grad_mask), uid=3)


def record(name, loss, image, depth, vp, **extra):
    loss.backward()
    assert depth.grad is None
    out[f"{name}/image"], out[f"{name}/depth"], out[f"{name}/loss"] = image.detach().numpy(), depth.detach().numpy(), loss.item()
    out[f"{name}/g_image"] = image.grad.numpy()
    out[f"{name}/g_a"] = vp.exposure_a.grad.numpy() if vp.exposure_a.grad is not None else np.zeros(0, np.float32)
    out[f"{name}/g_b"] = vp.exposure_b.grad.numpy() if vp.exposure_b.grad is not None else np.zeros(0, np.float32)
    for k, v in extra.items():
        out[f"{name}/{k}"] = v


fresh = lambda *s, lo=0.0, hi=1.0: torch.tensor(rng.uniform(lo, hi, size=s).astype(np.float32), requires_grad=True)
# flags: [rm_dynamic, mask given] -- get_loss_tracking does not pass either on to get_loss_tracking_rgb
tcases = {"track_plain": (False, False), "track_rm_dynamic_mask": (True, True)}
for name, (rm_dynamic, use_mask) in tcases.items():
    image, depth, vp = fresh(3, H, W), fresh(1, H, W, lo=0.2, hi=5.0), viewpoint()
    opacity = torch.tensor(rng.uniform(0.6, 1.0, size=(1, H, W)).astype(np.float32))
    loss = ref.get_loss_tracking(config, image, depth, opacity, vp, rm_dynamic=rm_dynamic, mask=torch.tensor(mask) if use_mask else None)
    record(name, loss, image, depth, vp, opacity=opacity.numpy(), flags=np.array([rm_dynamic, use_mask]))
# flags: [initialization, rm_dynamic]
mcases = {"map_plain": (False, False), "map_initialization": (True, False), "map_rm_dynamic": (False, True)}
for name, (initialization, rm_dynamic) in mcases.items():
    image, depth, vp = fresh(3, H, W), fresh(1, H, W, lo=0.2, hi=5.0), viewpoint()
    loss = ref.get_loss_mapping(config, image, depth, vp, None, initialization=initialization, rm_dynamic=rm_dynamic)
    record(name, loss, image, depth, vp, flags=np.array([initialization, rm_dynamic]))
out["tracking_cases"], out["mapping_cases"] = np.array(list(tcases)), np.array(list(mcases))
np.savez_compressed(os.path.join(HERE, "mono_losses.npz"), **out)
print("wrote mono_losses.npz", {k: out[f"{k}/loss"] for k in list(tcases) + list(mcases)})
