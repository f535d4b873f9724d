"""LPIPS v0.1 (AlexNet) restated in float64 on the CPU from its published definition, in plain torch: the reference of
tests/test_lpips_host.py and tests/test_hip_lpips.py. Written apart from slam/perceptual.py (it shares only the weight tables' names).

For x, y [B, 3, H, W] in [0, 1]: u = 2 v - 1; (u - shift) / scale; AlexNet.features with a tap after each ReLU; per tap and pixel the two
feature vectors unit-normalised over the channels (norm="torchmetrics": f / sqrt(1e-8 + sum f^2); "lpips": f / (sqrt(sum f^2) + 1e-10)),
squared difference, times lin[c], summed over the channels, mean over the pixels; the score is the sum of the five tap means."""
import torch
import torch.nn.functional as F

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# AlexNet.features: Conv(3, 64, 11, 4, 2) ReLU MaxPool(3, 2) Conv(64, 192, 5, 1, 2) ReLU MaxPool(3, 2) Conv(192, 384, 3, 1, 1) ReLU
# Conv(384, 256, 3, 1, 1) ReLU Conv(256, 256, 3, 1, 1) ReLU [MaxPool: after the last tap, not part of the metric]
LAYERS = (("conv", 0, 4, 2), ("tap",), ("pool",), ("conv", 3, 1, 2), ("tap",), ("pool",), ("conv", 6, 1, 1), ("tap",), ("conv", 8, 1, 1),
          ("tap",), ("conv", 10, 1, 1), ("tap",))


def network_input(x, y):
    """[2B, 3, H, W] float64: x's rows, then y's, scaled."""
    v = torch.cat((x.double().cpu(), y.double().cpu()))
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    return ((2.0 * v - 1.0) - shift) / scale


def features(alexnet_sd, batch):
    taps, t = [], batch.double()
    for layer in LAYERS:
        if layer[0] == "conv":
            _, idx, stride, pad = layer
            t = F.relu(F.conv2d(t, alexnet_sd[f"features.{idx}.weight"].double().cpu(), alexnet_sd[f"features.{idx}.bias"].double().cpu(),
                                stride, pad))
        elif layer[0] == "pool":
            t = F.max_pool2d(t, 3, 2)
        else:
            taps.append(t)
    return taps


def unit(f, norm):
    s = (f * f).sum(dim=1, keepdim=True)
    if norm == "torchmetrics":
        return f / torch.sqrt(1e-8 + s)
    if norm == "lpips":
        return f / (torch.sqrt(s) + 1e-10)
    raise ValueError(norm)


def distance(feats, lins, norm="torchmetrics"):
    """feats[l] [2B, C, h, w] (rows 0 .. B-1 against B .. 2B-1), lins[l] [C] (any shape with C values) -> (tap means [B, L], scores [B]),
    float64."""
    B = feats[0].shape[0] // 2
    means = []
    for f, w in zip(feats, lins):
        n = unit(f.double().cpu(), norm)
        d = (n[:B] - n[B:]) ** 2
        means.append((d * w.double().cpu().reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2)))
    means = torch.stack(means, dim=1)
    return means, means.sum(dim=1)


def lpips(alexnet_sd, lin_sd, x, y, norm="torchmetrics"):
    """Scores [B], float64."""
    lins = [lin_sd[f"lin{l}.model.1.weight"] for l in range(5)]
    return distance(features(alexnet_sd, network_input(x, y)), lins, norm)[1]


def ladder(height, width, seed=0, sigmas=(0.3, 0.03, 0.003)):
    """The noise ladder: a seeded uniform image smoothed by a 9 x 9 box filter, and that image plus Gaussian noise of each sigma, clamped
    to [0, 1]. Returns (base [1, 3, H, W], [noisy [1, 3, H, W] per sigma]), float32."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((1, 3, height, width), generator=g, dtype=torch.float64)
    base = F.avg_pool2d(F.pad(base, (4, 4, 4, 4), mode="replicate"), 9, 1).clamp(0, 1)
    noisy = [(base + s * torch.randn(base.shape, generator=g, dtype=torch.float64)).clamp(0, 1).float() for s in sigmas]
    return base.float(), noisy
