"""The YOLO-seg contract restated plainly in torch float64, for the tests: the unfused modules (convolution, then BatchNorm with its
running statistics, then the activation), ultralytics' Detect / Segment inference decode, ops.non_max_suppression with the greedy NMS
written out (torchvision is not installed here; nms() is the statement, nms_vectorised() what thousands of candidates need), and
ops.process_mask in its logit form; and two measures of an input's quality, min_iou_margin() and min_score_gap(). Runs over the stub
modules that slam.segmentation.load_checkpoint returns, on any device."""
import numpy as np
import torch
import torch.nn.functional as F

from slam.segmentation import child, children, kind, tensor

D = torch.float64
MAX_WH = 7680.0
MAX_NMS = 30000


def _p(m, name, dev):
    t = tensor(m, name, required=False)
    return None if t is None else t.to(dev, D)


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def conv2d(m, x):
    return F.conv2d(x, _p(m, "weight", x.device), _p(m, "bias", x.device), _pair(m.stride), m.padding if isinstance(m.padding, str)
                    else _pair(m.padding), _pair(m.dilation), int(m.groups))


def batch_norm(m, x):
    dev = x.device
    return F.batch_norm(x, _p(m, "running_mean", dev), _p(m, "running_var", dev), _p(m, "weight", dev), _p(m, "bias", dev), False, 0.0,
                        float(m.eps))


def act(m, x):
    return x if m is None or kind(m) == "Identity" else F.silu(x)


def run(m, x):
    """Module m (a stub) on x, unfused, in float64."""
    k = kind(m)
    c = children(m)
    if k == "Conv":
        return act(c.get("act"), batch_norm(c["bn"], conv2d(c["conv"], x)))
    if k == "Conv2d":
        return conv2d(m, x)
    if k in ("Sequential", "ModuleList"):
        for s in c.values():
            x = run(s, x)
        return x
    if k == "Silence":
        return x
    if k == "RepConvN":
        return act(c.get("act"), run(c["conv1"], x) + run(c["conv2"], x))
    if k == "RepBottleneck":
        y = run(c["cv2"], run(c["cv1"], x))
        return x + y if m.add else y
    if k == "RepCSP":
        return run(c["cv3"], torch.cat((run(c["m"], run(c["cv1"], x)), run(c["cv2"], x)), 1))
    if k == "RepNCSPELAN4":
        y = list(run(c["cv1"], x).chunk(2, 1))
        y.append(run(c["cv2"], y[-1]))
        y.append(run(c["cv3"], y[-1]))
        return run(c["cv4"], torch.cat(y, 1))
    if k == "ADown":
        x = F.avg_pool2d(x, 2, 1, 0, False, True)
        x1, x2 = x.chunk(2, 1)
        return torch.cat((run(c["cv1"], x1), run(c["cv2"], F.max_pool2d(x2, 3, 2, 1))), 1)
    if k == "MaxPool2d":
        return F.max_pool2d(x, m.kernel_size, m.stride, m.padding)
    if k == "SPPELAN":
        y = [run(c["cv1"], x)]
        for n in ("cv2", "cv3", "cv4"):
            y.append(run(c[n], y[-1]))
        return run(c["cv5"], torch.cat(y, 1))
    if k == "CBLinear":
        return conv2d(c["conv"], x).split([int(v) for v in m.c2s], dim=1)
    if k == "CBFuse":
        size = x[-1].shape[2:]
        out = x[-1]
        for i, xi in enumerate(x[:-1]):
            out = out + F.interpolate(xi[m.idx[i]], size=size, mode="nearest")
        return out
    if k == "Concat":
        return torch.cat(x, int(m.d))
    if k == "Upsample":
        return F.interpolate(x, scale_factor=m.scale_factor, mode="nearest")
    if k == "Proto":
        u = c["upsample"]
        x = run(c["cv1"], x)
        x = F.conv_transpose2d(x, _p(u, "weight", x.device), _p(u, "bias", x.device), _pair(u.stride), _pair(u.padding))
        return run(c["cv3"], run(c["cv2"], x))
    if k == "Segment":
        heads = [(torch.cat((run(child(m, "cv2")._modules[str(l)], x[l]), run(child(m, "cv3")._modules[str(l)], x[l])), 1)[0],
                  run(child(m, "cv4")._modules[str(l)], x[l])[0]) for l in range(int(m.nl))]
        return heads, run(c["proto"], x[0])[0]
    raise ValueError(f"yolo_reference: no {k}")


def network(model, image):
    """(per level (head [64 + nc, h, w], coef [nm, h, w]), proto) of the model's layer graph on image [3, H, W], float64."""
    x = image.to(D)[None]
    y = []
    for layer in children(child(model, "model")).values():
        f = layer.f
        if f != -1:
            x = y[f] if isinstance(f, int) else [x if j == -1 else y[j] for j in f]
        x = run(layer, x)
        y.append(x)
    return x


def decode(heads, strides, fp32_scores=False):
    """Detect's inference output per anchor: boxes xywh [A, 4], class scores [A, nc], coefficients [A, nm] (float64). fp32_scores: the
    sigmoid rounded to float32, as ultralytics computes it (ties that float32 makes stay ties)."""
    boxes, scores, coefs = [], [], []
    for (h, c), s in zip(heads, strides):
        h, c = h.to(D), c.to(D)
        nc = h.shape[0] - 64
        _, lh, lw = h.shape
        box = h[:64].reshape(4, 16, lh * lw).softmax(1)                         # DFL: softmax over the bins, then the expectation
        dist = (box * torch.arange(16, dtype=D, device=h.device)[None, :, None]).sum(1)       # [4, a]: l t r b
        ys, xs = torch.meshgrid(torch.arange(lh, dtype=D, device=h.device), torch.arange(lw, dtype=D, device=h.device), indexing="ij")
        ax, ay = xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5
        x1, y1, x2, y2 = ax - dist[0], ay - dist[1], ax + dist[2], ay + dist[3]
        boxes.append(torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), 1) * s)
        sc = torch.sigmoid(h[64:].reshape(nc, -1)).T
        scores.append(sc.float().double() if fp32_scores else sc)
        coefs.append(c.reshape(c.shape[0], -1).T)
    return torch.cat(boxes), torch.cat(scores), torch.cat(coefs)


def nms(boxes, scores, iou_thres):
    """Greedy NMS: visit boxes by score descending (ties: lower index first); keep a box unless its IoU with a kept box exceeds iou_thres.
    Returns the kept indices in visiting order."""
    order = sorted(range(len(scores)), key=lambda i: (-float(scores[i]), i))
    kept = []
    for i in order:
        ok = True
        for k in kept:
            b, q = boxes[i], boxes[k]
            iw = max(min(float(b[2]), float(q[2])) - max(float(b[0]), float(q[0])), 0.0)
            ih = max(min(float(b[3]), float(q[3])) - max(float(b[1]), float(q[1])), 0.0)
            inter = iw * ih
            union = float((b[2] - b[0]) * (b[3] - b[1])) + float((q[2] - q[0]) * (q[3] - q[1])) - inter
            if inter / union > iou_thres:
                ok = False
                break
        if ok:
            kept.append(i)
    return kept


def _np64(t):
    return t.detach().to("cpu", D).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def nms_vectorised(boxes, scores, iou_thres):
    """nms() with the inner loop as array arithmetic in float64: one visited box at a time against all boxes behind it in the visiting
    order (score descending, ties by lower index). The same expressions as nms(), so the same decisions. Kept indices, visiting order."""
    b, s = _np64(boxes).reshape(-1, 4), _np64(scores).reshape(-1)
    order = np.argsort(-s, kind="stable")
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    alive = np.ones(len(b), dtype=bool)
    kept = []
    for i in range(len(b)):
        if not alive[i]:
            continue
        kept.append(int(order[i]))
        r = b[i + 1:]
        iw = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]), 0.0)
        ih = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]), 0.0)
        inter = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            alive[i + 1:] &= ~(inter / (area[i] + area[i + 1:] - inter) > iou_thres)
    return kept


def survivors(boxes_xywh, scores, cls_id, conf=0.25, iou=0.7):
    """(the anchors of class cls_id that NMS keeps, in visiting order and before max_det; the number of candidates of the class)."""
    best, j = scores.max(1)
    idx = torch.nonzero((best > conf) & (j == cls_id)).flatten()
    xy, wh = boxes_xywh[:, :2], boxes_xywh[:, 2:]
    xyxy = torch.cat((xy - wh / 2, xy + wh / 2), 1)
    idx = idx[torch.sort(best[idx], descending=True, stable=True).indices][:MAX_NMS]     # score descending, anchor ascending
    off = xyxy[idx] + float(cls_id) * MAX_WH
    kept = idx[torch.as_tensor(nms_vectorised(off, best[idx], iou), dtype=torch.long, device=idx.device)]
    return kept, len(idx)


def _rows(boxes_xywh, scores, coefs, cls_id, kept):
    xy, wh = boxes_xywh[kept, :2], boxes_xywh[kept, 2:]
    rows = torch.cat((xy - wh / 2, xy + wh / 2, scores[kept, cls_id, None], torch.full((len(kept), 1), float(cls_id), dtype=D,
                      device=kept.device), kept.to(D)[:, None]), 1)
    return rows.cpu().reshape(-1, 7), coefs[kept]


def non_max_suppression(boxes_xywh, scores, coefs, cls_id, conf=0.25, iou=0.7, max_det=300):
    """One predict(classes=[cls_id]) call: rows (x1, y1, x2, y2, score, class, anchor) [n, 7] and coefficients [n, nm]."""
    kept, _ = survivors(boxes_xywh, scores, cls_id, conf, iou)
    return _rows(boxes_xywh, scores, coefs, cls_id, kept[:max_det])


def detections(heads, strides, classes, conf=0.25, iou=0.7, max_det=300, fp32_scores=False, max_dets=None, counts=False):
    """The reference's one predict per class, concatenated: rows [n, 7] and coefficients [n, nm]. max_dets (gsr_yolo_detect's row
    capacity): the survivors are visited in global order (score descending, then anchor ascending) and one is emitted while its class
    has fewer than max_det and fewer than max_dets are emitted in all; the rows stay per class, concatenated. counts: also return
    (emitted, candidates, NMS survivors before max_det), as gsr_yolo_detect reports them."""
    boxes, scores, coefs = decode(heads, strides, fp32_scores)
    classes = sorted(set(classes))
    kept, cand = zip(*(survivors(boxes, scores, c, conf, iou) for c in classes))
    cut = [k[:max_det] for k in kept]
    if max_dets is not None:
        first = sorted((-s, a, q) for q, (k, c) in enumerate(zip(cut, classes)) for s, a in zip(scores[k, c].tolist(), k.tolist()))
        cut = [torch.tensor([a for _, a, q in first[:max_dets] if q == p], dtype=torch.long, device=boxes.device)
               for p in range(len(classes))]
    out = [_rows(boxes, scores, coefs, c, k) for c, k in zip(classes, cut)]
    rows, co = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
    return (rows, co, (len(rows), sum(cand), sum(len(k) for k in kept))) if counts else (rows, co)


def _t64(x):
    return x.to(D) if isinstance(x, torch.Tensor) else torch.tensor(x, dtype=D)


def _pair_iou(a, b):
    """IoU [len(a), len(b)] of xyxy boxes in float64; 0 where the union is empty."""
    iw = (torch.minimum(a[:, None, 2], b[None, :, 2]) - torch.maximum(a[:, None, 0], b[None, :, 0])).clamp_(min=0)
    ih = (torch.minimum(a[:, None, 3], b[None, :, 3]) - torch.maximum(a[:, None, 1], b[None, :, 1])).clamp_(min=0)
    inter = iw * ih
    union = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] - inter
    return torch.where(union > 0, inter / union.clamp(min=1e-300), torch.zeros_like(inter))


def min_iou_margin(boxes_xyxy, cls, iou=0.7, block=512):
    """Input quality: the smallest |IoU - iou| over all pairs of candidates of equal class (float64, in blocks of rows); inf without
    such a pair. Far from 0, no NMS decision can turn on float32 rounding."""
    b = _t64(boxes_xyxy).reshape(-1, 4)
    cls = torch.as_tensor(cls, device=b.device).reshape(-1)
    best = float("inf")
    for i0 in range(0, len(b), block):
        m = (_pair_iou(b[i0:i0 + block], b) - iou).abs()
        rows = torch.arange(i0, min(i0 + block, len(b)), device=b.device)
        pair = (cls[i0:i0 + block, None] == cls[None, :]) & (rows[:, None] != torch.arange(len(b), device=b.device)[None, :])
        if bool(pair.any()):
            best = min(best, float(m[pair].min()))
    return best


def min_score_gap(scores, conf=0.25):
    """Input quality: the smallest difference between two distinct candidate scores, and between any candidate score and conf
    (float64); inf without scores. Above float32's rounding, neither the sort nor the conf test can turn on it; equal scores are ties."""
    s = torch.unique(_t64(scores).reshape(-1))                 # sorted ascending, distinct
    if len(s) == 0:
        return float("inf")
    gap = float((s - conf).abs().min())
    return min(gap, float((s[1:] - s[:-1]).min())) if len(s) > 1 else gap


def mask_logits(rows, coefs, proto, shape):
    """process_mask (upsample=True) before its threshold: per detection the cropped proto-resolution logits, bilinearly upsampled to
    shape (H, W) with align_corners=False. [n, H, W] float64."""
    proto = proto.to(D)
    c, mh, mw = proto.shape
    H, W = shape
    if len(rows) == 0:
        return torch.zeros((0, H, W), dtype=D, device=proto.device)
    m = (coefs.to(proto.device, D) @ proto.reshape(c, -1)).reshape(-1, mh, mw)
    b = rows[:, :4].to(proto.device, D).clone()
    b[:, 0] *= mw / W
    b[:, 2] *= mw / W
    b[:, 1] *= mh / H
    b[:, 3] *= mh / H
    x1, y1, x2, y2 = (b[:, k, None, None] for k in range(4))
    r = torch.arange(mw, dtype=D, device=proto.device)[None, None, :]            # columns
    cc = torch.arange(mh, dtype=D, device=proto.device)[None, :, None]           # rows
    m = m * ((r >= x1) & (r < x2) & (cc >= y1) & (cc < y2))
    return F.interpolate(m[None], (H, W), mode="bilinear", align_corners=False)[0]


def union_mask(rows, coefs, proto, shape):
    """(mask [H, W] bool: OR over detections of logit > 0, the logits [n, H, W])."""
    lg = mask_logits(rows, coefs, proto, shape)
    return (lg > 0).any(0) if len(lg) else torch.zeros(shape, dtype=torch.bool, device=proto.device), lg
