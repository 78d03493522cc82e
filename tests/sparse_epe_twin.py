"""Float64 twin of the sparse multi-scale EPE (include/flownet2_hip.h, csrc/sparse_epe.hip), restated from its definition:
  valid(p) = both label components finite;  M = #valid over the batch
  e = ||pred - label||_2, from float64 differences of the fp32 inputs
  L = weight * (h w) * sum_valid e / M
  dpred = grad_mult * weight * (h w) / M * (pred - label) / e on valid pixels with e > 0, +0 elsewhere
  M = 0: L = 0, dpred = 0
The `weight` the kernel sees is a float32; the twin takes the same rounded value."""
import numpy as np


def valid_mask(label):
    return np.isfinite(np.asarray(label)).all(axis=-1)


def loss_and_grad(pred, label, weight, grad_mult=1.0):
    """pred, label [n,h,w,2] (fp32 values).  Returns (L, dpred [n,h,w,2] float64, M)."""
    pred, label = np.asarray(pred, np.float32).astype(np.float64), np.asarray(label, np.float32).astype(np.float64)
    n, h, w, _ = pred.shape
    weight = float(np.float32(weight))
    valid = valid_mask(label)
    m = int(valid.sum())
    g = np.zeros(pred.shape, np.float64)
    if m == 0:
        return 0.0, g, 0
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.where(valid[..., None], pred - np.where(valid[..., None], label, 0.0), 0.0)
        e = np.sqrt((d * d).sum(axis=-1))
    coef = weight * (h * w) / m
    use = valid & (e > 0)
    g[use] = float(grad_mult) * coef * d[use] / e[use][:, None]
    return coef * float(e[valid].sum()), g, m


def torch_loss(pred, label, weight):
    """The forward alone on a float64 torch tensor `pred` (requires_grad), with M and the mask constant."""
    import torch
    lab = np.asarray(label, np.float32).astype(np.float64)
    n, h, w, _ = lab.shape
    valid = valid_mask(lab)
    m = int(valid.sum())
    if m == 0:
        return pred.sum() * 0.0
    vt = torch.tensor(valid)
    d = pred - torch.tensor(np.where(valid[..., None], lab, 0.0))
    e = torch.sqrt((d * d).sum(dim=-1))
    return float(np.float32(weight)) * (h * w) / m * e[vt].sum()
