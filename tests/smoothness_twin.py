"""float64 twin of the edge-aware smoothness term (fn2_smoothness_loss_grad, include/flownet2_hip.h), written from the
definition and not from the kernel: whole-array slices, and a gradient that SCATTERS each term's derivative onto the pixels
it touches (the kernel gathers).  Only f = scale * pred is formed in fp32, as the library forms it; everything behind it is
float64.

    order 1   a term between p and p + 1 of an axis:  D = f(p + 1) - f(p),           g = exp(-lambda mean_c |I(p + 1) - I(p)|)
    order 2   a term on p in [1, len - 2]:            D = f(p - 1) - 2 f(p) + f(p + 1), g = exp(-lambda mean_c |I(p + 1) - I(p - 1)| / 2)
    L = weight * smooth_weight * 0.5 * (sum_x-terms g rho(D_k) / Cx + sum_y-terms g rho(D_k) / Cy),  rho(d) = sqrt(d^2 + eps^2)

An axis shorter than order + 1 has no term; a level with min(h, w) == 1 has loss 0 and gradient 0."""
import numpy as np


def scaled(pred, scale):
    """f = scale * pred, one fp32 rounding, as float64."""
    return (np.float32(scale) * np.asarray(pred, np.float32)).astype(np.float64)


def _cut(a, axis, lo, hi):
    """a[..., lo:len + hi, ...] along `axis` (hi <= 0)."""
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(lo, a.shape[axis] + hi)
    return tuple(sl)


def axes_of(shape, order):
    """The axes (1: y, 2: x) of an [n, h, w, .] level that hold at least one term."""
    n, h, w = shape[:3]
    if min(h, w) == 1:
        return []
    return [ax for ax in (2, 1) if shape[ax] >= order + 1]


def terms(f, img, axis, order, edge_lambda):
    """(g [.., terms, ..], D [.., terms, .., 2]) of every term along `axis`."""
    img = np.asarray(img, np.float64)
    if order == 1:
        D = f[_cut(f, axis, 1, 0)] - f[_cut(f, axis, 0, -1)]
        dI = np.abs(img[_cut(img, axis, 1, 0)] - img[_cut(img, axis, 0, -1)])
    else:
        D = f[_cut(f, axis, 0, -2)] - 2.0 * f[_cut(f, axis, 1, -1)] + f[_cut(f, axis, 2, 0)]
        dI = np.abs(img[_cut(img, axis, 2, 0)] - img[_cut(img, axis, 0, -2)]) / 2.0
    return np.exp(-edge_lambda * dI.sum(-1) / 3.0), D


def weights(img, order, edge_lambda):
    """{axis: g} -- the edge weights alone (what the tests assert their span on)."""
    img = np.asarray(img, np.float64)
    zero = np.zeros(img.shape[:3] + (2,))
    return {ax: terms(zero, img, ax, order, edge_lambda)[0] for ax in axes_of(img.shape, order)}


def loss_and_grad(img, pred, scale=1.0, weight=1.0, order=1, edge_lambda=150.0, eps=1e-3, smooth_weight=1.0, grad_mult=1.0):
    """(L, dpred [n,h,w,2] float64)."""
    f = scaled(pred, scale)
    L, dLdf = 0.0, np.zeros_like(f)
    for ax in axes_of(f.shape, order):
        g, D = terms(f, img, ax, order, edge_lambda)
        rho = np.sqrt(D * D + eps * eps)
        c = 0.5 / g.size                                           # g.size = C of the axis: n h (w - order) or n (h - order) w
        L += c * float((g[..., None] * rho).sum())
        t = c * g[..., None] * D / rho
        if order == 1:
            dLdf[_cut(f, ax, 1, 0)] += t
            dLdf[_cut(f, ax, 0, -1)] -= t
        else:
            dLdf[_cut(f, ax, 0, -2)] += t
            dLdf[_cut(f, ax, 1, -1)] -= 2.0 * t
            dLdf[_cut(f, ax, 2, 0)] += t
    k = float(weight) * float(smooth_weight)
    return k * L, float(grad_mult) * k * float(np.float32(scale)) * dLdf


def torch_loss(img, pred, scale=1.0, weight=1.0, order=1, edge_lambda=150.0, eps=1e-3, smooth_weight=1.0):
    """The forward alone on a float64 torch tensor `pred` (f = scale * pred in float64: the caller picks inputs whose
    product is exact in fp32), for autograd."""
    import torch
    f = float(np.float32(scale)) * pred
    L = 0.0
    for ax in axes_of(tuple(f.shape), order):
        if order == 1:
            D = f[_cut(f, ax, 1, 0)] - f[_cut(f, ax, 0, -1)]
        else:
            D = f[_cut(f, ax, 0, -2)] - 2.0 * f[_cut(f, ax, 1, -1)] + f[_cut(f, ax, 2, 0)]
        g = torch.from_numpy(terms(np.zeros(tuple(f.shape)), img, ax, order, edge_lambda)[0])
        L = L + (0.5 / g.numel()) * (g[..., None] * torch.sqrt(D * D + eps * eps)).sum()
    return float(weight) * float(smooth_weight) * L


def total(imgs, preds, scales, weights_, **kw):
    """The trainer's sum over levels: ([(L, dpred)], sum of L)."""
    levels = [loss_and_grad(i, p, s, w, **kw) for i, p, s, w in zip(imgs, preds, scales, weights_)]
    return levels, sum(l[0] for l in levels)
