"""Float64 restatement of the ternary census data term, written from the definition in
include/flownet2_hip.h -- whole-array slices over the 49 offsets, and a gradient that SCATTERS every term's derivative to
the two pixels it depends on -- not from the kernel, which gathers.

As in photometric_twin.py, f = scale * pred, the sample position (X, Y) and with it the truncation are formed in float32,
one rounding per operation, and so is the grey value G = ((r + g) + b) * 85: the library stores it, and the twin has to
stand on the same number.  Everything behind them is float64.

`loss_and_grad_from_warp` takes the outputs of the warp pass as given (the trainer tests feed it the device's buffers);
`torch_loss` is the forward in torch float64 for autograd (test_census_cpu.py)."""
import numpy as np

import photometric_twin as pt

R = 3
PATCH = 2 * R + 1


def grey(img):
    """G [n,h,w] in float32: ((r + g) + b) * 85, each operation rounded on its own."""
    img = np.asarray(img, np.float32)
    return (((img[..., 0] + img[..., 1]).astype(np.float32) + img[..., 2]).astype(np.float32) * np.float32(85.0)).astype(np.float32)


def warp_pass(img, pred, scale=1.0):
    """dict(G, W, DX, DY [n,h,w] float64, V [n,h,w] bool, X, Y float32): the partner's grey values sampled by tf_warp, the
    derivatives of the sample by the position on the clamped taps, and V = 0 <= X < w - 1 and 0 <= Y < h - 1.  Where V is 0
    the library stores W = DX = DY = 0 and so does the twin."""
    G = grey(img).astype(np.float64)
    n, h, w = G.shape
    _, X, Y = pt.positions(pred, scale)
    Wv, (Ga, Gb, Gc, Gd), (x0, x1, y0, y1), _ = pt.warp(G[pt.partner(n)][..., None], X, Y)
    x, y = X.astype(np.float64), Y.astype(np.float64)
    with np.errstate(all="ignore"):
        V = (X >= 0) & (X < np.float32(w - 1)) & (Y >= 0) & (Y < np.float32(h - 1))     # a NaN fails
        Ga, Gb, Gc, Gd = Ga[..., 0], Gb[..., 0], Gc[..., 0], Gd[..., 0]
        DX = (y1 - y) * (Gc - Ga) + (y - y0) * (Gd - Gb)
        DY = (x1 - x) * (Gb - Ga) + (x - x0) * (Gd - Gc)
    zero = lambda v: np.where(V, v, 0.0)
    return dict(G=G, W=zero(Wv[..., 0]), DX=zero(DX), DY=zero(DY), V=V, X=X, Y=Y)


def interior(h, w):
    """Omega as a boolean [h,w]."""
    om = np.zeros((h, w), bool)
    if min(h, w) >= PATCH:
        om[R:h - R, R:w - R] = True
    return om


def _norm(t):
    return t / np.sqrt(0.81 + t * t)


def loss_and_grad_from_warp(G, W, DX, DY, V, mask=None, scale=1.0, weight=1.0, q=0.4, grad_mult=1.0):
    """(L, dpred [n,h,w,2], dict(S, c, mc [n,h,w], Mc)) from the warp pass outputs, all taken as constants but W."""
    G, W, DX, DY = (np.asarray(v, np.float64) for v in (G, W, DX, DY))
    V = np.asarray(V) != 0
    n, h, w = G.shape
    m = np.ones((n, h, w)) if mask is None else (np.asarray(mask, np.float64).reshape(n, h, w) != 0).astype(np.float64)
    S, dW = np.zeros((n, h, w)), np.zeros((n, h, w))
    mc = m * V * interior(h, w)[None]
    Mc = mc.sum()
    den = 2.0 * Mc + 1e-6
    if min(h, w) < PATCH:
        return 0.0, np.zeros((n, h, w, 2)), dict(S=S, c=np.zeros((n, h, w)), mc=mc, Mc=0.0)
    core = (slice(None), slice(R, h - R), slice(R, w - R))
    offsets = [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]
    shifted = lambda dy, dx: (slice(None), slice(R + dy, h - R + dy), slice(R + dx, w - R + dx))
    for dy, dx in offsets:                                         # forward: S(q) = sum_d V(q+d) e / (0.1 + e)
        nb = shifted(dy, dx)
        e = (_norm(G[nb] - G[core]) - _norm(W[nb] - W[core])) ** 2
        S[core] += np.where(V[nb], e / (0.1 + e), 0.0)
    psi = (S + 0.01) ** q
    L = weight * (mc * psi).sum() / den
    c = mc * q * psi / (S + 0.01)
    for dy, dx in offsets:                                         # backward: every term pushes on W(q+d) and pulls on W(q)
        nb = shifted(dy, dx)
        tb = W[nb] - W[core]
        ab = _norm(G[nb] - G[core]) - _norm(tb)
        e = ab * ab
        de_dtb = -2.0 * ab * 0.81 / (0.81 + tb * tb) ** 1.5        # d e / d tb, n'(t) = 0.81 / (0.81 + t^2)^1.5
        term = np.where(V[nb], c[core] * 0.1 / (0.1 + e) ** 2 * de_dtb, 0.0)
        dW[nb] += term
        dW[core] -= term
    k = grad_mult * weight * float(np.float32(scale)) / den
    return L, k * dW[..., None] * np.stack([DX, DY], -1), dict(S=S, c=c, mc=mc, Mc=Mc)


def loss_and_grad(img, pred, mask=None, scale=1.0, weight=1.0, q=0.4, grad_mult=1.0):
    """(L, dpred, parts of the warp pass and of the loss) for one level."""
    wp = warp_pass(img, pred, scale)
    L, g, parts = loss_and_grad_from_warp(wp["G"], wp["W"], wp["DX"], wp["DY"], wp["V"], mask, scale, weight, q, grad_mult)
    return L, g, dict(wp, **parts)


def torch_loss(img, pred, mask=None, scale=1.0, weight=1.0, q=0.4):
    """The forward in torch float64 on the CPU, differentiable in `pred` (a float64 leaf).  The position is moved onto the
    float32 one by a constant and the integer casts carry no gradient, as in photometric_twin.torch_loss; G, V, the mask
    and Mc are constants."""
    import torch
    G = torch.as_tensor(grey(img).astype(np.float64))
    n, h, w = G.shape
    _, X32, Y32 = pt.positions(pred.detach().numpy(), scale)
    s = float(np.float32(scale))
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    x, y = gx[None] + s * pred[..., 0], gy[None] + s * pred[..., 1]
    x = x + (torch.from_numpy(X32.astype(np.float64)) - x).detach()
    y = y + (torch.from_numpy(Y32.astype(np.float64)) - y).detach()
    V = torch.as_tensor((X32 >= 0) & (X32 < np.float32(w - 1)) & (Y32 >= 0) & (Y32 < np.float32(h - 1)))
    x0 = x.detach().trunc().long()
    y0 = y.detach().trunc().long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    src = G[torch.as_tensor(pt.partner(n))]
    b = torch.arange(n)[:, None, None]
    x0f, x1f, y0f, y1f = (v.double() for v in (x0, x1, y0, y1))
    Wv = ((x1f - x) * (y1f - y) * src[b, y0, x0] + (x1f - x) * (y - y0f) * src[b, y1, x0]
          + (x - x0f) * (y1f - y) * src[b, y0, x1] + (x - x0f) * (y - y0f) * src[b, y1, x1])
    Wv = torch.where(V, Wv, torch.zeros_like(Wv))
    m = torch.ones(n, h, w, dtype=torch.float64) if mask is None else torch.as_tensor(
        (np.asarray(mask).reshape(n, h, w) != 0).astype(np.float64))
    mc = m * V.double() * torch.as_tensor(interior(h, w).astype(np.float64))[None]
    if min(h, w) < PATCH:
        return (Wv * 0.0).sum()
    norm = lambda t: t / torch.sqrt(0.81 + t * t)
    S = torch.zeros(n, h - 2 * R, w - 2 * R, dtype=torch.float64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            nb = (slice(None), slice(R + dy, h - R + dy), slice(R + dx, w - R + dx))
            e = (norm(G[nb] - G[:, R:h - R, R:w - R]) - norm(Wv[nb] - Wv[:, R:h - R, R:w - R])) ** 2
            S = S + V[nb].double() * e / (0.1 + e)
    return weight * (mc[:, R:h - R, R:w - R] * (S + 0.01) ** q).sum() / (2.0 * mc.sum() + 1e-6)
