"""Float64 restatement of the occlusion-aware photometric loss, written from the reference's
src/utils.py:378-395 (abs_robust_loss, its loss_mean) and :453-538 (tf_warp, length_sq, occlusion) -- not from the kernel.

Slots: image j is a frame, image j ^ 1 its partner.  f = scale * pred and the sample position (X, Y) = (x + f_u, y + f_v)
are formed in float32, one rounding per product and per sum, because tf_warp truncates the position and a truncation is
discontinuous: the twin has to stand on the coordinate the device stands on.  Everything behind the position is float64.

`torch_loss` is the same forward written with torch ops on float64 tensors, for autograd: the analytic gradient of
`loss_and_grad` is checked against it on the CPU (test_photometric_cpu.py) before a GPU sees the formula."""
import numpy as np


def partner(n):
    return np.arange(n) ^ 1


def positions(pred, scale):
    """(f, X, Y) in float32: f [n,h,w,2] = fl(scale * pred), X = fl(x + f_u), Y = fl(y + f_v)."""
    pred = np.asarray(pred, np.float32)
    n, h, w, _ = pred.shape
    with np.errstate(all="ignore"):
        f = (np.float32(scale) * pred).astype(np.float32)
        gx, gy = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        X = (gx[None] + f[..., 0]).astype(np.float32)
        Y = (gy[None] + f[..., 1]).astype(np.float32)
    return f, X, Y


def _trunc(v, size):
    """tf.cast(float -> int32), made total as the library makes it: NaN -> 0, the rest saturates (no index the clamp
    behind it can tell apart is lost)."""
    with np.errstate(all="ignore"):
        t = np.clip(np.trunc(np.where(np.isnan(v), 0.0, v.astype(np.float64))), -2, size + 1)
    return t.astype(np.int64)


def taps(X, Y, h, w):
    """utils.py:477-505: the clamped taps and the four weights (float64, from the float32 position)."""
    tx, ty = _trunc(X, w), _trunc(Y, h)
    x0, x1 = np.clip(tx, 0, w - 1), np.clip(tx + 1, 0, w - 1)
    y0, y1 = np.clip(ty, 0, h - 1), np.clip(ty + 1, 0, h - 1)
    x, y = X.astype(np.float64), Y.astype(np.float64)
    with np.errstate(all="ignore"):
        wa, wb = (x1 - x) * (y1 - y), (x1 - x) * (y - y0)
        wc, wd = (x - x0) * (y1 - y), (x - x0) * (y - y0)
    return (x0, x1, y0, y1), (wa, wb, wc, wd)


def warp(src, X, Y):
    """tf_warp(src, .) at the positions (X, Y): src [n,h,w,c] float64 -> (warped [n,h,w,c], the four tap values, idx, wgt)."""
    n, h, w, _ = src.shape
    idx, wgt = taps(X, Y, h, w)
    x0, x1, y0, y1 = idx
    b = np.arange(n)[:, None, None]
    Ia, Ib, Ic, Id = src[b, y0, x0], src[b, y1, x0], src[b, y0, x1], src[b, y1, x1]
    wa, wb, wc, wd = (v[..., None] for v in wgt)
    with np.errstate(all="ignore"):
        out = ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id          # tf.add_n, :514
    return out, (Ia, Ib, Ic, Id), idx, wgt


def masks(pred, scale=1.0, alpha=0.01, beta=0.5):
    """m = valid & ~occ per slot [n,h,w] (bool) and the parts the tests reason about:
    dict(f, X, Y, d, t, occ, valid, warped)."""
    f32, X, Y = positions(pred, scale)
    n, h, w, _ = f32.shape
    f = f32.astype(np.float64)
    warped, _, _, _ = warp(f[partner(n)], X, Y)                  # flow_bw_warped, :527
    with np.errstate(all="ignore"):
        d = ((f + warped) ** 2).sum(-1)                          # :529, length_sq
        t = alpha * ((f ** 2).sum(-1) + (warped ** 2).sum(-1)) + beta   # :531-533
        occ = d > t                                              # :535; a NaN compares false
        valid = (X >= 0) & (X < np.float32(w - 1)) & (Y >= 0) & (Y < np.float32(h - 1))   # a NaN fails
    return valid & ~occ, dict(f=f, X=X, Y=Y, d=d, t=t, occ=occ, valid=valid, warped=warped)


def loss_and_grad(img, pred, mask, scale=1.0, weight=1.0, q=0.4, grad_mult=1.0):
    """(L, dpred [n,h,w,2], residual d [n,h,w,3]) with the mask [n,h,w] (0 / 1) and its sum as constants."""
    img = np.asarray(img, np.float64)
    n, h, w, _ = img.shape
    m = np.asarray(mask, np.float64).reshape(n, h, w)
    _, X, Y = positions(pred, scale)
    warped, (Ia, Ib, Ic, Id), (x0, x1, y0, y1), _ = warp(img[partner(n)], X, Y)
    x, y = X.astype(np.float64)[..., None], Y.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        d = img - warped
        mag = np.abs(d) + 0.01
        psi = mag ** q                                           # :389
        den = 2.0 * m.sum() + 1e-6                               # :392
        live = m[..., None] > 0                                  # (a masked pixel may hold anything: it is not looked at)
        L = weight * np.where(live, psi, 0.0).sum() / den
        dpsi = q * mag ** (q - 1.0) * np.sign(d)
        dwx = (y1[..., None] - y) * (Ic - Ia) + (y - y0[..., None]) * (Id - Ib)
        dwy = (x1[..., None] - x) * (Ib - Ia) + (x - x0[..., None]) * (Id - Ic)
        k = grad_mult * weight * float(np.float32(scale)) / den
        gu = np.where(live, dpsi * -dwx, 0.0).sum(-1)
        gv = np.where(live, dpsi * -dwy, 0.0).sum(-1)
    return L, k * np.stack([gu, gv], -1), d


def total(img_levels, preds, scales, weights, alpha=0.01, beta=0.5, q=0.4, grad_mult=1.0, given_masks=None):
    """The multi-scale loss: [(L_l, dpred_l, mask_l)] per level and the sum of the L_l."""
    out = []
    for i, (img, pred, s, wgt) in enumerate(zip(img_levels, preds, scales, weights)):
        m = masks(pred, s, alpha, beta)[0] if given_masks is None else given_masks[i]
        L, g, _ = loss_and_grad(img, pred, m, s, wgt, q, grad_mult)
        out.append((L, g, m))
    return out, sum(o[0] for o in out)


def torch_loss(img, pred, mask, scale=1.0, weight=1.0, q=0.4):
    """The forward of loss_and_grad in torch float64 on the CPU, differentiable in `pred` (a float64 leaf tensor).  The
    position is moved onto the float32 one by a constant, so that truncation sees what positions() computed; the casts
    to integer carry no gradient, as in TensorFlow."""
    import torch
    n, h, w, _ = img.shape
    _, X32, Y32 = positions(pred.detach().numpy(), scale)
    s = float(np.float32(scale))
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    x, y = gx[None] + s * pred[..., 0], gy[None] + s * pred[..., 1]
    x = x + (torch.from_numpy(X32.astype(np.float64)) - x).detach()
    y = y + (torch.from_numpy(Y32.astype(np.float64)) - y).detach()
    x0 = x.detach().trunc().long()
    y0 = y.detach().trunc().long()
    x1, y1 = (x0 + 1).clamp(0, w - 1), (y0 + 1).clamp(0, h - 1)
    x0, y0 = x0.clamp(0, w - 1), y0.clamp(0, h - 1)
    src = torch.as_tensor(np.asarray(img, np.float64))[torch.as_tensor(partner(n))]
    b = torch.arange(n)[:, None, None]
    Ia, Ib, Ic, Id = src[b, y0, x0], src[b, y1, x0], src[b, y0, x1], src[b, y1, x1]
    x0f, x1f, y0f, y1f = (v.double() for v in (x0, x1, y0, y1))
    wa, wb = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f)
    wc, wd = (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
    warped = wa[..., None] * Ia + wb[..., None] * Ib + wc[..., None] * Ic + wd[..., None] * Id
    diff = torch.as_tensor(np.asarray(img, np.float64)) - warped
    m = torch.as_tensor(np.asarray(mask, np.float64).reshape(n, h, w, 1))
    psi = (diff.abs() + 0.01) ** q * m                           # abs_robust_loss, :389-390
    return weight * psi.sum() / (m.sum() * 2 + 1e-6)             # loss_mean, :392
