"""``src.census`` -- the ternary census data term of unsupervised training, on libflownet2_hip.so (fn2_census_warp /
fn2_census_cost / fn2_census_grad): UnFlow's soft Hamming distance between the 7 x 7 census descriptors
of a frame's grey values and of its partner's grey values warped by ``tf_warp``, under ``abs_robust_loss`` in its
``loss_mean`` form (the reference's src/utils.py:378-395) as DDFlow's ``census_loss`` applies it.  Where the photometric
loss of src/photometric.py needs brightness constancy, this term compares the ORDER of the grey values around a pixel.

The slot layout is src/photometric.py's: the batch is even, image ``j`` is a frame and image ``j ^ 1`` its partner.

``census_loss(images, pred)`` is one level on device tensors; the trainer builds one table for the scales that hold a
7 x 7 patch (``level`` / ``level_table``) and launches the three entry points once each."""
import torch

from . import _hip
from .photometric import check_constants

RADIUS = 3
PATCH = 2 * RADIUS + 1  # a level with min(h, w) < PATCH has no interior pixel: loss 0, gradient 0
DATA_TERMS = ("photometric", "census")


def check_data_term(data_term, unsupervised):
    """'photometric' or 'census'; census only without ground truth."""
    if data_term not in DATA_TERMS:
        raise ValueError("data_term must be 'photometric' or 'census', got %r" % (data_term,))
    if data_term == "census" and not unsupervised:
        raise ValueError("data_term 'census' is a term of the unsupervised loss: it needs unsupervised=True")
    return data_term


def _check(images, pred, mask):
    """The argument rules, before anything touches the device: shapes first, then where the tensors live."""
    for name, t in (("images", images), ("pred", pred)) + ((("mask", mask),) if mask is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError("census_loss: %s must be a device tensor, got %r" % (name, type(t)))
    for name, t in (("images", images), ("pred", pred)):
        if t.ndim != 4:
            raise ValueError("census_loss: %s must have rank 4, got shape %s" % (name, tuple(t.shape)))
    si, sp = tuple(images.shape), tuple(pred.shape)
    if si[3] != 3:
        raise ValueError("census_loss: images must have 3 channels, got %d" % si[3])
    if sp[3] != 2:
        raise ValueError("census_loss: pred must have 2 channels, got %d" % sp[3])
    if si[:3] != sp[:3]:
        raise ValueError("census_loss: images %s and pred %s must have the same batch, height and width" % (si, sp))
    if 0 in si:
        raise ValueError("census_loss: empty images %s" % (si,))
    if si[0] % 2:
        raise ValueError("census_loss: the batch must be even (two slots per pair), got %d" % si[0])
    if mask is not None and tuple(mask.shape) not in (si[:3], si[:3] + (1,)):
        raise ValueError("census_loss: mask %s must be [N,h,w] or [N,h,w,1] for images %s" % (tuple(mask.shape), si))
    if not (images.is_cuda and pred.is_cuda and (mask is None or mask.is_cuda)):
        raise ValueError("census_loss: images, pred and mask must be device tensors (the loss runs on the GPU only)")


def level(pred, img, mask, dpred, grey, warp, valid, coef, count, scale, weight):
    """One fn2_census_level over contiguous fp32 device tensors: warp holds the planes W, DX, DY ([3,n,h,w]), coef the
    planes S and c ([2,n,h,w])."""
    for t in (pred, img, mask, dpred, grey, warp, valid, coef, count):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("census level: contiguous float32 device tensors only")
    n, h, w, _ = pred.shape
    npix = n * h * w
    if (tuple(img.shape) != (n, h, w, 3) or tuple(dpred.shape) != tuple(pred.shape) or mask.numel() != npix
            or grey.numel() != npix or valid.numel() != npix or warp.numel() != 3 * npix or coef.numel() != 2 * npix
            or count.numel() != 1):
        raise ValueError("census level: pred %s, img %s, mask %s, dpred %s, grey %s, warp %s, valid %s, coef %s and count %s "
                         "do not belong together" % tuple(tuple(t.shape) for t in (pred, img, mask, dpred, grey, warp, valid,
                                                                                   coef, count)))
    return _hip.Fn2CensusLevel(pred.data_ptr(), img.data_ptr(), mask.data_ptr(), dpred.data_ptr(), grey.data_ptr(),
                               warp.data_ptr(), valid.data_ptr(), coef.data_ptr(), count.data_ptr(), h, w, float(scale),
                               float(weight))


def level_table(levels):
    return (_hip.Fn2CensusLevel * len(levels))(*levels)


def census_loss(images, pred, mask=None, scale=1.0, weight=1.0, q=0.4, grad_mult=1.0):
    """One level.  images [N,h,w,3] (slot layout, already at the level's size), pred [N,h,w,2]; f = scale * pred is the flow
    in pixels; mask [N,h,w] or [N,h,w,1] of 0 / 1 (the occlusion mask; None: every pixel, so that m = V).  Returns
    (loss [1], S [N,h,w], count [1], dpred [N,h,w,2]) and a dict of the intermediate buffers G, W, DX, DY, V, c -- all
    device tensors."""
    _check(images, pred, mask)
    _, _, q = check_constants(0.0, 0.0, q)
    with torch.cuda.device(images.device):
        img = images.detach().to(torch.float32).contiguous()
        prd = pred.detach().to(torch.float32).contiguous()
        n, h, w, _ = prd.shape
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=img.device)
        msk = (torch.ones((n, h, w), dtype=torch.float32, device=img.device) if mask is None
               else mask.detach().to(torch.float32).reshape(n, h, w).contiguous())
        dpred, grey, warp, valid, coef = torch.empty_like(prd), new(n, h, w), new(3, n, h, w), new(n, h, w), new(2, n, h, w)
        scalars = torch.zeros(2, dtype=torch.float32, device=img.device)  # [loss, count]
        table = level_table([level(prd, img, msk, dpred, grey, warp, valid, coef, scalars[1:], scale, weight)])
        lib, s = _hip.lib(), _hip.stream_ptr()
        _hip.check(lib.fn2_census_warp(table, 1, n, s))
        _hip.check(lib.fn2_census_cost(table, 1, n, q, _hip.ptr(scalars), s))
        _hip.check(lib.fn2_census_grad(table, 1, n, float(grad_mult), s))
    return scalars[0:1], coef[0], scalars[1:2], dpred, dict(G=grey, W=warp[0], DX=warp[1], DY=warp[2], V=valid, c=coef[1])
