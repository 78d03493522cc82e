"""``src.photometric`` -- the occlusion-aware photometric loss of unsupervised training, on libflownet2_hip.so
(fn2_photometric_masks / fn2_photometric_loss_grad): SelFlow's ``abs_robust_loss`` (the reference's src/utils.py:378-395,
its ``loss_mean``) of a frame minus its partner warped by ``tf_warp`` (:453-515), over the pixels that the
forward-backward test (``occlusion``, :523-538) leaves and that sample inside the partner frame.  The reference carries
the pieces (:354-538) and never joins them.

Slot layout: the batch is even; image ``j`` is a frame and image ``j ^ 1`` its partner, the prediction of slot ``j ^ 1``
the partner flow (pair k in slots 2k and 2k + 1, one per direction -- ``interleave_pairs``).

``photometric_loss(images, pred)`` is one level on device tensors; the trainer builds one table for its five scales
(``level`` / ``level_table``) and launches the two entry points once each."""
import torch

from . import _hip


def _check(images, pred):
    """The argument rules, before anything touches the device: shapes first, then where the tensors live."""
    for name, t in (("images", images), ("pred", pred)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("photometric_loss: %s must be a device tensor, got %r" % (name, type(t)))
        if t.ndim != 4:
            raise ValueError("photometric_loss: %s must have rank 4, got shape %s" % (name, tuple(t.shape)))
    si, sp = tuple(images.shape), tuple(pred.shape)
    if si[3] != 3:
        raise ValueError("photometric_loss: images must have 3 channels, got %d" % si[3])
    if sp[3] != 2:
        raise ValueError("photometric_loss: pred must have 2 channels, got %d" % sp[3])
    if si[:3] != sp[:3]:
        raise ValueError("photometric_loss: images %s and pred %s must have the same batch, height and width" % (si, sp))
    if 0 in si:
        raise ValueError("photometric_loss: empty images %s" % (si,))
    if si[0] % 2:
        raise ValueError("photometric_loss: the batch must be even (two slots per pair), got %d" % si[0])
    if not (images.is_cuda and pred.is_cuda):
        raise ValueError("photometric_loss: images and pred must be device tensors (the loss runs on the GPU only)")


def check_constants(alpha, beta, q):
    """alpha, beta >= 0 and 0 < q <= 1 (NaN refused), as floats."""
    alpha, beta, q = float(alpha), float(beta), float(q)
    if not alpha >= 0.0 or not beta >= 0.0:
        raise ValueError("occlusion constants must be >= 0, got alpha=%r beta=%r" % (alpha, beta))
    if not 0.0 < q <= 1.0:
        raise ValueError("photometric q must lie in (0, 1], got %r" % (q,))
    return alpha, beta, q


def level(pred, img, mask, mask_sum, dpred, scale, weight):
    """One fn2_photometric_level over contiguous fp32 device tensors."""
    for t in (pred, img, mask, mask_sum, dpred):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("photometric level: contiguous float32 device tensors only")
    n, h, w, _ = pred.shape
    if tuple(img.shape) != (n, h, w, 3) or mask.numel() != n * h * w or tuple(dpred.shape) != tuple(pred.shape):
        raise ValueError("photometric level: pred %s, img %s, mask %s and dpred %s do not belong together"
                         % (tuple(pred.shape), tuple(img.shape), tuple(mask.shape), tuple(dpred.shape)))
    return _hip.Fn2PhotometricLevel(pred.data_ptr(), img.data_ptr(), mask.data_ptr(), mask_sum.data_ptr(),
                                    dpred.data_ptr(), h, w, float(scale), float(weight))


def level_table(levels):
    return (_hip.Fn2PhotometricLevel * len(levels))(*levels)


def interleave_pairs(image_a, image_b, out_a, out_b):
    """[P,H,W,3] frames -> the 2P slots: out_a = (a_0, b_0, a_1, b_1, ...), out_b = (b_0, a_0, b_1, a_1, ...)."""
    out_a[0::2].copy_(image_a, non_blocking=True)
    out_a[1::2].copy_(image_b, non_blocking=True)
    out_b[0::2].copy_(image_b, non_blocking=True)
    out_b[1::2].copy_(image_a, non_blocking=True)


def photometric_loss(images, pred, scale=1.0, weight=1.0, alpha=0.01, beta=0.5, q=0.4, grad_mult=1.0):
    """One level.  images [N,h,w,3] (slot layout, already at the level's size), pred [N,h,w,2]; f = scale * pred is the
    flow in pixels.  Returns (loss [1], mask [N,h,w,1] 0 / 1, mask count [1], dpred [N,h,w,2]), device tensors."""
    _check(images, pred)
    alpha, beta, q = check_constants(alpha, beta, q)
    with torch.cuda.device(images.device):
        img = images.detach().to(torch.float32).contiguous()
        prd = pred.detach().to(torch.float32).contiguous()
        n, h, w, _ = prd.shape
        mask = torch.empty((n, h, w, 1), dtype=torch.float32, device=img.device)
        dpred = torch.empty_like(prd)
        scalars = torch.zeros(2, dtype=torch.float32, device=img.device)  # [loss, mask count]
        table = level_table([level(prd, img, mask, scalars[1:], dpred, scale, weight)])
        lib, s = _hip.lib(), _hip.stream_ptr()
        _hip.check(lib.fn2_photometric_masks(table, 1, n, alpha, beta, s))
        _hip.check(lib.fn2_photometric_loss_grad(table, 1, n, q, float(grad_mult), _hip.ptr(scalars), s))
    return scalars[0:1], mask, scalars[1:2], dpred
