"""``src.sparse_epe`` -- the multi-scale endpoint error over sparse ground truth (KITTI, HD1K, Middlebury), on
libflownet2_hip.so (fn2_sparse_epe_count, fn2_sparse_epe_loss_grad, csrc/sparse_epe.hip).  A label pixel whose u or v is not
finite carries no ground truth: it takes no part in the loss and gets a gradient of exactly +0; the loss of a level is
weight * (h w) * sum_valid ||pred - label|| / M with M the number of valid pixels of the batch, which is
average_endpoint_error when every label is finite (include/flownet2_hip.h has the definition).

``sparse_epe_loss(pred, label, weight)`` is one level on device tensors; the trainer launches each entry point once for
its five scales on ``level_table``."""
import math

import torch

from . import _hip

MAX_LEVELS = 8


def _check(pred, label):
    """The argument rules, before anything touches the device: shapes and dtype first, then where the tensors live."""
    for name, t in (("pred", pred), ("label", label)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("sparse_epe_loss: %s must be a device tensor, got %r" % (name, type(t)))
        if t.ndim != 4:
            raise ValueError("sparse_epe_loss: %s must have rank 4, got shape %s" % (name, tuple(t.shape)))
        if t.shape[3] != 2:
            raise ValueError("sparse_epe_loss: %s must have 2 channels, got %d" % (name, t.shape[3]))
        if not t.dtype.is_floating_point:
            raise ValueError("sparse_epe_loss: %s must be a floating-point tensor, got %s" % (name, t.dtype))
    if tuple(pred.shape) != tuple(label.shape):
        raise ValueError("sparse_epe_loss: pred %s and label %s must have the same shape"
                         % (tuple(pred.shape), tuple(label.shape)))
    if 0 in pred.shape:
        raise ValueError("sparse_epe_loss: empty pred %s" % (tuple(pred.shape),))
    if pred.shape[0] * pred.shape[1] * pred.shape[2] >= 1 << 31:
        raise ValueError("sparse_epe_loss: n*h*w must be below 2^31, got shape %s" % (tuple(pred.shape),))
    if not (pred.is_cuda and label.is_cuda):
        raise ValueError("sparse_epe_loss: pred and label must be device tensors (the loss runs on the GPU only)")


def check_constants(weight, grad_mult):
    """Finite weight >= 0 and finite grad_mult > 0 (NaN refused), as floats."""
    weight, grad_mult = float(weight), float(grad_mult)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError("sparse EPE weight must be finite and >= 0, got %r" % (weight,))
    if not (math.isfinite(grad_mult) and grad_mult > 0.0):
        raise ValueError("sparse EPE grad_mult must be finite and > 0, got %r" % (grad_mult,))
    return weight, grad_mult


def level(pred, label, dpred, count, weight):
    """One fn2_sparse_epe_level over contiguous device tensors: pred, label, dpred fp32 [n,h,w,2], count one 4-byte
    integer."""
    for t in (pred, label, dpred):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise ValueError("sparse EPE level: contiguous float32 device tensors only")
    if not (count.is_cuda and count.element_size() == 4 and not count.dtype.is_floating_point and count.numel() == 1):
        raise ValueError("sparse EPE level: count must be one 32-bit integer on the device")
    if pred.ndim != 4 or pred.shape[3] != 2 or tuple(label.shape) != tuple(pred.shape) or tuple(dpred.shape) != tuple(pred.shape):
        raise ValueError("sparse EPE level: pred %s, label %s and dpred %s do not belong together"
                         % (tuple(pred.shape), tuple(label.shape), tuple(dpred.shape)))
    n, h, w, _ = pred.shape
    return _hip.Fn2SparseEpeLevel(pred.data_ptr(), label.data_ptr(), dpred.data_ptr(), count.data_ptr(), h, w,
                                  check_constants(weight, 1.0)[0])


def level_table(levels):
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError("sparse EPE: 1..%d levels, got %d" % (MAX_LEVELS, len(levels)))
    return (_hip.Fn2SparseEpeLevel * len(levels))(*levels)


def sparse_epe_loss(pred, label, weight, grad_mult=1.0):
    """One level.  pred, label [N,h,w,2]; a label pixel with a non-finite component carries no ground truth.
    Returns (loss [1], dpred [N,h,w,2], M [1] int32), device tensors."""
    _check(pred, label)
    weight, grad_mult = check_constants(weight, grad_mult)
    with torch.cuda.device(pred.device):
        prd = pred.detach().to(torch.float32).contiguous()
        lab = label.detach().to(device=prd.device, dtype=torch.float32).contiguous()
        n = prd.shape[0]
        dpred = torch.empty_like(prd)
        loss = torch.zeros(1, dtype=torch.float32, device=prd.device)
        count = torch.zeros(1, dtype=torch.int32, device=prd.device)
        table = level_table([level(prd, lab, dpred, count, weight)])
        s = _hip.stream_ptr()
        _hip.check(_hip.lib().fn2_sparse_epe_count(table, 1, n, s))
        _hip.check(_hip.lib().fn2_sparse_epe_loss_grad(table, 1, n, grad_mult, _hip.ptr(loss), s))
    return loss, dpred, count
