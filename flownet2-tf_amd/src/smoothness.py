"""``src.smoothness`` -- the edge-aware smoothness term of unsupervised training, on libflownet2_hip.so
(fn2_smoothness_loss_grad, csrc/smoothness.hip).  An addition to the reference, which has no flow regulariser: a first- or
second-order difference of the flow f = scale * pred under rho(d) = sqrt(d^2 + eps^2), every term weighted by
exp(-edge_lambda * mean |image difference|) across it, averaged per axis (include/flownet2_hip.h has the definition).

``smoothness_loss(images, pred)`` is one level on device tensors; the trainer launches the entry point once for its five
scales, on the level table of the photometric loss (``src.photometric.level_table``), behind that loss."""
import math

import torch

from . import _hip


def _check(images, pred):
    """The argument rules, before anything touches the device: shapes first, then where the tensors live."""
    for name, t in (("images", images), ("pred", pred)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("smoothness_loss: %s must be a device tensor, got %r" % (name, type(t)))
        if t.ndim != 4:
            raise ValueError("smoothness_loss: %s must have rank 4, got shape %s" % (name, tuple(t.shape)))
    si, sp = tuple(images.shape), tuple(pred.shape)
    if si[3] != 3:
        raise ValueError("smoothness_loss: images must have 3 channels, got %d" % si[3])
    if sp[3] != 2:
        raise ValueError("smoothness_loss: pred must have 2 channels, got %d" % sp[3])
    if si[:3] != sp[:3]:
        raise ValueError("smoothness_loss: images %s and pred %s must have the same batch, height and width" % (si, sp))
    if 0 in si:
        raise ValueError("smoothness_loss: empty images %s" % (si,))
    if not (images.is_cuda and pred.is_cuda):
        raise ValueError("smoothness_loss: images and pred must be device tensors (the loss runs on the GPU only)")


def check_constants(order, edge_lambda, eps, smooth_weight):
    """order 1 or 2, finite edge_lambda >= 0, eps > 0 and smooth_weight >= 0 (NaN refused), as (int, float, float, float)."""
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError("smoothness order must be 1 or 2, got %r" % (order,))
    edge_lambda, eps, smooth_weight = float(edge_lambda), float(eps), float(smooth_weight)
    if not (math.isfinite(edge_lambda) and edge_lambda >= 0.0):
        raise ValueError("edge_lambda must be finite and >= 0, got %r" % (edge_lambda,))
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("smoothness eps must be finite and > 0, got %r" % (eps,))
    if not (math.isfinite(smooth_weight) and smooth_weight >= 0.0):
        raise ValueError("smoothness weight must be finite and >= 0, got %r" % (smooth_weight,))
    return int(order), edge_lambda, eps, smooth_weight


def smoothness_loss(images, pred, scale=1.0, weight=1.0, order=1, edge_lambda=150.0, eps=1e-3, smooth_weight=1.0,
                    grad_mult=1.0):
    """One level.  images [N,h,w,3] (already at the level's size), pred [N,h,w,2]; f = scale * pred is the flow in pixels.
    Returns (loss [1], dpred [N,h,w,2]), device tensors."""
    _check(images, pred)
    order, edge_lambda, eps, smooth_weight = check_constants(order, edge_lambda, eps, smooth_weight)
    with torch.cuda.device(images.device):
        img = images.detach().to(torch.float32).contiguous()
        prd = pred.detach().to(torch.float32).contiguous()
        n, h, w, _ = prd.shape
        dpred = torch.empty_like(prd)
        loss = torch.zeros(1, dtype=torch.float32, device=img.device)
        table = (_hip.Fn2PhotometricLevel * 1)(_hip.Fn2PhotometricLevel(
            prd.data_ptr(), img.data_ptr(), None, None, dpred.data_ptr(), h, w, float(scale), float(weight)))
        _hip.check(_hip.lib().fn2_smoothness_loss_grad(table, 1, n, order, edge_lambda, eps, smooth_weight,
                                                       float(grad_mult), 0, _hip.ptr(loss), _hip.stream_ptr()))
    return loss, dpred
