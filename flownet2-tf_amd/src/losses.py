"""Training losses of the reference (FlowNetS.loss, src/flownet_s/flownet_s.py:122-161;
average_endpoint_error, src/utils.py:209-224; FlowNet2.loss, src/flownet2/flownet2.py:107-116).
The NaN-aware ground-truth downsample (with the label scaling inside it) and the endpoint-error reductions are
calls into libflownet2_hip.so (fn2_downsample_scaled_f32, fn2_epe_loss_grad), and so are the pixel weights of the
mining modes of FlowNetS_interp's loss that the trainer uses (hard_example_weights: fn2_hfem_hard_weights); only the
scalar average_endpoint_error_hfem below still selects with torch.topk."""
import numpy as np
import torch

from . import _hip
from .downsample import downsample

LOSS_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)


def _dev32(x, like=None):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=_hip.require_device() if like is None else like.device, dtype=torch.float32).contiguous()


def average_endpoint_error(labels, predictions):
    """sum over pixels of ||pred - label||_2, divided by the batch size only (utils.py:209-224): fn2_epe_loss_grad's
    loss output (its gradient output goes to a scratch tensor)."""
    pred = _dev32(predictions)
    lab = _dev32(labels, pred)
    if lab.shape != pred.shape or pred.ndim != 4 or pred.shape[3] != 2:
        raise ValueError("average_endpoint_error: labels and predictions must both be [N, H, W, 2]")
    n, h, w, _ = pred.shape
    lib, s = _hip.lib(), _hip.stream_ptr()
    scratch = torch.empty_like(pred)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    _hip.check(lib.fn2_fill_zero(_hip.ptr(loss), 4, s))
    _hip.check(lib.fn2_epe_loss_grad(_hip.ptr(pred), _hip.ptr(lab), _hip.ptr(scratch), _hip.ptr(loss), n, h, w, 1.0, 1.0, s))
    return loss[0]


def scaled_downsample(flow, scale, size):
    """downsample(scale * flow, size) in one pass (flownet_s.py:123-129): fn2_downsample_scaled_f32."""
    x = _dev32(flow)
    n, h, w, c = x.shape
    out = torch.empty((n, int(size[0]), int(size[1]), c), dtype=torch.float32, device=x.device)
    _hip.check(_hip.lib().fn2_downsample_scaled_f32(_hip.ptr(x), float(scale), _hip.ptr(out), n, h, w, c, int(size[0]),
                                                    int(size[1]), _hip.stream_ptr()))
    return out


def average_endpoint_error_hfem(labels, predictions, add_hfem='', lambda_w=2., perc_hfem=50, edges=None):
    """AEPE with optional hard-flow-example mining (src/utils.py:227-339).  add_hfem: '' plain AEPE; 'hard': only
    the round(perc_hfem % of all pixels of the batch) largest EPE values count, weighted (1 + lambda_w), divided by
    the batch size and scaled by #pixels / #hard pixels; 'edges': EPE map weighted by (1 + lambda_w * edges)."""
    n = predictions.shape[0]
    epe = torch.linalg.vector_norm(labels.float() - predictions.float(), dim=3, keepdim=True)
    mode = (add_hfem or '').lower()
    if mode == 'hard':
        flat = epe.reshape(-1)
        k = int(np.round(np.float32(perc_hfem / 100) * np.float32(flat.numel())))
        hard = torch.topk(flat, k).values
        return (1.0 + lambda_w) * hard.sum() / n * (flat.numel() / max(k, 1))
    if mode == 'edges' and edges is not None:
        return (epe + lambda_w * epe * _as_dev(edges, epe).float()).sum() / n
    return epe.sum() / n


def hard_k(numel, perc_hfem):
    """Number of hard pixels among `numel`: round(perc_hfem / 100 * numel) in fp32 with tf.round's half-to-even
    (utils.py:268-275)."""
    return int(np.round(np.float32(perc_hfem / 100) * np.float32(numel)))


def hfem_level(pred, label, epe, weight, k, hard_weight):
    """One fn2_hfem_level over contiguous fp32 device tensors (pred, label [..., 2]; epe, weight one value per pixel)."""
    return _hip.Fn2HfemLevel(pred.data_ptr(), label.data_ptr(), epe.data_ptr(), weight.data_ptr(), epe.numel(), int(k),
                             float(hard_weight))


def hard_weight_of(numel, k, lambda_w):
    """(1 + lambda) * #pixels / #hard pixels as fp32 (utils.py:305-312); 0 when no pixel is hard."""
    return np.float32((1.0 + lambda_w) * (numel / k)) if k > 0 else np.float32(0.0)


def hard_example_weights(labels, predictions, perc_hfem=50, lambda_w=2.0, return_epe=False):
    """The pixel weights of the 'hard' mining mode for one [N,H,W,2] pair of device tensors: (1 + lambda_w) * N H W / k
    on the k = hard_k(N H W, perc_hfem) pixels of the batch with the largest endpoint error, 0 elsewhere.  Equal values
    are taken in index order, as tf.nn.top_k takes them (utils.py:282).  One fn2_hfem_hard_weights launch, no sort.
    Returns the [N,H,W] fp32 weight map, and with return_epe the [N,H,W] endpoint-error map as well."""
    if not 0 <= perc_hfem <= 100:
        raise ValueError("hard_example_weights: perc_hfem must lie in [0, 100], not %r" % (perc_hfem,))
    if not (isinstance(labels, torch.Tensor) and isinstance(predictions, torch.Tensor)):
        raise ValueError("hard_example_weights: labels and predictions must be device tensors")
    if labels.shape != predictions.shape or predictions.ndim != 4 or predictions.shape[3] != 2:
        raise ValueError("hard_example_weights: labels and predictions must both be [N, H, W, 2]")
    if not (labels.is_cuda and predictions.is_cuda):
        raise ValueError("hard_example_weights: labels and predictions must be device tensors, not CPU tensors")
    pred = predictions.detach().to(dtype=torch.float32).contiguous()
    lab = labels.detach().to(device=pred.device, dtype=torch.float32).contiguous()
    n, h, w, _ = pred.shape
    numel = n * h * w
    if numel < 1:
        raise ValueError("hard_example_weights: empty tensors")
    k = hard_k(numel, perc_hfem)
    epe = torch.empty((n, h, w), dtype=torch.float32, device=pred.device)
    weight = torch.empty_like(epe)
    level = hfem_level(pred, lab, epe, weight, k, hard_weight_of(numel, k, lambda_w))
    _hip.check(_hip.lib().fn2_hfem_hard_weights(level, 1, _hip.stream_ptr()))
    return (weight, epe) if return_epe else weight


def mean_endpoint_error(gt_flow, pred_flow):
    """Mean over every pixel of the batch of ||gt - pred||_2 (src/utils.py:342-351) = average_endpoint_error / (H W)."""
    pred = _dev32(pred_flow)
    return average_endpoint_error(gt_flow, pred) / float(pred.shape[1] * pred.shape[2])


def multiscale_hfem_loss(targets, predictions, add_hard_flow_mining='', lambda_weight=2., hard_examples_perc=50,
                         edges=None, weights=None, scope=None, l2=4e-4):
    """FlowNetS_interp.loss (src/flownet_s_interp/flownet_s_interp.py:159-254): the five-scale weighted sum of
    average_endpoint_error_hfem on 0.05 * targets (edges downsampled per scale with the same NaN-aware op), + the
    slim L2 terms; returns (total loss, AEPE) where AEPE compares the SCALED targets with predictions['flow']
    exactly as the reference does (:251)."""
    p6 = predictions['predict_flow6']
    t = _as_dev(targets, p6).to(device=p6.device, dtype=torch.float32) * 0.05
    e = None if edges is None else _as_dev(edges, p6).to(device=p6.device, dtype=torch.float32)
    losses = []
    for lvl in (6, 5, 4, 3, 2):
        p = predictions['predict_flow%d' % lvl]
        size = [p.shape[1], p.shape[2]]
        e_l = downsample(e, size) if (e is not None and add_hard_flow_mining) else e
        losses.append(average_endpoint_error_hfem(downsample(t, size), p, add_hard_flow_mining, lambda_weight,
                                                  hard_examples_perc, e_l))
    total = sum(w * l for w, l in zip(LOSS_WEIGHTS, losses)) / 5.0
    if weights is not None and scope is not None:
        total = total + sum(0.5 * l2 * float(np.sum(np.square(np.asarray(w, np.float64))))
                            for name, w in weights.items()
                            if name.startswith(scope + "/") and name.endswith("/weights")
                            and "deconv" not in name and "upsample_flow" not in name)
    return total, mean_endpoint_error(t, predictions['flow'])


def _as_dev(x, like):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), device=like.device)


def multiscale_loss(flow, predictions, weights=None, scope=None, l2=4e-4, gt_scale=0.05):
    p6 = predictions['predict_flow6']
    flow = _dev32(flow, p6)
    losses = []
    for lvl in (6, 5, 4, 3, 2):
        p = predictions['predict_flow%d' % lvl]
        losses.append(average_endpoint_error(scaled_downsample(flow, gt_scale, [p.shape[1], p.shape[2]]), p))
    # tf.losses.compute_weighted_loss(list, weights) with SUM_BY_NONZERO_WEIGHTS: (sum w_i L_i) / 5
    total = sum(w * l for w, l in zip(LOSS_WEIGHTS, losses)) / 5.0
    if weights is not None and scope is not None:
        reg = 0.0
        for name, w in weights.items():
            if name.startswith(scope + "/") and name.endswith("/weights") \
                    and "deconv" not in name and "upsample_flow" not in name:
                reg += 0.5 * l2 * float(np.sum(np.square(np.asarray(w, np.float64))))
        total = total + reg
    return total


def fusion_loss(flow, predictions, weights=None, scope="FlowNet2", l2=4e-4):
    """FlowNet2.loss (src/flownet2/flownet2.py:107-116): average_endpoint_error(downsample(flow, size of
    predict_flow0), predict_flow0) -- the ground truth is NOT scaled and no 0.005 weight is applied, whatever the
    comment at :108 says -- added to the losses collection, then tf.losses.get_total_loss(): + every
    regularisation loss of the graph, i.e. 0.5 * l2 * |W|^2 of ALL slim.conv2d weights under the FlowNet2 scope,
    the frozen CSS / SD sub-networks included (regularisers are attached whether or not a variable is trainable;
    conv2d_transpose weights and biases carry none).  l2: the schedule's l2_regularization (the reference reads a
    'weight_decay' key no schedule defines for the fusion layers -- defect D2 -- the intended value is the same)."""
    p0 = predictions['predict_flow0']
    flow = _as_dev(flow, p0).to(device=p0.device, dtype=torch.float32)
    total = average_endpoint_error(downsample(flow, [p0.shape[1], p0.shape[2]]), p0)
    if weights is not None:
        total = total + sum(0.5 * l2 * float(np.sum(np.square(np.asarray(w, np.float64))))
                            for name, w in weights.items()
                            if name.startswith(scope + "/") and name.endswith("/weights")
                            and "deconv" not in name and "upsample_flow" not in name)
    return total
