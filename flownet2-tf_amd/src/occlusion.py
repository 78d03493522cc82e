"""``src.occlusion`` -- the forward-backward consistency check of /root/reference src/utils.py:426-538
(``tf_warp`` :453-515, ``occlusion`` :523-538, the SelFlow test), on libflownet2_hip.so (fn2_tf_warp_f32 /
fn2_fb_occlusion).  The reference carries the check but never runs it (its comment at :424).

``tf_warp(img, flow)`` -> tensor shaped like ``img`` (NHWC float32): backward bilinear warp with the reference's own
index rules, which are not those of ``flow_warp``: coordinates truncate toward zero, the taps are clamped after the
``+ 1``, nothing is tested for being in range (x in (-1, 0) extrapolates; x <= -1, x >= W - 1 and 1-wide images give
exactly 0).  ``occlusion(flow_fw, flow_bw)`` -> (occ_fw, occ_bw), [N,H,W,1]: float32 0 / 1 as the reference returns
them, or uint8 0 / 255 (``as_uint8``) as a mask file and ``compute_all_metrics`` hold them.

torch tensors (any device) or numpy arrays in, same kind out.  A ROCm tensor that is a crop of a larger buffer
(``buf[:, :h, :w, :]``, ``buf[0::2]``) goes to the library with its strides: nothing is copied."""
import numpy as np
import torch

from . import _hip


def _shape(name, x):
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise TypeError("%s: expected torch.Tensor or numpy.ndarray, got %r" % (name, type(x)))
    return tuple(x.shape)


def _check_warp(img, flow):
    """The shape rules, before anything touches the device."""
    si, sf = _shape("tf_warp: img", img), _shape("tf_warp: flow", flow)
    if len(si) != 4:
        raise ValueError("tf_warp: img must have rank 4, got shape %s" % (si,))
    if len(sf) != 4:
        raise ValueError("tf_warp: flow must have rank 4, got shape %s" % (sf,))
    if sf[3] != 2:
        raise ValueError("tf_warp: flow must have 2 channels, got %d" % sf[3])
    if si[:3] != sf[:3]:
        raise ValueError("tf_warp: img %s and flow %s must have the same batch, height and width" % (si, sf))
    if 0 in si:
        raise ValueError("tf_warp: empty img %s" % (si,))


def _check_flows(flow_fw, flow_bw):
    sf, sb = _shape("occlusion: flow_fw", flow_fw), _shape("occlusion: flow_bw", flow_bw)
    for name, s in (("flow_fw", sf), ("flow_bw", sb)):
        if len(s) != 4:
            raise ValueError("occlusion: %s must have rank 4, got shape %s" % (name, s))
        if s[3] != 2:
            raise ValueError("occlusion: %s must have 2 channels, got %d" % (name, s[3]))
    if sf != sb:
        raise ValueError("occlusion: flow_fw %s and flow_bw %s must have the same shape" % (sf, sb))
    if 0 in sf:
        raise ValueError("occlusion: empty flow %s" % (sf,))


def _device_f32(x):
    """(float32 ROCm tensor, kind).  A float32 ROCm tensor comes back as it is -- strides and all."""
    if isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32:
        return x.detach(), "cuda"
    return _hip.to_device_f32(x)


def _strides(t, even=False):
    """(pitch, batch stride) in floats of t [N,H,W,C] if the library can read it in place: pixels packed, rows and
    images not overlapping -- and, for a flow (`even`), 8-byte pairs.  None if it needs a copy.  A single row or image
    has no stride of its own."""
    n, h, w, c = t.shape
    if (c > 1 and t.stride(3) != 1) or (w > 1 and t.stride(2) != c):
        return None
    pitch = t.stride(1) if h > 1 else c * w
    bstride = t.stride(0) if n > 1 else pitch * h
    if pitch < c * w or bstride < pitch * h:
        return None
    if even and (pitch % 2 or bstride % 2 or t.data_ptr() % 8):
        return None
    return pitch, bstride


def _in_place(t, even=False):
    s = _strides(t, even)
    if s is None:
        t = t.clone(memory_format=torch.contiguous_format)  # (a dense tensor at an odd offset needs the copy too)
        s = _strides(t, even)
    return t, s


def tf_warp(img, flow):
    """utils.py:453-515 (the reference passes H and W as well; they are the image's)."""
    _check_warp(img, flow)
    im, kind = _device_f32(img)
    fl, _ = _device_f32(flow)
    n, h, w, c = im.shape
    im, (ip, ib) = _in_place(im)
    fl, (fp, fb) = _in_place(fl, even=True)
    with torch.cuda.device(im.device):
        out = torch.empty((n, h, w, c), dtype=torch.float32, device=im.device)
        _hip.check(_hip.lib().fn2_tf_warp_f32(_hip.ptr(im), ip, ib, _hip.ptr(fl), fp, fb, _hip.ptr(out), n, h, w, c,
                                              _hip.stream_ptr()))
    return _hip.from_device(out, kind)


def occlusion(flow_fw, flow_bw, alpha=0.01, beta=0.5, as_uint8=False):
    """utils.py:523-538 with its two constants as arguments.  Returns (occ_fw, occ_bw), [N,H,W,1]."""
    _check_flows(flow_fw, flow_bw)
    fw, kind = _device_f32(flow_fw)
    bw, _ = _device_f32(flow_bw)
    n, h, w, _ = fw.shape
    fw, sf = _in_place(fw, even=True)
    bw, sb = _in_place(bw, even=True)
    if sf != sb:  # one pitch and one batch stride serve both
        fw, bw = (t.clone(memory_format=torch.contiguous_format) for t in (fw, bw))
        sf = _strides(fw, even=True)
    with torch.cuda.device(fw.device):
        dtype = torch.uint8 if as_uint8 else torch.float32
        occ_fw = torch.empty((n, h, w, 1), dtype=dtype, device=fw.device)
        occ_bw = torch.empty_like(occ_fw)
        _hip.check(_hip.lib().fn2_fb_occlusion(_hip.ptr(fw), _hip.ptr(bw), sf[0], sf[1], _hip.ptr(occ_fw), _hip.ptr(occ_bw),
                                               _hip.MASK_U8 if as_uint8 else _hip.MASK_F32, n, h, w, float(alpha),
                                               float(beta), _hip.stream_ptr()))
    return _hip.from_device(occ_fw, kind), _hip.from_device(occ_bw, kind)
