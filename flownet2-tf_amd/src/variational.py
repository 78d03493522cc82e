"""``src.variational`` -- the EpicFlow variational refinement of the reference (src/SrcVariational, run by
utils.py:542-555 ``calc_variational_inference_map`` on the network's cropped flow), on libflownet2_hip.so
(fn2_variational_refine).

``refine(flow, img_a, img_b, preset=None, **params)`` refines ROCm device tensors: flow float32 [N,]H,W,2 and uint8
RGB frames [N,]H,W,3 of the same size.  The frames may be views into larger (padded) buffers: rows and pairs are
read through their strides, without a copy.  ``calc_variational_inference_map`` keeps the reference's file-in /
file-out signature.
"""
import numpy as np
import torch

from . import _hip

# variational_params_default (src/SrcVariational/variational.c:85-98): what the reference ALWAYS runs with
DEFAULTS = dict(alpha=1.0, gamma=0.71, delta=0.0, sigma=1.0, niter_outer=5, niter_inner=1, niter_solver=30,
                sor_omega=1.9)

# the binary's presets (variational_main.cpp:63-84); each overrides these fields of the defaults
PRESETS = {
    "sintel": dict(niter_outer=5, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
    "kitti": dict(niter_outer=2, alpha=1.0, gamma=0.77, delta=0.0, sigma=1.7),
    "middlebury": dict(niter_outer=25, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1),
}

_INT_PARAMS = ("niter_outer", "niter_inner", "niter_solver")


def params_for(preset=None, **params):
    """The parameter set of a refinement: the defaults, then the preset's fields, then explicit overrides."""
    out = dict(DEFAULTS)
    if preset is not None:
        if preset not in PRESETS:
            raise ValueError("unknown preset %r (expected None or one of %s)" % (preset, sorted(PRESETS)))
        out.update(PRESETS[preset])
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise TypeError("unknown variational parameter(s): %s" % ", ".join(sorted(unknown)))
    out.update(params)
    for k in _INT_PARAMS:
        if int(out[k]) != out[k] or out[k] < 0:
            raise ValueError("%s must be a non-negative integer, got %r" % (k, out[k]))
        out[k] = int(out[k])
    if not out["sigma"] > 0:
        raise ValueError("sigma must be > 0, got %r" % out["sigma"])
    return out


def binary_params(dataset):
    """What ``variational_main A B in.flo out.flo <dataset>`` runs with: its option loop starts at argv[6]
    (variational_main.cpp:50), so the fifth argument -- the dataset name utils.py:551 passes -- is never read and
    every call gets the defaults."""
    del dataset
    return dict(DEFAULTS)


def _check(flow, img_a, img_b):
    for name, t in (("flow", flow), ("img_a", img_a), ("img_b", img_b)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("refine: %s must be a torch.Tensor, got %r" % (name, type(t)))
    if flow.dtype != torch.float32:
        raise TypeError("refine: flow must be float32, got %s" % flow.dtype)
    for name, t in (("img_a", img_a), ("img_b", img_b)):
        if t.dtype != torch.uint8:
            raise TypeError("refine: %s must be uint8 RGB, got %s" % (name, t.dtype))
    if flow.dim() not in (3, 4) or flow.shape[-1] != 2:
        raise ValueError("refine: flow must be [N,]H,W,2, got %s" % (tuple(flow.shape),))
    want = tuple(flow.shape[:-1]) + (3,)
    for name, t in (("img_a", img_a), ("img_b", img_b)):
        if tuple(t.shape) != want:
            raise ValueError("refine: %s must be %s to match the flow, got %s" % (name, want, tuple(t.shape)))
    if any(d == 0 for d in flow.shape):
        raise ValueError("refine: empty flow %s" % (tuple(flow.shape),))
    for name, t in (("flow", flow), ("img_a", img_a), ("img_b", img_b)):
        if not t.is_cuda:
            raise ValueError("refine: %s is on %s; the refinement runs on the ROCm device only (no CPU path)"
                             % (name, t.device))
    if not (flow.device == img_a.device == img_b.device):
        raise ValueError("refine: flow and images must be on one device")


def _row_pitch(t, c):
    """Elements between the rows of t (4-D, pixels packed).  A single row has no pitch of its own: views of one-row
    tensors (a transposed column, say) carry whatever stride they were made with."""
    return t.stride(1) if t.shape[1] > 1 else c * t.shape[2]


def _pixel_rows(t, c):
    """t (4-D) if its pixels are packed (c consecutive elements) and its pairs do not overlap, else a copy."""
    if t.stride(-1) != 1 or t.stride(-2) != c or (t.shape[0] > 1 and t.stride(0) < _row_pitch(t, c) * t.shape[1]):
        t = t.contiguous()
    return t


def refine(flow, img_a, img_b, preset=None, inplace=False, **params):
    """Variational refinement of `flow` (float32 [N,]H,W,2) between the uint8 RGB frames `img_a` -> `img_b`
    ([N,]H,W,3, the original unpadded frames; views into padded buffers are read in place).  `preset` None runs
    the reference's defaults (what its binary always uses); 'sintel' / 'kitti' / 'middlebury' are the binary's
    presets; keyword `params` (alpha, gamma, delta, sigma, niter_outer, niter_inner, niter_solver, sor_omega)
    override single fields.  Returns the refined flow (the input tensor itself when `inplace`).  Runs on the
    current stream."""
    _check(flow, img_a, img_b)
    p = params_for(preset, **params)
    squeeze = flow.dim() == 3
    f4 = flow.unsqueeze(0) if squeeze else flow
    a4 = img_a.unsqueeze(0) if squeeze else img_a
    b4 = img_b.unsqueeze(0) if squeeze else img_b
    n, h, w, _ = f4.shape
    a4, b4 = _pixel_rows(a4, 3), _pixel_rows(b4, 3)
    if (_row_pitch(a4, 3), a4.stride(0)) != (_row_pitch(b4, 3), b4.stride(0)):
        a4, b4 = a4.contiguous(), b4.contiguous()
    work = f4 if inplace else f4.clone()
    work_k = _pixel_rows(work, 2)
    lib = _hip.lib()
    ws_bytes = int(lib.fn2_variational_workspace_bytes(n, h, w))
    if ws_bytes < 0:
        raise ValueError("refine: bad size %s" % ((n, h, w),))
    with torch.cuda.device(work_k.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=work_k.device)
        _hip.check(lib.fn2_variational_refine(
            _hip.ptr(a4), _hip.ptr(b4), _row_pitch(a4, 3), a4.stride(0), _hip.ptr(work_k), _row_pitch(work_k, 2),
            work_k.stride(0), n, h, w, float(p["alpha"]), float(p["gamma"]), float(p["delta"]), float(p["sigma"]),
            p["niter_outer"], p["niter_inner"], p["niter_solver"], float(p["sor_omega"]), _hip.ptr(ws), ws_bytes,
            _hip.stream_ptr()))
    if work_k is not work:
        work.copy_(work_k)
    if inplace:
        return flow
    return work[0] if squeeze else work


def calc_variational_inference_map(imgA_filename, imgB_filename, flo_filename, out_filename, dataset):
    """utils.py:542-555: refine the flow in `flo_filename` (the init) between the RGB images A -> B and write it
    to `out_filename`.  `dataset` is accepted and ignored, exactly as the reference binary ignores it (see
    binary_params): the result is always that of the default parameters."""
    from .flowlib import read_flow, write_flow
    from .net import imread
    p = binary_params(dataset)
    dev = _hip.require_device()
    a = torch.from_numpy(np.ascontiguousarray(imread(imgA_filename))).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(imread(imgB_filename))).to(dev)
    init = torch.from_numpy(np.ascontiguousarray(read_flow(flo_filename), np.float32)).to(dev)
    out = refine(init, a, b, **p)
    write_flow(out.cpu().numpy(), out_filename)
