"""FlowNetS / FlowNetSD training step on one MI355X (+ data-parallel gradient all-reduce over RCCL; FlowNetSD:
``model="FlowNetSD"``, labels 20 * gt as flownet_sd.py:122, linear interconvN layers before the heads):
forward -> multiscale EPE loss -> backward -> Adam, all fp32 on the matrix cores.

Reference semantics (what tf.gradients + tf.train.AdamOptimizer compute for it):
  loss      FlowNetS.loss, src/flownet_s/flownet_s.py:122-161 -- labels = downsample(0.05*gt) per scale,
            average_endpoint_error (src/utils.py:209-224), compute_weighted_loss over the 5 scalars
            (weights .32 .08 .02 .01 .005, /5), + slim L2 regularisers (l2 = 4e-4 on slim.conv2d weights)
  optimiser Adam(lr from piecewise_constant LONG_SCHEDULE, beta 0.9/0.999, eps 1e-8), src/net.py:1205-1207,
            :1290-1295; src/training_schedules.py:46-53.  optimizer= 'sgd' | 'momentum' | 'adamw' and clip_grad_norm=
            select the other optimisers of net.py:1209-1288 and slim's per-tensor clipping; every kind, Adam included,
            is one fn2_optim_step_multi_dev launch for all parameter tensors
  DP        not in the reference (single GPU).  Here: one process per GPU, each rank runs the step on its
            shard, ONE all-reduce of the flat gradient buffer, identical Adam on every rank.

Parameters stay in the packed layouts the forward kernels read (Adam is elementwise, so the layout is
irrelevant to it); filter gradients are produced directly in those layouts; the transposed / phase-decomposed
copies that the input-gradient convolutions read are refreshed once per step by an index-map gather.
"""
import ctypes as C
import math
import os
import types

import numpy as np
import torch

from . import _hip, loss_stages, weights as W
from .engine import Engine, _round_up
from .training_schedules import LONG_SCHEDULE

LOSS_WEIGHTS = {6: 0.32, 5: 0.08, 4: 0.02, 3: 0.01, 2: 0.005}
F32 = _hip.FN2_F32


def _index_hwio(rec):
    """Flat position inside the layer's packed master weight of every element of its reference-layout
    weight (HWIO for conv, HW-O-I for deconv): pack an enumeration with the same packer and invert it.
    Cached on the layer record (checkpointing asks for it three times per layer: weight, m, v)."""
    if "_hwio_index" in rec:
        return rec["_hwio_index"]
    rec["_hwio_index"] = _index_hwio_uncached(rec)
    return rec["_hwio_index"]


def _index_hwio_uncached(rec):
    kind = rec["kind"]
    if kind == 1:
        shape = (4, 4, rec["cout"], rec["cin"])
        enum = np.arange(1, int(np.prod(shape)) + 1, dtype=np.float64).reshape(shape)
        pk = W.pack_deconv(enum, rec["tile"], rec["kstep"], rec["cin_pad"], rec["layout"], dtype=np.float64)[0]
    else:
        shape = (rec["k"], rec["k"], rec["cin"], rec["cout"])
        enum = np.arange(1, int(np.prod(shape)) + 1, dtype=np.float64).reshape(shape)
        if kind == 2:
            pk = W.pack_stem(enum, rec["cs"], rec["cin_pad"], rec["tile"], rec["layout"], dtype=np.float64)[0]
        else:
            pk = W.pack_conv(enum, rec["tile"], rec["kstep"], rec["cin_pad"], rec["layout"], dtype=np.float64)[0]
    flat = pk.reshape(-1)
    pos = np.nonzero(flat)[0]
    inv = np.empty(int(np.prod(shape)), np.int64)
    inv[flat[pos].astype(np.int64) - 1] = pos
    return inv.reshape(shape)


class FlowNetSTrainer:
    def __init__(self, weights, batch, height, width, schedule=LONG_SCHEDULE, eps=1e-8, dtype="f32", model="FlowNetS",
                 add_hard_flow_mining="", lambda_weight=2.0, hard_examples_perc=50, optimizer="adam", momentum=None,
                 min_momentum=0.85, max_momentum=0.95, weight_decay=None, clip_grad_norm=-1.0, unsupervised=False,
                 photometric_q=0.4, occ_alpha=0.01, occ_beta=0.5, smoothness_weight=0.0, smoothness_order=1,
                 edge_lambda=150.0, smoothness_eps=1e-3, sparse_gt=False, data_term="photometric"):
        """dtype 'f32': everything on the fp32 matrix cores.  'f16x2': activations, activation gradients and the
        weight copies the convolutions read are split fp16 (3 fp16 MFMAs per product, fp32 accumulate); the master
        weights, their gradients and the Adam state stay fp32.

        optimizer (Net.train, net.py:1209-1288): 'adam' (default), 'sgd', 'momentum' (Nesterov; a fixed `momentum`, or
        cyclical between min_momentum and max_momentum along a computed rate policy) or 'adamw' (decoupled
        `weight_decay`, default 1e-4).  For 'momentum' a given weight_decay replaces the schedule's l2_regularization;
        'sgd' and 'adam' ignore it.  clip_grad_norm > 0: every gradient tensor is clipped to that norm
        (slim's clip_gradient_norms); <= 0: off.

        unsupervised: no ground truth.  The batch holds batch / 2 pairs in both directions (slots 2k and 2k + 1) and the
        loss is the occlusion-aware photometric loss of src/photometric.py at the five scales, with the supervised loss's
        weights: psi = (|d| + 0.01)^photometric_q on the pixels that the forward-backward test (occ_alpha, occ_beta)
        leaves.  Steps go through train_step_unsupervised / forward_backward_unsupervised.

        smoothness_weight > 0 (unsupervised only): the edge-aware smoothness term of src/smoothness.py is added at the
        five scales, times that weight and the scale's loss weight -- first or second differences of the flow
        (smoothness_order) under sqrt(d^2 + smoothness_eps^2), weighted by exp(-edge_lambda * mean |frame difference|).
        0 (default): the step launches what it launches without the argument.

        sparse_gt: the ground truth does not cover the frame (KITTI, HD1K, Middlebury): a pixel whose u or v is not finite
        carries no label.  The labels stay the five NaN-aware downsamples; the loss behind them is src/sparse_epe.py's --
        every scale normalised by its own count of valid label pixels, gradient exactly 0 where there is none -- in two
        launches for all scales.  FlowNetS, FlowNetSD, FlowNetC and the last network of FlowNetCS / FlowNetCSS.  False
        (default): the step launches what it launches without the argument.

        data_term (unsupervised only): 'photometric' (default) is the loss above.  'census' replaces it by the ternary
        census term of src/census.py at every scale that holds a 7 x 7 patch -- the soft Hamming distance between the
        census descriptors of a frame's grey values and of its partner's warped ones, under the same robust function,
        exponent and occlusion masks; it needs no brightness constancy.  Smaller scales keep the photometric term."""
        from .census import check_data_term
        self.data_term = check_data_term(data_term, unsupervised)  # before anything else is built
        self.sparse_gt = bool(sparse_gt)
        if self.sparse_gt:  # before anything else is built
            if unsupervised:
                raise ValueError("sparse_gt is a supervised loss: not with unsupervised=True")
            if add_hard_flow_mining:
                raise ValueError("sparse_gt does not combine with hard-flow-example mining")
            if model in ("FlowNetS_interp", "FlowNet2"):
                raise ValueError("sparse_gt covers FlowNetS, FlowNetSD, FlowNetC, FlowNetCS and FlowNetCSS, not %s" % model)
        self._set_optimizer(optimizer, momentum, min_momentum, max_momentum, weight_decay, clip_grad_norm, schedule)
        if dtype not in ("f32", "f16x2"):
            raise ValueError("trainer dtype must be 'f32' or 'f16x2'")
        self.x2 = dtype == "f16x2"
        # loss scaling: activation gradients of this loss are 1e-4 .. 1e-7, under the fp16 normal range that the
        # split (hi + lo) format needs for its lo parts; 2^14 brings them to O(1).  Linear, so every parameter
        # gradient carries the same factor and Adam's grad_scale removes it exactly.
        self.loss_scale = 16384.0 if self.x2 else 1.0
        self.code = _hip.FN2_F16X2 if self.x2 else F32
        self.host_weights = weights
        # What the reference's Net.train optimises per model (net.py:1316-1323 builds self.model(..., trainable=True)):
        #   FlowNetS / SD / S_interp  the whole network;
        #   FlowNetCS / CSS           the LAST FlowNetS only -- the networks in front are built trainable=False
        #                             (flownet_cs.py:18, flownet_css.py:18) and feed it flow_warp / brightness-error
        #                             inputs, so no gradient passes through flow_warp;
        #   FlowNet2                  the fusion network only (flownet2.py:22-23: CSS and SD trainable=False), with the
        #                             single-scale loss of flownet2.py:107-116.
        #   FlowNetC                  the whole network: the towers share conv1-3 (reuse=True, flownet_c.py:34-37: one
        #                             variable, gradients of both towers summed) and the gradient passes through the
        #                             correlation (CorrelationGrad, correlation.py:17-35); fp32 only -- the op surface of
        #                             the correlation gradient is fp32 as the reference's.
        scopes = {"FlowNetS": "FlowNetS", "FlowNetSD": "FlowNetSD", "FlowNetS_interp": "FlowNetS", "FlowNetC": "FlowNetC",
                  "FlowNetCS": "FlowNetCS/FlowNetS", "FlowNetCSS": "FlowNetCSS/FlowNetS", "FlowNet2": "FlowNet2"}
        if model not in scopes:
            raise ValueError("the trainer covers FlowNetS, FlowNetSD, FlowNetS_interp, FlowNetC, the last network of "
                             "FlowNetCS / FlowNetCSS and the fusion network of FlowNet2")
        if model == "FlowNetC" and dtype != "f32":
            raise ValueError("FlowNetC trains in dtype 'f32' (the correlation gradient op is fp32)")
        self.model = model
        self.train_scope = scopes[model]
        # hard-flow-example mining of FlowNetS_interp.loss (flownet_s_interp.py:159-254, utils.py:227-339): '' plain
        # AEPE, 'hard' the top hard_examples_perc % EPE pixels of the batch weighted (1 + lambda), 'edges' every pixel
        # weighted 1 + lambda * edge map (given per batch)
        self.hfem = (add_hard_flow_mining or "").lower()
        if self.hfem not in ("", "hard", "edges"):
            raise ValueError("add_hard_flow_mining must be '', 'hard' or 'edges'")
        self.lambda_w, self.hard_perc = float(lambda_weight), float(hard_examples_perc)
        self.unsupervised = bool(unsupervised)
        from .smoothness import check_constants as check_smoothness
        (self.smoothness_order, self.edge_lambda, self.smoothness_eps,
         self.smoothness_weight) = check_smoothness(smoothness_order, edge_lambda, smoothness_eps, smoothness_weight)
        if self.smoothness_weight and not self.unsupervised:
            raise ValueError("smoothness_weight regularises the unsupervised loss: it needs unsupervised=True")
        if self.unsupervised:
            from .photometric import check_constants
            # the models with two image inputs and the five-scale loss (FlowNet2's loss is single-scale, FlowNetS_interp's
            # second input is no image)
            if model not in ("FlowNetS", "FlowNetSD", "FlowNetC", "FlowNetCS", "FlowNetCSS"):
                raise ValueError("unsupervised training covers FlowNetS, FlowNetSD, FlowNetC, FlowNetCS and FlowNetCSS, "
                                 "not %s" % model)
            if self.hfem:
                raise ValueError("hard-flow-example mining needs a ground truth: not with unsupervised=True")
            if batch % 2:
                raise ValueError("unsupervised training runs every pair in both directions: batch must be even, got %d"
                                 % batch)
            self.occ_alpha, self.occ_beta, self.photometric_q = check_constants(occ_alpha, occ_beta, photometric_q)
        # label scale of the loss: 0.05 * gt for FlowNetS (flownet_s.py:123), 20 * gt for FlowNetSD (flownet_sd.py:122)
        self.gt_scale = 20.0 if model == "FlowNetSD" else 0.05
        # {prediction name: loss weight}: the five scales of FlowNetS.loss through compute_weighted_loss (weights / 5,
        # flownet_s.py:122-161); FlowNet2.loss is the plain average_endpoint_error of predict_flow0 against the
        # UNSCALED ground truth (flownet2.py:107-116)
        self.loss_terms = {"predict_flow%d" % lvl: wgt / 5.0 for lvl, wgt in LOSS_WEIGHTS.items()}
        if model == "FlowNet2":
            self.loss_terms, self.gt_scale = {"predict_flow0": 1.0}, 1.0
            if self.hfem:
                raise ValueError("hard-flow-example mining belongs to FlowNetS_interp")
        # FN2_TRAIN_WREG=1: the split-fp16 COPIES the convolutions read are kept in MFMA-fragment order where the library
        # has the register-operand kernel (masters, gradients and Adam state stay row-major).  Off by default: the
        # convolutions gain 0.09 ms per step (batch 8) but the per-step refresh of those copies -- Adam's 8-byte pieces and
        # the gathers' 16-byte chunks scattered over the fragment blocks -- costs 0.25 ms: 4.76 -> 4.92 ms.
        self.eng = Engine(model, weights, batch, height, width, dtype, heads_as_gemm=False, plain_stems=True,
                          fragment_weights=self.x2 and bool(int(os.environ.get("FN2_TRAIN_WREG", "0"))))
        self.lib, self.dev = self.eng.lib, self.eng.device
        self.N, self.H, self.W = batch, height, width
        self.schedule, self.eps = schedule, eps
        self.step_count = 0
        self.keep = []
        self.gt = torch.zeros((batch, height, width, 2), dtype=torch.float32, device=self.dev)
        self.loss_dev = torch.zeros(1, dtype=torch.float32, device=self.dev)
        # the loss stages built so far by "with an edge map" ('edges' mode only), the latest step's, the captured step's
        self._stages, self._stage, self._captured = {}, None, None
        self._build()

    # ------------------------------------------------------------------ construction
    def _set_optimizer(self, optimizer, momentum, min_momentum, max_momentum, weight_decay, clip_grad_norm, schedule):
        """Validate and record the optimiser arguments (host only: runs before the engine is built)."""
        from .training_schedules import momentum_value
        kind = "adam" if optimizer is None else str(optimizer).lower()
        if kind not in _hip.OPTIM_KINDS:
            raise ValueError("optimizer must be one of 'adam', 'sgd', 'momentum', 'adamw', not %r" % (optimizer,))
        for name, val in (("momentum", momentum), ("min_momentum", min_momentum), ("max_momentum", max_momentum)):
            if val is not None and not 0.0 <= float(val) < 1.0:
                raise ValueError("%s must lie in [0, 1), not %r" % (name, val))
        if weight_decay is not None and not float(weight_decay) >= 0.0:
            raise ValueError("weight_decay must be >= 0, not %r" % (weight_decay,))
        clip = float(clip_grad_norm)
        if clip != clip or clip == float("inf"):
            raise ValueError("clip_grad_norm must be finite (<= 0 disables clipping), not %r" % (clip_grad_norm,))
        self.optimizer = kind
        self.momentum = None if momentum is None else float(momentum)
        self.min_momentum, self.max_momentum = min_momentum, max_momentum
        self.clip_norm = clip if clip > 0.0 else 0.0
        if kind == "momentum":
            if momentum is None and (min_momentum is None or max_momentum is None):
                raise ValueError("the momentum optimizer needs --momentum, or --min_momentum and --max_momentum")
            momentum_value(schedule, 0, None, momentum, min_momentum, max_momentum)  # cyclical on a piecewise schedule raises
        # decoupled decay of adamw (net.py:1267-1270); for momentum a given weight_decay IS the L2 coefficient (net.py:1221-1222)
        self.weight_decay = (1e-4 if weight_decay is None else float(weight_decay)) if kind == "adamw" else 0.0
        self.l2_reg = float(weight_decay) if kind == "momentum" and weight_decay is not None else schedule["l2_regularization"]
        # slots per parameter: Adam's m and v, momentum's accumulator, none for sgd
        self.n_slots = {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 2}[kind]

    def _gbuf(self, buf):
        """Gradient buffer mirroring an activation buffer (fp32, same shape)."""
        key = buf.untyped_storage().data_ptr()
        if key not in self.gbufs:
            base = self.base_of[key]
            self.gbufs[key] = torch.zeros_like(base)
        g = self.gbufs[key]
        self.gcode[g.data_ptr()] = self.eng._code(buf)
        if buf.shape[0] != g.shape[0]:  # batch slice of a 2N buffer (FlowNetC's towers): the same rows of the mirror
            base = self.base_of[key]
            row = base.stride(0) * base.element_size()
            n0 = (buf.data_ptr() - base.data_ptr()) // row
            g = g[n0:n0 + buf.shape[0]]
            self.gcode[g.data_ptr()] = self.eng._code(buf)
        return g

    def _view(self, buf, c, c0):
        """View of an activation / gradient buffer (fp32 buffers -- flow heads -- stay fp32 in every mode)."""
        code = self.gcode.get(buf.data_ptr())
        return _hip.view(buf, c, c0, code if code is not None else self.eng._code(buf))

    def _master(self, rec):
        """fp32 master of a layer's packed weight.  fp32 trainer: the tensor the forward reads.  f16x2 trainer: a
        separate fp32 tensor in the same packed geometry (the forward reads a split-fp16 copy, refreshed per step)."""
        if not self.x2 or rec["kind"] == "upflow" or rec["w"].dtype == torch.float32 and rec.get("cout") == 2:
            return rec["w"]
        name = f"{rec['scope']}/{rec['name']}/weights"
        w = np.asarray(self.host_weights[name], np.float32)
        if rec["kind"] == 1:
            pk = W.pack_deconv(w, rec["tile"], rec["kstep"], rec["cin_pad"], rec["layout"])[0]
        elif rec["kind"] == 2:
            pk = W.pack_stem(w, rec["cs"], rec["cin_pad"], rec["tile"], rec["layout"])[0]
        else:
            pk = W.pack_conv(w, rec["tile"], rec["kstep"], rec["cin_pad"], rec["layout"])[0]
        return torch.from_numpy(np.ascontiguousarray(pk, np.float32)).to(self.dev)

    def _build(self):
        eng = self.eng
        self.base_of = {b.untyped_storage().data_ptr(): b for b in eng.bufs.values()}
        self.gbufs = {}
        self.gcode = {}  # gradient buffer -> fn2_dtype of the activation buffer it mirrors
        # trainable layers: those of the trained scope, in forward order (everything in front of them is frozen)
        layers = self.layers = [rec for rec in eng.layers if rec["scope"] == self.train_scope]
        for rec in layers:
            # a bias the checkpoint does not define (FlowNetS_interp's heads, flownet_s_interp.py:86-95) is the engine's
            # constant zero vector, not a variable: no gradient, no Adam state, not saved
            if rec.get("b") is not None and f"{rec['scope']}/{rec['name']}/biases" not in self.host_weights:
                rec["b"] = None
        # ---- parameters and one flat gradient / moment arena (single all-reduce, single memset)
        params = []  # (tensor, l2 flag)
        self.fwd_copies = []  # f16x2 trainer: (split-fp16 forward weight, fp32 master, scale)
        first_of = {}
        for rec in layers:
            if rec["kind"] == "corr":
                continue
            key = f"{rec['scope']}/{rec['name']}"
            if key in first_of:
                # a second launch of the same variable (FlowNetC's second tower, reuse=True): one parameter; the
                # forward of this launch reads the first launch's tensors, its gradients add into the same slices
                first = first_of[key]
                rec["shared_with"] = first
                rec["master"] = first["master"]
                rec["w"], rec["desc"].wgt = first["w"], first["w"].data_ptr()
                if first.get("b") is not None:
                    rec["b"], rec["desc"].bias = first["b"], first["b"].data_ptr()
                continue
            first_of[key] = rec
            reg = rec["kind"] in (0, 2)  # slim.conv2d weights (heads included); deconv / upsample / biases are not
            rec["master"] = self._master(rec)
            if rec["master"] is not rec["w"]:
                rec["scale"] = 1.0 / float(rec["desc"].out_scale)
                self.fwd_copies.append((rec["w"], rec["master"], rec["scale"], rec["kpad"] if rec.get("frag") else 0))
            params.append((rec["master"], reg, rec))
            if rec.get("b") is not None:
                params.append((rec["b"], False, None))
        total = sum(_round_up(t.numel(), 4) for t, _, _ in params)
        self.grad_arena = torch.zeros(total, dtype=torch.float32, device=self.dev)
        self.m_arena = torch.zeros_like(self.grad_arena) if self.n_slots >= 1 else None   # Adam's m / the momentum accumulator
        self.v_arena = torch.zeros_like(self.grad_arena) if self.n_slots >= 2 else None
        self.params = []
        off = 0
        last = None
        for t, reg, rec in params:
            n = t.numel()
            g = self.grad_arena[off:off + n]
            # rec is None for a bias: it follows its layer's weight in `params`
            name = f"{rec['scope']}/{rec['name']}/weights" if rec is not None else f"{last['scope']}/{last['name']}/biases"
            last = rec if rec is not None else last
            self.params.append(dict(w=t, g=g, m=self.m_arena[off:off + n] if self.n_slots >= 1 else None,
                                    v=self.v_arena[off:off + n] if self.n_slots >= 2 else None, reg=reg, n=n,
                                    name=name, rec=rec))
            if rec is not None:
                rec["dw"] = g
            off += _round_up(n, 4)
        # map bias tensors to their grads
        bias_grad = {p["w"].data_ptr(): p["g"] for p in self.params}
        for rec in layers:
            if rec.get("shared_with") is not None:
                rec["dw"] = rec["shared_with"]["dw"]
            if rec.get("b") is not None:
                rec["db"] = bias_grad[rec["b"].data_ptr()]

        # ---- per-layer backward launches, in reverse forward order
        self.bwd_ops = []
        self.gathers = []
        self._act_ops = []
        order = list(reversed(layers))
        for i in range(len(order) - 1):
            # a flow head and the transposed conv of the next level read the same tensor (predict_flowN and deconvN-1 on
            # concatN / conv6_1); both add into its gradient.  The head goes first, so that the LAST writer of that
            # gradient is a convolution, whose epilogue can apply the LeakyReLU factor (_fuse_act_grads)
            a, b = order[i], order[i + 1]
            if a["kind"] == 1 and b["kind"] == 0 and b.get("cout") == 2 and a["src"][0].data_ptr() == b["src"][0].data_ptr():
                order[i], order[i + 1] = b, a
        self.bwd_recs = order  # bwd_ops[i] is the backward of bwd_recs[i]
        for rec in order:
            if rec["kind"] == "corr":
                self._plan_corr(rec)
            elif rec["kind"] == "upflow":
                self._plan_upflow(rec)
            elif rec["cout"] == 2:
                self._plan_head(rec)
            else:
                self._plan_conv(rec)
        if self.x2 and os.environ.get("FN2_HEAD_MFMA", "1") != "0":
            for rec in layers:
                if rec["kind"] == 0 and rec.get("cout") == 2 and rec.get("shared_with") is None:
                    self._head_forward_gemm(rec)
        self._fuse_act_grads()
        self._plan_zeroing()
        eng._alloc_workspace()  # the input-gradient convolutions share the split-K scratch buffer
        self.refresh_backward_weights()
        self._plan_buckets(4)
        self._build_optim_tables()

    def _head_forward_gemm(self, rec):
        """Forward of a flow head in the split-fp16 trainer as the engine's inference form (Engine._head_gemm): a 1x1
        convolution to the 18 (tap, output) partials of a pixel + fn2_flow_head_gather, instead of the wave-per-pixel
        dot-product kernel.  Its packed weight is one more copy derived from the fp32 master every step."""
        eng, lib = self.eng, self.lib
        sbuf, sc0, sc = rec["src"]
        pf = rec["dst"][0]
        code = eng._code(sbuf)
        line, whole = eng._cin_run(code, sbuf, sc0, sc, 18)
        if not whole:
            return False
        plan = _hip.conv_plan(code, line, 18)
        idx = np.zeros((1, 1, sc, 18), np.float64)
        for tap in range(9):
            for o in range(2):
                idx[0, 0, :, tap * 2 + o] = o * rec["kpad"] + tap * rec["cin_pad"] + np.arange(sc)
        pk, cin_pad, cout_pad, kpad = W.pack_conv(idx + 1.0, plan.cout_tile, plan.kstep_elems, line, plan.layout, dtype=np.float64)
        gmap = torch.from_numpy((pk.reshape(-1) - 1.0).astype(np.int32)).to(self.dev)
        wf = torch.zeros(gmap.numel(), dtype=torch.float32, device=self.dev)  # split fp16 in an fp32 container
        out_scale = W.scale_f16x2(rec["master"].detach().cpu().numpy())[1]   # (the gather applies 1 / out_scale every step)
        self.gathers.append([wf, rec["master"], gmap, 1.0 / out_scale, 0])
        n, h, w = int(pf.shape[0]), int(pf.shape[1]), int(pf.shape[2])
        t18 = torch.zeros((n * h * w, 32), dtype=torch.float32, device=self.dev)
        d = eng._conv_desc(self._view(sbuf, sc, sc0), _hip.Fn2Tensor(t18.data_ptr(), _hip.FN2_F32, n, h, w, 18, 32, 0),
                           types.SimpleNamespace(w=wf, cin_pad=cin_pad, cout_pad=cout_pad, kpad=kpad, layout=plan.layout,
                                                 out_scale=out_scale), lane=0)
        bias = _hip.ptr(rec["b"]) if rec.get("b") is not None else None
        self.keep += [d, wf, gmap, t18]

        def head_forward(s):
            return lib.fn2_conv2d(C.byref(d), s) or lib.fn2_flow_head_gather(_hip.ptr(t18), 32, bias, _hip.ptr(pf), n, h, w, s)

        name = f"{rec['scope']}/{rec['name']}"
        for i, (nm, fn, args) in enumerate(eng.ops):
            if nm == name and fn is lib.fn2_conv2d and args[0]._obj is rec["desc"]:
                eng.ops[i] = (nm, head_forward, ())
                eng.kernel_of[i] = "conv_igemm2_kernel (1x1, 18 partials) + flow_head_gather"
                return True
        raise RuntimeError("flow head %s not found in the engine's plan" % name)

    def _writes(self, fn, args):
        """[(first byte, end byte, c0, c)] of the activation-gradient buffers a backward launch adds into (4-byte
        elements in every gradient buffer)."""
        span = lambda v: (v.data, v.data + 4 * v.n * v.h * v.w * v.cs, v.c0, v.c)
        if fn is self.lib.fn2_conv2d:
            return [span(args[0]._obj.out)]
        if fn is self.lib.fn2_head_bwd_data:
            return [span(args[2]._obj)]
        return list(getattr(fn, "writes", []))

    def _plan_zeroing(self):
        """Gradient buffers that need no memset per step: when the FIRST launch that adds into a buffer is an
        input-gradient convolution over all the channels anyone adds into, that launch stores instead of adding
        (fn2_conv_desc.accumulate = 0: no zero fill, no read of the old contents).  The pad channels past the real ones
        are never written and stay zero from the allocation.  FN2_SKIP_ZERO=0: zero everything (A/B)."""
        self._no_zero = set()  # data pointers of the buffers whose first writer stores
        if os.environ.get("FN2_SKIP_ZERO", "1") == "0":
            return
        for g in self.gbufs.values():
            g0, g1 = g.data_ptr(), g.data_ptr() + 4 * g.numel()
            ws = [(fn, args, w) for _name, ops in self.bwd_ops for fn, args in ops for w in self._writes(fn, args)
                  if w[0] < g1 and g0 < w[1]]
            if ws and ws[0][0] is self.lib.fn2_conv2d:
                d = ws[0][1][0]._obj
                o = d.out
                top = max(w[2] + w[3] for _fn, _args, w in ws)
                if d.accumulate and o.data == g0 and (o.n, o.h, o.w, o.cs) == tuple(g.shape) and o.c0 == 0 and o.c >= top:
                    d.accumulate = 0
                    self._no_zero.add(g0)

    def _fuse_act_grads(self):
        """LeakyReLU backward without its own pass over the tensor: when the last launch that adds into a layer's output
        gradient is an input-gradient convolution (the next encoder layer's, the next level's transposed conv or
        interconv), that launch multiplies the finished sums by the LeakyReLU factor in its epilogue
        (fn2_conv_desc.act_grad_y) and the layer keeps only the bias-gradient reduction.  Everything else -- a slice
        completed by a flow head's input gradient, ranges off the 16-channel grid of the epilogue, FN2_FUSE_ACT_GRAD=0
        -- stays on fn2_leaky_bwd."""
        self.fused_act = []
        if os.environ.get("FN2_FUSE_ACT_GRAD", "1") == "0":
            return
        lib, writes = self.lib, self._writes
        for act in self._act_ops:
            bi = act["block"]  # (names repeat: FlowNetC runs conv2 / conv3 once per tower)
            vg, vy = act["vg"], act["vy"]
            lo, hi = vg.c0, vg.c0 + vg.c
            g0, g1 = vg.data, vg.data + 4 * vg.n * vg.h * vg.w * vg.cs
            last = None
            for bj in range(bi - 1, -1, -1):
                for fn, args in reversed(self.bwd_ops[bj][1]):
                    if any(b0 < g1 and g0 < b1 and c0 < hi and lo < c0 + c for b0, b1, c0, c in writes(fn, args)):
                        last = (fn, args)
                        break
                if last is not None:
                    break
            if last is None or last[0] is not lib.fn2_conv2d:
                continue
            d = last[1][0]._obj
            o = d.out
            rel0, rel1 = lo - o.c0, hi - o.c0
            if d.act_grad_y or rel0 < 0 or rel1 > o.c or rel0 % 16 or (rel1 % 16 and rel1 != o.c) or o.dtype != vy.dtype:
                continue
            if (o.data, o.n, o.h, o.w, o.cs) != (vg.data, vg.n, vg.h, vg.w, vg.cs):
                continue  # the writer covers a batch slice only (FlowNetC's conv1 runs both towers as one 2N batch)
            d.act_grad_y, d.act_grad_c0, d.act_grad_c1 = vy.data, rel0, rel1
            ops = self.bwd_ops[bi][1]
            assert ops[0][0] is lib.fn2_leaky_bwd
            if act["db"] is not None:
                ops[0] = (lib.fn2_bias_grad, (C.byref(vg), act["db"]))
            else:
                del ops[0]
            self.fused_act.append(act["name"])

    def _plan_buckets(self, n_buckets):
        """Gradient exchange overlapped with backward: the arena is laid out in FORWARD layer order and backward
        completes it from the tail, so a bucket is a contiguous tail slice; it is reduced as soon as the backward
        of its first (earliest-forward) layer has been enqueued.  ~40 MB buckets keep the xGMI ring
        bandwidth-bound.  self.buckets[i] = (index into bwd_ops after which it is complete, arena slice)."""
        offs, off = {}, 0
        for rec in self.layers:
            lo = off
            if rec["kind"] != "corr" and rec.get("shared_with") is None:  # (those own no slice of the arena)
                off += _round_up(rec["master"].numel(), 4)
                if rec.get("b") is not None:
                    off += _round_up(rec["b"].numel(), 4)
            offs[id(rec)] = (lo, off)  # (by layer, not by name: FlowNetC launches conv2 / conv3 once per tower)
        total, target = off, off / float(n_buckets)
        # (backward runs the layers in reverse forward order except that a flow head goes in front of the transposed
        # conv that follows it in the forward pass: a tail is complete once the launches so far cover exactly it)
        self.buckets, hi, done, tail = [], total, 0, total
        assert len(self.bwd_recs) == len(self.bwd_ops)
        for i, rec in enumerate(self.bwd_recs):
            lo, up = offs[id(rec)]
            done, tail = done + up - lo, min(tail, lo)
            last = i == len(self.bwd_ops) - 1
            if total - tail == done and (hi - tail >= target or last):
                self.buckets.append((i, self.grad_arena[tail:hi]))
                hi = tail
        assert hi == 0 and sum(b.numel() for _, b in self.buckets) == total

    def _bwd_data_conv(self, rec, hwio_index, kind, k, stride, pad, g_src, g_dst):
        """fn2_conv2d launch computing the input gradient: in = gradient of the layer output slice,
        out = gradient of the layer input slice (accumulated)."""
        gy_buf, gy_c0, gy_c = g_src
        gx_buf, gx_c0, gx_c = g_dst
        cin_b, cout_b = gy_c, gx_c
        cin_pad = self.eng._cin_run(self.code, gy_buf, gy_c0, cin_b, cout_b)[0]
        plan = _hip.conv_plan(self.code, cin_pad, cout_b)
        enum = hwio_index.astype(np.float64) + 1.0
        if kind == 3:
            pk, cin_pad, cout_pad, kpad = W.pack_conv_transpose_s2(enum, pad, plan.cout_tile, plan.kstep_elems, cin_pad,
                                                                   plan.layout, dtype=np.float64)
        else:
            pk, cin_pad, cout_pad, kpad = W.pack_conv(enum, plan.cout_tile, plan.kstep_elems, cin_pad, plan.layout,
                                                      dtype=np.float64)
        gmap = torch.from_numpy((pk.reshape(-1) - 1.0).astype(np.int32)).to(self.dev)
        wb = torch.zeros(gmap.numel(), dtype=torch.float32, device=self.dev)  # fp32, or split fp16 in an fp32 container
        scale = rec.get("scale", 1.0)
        gather = [wb, rec["master"], gmap, scale, 0]   # (last: packed row length when the copy is in fragment order)
        self.gathers.append(gather)
        # (registered on lane 0 with the engine's descriptors: shares the split-K workspace)
        d = self.eng._conv_desc(self._view(gy_buf, gy_c, gy_c0), self._view(gx_buf, gx_c, gx_c0),
                                types.SimpleNamespace(w=wb, cin_pad=cin_pad, cout_pad=cout_pad, kpad=kpad, layout=plan.layout,
                                                      out_scale=1.0 / scale),
                                kind, k, stride, pad, accumulate=True, lane=0)
        if self.eng.fragment_weights and plan.layout == 1 and plan.cout_tile == 128 and self.eng._wants_fragments(d):
            d.wgt_layout, gather[4] = 2, kpad   # the gather writes this copy in MFMA-fragment order
        self.keep += [d, wb, gmap]
        return d

    def _plan_conv(self, rec):
        sbuf, sc0, sc = rec["src"]
        dbuf, dc0, dc = rec["dst"]
        gy = self._gbuf(dbuf)
        ops = []
        vy, vg = self._view(dbuf, dc, dc0), self._view(gy, dc, dc0)
        self.keep += [vy, vg]
        db = _hip.ptr(rec["db"]) if rec.get("b") is not None else None
        # a convolution's bias gradient (the pixel sum of dy) comes out of its filter-gradient launch, which reads dy
        # anyway; a transposed conv's filter gradient walks x, so its bias (the fusion net's) keeps its own reduction
        db_fused, db = (db, None) if rec["kind"] != 1 else (None, db)
        if rec["act"]:
            ops.append((self.lib.fn2_leaky_bwd, (C.byref(vy), C.byref(vg), db)))  # (+ bias gradient, same pass)
            self._act_ops.append(dict(name=f"{rec['scope']}/{rec['name']}", block=len(self.bwd_ops), vy=vy, vg=vg, db=db))
        elif db is not None:
            ops.append((self.lib.fn2_bias_grad, (C.byref(vg), db)))
        bd = _hip.Fn2BwdwDesc()
        bd.x = self._view(sbuf, sc, sc0)
        bd.dy = vg
        bd.dw = rec["dw"].data_ptr()
        bd.kind, bd.kh, bd.kw, bd.stride, bd.pad = rec["kind"], rec["k"], rec["k"], rec["stride"], \
            (0 if rec["kind"] == 2 else rec["pad"])
        bd.cin_pad, bd.cout_pad, bd.kpad, bd.wgt_layout = rec["cin_pad"], rec["cout_pad"], rec["kpad"], rec["layout"]
        bd.db = db_fused
        self.keep.append(bd)
        ops.append((self.lib.fn2_conv2d_bwd_filter, (C.byref(bd),)))
        if rec["kind"] != 2:  # the stem's input is the image pair: no gradient needed
            gx = self._gbuf(sbuf)
            idx = _index_hwio(rec)
            k, p = rec["k"], rec["pad"]
            if rec["kind"] == 1:
                # transposed conv forward -> plain conv k4 s2 p1 backward, HWIO' = Wt[ky,kx,co,ci]
                d = self._bwd_data_conv(rec, idx, 0, 4, 2, 1, (gy, dc0, dc), (gx, sc0, sc))
            elif rec["stride"] == 1:
                rot = np.ascontiguousarray(idx[::-1, ::-1].transpose(0, 1, 3, 2))  # flip taps, swap ci/co
                d = self._bwd_data_conv(rec, rot, 0, k, 1, k - 1 - p, (gy, dc0, dc), (gx, sc0, sc))
            else:
                d = self._bwd_data_conv(rec, idx, 3, k, 2, p, (gy, dc0, dc), (gx, sc0, sc))
            ops.append((self.lib.fn2_conv2d, (C.byref(d),)))
        self.bwd_ops.append((f"{rec['scope']}/{rec['name']}", ops))

    def _plan_head(self, rec):
        sbuf, sc0, sc = rec["src"]
        pf = rec["dst"][0]
        dpf = self._gbuf(pf)
        gx = self._gbuf(sbuf)
        vx, vg = self._view(sbuf, sc, sc0), self._view(dpf, 2, 0)
        self.keep += [vx, vg]
        if self.x2 and os.environ.get("FN2_HEAD_MFMA", "1") != "0":
            # split-fp16 trainer: the head's output gradient as the 18-channel tensor G18 (fn2_head_g18), then both
            # gradients are matrix products on the kernels of the other layers -- the filter gradient a 1x1 launch of
            # the filter-gradient kernel (kind 4), the input gradient a 1x1 accumulating convolution from G18
            n, h, w = int(pf.shape[0]), int(pf.shape[1]), int(pf.shape[2])
            g18 = torch.zeros((n, h, w, 32), dtype=torch.float32, device=self.dev)  # split fp16 in an fp32 container
            self.gcode[g18.data_ptr()] = _hip.FN2_F16X2
            v18 = self._view(g18, 18, 0)
            self.keep += [g18, v18]
            ops = [(self.lib.fn2_head_g18, (_hip.ptr(dpf), C.byref(v18)))]
            bd = _hip.Fn2BwdwDesc()
            bd.x, bd.dy, bd.dw = vx, v18, rec["dw"].data_ptr()
            bd.kind, bd.kh, bd.kw, bd.stride, bd.pad = 4, 3, 3, 1, 1
            bd.cin_pad, bd.cout_pad, bd.kpad, bd.wgt_layout = rec["cin_pad"], 32, rec["kpad"], 0
            self.keep.append(bd)
            ops.append((self.lib.fn2_conv2d_bwd_filter, (C.byref(bd),)))
            if rec.get("b") is not None:
                ops.append((self.lib.fn2_bias_grad, (C.byref(vg), _hip.ptr(rec["db"]))))
            # W18[c18 = tap * 2 + o][ci] = w[o][tap * cin_pad + ci] of the natural-order master, as a 1x1 HWIO index
            idx = np.zeros((1, 1, 18, sc), np.int64)
            for tap in range(9):
                for o in range(2):
                    idx[0, 0, tap * 2 + o, :] = o * rec["kpad"] + tap * rec["cin_pad"] + np.arange(sc)
            d = self._bwd_data_conv(rec, idx, 0, 1, 1, 0, (g18, 0, 18), (gx, sc0, sc))
            ops.append((self.lib.fn2_conv2d, (C.byref(d),)))
            self.bwd_ops.append((f"{rec['scope']}/{rec['name']}", ops))
            return
        ops = [(self.lib.fn2_head_bwd_filter, (C.byref(vx), _hip.ptr(dpf), _hip.ptr(rec["dw"]), rec["cin_pad"], rec["kpad"]))]
        if rec.get("b") is not None:  # FlowNetS_interp's heads carry no biases (no_deconv_biases, flownet_s_interp.py:86-95)
            ops.append((self.lib.fn2_bias_grad, (C.byref(vg), _hip.ptr(rec["db"]))))
        vdx = self._view(gx, sc, sc0)
        self.keep.append(vdx)
        ops.append((self.lib.fn2_head_bwd_data, (_hip.ptr(dpf), _hip.ptr(rec["master"]), C.byref(vdx), rec["cin_pad"], rec["kpad"])))
        self.bwd_ops.append((f"{rec['scope']}/{rec['name']}", ops))

    def _plan_corr(self, rec):
        """Backward of correlation + LeakyReLU (flownet_c.py:40-41): the LeakyReLU factor on the 441-channel slice of the
        concat gradient, then CorrelationGrad (fn2_correlation_grad_f32, dense fp32 operands as the reference's op) into
        scratch, added to the gradients of both towers' conv3 outputs (conv_redir adds its own share to tower a)."""
        net, c0, c = rec["dst"]
        a, b = rec["fa"], rec["fb"]
        gnet, ga, gb = self._gbuf(net), self._gbuf(a), self._gbuf(b)
        n, h, w, ch = a.shape
        cpad = (net.shape[3] - c0) // 4 * 4  # the slice widened to the buffer's zero pad channels: 4-aligned for the pass
        vy, vg = self._view(net, cpad, c0), self._view(gnet, cpad, c0)
        gd = torch.empty((n, h, w, c), dtype=torch.float32, device=self.dev)
        da, db = torch.empty_like(a), torch.empty_like(b)
        self.keep += [vy, vg, gd, da, db]

        vslice = _hip.view(gnet, c, c0, F32)
        self.keep.append(vslice)

        def copy_grad(s):
            return self.lib.fn2_slice_copy_f32(C.byref(vslice), _hip.ptr(gd), s)

        def add_grads(s):
            return (self.lib.fn2_add_f32(_hip.ptr(ga), _hip.ptr(da), ga.numel(), s)
                    or self.lib.fn2_add_f32(_hip.ptr(gb), _hip.ptr(db), gb.numel(), s))
        add_grads.writes = [(t.data_ptr(), t.data_ptr() + 4 * t.numel(), 0, t.shape[3]) for t in (ga, gb)]

        ops = [(self.lib.fn2_leaky_bwd, (C.byref(vy), C.byref(vg), None)),
               (copy_grad, ()),
               (self.lib.fn2_correlation_grad_f32, (_hip.ptr(gd), _hip.ptr(a), _hip.ptr(b), _hip.ptr(da), _hip.ptr(db),
                                                    n, h, w, ch, 1, 20, 1, 2, 20)),
               (add_grads, ())]
        self.bwd_ops.append((f"{rec['scope']}/{rec['name']}", ops))

    def _plan_upflow(self, rec):
        pf = rec["src"]
        dbuf, dc0, dc = rec["dst"]
        vg = self._view(self._gbuf(dbuf), 2, dc0)
        self.keep.append(vg)
        ops = [(self.lib.fn2_upsample_flow_bwd, (C.byref(vg), _hip.ptr(pf), _hip.ptr(rec["w"]), _hip.ptr(self._gbuf(pf)),
                                                 _hip.ptr(rec["dw"]), 1))]
        if rec.get("b") is not None:  # the fusion net's fuse_upsample_flow2to1 / 1to0 carry a bias (flownet2.py:70-73, :86-89)
            ops.append((self.lib.fn2_bias_grad, (C.byref(vg), _hip.ptr(rec["db"]))))
        self.bwd_ops.append((f"{rec['scope']}/{rec['name']}", ops))

    def backward_launches(self):
        """[(name, fn, args, device kernel, algorithmic flop)] of one backward pass, for per-launch timing."""
        flops = dict(self.eng.layer_flops)
        out = []
        for name, ops in self.bwd_ops:
            for fn, args in ops:
                fl, kern = 0.0, fn.__name__.replace("fn2_", "") + "_kernel"
                if fn is self.lib.fn2_conv2d:
                    fl, kern = flops.get(name, 0.0), self.eng.kernel_name(fn, args)   # (tile, ring, fragment order, split)
                elif fn is self.lib.fn2_conv2d_bwd_filter:
                    fl, kern = flops.get(name, 0.0), ("bwd_filter_x2_kernel" if self.x2 else "bwd_filter_kernel")
                out.append(("bwd " + name, fn, args, kern, fl))
        return out

    # ------------------------------------------------------------------ step
    def refresh_backward_weights(self, forward=True):
        """Derive every weight copy the convolutions read from the fp32 masters: the transposed / phase-decomposed
        layouts of the input-gradient convolutions and, in the f16x2 trainer, the split-fp16 forward weights."""
        s = _hip.stream_ptr()
        for wb, wsrc, gmap, scale, frag_k in self.gathers:
            if self.x2 and frag_k:
                _hip.check(self.lib.fn2_to_f16x2_frag(_hip.ptr(wb), _hip.ptr(wsrc), _hip.ptr(gmap), wb.numel(), scale, frag_k, s))
            elif self.x2:
                _hip.check(self.lib.fn2_to_f16x2(_hip.ptr(wb), _hip.ptr(wsrc), _hip.ptr(gmap), wb.numel(), scale, s))
            else:
                _hip.check(self.lib.fn2_gather_f32(_hip.ptr(wb), _hip.ptr(wsrc), _hip.ptr(gmap), wb.numel(), s))
        if forward:  # (after an optimiser step the forward copies are fresh: fn2_optim_step_multi_dev writes them)
            for wx2, master, scale, frag_k in self.fwd_copies:
                if frag_k:
                    _hip.check(self.lib.fn2_to_f16x2_frag(_hip.ptr(wx2), _hip.ptr(master), None, master.numel(), scale, frag_k, s))
                else:
                    _hip.check(self.lib.fn2_to_f16x2(_hip.ptr(wx2), _hip.ptr(master), None, master.numel(), scale, s))

    def learning_rate(self, step):
        """Piecewise-constant schedules and the computed policies (CLR, one-cycle, exponential, LR range test):
        src/training_schedules.py; policy parameters in self.train_params (clr_min_lr, clr_max_lr, clr_stepsize, ...)."""
        from .training_schedules import learning_rate
        return learning_rate(self.schedule, step, getattr(self, "train_params", None))

    def _f32(self, x):
        """A tensor or array as a fp32 device tensor."""
        return (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(device=self.dev, dtype=torch.float32)

    def _pack_interp(self, input_a, matches_a, sparse_flow):
        """FlowNetS_interp: the tower's second 'image' is [0.05 * sparse_flow | matches] (flownet_s_interp.py:34-38)."""
        m = self._f32(matches_a)
        if m.ndim == 3:
            m = m[..., None]
        return self._f32(input_a), torch.cat([self._f32(sparse_flow) * 0.05, m], dim=3)

    def forward_backward_interp(self, input_a, matches_a, sparse_flow, gt_flow, edges=None, reduce=False):
        """forward_backward on the packed inputs of FlowNetS_interp (_pack_interp)."""
        a, b = self._pack_interp(input_a, matches_a, sparse_flow)
        return self.forward_backward(a, b, gt_flow, reduce=reduce, edges=edges)

    def train_step_interp(self, input_a, matches_a, sparse_flow, gt_flow, edges=None):
        """train_step on the packed inputs of FlowNetS_interp; the packing happens outside the captured graph."""
        a, b = self._pack_interp(input_a, matches_a, sparse_flow)
        return self.train_step(a, b, gt_flow, edges=edges)

    # the loss state by the names its readers know: that kind's stage or None, the latest labels, the captured mode
    _photo = property(lambda self: next((st for st in self._stages.values() if st.kind == "photometric"), None))
    _census = property(lambda self: next((st for st in self._stages.values() if st.kind == "census"), None))
    _sparse = property(lambda self: next((st for st in self._stages.values() if st.kind == "sparse"), None))
    _labels = property(lambda self: self._stage.labels)
    _mining = property(lambda self: self._captured.kind if self._captured.kind in ("hard", "edges") else None)

    def _pick_stage(self, edges, captured=False):
        """The loss stage (src/loss_stages.py) of this call, built on first use and allocated: before the zeroing and before
        any capture.  'edges' without an edge map is plain AEPE; the captured step stays with its first call's choice."""
        with_map = self.hfem == "edges" and edges is not None
        if captured and self._captured is not None and self._captured is not self._stages.get(with_map):
            raise ValueError("train_step: the captured step was built %s an edge map; this call is %s one"
                             % (("without", "with") if with_map else ("with", "without")))
        if with_map not in self._stages:
            self._stages[with_map] = loss_stages.stage_for(self, with_map)
        stage = self._stage = self._stages[with_map]
        stage.alloc()
        if with_map:  # [N,H,W] or [N,H,W,1] into the stage's static input
            stage.edges_in.copy_(self._f32(edges).reshape(stage.edges_in.shape), non_blocking=True)
        return stage

    def _set_inputs(self, input_a, input_b, gt_flow):
        """The step's inputs: frame pairs in both directions (no ground truth), else two inputs and the ground truth."""
        if self.unsupervised:
            return self._set_pairs(input_a, input_b)
        self.gt.copy_(torch.as_tensor(gt_flow).to(dtype=torch.float32), non_blocking=True)
        self.eng.set_inputs(input_a, input_b)

    def forward_backward(self, input_a, input_b, gt_flow, reduce=False, edges=None):
        """Loss and all parameter gradients (left in self.grad_arena).  Returns the loss as a device scalar.
        reduce=True: every gradient bucket is all-reduced as soon as backward has produced it (overlap);
        finish with apply_gradients(reduced_world=...) / wait_reduction()."""
        self._require_mode(False, "forward_backward")
        return self._forward_backward(input_a, input_b, gt_flow, edges, reduce)

    def _forward_backward(self, input_a, input_b, gt_flow, edges, reduce):
        """The eager step up to the gradients: inputs, zeroing, forward, the loss stage, backward."""
        s = _hip.stream_ptr()
        self._set_inputs(input_a, input_b, gt_flow)
        stage = self._pick_stage(edges)
        self._zero_buffers(s, stage)
        self.eng.launch()
        stage.launch(s)
        return self._backward(s, reduce)

    def _backward(self, s, reduce):
        """The backward launches behind the loss gradients in the _gbufs; returns the loss scalar."""
        from .dist import allreduce_bucket_async
        self._pending, nb = [], 0
        for i, (name, ops) in enumerate(self.bwd_ops):
            for fn, args in ops:
                rc = fn(*args, s)
                if rc:
                    try:
                        _hip.check(rc)
                    except Exception as e:
                        raise type(e)("backward of %s: %s" % (name, e)) from None
            if reduce and nb < len(self.buckets) and self.buckets[nb][0] == i:
                h = allreduce_bucket_async(self.buckets[nb][1])
                if h is not None:
                    self._pending.append(h)
                nb += 1
        return self.loss_dev

    def _zero_buffers(self, s, stage):
        """Zero what the step accumulates into: the flat parameter-gradient arena, the activation-gradient buffers whose
        first writer adds (the others are stored into, _plan_zeroing), the loss scalar, stage.zeroed -- memset nodes."""
        lib = self.lib
        _hip.check(lib.fn2_fill_zero(_hip.ptr(self.grad_arena), self.grad_arena.numel() * 4, s))
        for g in self.gbufs.values():
            if g.data_ptr() not in self._no_zero:
                _hip.check(lib.fn2_fill_zero(_hip.ptr(g), g.numel() * g.element_size(), s))
        _hip.check(lib.fn2_fill_zero(_hip.ptr(self.loss_dev), 4, s))
        for buf in stage.zeroed:
            _hip.check(lib.fn2_fill_zero(_hip.ptr(buf), buf.numel() * buf.element_size(), s))

    def wait_reduction(self):
        """Block the compute stream on the outstanding bucket all-reduces; returns the number of ranks summed."""
        from .dist import world_size
        for h in getattr(self, "_pending", []):
            h.wait()
        self._pending = []
        return world_size()

    def l2_term(self):
        """0.5*l2*sum |W|^2 over the regularised weights (host-side report only)."""
        l2 = self.l2_reg
        return float(sum(0.5 * l2 * float((p["w"].double() ** 2).sum()) for p in self.params if p["reg"]))

    def apply_gradients(self, reduced_world=None):
        """All-reduce (unless the caller already did: reduced_world = number of ranks summed) + the optimiser update."""
        from .dist import allreduce_gradients
        # RCCL sum over xGMI; the mean is folded into the update's grad_scale
        world = reduced_world if reduced_world is not None else allreduce_gradients(self.grad_arena)
        self.step_count += 1
        self._upload_optim_hyper(world)
        self._launch_optim(_hip.stream_ptr())
        self.refresh_backward_weights(forward=False)

    # ------------------------------------------------------------------ validation
    def _crop(self, x):
        """Centre crop of a [N,H,W,C] batch to the engine's size (validation frames are not augmented, so they arrive
        at the dataset's size while the engine has the augmentation crop's, dataloader.FLYING_CHAIRS_PREPROCESS)."""
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        h, w = int(t.shape[1]), int(t.shape[2])
        if (h, w) == (self.H, self.W):
            return t
        if h < self.H or w < self.W:
            raise ValueError("validation frames %dx%d are smaller than the trainer's %dx%d" % (h, w, self.H, self.W))
        y0, x0 = (h - self.H) // 2, (w - self.W) // 2
        return t[:, y0:y0 + self.H, x0:x0 + self.W]

    def evaluate(self, batches, max_batches=None):
        """Forward-only pass over an iterable of (image_a, image_b, gt_flow) device batches with the CURRENT weights:
        mean endpoint error of the full-resolution `flow` output against the ground truth, in pixels -- the validation
        the reference interleaves with training (Net.train's custom train_step_fn, net.py:1300-1380: every
        `valid_iters` steps, average EPE over the validation batches)."""
        total, count, crop = 0.0, 0, self._crop
        for i, (a, b, gt) in enumerate(batches):
            if max_batches is not None and i >= max_batches:
                break
            a, b, gt = crop(a), crop(b), crop(gt)
            self.eng.set_inputs(a, b)
            self.eng.launch()
            d = self.eng.outputs["flow"] - self._f32(gt)
            total += float(torch.sqrt((d * d).sum(dim=3)).mean().item())
            count += 1
        return total / max(count, 1)

    # ------------------------------------------------------------------ optimizer state (checkpoint resume)
    def _to_reference_layout(self, p, flat):
        """A packed fp32 tensor with the geometry of parameter p -> the reference layout of that variable."""
        rec = p["rec"]
        a = flat.detach().cpu().numpy().reshape(-1)
        if rec is None:
            return a.copy()                       # bias
        if rec["kind"] == "upflow":
            return a.reshape(4, 4, 2, 2).copy()
        return a[_index_hwio(rec)].astype(np.float32)

    def _from_reference_layout(self, p, arr):
        rec = p["rec"]
        arr = np.asarray(arr, np.float32)
        if rec is None or rec["kind"] == "upflow":
            return arr.reshape(-1)
        out = np.zeros(p["n"], np.float32)
        out[_index_hwio(rec).reshape(-1)] = arr.reshape(-1)
        return out

    def _optim_hyper(self, world):
        """The eight floats of fn2_optim_step_multi_dev for the step that self.step_count already counts: the rate and
        the momentum are taken at the global step before the update, as the reference's graph reads them."""
        step = self.step_count - 1
        lr = self.learning_rate(step)
        b1, b2 = self.schedule["momentum"], self.schedule["momentum2"]
        if self.optimizer == "momentum":
            from .training_schedules import momentum_value
            b1 = momentum_value(self.schedule, step, getattr(self, "train_params", None), self.momentum,
                                self.min_momentum, self.max_momentum)
        elif self.optimizer in ("adam", "adamw"):
            t = float(self.step_count)
            lr = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
        return [lr, b1, b2, self.eps, 1.0 / (world * self.loss_scale), self.weight_decay, self.clip_norm, 0.0]

    def _build_optim_tables(self):
        """What fn2_optim_step_multi_dev reads, built once at construction (nothing is allocated in a capture): the table
        {w, m, v, g, split-fp16 forward copy of w (or 0), its scale} per parameter tensor -- the update rewrites the copy the
        forward convolutions read while it has the new master in registers --, the counts and L2 coefficients, the eight
        per-step floats (device + pinned staging) and, when clipping, the per-block partial sums."""
        l2 = self.l2_reg
        fwd = {master.data_ptr(): (wx2.data_ptr(), scale, frag_k) for wx2, master, scale, frag_k in self.fwd_copies}
        ptrs = []
        for p in self.params:
            wx2, scale, frag_k = fwd.get(p["w"].data_ptr(), (0, 1.0, 0))
            bits = int(np.float32(scale).view(np.uint32)) | (int(frag_k) << 32)
            slot = lambda t: t.data_ptr() if t is not None else 0  # (a slot this optimiser lacks: null, never read)
            ptrs.append([p["w"].data_ptr(), slot(p["m"]), slot(p["v"]), p["g"].data_ptr(), wx2, bits])
        self._adam_table = torch.tensor(ptrs, dtype=torch.int64, device=self.dev)
        self._adam_counts = torch.tensor([p["n"] for p in self.params], dtype=torch.int64, device=self.dev)
        self._adam_l2 = torch.tensor([l2 if p["reg"] else 0.0 for p in self.params], dtype=torch.float32, device=self.dev)
        self._hyper = torch.zeros(8, dtype=torch.float32, device=self.dev)
        self._hyper_host = torch.zeros(8, dtype=torch.float32).pin_memory()
        self._hyper_event = None
        if self.clip_norm > 0.0:  # (every slot is written by the first pass: no zeroing)
            self._partials = torch.empty(len(self.params) * _hip.OPTIM_PARTIALS, dtype=torch.float32, device=self.dev)

    def _upload_optim_hyper(self, world):
        """The step's eight floats through pinned staging: the device copy is overwritten in stream order, behind the
        previous step's update; the event makes the host wait until the previous copy has left the pinned floats."""
        if self._hyper_event is not None:
            self._hyper_event.synchronize()
        self._hyper_host.copy_(torch.tensor(self._optim_hyper(world), dtype=torch.float32))
        self._hyper.copy_(self._hyper_host, non_blocking=True)
        self._hyper_event = torch.cuda.Event()
        self._hyper_event.record()

    def _launch_optim(self, s):
        """The per-tensor squared norms (only when clipping) and the update: two launches for all parameter tensors."""
        args = (_hip.ptr(self._adam_table), _hip.ptr(self._adam_counts), _hip.ptr(self._adam_l2), len(self.params),
                _hip.ptr(self._hyper))
        partials = None
        if self.clip_norm > 0.0:
            partials = _hip.ptr(self._partials)
            _hip.check(self.lib.fn2_optim_grad_sumsq_multi(*args, partials, s))
        _hip.check(self.lib.fn2_optim_step_multi_dev(_hip.OPTIM_KINDS[self.optimizer], *args, partials, s))

    def _slots(self, p):
        """[(TensorFlow slot suffix, tensor)] of parameter p under this optimiser."""
        if self.optimizer == "momentum":
            return [("/Momentum", p["m"])]
        if self.optimizer == "sgd":
            return []
        return [("/Adam", p["m"]), ("/Adam_1", p["v"])]

    def optimizer_state(self):
        """Adam's moments and counters under TensorFlow's slot names, in the reference layouts: ``<var>/Adam`` (m),
        ``<var>/Adam_1`` (v), ``beta1_power``, ``beta2_power`` (tf.train.AdamOptimizer, net.py:1290-1295) and
        ``global_step`` -- what the reference's Saver writes next to the variables, so a resumed run continues the
        moment estimates and the learning-rate schedule instead of restarting them.  adamw writes the same names (the
        generated class keeps the base optimiser's), momentum ``<var>/Momentum``, sgd nothing but ``global_step``."""
        b1, b2 = self.schedule["momentum"], self.schedule["momentum2"]
        out = {"global_step": np.int64(self.step_count)}
        if self.n_slots == 2:
            out.update(beta1_power=np.float32(b1 ** (self.step_count + 1)), beta2_power=np.float32(b2 ** (self.step_count + 1)))
        for p in self.params:
            for suffix, slot in self._slots(p):
                out[p["name"] + suffix] = self._to_reference_layout(p, slot)
        return out

    def load_optimizer_state(self, state):
        """Restore what optimizer_state() wrote (or a TensorFlow checkpoint of the reference holds).  Returns the
        number of slot tensors restored; variables without slots keep zero moments.  Only this optimiser's own slots are
        read: from a checkpoint written under another optimiser nothing but ``global_step`` is restored."""
        n = 0
        for p in self.params:
            for suffix, dst in self._slots(p):
                if p["name"] + suffix in state:
                    dst.copy_(torch.from_numpy(np.array(self._from_reference_layout(p, state[p["name"] + suffix]))))
                    n += 1
        if "global_step" in state:
            self.step_count = int(np.asarray(state["global_step"]).reshape(-1)[0])
        return n

    def train_step(self, input_a, input_b, gt_flow, edges=None):
        """One step: forward, loss, backward, gradient all-reduce (data parallel), Adam.  The launch sequence is
        captured once as hipGraph segments (cut where a gradient bucket is handed to the all-reduce) and replayed:
        the per-step scalars of the update live in device memory, so nothing in the segments changes between steps.  The
        mining losses are part of the graph: their pixel weights come from fn2_hfem_hard_weights (one launch for the
        five scales) or fn2_hfem_edge_weights, on buffers allocated before the capture.
        edges: the edge map of the 'edges' mode, [N,H,W] or [N,H,W,1]; the other modes ignore it.  Whether it is given
        is fixed by the first captured step ('edges' without a map is plain AEPE, as on the eager path): a later step
        that contradicts that choice raises ValueError.
        FN2_TRAIN_GRAPH=0: the eager launch sequence."""
        self._require_mode(False, "train_step")
        return self._step(input_a, input_b, gt_flow, edges)

    def _step(self, input_a, input_b, gt_flow, edges=None):
        """train_step* behind their mode checks: the captured step, or with FN2_TRAIN_GRAPH=0 the eager sequence."""
        if int(os.environ.get("FN2_TRAIN_GRAPH", "1")):
            return self._train_step_graph(input_a, input_b, gt_flow, edges)
        loss = self._forward_backward(input_a, input_b, gt_flow, edges, reduce=True)
        self.apply_gradients(reduced_world=self.wait_reduction())
        return loss

    # ------------------------------------------------------------------ unsupervised step
    def _require_mode(self, unsupervised, what):
        if self.unsupervised != unsupervised:
            raise ValueError("%s belongs to %s trainer; this one was built with unsupervised=%s"
                             % (what, "an unsupervised" if unsupervised else "a supervised", self.unsupervised))

    def _set_pairs(self, image_a, image_b):
        """[P,H,W,3] frames of P = batch / 2 pairs into the engine's 2P slots, both directions (device copies)."""
        from .photometric import interleave_pairs
        a, b = self._f32(image_a), self._f32(image_b)
        want = (self.N // 2, self.H, self.W, 3)
        if tuple(a.shape) != want or tuple(b.shape) != want:
            raise ValueError("unsupervised step: frames must be %s (batch / 2 pairs), got %s and %s"
                             % (want, tuple(a.shape), tuple(b.shape)))
        interleave_pairs(a, b, self.eng.in_a, self.eng.in_b)

    def forward_backward_unsupervised(self, image_a, image_b, reduce=False):
        """forward_backward without a ground truth: image_a / image_b are [batch / 2, H, W, 3] frames in [0,1]; the
        loss is the photometric one (left in self.loss_dev, returned), the gradients are left in self.grad_arena."""
        self._require_mode(True, "forward_backward_unsupervised")
        return self._forward_backward(image_a, image_b, None, None, reduce)

    def train_step_unsupervised(self, image_a, image_b):
        """train_step without a ground truth, captured and replayed the same way (FN2_TRAIN_GRAPH=0: eager)."""
        self._require_mode(True, "train_step_unsupervised")
        return self._step(image_a, image_b, None)

    # ------------------------------------------------------------------ sparse ground truth
    def evaluate_sparse(self, batches, max_batches=None):
        """evaluate() for sparse ground truth: forward-only over (image_a, image_b, gt_flow) batches with the current
        weights, the full-resolution `flow` output scored over the pixels whose ground truth is finite.  Returns
        {"epe": mean endpoint error in pixels, "fl_all": share of those pixels with an error above 3 px AND above 5 % of
        the ground truth's magnitude (the KITTI devkit's outlier rule), "valid_share": valid pixels / all pixels}; epe and
        fl_all are NaN when no pixel is valid."""
        err = torch.zeros((), dtype=torch.float64, device=self.dev)
        bad = torch.zeros((), dtype=torch.float64, device=self.dev)
        valid_n, total_n, crop = torch.zeros((), dtype=torch.float64, device=self.dev), 0, self._crop
        for i, (a, b, gt) in enumerate(batches):
            if max_batches is not None and i >= max_batches:
                break
            a, b, gt = crop(a), crop(b), crop(gt)
            self.eng.set_inputs(a, b)
            self.eng.launch()
            gt_dev = self._f32(gt)
            valid = torch.isfinite(gt_dev).all(dim=3)
            gt0 = torch.where(valid[..., None], gt_dev, torch.zeros_like(gt_dev))
            d = self.eng.outputs["flow"] - gt0
            e = torch.sqrt((d * d).sum(dim=3))
            mag = torch.sqrt((gt0 * gt0).sum(dim=3))
            err += torch.where(valid, e, torch.zeros_like(e)).double().sum()
            bad += (valid & (e > 3.0) & (e > 0.05 * mag)).double().sum()
            valid_n += valid.double().sum()
            total_n += valid.numel()
        m = float(valid_n.item())
        nan = float("nan")
        return {"epe": float(err.item()) / m if m else nan, "fl_all": float(bad.item()) / m if m else nan,
                "valid_share": m / total_n if total_n else 0.0}

    # ------------------------------------------------------------------ captured step
    def _segment_body(self, seg):
        """Launches of segment `seg` on torch's current stream.  Segment 0 starts with the zeroing, the forward and
        the loss; segment i ends behind the backward launch that completes gradient bucket i; the last segment is the
        optimiser update and the refresh of the derived weight copies."""
        eng, s = self.eng, _hip.stream_ptr()
        nseg = len(self._seg_ends)
        if seg == 0:
            self._zero_buffers(s, self._captured)
            eng.launch()
            self._captured.launch(s)
        if seg < nseg:
            lo = 0 if seg == 0 else self._seg_ends[seg - 1] + 1
            # (the filter gradients as a parallel path of the graph -- they need only the layer's finished output
            # gradient and nothing waits for them before the segment ends -- measured 6.63 -> 6.55 ms: not taken)
            for name, ops in self.bwd_ops[lo:self._seg_ends[seg] + 1]:
                for fn, args in ops:
                    _hip.check(fn(*args, s))
            return
        self._launch_optim(s)
        self.refresh_backward_weights(forward=False)

    def _capture_step(self, stage):
        from .dist import exchange_enabled
        # one segment per gradient bucket when the gradients are exchanged, else a single backward segment
        self._seg_ends = [i for i, _ in self.buckets] if exchange_enabled() else [len(self.bwd_ops) - 1]
        self._captured = stage  # (allocated, and with it the _gbufs of the predictions: nothing is allocated in the capture)
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream())
        graphs = []
        with torch.cuda.stream(side):
            for seg in range(len(self._seg_ends) + 1):
                if seg < len(self._seg_ends):
                    self._segment_body(seg)  # warm (module load, first touch); Adam is NOT run un-captured
                side.synchronize()
                _hip.check(self.lib.fn2_capture_begin(_hip.stream_ptr()))
                try:
                    self._segment_body(seg)
                finally:
                    g = C.c_void_p()
                    rc = self.lib.fn2_capture_end(_hip.stream_ptr(), C.byref(g))
                _hip.check(rc)
                graphs.append(g)
        torch.cuda.current_stream().wait_stream(side)
        self._step_graphs = graphs

    def _train_step_graph(self, input_a, input_b, gt_flow, edges=None):
        from .dist import allreduce_bucket_async, exchange_enabled, world_size
        stage = self._pick_stage(edges, captured=True)
        if getattr(self, "_step_graphs", None) is None:
            self._capture_step(stage)
        self._set_inputs(input_a, input_b, gt_flow)
        world = world_size()
        self.step_count += 1
        self._upload_optim_hyper(world)
        s = _hip.stream_ptr()
        pending = []
        for i in range(len(self._seg_ends)):
            _hip.check(self.lib.fn2_graph_launch(self._step_graphs[i], s))
            if exchange_enabled():
                h = allreduce_bucket_async(self.buckets[i][1])
                if h is not None:
                    pending.append(h)
        timed = pending and getattr(self, "wait_events", None) is not None
        if timed:  # bench.py: how long the compute stream sits in the bucket waits (the part of the exchange backward did not hide)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for h in pending:
            h.wait()
        if timed:
            e1.record()
            self.wait_events.append((e0, e1))
        _hip.check(self.lib.fn2_graph_launch(self._step_graphs[-1], s))
        return self.loss_dev
