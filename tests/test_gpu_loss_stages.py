"""The loss stage of the trainer (src/loss_stages.py): the eager step and segment 0 of the captured step issue the same
launches, on the same preallocated buffers, in every loss mode.

trainer.lib is replaced by a proxy that notes the name of every fn2_* entry point called through it and passes the call on.
The engine and the backward launch lists hold their own bound functions, so what is noted is the trainer's own: the
zeroing (fn2_fill_zero) and the loss stage.  Batch 2 at 128 x 128, fp32: five loss scales of 2 x 2 to 32 x 32."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LABEL, L = "fn2_downsample_scaled_f32", 5
WEIGHTED = "fn2_epe_loss_grad_weighted"
PHOTOMETRIC = L * ["fn2_downsample_f32"] + ["fn2_photometric_masks", "fn2_photometric_loss_grad"]
# mode: (model, trainer arguments, step with an edge map, kind of the stage, the fn2_* calls behind the zeroing)
MODES = {
    "dense": ("FlowNetS", {}, False, "dense", L * [LABEL, "fn2_epe_loss_grad"]),
    "photometric": ("FlowNetS", dict(unsupervised=True), False, "photometric", PHOTOMETRIC),
    "photometric+smoothness": ("FlowNetS", dict(unsupervised=True, smoothness_weight=0.5), False, "photometric",
                               PHOTOMETRIC + ["fn2_smoothness_loss_grad"]),
    "sparse": ("FlowNetS", dict(sparse_gt=True), False, "sparse",
               L * [LABEL] + ["fn2_sparse_epe_count", "fn2_sparse_epe_loss_grad"]),
    "hard": ("FlowNetS_interp", dict(add_hard_flow_mining="hard"), False, "hard",
             L * [LABEL] + ["fn2_hfem_hard_weights"] + L * [WEIGHTED]),
    "edges": ("FlowNetS_interp", dict(add_hard_flow_mining="edges"), True, "edges",
              L * [LABEL] + L * ["fn2_downsample_f32", "fn2_hfem_edge_weights", WEIGHTED]),
    "edges, no map": ("FlowNetS_interp", dict(add_hard_flow_mining="edges"), False, "dense",
                      L * [LABEL, "fn2_epe_loss_grad"]),
}


class Recorder:
    """Notes the fn2_* names called through it; every call goes through to the library."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("fn2_"):
            return fn

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def stage_pointers(stage):
    """{attribute or (attribute, key): data_ptr} of every tensor the stage holds, directly or in a dict or level list."""
    out = {}
    for name, v in vars(stage).items():
        items = v.items() if isinstance(v, dict) else enumerate(v) if isinstance(v, list) else [(None, v)]
        for key, t in items:
            for j, u in enumerate(t if isinstance(t, tuple) else (t,)):
                if isinstance(u, torch.Tensor):
                    out[(name, key, j)] = u.data_ptr()
    return out


def steps_of(tr, model, with_map):
    """(captured step, eager step) as functions of a seed, on seeded inputs of the trainer's mode."""
    from test_gpu_hfem import _interp_batch
    from test_gpu_photometric_train import frames
    from test_gpu_train import data
    if tr.unsupervised:
        args = lambda seed: frames(1, 128, 128, seed)
        return (lambda seed: tr.train_step_unsupervised(*args(seed)),
                lambda seed: tr.forward_backward_unsupervised(*args(seed)))
    if model == "FlowNetS_interp":
        def args(seed):
            a, matches, sparse, gt, edges = _interp_batch(seed)
            return (a, matches, sparse, gt), dict(edges=edges if with_map else None)
        return (lambda seed: tr.train_step_interp(*args(seed)[0], **args(seed)[1]),
                lambda seed: tr.forward_backward_interp(*args(seed)[0], **args(seed)[1]))

    def args(seed):
        a, b, gt = data(2, 128, 128, seed)
        if tr.sparse_gt:
            gt = gt.copy()
            gt[:, :, 64:] = np.nan
        return a, b, gt
    return (lambda seed: tr.train_step(*args(seed)), lambda seed: tr.forward_backward(*args(seed)))


@pytest.mark.parametrize("mode", list(MODES))
def test_eager_and_captured_steps_issue_the_same_loss_launches_on_the_same_buffers(mode):
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    model, kw, with_map, kind, want = MODES[mode]
    tr = FlowNetSTrainer(W.init_weights(model, 9), 2, 128, 128, dtype="f32", model=model, **kw)
    captured_step, eager_step = steps_of(tr, model, with_map)
    old = os.environ.get("FN2_TRAIN_GRAPH")
    try:
        os.environ["FN2_TRAIN_GRAPH"] = "1"
        captured_step(4)
    finally:
        if old is None:
            os.environ.pop("FN2_TRAIN_GRAPH", None)
        else:
            os.environ["FN2_TRAIN_GRAPH"] = old
    assert getattr(tr, "_step_graphs", None) is not None and tr._captured.kind == kind
    assert len(tr._seg_ends) == 1                                  # one rank: segment 0 holds the whole backward pass
    rec = tr.lib = Recorder(tr.lib)
    try:
        tr._segment_body(0)
        segment = rec.take()
        eager_step(4)
        eager = rec.take()
        stage = tr._stage
        before = stage_pointers(stage)
        eager_step(40)
        second = rec.take()
    finally:
        tr.lib = rec._lib
    torch.cuda.synchronize()
    print("%s: %s" % (mode, eager))
    assert stage is tr._captured and tr._stage is stage and stage.kind == kind
    for calls in (segment, eager, second):
        zeroing = len(calls) - len(want)
        assert zeroing >= 2 and calls[:zeroing] == zeroing * ["fn2_fill_zero"]     # the arena and the loss at the least
        assert calls[zeroing:] == want
    assert segment == eager == second
    assert len(before) >= L and stage_pointers(stage) == before     # the second step allocated nothing in the stage
    assert np.isfinite(float(tr.loss_dev.item()))
