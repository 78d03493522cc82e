"""The smoothness term inside the unsupervised train step (FlowNetSTrainer(unsupervised=True, smoothness_weight=...)).

The argument continues the one of test_gpu_photometric_train.py: everything behind the gradient buffers `_gbuf(predict_flow_l)`
is pinned whatever filled them, and the photometric loss that fills them first is pinned there.  So the term is right end to
end if (1) a weight of 0 leaves the step exactly what it was, (2) with a weight the five `_gbuf`s are the photometric-only
ones plus the float64 twin's smoothness gradient on the device's predictions and level frames, and `loss_dev` the sum, and
(3) the captured step replays that sequence.  The forward pass is deterministic, so two trainers on the same weights and
frames hold the same predictions bit for bit (asserted): the photometric part of (2) is taken from a weight-0 trainer."""
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import smoothness_twin as twin
from test_gpu_photometric_train import FRAME_SEED, PKG, ROOT, SAMPLES, frames, level_scale

GRAD_TOL, LOSS_TOL, STEP_TOL = 2e-5, 1e-5, 2e-5
N, H, W = 2, 64, 128
SMOOTH = dict(smoothness_weight=0.75, edge_lambda=150.0, smoothness_eps=1e-3)
CONFIGS = [("f32", 1), ("f32", 2), ("f16x2", 1)]


def one_forward_backward(dtype, **kw):
    """forward_backward_unsupervised on the seeded frames; the gradient buffers are read where the losses have filled them
    and backward has not yet added the upsampling paths into them."""
    import torch
    from src import weights as Wt
    from src.trainer import FlowNetSTrainer
    tr = FlowNetSTrainer(Wt.init_weights("FlowNetS", 1234), N, H, W, dtype=dtype, model="FlowNetS", unsupervised=True, **kw)
    a, b = frames(N // 2, H, W, FRAME_SEED)
    snap = {}
    real = tr._backward

    def spy(s, reduce):
        torch.cuda.synchronize()
        snap["g"] = {p: tr._gbuf(tr.eng.outputs[p]).cpu().numpy().copy() for p in tr.loss_terms}
        snap["loss"] = float(tr.loss_dev.item())
        return real(s, reduce)

    tr._backward = spy
    tr.forward_backward_unsupervised(a, b)
    torch.cuda.synchronize()
    ph = tr._photo
    return types.SimpleNamespace(
        g=snap["g"], loss=snap["loss"], weights=dict(tr.loss_terms), loss_scale=tr.loss_scale,
        preds={p: tr.eng.outputs[p].cpu().numpy().copy() for p in tr.loss_terms},
        imgs={p: ph.imgs[p].cpu().numpy() for p in ph.names}, arena=tr.grad_arena.cpu().numpy())


@functools.lru_cache(maxsize=None)
def photometric_only(dtype):
    """The step of a trainer built without the new arguments."""
    return one_forward_backward(dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_weight_zero_leaves_the_step_bitwise_what_it_was(dtype):
    base = photometric_only(dtype)
    zero = one_forward_backward(dtype, smoothness_weight=0.0, smoothness_order=2, edge_lambda=10.0)
    assert list(zero.g) == list(base.g) and len(base.g) == 5
    for p in base.g:
        np.testing.assert_array_equal(zero.preds[p], base.preds[p])
        np.testing.assert_array_equal(zero.g[p], base.g[p])
    assert abs(zero.loss - base.loss) <= 1e-6 * base.loss          # (one atomic per block and level: the order is free)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,order", CONFIGS, ids=["%s-order%d" % c for c in CONFIGS])
def test_gradient_buffers_and_loss_are_photometric_plus_the_twin(dtype, order):
    base = photometric_only(dtype)
    got = one_forward_backward(dtype, smoothness_order=order, **SMOOTH)
    names = list(base.g)
    scales = [level_scale("FlowNetS", got.preds[p].shape[2], W) for p in names]
    levels, want_smooth = twin.total([got.imgs[p] for p in names], [got.preds[p] for p in names], scales,
                                     [got.weights[p] for p in names], order=order, edge_lambda=SMOOTH["edge_lambda"],
                                     eps=SMOOTH["smoothness_eps"], smooth_weight=SMOOTH["smoothness_weight"],
                                     grad_mult=got.loss_scale)
    assert want_smooth > 0
    for p, (L, g) in zip(names, levels):
        np.testing.assert_array_equal(got.preds[p], base.preds[p])  # the same forward pass, bit for bit
        np.testing.assert_array_equal(got.imgs[p], base.imgs[p])
        want = base.g[p].astype(np.float64) + g
        if min(got.preds[p].shape[1:3]) == 1:
            assert L == 0.0 and not g.any()
            np.testing.assert_array_equal(got.g[p], base.g[p])
            continue
        err = np.abs(got.g[p] - want).max() / np.abs(want).max()
        print("%s order %d %s: smoothness L = %.6g, its largest gradient %.3g of the photometric one's; worst error %.3e of the "
              "largest" % (dtype, order, p, L, np.abs(g).max() / max(np.abs(base.g[p]).max(), 1e-30), err))
        assert g.any() and err <= GRAD_TOL
    want_loss = base.loss + want_smooth
    print("%s order %d: loss %.9g, photometric %.9g + twin %.9g" % (dtype, order, got.loss, base.loss, want_smooth))
    assert abs(got.loss - want_loss) <= LOSS_TOL * want_loss
    assert np.isfinite(got.arena).all() and not np.array_equal(got.arena, base.arena)


# ------------------------------------------------------------------------------------------------ one training step
@pytest.fixture(scope="module", params=["f32", "f16x2"])
def steps(request):
    """Two captured steps (other frames in the second) and one eager step from the same weights, smoothness on."""
    import torch
    from src import weights as Wt
    from src.trainer import FlowNetSTrainer
    wts = Wt.init_weights("FlowNetS", 1234)
    make = lambda: FlowNetSTrainer(wts, N, H, W, dtype=request.param, model="FlowNetS", unsupervised=True,
                                   smoothness_order=2, **SMOOTH)
    b1, b2 = frames(1, H, W, 7), frames(1, H, W, 70)
    old = os.environ.get("FN2_TRAIN_GRAPH")
    try:
        os.environ["FN2_TRAIN_GRAPH"] = "1"
        tr = make()
        loss1 = float(tr.train_step_unsupervised(*b1).item())
        captured = getattr(tr, "_step_graphs", None) is not None
        g1 = tr.grad_arena.cpu().numpy().copy()
        loss2 = float(tr.train_step_unsupervised(*b2).item())
        os.environ["FN2_TRAIN_GRAPH"] = "0"
        eager = make()
        eager_loss = float(eager.train_step_unsupervised(*b1).item())
        eager_captured = getattr(eager, "_step_graphs", None) is not None
        torch.cuda.synchronize()
        eager_g = eager.grad_arena.cpu().numpy().copy()
    finally:
        if old is None:
            os.environ.pop("FN2_TRAIN_GRAPH", None)
        else:
            os.environ["FN2_TRAIN_GRAPH"] = old
    return types.SimpleNamespace(tr=tr, g1=g1, loss1=loss1, loss2=loss2, captured=captured, eager_loss=eager_loss,
                                 eager_captured=eager_captured, eager_g=eager_g, dtype=request.param)


@pytest.mark.gpu
def test_captured_step_matches_the_eager_sequence_and_replays(steps):
    assert steps.captured and not steps.eager_captured and steps.tr.step_count == 2
    print("%s: captured loss %.9g, eager %.9g, second replay %.9g" % (steps.dtype, steps.loss1, steps.eager_loss, steps.loss2))
    assert np.isfinite(steps.loss1) and steps.loss1 > 0
    assert abs(steps.loss1 - steps.eager_loss) <= STEP_TOL * abs(steps.eager_loss)
    assert np.abs(steps.g1 - steps.eager_g).max() <= STEP_TOL * np.abs(steps.eager_g).max()
    assert np.isfinite(steps.loss2) and steps.loss2 != steps.loss1   # the replay reads this step's frames


@pytest.mark.gpu
def test_cli_trains_with_pair_augmentation_and_the_smoothness_term(tmp_path):
    from src import weights as Wt
    lst = tmp_path / "pairs.txt"
    lst.write_text("%s %s\n" % (os.path.join(SAMPLES, "0img0.ppm"), os.path.join(SAMPLES, "0img1.ppm")))
    out = tmp_path / "ck"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-m", "src.flownet_s.train", "--unsupervised", "--augmentation", "pair",
                          "--smoothness_weight", "1", "--steps", "2", "--batch", "2", "--list", str(lst), "--out", str(out),
                          "--log-every", "1"], cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "global step      2" in res.stdout
    ck = Wt.load_weights(str(out / "flownet_s-2.npz"))
    assert "FlowNetS/conv1/weights" in ck and all(np.isfinite(np.asarray(v)).all() for v in ck.values())
