"""The unsupervised train step (FlowNetSTrainer(unsupervised=True), src/trainer.py) end to end.

The argument: the trainer's backward pass, gradient buckets, all-reduce, optimisers and the captured step are pinned to
2e-5 by test_gpu_train.py, test_gpu_optimizers.py and test_gpu_hfem.py from the gradient buffers `_gbuf(predict_flow_l)`
onward -- whatever loss filled them.  So the new loss is right end to end if (1) the engine's inputs hold the interleaved
slots, (2) the level images are the pinned downsample of them, (3) the masks are the pinned occlusion op on s_l * pred
within `valid`, (4) the five `_gbuf`s and `loss_dev` equal the float64 twin fed the device's predictions, level images and
masks, and (5) the captured step replays exactly that sequence.  These are the tests below.

One discontinuity is left out of (4) by construction of the inputs, not by a tolerance: psi'(d) jumps by 2 q 0.01^(q-1) at
d = 0, so a residual within fp32 rounding (1e-7) of 0 could take the other sign on the device.  The frames are random fields
with contrast at every scale, seeded so that no unmasked residual is below 1e-6, and the twin's residuals are asserted to
keep that distance (on the CPU too, with the oracle's predictions: test_photometric_cpu.py)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import photometric_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "flownet2-tf_amd")
SAMPLES = os.path.join(ROOT, "tests", "golden", "samples")
U = 2.0 ** -24
GRAD_TOL, LOSS_TOL, STEP_TOL = 2e-5, 1e-5, 2e-5   # STEP_TOL: captured against eager, as test_gpu_hfem.py
BAND_CAP = 0.01
FRAME_SEED = 12   # smallest unmasked residual over the f32 configurations: 1.6e-5 on the oracle's predictions
CONFIGS = [("FlowNetS", 2, 64, 128, "f32"), ("FlowNetSD", 2, 64, 128, "f32"), ("FlowNetS", 4, 128, 192, "f32"),
           ("FlowNetS", 2, 64, 128, "f16x2")]
IDS = ["%s-b%d-%dx%d-%s" % c for c in CONFIGS]


def _field(rng, pairs, h, w):
    """Random colours at six octaves (blocks of 1, 2, ... 32 pixels) averaged: contrast at every loss scale, and the
    finest octave leaves no patch flat."""
    out = 0.0
    for k in range(6):
        b = 1 << k
        coarse = rng.random((pairs, -(-h // b), -(-w // b), 3))
        out = out + np.kron(coarse, np.ones((1, b, b, 1)))[:, :h, :w]
    return out / 6.0


def frames(pairs, h, w, seed):
    """(a, b) [pairs,h,w,3] in [0,1]: a multi-octave random field, and the same shifted by (1, -2) mixed with a fifth of
    another field, so that the residuals are of the order 0.01 .. 0.1 at every scale and none sits at the kink of psi."""
    rng = np.random.default_rng(seed)
    a = _field(rng, pairs, h, w)
    b = 0.8 * np.roll(a, (1, -2), (1, 2)) + 0.2 * _field(rng, pairs, h, w)
    return a.astype(np.float32), b.astype(np.float32)


def slots(a, b):
    """The engine's two inputs for the pairs (a_k, b_k): A = (a_0, b_0, a_1, ...), B = (b_0, a_0, b_1, ...)."""
    A, B = np.empty((2 * len(a),) + a.shape[1:], np.float32), np.empty((2 * len(a),) + a.shape[1:], np.float32)
    A[0::2], A[1::2], B[0::2], B[1::2] = a, b, b, a
    return A, B


def level_scale(model, w_l, W):
    """s_l = (1 / gt_scale) * (w_l / W): 0.05-scaled predictions for FlowNetS, 20-scaled for FlowNetSD."""
    return (1.0 / (20.0 if model == "FlowNetSD" else 0.05)) * (w_l / float(W))


def band_of(parts, h, w):
    """Pixels whose mask may differ between two fp32 evaluations: |d - t| within 8 roundings of d + t, or a position
    within one fp32 ulp of a bound of `valid`."""
    near = lambda v, bound: np.abs(v.astype(np.float64) - bound) <= np.spacing(np.float32(max(bound, 1.0)))
    with np.errstate(all="ignore"):
        close = np.abs(parts["d"] - parts["t"]) <= 8 * U * (parts["d"] + parts["t"])
    return close | near(parts["X"], 0.0) | near(parts["X"], w - 1.0) | near(parts["Y"], 0.0) | near(parts["Y"], h - 1.0)


def twin_levels(model, W, preds, alpha=0.01, beta=0.5):
    """{name: (mask, parts, band)} of the twin on the predictions {name: [n,h,w,2]}."""
    out = {}
    for name, p in preds.items():
        mask, parts = twin.masks(p, level_scale(model, p.shape[2], W), alpha, beta)
        out[name] = (mask, parts, band_of(parts, p.shape[1], p.shape[2]))
    return out


# ------------------------------------------------------------------------------------------------ one forward-backward
@pytest.fixture(scope="module", params=CONFIGS, ids=IDS)
def fb(request):
    """One forward_backward_unsupervised per configuration; the gradient buffers are read where the loss has filled them
    and backward has not yet added the upsampling paths into them."""
    import torch
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    model, n, h, w, dtype = request.param
    wts = W.init_weights(model, 1234)
    tr = FlowNetSTrainer(wts, n, h, w, dtype=dtype, model=model, unsupervised=True)
    a, b = frames(n // 2, h, w, FRAME_SEED)
    snap = {}
    real = tr._backward

    def spy(s, reduce):
        torch.cuda.synchronize()
        snap["g"] = {p: tr._gbuf(tr.eng.outputs[p]).cpu().numpy().copy() for p in tr.loss_terms}
        snap["loss"] = float(tr.loss_dev.item())
        return real(s, reduce)

    tr._backward = spy
    loss = tr.forward_backward_unsupervised(a, b)
    torch.cuda.synchronize()
    del tr._backward
    ph = tr._photo
    return types.SimpleNamespace(
        cfg=request.param, tr=tr, a=a, b=b, snap=snap, loss=float(loss.item()),
        preds={p: tr.eng.outputs[p].cpu().numpy().copy() for p in tr.loss_terms},
        imgs={p: ph.imgs[p].cpu().numpy() for p in ph.names}, masks={p: ph.masks[p].cpu().numpy() for p in ph.names},
        counts=ph.counts.cpu().numpy(), arena=tr.grad_arena.cpu().numpy())


@pytest.mark.gpu
def test_engine_inputs_hold_the_interleaved_slots(fb):
    from src.downsample import downsample
    A, B = slots(fb.a, fb.b)
    np.testing.assert_array_equal(fb.tr.eng.in_a.cpu().numpy(), A)
    np.testing.assert_array_equal(fb.tr.eng.in_b.cpu().numpy(), B)
    for p, img in fb.imgs.items():                                 # the frames at the level's size: the pinned op on A
        if min(img.shape[1:3]) == 1:                               # (no valid pixel there: never formed, never read)
            assert not img.any() and not fb.masks[p].any()
            continue
        np.testing.assert_array_equal(img, downsample(fb.tr.eng.in_a, list(img.shape[1:3])).cpu().numpy())
    assert list(fb.tr._photo.scales.values()) == [level_scale(fb.cfg[0], fb.preds[p].shape[2], fb.cfg[3]) for p in fb.preds]


@pytest.mark.gpu
def test_level_masks_are_the_pinned_occlusion_op_within_valid(fb):
    import torch
    from src.occlusion import occlusion
    model, n, h, w, _ = fb.cfg
    lv = twin_levels(model, w, fb.preds)
    in_band = total = 0
    for i, (p, (mask, parts, band)) in enumerate(lv.items()):
        got = fb.masks[p]
        assert np.all((got == 0) | (got == 1)) and fb.counts[i] == got.sum()
        f = fb.tr.eng.outputs[p] * fb.tr._photo.scales[p]          # fl(s_l * pred), as the kernel forms it
        np.testing.assert_array_equal(f.cpu().numpy(), parts["f"].astype(np.float32))
        occ_fw, occ_bw = occlusion(f[0::2], f[1::2])
        occ = torch.stack([occ_fw, occ_bw], 1).reshape(got.shape).cpu().numpy()
        want = parts["valid"] & (occ == 0)
        np.testing.assert_array_equal(got[~band], want[~band].astype(np.float32))
        np.testing.assert_array_equal(got[~band], mask[~band].astype(np.float32))   # ... and the twin's
        in_band, total = in_band + int(band.sum()), total + band.size
    print("%s: %d of %d mask pixels in the band" % (fb.cfg, in_band, total))
    assert in_band <= BAND_CAP * total
    assert any(m.any() and not m.all() for m in fb.masks.values())


@pytest.mark.gpu
def test_gradient_buffers_and_loss_equal_the_twin(fb):
    """(4) of the module docstring: behind these buffers everything is pinned already."""
    model, n, h, w, _ = fb.cfg
    tr, names = fb.tr, list(fb.preds)
    scales = [level_scale(model, fb.preds[p].shape[2], w) for p in names]
    levels, want_loss = twin.total([fb.imgs[p] for p in names], [fb.preds[p] for p in names], scales,
                                   [tr.loss_terms[p] for p in names], q=0.4, grad_mult=tr.loss_scale,
                                   given_masks=[fb.masks[p] for p in names])
    for p, s, (L, g, m) in zip(names, scales, levels):
        d = twin.loss_and_grad(fb.imgs[p], fb.preds[p], m, s)[2]
        assert not m.any() or np.abs(d[m > 0]).min() > 1e-6      # no residual at the kink of psi (module docstring)
        got = fb.snap["g"][p]
        if not m.any():
            assert not got.any()
            continue
        err = np.abs(got - g).max() / np.abs(g).max()
        print("%s %s: M = %d, L = %.6g, worst gradient error %.3e of the largest" % (fb.cfg, p, m.sum(), L, err))
        assert err <= GRAD_TOL
        assert not got[m == 0].any()
    print("%s: loss %.9g, twin %.9g" % (fb.cfg, fb.snap["loss"], want_loss))
    assert want_loss > 0 and abs(fb.snap["loss"] - want_loss) <= LOSS_TOL * want_loss
    assert fb.loss == fb.snap["loss"]                              # backward leaves the scalar alone
    assert np.isfinite(fb.arena).all() and np.abs(fb.arena).max() > 0


# ------------------------------------------------------------------------------------------------ one training step
@pytest.fixture(scope="module", params=["f32", "f16x2"])
def steps(request):
    """Two captured steps (other frames in the second) and one eager step from the same weights."""
    import torch
    from src import weights as W
    from src.flownet_s.train import unpack_weights
    from src.trainer import FlowNetSTrainer
    wts = W.init_weights("FlowNetS", 1234)
    make = lambda: FlowNetSTrainer(wts, 2, 64, 128, dtype=request.param, model="FlowNetS", unsupervised=True)
    b1, b2 = frames(1, 64, 128, 7), frames(1, 64, 128, 70)
    old = os.environ.get("FN2_TRAIN_GRAPH")
    try:
        os.environ["FN2_TRAIN_GRAPH"] = "1"
        tr = make()
        w0 = unpack_weights(tr)
        loss1 = float(tr.train_step_unsupervised(*b1).item())
        captured = getattr(tr, "_step_graphs", None) is not None
        g1 = tr.grad_arena.cpu().numpy().copy()
        w1 = unpack_weights(tr)
        loss2 = float(tr.train_step_unsupervised(*b2).item())
        os.environ["FN2_TRAIN_GRAPH"] = "0"
        eager = make()
        eager_loss = float(eager.train_step_unsupervised(*b1).item())
        eager_captured = getattr(eager, "_step_graphs", None) is not None
        torch.cuda.synchronize()
        eager_g, eager_w = eager.grad_arena.cpu().numpy().copy(), unpack_weights(eager)
    finally:
        if old is None:
            os.environ.pop("FN2_TRAIN_GRAPH", None)
        else:
            os.environ["FN2_TRAIN_GRAPH"] = old
    return types.SimpleNamespace(tr=tr, w0=w0, w1=w1, g1=g1, loss1=loss1, loss2=loss2, captured=captured, eager_loss=eager_loss,
                                 eager_captured=eager_captured, eager_g=eager_g, eager_w=eager_w, dtype=request.param)


@pytest.mark.gpu
def test_captured_step_trains_and_matches_the_eager_sequence(steps):
    assert steps.captured and not steps.eager_captured and steps.tr.step_count == 2
    trained = [k for k in steps.w0 if k.startswith("FlowNetS/")]
    assert trained
    for k in trained:
        assert np.isfinite(steps.w1[k]).all() and not np.array_equal(steps.w1[k], steps.w0[k]), k
    print("%s: captured loss %.9g, eager %.9g, second replay %.9g" % (steps.dtype, steps.loss1, steps.eager_loss, steps.loss2))
    assert np.isfinite(steps.loss1) and steps.loss1 > 0
    assert abs(steps.loss1 - steps.eager_loss) <= STEP_TOL * abs(steps.eager_loss)
    assert np.abs(steps.g1 - steps.eager_g).max() <= STEP_TOL * np.abs(steps.eager_g).max()
    assert np.isfinite(steps.loss2) and steps.loss2 != steps.loss1   # the replay reads this step's frames


@pytest.mark.gpu
def test_cli_trains_on_a_list_without_ground_truth(tmp_path):
    from src import weights as W
    lst = tmp_path / "pairs.txt"
    lst.write_text("%s %s\n" % (os.path.join(SAMPLES, "0img0.ppm"), os.path.join(SAMPLES, "0img1.ppm")))
    out = tmp_path / "ck"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-m", "src.flownet_s.train", "--unsupervised", "--no-augment", "--steps", "2",
                          "--batch", "2", "--list", str(lst), "--out", str(out), "--log-every", "1"],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "global step      2" in res.stdout
    ck = W.load_weights(str(out / "flownet_s-2.npz"))
    assert "FlowNetS/conv1/weights" in ck and all(np.isfinite(np.asarray(v)).all() for v in ck.values())


@pytest.mark.gpu
def test_errors(fb, tmp_path):
    from src import weights as W
    from src.flownet_s import train as cli
    from src.trainer import FlowNetSTrainer
    for kw in (dict(batch=3), dict(model="FlowNet2"), dict(model="FlowNetS_interp"), dict(add_hard_flow_mining="hard")):
        with pytest.raises(ValueError):
            FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128, unsupervised=True), **kw))
    flags = cli.build_parser().parse_args(["--list", "l.txt", "--out", str(tmp_path), "--unsupervised"])
    with pytest.raises(ValueError, match="--no-augment"):
        cli.main(flags)
    model, n, h, w, dtype = fb.cfg
    A, B = slots(fb.a, fb.b)
    with pytest.raises(ValueError, match="supervised"):
        fb.tr.train_step(A, B, np.zeros((n, h, w, 2), np.float32))
    with pytest.raises(ValueError, match="supervised"):
        fb.tr.forward_backward(A, B, np.zeros((n, h, w, 2), np.float32))
    with pytest.raises(ValueError, match="batch / 2"):
        fb.tr.forward_backward_unsupervised(A, B)                  # slots, not pairs
    if fb.cfg == CONFIGS[0]:
        sup = FlowNetSTrainer(W.init_weights("FlowNetS", 1234), 2, 64, 128, dtype="f32")
        for call in (sup.train_step_unsupervised, sup.forward_backward_unsupervised):
            with pytest.raises(ValueError, match="unsupervised"):
                call(fb.a, fb.b)
