"""The unsupervised train step with data_term='census' (FlowNetSTrainer, src/loss_stages.py: Census) end to end.

The argument is test_gpu_photometric_train.py's: everything behind the gradient buffers `_gbuf(predict_flow_l)` is pinned
whatever loss filled them, and so are the level frames and the occlusion masks, which the census stage forms as the
photometric stage does.  Left to show: (1) on the scales that hold a 7 x 7 patch the warp pass turns the device's frames
and predictions into G, W, DX, DY, V; (2) S, the `_gbuf`s and `loss_dev` equal the float64 twin fed the device's buffers;
(3) the smaller scales keep the photometric term; (4) the eager and the captured step issue one launch list and agree.

2 x 64 x 128 frames: the scales are 1x2, 2x4, 4x8 (photometric) and 8x16, 16x32 (census).

Bound of (1).  G is compared exactly: it is three fp32 operations on the device's frames and NumPy performs the same three.
W is a sum of four products w_i G_i, DX and DY of four products w_i (+-G_i): the twin forms them in float64 from the same
fp32 position and the same G, the device in fp32 with at most eight roundings (weight factors, weights or differences,
products, sums -- contraction can only drop some), each bounded by 2^-24 times the largest intermediate, which is at most
max|G| sum|w_i| <= 255 sum|w_i|.  Where V = 1 the weights are products of factors in [0, 1] that sum to 1 per axis, so
sum|w_i| = 1 for W and 2 for DX and DY (every factor meets two taps): |error| <= 8 * 2^-24 * 255 * sum|w_i|.  Where V = 0
both store 0.  V itself compares fp32 positions formed alike on both sides, so it is exact unless a position lies within
an ulp of a bound of V -- that band is asserted empty."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import census_twin as twin
import photometric_twin as ptwin
from test_gpu_photometric_train import PKG, ROOT, SAMPLES, frames, level_scale

U = 2.0 ** -24
GRAD_TOL, LOSS_TOL, STEP_TOL = 2e-5, 1e-5, 2e-5
FRAME_SEED = 12
CONFIGS = [("FlowNetS", "f32"), ("FlowNetSD", "f32"), ("FlowNetS", "f16x2")]
N, H, W = 2, 64, 128
CENSUS, SMALL = ["predict_flow3", "predict_flow2"], ["predict_flow6", "predict_flow5", "predict_flow4"]
# the fn2_* calls of the loss stage at this size: no frame is formed for the 1 x 2 scale
FRAMES_AND_MASKS = 4 * ["fn2_downsample_f32"] + ["fn2_photometric_masks"]
CENSUS_CALLS = FRAMES_AND_MASKS + ["fn2_census_warp", "fn2_census_cost", "fn2_census_grad", "fn2_photometric_loss_grad"]
PHOTOMETRIC_CALLS = FRAMES_AND_MASKS + ["fn2_photometric_loss_grad"]


def graph_env(value):
    """Context manager: FN2_TRAIN_GRAPH set to `value`, restored behind."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        old = os.environ.get("FN2_TRAIN_GRAPH")
        os.environ["FN2_TRAIN_GRAPH"] = value
        try:
            yield
        finally:
            if old is None:
                os.environ.pop("FN2_TRAIN_GRAPH", None)
            else:
                os.environ["FN2_TRAIN_GRAPH"] = old
    return cm()


# ------------------------------------------------------------------------------------------------ one forward-backward
@pytest.fixture(scope="module", params=CONFIGS, ids=["%s-%s" % c for c in CONFIGS])
def fb(request):
    """One forward_backward_unsupervised per configuration; the gradient buffers are read where the loss has filled them
    and backward has not yet added the upsampling paths into them."""
    import torch
    from src import weights as Wt
    from src.trainer import FlowNetSTrainer
    model, dtype = request.param
    tr = FlowNetSTrainer(Wt.init_weights(model, 1234), N, H, W, dtype=dtype, model=model, unsupervised=True,
                         data_term="census")
    a, b = frames(N // 2, H, W, FRAME_SEED)
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
    st = tr._census
    get = lambda d: {p: v.cpu().numpy() for p, v in d.items()}
    return types.SimpleNamespace(
        cfg=request.param, model=model, tr=tr, st=st, a=a, b=b, snap=snap, loss=float(loss.item()),
        preds={p: tr.eng.outputs[p].cpu().numpy().copy() for p in tr.loss_terms}, imgs=get(st.imgs), masks=get(st.masks),
        grey=get(st.grey), warp=get(st.warp), valid=get(st.valid), coef=get(st.coef), counts=st.counts.cpu().numpy(),
        census_counts=st.census_counts.cpu().numpy(), arena=tr.grad_arena.cpu().numpy())


@pytest.mark.gpu
def test_the_stage_splits_the_scales(fb):
    st = fb.st
    assert st.kind == "census" and fb.tr._photo is None and list(fb.preds) == SMALL + CENSUS
    assert [tuple(fb.preds[p].shape[1:3]) for p in fb.preds] == [(1, 2), (2, 4), (4, 8), (8, 16), (16, 32)]
    assert st.census_names == CENSUS and list(st.grey) == CENSUS and len(st.census_table) == 2 and len(st.small_table) == 3
    assert st.zeroed[0] is st.counts and st.zeroed[1] is st.census_counts and len(st.zeroed) == 2
    assert list(st.scales.values()) == [level_scale(fb.model, fb.preds[p].shape[2], W) for p in fb.preds]


@pytest.mark.gpu
def test_warp_pass_on_the_device_frames_and_predictions(fb):
    """(1) of the module docstring."""
    for i, p in enumerate(CENSUS):
        img, pred = fb.imgs[p], fb.preds[p]
        n, h, w, _ = pred.shape
        np.testing.assert_array_equal(fb.grey[p], twin.grey(img))
        wp = twin.warp_pass(img, pred, fb.st.scales[p])
        near = lambda v, bound: np.abs(v.astype(np.float64) - bound) <= np.spacing(np.float32(max(bound, 1.0)))
        band = near(wp["X"], 0.0) | near(wp["X"], w - 1.0) | near(wp["Y"], 0.0) | near(wp["Y"], h - 1.0)
        assert not band.any()
        np.testing.assert_array_equal(fb.valid[p], wp["V"].astype(np.float32))
        assert wp["V"].any() and wp["G"].max() <= 255.0
        for k, name, sum_w in ((0, "W", 1.0), (1, "DX", 2.0), (2, "DY", 2.0)):
            err = np.abs(fb.warp[p][k] - wp[name]).max()
            print("%s %s %s: worst error %.3e, bound %.3e" % (fb.cfg, p, name, err, 8 * U * 255 * sum_w))
            assert err <= 8 * U * 255 * sum_w
            assert not fb.warp[p][k][~wp["V"]].any()
        mc = fb.masks[p] * fb.valid[p] * twin.interior(h, w)[None]
        assert fb.census_counts[i] == mc.sum() >= 1
        assert np.all((fb.masks[p] == 0) | (fb.masks[p] == 1)) and fb.counts[len(SMALL) + i] == fb.masks[p].sum()


@pytest.mark.gpu
def test_gradient_buffers_distance_and_loss_equal_the_twins(fb):
    """(2) and (3): the census scales against census_twin fed the device's G, W, DX, DY, V and masks, the small scales
    against photometric_twin fed the device's frames, predictions and masks; loss_dev is the sum of both."""
    tr, want_loss = fb.tr, 0.0
    for p in CENSUS:
        L, g, parts = twin.loss_and_grad_from_warp(fb.grey[p], fb.warp[p][0], fb.warp[p][1], fb.warp[p][2], fb.valid[p],
                                                   fb.masks[p], fb.st.scales[p], tr.loss_terms[p], 0.4, tr.loss_scale)
        want_loss += L
        got_S, got_c, got = fb.coef[p][0], fb.coef[p][1], fb.snap["g"][p]
        s_err = np.abs(got_S - parts["S"]).max() / np.abs(parts["S"]).max()
        c_err = np.abs(got_c - parts["c"]).max() / np.abs(parts["c"]).max()
        g_err = np.abs(got - g).max() / np.abs(g).max()
        print("%s %s: Mc = %d, L = %.6g, worst S error %.3e, c %.3e, gradient %.3e of the largest"
              % (fb.cfg, p, parts["Mc"], L, s_err, c_err, g_err))
        assert parts["Mc"] >= 1 and s_err <= GRAD_TOL and g_err <= GRAD_TOL
        assert not got[fb.valid[p] == 0].any() and np.isfinite(got).all()
    for p in SMALL:
        m = fb.masks[p]
        L, g, _ = ptwin.loss_and_grad(fb.imgs[p], fb.preds[p], m, fb.st.scales[p], tr.loss_terms[p], 0.4, tr.loss_scale)
        want_loss += L
        got = fb.snap["g"][p]
        if not m.any():
            assert not got.any()
            continue
        assert np.abs(got - g).max() <= GRAD_TOL * np.abs(g).max() and not got[m == 0].any()
    assert any(fb.masks[p].any() for p in SMALL)
    print("%s: loss %.9g, twins %.9g" % (fb.cfg, fb.snap["loss"], want_loss))
    assert want_loss > 0 and abs(fb.snap["loss"] - want_loss) <= LOSS_TOL * want_loss
    assert fb.loss == fb.snap["loss"]                              # backward leaves the scalar alone
    assert np.isfinite(fb.arena).all() and np.abs(fb.arena).max() > 0


# ------------------------------------------------------------------------------------------------ the launch list
@pytest.mark.gpu
@pytest.mark.parametrize("kw,kind,want", [
    (dict(data_term="census"), "census", CENSUS_CALLS),
    (dict(data_term="census", smoothness_weight=0.5), "census", CENSUS_CALLS + ["fn2_smoothness_loss_grad"]),
    (dict(), "photometric", PHOTOMETRIC_CALLS),
    (dict(data_term="photometric", smoothness_weight=0.5), "photometric", PHOTOMETRIC_CALLS + ["fn2_smoothness_loss_grad"]),
], ids=["census", "census+smoothness", "default", "photometric+smoothness"])
def test_eager_and_captured_steps_issue_the_same_loss_launches(kw, kind, want):
    import torch
    from src import weights as Wt
    from src.trainer import FlowNetSTrainer
    from test_gpu_loss_stages import Recorder, stage_pointers
    tr = FlowNetSTrainer(Wt.init_weights("FlowNetS", 9), N, H, W, dtype="f32", unsupervised=True, **kw)
    with graph_env("1"):
        tr.train_step_unsupervised(*frames(1, H, W, 4))
    assert getattr(tr, "_step_graphs", None) is not None and tr._captured.kind == kind and len(tr._seg_ends) == 1
    rec = tr.lib = Recorder(tr.lib)
    try:
        tr._segment_body(0)
        segment = rec.take()
        tr.forward_backward_unsupervised(*frames(1, H, W, 4))
        eager = rec.take()
        before = stage_pointers(tr._stage)
        tr.forward_backward_unsupervised(*frames(1, H, W, 40))
        second = rec.take()
    finally:
        tr.lib = rec._lib
    torch.cuda.synchronize()
    print("%s: %s" % (kw, eager))
    assert tr._stage is tr._captured and tr._stage.kind == kind
    for calls in (segment, eager, second):
        zeroing = len(calls) - len(want)
        assert zeroing >= 2 + (kind == "census") and calls[:zeroing] == zeroing * ["fn2_fill_zero"]
        assert calls[zeroing:] == want
    assert segment == eager == second
    assert stage_pointers(tr._stage) == before                     # the second step allocated nothing in the stage
    assert np.isfinite(float(tr.loss_dev.item()))


# ------------------------------------------------------------------------------------------------ one training step
@pytest.fixture(scope="module", params=["f32", "f16x2"])
def steps(request):
    """Two captured steps (other frames in the second), segment 0 of the captured step replayed twice behind them, and
    one eager step from the same weights."""
    import torch
    from src import _hip, weights as Wt
    from src.flownet_s.train import unpack_weights
    from src.trainer import FlowNetSTrainer
    wts = Wt.init_weights("FlowNetS", 1234)
    make = lambda: FlowNetSTrainer(wts, N, H, W, dtype=request.param, model="FlowNetS", unsupervised=True, data_term="census")
    b1, b2 = frames(1, H, W, 7), frames(1, H, W, 70)
    with graph_env("1"):
        tr = make()
        w0 = unpack_weights(tr)
        loss1 = float(tr.train_step_unsupervised(*b1).item())
        captured = getattr(tr, "_step_graphs", None) is not None
        g1 = tr.grad_arena.cpu().numpy().copy()
        w1 = unpack_weights(tr)
        loss2 = float(tr.train_step_unsupervised(*b2).item())
        replays = []
        for _ in range(2):                                         # forward, loss and backward only: the weights stay
            _hip.check(tr.lib.fn2_graph_launch(tr._step_graphs[0], _hip.stream_ptr()))
            torch.cuda.synchronize()
            st = tr._census
            replays.append(dict(loss=float(tr.loss_dev.item()), arena=tr.grad_arena.cpu().numpy().copy(),
                                stage={(k, p): v.cpu().numpy().copy() for k in ("grey", "warp", "valid", "coef", "masks")
                                       for p, v in getattr(st, k).items()},
                                counts=st.census_counts.cpu().numpy().copy()))
    with graph_env("0"):
        eager = make()
        eager_loss = float(eager.train_step_unsupervised(*b1).item())
        eager_captured = getattr(eager, "_step_graphs", None) is not None
        torch.cuda.synchronize()
        eager_g = eager.grad_arena.cpu().numpy().copy()
    return types.SimpleNamespace(tr=tr, w0=w0, w1=w1, g1=g1, loss1=loss1, loss2=loss2, captured=captured, replays=replays,
                                 eager_loss=eager_loss, eager_captured=eager_captured, eager_g=eager_g, dtype=request.param)


@pytest.mark.gpu
def test_captured_step_trains_matches_the_eager_sequence_and_replays_alike(steps):
    assert steps.captured and not steps.eager_captured and steps.tr.step_count == 2 and steps.tr._captured.kind == "census"
    trained = [k for k in steps.w0 if k.startswith("FlowNetS/")]
    assert trained
    for k in trained:
        assert np.isfinite(steps.w1[k]).all() and not np.array_equal(steps.w1[k], steps.w0[k]), k
    print("%s: captured loss %.9g, eager %.9g, second step %.9g, replays %.9g %.9g"
          % (steps.dtype, steps.loss1, steps.eager_loss, steps.loss2, steps.replays[0]["loss"], steps.replays[1]["loss"]))
    assert np.isfinite(steps.loss1) and steps.loss1 > 0
    assert abs(steps.loss1 - steps.eager_loss) <= STEP_TOL * abs(steps.eager_loss)
    assert np.abs(steps.g1 - steps.eager_g).max() <= STEP_TOL * np.abs(steps.eager_g).max()
    assert np.isfinite(steps.loss2) and steps.loss2 != steps.loss1   # the replay reads this step's frames
    r1, r2 = steps.replays
    for key in r1["stage"]:                                        # the loss stage is deterministic: plain stores
        np.testing.assert_array_equal(r1["stage"][key], r2["stage"][key], err_msg=str(key))
    np.testing.assert_array_equal(r1["counts"], r2["counts"])      # ... and its counters were zeroed in between
    assert r1["counts"].max() >= 1                                 # (the 8 x 16 scale has 40 interior pixels: all may be occluded)
    assert abs(r1["loss"] - r2["loss"]) <= LOSS_TOL * abs(r1["loss"])
    assert np.abs(r1["arena"] - r2["arena"]).max() <= STEP_TOL * np.abs(r1["arena"]).max()


@pytest.mark.gpu
def test_cli_trains_with_the_census_term(tmp_path):
    from src import weights as Wt
    lst = tmp_path / "pairs.txt"
    lst.write_text("%s %s\n" % (os.path.join(SAMPLES, "0img0.ppm"), os.path.join(SAMPLES, "0img1.ppm")))
    out = tmp_path / "ck"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT, os.environ.get("PYTHONPATH", "")]))
    res = subprocess.run([sys.executable, "-m", "src.flownet_s.train", "--unsupervised", "--no-augment", "--data_term",
                          "census", "--steps", "2", "--batch", "2", "--list", str(lst), "--out", str(out), "--log-every", "1"],
                         cwd=PKG, env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0
    assert "global step      2" in res.stdout
    ck = Wt.load_weights(str(out / "flownet_s-2.npz"))
    assert "FlowNetS/conv1/weights" in ck and all(np.isfinite(np.asarray(v)).all() for v in ck.values())


@pytest.mark.gpu
def test_errors(tmp_path):
    from src.flownet_s import train as cli
    from src.trainer import FlowNetSTrainer
    for kw in (dict(unsupervised=True, data_term="ssim"), dict(data_term="census"), dict(data_term="census", sparse_gt=True),
               dict(unsupervised=True, data_term="census", batch=3),
               dict(unsupervised=True, data_term="census", add_hard_flow_mining="hard")):
        with pytest.raises(ValueError):
            FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128), **kw))
    flags = cli.build_parser().parse_args(["--list", "l.txt", "--out", str(tmp_path), "--data_term", "census"])
    with pytest.raises(ValueError, match="needs --unsupervised"):
        cli.main(flags)
    flags = cli.build_parser().parse_args(["--list", "l.txt", "--out", str(tmp_path), "--unsupervised", "--data_term", "census"])
    with pytest.raises(ValueError, match="--no-augment"):
        cli.main(flags)
