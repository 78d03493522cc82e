"""The edge-aware smoothness term and the pair-consistent augmentation without a GPU: the float64 twin checked against torch
autograd of its own forward and against cases worked by hand, the preconditions of the GPU tests, the exported symbol, and
every argument check of the library, the wrapper, the trainer, the loader and the CLI that has to come before any device use."""
import inspect
import math
import os

import numpy as np
import pytest

import smoothness_twin as twin
from test_gpu_smoothness import (DEGENERATE, LAMBDAS, ORDERS, SHAPES, case, check_invalid_arguments, poisoned_case, span_ok,
                                 weight_span)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape,scale", [((2, 5, 7), 1.0), ((3, 4, 9), 0.625), ((2, 3, 70), 5.0), ((2, 2, 9), 1.0)])
def test_twin_gradient_is_autograd_of_its_forward(shape, scale, order):
    """Random inputs (pred a multiple of 2^-10, so that scale * pred is exact in fp32 and the twin's one fp32 rounding
    changes nothing): dL/dpred by autograd against the analytic formula, and the two forwards."""
    import torch
    n, h, w = shape
    rng = np.random.default_rng(5)
    img = rng.random((n, h, w, 3))
    pred = (np.round(rng.standard_normal((n, h, w, 2)) * 1.2 / scale * 1024) / 1024).astype(np.float32)
    assert np.array_equal(twin.scaled(pred, scale), float(scale) * pred.astype(np.float64))
    kw = dict(scale=scale, weight=0.064, order=order, edge_lambda=4.0, eps=0.05, smooth_weight=1.5)
    L, g = twin.loss_and_grad(img, pred, grad_mult=3.0, **kw)
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    Lt = twin.torch_loss(img, p, **kw)
    Lt.backward()
    assert abs(float(Lt.detach()) - L) <= 1e-12 * abs(L)
    np.testing.assert_allclose(3.0 * p.grad.numpy(), g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    assert L > 0 and np.abs(g).min() > 0
    assert abs(g.sum()) <= 1e-9 * np.abs(g).sum()                  # a constant added to the flow changes nothing


def test_twin_order_1_on_a_case_worked_by_hand():
    """n 1, h 2, w 3; scale 2, so f = 2 pred.  f_u = [[0, 1, 3], [0, 0, 0]], f_v = 0.  Frame channel 0 = [[0, 0, .3], [0, .6, .3]],
    channels 1 and 2 zero; lambda 2, eps 0.5.  Cx = 1 * 2 * 2 = 4, Cy = 1 * 1 * 3 = 3.
      x terms  row 0: D_u = (1, 2), gx = (1, e^-.2);  row 1: D_u = (0, 0), gx = (e^-.4, e^-.2)      (mean over 3 channels: dI / 3)
      y terms  columns 0..2: D_u = (0, -1, -3), gy = (1, e^-.4, 1)
    D_v = 0 everywhere: rho = eps, rho' = 0."""
    lam, eps, wgt, sw, gm, s = 2.0, 0.5, 0.064, 1.5, 16384.0, 2.0
    pred = np.zeros((1, 2, 3, 2), np.float32)
    pred[0, 0, :, 0] = (0, 0.5, 1.5)
    img = np.zeros((1, 2, 3, 3))
    img[0, :, :, 0] = [[0, 0, .3], [0, .6, .3]]
    rho = lambda d: math.sqrt(d * d + eps * eps)
    drho = lambda d: d / rho(d)
    e2, e4 = math.exp(-.2), math.exp(-.4)
    Sx = (1 * (rho(1) + eps) + e2 * (rho(2) + eps)) + (e4 * 2 * eps + e2 * 2 * eps)
    Sy = 1 * 2 * eps + e4 * (rho(-1) + eps) + 1 * (rho(-3) + eps)
    L, g = twin.loss_and_grad(img, pred, s, wgt, 1, lam, eps, sw, gm)
    assert L == pytest.approx(wgt * sw * 0.5 * (Sx / 4 + Sy / 3), rel=1e-14)
    k = gm * wgt * sw * s
    want = np.zeros((1, 2, 3, 2))
    want[0, 0, 0, 0] = k * ((0.5 / 4) * (-1 * drho(1)) + (0.5 / 3) * (-1 * drho(0)))
    want[0, 0, 1, 0] = k * ((0.5 / 4) * (1 * drho(1) - e2 * drho(2)) + (0.5 / 3) * (-e4 * drho(-1)))
    want[0, 0, 2, 0] = k * ((0.5 / 4) * (e2 * drho(2)) + (0.5 / 3) * (-1 * drho(-3)))
    want[0, 1, 0, 0] = 0.0
    want[0, 1, 1, 0] = k * ((0.5 / 3) * (e4 * drho(-1)))
    want[0, 1, 2, 0] = k * ((0.5 / 3) * (1 * drho(-3)))
    np.testing.assert_allclose(g, want, rtol=1e-13, atol=0)
    assert not g[..., 1].any()


def test_twin_order_2_on_a_case_worked_by_hand():
    """The same level, order 2: h = 2 holds no y term; one x term per row, on x = 1, Cx = 1 * 2 * 1 = 2.
      row 0: D_u = 0 - 2 * 1 + 3 = 1, gx = exp(-2 * (|.3 - 0| / 2) / 3) = e^-.1;  row 1: D_u = 0, gx = e^-.1."""
    lam, eps, wgt, sw, gm, s = 2.0, 0.5, 0.064, 1.5, 16384.0, 2.0
    pred = np.zeros((1, 2, 3, 2), np.float32)
    pred[0, 0, :, 0] = (0, 0.5, 1.5)
    img = np.zeros((1, 2, 3, 3))
    img[0, :, :, 0] = [[0, 0, .3], [0, .6, .3]]
    rho1 = math.sqrt(1 + eps * eps)
    e1 = math.exp(-.1)
    L, g = twin.loss_and_grad(img, pred, s, wgt, 2, lam, eps, sw, gm)
    assert L == pytest.approx(wgt * sw * 0.5 * ((e1 * (rho1 + eps) + e1 * 2 * eps) / 2), rel=1e-14)
    t = gm * wgt * sw * s * (0.5 / 2) * e1 * (1 / rho1)
    want = np.zeros((1, 2, 3, 2))
    want[0, 0, :, 0] = (t, -2 * t, t)
    np.testing.assert_allclose(g, want, rtol=1e-13, atol=0)
    # too short for a term on either axis, and 1-high / 1-wide levels: loss and gradient exactly 0
    for shape, order in (((2, 2, 2), 2), ((2, 1, 9), 1), ((2, 9, 1), 1), ((2, 1, 1), 2), ((2, 1, 9), 2)):
        L0, g0 = twin.loss_and_grad(np.ones(shape + (3,)), np.ones(shape + (2,), np.float32), order=order)
        assert L0 == 0.0 and not g0.any()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES + DEGENERATE)
def test_preconditions_of_the_gpu_op_tests_hold(shape, order):
    """The edge weights are exactly 1 for edge_lambda 0 and span (1e-3, 1] for the other value; every difference the kernel
    forms in fp32 is exact on these inputs."""
    for edge_lambda in LAMBDAS:
        assert shape in DEGENERATE or span_ok(shape, order, edge_lambda), weight_span(case(0, shape)[1], order, edge_lambda)
    for scale in (1.0, 0.625, 5.0):
        pred, img = case(0, shape, scale)
        f = twin.scaled(pred, scale)
        assert np.all(f * 2 == np.round(f * 2)) and np.abs(f).max() <= 5 and np.all(img * 8 == np.round(img * 8))
    if shape in ((2, 5, 7), (4, 6, 130)):
        poisoned_case(shape, order)


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


def test_entry_point_is_exported_declared_and_validates_without_a_device(hip):
    import ctypes as C
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    name = "fn2_smoothness_loss_grad"
    assert name in hip.PROTOTYPES and hasattr(lib, name) and ("int %s(" % name) in header
    res, args = hip.PROTOTYPES[name]
    assert res is C.c_int and len(args) == 11 and args[0] == C.POINTER(hip.Fn2PhotometricLevel)
    assert args[3] is C.c_int and args[4:8] == [C.c_float] * 4 and args[8] is C.c_int
    assert "ADDITION to the reference" in header
    check_invalid_arguments(hip)


# ------------------------------------------------------------------------------------------------ Python surface
def test_wrapper_rejects_bad_arguments_before_touching_a_device(monkeypatch):
    import torch
    from src import _hip, smoothness
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was asked for"))
    img, pred = torch.zeros(2, 4, 5, 3), torch.zeros(2, 4, 5, 2)
    with pytest.raises(ValueError, match="device tensor"):
        smoothness.smoothness_loss(img, pred)
    with pytest.raises(ValueError, match="device tensor"):
        smoothness.smoothness_loss(img.numpy(), pred.numpy())
    z = torch.zeros
    for i, p, word in ((z(4, 5, 3), z(4, 5, 2), "rank 4"), (z(2, 4, 5, 2), z(2, 4, 5, 2), "3 channels"),
                       (z(2, 4, 5, 3), z(2, 4, 5, 3), "2 channels"), (z(2, 4, 5, 3), z(2, 4, 6, 2), "same batch"),
                       (z(2, 0, 5, 3), z(2, 0, 5, 2), "empty")):
        with pytest.raises(ValueError, match=word):
            smoothness.smoothness_loss(i, p)
    good = dict(order=1, edge_lambda=150.0, eps=1e-3, smooth_weight=1.0)
    nan = float("nan")
    for bad in (dict(order=3), dict(order=0), dict(order=nan), dict(eps=0.0), dict(eps=-1e-3), dict(eps=nan),
                dict(edge_lambda=-1.0), dict(edge_lambda=nan), dict(edge_lambda=float("inf")), dict(smooth_weight=-0.5),
                dict(smooth_weight=nan)):
        with pytest.raises(ValueError):
            smoothness.check_constants(**dict(good, **bad))
    assert smoothness.check_constants(2, 0, 0.5, 0) == (2, 0.0, 0.5, 0.0)
    assert smoothness.check_constants(**good) == (1, 150.0, 1e-3, 1.0)


def test_trainer_arguments_are_checked_before_the_engine_is_built(monkeypatch):
    from src import trainer
    monkeypatch.setattr(trainer, "Engine", lambda *a, **k: pytest.fail("the engine was asked for"))
    make = lambda **kw: trainer.FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128), **kw))
    with pytest.raises(ValueError, match="unsupervised=True"):
        make(smoothness_weight=0.5)                                # a supervised trainer has no loss to regularise
    for kw, word in ((dict(smoothness_order=3), "order"), (dict(smoothness_weight=-1.0), "weight"),
                     (dict(smoothness_weight=float("nan")), "weight"), (dict(edge_lambda=-2.0), "edge_lambda"),
                     (dict(smoothness_eps=0.0), "eps")):
        with pytest.raises(ValueError, match=word):
            make(**dict(dict(unsupervised=True, smoothness_weight=1.0), **kw))
    sig = inspect.signature(trainer.FlowNetSTrainer.__init__).parameters
    assert (sig["smoothness_weight"].default, sig["smoothness_order"].default, sig["edge_lambda"].default,
            sig["smoothness_eps"].default) == (0.0, 1, 150.0, 1e-3)


@pytest.mark.parametrize("model", ["flownet_s", "flownet_sd", "flownet_c", "flownet_cs", "flownet_css"])
def test_cli_flags_and_their_checks(model, tmp_path):
    import importlib
    from src.flownet_s import train as cli
    mod = importlib.import_module("src.%s.train" % model)
    assert mod.parse_and_run is cli.parse_and_run                  # one CLI for the five models
    base = ["--list", "l.txt", "--out", str(tmp_path)]
    flags = cli.build_parser().parse_args(base)
    assert (flags.smoothness_weight, flags.smoothness_order, flags.edge_lambda) == (0.0, 1, 150.0)
    assert cli.unsupervised_kwargs(flags) == {}
    flags = cli.build_parser().parse_args(base + ["--smoothness_weight", "2"])
    assert cli.unsupervised_kwargs(flags) == {}                    # without --unsupervised nothing is handed on
    on = base + ["--unsupervised", "--no-augment"]
    assert cli.unsupervised_kwargs(cli.build_parser().parse_args(on)) == dict(unsupervised=True, photometric_q=0.4,
                                                                             occ_alpha=0.01, occ_beta=0.5)
    flags = cli.build_parser().parse_args(on + ["--smoothness_weight", "2", "--smoothness_order", "2", "--edge_lambda", "10"])
    assert cli.unsupervised_kwargs(flags) == dict(unsupervised=True, photometric_q=0.4, occ_alpha=0.01, occ_beta=0.5,
                                                  smoothness_weight=2.0, smoothness_order=2, edge_lambda=10.0)
    for extra, word in ((["--smoothness_order", "3"], "order"), (["--smoothness_weight", "-1"], "weight"),
                        (["--smoothness_weight", "nan"], "weight"), (["--edge_lambda", "-5"], "edge_lambda"),
                        (["--edge_lambda", "inf"], "edge_lambda")):
        with pytest.raises(ValueError, match=word):
            cli.main(cli.build_parser().parse_args(on + extra))    # raised before torch or the device are touched
    assert not os.listdir(str(tmp_path))
    # --augmentation pair is the one augmentation --unsupervised takes; the others are refused as before
    flags = cli.build_parser().parse_args(base + ["--unsupervised", "--augmentation", "pair"])
    assert flags.augment is True and cli.unsupervised_kwargs(flags)["unsupervised"] is True
    for aug in ([], ["--augmentation", "plugin"], ["--augmentation", "selflow"]):
        with pytest.raises(ValueError, match="brightness constancy") as err:
            cli.main(cli.build_parser().parse_args(base + ["--unsupervised"] + aug))
        assert "--no-augment" in str(err.value)
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--augmentation", "nothing"])


# ------------------------------------------------------------------------------------------------ pair augmentation
@pytest.mark.parametrize("fast_mode", [False, True])
def test_shared_colour_tables_carry_one_record_for_both_frames(fast_mode):
    from src import data_augmentation as DA
    colour = [DA.COLOUR_ORDER, DA.D_BRIGHTNESS, DA.F_SATURATION, DA.D_HUE, DA.F_CONTRAST]
    a, b = DA.draw_estimation_params(np.random.default_rng(3), 64, fast_mode=fast_mode, shared_colour=True)
    np.testing.assert_array_equal(b[:, colour], a[:, colour])
    np.testing.assert_array_equal(a.view(np.float32)[:, DA.F_CONTRAST], np.float32(1.0))
    np.testing.assert_array_equal(b[:, [DA.FLIP_LR, DA.FLIP_UD, DA.PERM]], a[:, [DA.FLIP_LR, DA.FLIP_UD, DA.PERM]])
    np.testing.assert_array_equal(a, b)                            # nothing else is set in an estimation table
    orders = set(a.view(np.int32)[:, DA.COLOUR_ORDER].tolist())
    assert orders == ({0} if fast_mode else {0, 1, 2, 3})
    assert set(a[:, DA.FLIP_LR].tolist()) == {0, 1} and set(a[:, DA.FLIP_UD].tolist()) == {0, 1}
    assert set(a[:, DA.PERM].tolist()) == set(range(6))
    f = a.view(np.float32)
    for word, (lo, hi) in ((DA.D_BRIGHTNESS, DA.COLOUR_RANGES["d_brightness"]), (DA.F_SATURATION, DA.COLOUR_RANGES["f_saturation"]),
                           (DA.D_HUE, DA.COLOUR_RANGES["d_hue"])):
        assert np.all((f[:, word] >= np.float32(lo)) & (f[:, word] < np.float32(hi))) and len(set(f[:, word].tolist())) > 32


def test_independent_colour_draws_are_what_they_were():
    """shared_colour=False consumes the generator exactly as before the argument existed: the draws of the function restated
    here from its definition, and the generator's state behind them."""
    from src import data_augmentation as DA
    rng, ref = np.random.default_rng(11), np.random.default_rng(11)
    a, b = DA.draw_estimation_params(rng, 5)
    wa, wb = DA.empty_params(5), DA.empty_params(5)
    for ra, rb in zip(wa, wb):
        ra[DA.FLIP_LR], ra[DA.FLIP_UD] = ref.integers(0, 2, size=2)
        ra[DA.PERM] = ref.integers(6)
        rb[[DA.FLIP_LR, DA.FLIP_UD, DA.PERM]] = ra[[DA.FLIP_LR, DA.FLIP_UD, DA.PERM]]
        DA._draw_colour(ref, ra, False)
        DA._draw_colour(ref, rb, False)
    np.testing.assert_array_equal(a, wa)
    np.testing.assert_array_equal(b, wb)
    assert rng.integers(1 << 30) == ref.integers(1 << 30)
    assert not np.array_equal(a, b)
    a2, b2 = DA.draw_estimation_params(np.random.default_rng(11), 5, shared_colour=False)
    np.testing.assert_array_equal(a2, a)
    np.testing.assert_array_equal(b2, b)


def test_loader_takes_pair_on_unlabeled_lists_up_to_the_device(tmp_path, monkeypatch):
    """`pair` passes the argument checks with a two-field list and reaches the augmentation call with shared-colour tables,
    flow None; `plugin` and `selflow` are refused with the message they always had."""
    from src import data_augmentation as DA
    from src import dataloader
    samples = os.path.join(ROOT, "tests", "golden", "samples")
    two = tmp_path / "two.txt"
    two.write_text("%s %s\n" % (os.path.join(samples, "0img0.ppm"), os.path.join(samples, "0img1.ppm")))
    three = tmp_path / "three.txt"
    three.write_text("%s %s %s\n" % (os.path.join(samples, "0img0.ppm"), os.path.join(samples, "0img1.ppm"),
                                     os.path.join(samples, "0flow.flo")))
    for aug in ("plugin", "selflow"):
        with pytest.raises(ValueError, match="data_augmentation=False"):
            next(dataloader.load_batches(str(two), 1, allow_unlabeled=True, augmentation=aug))
    with pytest.raises(ValueError, match="'pair'"):
        next(dataloader.load_batches(str(two), 1, augmentation="both"))
    seen = []

    def stop(image1, image2, gt_flow, params=None, **kw):
        seen.append((image1, image2, gt_flow, params))
        raise RuntimeError("the device is next")

    monkeypatch.setattr(DA, "augment_all_estimation", stop)
    with pytest.raises(RuntimeError, match="the device is next"):
        next(dataloader.load_batches(str(two), 1, allow_unlabeled=True, augmentation="pair"))
    with pytest.raises(RuntimeError, match="the device is next"):
        next(dataloader.load_batches(str(three), 1, augmentation="pair"))
    (a, b, f, (ta, tb)), labeled = seen
    assert f is None and a.shape == b.shape and a.shape[0] == 1 and a.shape[3] == 3
    np.testing.assert_array_equal(ta, tb)
    assert ta.view(np.float32)[0, DA.F_CONTRAST] == 1.0
    assert labeled[2] is not None and labeled[2].shape == a.shape[:3] + (2,)
