"""The edge-aware smoothness term op by op (csrc/smoothness.hip, src/smoothness.py) against its float64 twin
(smoothness_twin.py).

Inputs, after the exact-arithmetic method of test_gpu_photometric.py: the flows f = scale * pred are multiples of 1/2 with
|component| <= 5 (for scale 5 and 0.625 multiples of 2.5, so that the product is exact), so every first and second difference
D is exact in fp32; the frames are multiples of 1/8 in [0, 1], so every frame difference is exact.  What is left to rounding is
expf, sqrtf, the division and the sums: the loss is held to rel 1e-5 and the gradient to 2e-5 of the largest per level, the
project's bars (DESIGN sections 5, 9 and 15).  The loss has no discontinuity, so no pixel is left out.  Because D is a multiple of
1/2, eps = 1e-3 alone would leave rho' at 0 or +-1 to six digits; every comparison also runs with eps = 3/4 (eps^2 exact),
where rho' takes values all over (-1, 1).

Columns 1 and 2 of every frame repeat column 0, so each order has x terms whose weight is exactly 1; with edge_lambda = 40 the
other weights go down to exp(-40): the span (1e-3, 1] is asserted on the twin's weights."""
import functools

import numpy as np
import pytest

import smoothness_twin as twin

SHAPES = [(2, 2, 2),      # one term per row and column (order 1); none at all for order 2
          (2, 3, 3),      # the smallest with a second-order term on both axes
          (2, 2, 9),      # order 2 has no y term
          (2, 5, 7),      # general small case
          (2, 3, 70),     # crosses a wave's 64-pixel segment
          (4, 6, 130),    # two segments plus a tail, more than one block
          (3, 4, 5)]      # odd n
DEGENERATE = [(2, 1, 1), (2, 1, 9), (2, 9, 1)]                     # min(h, w) == 1: loss 0, gradient 0
SCALES = [1.0, 0.625, 5.0]
GRAD_MULTS = [1.0, 16384.0]
ORDERS = [1, 2]
LAMBDAS = [0.0, 40.0]
EPSILONS = [1e-3, 0.75]
GRAD_TOL, LOSS_TOL = 2e-5, 1e-5
WEIGHT, SMOOTH_WEIGHT = 0.064, 1.5


# ------------------------------------------------------------------------------------------------ inputs
def case(seed, shape, scale=1.0):
    """(pred [n,h,w,2], img [n,h,w,3]) float32; f = scale * pred exactly, multiples of 1/2 (2.5), |f| <= 5."""
    n, h, w = shape
    rng = np.random.default_rng([seed, n, h, w])
    step = 0.5 if scale == 1.0 else 2.5
    f = (rng.integers(-int(5 / step), int(5 / step) + 1, size=(n, h, w, 2)) * step).astype(np.float32)
    pred = (f / np.float32(scale)).astype(np.float32)
    assert np.array_equal(np.float32(scale) * pred, f)
    img = (rng.integers(0, 9, size=(n, h, w, 3)) / 8.0).astype(np.float32)
    img[:, :, 1:3] = img[:, :, 0:1]                                # x terms of weight exactly 1, for either order
    return pred, img


@functools.lru_cache(maxsize=None)
def reference(seed, shape, scale, order, edge_lambda, eps, grad_mult, weight=WEIGHT, smooth_weight=SMOOTH_WEIGHT):
    """The twin on case(seed, shape, scale), computed once: (pred, img, L, dpred)."""
    pred, img = case(seed, shape, scale)
    L, g = twin.loss_and_grad(img, pred, scale, weight, order, edge_lambda, eps, smooth_weight, grad_mult)
    return pred, img, L, g


def weight_span(img, order, edge_lambda):
    """(smallest, largest) edge weight of the level, None where it has no term."""
    g = [v.ravel() for v in twin.weights(img, order, edge_lambda).values()]
    return (float(np.concatenate(g).min()), float(np.concatenate(g).max())) if g else None


def span_ok(shape, order, edge_lambda):
    """edge_lambda 0: every weight exactly 1.  Else the weights span at least (1e-3, 1] -- on every shape with more than a
    handful of terms ((2, 2, 2) has 8 for order 1 and none for order 2; (2, 3, 3) has 6 per axis for order 2)."""
    span = weight_span(case(0, shape)[1], order, edge_lambda)
    if span is None:
        return shape == (2, 2, 2) and order == 2
    if edge_lambda == 0.0:
        return span == (1.0, 1.0)
    return span[1] == 1.0 and (span[0] <= 1e-3 or shape in ((2, 2, 2), (2, 3, 3)))


def poisoned_case(shape, order):
    """case() with NaN, +-inf and +-1e30 in a few flow components (three of them on a small level).  `far` [n,h,w]: the pixels farther than `order` (in rows or
    columns, whichever is larger) from every poisoned pixel of their image: none of their terms reads a poisoned flow."""
    n, h, w = shape
    pred, img = case(21, shape)
    clean, pred = pred, pred.copy()
    rng = np.random.default_rng(22)
    far = np.ones((n, h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for k, v in enumerate([np.nan, np.inf, -1e30, -np.inf, 1e30, np.nan][:6 if h * w > 100 else 3]):
        i, y, x = rng.integers(n), rng.integers(h), rng.integers(w)
        pred[i, y, x, k % 2] = v
        far[i] &= np.maximum(np.abs(yy - y), np.abs(xx - x)) > order
    assert far.mean() > 0.3 and not far.all()
    return clean, pred, img, far


# ------------------------------------------------------------------------------------------------ device helpers
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def launch(levels, order, edge_lambda, eps, smooth_weight, grad_mult, accumulate=0, groups=None):
    """levels: [(pred, img, dpred start value or None, scale, weight)] host arrays -> (rc, loss, [dpred]); `groups`: lists of
    level indices, one launch each (default: one launch for all).  mask and mask_sum stay null: the entry point ignores them."""
    import torch
    from src import _hip
    lib = _hip.lib()
    n = levels[0][0].shape[0]
    bufs = []
    for pred, img, start, scale, weight in levels:
        d = torch.full(pred.shape, -7.0, device="cuda") if start is None else dev(start.astype(np.float32))
        bufs.append((dev(pred), dev(img), d))
    loss = torch.zeros(1, device="cuda")
    rc = 0
    for grp in groups or [list(range(len(levels)))]:
        table = (_hip.Fn2PhotometricLevel * len(grp))(*[
            _hip.Fn2PhotometricLevel(bufs[i][0].data_ptr(), bufs[i][1].data_ptr(), None, None, bufs[i][2].data_ptr(),
                                     levels[i][0].shape[1], levels[i][0].shape[2], levels[i][3], levels[i][4]) for i in grp])
        rc = rc or lib.fn2_smoothness_loss_grad(table, len(grp), n, order, edge_lambda, eps, smooth_weight, grad_mult,
                                                accumulate, _hip.ptr(loss), _hip.stream_ptr())
    return rc, float(host(loss)[0]), [host(b[2]) for b in bufs]


def check_loss_and_grad(got_loss, got_g, L, g, what=""):
    if not g.any() and L == 0.0:
        assert got_loss == 0.0 and not got_g.any()                 # exactly
        return
    err = np.abs(got_g - g).max() / np.abs(g).max()
    print("%s loss %.9g, twin %.9g; worst gradient error %.3e of the largest" % (what, got_loss, L, err))
    assert abs(got_loss - L) <= LOSS_TOL * abs(L), (got_loss, L)
    assert err <= GRAD_TOL


# ------------------------------------------------------------------------------------------------ 1. loss and gradient
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", SHAPES + DEGENERATE)
def test_loss_and_gradient_match_the_twin(shape, order, scale):
    """Through the wrapper, for both lambdas, both eps and both gradient multipliers."""
    from src.smoothness import smoothness_loss
    for edge_lambda in LAMBDAS:
        assert shape in DEGENERATE or span_ok(shape, order, edge_lambda)
        for eps in EPSILONS:
            for grad_mult in GRAD_MULTS:
                pred, img, L, g = reference(0, shape, scale, order, edge_lambda, eps, grad_mult)
                loss, dpred = smoothness_loss(dev(img), dev(pred), scale=scale, weight=WEIGHT, order=order,
                                              edge_lambda=edge_lambda, eps=eps, smooth_weight=SMOOTH_WEIGHT,
                                              grad_mult=grad_mult)
                if shape in DEGENERATE or (shape == (2, 2, 2) and order == 2):
                    assert L == 0.0 and not g.any()
                check_loss_and_grad(float(host(loss)[0]), host(dpred), L, g,
                                    "%s order %d lambda %g eps %g x%g:" % (shape, order, edge_lambda, eps, grad_mult))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 6, 130), (2, 2, 9), (2, 1, 9)])
def test_accumulate_adds_onto_what_dpred_holds_and_runs_repeat_bitwise(shape, order):
    """accumulate = 1 onto a random dpred is that dpred plus the accumulate = 0 result, to 1 ulp of the sum (the product and
    the sum may contract into one fma); two accumulate = 0 runs agree bit for bit."""
    pred, img = case(5, shape, 0.625)
    start = np.random.default_rng(6).standard_normal(pred.shape).astype(np.float32)
    lv = lambda s: [(pred, img, s, 0.625, WEIGHT)]
    rc0, loss0, (g0,) = launch(lv(None), order, 20.0, 0.75, SMOOTH_WEIGHT, 3.0)
    rc1, loss1, (g1,) = launch(lv(None), order, 20.0, 0.75, SMOOTH_WEIGHT, 3.0)
    rc2, loss2, (acc,) = launch(lv(start), order, 20.0, 0.75, SMOOTH_WEIGHT, 3.0, accumulate=1)
    assert rc0 == rc1 == rc2 == 0
    np.testing.assert_array_equal(g0, g1)
    assert abs(loss0 - loss1) <= 1e-6 * abs(loss0) and abs(loss0 - loss2) <= 1e-6 * abs(loss0)
    want = start + g0
    assert np.all(np.abs(acc.astype(np.float64) - (start.astype(np.float64) + g0)) <= np.spacing(np.abs(want)))
    if min(shape[1:]) == 1:
        np.testing.assert_array_equal(acc, start)                  # gradient 0: nothing is added
        assert loss0 == 0.0 and not g0.any()
    else:
        assert g0.any() and not np.array_equal(acc, start)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
def test_five_levels_in_one_launch_equal_five_launches(order):
    """One table of five levels (different sizes, scales and weights) against the same levels one launch each: gradients bit
    for bit (nothing in a pixel depends on the table), the loss to rel 1e-6 (atomics in another order) -- and the twin."""
    shapes = [(4, 6, 130), (4, 3, 70), (4, 5, 7), (4, 2, 3), (4, 1, 2)]
    scales, weights = [5.0, 1.0, 0.625, 1.0, 5.0], [0.064, 0.016, 0.004, 0.002, 0.001]
    refs = [reference(3, shp, s, order, 20.0, 0.75, 16384.0, wgt) for shp, s, wgt in zip(shapes, scales, weights)]
    levels = [(r[0], r[1], None, s, wgt) for r, s, wgt in zip(refs, scales, weights)]
    rc1, one_loss, one = launch(levels, order, 20.0, 0.75, SMOOTH_WEIGHT, 16384.0)
    rc5, five_loss, five = launch(levels, order, 20.0, 0.75, SMOOTH_WEIGHT, 16384.0, groups=[[i] for i in range(5)])
    assert rc1 == rc5 == 0
    want_loss = sum(r[2] for r in refs)
    assert abs(one_loss - five_loss) <= 1e-6 * abs(five_loss) and abs(one_loss - want_loss) <= LOSS_TOL * abs(want_loss)
    for g1, g5, r in zip(one, five, refs):
        np.testing.assert_array_equal(g1, g5)
        if r[3].any():
            assert np.abs(g1 - r[3]).max() <= GRAD_TOL * np.abs(r[3]).max()
        else:
            assert not g1.any()


@pytest.mark.gpu
@pytest.mark.parametrize("order,edge_lambda", [(1, 0.0), (1, 20.0), (1, 150.0), (2, 0.0)])
@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 6, 130)])
def test_constant_flow_has_gradient_zero_and_the_loss_of_eps(shape, order, edge_lambda):
    """Every D is exactly 0, so rho' = 0 and the gradient is exactly 0, and rho = eps in every term:
        L = weight * smooth_weight * 0.5 * (2 eps mean(gx) + 2 eps mean(gy)) = weight * smooth_weight * eps * (mean gx + mean gy)
    -- the sum over the two flow components is not averaged in the definition, so with all weights 1 (edge_lambda 0) the loss
    is 2 * weight * smooth_weight * eps, and with edge_lambda > 0 the frames' mean weights enter.  (The issue that asked for
    this test wrote the expected value as weight * smooth_weight * eps; that is the definition's value with ONE axis
    present, and contradicts it with both.  The definition is what the twin, the hand-worked cases and autograd pin.)"""
    pred, img = case(9, shape)
    pred = np.broadcast_to(np.float32([1.7, -0.3]), pred.shape).copy()
    for eps in EPSILONS:
        rc, loss, (g,) = launch([(pred, img, None, 0.625, WEIGHT)], order, edge_lambda, eps, SMOOTH_WEIGHT, 16384.0)
        mean_g = sum(float(v.mean()) for v in twin.weights(img, order, edge_lambda).values())
        want = float(np.float32(WEIGHT)) * SMOOTH_WEIGHT * float(np.float32(eps)) * mean_g   # (the fp32 arguments)
        if edge_lambda == 0.0:
            assert mean_g == 2.0
        print("constant flow %s order %d lambda %g eps %g: loss %.9g, want %.9g" % (shape, order, edge_lambda, eps, loss, want))
        assert rc == 0 and not g.any()
        assert abs(loss - want) <= 1e-6 * want


@pytest.mark.gpu
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 6, 130)])
def test_poisoned_predictions_move_no_load(shape, order):
    """NaN, +-inf and +-1e30 in a few flow components: no address depends on the data, so the call returns 0, the inputs and
    the guard words behind dpred are untouched, and every pixel farther than `order` from a poisoned one holds what the clean
    run stores, bit for bit."""
    import torch
    from src import _hip
    clean, pred, img, far = poisoned_case(shape, order)
    n, h, w = shape
    npix, guard = n * h * w, 64
    out = []
    for p in (clean, pred):
        d_pred, d_img = dev(p), dev(img)
        g = torch.full((2 * npix + guard,), -7.0, device="cuda")
        loss = torch.zeros(1, device="cuda")
        table = (_hip.Fn2PhotometricLevel * 1)(_hip.Fn2PhotometricLevel(d_pred.data_ptr(), d_img.data_ptr(), None, None,
                                                                        g.data_ptr(), h, w, 1.0, 1.0))
        rc = _hip.lib().fn2_smoothness_loss_grad(table, 1, n, order, 20.0, 0.75, 1.0, 1.0, 0, _hip.ptr(loss),
                                                 _hip.stream_ptr())
        assert rc == 0
        got = host(g)
        assert np.all(got[2 * npix:] == -7.0)
        np.testing.assert_array_equal(host(d_pred), p)             # inputs are only read (NaN == NaN here)
        np.testing.assert_array_equal(host(d_img), img)
        out.append(got[:2 * npix].reshape(n, h, w, 2))
    assert np.isfinite(out[0]).all()
    np.testing.assert_array_equal(out[1][far], out[0][far])
    assert not np.array_equal(out[1], out[0], equal_nan=True)      # ... and the poison did reach its neighbourhood


# ------------------------------------------------------------------------------------------------ 2. arguments
def check_invalid_arguments(hip):
    """Every check sits in front of the launch: the pointers are never followed."""
    lib = hip.lib()
    L = hip.Fn2PhotometricLevel
    fake = 0x1000
    ok = lambda **kw: L(**dict(dict(pred=fake, img=fake, mask=None, mask_sum=None, dpred=fake, h=4, w=5, scale=1.0,
                                    weight=1.0), **kw))
    base = dict(nl=1, n=2, order=1, lam=150.0, eps=1e-3, sw=1.0, acc=0, loss=fake)

    def call(table, **kw):
        a = dict(base, **kw)
        return lib.fn2_smoothness_loss_grad(table, a["nl"], a["n"], a["order"], a["lam"], a["eps"], a["sw"], 1.0, a["acc"],
                                            a["loss"], None)

    nan, inf = float("nan"), float("inf")
    cases = [(None, {}, b"null level table"), (ok(), dict(nl=0), b"n_levels"),
             ((L * 9)(*[ok() for _ in range(9)]), dict(nl=9), b"n_levels"), (ok(), dict(n=0), b"n must"),
             (ok(), dict(n=-2), b"n must"), (ok(h=0), {}, b"bad size"), (ok(w=0), {}, b"bad size"), (ok(w=-2), {}, b"bad size"),
             (ok(h=1 << 16, w=(1 << 14) + 1), {}, b"too large"), (ok(pred=0x1004), {}, b"aligned"),
             (ok(dpred=0x1004), {}, b"aligned"), ((L * 3)(ok(), ok(), ok(img=None)), dict(nl=3), b"level 2"),
             (ok(pred=None), {}, b"null pointer"), (ok(img=None), {}, b"null pointer"), (ok(dpred=None), {}, b"null pointer"),
             (ok(), dict(loss=None), b"loss_accum"), (ok(), dict(order=0), b"order"), (ok(), dict(order=3), b"order"),
             (ok(), dict(lam=-1.0), b"edge_lambda"), (ok(), dict(lam=nan), b"edge_lambda"), (ok(), dict(lam=inf), b"edge_lambda"),
             (ok(), dict(eps=0.0), b"eps"), (ok(), dict(eps=-1e-3), b"eps"), (ok(), dict(eps=nan), b"eps"),
             (ok(), dict(sw=-1.0), b"smooth_weight"), (ok(), dict(sw=nan), b"smooth_weight"),
             (ok(), dict(acc=2), b"accumulate"), (ok(), dict(acc=-1), b"accumulate")]
    for table, kw, word in cases:
        rc = call(table, **kw)
        msg = lib.fn2_last_error()
        assert rc == hip.ERR_INVALID_ARGUMENT and word in msg and b"smoothness" in msg, (word, rc, msg)
    with pytest.raises(ValueError, match="smoothness"):
        hip.check(call(ok(), order=3))


@pytest.mark.gpu
def test_invalid_arguments_launch_nothing_on_the_device_box():
    """The error code comes back and dpred and the loss keep what they held."""
    import torch
    from src import _hip
    from src.smoothness import smoothness_loss
    check_invalid_arguments(_hip)
    pred, img = case(0, (3, 4, 5))                                  # (odd n is fine here)
    for kw in (dict(order=3), dict(eps=0.0), dict(edge_lambda=-1.0), dict(smooth_weight=float("nan")), dict(accumulate=2)):
        a = dict(dict(order=1, edge_lambda=150.0, eps=1e-3, smooth_weight=1.0, accumulate=0), **kw)
        rc, loss, (g,) = launch([(pred, img, None, 1.0, 1.0)], a["order"], a["edge_lambda"], a["eps"], a["smooth_weight"], 1.0,
                                a["accumulate"])
        assert rc == _hip.ERR_INVALID_ARGUMENT and loss == 0.0 and np.all(g == -7.0)
    d_img, d_pred = dev(img), dev(pred)
    for bad_img, bad_pred in ((d_img[0], d_pred[0]), (d_img, d_pred[:, :3]), (d_img[..., :2], d_pred), (d_img, d_img),
                              (d_img.cpu(), d_pred.cpu())):
        with pytest.raises(ValueError):
            smoothness_loss(bad_img, bad_pred)
    for kw in (dict(order=3), dict(eps=0.0), dict(edge_lambda=-1.0), dict(smooth_weight=-1.0)):
        with pytest.raises(ValueError):
            smoothness_loss(d_img, d_pred, **kw)
    assert torch.cuda.is_available()
