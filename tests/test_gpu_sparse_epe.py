"""fn2_sparse_epe_count / fn2_sparse_epe_loss_grad op by op against the float64 twin (tests/sparse_epe_twin.py).

Inputs follow the method of the other loss tests: pred and label are multiples of 1/2 with |x| <= 8, so du, dv and
du^2 + dv^2 are exact in fp32 and only sqrtf, the division and the sums round.  The bars are the project's: the loss within
rel 1e-5, the gradients within 2e-5 of the largest per level; M and the zeros of dpred are exact.  Against the dense op the
coefficient is one double division against a float one (at most an ulp apart) and everything else is the same arithmetic:
gradients to 1e-6 of the largest, the loss to rel 1e-6."""
import ctypes as C

import numpy as np
import pytest

import sparse_epe_twin as twin

SHAPES = [(2, 1, 1), (2, 2, 3), (2, 5, 7), (3, 4, 5), (2, 3, 70), (4, 6, 130)]
PATTERNS = ["all", "none", "one", "half", "u_only", "v_only", "inf"]
WEIGHTS = [0.064, 0.0]
GRAD_MULTS = [1.0, 16384.0]
LOSS_REL, GRAD_REL, DENSE_REL = 1e-5, 2e-5, 1e-6


def case(seed, shape, pattern):
    """(pred, label) fp32 [n,h,w,2]: multiples of 1/2 in [-8, 8]; about a quarter of the valid pixels have pred == label.
    `pattern` picks the pixels without ground truth and how they are marked."""
    n, h, w = shape
    rng = np.random.default_rng([seed, n, h, w])
    pred = (rng.integers(-16, 17, size=(n, h, w, 2)) / 2.0).astype(np.float32)
    label = (rng.integers(-16, 17, size=(n, h, w, 2)) / 2.0).astype(np.float32)
    same = rng.random((n, h, w)) < 0.25
    label[same] = pred[same]
    nan, inf = np.float32("nan"), np.float32("inf")
    half = rng.random((n, h, w)) < 0.5
    if pattern == "none":
        label[...] = nan
    elif pattern == "one":
        keep = np.zeros(n * h * w, bool)
        keep[int(rng.integers(n * h * w))] = True
        label[~keep.reshape(n, h, w)] = nan
    elif pattern == "half":
        label[half] = nan
    elif pattern == "u_only":
        label[half, 0] = nan
    elif pattern == "v_only":
        label[half, 1] = nan
    elif pattern == "inf":
        label[half, 0] = np.where(rng.random(int(half.sum())) < 0.5, inf, -inf)
        other = rng.random((n, h, w)) < 0.25
        label[other, 1] = -inf
    else:
        assert pattern == "all"
    return pred, label


def launch(levels, grad_mult=1.0, one_by_one=False, loss_init=0.0, dpred_init=None):
    """levels: [(pred, label, weight)] host arrays of one batch size.  Runs count then loss_grad (one launch each for all
    levels, or level by level).  Returns ((rc_count, rc_loss), loss, [dpred], [M]) as host values."""
    import torch
    from src import _hip
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    n = levels[0][0].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    preds, labels = [up(l[0]) for l in levels], [up(l[1]) for l in levels]
    fill = float("nan") if dpred_init is None else dpred_init
    dpreds = [torch.full_like(p, fill) for p in preds]
    counts = torch.zeros(len(levels), dtype=torch.int32, device=dev)
    loss = torch.full((1,), loss_init, dtype=torch.float32, device=dev)
    recs = [_hip.Fn2SparseEpeLevel(p.data_ptr(), l.data_ptr(), d.data_ptr(), counts[i:i + 1].data_ptr(), p.shape[1],
                                   p.shape[2], float(lv[2]))
            for i, (p, l, d, lv) in enumerate(zip(preds, labels, dpreds, levels))]
    s = _hip.stream_ptr()
    groups = [[r] for r in recs] if one_by_one else [recs]
    rc_c = rc_l = 0
    for grp in groups:
        table = (_hip.Fn2SparseEpeLevel * len(grp))(*grp)
        rc_c = rc_c or lib.fn2_sparse_epe_count(table, len(grp), n, s)
    for grp in groups:
        table = (_hip.Fn2SparseEpeLevel * len(grp))(*grp)
        rc_l = rc_l or lib.fn2_sparse_epe_loss_grad(table, len(grp), n, float(grad_mult), _hip.ptr(loss), s)
    torch.cuda.synchronize()
    return (rc_c, rc_l), float(loss.cpu()[0]), [d.cpu().numpy() for d in dpreds], [int(c) for c in counts.cpu().numpy()]


def positive_zero(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) == 0)


def check_level(got_g, got_m, pred, label, weight, grad_mult, report=None):
    """M exact, dpred exactly +0 at invalid pixels and where pred == label, the gradients within GRAD_REL of the largest.
    No pixel is excluded.  Returns the twin's loss."""
    L, g, m = twin.loss_and_grad(pred, label, weight, grad_mult)
    assert got_m == m
    valid = twin.valid_mask(label)
    zero = ~valid | (pred == label).all(axis=-1)
    assert positive_zero(got_g[zero]).all()
    assert np.isfinite(got_g).all()
    top = np.abs(g).max()
    worst = np.abs(got_g.astype(np.float64) - g).max()
    if report is not None:
        report.append(worst / top if top else 0.0)
    assert worst <= GRAD_REL * top, (worst, top)
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_count_loss_and_gradient_match_the_twin(shape, pattern):
    for weight in WEIGHTS:
        for grad_mult in GRAD_MULTS:
            pred, label = case(1, shape, pattern)
            (rc_c, rc_l), loss, (g,), (m,) = launch([(pred, label, weight)], grad_mult)
            assert rc_c == 0 and rc_l == 0
            rel = []
            L = check_level(g, m, pred, label, weight, grad_mult, rel)
            print("sparse_epe %s %-6s w=%g gm=%g: M=%d loss rel err %.2e, grad err / max %.2e"
                  % (shape, pattern, weight, grad_mult, m, abs(loss - L) / L if L else abs(loss), rel[0]))
            assert abs(loss - L) <= LOSS_REL * abs(L)
            if pattern == "none" or weight == 0.0:
                assert loss == 0.0
            if pattern == "none":
                assert m == 0 and positive_zero(g).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_full_validity_is_the_dense_loss(shape):
    """With every label finite M = n h w and the op is fn2_epe_loss_grad on the same buffers."""
    import torch
    from src import _hip
    lib = _hip.lib()
    pred, label = case(2, shape, "all")
    n, h, w = shape
    for grad_mult in GRAD_MULTS:
        _, loss, (g,), (m,) = launch([(pred, label, 0.064)], grad_mult)
        assert m == n * h * w
        dev = torch.device("cuda", 0)
        p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
        d, acc = torch.full_like(p, float("nan")), torch.zeros(1, dtype=torch.float32, device=dev)
        _hip.check(lib.fn2_epe_loss_grad(_hip.ptr(p), _hip.ptr(l), _hip.ptr(d), _hip.ptr(acc), n, h, w, 0.064, grad_mult,
                                         _hip.stream_ptr()))
        torch.cuda.synchronize()
        dense_g, dense_loss = d.cpu().numpy().astype(np.float64), float(acc.cpu()[0])
        top = np.abs(dense_g).max()
        worst = np.abs(g - dense_g).max()
        print("sparse vs dense %s gm=%g: grad diff / max %.2e, loss rel diff %.2e"
              % (shape, grad_mult, worst / top, abs(loss - dense_loss) / dense_loss))
        assert worst <= DENSE_REL * top
        assert abs(loss - dense_loss) <= DENSE_REL * dense_loss


def five_levels(seed):
    shapes = [(2, 1, 1), (2, 2, 3), (2, 5, 7), (2, 3, 70), (2, 6, 130)]
    patterns = ["one", "half", "u_only", "inf", "half"]
    weights = [0.064, 0.016, 0.004, 0.002, 0.001]
    return [case(seed, s, p) + (w,) for s, p, w in zip(shapes, patterns, weights)]


@pytest.mark.gpu
def test_five_levels_in_one_launch_are_five_launches_and_repeat_bitwise():
    levels = five_levels(3)
    rcs, loss, gs, ms = launch(levels, 16384.0)
    rcs1, loss1, gs1, ms1 = launch(levels, 16384.0, one_by_one=True)
    rcs2, loss2, gs2, ms2 = launch(levels, 16384.0)
    assert rcs == (0, 0) and rcs1 == (0, 0) and rcs2 == (0, 0)
    assert ms == ms1 == ms2
    want = 0.0
    for g, g1, g2, m, (pred, label, weight) in zip(gs, gs1, gs2, ms, levels):
        assert np.array_equal(g.view(np.uint32), g1.view(np.uint32))
        assert np.array_equal(g.view(np.uint32), g2.view(np.uint32))
        want += check_level(g, m, pred, label, weight, 16384.0)
    for got in (loss, loss1, loss2):                               # (the order of the atomics is free: the sum is not bitwise)
        assert abs(got - want) <= LOSS_REL * want


@pytest.mark.gpu
def test_the_loss_is_added_and_dpred_is_stored():
    pred, label = case(4, (2, 5, 7), "half")
    _, loss0, (g0,), _ = launch([(pred, label, 0.064)], 1.0)
    _, loss1, (g1,), _ = launch([(pred, label, 0.064)], 1.0, loss_init=2.5, dpred_init=7.0)
    assert abs(loss1 - (2.5 + loss0)) <= 1e-6 * loss1
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 6, 130)])
def test_poisoned_predictions_at_invalid_pixels_reach_nothing(shape):
    """NaN, inf and 1e30 predictions where there is no ground truth: M, every dpred bit and the loss stay."""
    pred, label = case(5, shape, "half")
    invalid = ~twin.valid_mask(label)
    assert invalid.sum() >= 3 and (~invalid).sum() >= 3
    _, loss, (g,), (m,) = launch([(pred, label, 0.064)], 16384.0)
    bad = pred.copy()
    poison = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)
    idx = np.argwhere(invalid)
    for k, (i, y, x) in enumerate(idx):
        bad[i, y, x, k % 2] = poison[k % len(poison)]
        if k % 3 == 0:
            bad[i, y, x, 1 - k % 2] = poison[(k + 1) % len(poison)]
    _, loss_b, (g_b,), (m_b,) = launch([(bad, label, 0.064)], 16384.0)
    assert m_b == m
    assert np.array_equal(g.view(np.uint32), g_b.view(np.uint32))
    assert np.isfinite(loss_b) and abs(loss_b - loss) <= 1e-6 * loss


def check_invalid_arguments(hip):
    """Every check sits in front of the launch: the pointers are never followed."""
    lib = hip.lib()
    L = hip.Fn2SparseEpeLevel
    fake = 0x1000
    ok = lambda **kw: L(**dict(dict(pred=fake, label=fake, dpred=fake, count=fake, h=4, w=5, weight=0.5), **kw))
    nan, inf = float("nan"), float("inf")
    table_cases = [(None, {}, b"null level table"), (ok(), dict(nl=0), b"n_levels"),
                   ((L * 9)(*[ok() for _ in range(9)]), dict(nl=9), b"n_levels"), (ok(), dict(n=0), b"n must"),
                   (ok(), dict(n=-2), b"n must"), (ok(h=0), {}, b"bad size"), (ok(w=0), {}, b"bad size"),
                   (ok(w=-2), {}, b"bad size"), (ok(h=1 << 15, w=1 << 15), {}, b"2^31"), (ok(h=1 << 15, w=1 << 16), dict(n=1), b"2^31"),
                   (ok(pred=0x1004), {}, b"aligned"), (ok(label=0x1004), {}, b"aligned"), (ok(dpred=0x1004), {}, b"aligned"),
                   (ok(count=0x1002), {}, b"4-byte aligned"), ((L * 3)(ok(), ok(), ok(label=None)), dict(nl=3), b"level 2"),
                   (ok(pred=None), {}, b"null pointer"), (ok(label=None), {}, b"null pointer"),
                   (ok(dpred=None), {}, b"null pointer"), (ok(count=None), {}, b"null pointer"),
                   (ok(weight=-0.5), {}, b"weight"), (ok(weight=nan), {}, b"weight"), (ok(weight=inf), {}, b"weight")]
    loss_cases = [(ok(), dict(loss=None), b"loss_accum"), (ok(), dict(gm=0.0), b"grad_mult"), (ok(), dict(gm=-1.0), b"grad_mult"),
                  (ok(), dict(gm=nan), b"grad_mult"), (ok(), dict(gm=inf), b"grad_mult")]
    base = dict(nl=1, n=2, gm=1.0, loss=fake)

    def table_of(t):
        return t if t is None or not isinstance(t, L) else (L * 1)(t)

    for t, kw, word in table_cases:
        a = dict(base, **kw)
        rc = lib.fn2_sparse_epe_count(table_of(t), a["nl"], a["n"], None)
        msg = lib.fn2_last_error()
        assert rc == hip.ERR_INVALID_ARGUMENT and word in msg and b"sparse_epe_count" in msg, (word, rc, msg)
    for t, kw, word in table_cases + loss_cases:
        a = dict(base, **kw)
        rc = lib.fn2_sparse_epe_loss_grad(table_of(t), a["nl"], a["n"], a["gm"], a["loss"], None)
        msg = lib.fn2_last_error()
        assert rc == hip.ERR_INVALID_ARGUMENT and word in msg and b"sparse_epe_loss_grad" in msg, (word, rc, msg)
    with pytest.raises(ValueError, match="sparse_epe_loss_grad"):
        hip.check(lib.fn2_sparse_epe_loss_grad(table_of(ok()), 1, 2, 0.0, fake, None))
    assert C.sizeof(L) == 48                                        # four pointers, h, w, weight, padded to 8 bytes


@pytest.mark.gpu
def test_invalid_arguments_launch_nothing_on_the_device_box():
    """The error code comes back and dpred, the counter and the loss keep what they held."""
    import torch
    from src import _hip
    check_invalid_arguments(_hip)
    lib = _hip.lib()
    dev = torch.device("cuda", 0)
    pred, label = case(6, (3, 4, 5), "half")
    p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    d = torch.full_like(p, 7.0)
    count = torch.full((1,), 11, dtype=torch.int32, device=dev)
    loss = torch.full((1,), 2.5, dtype=torch.float32, device=dev)
    rec = lambda **kw: (_hip.Fn2SparseEpeLevel * 1)(_hip.Fn2SparseEpeLevel(**dict(dict(
        pred=p.data_ptr(), label=l.data_ptr(), dpred=d.data_ptr(), count=count.data_ptr(), h=4, w=5, weight=0.064), **kw)))
    s = _hip.stream_ptr()
    bad = _hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_sparse_epe_count(rec(h=0), 1, 3, s) == bad
    assert lib.fn2_sparse_epe_count(rec(), 0, 3, s) == bad
    assert lib.fn2_sparse_epe_loss_grad(rec(), 1, 3, 0.0, _hip.ptr(loss), s) == bad
    assert lib.fn2_sparse_epe_loss_grad(rec(weight=float("nan")), 1, 3, 1.0, _hip.ptr(loss), s) == bad
    assert lib.fn2_sparse_epe_loss_grad(rec(), 1, 3, 1.0, None, s) == bad
    assert lib.fn2_sparse_epe_loss_grad(rec(dpred=d.data_ptr() + 4), 1, 3, 1.0, _hip.ptr(loss), s) == bad
    torch.cuda.synchronize()
    assert int(count.cpu()[0]) == 11 and float(loss.cpu()[0]) == 2.5 and bool((d == 7.0).all())


@pytest.mark.gpu
def test_python_wrapper_returns_loss_gradient_and_count():
    import torch
    from src.sparse_epe import sparse_epe_loss
    pred, label = case(7, (2, 5, 7), "half")
    dev = torch.device("cuda", 0)
    loss, dpred, m = sparse_epe_loss(torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev), 0.064, grad_mult=4.0)
    L = check_level(dpred.cpu().numpy(), int(m.cpu()[0]), pred, label, 0.064, 4.0)
    assert abs(float(loss.cpu()[0]) - L) <= LOSS_REL * L
