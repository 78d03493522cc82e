"""The optimiser kernels beside Adam (csrc/train.hip: fn2_optim_grad_sumsq_multi, fn2_optim_step_multi_dev) on the C ABI
against float64 NumPy, and the trainer, its checkpoints and the interp command line on top of them.

Op level follows tests/test_gpu_train_ops.py section 6 (its helpers are imported, not copied): the tensor set of
ADAM_TENSORS in one guarded arena, every table word a kind does not use null, `partials` pre-filled with NaN, every bit
outside the updated tensors compared.  Tolerances are absolute, per element, to first order in the unit roundoff
U = 2^-24; `optim_ref` derives them from the operation count next to the float64 value they belong to."""
import math

import numpy as np
import pytest

import test_gpu_train_ops as ops
from test_gpu_train_ops import U, dev, host

B1, B2, EPS, L2, LR, GSCALE = ops.B1, ops.B2, ops.EPS, ops.L2, ops.LR, ops.GSCALE
KINDS = ["sgd", "momentum", "adam", "adamw"]
KIND_CODE = {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 3}
N_SLOTS = {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 2}
NPART = 128


# ------------------------------------------------------------------------------------------------ float64 reference
def f32(x):
    return float(np.float32(x))


def hyper_of(kind, lr=LR, mu=0.9, wd=0.0, clip=0.0, step=1, gscale=GSCALE):
    """The eight floats of the C ABI: {lr (lr_t for the Adam kinds), mu | beta1, beta2, eps, grad_scale, wd, clip, 0}."""
    if kind in ("adam", "adamw"):
        return np.array([ops.adam_lr_t(lr, B1, B2, step), B1, B2, EPS, gscale, wd, clip, 0.0], np.float32)
    return np.array([lr, mu, B2, EPS, gscale, wd, clip, 0.0], np.float32)


def grad_terms(w, g, hyper, reg):
    """G = gs g + reg w in float64 and its bound eG = 3 U (|gs g| + |reg w|) (see optim_ref)."""
    w, g = np.asarray(w, np.float64), np.asarray(g, np.float64)
    gs, reg = f32(hyper[4]), f32(reg)
    return gs * g + reg * w, 3 * U * (np.abs(gs * g) + np.abs(reg * w))


def grad_stats(w, g, hyper, reg):
    """(S = sum G^2, the sum of the per-term bounds 2 |G| eG + U G^2, n) of one whole tensor (see optim_ref)."""
    G, eG = grad_terms(w, g, hyper, reg)
    return float((G * G).sum()), float((2 * np.abs(G) * eG + U * G * G).sum()), G.size


def optim_ref(kind, w, a, v, g, hyper, reg, clip, stats=None):
    """One update of one tensor in float64 on the fp32 inputs and the fp32 scalars the kernels read, with the bound of
    every result (absolute, first order in U; each fp32 operation adds U times the magnitude of its result, FMA
    contraction only removes roundings):

      G = gs g + reg w        two products, one sum: eG = 3 U A, A = |gs g| + |reg w| >= |G|
      S = sum G^2             per term 2 |G| eG + U G^2 (the product), plus the summation, (n - 1) U S in any order
                              (written gamma_(n-1) S, so that it also holds for the largest tensor)
      c = clip / max(sqrt(S), clip)   relative ec = eS / (2 S) + 2 U (root, divide); exactly 1 below the threshold
      G <- G c                eG <- c eG + |G c| (ec + U)
      sgd        w' = w - lr G                    lr eG + 2 U lr |G| + U |w|        (product; difference <= |w| + lr |G|)
      momentum   a' = mu a + G                    ea = 2 U |mu a| + eG + U |G|      (product; sum <= |mu a| + |G|)
                 w' = w - (lr G + (lr mu) a')     lr eG + lr mu ea + U (3 lr |G| + 4 lr mu |a'| + |w|)
                                                  (lr G: 1; lr mu, its product with a': 2; the sum and the difference, each
                                                  bounded by the sum of magnitudes)
      adam       m' = b1 m + (1 - b1) G           em = 2 U |b1 m| + (1 - b1) (eG + 3 U |G|)     (1 - b1 itself rounds)
                 v' = b2 v + (1 - b2) G G         ev = 2 U b2 v + (1 - b2) (2 |G| eG + 4 U G^2)
                 u = lr_t m' / (sqrt(v') + eps)   eu = lr_t em / den + |u| (ev / (2 v') + 5 U)   (lr_t m', root, + eps,
                                                  the correctly rounded divide; sqrt(v') <= den)
                 w' = w - u                       eu + U |u| + U |w|
      adamw      w_d = w - wd w first             + 2 U |w| (product, difference); the rest as adam on w_d
    `stats`: grad_stats of the whole tensor when w, a, v, g are a chunk of it (everything but S is elementwise).
    Returns (w', {slot: (value, bound)}, bound of w', S, c)."""
    w = np.asarray(w, np.float64)
    lr, b1, b2, eps, gs, wd = (f32(x) for x in hyper[:6])
    clip = f32(clip)
    G, eG = grad_terms(w, g, hyper, reg)
    S, c = 0.0, 1.0
    if clip > 0.0:
        S, terms, n = stats if stats is not None else grad_stats(w, g, hyper, reg)
        k = (n - 1) * U
        eS = terms + k / (1 - k) * S
        norm = math.sqrt(S)
        c = clip / max(norm, clip)
        ec = (eS / (2 * S) + 2 * U) if S > 0 and norm + eS / (2 * norm) > clip else 0.0
        eG = c * eG + np.abs(G * c) * (ec + U)
        G = G * c
    aG = np.abs(G)
    slots = {}
    if kind == "sgd":
        return w - lr * G, slots, lr * eG + 2 * U * lr * aG + U * np.abs(w), S, c
    if kind == "momentum":
        a = np.asarray(a, np.float64)
        a2 = b1 * a + G
        ea = 2 * U * np.abs(b1 * a) + eG + U * aG
        slots["m"] = (a2, ea)
        tol = lr * eG + lr * b1 * ea + U * (3 * lr * aG + 4 * lr * b1 * np.abs(a2) + np.abs(w))
        return w - (lr * G + lr * b1 * a2), slots, tol, S, c
    m, v = np.asarray(a, np.float64), np.asarray(v, np.float64)
    tol = U * np.abs(w)
    if kind == "adamw":
        tol = tol + 2 * U * np.abs(w)
        w = w - wd * w
    m2 = b1 * m + (1 - b1) * G
    em = 2 * U * np.abs(b1 * m) + (1 - b1) * (eG + 3 * U * aG)
    v2 = b2 * v + (1 - b2) * G * G
    ev = 2 * U * b2 * v + (1 - b2) * (2 * aG * eG + 4 * U * G * G)
    den = np.sqrt(v2) + eps
    u = lr * m2 / den
    eu = lr * em / den + np.abs(u) * (ev / (2 * np.maximum(v2, 1e-300)) + 5 * U)
    slots["m"], slots["v"] = (m2, em), (v2, ev)
    return w - u, slots, tol + eu + U * np.abs(u), S, c


def assert_within(got, want, tol, what):
    err = np.abs(np.asarray(got, np.float64) - want)
    assert np.all(np.isfinite(got)), what
    bad = err > tol
    assert not bad.any(), (what, int(bad.sum()), float((err[bad] / tol[bad]).max()))


def expected_partials(G, n):
    """Which elements block x of a tensor's 128 strides: float4 i with (i mod 128 * 256) // 256 == x, and the scalar tail
    (at most three elements) in block 0.  float64 sums (exact on the dyadic data this is used with)."""
    out = np.zeros(NPART, np.float64)
    n4 = n >> 2
    sq = np.asarray(G, np.float64) ** 2
    blk = (np.arange(n4) % (NPART * 256)) // 256
    np.add.at(out, blk, sq[:4 * n4].reshape(n4, 4).sum(1))
    out[0] += sq[4 * n4:].sum()
    return out


# ------------------------------------------------------------------------------------------------ the arena
def tensor_inputs(seed, n, data):
    w, m, v, g = ops.adam_inputs(seed, n)
    rng = np.random.default_rng(seed + 1000)
    if data == "gauss":              # G ~ N(0, 1): cancellation in m', gradients of either sign, reg w in the norm
        g = (rng.standard_normal(n) / GSCALE).astype(np.float32)
    elif data == "exact":            # G = k / 2, k in +-1..+-4: G^2 a multiple of 1/4 <= 4, every partial sum exact in fp32
        k = rng.integers(1, 5, size=n) * rng.choice(np.array([-1, 1]), size=n)
        g = (k / 2.0 / GSCALE).astype(np.float32)
    elif data == "zero":
        g = np.zeros(n, np.float32)
    return w, m, v, g


def arena(seed, data):
    """ops.adam_arena with a choice of gradients: every tensor of ADAM_TENSORS with its three companions in one fp32
    arena, the split-fp16 copies in another, eight guard words in front of, between and behind them."""
    fl, xl, offs = [], [], []
    pos = {"f": 0, "x": 0}

    def put(lst, key, arr):
        lst.append(np.full(8, -2.25, np.float32))
        at = pos[key] + 8
        lst.append(arr)
        pad = -(at + arr.size) % 8
        lst.append(np.full(pad, -2.25, np.float32))
        pos[key] = at + arr.size + pad
        return at

    for t, (n, l2, copy, scale, frag_k) in enumerate(ops.ADAM_TENSORS):
        o = {name: put(fl, "f", a) for name, a in zip("wmvg", tensor_inputs(seed + t, n, data))}
        if copy is not None:
            o["x"] = put(xl, "x", np.full((n + 7) // 8 * 8, 1.5, np.float32))
        offs.append(o)
    fl.append(np.full(8, -2.25, np.float32))
    xl.append(np.full(8, -2.25, np.float32))
    return np.concatenate(fl), np.concatenate(xl), offs


class Run:
    """One arena on the device and the launches on it."""

    def __init__(self, seed, data, use_reg=True):
        import torch
        self.farena, self.xarena, self.offs = arena(seed, data)
        self.fd, self.xd = dev(self.farena), dev(self.xarena)
        assert self.fd.data_ptr() % 32 == 0 and self.xd.data_ptr() % 32 == 0
        self.regs = [t[1] if use_reg else 0.0 for t in ops.ADAM_TENSORS]
        self.counts = torch.tensor([t[0] for t in ops.ADAM_TENSORS], dtype=torch.int64, device="cuda")
        self.l2s = torch.tensor(self.regs, dtype=torch.float32, device="cuda")
        self.partials = dev(np.full(len(ops.ADAM_TENSORS) * NPART + 16, np.nan, np.float32))   # (+ 16 NaN guards behind)

    def table(self, kind):
        import torch
        rows = []
        for (n, l2, copy, scale, frag_k), o in zip(ops.ADAM_TENSORS, self.offs):
            at = lambda k: self.fd.data_ptr() + 4 * o[k]
            wx2 = self.xd.data_ptr() + 4 * o["x"] if copy is not None else 0
            bits = int(np.float32(scale).view(np.uint32)) | (int(frag_k) << 32)
            # the slots a kind lacks are null: a kernel that read them would fault
            rows.append([at("w"), at("m") if N_SLOTS[kind] >= 1 else 0, at("v") if N_SLOTS[kind] >= 2 else 0, at("g"), wx2, bits])
            assert all(p % 16 == 0 for p in rows[-1][:5])
        return torch.tensor(rows, dtype=torch.int64, device="cuda")

    def step(self, kind, hyper, clip):
        from src import _hip
        lib = _hip.lib()
        table, hd = self.table(kind), dev(np.asarray(hyper, np.float32))
        args = (_hip.ptr(table), _hip.ptr(self.counts), _hip.ptr(self.l2s), len(ops.ADAM_TENSORS), _hip.ptr(hd))
        if clip:
            _hip.check(lib.fn2_optim_grad_sumsq_multi(*args, _hip.ptr(self.partials), _hip.stream_ptr()))
            np.testing.assert_array_equal(host(self.fd).view(np.uint32), self.farena.view(np.uint32))   # writes only `partials`
            np.testing.assert_array_equal(host(self.xd).view(np.uint32), self.xarena.view(np.uint32))
        _hip.check(lib.fn2_optim_step_multi_dev(KIND_CODE[kind], *args, _hip.ptr(self.partials) if clip else None,
                                                _hip.stream_ptr()))
        return host(self.fd), host(self.xd), host(self.partials)


def check_run(run, kind, hyper, clip, fgot, xgot, pgot, before=None):
    """Everything the issue asks of one launch: values and slots within the derived bounds, g and every word outside the
    updated tensors bit for bit (guards, the slots the kind does not have), the copies bit-equal to the library's own
    conversion of the updated master, every partial written.  Returns [(S, c)] per tensor."""
    from src import _hip
    lib = _hip.lib()
    farena = run.farena if before is None else before
    touched_f, touched_x = np.zeros(farena.size, bool), np.zeros(run.xarena.size, bool)
    stats = []
    for t, ((n, l2, copy, scale, frag_k), o) in enumerate(zip(ops.ADAM_TENSORS, run.offs)):
        inp = {k: farena[o[k]:o[k] + n] for k in "wmvg"}
        out = {k: fgot[o[k]:o[k] + n] for k in "wmvg"}
        np.testing.assert_array_equal(out["g"].view(np.uint32), inp["g"].view(np.uint32))
        rw, slots, tol, S, c = optim_ref(kind, inp["w"], inp["m"], inp["v"], inp["g"], hyper, run.regs[t], hyper[6] if clip else 0.0)
        stats.append((S, c))
        assert_within(out["w"], rw, tol, (kind, "w", n))
        touched_f[o["w"]:o["w"] + n] = True
        for k, (val, bound) in slots.items():
            assert_within(out[k], val, bound, (kind, k, n))
            touched_f[o[k]:o[k] + n] = True
        if clip:
            p = pgot[t * NPART:(t + 1) * NPART]
            assert np.all(np.isfinite(p)) and np.all(p >= 0), (kind, n)            # every slot written, NaN nowhere left
        if copy is None:
            continue
        n8 = (n + 7) // 8 * 8
        src = np.zeros(n8, np.float32)
        src[:n] = out["w"]
        srcd, dstd = dev(src), dev(np.full(n8, 1.5, np.float32))
        if copy == "frag":
            _hip.check(lib.fn2_to_f16x2_frag(_hip.ptr(dstd), _hip.ptr(srcd), None, n8, scale, frag_k, _hip.stream_ptr()))
        else:
            _hip.check(lib.fn2_to_f16x2(_hip.ptr(dstd), _hip.ptr(srcd), None, n8, scale, _hip.stream_ptr()))
        want_bits, got_bits = ops.x2_bits(host(dstd)), ops.x2_bits(xgot[o["x"]:o["x"] + n8])
        if copy == "frag":
            np.testing.assert_array_equal(got_bits, want_bits)
        else:
            np.testing.assert_array_equal(got_bits[:n], want_bits[:n])
            np.testing.assert_array_equal(got_bits[n:], ops.x2_bits(run.xarena[o["x"]:o["x"] + n8])[n:])
        touched_x[o["x"]:o["x"] + n8] = True
    np.testing.assert_array_equal(fgot[~touched_f].view(np.uint32), farena[~touched_f].view(np.uint32))
    np.testing.assert_array_equal(xgot[~touched_x].view(np.uint32), run.xarena[~touched_x].view(np.uint32))
    if clip:
        assert np.all(np.isnan(pgot[len(ops.ADAM_TENSORS) * NPART:]))                # nothing behind the last tensor's row
    else:
        assert np.all(np.isnan(pgot))                                                # no clipping: partials are not touched
    return stats


# ------------------------------------------------------------------------------------------------ op level
@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 16.0])      # 16: the short tensors stay below it, the long ones are scaled
@pytest.mark.parametrize("kind", KINDS)
def test_optim_step_every_kind_with_and_without_clipping(kind, clip):
    run = Run(300, "adam")
    hyper = hyper_of(kind, wd=1e-2, clip=clip, step=3)
    stats = check_run(run, kind, hyper, clip > 0, *run.step(kind, hyper, clip > 0))
    if clip:
        cs = [c for _, c in stats]
        assert min(cs) < 0.5 and max(cs) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_clipping_with_a_regulariser_on_gaussian_gradients(kind):
    """reg != 0 (the norm is that of the regularised G) and gradients of either sign; the bound of S carries the
    (n - 1) U S summation term (optim_ref)."""
    run = Run(400, "gauss")
    assert any(r != 0 for r in run.regs)
    hyper = hyper_of(kind, wd=1e-2, clip=8.0, step=2)
    stats = check_run(run, kind, hyper, True, *run.step(kind, hyper, True))
    assert min(c for _, c in stats) < 0.1 and max(c for _, c in stats) == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["below", "above", "zero"])
@pytest.mark.parametrize("kind", KINDS)
def test_clipping_regimes_on_exact_data(kind, regime):
    """reg = 0, grad_scale a power of two, G = k / 2 with 1 <= |k| <= 4: every G^2 is a multiple of 1/4 and every partial
    sum an fp32 number in any order, so all 128 partials of every tensor are compared exactly (127 of them exactly 0 for
    n = 2).  below: clip_norm above every norm, the factor is exactly 1 and the result is the no-clip run's to 2 U;
    above: clip_norm below every norm; zero: an all-zero gradient, S = 0 -> factor 1, no NaN, and w moves by decay and
    momentum only."""
    data = "zero" if regime == "zero" else "exact"
    clip = {"below": 4096.0, "above": 0.25, "zero": 0.25}[regime]
    run = Run(500, data, use_reg=False)
    hyper = hyper_of(kind, wd=1e-2, clip=clip, step=2)
    fgot, xgot, pgot = run.step(kind, hyper, True)
    stats = check_run(run, kind, hyper, True, fgot, xgot, pgot)
    for t, ((n, *_), o) in enumerate(zip(ops.ADAM_TENSORS, run.offs)):
        G = run.farena[o["g"]:o["g"] + n].astype(np.float64) * GSCALE
        ops.exact_ok(4.0 * n, 0.25)                                   # S <= 4 n in quanta of 1/4: below 2^24 of them
        want = expected_partials(G, n)
        np.testing.assert_array_equal(pgot[t * NPART:(t + 1) * NPART].astype(np.float64), want)
        S, c = stats[t]
        assert S == want.sum()
        if n == 2:
            assert np.count_nonzero(want) == (0 if regime == "zero" else 1) and not pgot[1:NPART].any()
        assert {"below": c == 1.0, "above": c < 1.0, "zero": c == 1.0 and S == 0.0}[regime], (n, S, c)
    if regime == "below":
        plain = Run(500, data, use_reg=False)
        fplain, xplain, _ = plain.step(kind, hyper, False)
        for (n, *_), o in zip(ops.ADAM_TENSORS, run.offs):
            for k in "wmv":
                a, b = fgot[o[k]:o[k] + n].astype(np.float64), fplain[o[k]:o[k] + n].astype(np.float64)
                before = run.farena[o[k]:o[k] + n].astype(np.float64)
                assert np.all(np.abs(a - b) <= 2 * U * (np.abs(before) + np.abs(b - before))), (kind, k, n)
    if regime == "zero" and kind == "sgd":
        np.testing.assert_array_equal(fgot.view(np.uint32), run.farena.view(np.uint32))     # nothing moves at all


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 16.0])
def test_momentum_two_steps_with_cyclical_scalars(clip):
    """Two consecutive launches with different mu and lr in `hyper`, as cyclical momentum along a computed rate policy
    produces: the second starts from the first's accumulators and weights."""
    run = Run(600, "adam")
    h1 = hyper_of("momentum", lr=1e-3, mu=0.95, clip=clip)
    f1, x1, p1 = run.step("momentum", h1, clip > 0)
    check_run(run, "momentum", h1, clip > 0, f1, x1, p1)
    h2 = hyper_of("momentum", lr=3e-3, mu=0.85, clip=clip)
    run.partials.fill_(float("nan"))
    f2, x2, p2 = second_step(run, f1, x1, h2, clip > 0)
    check_run(run, "momentum", h2, clip > 0, f2, x2, p2, before=f1)


def second_step(run, f1, x1, hyper, clip):
    """The next launch on the arena as the first left it (Run.step compares against run.farena / run.xarena)."""
    keep = run.farena, run.xarena
    run.farena, run.xarena = f1, x1
    try:
        return run.step("momentum", hyper, clip)
    finally:
        run.farena, run.xarena = keep


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [0.0, 16.0])
def test_adamw_without_decay_is_the_adam_kind_bit_for_bit(clip):
    a, b = Run(700, "gauss"), Run(700, "gauss")
    fa, xa, pa = a.step("adam", hyper_of("adam", clip=clip, step=5), clip > 0)
    fb, xb, pb = b.step("adamw", hyper_of("adamw", wd=0.0, clip=clip, step=5), clip > 0)
    np.testing.assert_array_equal(fa.view(np.uint32), fb.view(np.uint32))
    np.testing.assert_array_equal(xa.view(np.uint32), xb.view(np.uint32))
    np.testing.assert_array_equal(pa.view(np.uint32), pb.view(np.uint32))
    assert not np.array_equal(fa.view(np.uint32), a.farena.view(np.uint32))


# ------------------------------------------------------------------------------------------------ trainer level
def batch(n, seed):
    from test_gpu_train import data
    return data(n, 128, 128, seed)


def snapshot(tr, keys):
    """Host copies of every parameter's tensors: the arenas in one transfer each, the masters one by one."""
    arenas = {"g": tr.grad_arena, "m": tr.m_arena, "v": tr.v_arena}
    flat = {k: a.detach().cpu().numpy() for k, a in arenas.items() if k in keys and a is not None}
    out, off = [], 0
    for p in tr.params:
        d = {k: (flat[k][off:off + p["n"]] if k in flat else None) for k in "gmv"}
        d["w"] = p["w"].detach().cpu().numpy().reshape(-1).copy()
        out.append(d)
        off += (p["n"] + 3) // 4 * 4
    return out


CHUNK = 1 << 20


def check_update(pool, kind, name, b, a, hyper, reg):
    """One tensor of the trainer against optim_ref: the norm over the whole tensor, the elementwise rest in chunks on
    the thread pool (NumPy releases the GIL; 36 M parameters in float64 otherwise take seconds per step)."""
    stats = grad_stats(b["w"], b["g"], hyper, reg)

    def chunk(lo):
        hi = min(lo + CHUNK, b["w"].size)
        cut = lambda d, k: d[k][lo:hi] if d[k] is not None else None
        rw, slots, tol, S, c = optim_ref(kind, cut(b, "w"), cut(b, "m"), cut(b, "v"), cut(b, "g"), hyper, reg, hyper[6], stats)
        assert_within(cut(a, "w"), rw, tol, (name, "w", lo))
        for k, (val, bound) in slots.items():
            assert_within(cut(a, k), val, bound, (name, k, lo))
        return c
    return [pool.submit(chunk, lo) for lo in range(0, b["w"].size, CHUNK)]


def trainer_hyper(tr, step):
    """The eight floats of global step `step` (0-based), computed here from the schedule functions."""
    from src.training_schedules import learning_rate, momentum_value
    params = getattr(tr, "train_params", None)           # (set by the command lines and by tests, not by the trainer)
    lr = learning_rate(tr.schedule, step, params)
    mu, b2 = tr.schedule["momentum"], tr.schedule["momentum2"]
    if tr.optimizer == "momentum":
        mu = momentum_value(tr.schedule, step, params, tr.momentum, tr.min_momentum, tr.max_momentum)
    if tr.optimizer in ("adam", "adamw"):
        t = float(step + 1)
        lr = lr * math.sqrt(1.0 - b2 ** t) / (1.0 - mu ** t)
    return np.array([lr, mu, b2, tr.eps, 1.0 / tr.loss_scale, tr.weight_decay, tr.clip_norm, 0.0], np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
@pytest.mark.parametrize("kind", KINDS)
def test_trainer_update_equals_numpy(kind, dtype):
    """forward_backward, snapshot the gradient arena, every master and slot, apply_gradients, compare with the NumPy
    optimiser on the snapshots (no autograd oracle needed; the bounds are the op level's).  Two steps on one_cycle with
    clr_stepsize = 1: the rate goes 1e-5 -> 1e-4 and the cyclical momentum 0.95 -> 0.85, and the second step starts from
    the first's accumulators.  clip_grad_norm = 1e-3: some tensors are clipped, some are not."""
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    from src.training_schedules import SCHEDULES
    tr = FlowNetSTrainer(W.init_weights("FlowNetS", 6), 1, 128, 128, schedule=SCHEDULES["one_cycle"], dtype=dtype,
                         optimizer=kind, clip_grad_norm=1e-3, weight_decay=1e-3 if kind == "adamw" else None)
    tr.train_params = {"clr_stepsize": 1}
    assert tr.m_arena is None if kind == "sgd" else tr.m_arena is not None
    assert tr.v_arena is None if kind in ("sgd", "momentum") else tr.v_arena is not None
    import torch
    from concurrent.futures import ThreadPoolExecutor
    hypers, factors = [], []
    with ThreadPoolExecutor(8) as pool:
        for step in (0, 1):
            tr.forward_backward(*batch(1, 2 + step))
            before = snapshot(tr, "gmv")
            g_before = tr.grad_arena.clone()
            tr.apply_gradients()
            after = snapshot(tr, "mv")
            assert torch.equal(tr.grad_arena.view(torch.int32), g_before.view(torch.int32))      # g is read only
            hyper = trainer_hyper(tr, step)
            hypers.append(hyper)
            jobs = []
            for p, b, a in zip(tr.params, before, after):
                jobs += check_update(pool, kind, p["name"], b, a, hyper, tr.l2_reg if p["reg"] else 0.0)
            factors += [j.result() for j in jobs]
    assert tr.step_count == 2 and hypers[0][0] != hypers[1][0]
    if kind == "momentum":
        assert abs(hypers[0][1] - 0.95) < 1e-6 and abs(hypers[1][1] - 0.85) < 1e-6
    assert min(factors) < 1.0 and max(factors) == 1.0            # both occur: clipped and unclipped tensors


@pytest.mark.gpu
def test_captured_momentum_step_equals_eager(monkeypatch):
    """train_step on momentum + clipping, three steps: the captured segments (sumsq + step in the last one) end at the
    weights and accumulators of the eager launch sequence, within the tolerances test_captured_train_step_equals_eager
    uses for Adam (the filter gradients are summed with fp32 atomics, whose order differs run to run; a step of
    lr 1e-4 on a gradient clipped to norm 1e-3 moves a weight far less than Adam's 1e-4)."""
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    wts = W.init_weights("FlowNetS", 6)
    batches = [batch(2, 20 + i) for i in range(3)]
    kw = dict(dtype="f16x2", optimizer="momentum", momentum=0.9, clip_grad_norm=1e-3)
    monkeypatch.setenv("FN2_TRAIN_GRAPH", "0")
    eager = FlowNetSTrainer(wts, 2, 128, 128, **kw)
    start = [p["w"].cpu().numpy().copy() for p in eager.params]
    le = [float(eager.train_step(*b).item()) for b in batches]
    monkeypatch.setenv("FN2_TRAIN_GRAPH", "1")
    graph = FlowNetSTrainer(wts, 2, 128, 128, **kw)
    lg = [float(graph.train_step(*b).item()) for b in batches]
    assert graph._step_graphs is not None and eager.step_count == graph.step_count == 3
    np.testing.assert_allclose(lg, le, rtol=1e-5)
    moved = 0.0
    for pe, pg, w0 in zip(eager.params, graph.params, start):
        we, wg = pe["w"].cpu().numpy(), pg["w"].cpu().numpy()
        diff = np.abs(we - wg)
        assert diff.max() <= 6.1e-4 and (diff > 3e-5).mean() < 1e-2, (pe["name"], diff.max())
        ae, ag = pe["m"].cpu().numpy(), pg["m"].cpu().numpy()
        assert np.abs(ag - ae).max() <= 1e-2 * max(np.abs(ae).max(), 1e-30), pe["name"]
        assert pe["v"] is None and pg["v"] is None
        moved = max(moved, float(np.abs(wg - w0).max()))
    assert moved > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_momentum_checkpoint_round_trip(fmt, tmp_path):
    from src import weights as W
    from src.flownet_s import train as cli
    from src.trainer import FlowNetSTrainer
    kw = dict(dtype="f32", optimizer="momentum", momentum=0.9)
    tr = FlowNetSTrainer(W.init_weights("FlowNetS", 6), 1, 128, 128, **kw)
    tr.forward_backward(*batch(1, 2))
    tr.apply_gradients()
    state = tr.optimizer_state()
    slots = [k for k in state if k != "global_step"]
    assert len(slots) == len(tr.params) and all(k.endswith("/Momentum") for k in slots) and int(state["global_step"]) == 1
    path = cli.save_checkpoint(str(tmp_path), 1, dict(cli.unpack_weights(tr), **state), fmt)
    full = cli.load_full_checkpoint(path)
    tr2 = FlowNetSTrainer(W.load_weights(path), 1, 128, 128, **kw)
    assert tr2.load_optimizer_state(full) == len(tr.params) and tr2.step_count == 1
    for p, q in zip(tr.params, tr2.params):
        np.testing.assert_array_equal(q["m"].cpu().numpy(), p["m"].cpu().numpy())
        np.testing.assert_array_equal(q["w"].cpu().numpy(), p["w"].cpu().numpy())
    w1 = [p["w"].cpu().numpy().copy() for p in tr.params]
    for t in (tr, tr2):
        t.forward_backward(*batch(1, 3))
        t.apply_gradients()
    assert tr2.step_count == 2
    for p, q, w in zip(tr.params, tr2.params, w1):
        a, b = p["w"].cpu().numpy(), q["w"].cpu().numpy()
        # the same masters and accumulators, gradients equal up to the order of the fp32 atomics: the second steps agree
        # to 1 % of the largest movement of the tensor (without the accumulators the step would lack its mu a' share,
        # about half of it) plus the rounding of the difference
        assert np.abs(a - b).max() <= 1e-2 * np.abs(a - w).max() + 2 * U * np.abs(a).max(), p["name"]
    if fmt == "npz":   # a checkpoint with another optimiser's slots: the step counter alone
        adam_state = {"global_step": np.int64(7), "beta1_power": np.float32(0.9 ** 8), "beta2_power": np.float32(0.999 ** 8)}
        for k in slots:     # what Adam writes for the same variables: <var>/Adam and <var>/Adam_1
            adam_state[k[:-len("/Momentum")] + "/Adam"] = adam_state[k[:-len("/Momentum")] + "/Adam_1"] = state[k]
        assert tr2.load_optimizer_state(adam_state) == 0 and tr2.step_count == 7


@pytest.mark.gpu
def test_default_trainer_is_the_adam_kind_on_the_one_update_path(monkeypatch):
    """optimizer='adam' without clipping is a kind like the others: the eager and the captured step launch
    fn2_optim_step_multi_dev with the Adam kind and null partials, and upload the same eight floats.  The two optimiser
    entries of trainer.lib are wrapped by functions that note the call and pass it on
    (test_adam_steps_match_oracle checks the values)."""
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    tr = FlowNetSTrainer(W.init_weights("FlowNetS", 6), 1, 128, 128, dtype="f16x2")
    calls = []

    def record(name):
        real = getattr(tr.lib, name)

        def call(*args):
            calls.append((name, args))
            return real(*args)
        monkeypatch.setattr(tr.lib, name, call)
    record("fn2_optim_grad_sumsq_multi")
    record("fn2_optim_step_multi_dev")

    def taken():
        out = calls[:]
        del calls[:]
        return out

    def device_hyper(t):
        return t._hyper.cpu().numpy().view(np.uint32)
    assert tr.optimizer == "adam" and tr.clip_norm == 0.0 and tr.m_arena is not None and tr.v_arena is not None
    tr.forward_backward(*batch(1, 2))
    assert taken() == []
    tr.apply_gradients()
    (name, args), = taken()                                         # exactly one launch, and no squared norms
    assert name == "fn2_optim_step_multi_dev" and args[0] == KIND_CODE["adam"] and args[6] is None
    np.testing.assert_array_equal(device_hyper(tr), trainer_hyper(tr, 0).view(np.uint32))
    tr.train_step(*batch(1, 3))
    (name, args), = taken()                                         # the capture; nothing is launched un-captured
    assert name == "fn2_optim_step_multi_dev" and args[0] == KIND_CODE["adam"] and args[6] is None
    np.testing.assert_array_equal(device_hyper(tr), trainer_hyper(tr, 1).view(np.uint32))
    tr.train_step(*batch(1, 4))
    assert taken() == []                                            # a replay calls no entry
    np.testing.assert_array_equal(device_hyper(tr), trainer_hyper(tr, 2).view(np.uint32))
    assert tr.step_count == 3 and tr._step_graphs is not None
    assert sorted(k.rsplit("/", 1)[1] for k in tr.optimizer_state() if "/weights/" in k)[0] == "Adam"
    # a checkpoint of the Momentum optimiser holds no slot of Adam's: the step counter alone is restored
    foreign = {"FlowNetS/conv1/weights/Momentum": np.zeros(1, np.float32), "global_step": np.int64(5)}
    assert tr.load_optimizer_state(foreign) == 0 and tr.step_count == 5
    clipped = FlowNetSTrainer(W.init_weights("FlowNetS", 6), 1, 128, 128, dtype="f16x2", clip_grad_norm=1.0)
    clipped.forward_backward(*batch(1, 2))
    clipped.apply_gradients()
    (sumsq, sargs), (step, args) = taken()                          # both passes, in that order, on the same partials
    assert sumsq == "fn2_optim_grad_sumsq_multi" and step == "fn2_optim_step_multi_dev" and args[0] == KIND_CODE["adam"]
    assert args[6] is not None and args[6].value and args[6].value == sargs[5].value == clipped._partials.data_ptr()
    np.testing.assert_array_equal(device_hyper(clipped), trainer_hyper(clipped, 0).view(np.uint32))


@pytest.mark.gpu
def test_interp_cli_with_momentum_one_cycle_and_clipping(tmp_path):
    """src.flownet_s_interp.train.main with --optimizer momentum --training_schedule one_cycle --clip_grad_norm 1.0, two
    steps on a two-record file: the checkpoint carries <var>/Momentum slots and none of Adam's."""
    import types
    from src import tfrecord, weights as W
    from src.flownet_s_interp import train as cli
    rng = np.random.default_rng(11)
    path = str(tmp_path / "interp.tfrecords")
    with tfrecord.TFRecordWriter(path) as w:
        for _ in range(2):
            img = rng.random((128, 192, 3))
            flow = np.clip(rng.standard_normal((128, 192, 2)) * 3, -20, 20).astype(np.float32)
            m = (rng.random((128, 192, 1)) < 0.05).astype(np.float64)
            w.write(tfrecord.encode_sample(img, flow=flow, matches_a=m, sparse_flow=(flow * m).astype(np.float32),
                                           edges_a=rng.random((128, 192, 1)).astype(np.float32)))
    flags = types.SimpleNamespace(records=path, out=str(tmp_path / "ck"), checkpoint=None, ckpt_format="npz", steps=2,
                                  batch=1, dtype="f16x2", height=128, width=192, add_hard_flow_mining="",
                                  lambda_weight=2.0, hard_examples_perc=50, seed=3, log_every=1, save_every=10,
                                  optimizer="momentum", training_schedule="one_cycle", clip_grad_norm=1.0)
    tr = cli.main(flags)
    assert tr.step_count == 2 and np.isfinite(float(tr.loss_dev.item()))
    assert tr.optimizer == "momentum" and tr.clip_norm == 1.0 and tr.schedule["learning_rates"] == "one_cycle"
    saved = W.load_npz(str(tmp_path / "ck" / "flownet_s_interp-2.npz"))
    assert "FlowNetS/conv1/weights" in saved and "FlowNetS/conv1/weights/Momentum" in saved
    assert any(k.endswith("/Momentum") for k in saved) and not any(k.endswith(("/Adam", "/Adam_1")) for k in saved)
    assert "beta1_power" not in saved and int(saved["global_step"]) == 2
    assert float(np.abs(saved["FlowNetS/conv1/weights/Momentum"]).max()) > 0.0
