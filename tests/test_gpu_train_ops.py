"""The trainer's loss, bias, activation, flow-head, Adam and copy kernels (csrc/train.hip) one by one on the C ABI against
plain float64 NumPy.

Method: inputs come from small dyadic grids (integers in [-8, 8] divided by 4), so every product is a multiple of 1/16 of
magnitude <= 4 and every sum of such terms is exact in fp32 in ANY order -- per-thread chains, shuffles, LDS, atomics,
with or without FMA contraction -- as long as sum |terms| / quantum < 2^24.  Each exact test asserts that precondition on
its float64 reference (`exact_ok`) and then compares with assert_array_equal: a lost, doubled or misplaced pixel moves
the result by at least one quantum.  The same values are exact in split fp16 with a zero lo part.  A tolerance remains
only where an inexact operation is part of the definition (the slopes 0.1 / 0.55, a division, a square root); it is
derived from the unit roundoff U = 2^-24 where it is used.

Every output buffer is pre-filled with dyadic sentinels: what lies outside the addressed channel slice (pad channels of
a view, rows of dw beyond cin, guard words behind a buffer) must come back bit for bit, and so must read-only inputs.
The tests pin: db, dw and dx always accumulate; dpf accumulates only when asked; loss_accum accumulates."""
import ctypes as C

import numpy as np
import pytest

U = 2.0 ** -24          # unit roundoff of fp32
BIG = 4096 * 256        # threads of the largest grid (grid_for): more work items than this run the grid-stride loops


# ------------------------------------------------------------------------------------------------ helpers
def dyadic(seed, shape, nonzero=False):
    """Integers in [-8, 8] / 4 (nonzero: without 0, where a lost term must be visible)."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-8, 9, size=shape)
    if nonzero:
        k = np.where(k == 0, rng.integers(1, 9, size=shape), k)
    return (k / 4.0).astype(np.float32)


def exact_ok(abs_bound, quantum, bits=24):
    """The exactness precondition: every partial sum is a multiple of `quantum` bounded by sum |terms| = abs_bound, so it
    is an integer below 2^bits times the quantum (24: fp32; 22: also exact as split fp16, 11 bits hi + 11 bits lo)."""
    assert float(np.max(abs_bound)) / quantum < 2.0 ** bits, (float(np.max(abs_bound)), quantum)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def split(x):
    """fp32 [..., cs] -> the float32 container of its split-fp16 image."""
    from src import weights as W
    return W.split_f16x2(x).view(np.float32)


def x2_bits(raw):
    """float32 container [..., cs] of a split-fp16 buffer -> uint16 [..., cs, 2]: the (hi, lo) bit patterns per channel."""
    h = np.ascontiguousarray(raw).view(np.uint16)
    h = h.reshape(h.shape[:-1] + (h.shape[-1] // 16, 2, 8))
    return np.swapaxes(h, -1, -2).reshape(raw.shape + (2,))


def x2_join(raw):
    """The logical values hi + lo of a split-fp16 container, in float64."""
    b = x2_bits(raw).view(np.float16).astype(np.float64)
    return b[..., 0] + b[..., 1]


def make_buf(x, dtype):
    """Device buffer (float32 container) of the host fp32 array x in the given storage."""
    return dev(split(x) if dtype == "f16x2" else x)


def logical(raw, dtype):
    return x2_join(raw) if dtype == "f16x2" else raw.astype(np.float64)


def bits_of(raw, dtype):
    return x2_bits(raw) if dtype == "f16x2" else np.ascontiguousarray(raw).view(np.uint32)[..., None]


def assert_outside_unchanged(before, after, dtype, c, c0):
    """Channels outside [c0, c0 + c) of a buffer come back bit for bit."""
    b, a = bits_of(before, dtype), bits_of(after, dtype)
    keep = np.ones(b.shape[-2], bool)
    keep[c0:c0 + c] = False
    np.testing.assert_array_equal(a[..., keep, :], b[..., keep, :])


def code_of(dtype):
    return 3 if dtype == "f16x2" else 0


def guarded(values, guard=-1.75, n_guard=8):
    """[n_guard guards | values | n_guard guards] on the device and the (16-byte aligned) pointer to the values."""
    v = np.asarray(values, np.float32).ravel()
    full = np.concatenate([np.full(n_guard, guard, np.float32), v, np.full(n_guard, guard, np.float32)])
    t = dev(full)
    return t, C.c_void_p(t.data_ptr() + 4 * n_guard), full


def guards_ok(t, full, n, n_guard=8):
    got = host(t)
    np.testing.assert_array_equal(got[:n_guard], full[:n_guard])
    np.testing.assert_array_equal(got[n_guard + n:], full[n_guard + n:])
    return got[n_guard:n_guard + n]


# ------------------------------------------------------------------------------------------------ float64 references
def upsample_flow_bwd_ref(g, pf, w):
    """dpf[n,y,x,i] = sum g[n,2y+ky-1,2x+kx-1,o] w[ky,kx,o,i];  dw[ky,kx,o,i] = sum g[n,2y+ky-1,2x+kx-1,o] pf[n,y,x,i]."""
    g, pf, w = np.asarray(g, np.float64), np.asarray(pf, np.float64), np.asarray(w, np.float64)
    N, H, W_, _ = pf.shape
    gp = np.pad(g, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dpf, dw = np.zeros_like(pf), np.zeros((4, 4, 2, 2))
    for ky in range(4):
        for kx in range(4):
            gs = gp[:, ky:ky + 2 * H:2, kx:kx + 2 * W_:2]             # g[n, 2y + ky - 1, 2x + kx - 1, o]
            dpf += gs @ w[ky, kx]
            dw[ky, kx] = np.einsum("nyxo,nyxi->oi", gs, pf)
    return dpf, dw


def head_bwd_data_ref(g, w):
    """dx[n,y,x,ci] = sum_{ky,kx,co} g[n, y+1-ky, x+1-kx, co] w[ky,kx,ci,co]  (w HWIO; g zero outside)."""
    g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
    N, H, W_, _ = g.shape
    gp = np.pad(g, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dx = np.zeros((N, H, W_, w.shape[2]))
    for ky in range(3):
        for kx in range(3):
            dx += gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W_] @ w[ky, kx].T
    return dx


def filter_grad(x, dy):
    """dW[ky,kx,ci,co] = sum_{n,y,x} xpad[n, y+ky, x+kx, ci] dy[n,y,x,co]  (k = 3, pad = 1; as tests/test_gpu_bwd_ops.py)."""
    n, h, w, ci = x.shape
    co = dy.shape[-1]
    xp = np.zeros((n, h + 2, w + 2, ci), np.float64)
    xp[:, 1:1 + h, 1:1 + w] = x
    out = np.zeros((3, 3, ci, co), np.float64)
    d = dy.astype(np.float64).reshape(-1, co)
    for ky in range(3):
        for kx in range(3):
            out[ky, kx] = xp[:, ky:ky + h, kx:kx + w].reshape(-1, ci).T @ d
    return out


def adam_ref(w, m, v, g, lr_t, b1, b2, eps, l2, gscale):
    """One step in float64 on the fp32 inputs; the scalars are the fp32 values the C ABI receives."""
    w, m, v, g = (np.asarray(a, np.float64) for a in (w, m, v, g))
    b1, b2, eps, l2, gscale, lr_t = (float(np.float32(a)) for a in (b1, b2, eps, l2, gscale, lr_t))
    g2 = g * gscale + l2 * w
    m2 = b1 * m + (1.0 - b1) * g2
    v2 = b2 * v + (1.0 - b2) * g2 * g2
    upd = lr_t * m2 / (np.sqrt(v2) + eps)
    return w - upd, m2, v2, upd


def adam_lr_t(lr, b1, b2, step):
    lr, b1, b2 = (float(np.float32(a)) for a in (lr, b1, b2))
    return np.float32(lr * np.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step))


# ------------------------------------------------------------------------------------------------ CPU: the references
def test_upsample_flow_bwd_reference_is_the_adjoint_of_the_oracle():
    """<conv2d_transpose(pf, w), g> = <pf, dpf> = <w, dw>: the forward op is bilinear in (pf, w).  Dyadic: exact."""
    from oracle import nn
    pf, w, g = dyadic(1, (1, 3, 4, 2)), dyadic(2, (4, 4, 2, 2)), dyadic(3, (1, 6, 8, 2))
    out = nn.conv2d_transpose(pf, w)
    assert out.shape == g.shape
    dpf, dw = upsample_flow_bwd_ref(g, pf, w)
    lhs = float((out * g.astype(np.float64)).sum())
    assert lhs != 0.0
    assert lhs == float((pf.astype(np.float64) * dpf).sum())
    assert lhs == float((w.astype(np.float64) * dw).sum())


def test_head_references_are_the_adjoints_of_the_oracle():
    """<conv2d(x, w, padding=1), g> = <x, dx> = <w, dW> for the 3x3 flow head.  Dyadic: exact."""
    from oracle import nn
    x, w, g = dyadic(4, (2, 4, 5, 6)), dyadic(5, (3, 3, 6, 2)), dyadic(6, (2, 4, 5, 2))
    out = nn.conv2d(x, w, padding=1)
    lhs = float((out * g.astype(np.float64)).sum())
    assert lhs != 0.0
    assert lhs == float((x.astype(np.float64) * head_bwd_data_ref(g, w)).sum())
    assert lhs == float((w.astype(np.float64) * filter_grad(x, g)).sum())


def test_split_helpers_round_trip():
    """x2_bits / x2_join read the storage the way src.weights writes it (8 hi parts, then 8 lo parts, per group)."""
    from src import weights as W
    x = (np.random.default_rng(7).standard_normal((3, 24)) * 3).astype(np.float32)
    raw = split(x)
    np.testing.assert_array_equal(x2_join(raw), W.join_f16x2(raw.view(np.float16)).astype(np.float64))
    hi = x.astype(np.float16)
    np.testing.assert_array_equal(x2_bits(raw)[..., 0], hi.view(np.uint16))
    assert np.all(x2_bits(split(dyadic(8, (2, 16))))[..., 1] == 0)      # dyadic values: zero lo part


# ------------------------------------------------------------------------------------------------ 1. fn2_bias_grad
PIX_A, PIX_B, PIX_C, PIX_D = (3, 29, 31), (2, 9, 11), (1, 5, 7), (1, 2, 3)      # 2697, 198, 35 and 6 pixels
# act_bias_bwd_kernel (fp32, a thread owns a float4 of channels): gpb_log2_for picks the groups per block, bias_splits the
# pixel ranges; inside a range a thread row runs the four-pixels-per-trip main loop, then the tail loop
F32_ALIGNED = [
    ("f32", 8, 24, 12, PIX_A),       # 2 groups per block, 128 thread rows, 2 pixel splits: main loop (2 trips) + tail
    ("f32", 200, 208, 4, PIX_B),     # 64 groups per block (50 busy), 4 thread rows, 6 splits of 33 pixels: 2 trips + tail
    ("f32", 1028, 1032, 4, PIX_C),   # 257 groups: the cap of 256 per block, so a second channel block that holds ONE
                                     # group; 1 thread row, 2 splits of 18 / 17 pixels: 4 trips + tail
    ("f32", 4, 4, 0, PIX_D),         # one group, one split, 6 of 256 thread rows busy: tail loop only
]
# act_bias_bwd_x2_kernel (split fp16, a thread owns a group of 8 channels)
X2_GROUPS = [
    ("f16x2", 8, 24, 8, PIX_A),      # 1 group per block, 256 thread rows, 1 split: main loop (2 trips) + tail
    ("f16x2", 200, 208, 8, PIX_B),   # 32 groups per block (25 busy), 8 thread rows, 3 splits of 66 pixels: 2 trips + tail
    ("f16x2", 2056, 2064, 8, PIX_C), # 257 groups: two channel blocks, the second with one group; 2 splits: 4 trips + tail
]
BIAS_CASES = [
    # bias_grad2_kernel (dense fp32, c == cs == 2): one partly filled block; three blocks
    ("f32", 2, 2, 0, PIX_D), ("f32", 2, 2, 0, PIX_A),
] + F32_ALIGNED + [
    # bias_grad_kernel (generic fp32: c % 4 != 0 or an unaligned slice; serves the biased fuse_upsample_flow slices):
    # one pixel split (2697 pixels); three pixel splits (10240 pixels); 70 channels: a second, ragged channel block
    ("f32", 2, 16, 6, PIX_A), ("f32", 70, 72, 1, PIX_A), ("f32", 2, 16, 6, (2, 64, 80)), ("f32", 70, 72, 1, (2, 64, 80)),
] + X2_GROUPS + [
    # bias_grad_x2_narrow_kernel (split fp16, c < 8): a slice inside one group, at its end and from its second channel
    ("f16x2", 2, 16, 6, PIX_A), ("f16x2", 7, 8, 1, PIX_A),
]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,c,cs,c0,nhw", BIAS_CASES)
def test_bias_grad_is_the_exact_pixel_sum(dtype, c, cs, c0, nhw):
    from src import _hip
    lib = _hip.lib()
    g = dyadic(10 + c, nhw + (cs,), nonzero=True)
    sl = g[..., c0:c0 + c].astype(np.float64)
    want = 3.0 + sl.sum((0, 1, 2))
    exact_ok(3.0 + np.abs(sl).sum((0, 1, 2)), 0.25)
    gd = make_buf(g, dtype)
    g_before = host(gd)
    db, dbp, full = guarded(np.full(c, 3.0, np.float32))
    v = _hip.view(gd, c, c0, code_of(dtype))
    _hip.check(lib.fn2_bias_grad(C.byref(v), dbp, _hip.stream_ptr()))
    got = guards_ok(db, full, c)
    np.testing.assert_array_equal(got.astype(np.float64), want)
    np.testing.assert_array_equal(bits_of(host(gd), dtype), bits_of(g_before, dtype))     # g is read-only


# ------------------------------------------------------------------------------------------------ 2. fn2_leaky_bwd


@pytest.mark.gpu
@pytest.mark.parametrize("with_db", [True, False])     # False: the db == nullptr early return (activation only)
@pytest.mark.parametrize("dtype,c,cs,c0,nhw", F32_ALIGNED + X2_GROUPS)   # the branches named in the two tables
def test_leaky_bwd_slopes_and_bias_sum(dtype, c, cs, c0, nhw, with_db):
    from src import _hip
    lib = _hip.lib()
    rng = np.random.default_rng(200 + c)
    y_cs, y_c0 = c + 24, 16                              # y lives in another buffer with another stride and offset
    y = dyadic(20 + c, nhw + (y_cs,), nonzero=True)
    r = rng.random(y.shape)
    y[r < 0.05] = 0.0                                    # +0.0 and -0.0 both take the slope 0.55
    y[r < 0.01] = -0.0
    y[0, 0, 0, y_c0], y[0, 0, 0, y_c0 + 1] = 0.0, -0.0   # both zeros inside the slice at every size
    g = dyadic(30 + c, nhw + (cs,), nonzero=True)
    ys, gs = y[..., y_c0:y_c0 + c], g[..., c0:c0 + c]
    assert (ys == 0).any() and np.signbit(ys[ys == 0]).any() and (ys > 0).any() and (ys < 0).any()
    slope = np.where(ys > 0, np.float32(1.0), np.where(ys < 0, np.float32(0.1), np.float32(0.55))).astype(np.float32)
    want32 = gs * slope                                  # one fp32 multiply: nothing to contract
    assert want32.dtype == np.float32
    yd, gd = make_buf(y, dtype), make_buf(g, dtype)
    y_before, g_before = host(yd), host(gd)
    db, dbp, full = guarded(np.full(c, 0.5, np.float32))
    vy, vg = _hip.view(yd, c, y_c0, code_of(dtype)), _hip.view(gd, c, c0, code_of(dtype))
    _hip.check(lib.fn2_leaky_bwd(C.byref(vy), C.byref(vg), dbp if with_db else None, _hip.stream_ptr()))
    g_after = host(gd)
    np.testing.assert_array_equal(bits_of(host(yd), dtype), bits_of(y_before, dtype))     # y is read-only
    assert_outside_unchanged(g_before, g_after, dtype, c, c0)
    if dtype == "f32":
        new_g = g_after[..., c0:c0 + c]
        np.testing.assert_array_equal(new_g.view(np.uint32), want32.view(np.uint32))
        stored = new_g.astype(np.float64)
    else:
        # hi = the product rounded to 11 bits leaves a remainder that fp32 holds exactly; lo rounds that remainder to 11
        # bits (relative 2^-11 * 2^-11) or to the fp16 subnormal spacing 2^-24 (absolute 2^-25)
        stored = x2_join(g_after)[..., c0:c0 + c]
        w64 = want32.astype(np.float64)
        err = np.abs(stored - w64)
        bound = 2.0 ** -22 * np.abs(w64) + 2.0 ** -25
        assert np.all(err <= bound), float((err / bound).max())
    got_db = guards_ok(db, full, c)
    if not with_db:
        np.testing.assert_array_equal(got_db, np.full(c, 0.5, np.float32))
        return
    # db: the terms are inexact, so a bound: |db - ref64| <= 64 U sum |g'|, ref64 the float64 sum of the STORED new g.
    # An fp32 addition errs by at most U / 2 times its result, which sum |g'| (+ the 0.5 db starts from) bounds, so a
    # summation whose longest chain of additions is L stays within L U / 2 of that.  Here the per-thread chain is <= 17
    # pixels, the thread rows of a block are added one after the other (up to 255 additions at c = 8, 3 at c = 200, none
    # at c >= 1028) and the pixel splits meet in <= 6 atomics, so 64 covers every chain of up to 128 additions; random
    # signs keep the observed ratio near one.  The split-fp16 kernel sums the products BEFORE it stores them as hi + lo,
    # which adds at most 4 U sum |g'| + npix U / 2 against the stored values.
    ref = 0.5 + stored.sum((0, 1, 2))
    mag = np.abs(stored).sum((0, 1, 2))
    ratio = np.abs(got_db.astype(np.float64) - ref) / (U * mag)
    print("leaky_bwd db: %s c=%d npix=%d  max err / (U sum|g'|) = %.3f" % (dtype, c, int(np.prod(nhw)), ratio.max()))
    assert np.all(ratio <= 64.0), float(ratio.max())


# ------------------------------------------------------------------------------------------------ 3. fn2_epe_loss_grad
EPE_D = np.array([(0, 0), (3, 4), (4, 3), (0, 5), (5, 0), (6, 8), (5, 12)], np.float32) / 4   # |d| = 0, 5/4, 10/4, 13/4


@pytest.mark.gpu
@pytest.mark.parametrize("nhw,weighted", [
    ((4, 5, 7), False), ((4, 5, 7), True),           # one partly filled block
    ((2, 64, 80), False), ((2, 64, 80), True),       # 40 blocks
    ((4, 512, 513), False),                          # > 4096 * 256 pixels: the grid-stride loop; d from {0, (3,4)/4}, no
])                                                   # pixel weights, so that the loss stays exact
def test_epe_loss_and_gradient(nhw, weighted):
    from src import _hip
    lib = _hip.lib()
    big = np.prod(nhw) > BIG
    rng = np.random.default_rng(40 + nhw[1])
    label = dyadic(41, nhw + (2,))
    d = EPE_D[rng.integers(0, 2 if big else len(EPE_D), size=nhw)]
    pred = label + d
    np.testing.assert_array_equal(pred.astype(np.float64), label.astype(np.float64) + d)   # pred - label is exactly d
    pw = rng.choice(np.array([0, 0.5, 1, 2], np.float32), size=nhw) if weighted else np.ones(nhw, np.float32)
    weight, grad_mult, n = 0.25, 64.0, nhw[0]
    scale = weight / n                                                    # a power of two
    e = np.sqrt((d.astype(np.float64) ** 2).sum(-1))
    np.testing.assert_array_equal(e * 4, np.round(e * 4))                 # the endpoint error is dyadic
    terms = pw.astype(np.float64) * e
    want_loss = 0.5 + scale * terms.sum()
    exact_ok(0.5 + scale * terms.sum(), scale / 8)                        # terms: multiples of 1/8; the 0.5 of scale / 8
    with np.errstate(invalid="ignore", divide="ignore"):
        want_d = np.where(e[..., None] > 0, grad_mult * scale * pw[..., None] * d / e[..., None], 0.0)
    pd, ld, wd = dev(pred), dev(label), dev(pw)
    npix = int(np.prod(nhw))
    dp, dpp, dfull = guarded(dyadic(42, (2 * npix,)))
    la, lap, lfull = guarded(np.array([0.5], np.float32))
    if weighted:
        rc = lib.fn2_epe_loss_grad_weighted(_hip.ptr(pd), _hip.ptr(ld), _hip.ptr(wd), dpp, lap, nhw[0], nhw[1], nhw[2],
                                            weight, grad_mult, _hip.stream_ptr())
    else:
        rc = lib.fn2_epe_loss_grad(_hip.ptr(pd), _hip.ptr(ld), dpp, lap, nhw[0], nhw[1], nhw[2], weight, grad_mult,
                                   _hip.stream_ptr())
    _hip.check(rc)
    got_loss = guards_ok(la, lfull, 1)
    assert float(got_loss[0]) == want_loss, (float(got_loss[0]), want_loss)
    got = guards_ok(dp, dfull, 2 * npix).reshape(nhw + (2,)).astype(np.float64)
    assert np.isfinite(got).all()
    zero = (e == 0) | (pw == 0)
    assert zero.any() and not zero.all()
    np.testing.assert_array_equal(got[zero], 0.0)                         # d == 0 (never NaN) and zero pixel weight
    # elsewhere: one subtraction (exact here), one correctly rounded divide, three multiplies
    assert np.all(np.abs(got - want_d) <= 8 * U * np.abs(want_d)), float(np.abs(got - want_d).max())
    np.testing.assert_array_equal(host(pd), pred)
    np.testing.assert_array_equal(host(ld), label)


# ------------------------------------------------------------------------------------------------ 4. fn2_upsample_flow_bwd
@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nhw", [(2, 5, 7), (3, 33, 47)])                 # coarse sizes: one block; 19 blocks, odd sizes
@pytest.mark.parametrize("dtype,cs,c0", [("f32", 2, 0), ("f32", 16, 6),   # dense; a slice of a concat gradient buffer
                                         ("f16x2", 16, 6), ("f16x2", 16, 8)])   # the last two of a group; the first two
def test_upsample_flow_bwd_exact(dtype, cs, c0, nhw, accumulate):
    from src import _hip
    lib = _hip.lib()
    N, H, W_ = nhw
    g = dyadic(50, (N, 2 * H, 2 * W_, cs), nonzero=True)
    pf, w = dyadic(51, (N, H, W_, 2), nonzero=True), dyadic(52, (4, 4, 2, 2), nonzero=True)
    dpf0, dw0 = dyadic(53, (N, H, W_, 2)), dyadic(54, (4, 4, 2, 2))
    gs = g[..., c0:c0 + 2]
    dpf_ref, dw_ref = upsample_flow_bwd_ref(gs, pf, w)
    want_dpf = dpf_ref + (dpf0 if accumulate else 0.0)
    want_dw = dw0 + dw_ref
    a_dpf, a_dw = upsample_flow_bwd_ref(np.abs(gs), np.abs(pf), np.abs(w))
    exact_ok(a_dpf + np.abs(dpf0), 1 / 16)
    exact_ok(a_dw + np.abs(dw0), 1 / 16)
    gd, pfd, wd = make_buf(g, dtype), dev(pf), dev(w)
    g_before = host(gd)
    dpf, dpfp, dpf_full = guarded(dpf0)
    dw, dwp, dw_full = guarded(dw0)
    v = _hip.view(gd, 2, c0, code_of(dtype))
    _hip.check(lib.fn2_upsample_flow_bwd(C.byref(v), _hip.ptr(pfd), _hip.ptr(wd), dpfp, dwp, accumulate, _hip.stream_ptr()))
    np.testing.assert_array_equal(guards_ok(dpf, dpf_full, dpf0.size).reshape(dpf0.shape).astype(np.float64), want_dpf)
    np.testing.assert_array_equal(guards_ok(dw, dw_full, 64).reshape(4, 4, 2, 2).astype(np.float64), want_dw)
    np.testing.assert_array_equal(bits_of(host(gd), dtype), bits_of(g_before, dtype))
    np.testing.assert_array_equal(host(pfd), pf)
    np.testing.assert_array_equal(host(wd), w)


# ------------------------------------------------------------------------------------------------ 5. the flow heads
def head_pads(cin):
    cin_pad = (cin + 7) // 8 * 8 + 8
    return cin_pad, 9 * cin_pad + 32


@pytest.mark.gpu
@pytest.mark.parametrize("nhw", [(2, 6, 8),          # 96 pixels: 3 pixel ranges of 32, a range straddles the two images
                                 (1, 37, 53)])       # 1961 pixels: 62 ranges of 32, the last one partly filled
@pytest.mark.parametrize("dtype,cin,cs,c0", [("f32", 72, 80, 4),       # two channel blocks, the second with 8 channels
                                             ("f32", 194, 200, 4),     # view padded to exactly 196: a ragged last float4
                                             ("f16x2", 72, 80, 8),
                                             ("f16x2", 194, 200, 4)])  # half-group offset, ragged last half group
def test_head_bwd_filter_exact(dtype, cin, cs, c0, nhw):
    from src import _hip
    lib = _hip.lib()
    x = dyadic(60 + cin, nhw + (cs,), nonzero=True)      # pad channels hold dyadic garbage that must not reach dw
    g = dyadic(61, nhw + (2,), nonzero=True)
    cin_pad, kpad = head_pads(cin)
    dw0 = dyadic(62, (2, kpad))
    xs = x[..., c0:c0 + cin]
    want, fg = dw0.astype(np.float64), filter_grad(xs, g)
    for o in range(2):                                   # dw[o * kpad + tap * cin_pad + ci]
        want[o, :9 * cin_pad].reshape(3, 3, cin_pad)[..., :cin] += fg[..., o]
    assert np.abs(want - dw0).max() > 0 and np.shares_memory(want, want[0, :9 * cin_pad].reshape(3, 3, cin_pad))
    exact_ok(filter_grad(np.abs(xs), np.abs(g)).max() + 2.0, 1 / 16)
    xd, gd = make_buf(x, dtype), dev(g)
    x_before = host(xd)
    dw, dwp, full = guarded(dw0)
    v = _hip.view(xd, cin, c0, code_of(dtype))
    _hip.check(lib.fn2_head_bwd_filter(C.byref(v), _hip.ptr(gd), dwp, cin_pad, kpad, _hip.stream_ptr()))
    # the whole of dw: rows beyond cin and everything behind the last tap come back as they were
    np.testing.assert_array_equal(guards_ok(dw, full, 2 * kpad).reshape(2, kpad).astype(np.float64), want)
    np.testing.assert_array_equal(bits_of(host(xd), dtype), bits_of(x_before, dtype))
    np.testing.assert_array_equal(host(gd), g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,cin,cs,c0,nhw", [
    ("f32", 194, 200, 4, (2, 6, 8)), ("f32", 194, 200, 4, (1, 37, 53)),          # ragged last float4, scalar adds
    ("f16x2", 194, 200, 4, (2, 6, 8)), ("f16x2", 194, 200, 4, (1, 37, 53)),      # ragged last half group, rewritten whole
    ("f16x2", 72, 80, 8, (2, 6, 8)), ("f16x2", 72, 80, 8, (1, 37, 53)),
    ("f32", 194, 200, 4, (2, 96, 128)), ("f16x2", 194, 200, 4, (2, 96, 128)),    # 49 * 24576 > 4096 * 256: grid-stride loop
])
def test_head_bwd_data_exact(dtype, cin, cs, c0, nhw):
    from src import _hip
    lib = _hip.lib()
    cin_pad, kpad = head_pads(cin)
    g = dyadic(70, nhw + (2,), nonzero=True)
    wp = dyadic(71, (2, kpad), nonzero=True)            # rows beyond cin hold garbage that must not reach dx
    w = wp[:, :9 * cin_pad].reshape(2, 3, 3, cin_pad)[..., :cin].transpose(1, 2, 3, 0)      # HWIO
    dx0 = dyadic(72, nhw + (cs,))
    want = dx0.astype(np.float64)
    want[..., c0:c0 + cin] += head_bwd_data_ref(g, w)
    bound = head_bwd_data_ref(np.abs(g), np.abs(w)) + 2.0
    exact_ok(bound, 1 / 16, 22 if dtype == "f16x2" else 24)
    gd, wd, dxd = dev(g), dev(wp), make_buf(dx0, dtype)
    dx_before = host(dxd)
    v = _hip.view(dxd, cin, c0, code_of(dtype))
    _hip.check(lib.fn2_head_bwd_data(_hip.ptr(gd), _hip.ptr(wd), C.byref(v), cin_pad, kpad, _hip.stream_ptr()))
    dx_after = host(dxd)
    np.testing.assert_array_equal(logical(dx_after, dtype), want)
    assert_outside_unchanged(dx_before, dx_after, dtype, cin, c0)        # pad channels of the view included
    np.testing.assert_array_equal(host(gd), g)
    np.testing.assert_array_equal(host(wd), wp)


@pytest.mark.gpu
def test_head_g18_grid_stride():
    """2 x 384 x 512 pixels x 3 groups > 4096 * 256 work items: the slicing check of
    tests/test_gpu_bwd_ops.py::test_flow_head_gradients_through_g18 on dyadic g, exact."""
    from src import _hip
    lib = _hip.lib()
    import torch
    N, H, W_ = 2, 384, 512
    assert N * H * W_ * 3 > BIG
    g = dyadic(80, (N, H, W_, 2), nonzero=True)
    sentinel = split(np.full((1, 32), 1.5, np.float32))
    g18 = dev(sentinel).repeat(N * H * W_, 1).reshape(N, H, W_, 32).contiguous()
    gd = dev(g)
    v18 = _hip.view(g18, 18, 0, 3)
    _hip.check(lib.fn2_head_g18(_hip.ptr(gd), C.byref(v18), _hip.stream_ptr()))
    torch.cuda.synchronize()
    bits = x2_bits(host(g18))
    t = bits[..., 0].view(np.float16)
    assert not bits[..., :24, 1].any()                                   # zero lo parts
    gp = np.zeros((N, H + 2, W_ + 2, 2), np.float16)
    gp[:, 1:-1, 1:-1] = g
    for tap in range(9):
        ky, kx = divmod(tap, 3)
        np.testing.assert_array_equal(t[..., tap * 2:tap * 2 + 2], gp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W_])
    assert not t[..., 18:24].any()
    np.testing.assert_array_equal(bits[..., 24:, :], np.broadcast_to(x2_bits(sentinel)[0, 24:], bits[..., 24:, :].shape))


# ------------------------------------------------------------------------------------------------ 6. Adam
B1, B2, EPS, L2, LR, GSCALE = 0.9, 0.999, 1e-8, 4e-4, 1e-4, 0.125


def adam_inputs(seed, n):
    """w normal, every fifth element 0 as a zero-initialised bias is: there w' is the update alone and the bound on w'
    is 16 U |update|, which resolves lr_t (elsewhere 2 U |w| hides it); g and m of one sign per element and bounded away
    from 0 (no cancellation in m' or g'); v >= 0."""
    rng = np.random.default_rng(seed)
    sign = rng.choice(np.array([-1.0, 1.0]), size=n)
    w = rng.standard_normal(n).astype(np.float32)
    w[::5] = 0.0
    g = (sign * rng.uniform(4.0, 16.0, n)).astype(np.float32)           # times grad_scale = 1/8: 0.5 .. 2 >> l2 |w|
    m = (sign * rng.uniform(0.1, 1.0, n)).astype(np.float32)
    v = rng.uniform(0.0, 1.0, n).astype(np.float32)
    v[::7] = 0.0
    return w, m, v, g


def check_adam(got_w, got_m, got_v, w, m, v, g, lr_t, l2):
    """m' within 4 U (two products, the g' expression, one sum), v' within 6 U (g' enters twice), and
    |w' - ref| <= 2 U |w| + 16 U |update| (m', the root of v', eps, one correctly rounded divide, lr_t, the difference)."""
    rw, rm, rv, upd = adam_ref(w, m, v, g, lr_t, B1, B2, EPS, l2, GSCALE)
    assert np.all(np.abs(got_m - rm) <= 4 * U * np.abs(rm)), float((np.abs(got_m - rm) / np.abs(rm)).max() / U)
    assert np.all(np.abs(got_v - rv) <= 6 * U * np.abs(rv)), float((np.abs(got_v - rv) / np.abs(rv)).max() / U)
    tol = 2 * U * np.abs(w.astype(np.float64)) + 16 * U * np.abs(upd)
    assert np.all(np.abs(got_w - rw) <= tol), float((np.abs(got_w - rw) / tol).max())


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("n", [1, 1000, BIG + 5])       # one thread; four blocks; the grid-stride loop
def test_adam_step(n, step):
    from src import _hip
    lib = _hip.lib()
    w, m, v, g = adam_inputs(90 + step, n)
    bufs = [guarded(a) for a in (w, m, v, g)]
    _hip.check(lib.fn2_adam_step(bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], n, LR, B1, B2, EPS, step, L2, GSCALE,
                                 _hip.stream_ptr()))
    got = [guards_ok(t, full, n) for t, _, full in bufs]
    np.testing.assert_array_equal(got[3], g)
    check_adam(got[0], got[1], got[2], w, m, v, g, adam_lr_t(LR, B1, B2, step), L2)


# (n, l2, split-fp16 copy, scale, frag_k).  A tensor without a copy carries a null pointer in the table: the kernel must
# skip it (a store through it would fault), and its scale word is not read.
ADAM_TENSORS = [
    (2, 0.0, None, 1.0, 0),                      # shorter than a float4
    (3, 0.0, None, 1.0, 0),                      # scalar tail only
    (4, L2, None, 1.0, 0),                       # one float4, no tail
    (135, L2, "row", 1.0, 0),                    # body and tail into a row-major copy; element 135 of the last group untouched
    (128 * 256 * 4 + 8, L2, "row", 8.0, 0),      # the second sweep of a row's 128 blocks
    (64 * 96, L2, "frag", 32.0, 96),             # MFMA-fragment order, 64 rows of k = 96
]


def adam_arena(seed):
    """All tensors in one fp32 arena and their copies in one split-fp16 arena, each 32-byte aligned (a split-fp16 group),
    with eight dyadic guard words in front of, between and behind them.  Returns the host arrays and word offsets."""
    fl, xl, offs = [], [], []
    fpos = xpos = 0

    def put(lst, pos, a):
        lst.append(np.full(8, -2.25, np.float32)); pos += 8
        at = pos
        lst.append(a); pos += a.size
        pad = -pos % 8
        lst.append(np.full(pad, -2.25, np.float32)); pos += pad
        return at, pos

    for t, (n, l2, copy, scale, frag_k) in enumerate(ADAM_TENSORS):
        o = {}
        for name, a in zip("wmvg", adam_inputs(seed + t, n)):
            o[name], fpos = put(fl, fpos, a)
        if copy is not None:
            o["x"], xpos = put(xl, xpos, np.full((n + 7) // 8 * 8, 1.5, np.float32))   # container words as sentinels
        offs.append(o)
    fl.append(np.full(8, -2.25, np.float32))
    xl.append(np.full(8, -2.25, np.float32))
    return np.concatenate(fl), np.concatenate(xl), offs


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 7])
def test_adam_step_multi_and_its_weight_copies(step):
    from src import _hip
    lib = _hip.lib()
    import torch
    farena, xarena, offs = adam_arena(100 + step)
    fd, xd = dev(farena), dev(xarena)
    assert fd.data_ptr() % 32 == 0 and xd.data_ptr() % 32 == 0
    rows = []
    for (n, l2, copy, scale, frag_k), o in zip(ADAM_TENSORS, offs):
        wx2 = xd.data_ptr() + 4 * o["x"] if copy is not None else 0
        bits = int(np.float32(scale).view(np.uint32)) | (int(frag_k) << 32)     # as Trainer._build_optim_tables
        rows.append([fd.data_ptr() + 4 * o[k] for k in "wmvg"] + [wx2, bits])
        assert all(p % 16 == 0 for p in rows[-1][:5])
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    counts = torch.tensor([t[0] for t in ADAM_TENSORS], dtype=torch.int64, device="cuda")
    l2s = torch.tensor([t[1] for t in ADAM_TENSORS], dtype=torch.float32, device="cuda")
    lr_t = adam_lr_t(LR, B1, B2, step)
    hyper = dev(np.array([lr_t, B1, B2, EPS, GSCALE, 0.0, 0.0, 0.0], np.float32))
    _hip.check(lib.fn2_optim_step_multi_dev(_hip.OPTIM_KINDS["adam"], _hip.ptr(table), _hip.ptr(counts), _hip.ptr(l2s), len(rows),
                                            _hip.ptr(hyper), None, _hip.stream_ptr()))
    fgot, xgot = host(fd), host(xd)
    touched_f, touched_x = np.zeros(farena.size, bool), np.zeros(xarena.size, bool)
    for (n, l2, copy, scale, frag_k), o in zip(ADAM_TENSORS, offs):
        inp = {k: farena[o[k]:o[k] + n] for k in "wmvg"}
        out = {k: fgot[o[k]:o[k] + n] for k in "wmvg"}
        for k in "wmv":
            touched_f[o[k]:o[k] + n] = True
        np.testing.assert_array_equal(out["g"], inp["g"])
        check_adam(out["w"], out["m"], out["v"], inp["w"], inp["m"], inp["v"], inp["g"], lr_t, l2)
        if copy is None:
            continue
        # the copy is bit-equal to what the library's own converter writes for the updated master: both run the same
        # multiply by the scale and the same two conversions
        n8 = (n + 7) // 8 * 8
        src = np.zeros(n8, np.float32)
        src[:n] = out["w"]
        srcd, dstd = dev(src), dev(np.full(n8, 1.5, np.float32))
        if copy == "frag":
            rc = lib.fn2_to_f16x2_frag(_hip.ptr(dstd), _hip.ptr(srcd), None, n8, scale, frag_k, _hip.stream_ptr())
        else:
            rc = lib.fn2_to_f16x2(_hip.ptr(dstd), _hip.ptr(srcd), None, n8, scale, _hip.stream_ptr())
        _hip.check(rc)
        want_bits, got_bits = x2_bits(host(dstd)), x2_bits(xgot[o["x"]:o["x"] + n8])
        if copy == "frag":
            np.testing.assert_array_equal(got_bits, want_bits)            # a permutation of chunks: compare the image
            touched_x[o["x"]:o["x"] + n8] = True
        else:
            np.testing.assert_array_equal(got_bits[:n], want_bits[:n])
            sent = x2_bits(xarena[o["x"]:o["x"] + n8])
            np.testing.assert_array_equal(got_bits[n:], sent[n:])         # elements behind n of the last group: untouched
            touched_x[o["x"]:o["x"] + n8] = True
        # and the copy holds the scaled master to split-fp16 precision
        val = x2_join(host(dstd))
        if copy == "row":
            ref = out["w"].astype(np.float64) * scale
            assert np.all(np.abs(val[:n] - ref) <= 2.0 ** -22 * np.abs(ref) + 2.0 ** -25)
    np.testing.assert_array_equal(fgot[~touched_f].view(np.uint32), farena[~touched_f].view(np.uint32))   # guards, g
    np.testing.assert_array_equal(xgot[~touched_x].view(np.uint32), xarena[~touched_x].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 7. copies, conversions
def make_map(seed, n, n_src):
    """Permutes, repeats and holds -1 entries (which give 0)."""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, n_src, size=n).astype(np.int32)                   # repeats
    m[:min(n, n_src)] = rng.permutation(n_src)[:min(n, n_src)]            # a permuted stretch
    m[rng.random(n) < 0.2] = -1
    m[n // 2] = -1
    return m


def gathered(src, m, n):
    if m is None:
        return src[:n]
    return np.where(m >= 0, src[np.maximum(m, 0)], np.float32(0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -4])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n", [8, 8 * (BIG + 3)])       # one group; more groups than threads: the grid-stride loop
def test_to_f16x2(n, mapped, scale):
    from src import _hip
    lib = _hip.lib()
    m = make_map(110, n, n) if mapped else None
    md = dev(m) if mapped else None
    for kind in ("dyadic", "normal"):
        src = dyadic(111, (n,), nonzero=True) if kind == "dyadic" else \
            np.random.default_rng(112).standard_normal(n).astype(np.float32)
        srcd = dev(src)
        dst, dstp, full = guarded(np.full(n, 1.5, np.float32))
        _hip.check(lib.fn2_to_f16x2(dstp, _hip.ptr(srcd), _hip.ptr(md) if mapped else None, n, scale, _hip.stream_ptr()))
        got = x2_join(guards_ok(dst, full, n))
        want = gathered(src, m, n).astype(np.float64) * scale             # a power of two: exact
        if kind == "dyadic":
            np.testing.assert_array_equal(got, want)                      # multiples of 1/64 up to 2: 11 bits
        else:
            assert np.all(np.abs(got - want) <= 2.0 ** -22 * np.abs(want) + 2.0 ** -25)
        np.testing.assert_array_equal(host(srcd), src)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 8 * (BIG + 3)])
def test_gather_f32(n):
    from src import _hip
    lib = _hip.lib()
    n_src = max(5, n // 2)
    src, m = dyadic(120, (n_src,), nonzero=True), make_map(121, n, n_src)
    srcd, md = dev(src), dev(m)
    dst, dstp, full = guarded(np.full(n, 1.5, np.float32))
    _hip.check(lib.fn2_gather_f32(dstp, _hip.ptr(srcd), _hip.ptr(md), n, _hip.stream_ptr()))
    np.testing.assert_array_equal(guards_ok(dst, full, n), gathered(src, m, n))
    np.testing.assert_array_equal(host(srcd), src)


@pytest.mark.gpu
@pytest.mark.parametrize("c,cs,c0,nhw", [(441, 476, 32, (2, 12, 16)),     # FlowNetC's correlation slice
                                         (1, 3, 2, (1, 1, 1)),            # the last channel of one pixel
                                         (441, 476, 32, (2, 40, 32))])    # npix * c > 4096 * 256: the grid-stride loop
def test_slice_copy_f32(c, cs, c0, nhw):
    from src import _hip
    lib = _hip.lib()
    src = dyadic(130, nhw + (cs,), nonzero=True)
    n = int(np.prod(nhw)) * c
    srcd = dev(src)
    dst, dstp, full = guarded(np.full(n, 1.5, np.float32))
    v = _hip.view(srcd, c, c0, 0)
    _hip.check(lib.fn2_slice_copy_f32(C.byref(v), dstp, _hip.stream_ptr()))
    np.testing.assert_array_equal(guards_ok(dst, full, n), src[..., c0:c0 + c].ravel())
    np.testing.assert_array_equal(host(srcd), src)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 7, 4 * BIG + 6])     # tail only; tail; body only; both; grid-stride body + tail
def test_add_f32(n):
    from src import _hip
    lib = _hip.lib()
    a, b = dyadic(140, (n,)), dyadic(141, (n,), nonzero=True)
    exact_ok(4.0, 0.25)
    dst, dstp, full = guarded(a)
    bd = dev(b)
    _hip.check(lib.fn2_add_f32(dstp, _hip.ptr(bd), n, _hip.stream_ptr()))
    np.testing.assert_array_equal(guards_ok(dst, full, n), a + b)          # elements after n stay unchanged
    np.testing.assert_array_equal(host(bd), b)


# ------------------------------------------------------------------------------------------------ validation
@pytest.mark.gpu
def test_bad_arguments_are_refused_without_a_launch():
    from src import _hip
    lib = _hip.lib()
    bad, st = _hip.ERR_INVALID_ARGUMENT, _hip.stream_ptr()
    a = dyadic(150, (1, 4, 6, 16), nonzero=True)
    yd, gd, xd = dev(a), dev(a + 1), dev(split(a))
    out, outp, full = guarded(np.full(4096, 1.5, np.float32))
    f32, x2 = 0, 3
    V = lambda t, c, c0=0, code=f32, h=None: _hip.Fn2Tensor(t.data_ptr(), code, 1, 4 if h is None else h, 6, c, 16, c0)
    by = C.byref
    assert lib.fn2_leaky_bwd(by(V(yd, 6)), by(V(gd, 6)), outp, st) == bad                  # c % 4 != 0
    assert lib.fn2_leaky_bwd(by(V(yd, 8)), by(V(xd, 8, 0, x2)), outp, st) == bad           # unequal dtypes
    assert lib.fn2_leaky_bwd(by(V(yd, 8)), by(V(gd, 8, h=2)), outp, st) == bad             # shape mismatch
    assert lib.fn2_leaky_bwd(by(V(yd, 8)), by(V(gd, 4)), outp, st) == bad                  # channel count mismatch
    assert lib.fn2_bias_grad(by(V(xd, 12, 0, x2)), outp, st) == bad                        # split fp16: c = 12
    small = dev(dyadic(151, (64,)))
    assert lib.fn2_upsample_flow_bwd(by(V(gd, 2, h=3)), _hip.ptr(small), _hip.ptr(small), outp, outp, 0, st) == bad   # odd h
    assert lib.fn2_upsample_flow_bwd(by(V(gd, 4)), _hip.ptr(small), _hip.ptr(small), outp, outp, 0, st) == bad        # c != 2
    assert lib.fn2_head_bwd_data(_hip.ptr(small), _hip.ptr(small), by(V(yd, 6)), 6, 9 * 6, st) == bad    # cin_pad % 4 != 0
    assert lib.fn2_to_f16x2(outp, _hip.ptr(small), None, 12, 1.0, st) == bad               # n % 8 != 0
    assert lib.fn2_adam_step(outp, outp, outp, _hip.ptr(small), 8, LR, B1, B2, EPS, 0, L2, 1.0, st) == bad   # step = 0
    with pytest.raises(ValueError):
        _hip.check(bad)
    np.testing.assert_array_equal(host(out), full)                                         # nothing was launched
    np.testing.assert_array_equal(host(gd), a + 1)
    np.testing.assert_array_equal(host(small), dyadic(151, (64,)))
