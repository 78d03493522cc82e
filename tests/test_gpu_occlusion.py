"""The forward-backward occlusion check (csrc/occlusion.hip, src/occlusion.py, Net.test / test_batch `occlusions`)
against a float64 NumPy restatement of the reference's tf_warp / occlusion (src/utils.py:453-538).

Method, as in test_gpu_train_ops.py: flows are multiples of 1/2 -- a per-image integer translation in [-2, 2]^2 (negated
for the backward flow) plus a half-integer bump in [-3, 3] on about 35 % of the pixels.  The weight factors are then
multiples of 1/2, the weights multiples of 1/4, the warped values multiples of 1/8, and d = |fw + warp(bw)|^2 and
mag = |fw|^2 + |warp(bw)|^2 multiples of 1/64 far below 2^24 quanta: everything up to d and mag is exact in fp32 in any
order, with or without FMA contraction.  Every exact test asserts that precondition on the float64 reference and compares
with assert_array_equal.  With the dyadic alpha = 1/64 the threshold is exact as well; with the reference's 0.01 it
carries at most three roundings, and the test first shows on the reference that no pixel is that close to its threshold."""
import ctypes as C
import os

import numpy as np
import pytest

U = 2.0 ** -24

SHAPES = [(2, 5, 7),      # general small case
          (1, 3, 70),     # crosses a wave
          (2, 6, 130),    # general, wider than two waves
          (1, 1, 1),      # every tap clamped
          (2, 9, 1),      # 1-wide image
          (1, 1, 9)]      # 1-high image
LARGER = SHAPES[:3]


# ------------------------------------------------------------------------------------------------ the reference
def tf_warp_ref(img, flow, dt=np.float64):            # reference utils.py:453-515
    img, flow = img.astype(dt), flow.astype(dt)
    n, h, w, c = img.shape
    gx, gy = np.meshgrid(np.arange(w, dtype=dt), np.arange(h, dtype=dt))
    x, y = gx[None] + flow[..., 0], gy[None] + flow[..., 1]
    tx = np.clip(np.trunc(x), -2, w + 1).astype(np.int64)   # clip first: the cast of a huge float is undefined in NumPy
    ty = np.clip(np.trunc(y), -2, h + 1).astype(np.int64)
    x0, x1 = np.clip(tx, 0, w - 1), np.clip(tx + 1, 0, w - 1)
    y0, y1 = np.clip(ty, 0, h - 1), np.clip(ty + 1, 0, h - 1)
    b = np.arange(n)[:, None, None]
    Ia, Ib, Ic, Id = img[b, y0, x0], img[b, y1, x0], img[b, y0, x1], img[b, y1, x1]
    x0f, x1f, y0f, y1f = (a.astype(dt) for a in (x0, x1, y0, y1))
    wa, wb = (x1f - x) * (y1f - y), (x1f - x) * (y - y0f)
    wc, wd = (x - x0f) * (y1f - y), (x - x0f) * (y - y0f)
    return ((wa[..., None] * Ia + wb[..., None] * Ib) + wc[..., None] * Ic) + wd[..., None] * Id


def occlusion_ref(fw, bw, alpha=0.01, beta=0.5, dt=np.float64):   # utils.py:519-538
    bww, fww = tf_warp_ref(bw, fw, dt), tf_warp_ref(fw, bw, dt)
    fw, bw = fw.astype(dt), bw.astype(dt)
    lsq = lambda v: np.sum(v * v, axis=3, keepdims=True)
    d_fw, d_bw = lsq(fw + bww), lsq(bw + fww)
    t_fw, t_bw = dt(alpha) * (lsq(fw) + lsq(bww)) + dt(beta), dt(alpha) * (lsq(bw) + lsq(fww)) + dt(beta)
    return d_fw > t_fw, d_bw > t_bw, (d_fw, t_fw, d_bw, t_bw, bww, fww)


# ------------------------------------------------------------------------------------------------ inputs
def dyadic_flows(seed, shape):
    """(fw, bw) float32 [n,h,w,2], multiples of 1/2 with |component| <= 5."""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    shift = rng.integers(-2, 3, size=(n, 1, 1, 2)).astype(np.float64)

    def bump():
        k = rng.integers(-6, 7, size=(n, h, w, 2)) / 2.0
        return np.where(rng.random((n, h, w, 1)) < 0.35, k, 0.0)

    return (shift + bump()).astype(np.float32), (-shift + bump()).astype(np.float32)


def dyadic_image(seed, shape, c):
    """float32 [n,h,w,c], multiples of 1/2 in [-4, 4]."""
    n, h, w = shape
    return (np.random.default_rng(seed).integers(-8, 9, size=(n, h, w, c)) / 2.0).astype(np.float32)


def warp_exact_ok(img, flow):
    """A coordinate leaves the image by at most max|flow|, so a weight factor is at most max|flow| + 1 and the four
    products sum to at most 4 (max|flow| + 1)^2 max|img|, in quanta of 1/8: below 2^24 -> the warp is exact in fp32."""
    f, m = float(np.abs(flow).max()), float(np.abs(img).max())
    assert np.all(flow * 2 == np.round(flow * 2)) and np.all(img * 2 == np.round(img * 2))
    assert 4 * (f + 1) ** 2 * m * 8 < 2.0 ** 24


def occlusion_exact_ok(fw, bw, parts):
    """d and mag are multiples of 1/64 below 2^17 quanta (and every term of them is bounded by them)."""
    warp_exact_ok(bw, fw)
    warp_exact_ok(fw, bw)
    d_fw, _, d_bw, _, bww, fww = parts
    lsq = lambda v: np.sum(v * v, axis=3, keepdims=True)
    for v in (d_fw, d_bw, lsq(fw.astype(np.float64)) + lsq(bww), lsq(bw.astype(np.float64)) + lsq(fww)):
        assert np.all(v * 64 == np.round(v * 64)) and float(v.max()) * 64 < 2.0 ** 17


def quirk_cases():
    """Hand-written rows for tf_warp's index rules on the 4 x 6 image I[y, x] = 10 (y + 1) + (x + 1): one image per case,
    zero flow except at one pixel.  Returns (img [k,4,6,1], flow [k,4,6,2], expected [k,4,6,1]).  A zero flow maps a pixel
    to itself -- except in the last row and the last column, where both taps clamp to one index and the result is 0."""
    h, w = 4, 6
    base = (10.0 * (np.arange(h)[:, None] + 1) + (np.arange(w)[None, :] + 1))
    still = base.copy()
    still[-1, :] = 0.0
    still[:, -1] = 0.0
    cases = [  # (py, px, u, v, expected)
        (1, 0, -0.5, 0.0, 1.5 * 21 - 0.5 * 22),    # x = -0.5: truncates to 0, extrapolates from columns 0 and 1
        (1, 0, -1.5, 0.0, 0.0),                    # x = -1.5: taps -1 and 0 both clamp to 0, weights 1.5 and -1.5 cancel
        (1, 2, 3.0, 0.0, 0.0),                     # x = W - 1 exactly: taps W-1 and W clamp to W-1, both weights 0
        (1, 3, 6.0, 0.0, 0.0),                     # x = W + 3: weights -4 and 4 on the same tap
        (1, 2, 0.5, 0.0, 0.5 * 23 + 0.5 * 24),     # an ordinary interior sample
        (0, 2, 0.0, -0.5, 1.5 * 13 - 0.5 * 23),    # the same in y
        (0, 2, 0.0, -1.5, 0.0),
        (1, 2, 0.0, 2.0, 0.0),                     # y = H - 1 exactly
        (1, 2, 0.0, 6.0, 0.0),                     # y = H + 3
        (2, 1, -0.25, 0.0, 0.25 * 31 + 0.75 * 32),  # x = 0.75: interior
        (2, 0, -0.25, 0.0, 1.25 * 31 - 0.25 * 32),  # x = -0.25: weights 1.25 and -0.25 on columns 0 and 1
    ]
    k = len(cases)
    img = np.broadcast_to(base[None, :, :, None], (k, h, w, 1)).astype(np.float32).copy()
    flow = np.zeros((k, h, w, 2), np.float32)
    want = np.broadcast_to(still[None, :, :, None], (k, h, w, 1)).astype(np.float64).copy()
    for i, (py, px, u, v, e) in enumerate(cases):
        flow[i, py, px] = (u, v)
        want[i, py, px, 0] = e
    return img, flow, want


def tap_hits(flag, flow):
    """[n,h,w] bool: one of the four taps of the pixel displaced by `flow` (finite) lands on a flagged pixel."""
    n, h, w = flag.shape
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = gx[None] + flow[..., 0], gy[None] + flow[..., 1]
    tx, ty = np.clip(np.trunc(x), -2, w + 1).astype(np.int64), np.clip(np.trunc(y), -2, h + 1).astype(np.int64)
    x0, x1 = np.clip(tx, 0, w - 1), np.clip(tx + 1, 0, w - 1)
    y0, y1 = np.clip(ty, 0, h - 1), np.clip(ty + 1, 0, h - 1)
    b = np.arange(n)[:, None, None]
    return flag[b, y0, x0] | flag[b, y1, x0] | flag[b, y0, x1] | flag[b, y1, x1]


def poisoned_case(shape, alpha, beta):
    """Dyadic flows with NaN, +-inf and +-1e30 in a few pixels each.  Returns (fw, bw, check, want_fw, want_bw): `check`
    [n,h,w] marks the pixels that neither are poisoned nor read a poisoned pixel in either direction; there the reference
    on the poisoned flows equals the reference on the flows with the poison taken out (asserted), exactly."""
    import warnings
    n, h, w = shape
    fw, bw = dyadic_flows(21, shape)
    rng = np.random.default_rng(22)
    poison = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    bad = {}
    for name, f in (("fw", fw), ("bw", bw)):
        flag = np.zeros((n, h, w), bool)
        for k, v in enumerate(poison):
            i, y, x = rng.integers(n), rng.integers(h), rng.integers(w)
            f[i, y, x, k % 2] = v
            flag[i, y, x] = True
        bad[name] = flag
    clean_fw = np.where(bad["fw"][..., None], 0, fw).astype(np.float32)
    clean_bw = np.where(bad["bw"][..., None], 0, bw).astype(np.float32)
    own = bad["fw"] | bad["bw"]
    check = ~(own | tap_hits(bad["bw"], clean_fw) | tap_hits(bad["fw"], clean_bw))     # the same set serves both masks
    assert check.mean() > 0.5 and not check.all()
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want_fw, want_bw, _ = occlusion_ref(fw, bw, alpha, beta)
    ref_fw, ref_bw, parts = occlusion_ref(clean_fw, clean_bw, alpha, beta)
    occlusion_exact_ok(clean_fw, clean_bw, parts)
    assert np.array_equal(ref_fw[check], want_fw[check]) and np.array_equal(ref_bw[check], want_bw[check])
    return fw, bw, check, want_fw, want_bw


# ------------------------------------------------------------------------------------------------ device helpers
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from src import _hip
    return _hip


# ------------------------------------------------------------------------------------------------ 1. tf_warp
@pytest.mark.gpu
@pytest.mark.parametrize("c", [1, 2, 3, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_tf_warp_equals_the_reference(shape, c):
    from src.occlusion import tf_warp
    img, (flow, _) = dyadic_image(5 + c, shape, c), dyadic_flows(11, shape)
    warp_exact_ok(img, flow)
    want = tf_warp_ref(img, flow)
    got = tf_warp(img, flow)                                    # NumPy in, NumPy out
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == img.shape
    np.testing.assert_array_equal(got.astype(np.float64), want)
    got = tf_warp(dev(img), dev(flow))                          # device in, device out
    assert got.is_cuda
    np.testing.assert_array_equal(host(got).astype(np.float64), want)


@pytest.mark.gpu
@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 6, 130), (2, 9, 1)])
def test_tf_warp_reads_a_pitched_view_in_place(shape, c):
    """Image and flow are crops of larger buffers whose surround is NaN: a tap outside the crop poisons the result."""
    import torch
    from src import occlusion as occ
    n, h, w = shape
    img, (flow, _) = dyadic_image(3, shape, c), dyadic_flows(12, shape)
    big_i = torch.full((n + 1, h + 3, w + 5, c), float("nan"), device="cuda")
    big_f = torch.full((n + 1, h + 2, w + 4, 2), float("nan"), device="cuda")
    vi, vf = big_i[:n, 1:1 + h, 2:2 + w], big_f[:n, 2:2 + h, 1:1 + w]
    vi.copy_(dev(img))
    vf.copy_(dev(flow))
    assert not vi.is_contiguous() and not vf.is_contiguous()
    assert occ._in_place(vi)[0].data_ptr() == vi.data_ptr() and occ._in_place(vf, even=True)[0].data_ptr() == vf.data_ptr()
    got = host(occ.tf_warp(vi, vf))
    np.testing.assert_array_equal(got.astype(np.float64), tf_warp_ref(img, flow))
    assert torch.isnan(big_i[n]).all() and torch.isnan(big_f[n]).all()       # read-only inputs stay as they were


@pytest.mark.gpu
def test_tf_warp_quirk_rows_by_hand():
    from src.occlusion import tf_warp
    img, flow, want = quirk_cases()
    np.testing.assert_array_equal(tf_warp(img, flow).astype(np.float64), want)


# ------------------------------------------------------------------------------------------------ 2. / 3. occlusion
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_occlusion_dyadic_threshold_is_exact(shape, seed):
    from src.occlusion import occlusion
    fw, bw = dyadic_flows(seed, shape)
    alpha, beta = 1.0 / 64, 0.5
    want_fw, want_bw, parts = occlusion_ref(fw, bw, alpha, beta)
    occlusion_exact_ok(fw, bw, parts)                           # then t = mag / 64 + 1/2 is exact too
    got_fw, got_bw = occlusion(fw, bw, alpha=alpha, beta=beta)
    assert got_fw.dtype == np.float32 and got_fw.shape == fw.shape[:3] + (1,) and got_bw.shape == got_fw.shape
    np.testing.assert_array_equal(got_fw, want_fw.astype(np.float32))
    np.testing.assert_array_equal(got_bw, want_bw.astype(np.float32))
    u_fw, u_bw = occlusion(dev(fw), dev(bw), alpha=alpha, beta=beta, as_uint8=True)
    assert u_fw.is_cuda and host(u_fw).dtype == np.uint8
    np.testing.assert_array_equal(host(u_fw), want_fw.astype(np.uint8) * 255)
    np.testing.assert_array_equal(host(u_bw), want_bw.astype(np.uint8) * 255)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_occlusion_reference_constants(shape, seed):
    """alpha = 0.01: d and mag are still exact; t = fl(fl(alpha) * mag) + 0.5 carries at most three roundings (alpha, the
    product, the sum -- or two with a fused multiply-add), an error <= 4 U (1 + t).  The inputs keep every pixel at least
    2^-18 (1 + t) away from its threshold, 2^4 times that, so the comparison cannot flip."""
    from src.occlusion import occlusion
    fw, bw = dyadic_flows(seed, shape)
    want_fw, want_bw, parts = occlusion_ref(fw, bw)
    occlusion_exact_ok(fw, bw, parts)
    d_fw, t_fw, d_bw, t_bw = parts[:4]
    margin = min(float((np.abs(d_fw - t_fw) / (1 + t_fw)).min()), float((np.abs(d_bw - t_bw) / (1 + t_bw)).min()))
    print("shape %s seed %d: smallest margin %.3e, occluded share %.2f / %.2f" % (shape, seed, margin, want_fw.mean(), want_bw.mean()))
    assert margin > 2.0 ** -18 > 4 * U
    if shape in LARGER:
        for m in (want_fw, want_bw):
            assert m.any() and not m.all()                      # both mask values occur
    got_fw, got_bw = occlusion(fw, bw)
    np.testing.assert_array_equal(got_fw, want_fw.astype(np.float32))
    np.testing.assert_array_equal(got_bw, want_bw.astype(np.float32))
    u_fw, u_bw = occlusion(fw, bw, as_uint8=True)
    np.testing.assert_array_equal(u_fw, want_fw.astype(np.uint8) * 255)
    np.testing.assert_array_equal(u_bw, want_bw.astype(np.uint8) * 255)


@pytest.mark.gpu
def test_occlusion_reads_two_slices_of_one_padded_buffer():
    """The layout Net._infer_pairs hands over: directions interleaved along the batch, cropped from a padded buffer."""
    import torch
    from src import occlusion as occ
    shape = (2, 6, 130)
    fw, bw = dyadic_flows(7, shape)
    n, h, w = shape
    buf = torch.full((2 * n + 2, h + 2, w + 62, 2), float("nan"), device="cuda")
    vf, vb = buf[0:2 * n:2, :h, :w], buf[1:2 * n:2, :h, :w]
    vf.copy_(dev(fw))
    vb.copy_(dev(bw))
    assert occ._strides(vf, even=True) == occ._strides(vb, even=True) == ((w + 62) * 2, 2 * (h + 2) * (w + 62) * 2)
    want_fw, want_bw, parts = occlusion_ref(fw, bw, 1.0 / 64, 0.5)
    occlusion_exact_ok(fw, bw, parts)
    got_fw, got_bw = occ.occlusion(vf, vb, alpha=1.0 / 64, beta=0.5, as_uint8=True)
    np.testing.assert_array_equal(host(got_fw), want_fw.astype(np.uint8) * 255)
    np.testing.assert_array_equal(host(got_bw), want_bw.astype(np.uint8) * 255)


# ------------------------------------------------------------------------------------------------ 4. robustness
@pytest.mark.gpu
@pytest.mark.parametrize("mask_dtype", ["f32", "u8"])
@pytest.mark.parametrize("shape", [(2, 5, 7), (2, 6, 130)])
def test_occlusion_survives_poisoned_flows(hip, shape, mask_dtype):
    """NaN, +-inf and +-1e30 in a few pixels of each flow.  No tap may leave the image (the guard words behind both mask
    buffers come back untouched, the call completes), and every pixel that neither IS poisoned nor READS a poisoned pixel
    must match the reference exactly.  What is written at the others is unspecified: a coordinate of 1e30 is as undefined
    in the reference as an infinite one (|flow|^2 = 1e60 is not even an fp32 number), so a pixel whose own flow is one of
    the poison values is not compared."""
    import torch
    n, h, w = shape
    alpha, beta = 1.0 / 64, 0.5
    fw, bw, check, want_fw, want_bw = poisoned_case(shape, alpha, beta)

    npix, guard = n * h * w, 64
    tdt, one, sentinel = (torch.float32, 1.0, -7.0) if mask_dtype == "f32" else (torch.uint8, 255, 0x5A)
    m_fw = torch.full((npix + guard,), sentinel, dtype=tdt, device="cuda")
    m_bw = torch.full((npix + guard,), sentinel, dtype=tdt, device="cuda")
    d_fw, d_bw = dev(fw), dev(bw)
    rc = hip.lib().fn2_fb_occlusion(hip.ptr(d_fw), hip.ptr(d_bw), 2 * w, 2 * w * h, hip.ptr(m_fw), hip.ptr(m_bw),
                                    hip.MASK_F32 if mask_dtype == "f32" else hip.MASK_U8, n, h, w, alpha, beta,
                                    hip.stream_ptr())
    hip.check(rc)
    got_fw, got_bw = host(m_fw), host(m_bw)
    for got, want in ((got_fw, want_fw), (got_bw, want_bw)):
        assert np.all(got[npix:] == sentinel)
        body = got[:npix].reshape(n, h, w)
        assert np.all((body == 0) | (body == one))               # whatever is written is a mask value
        np.testing.assert_array_equal(body[check], want[..., 0][check].astype(body.dtype) * body.dtype.type(one))
    np.testing.assert_array_equal(host(d_fw), fw)                # inputs are only read
    np.testing.assert_array_equal(host(d_bw), bw)


# ------------------------------------------------------------------------------------------------ 5. arguments
def invalid_argument_cases(hip, base):
    """(call, word of the message) for the four kinds of invalid argument, on pointers that are never dereferenced."""
    lib = hip.lib()
    p = [base + 256 * k for k in range(5)]

    def warp(img=p[0], ip=3 * 7, flow=p[1], fp=2 * 7, out=p[2], h=5, w=7):
        return lib.fn2_tf_warp_f32(img, ip, ip * 5, flow, fp, fp * 5, out, 2, h, w, 3, None)

    def occ(fw=p[0], bw=p[1], fp=2 * 7, o1=p[2], o2=p[3], md=hip.MASK_F32, h=5, w=7):
        return lib.fn2_fb_occlusion(fw, bw, fp, fp * 5, o1, o2, md, 2, h, w, 0.01, 0.5, None)

    return [(lambda: occ(h=0), b"bad size"), (lambda: occ(w=0), b"bad size"), (lambda: occ(w=-3), b"bad size"),
            (lambda: occ(fp=2 * 7 - 2), b"flow_pitch"),
            (lambda: occ(fw=None), b"null"), (lambda: occ(bw=None), b"null"), (lambda: occ(o1=None), b"null"),
            (lambda: occ(o2=None), b"null"),
            (lambda: occ(md=2), b"mask_dtype"), (lambda: occ(md=-1), b"mask_dtype"),
            (lambda: warp(h=0), b"bad size"), (lambda: warp(w=0), b"bad size"),
            (lambda: warp(fp=2 * 7 - 2), b"flow_pitch"), (lambda: warp(ip=3 * 7 - 1), b"img_pitch"),
            (lambda: warp(img=None), b"null"), (lambda: warp(flow=None), b"null"), (lambda: warp(out=None), b"null")]


def check_invalid_arguments(hip):
    store = (C.c_char * 4096)()
    base = (C.addressof(store) + 255) & ~255
    lib = hip.lib()
    for call, word in invalid_argument_cases(hip, base):
        rc = call()
        assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (word, rc, lib.fn2_last_error())
        with pytest.raises(ValueError):
            hip.check(rc)


@pytest.mark.gpu
def test_invalid_arguments_and_ranks(hip):
    from src.occlusion import occlusion, tf_warp
    check_invalid_arguments(hip)
    f = np.zeros((1, 4, 5, 2), np.float32)
    for bad_fw, bad_bw in ((f[0], f[0]), (f, f[0]), (f, f[:, :3]), (f[..., :1], f[..., :1]), (np.zeros((1, 4, 5, 3), np.float32),) * 2):
        with pytest.raises(ValueError):
            occlusion(bad_fw, bad_bw)
        with pytest.raises(ValueError):
            occlusion(dev(bad_fw), dev(bad_bw))
    img = np.zeros((1, 4, 5, 3), np.float32)
    for bad_img, bad_flow in ((img[0], f[0]), (img, f[0]), (img[0], f), (img, f[:, :3]), (img, img)):
        with pytest.raises(ValueError):
            tf_warp(bad_img, bad_flow)


# ------------------------------------------------------------------------------------------------ 6. end to end
EPE_TOL = 1e-3   # the README's bound between two runs of the engine, used only if the engine is not deterministic
BAND = 1e-4      # relative half-width of the band around the threshold inside which a mask pixel may differ
BAND_CAP = 0.005  # at most this share of the pixels may lie in the band


def _net():
    from src.flownet_s.flownet_s import FlowNetS
    from src.net import Mode
    net = FlowNetS(mode=Mode.TEST)
    net.load_weights(None)
    return net


def _frames(rng, h, w):
    a = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1, 3)).astype(np.uint8)
    a = np.kron(a, np.ones((4, 4, 1), np.uint8))[:h, :w]        # blocks, so that a shift is visible
    return a, np.roll(a, (2, -3), (0, 1))


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """Three PNG pairs, two at 64 x 64 and one at 50 x 70 (padded to 64 x 128), and a synthetic ground truth for the first."""
    from PIL import Image
    from src import flowlib
    root = tmp_path_factory.mktemp("occ_pairs")
    seq = root / "seq"
    seq.mkdir()
    rng = np.random.default_rng(2024)
    recs = []
    for k, (h, w) in enumerate([(64, 64), (64, 64), (50, 70)]):
        a, b = _frames(rng, h, w)
        pa, pb = str(seq / ("p%d_a.png" % k)), str(seq / ("p%d_b.png" % k))
        Image.fromarray(a).save(pa)
        Image.fromarray(b).save(pb)
        recs.append(dict(a=pa, b=pb, name="p%d_a" % k, back="p%d_b" % k, size=(h, w)))
    gt = str(seq / "p0_gt.flo")
    flowlib.write_flow(rng.standard_normal((64, 64, 2)).astype(np.float32), gt)
    recs[0]["gt"] = gt
    return dict(root=root, recs=recs)


@pytest.fixture(scope="module")
def runs(pairs):
    """One net, three list runs with batch_size 4: the bidirectional one, and plain ones over lists that spell the same
    slots out -- `a b` / `b a` alternating, each padded size in its own list."""
    root, recs = pairs["root"], pairs["recs"]
    net = _net()
    lst = root / "bidi.txt"
    lst.write_text("".join("%s %s%s\n" % (r["a"], r["b"], " " + r["gt"] if "gt" in r else "") for r in recs))
    out = root / "out_bidi"
    flows = net.test_batch(None, str(lst), str(out), occlusions=True, occlusions_for_metrics=True, batch_size=4)
    masks = list(net.last_occlusions)
    engines = {k[:3] for k in net._engines}
    plain = {}
    for tag, members in (("s64", recs[:2]), ("s128", recs[2:])):
        pl = root / ("plain_%s.txt" % tag)
        pl.write_text("".join("%s %s\n%s %s\n" % (r["a"], r["b"], r["b"], r["a"]) for r in members))
        res = net.test_batch(None, str(pl), str(root / "out_plain"), batch_size=4, save_image=False)
        for k, r in enumerate(members):
            plain[r["name"]] = (res[2 * k], res[2 * k + 1])
    return dict(net=net, out=out, flows=flows, masks=masks, plain=plain, engines=engines, log=(out / "bidi_metrics.log").read_text())


@pytest.mark.gpu
def test_bidirectional_flows_equal_the_plain_run_slot_for_slot(pairs, runs):
    """The engine sees identical bytes in identical slots, so the flows are those of the plain run bit for bit -- if one
    engine launched twice on the same inputs gives the same bits twice, which is checked first.  Only if it does not is
    the comparison the README's run-to-run bound of 1e-3 px."""
    import torch
    from src import flowlib
    net, recs = runs["net"], pairs["recs"]
    assert runs["engines"] == {(4, 64, 64), (4, 64, 128)}      # the bidirectional run built the plain run's engines, no other
    eng = net.engine(4, 64, 64, uint8_inputs=True)
    eng.launch()
    first = eng.outputs["flow"].clone()
    eng.launch()
    deterministic = torch.equal(first, eng.outputs["flow"])
    print("engine run-to-run deterministic: %s" % deterministic)
    for r, fw in zip(recs, runs["flows"]):
        bw = flowlib.read_flow(str(runs["out"] / "seq" / (r["name"] + "_flow_bw.flo")))
        want_fw, want_bw = runs["plain"][r["name"]]
        assert fw.shape == r["size"] + (2,) and fw.dtype == np.float32 and bw.shape == fw.shape
        for got, want in ((fw, want_fw), (bw, want_bw)):
            if deterministic:
                np.testing.assert_array_equal(got, want)
            else:
                assert float(np.sqrt(((got.astype(np.float64) - want) ** 2).sum(-1)).max()) < EPE_TOL


@pytest.mark.gpu
def test_bidirectional_masks_files_and_metrics(pairs, runs):
    """The masks against occlusion_ref on the returned flows.  The device's d differs from the float64 one by about
    2 sqrt(d) 8 U M (8 roundings on components of size M) ~ 1e-5 t near the threshold, a tenth of the band
    |d - t| <= 1e-4 (1 + t + d); outside the band the masks must agree, and at most 0.5 % of the pixels may lie inside."""
    from PIL import Image
    from src import flowlib
    recs, out = pairs["recs"], runs["out"] / "seq"
    assert len(runs["flows"]) == len(runs["masks"]) == len(recs)
    for r, fw, (occ_fw, occ_bw) in zip(recs, runs["flows"], runs["masks"]):
        bw = flowlib.read_flow(str(out / (r["name"] + "_flow_bw.flo")))
        assert np.array_equal(flowlib.read_flow(str(out / (r["name"] + "_flow.flo"))), fw)
        for m, suffix in ((occ_fw, "_occ.png"), (occ_bw, "_occ_bw.png")):
            assert m.shape == r["size"] and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255}
            assert np.array_equal(np.asarray(Image.open(str(out / (r["name"] + suffix)))), m)
        assert (out / (r["name"] + "_viz.png")).exists()
        want_fw, want_bw, (d_fw, t_fw, d_bw, t_bw, _, _) = occlusion_ref(fw[None], bw[None])
        for got, want, d, t in ((occ_fw, want_fw, d_fw, t_fw), (occ_bw, want_bw, d_bw, t_bw)):
            band = (np.abs(d - t) <= BAND * (1 + t + d))[0, :, :, 0]
            print("%s: %.2f occluded, %d of %d pixels in the band" % (r["name"], want.mean(), band.sum(), band.size))
            assert band.mean() <= BAND_CAP
            np.testing.assert_array_equal(got[~band], want[0, :, :, 0][~band].astype(np.uint8) * 255)
    # the line with a ground truth and no mask file: its matched / unmatched split is that of the estimated forward mask
    log = runs["log"]
    assert log.count("MPI-Sintel Flow Error Metrics") == 1 and recs[0]["name"] in log
    m, *_ = flowlib.compute_all_metrics(runs["flows"][0], flowlib.read_flow(recs[0]["gt"]), occ_mask=runs["masks"][0][0])
    plain_m, *_ = flowlib.compute_all_metrics(runs["flows"][0], flowlib.read_flow(recs[0]["gt"]))
    assert 0 < (runs["masks"][0][0] == 255).mean() < 1 and m["EPEmat"] != plain_m["EPEmat"]
    rows = {ln.split()[0]: ln for ln in log.splitlines() if ln.startswith("(")}
    assert rows["(mat)"].split()[-1] == "%.4f" % m["EPEmat"] and rows["(umt)"].split()[-1] == "%.4f" % m["EPEumat"]
    assert rows["(all)"].split()[-1] == "%.4f" % m["EPEall"]


@pytest.mark.gpu
def test_a_mask_file_wins_and_defaults_write_what_they_wrote(pairs, runs, tmp_path):
    from PIL import Image
    from src import flowlib
    net, r = runs["net"], pairs["recs"][0]
    occ = np.zeros((64, 64), np.uint8)
    occ[:, :20] = 255
    Image.fromarray(occ).save(str(tmp_path / "occ.png"))
    lst = tmp_path / "with_file.txt"
    lst.write_text("%s %s %s %s\n" % (r["a"], r["b"], r["gt"], tmp_path / "occ.png"))
    flows = net.test_batch(None, str(lst), str(tmp_path / "o1"), occlusions_for_metrics=True, batch_size=4, save_image=False)
    m, *_ = flowlib.compute_all_metrics(flows[0], flowlib.read_flow(r["gt"]), occ_mask=occ)
    rows = {ln.split()[0]: ln for ln in (tmp_path / "o1" / "with_file_metrics.log").read_text().splitlines() if ln.startswith("(")}
    assert rows["(umt)"].split()[-1] == "%.4f" % m["EPEumat"]
    assert not (tmp_path / "o1" / "seq" / (r["name"] + "_occ.png")).exists()        # metrics only: no mask files
    # a default run leaves exactly the files it left before
    lst2 = tmp_path / "plain.txt"
    lst2.write_text("%s %s\n" % (r["a"], r["b"]))
    net.test_batch(None, str(lst2), str(tmp_path / "o2"), batch_size=4)
    assert sorted(os.listdir(str(tmp_path / "o2" / "seq"))) == [r["name"] + s for s in
                                                                ("_flow.flo", "_viz.png", "_viz_norm_gt_max_motion.png")]
    with pytest.raises(ValueError):
        net.test_batch(None, str(lst2), str(tmp_path / "o3"), occlusions=True, batch_size=3)


@pytest.mark.gpu
def test_single_pair_and_refinement(pairs, runs, tmp_path):
    """Net.test(occlusions=True) writes the same kinds of files and returns the forward flow; with
    variational_refinement only the forward flow changes, and the masks are those of the unrefined flows."""
    from PIL import Image
    from src import flowlib
    net, r = runs["net"], pairs["recs"][2]
    flow = net.test(None, r["a"], r["b"], out_path=str(tmp_path), occlusions=True)
    d = tmp_path / "seq"
    assert isinstance(flow, np.ndarray) and flow.shape == r["size"] + (2,)
    assert np.array_equal(flowlib.read_flow(str(d / (r["name"] + "_flow.flo"))), flow)
    occ_fw, occ_bw = net.last_occlusions[0]
    assert np.array_equal(np.asarray(Image.open(str(d / (r["name"] + "_occ.png")))), occ_fw)
    assert np.array_equal(np.asarray(Image.open(str(d / (r["name"] + "_occ_bw.png")))), occ_bw)
    bw = flowlib.read_flow(str(d / (r["name"] + "_flow_bw.flo")))
    want_fw, want_bw = runs["plain"][r["name"]]
    assert float(np.sqrt(((flow.astype(np.float64) - want_fw) ** 2).sum(-1)).max()) < EPE_TOL   # another engine (batch 2)
    assert float(np.sqrt(((bw.astype(np.float64) - want_bw) ** 2).sum(-1)).max()) < EPE_TOL
    refined = net.test(None, r["a"], r["b"], out_path=str(tmp_path / "ref"), occlusions=True, variational_refinement=True,
                       save_image=False)
    assert refined.shape == flow.shape and not np.array_equal(refined, flow)
    assert np.array_equal(net.last_occlusions[0][0], occ_fw) and np.array_equal(net.last_occlusions[0][1], occ_bw)
    assert np.array_equal(flowlib.read_flow(str(tmp_path / "ref" / "seq" / (r["name"] + "_flow_bw.flo"))), bw)
    with pytest.raises(ValueError):
        net.test(None, r["a"], matches_a_path="m", sparse_flow_path="s", input_type="image_matches", occlusions=True)
