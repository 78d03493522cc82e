"""The occlusion-aware photometric loss op by op (csrc/photometric.hip, src/photometric.py) against its float64 twin
(photometric_twin.py), with the exact-arithmetic method of test_gpu_occlusion.py.

Inputs: the flows f = scale * pred are multiples of 1/2 with |component| <= 5 (for scale 5 and 0.625 multiples of 2.5: pred
is a multiple of 1/2 resp. 4, so that the product is exact), the images multiples of 1/2 in [-4, 4].  Then the position, the
weight factors (multiples of 1/2), the weights (1/4), the warped flows and image values (1/8), d = |f + warp(f')|^2 and the
magnitudes (1/64) are all exact in fp32 in any order, with or without contraction; every exact test asserts that on the
twin (the helpers of test_gpu_occlusion.py) and then compares with assert_array_equal.  The residual d_c = I - warp_c is
exact too; psi and psi' are not (powf), so the loss is held to rel 1e-5 (the bar test_gpu_train.py uses for losses) and the gradient to
2e-5 * max|want| per level (DESIGN sections 5 and 9)."""
import ctypes as C
import functools

import numpy as np
import pytest

import photometric_twin as twin
from test_gpu_occlusion import dyadic_flows, dyadic_image, occlusion_exact_ok, occlusion_ref, warp_exact_ok

U = 2.0 ** -24
SHAPES = [(2, 5, 7),      # general small case
          (2, 3, 70),     # crosses a wave
          (4, 6, 130),    # two pairs, wider than two waves
          (2, 1, 1),      # no valid pixel: loss and gradient exactly 0
          (2, 9, 1),      # 1-wide: nothing valid either
          (2, 1, 9)]      # 1-high
SCALES = [1.0, 0.625, 5.0]      # dyadic, as 20 / 2^l is
GRAD_TOL, LOSS_TOL = 2e-5, 1e-5


# ------------------------------------------------------------------------------------------------ inputs
def slot_case(seed, shape, scale=1.0):
    """(pred [n,h,w,2], img [n,h,w,3]) float32 in the slot layout; f = scale * pred exactly, multiples of 1/2, |f| <= 5."""
    n, h, w = shape
    fw, bw = dyadic_flows(seed, (n // 2, h, w))
    f = np.empty((n, h, w, 2), np.float32)
    f[0::2], f[1::2] = fw, bw
    if scale != 1.0:
        f = (np.round(f / 2.5) * 2.5).astype(np.float32)         # multiples of 2.5: divisible by 5 and by 0.625 in fp32
    pred = (f / np.float32(scale)).astype(np.float32)
    assert np.array_equal(np.float32(scale) * pred, f) and np.all(f * 2 == np.round(f * 2)) and np.abs(f).max() <= 5
    return pred, dyadic_image(seed + 100, shape, 3)


@functools.lru_cache(maxsize=None)
def reference(seed, shape, scale, alpha, weight=1.0, grad_mult=1.0, q=0.4):
    """The twin on slot_case(seed, shape, scale), computed once: (pred, img, mask, parts, L, dpred), with the exactness
    preconditions asserted."""
    pred, img = slot_case(seed, shape, scale)
    mask, parts = twin.masks(pred, scale, alpha, 0.5)
    f = parts["f"].astype(np.float32)
    fw, bw = f[0::2], f[1::2]
    occ_fw, occ_bw, oparts = occlusion_ref(fw, bw, alpha, 0.5)
    occlusion_exact_ok(fw, bw, oparts)                             # d and the magnitudes are exact in fp32
    warp_exact_ok(img, f)                                          # ... and so is the warped image, hence I - warp
    # the pinned restatement of the occlusion test says the same as the twin's
    assert np.array_equal(parts["occ"][0::2], occ_fw[..., 0]) and np.array_equal(parts["occ"][1::2], occ_bw[..., 0])
    L, g, d = twin.loss_and_grad(img, pred, mask, scale, weight, q, grad_mult)
    assert np.all(d[mask] * 8 == np.round(d[mask] * 8))
    return pred, img, mask, parts, L, g


def margin_ok(parts):
    """alpha = 0.01: t = fl(fl(alpha) * mag) + 0.5 carries at most three roundings, an error <= 4 U (1 + t); every pixel
    keeps 2^-18 (1 + t) from its threshold."""
    return float((np.abs(parts["d"] - parts["t"]) / (1 + parts["t"])).min()) > 2.0 ** -18 > 4 * U


def quirk_case():
    """Hand-written rows on a 4 x 6 level, slot 0 zero flow except one pixel per row of the table; slot 1 zero flow.  Returns
    (pred, img, want mask of slot 0): a zero flow is valid and unoccluded except in the last row and the last column, where
    tf_warp returns 0; the hand-placed pixels are all invalid."""
    h, w = 4, 6
    pred = np.zeros((2, h, w, 2), np.float32)
    want = np.ones((h, w), np.float32)
    want[-1, :] = 0
    want[:, -1] = 0
    for py, px, u, v in [(0, 0, -0.5, 0.0),      # X in (-1, 0): tf_warp extrapolates, the loss must not look
                         (1, 0, -0.25, 0.0),
                         (1, 2, 3.0, 0.0),       # X = w - 1 exactly
                         (2, 3, 2.5, 0.0),       # X > w - 1
                         (0, 2, 0.0, -0.5),      # Y in (-1, 0)
                         (1, 4, 0.0, 2.0),       # Y = h - 1
                         (2, 1, 0.0, 1.5)]:      # Y > h - 1
        pred[0, py, px] = (u, v)
        want[py, px] = 0
    img = ((10.0 * (np.arange(h)[:, None] + 1) + np.arange(w)[None, :] + 1)[None, :, :, None]
           * np.array([0.5, 1.0, 1.5])).astype(np.float32)
    img = np.concatenate([img, img[:, ::-1]], 0)
    return pred, img, want


def poisoned_case(shape):
    """slot_case with NaN, +-inf and +-1e30 in a few flow components.  `check` [n,h,w]: pixels that neither are poisoned nor
    read a poisoned partner pixel; there the twin on the poisoned flows equals the twin on the flows with the poison taken
    out (asserted), masks exactly."""
    from test_gpu_occlusion import tap_hits
    n, h, w = shape
    pred, img = slot_case(21, shape)
    pred = pred.copy()
    rng = np.random.default_rng(22)
    bad = np.zeros((n, h, w), bool)
    for k, v in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan]):
        i, y, x = rng.integers(n), rng.integers(h), rng.integers(w)
        pred[i, y, x, k % 2] = v
        bad[i, y, x] = True
    clean = np.where(bad[..., None], 0, pred).astype(np.float32)
    check = ~(bad | tap_hits(bad[twin.partner(n)], clean))
    assert check.mean() > 0.5 and not check.all()
    mask, _ = twin.masks(pred, 1.0, 1.0 / 64, 0.5)
    clean_mask, parts = twin.masks(clean, 1.0, 1.0 / 64, 0.5)
    occlusion_exact_ok(clean[0::2], clean[1::2], occlusion_ref(clean[0::2], clean[1::2], 1.0 / 64, 0.5)[2])
    assert np.array_equal(mask[check], clean_mask[check]) and not mask[bad].any()
    return pred, img, check, mask


# ------------------------------------------------------------------------------------------------ device helpers
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(pred, img, **kw):
    from src.photometric import photometric_loss
    loss, mask, count, dpred = photometric_loss(dev(img), dev(pred), **kw)
    return float(host(loss)[0]), host(mask)[..., 0], float(host(count)[0]), host(dpred)


def check_loss_and_grad(got_loss, got_g, L, g, mask):
    if not mask.any():
        assert got_loss == 0.0 and not got_g.any()                 # exactly
        return
    print("loss %.9g, twin %.9g; worst gradient error %.3e of the largest" %
          (got_loss, L, np.abs(got_g - g).max() / np.abs(g).max()))
    assert abs(got_loss - L) <= LOSS_TOL * abs(L), (got_loss, L)
    assert np.abs(got_g - g).max() <= GRAD_TOL * np.abs(g).max()
    assert not got_g[~mask].any()                                  # a masked pixel gets an exact zero


# ------------------------------------------------------------------------------------------------ 1. masks
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_masks_with_a_dyadic_alpha_are_exact(shape, scale):
    """alpha = 1/64: the threshold is exact too.  Second witness: the pinned op on the same flows."""
    import torch
    from src.occlusion import occlusion
    pred, img, mask, parts, _, _ = reference(0, shape, scale, 1.0 / 64)
    _, got, count, _ = run(pred, img, scale=scale, alpha=1.0 / 64)
    np.testing.assert_array_equal(got, mask.astype(np.float32))
    assert count == mask.sum()
    f = dev(parts["f"].astype(np.float32))
    occ_fw, occ_bw = occlusion(f[0::2], f[1::2], alpha=1.0 / 64, beta=0.5)
    occ = torch.stack([occ_fw, occ_bw], 1).reshape(f.shape[:3])
    np.testing.assert_array_equal(got[parts["valid"]], 1 - host(occ)[parts["valid"]])
    assert not got[~parts["valid"]].any()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_masks_with_the_reference_constants(shape, seed):
    pred, img, mask, parts, _, _ = reference(seed, shape, 1.0, 0.01)
    assert margin_ok(parts)                                        # no pixel within three roundings of its threshold
    if shape in SHAPES[:3]:
        assert mask.any() and not mask.all() and parts["occ"].any()
    _, got, count, _ = run(pred, img)
    np.testing.assert_array_equal(got, mask.astype(np.float32))
    assert count == mask.sum()


# ------------------------------------------------------------------------------------------------ 2. loss and gradient
@pytest.mark.gpu
@pytest.mark.parametrize("grad_mult", [1.0, 16384.0])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_match_the_twin(shape, scale, grad_mult):
    pred, img, mask, parts, L, g = reference(0, shape, scale, 0.01, 0.064, grad_mult)
    assert margin_ok(parts)
    got_loss, got_mask, _, got_g = run(pred, img, scale=scale, weight=0.064, grad_mult=grad_mult)
    np.testing.assert_array_equal(got_mask, mask.astype(np.float32))
    check_loss_and_grad(got_loss, got_g, L, g, mask)


@pytest.mark.gpu
def test_five_levels_in_one_launch_equal_five_launches():
    """One table of five levels (different sizes, scales and weights) against the same levels one launch each: masks, counts
    and gradients bit for bit (nothing in a pixel depends on the table), the loss to LOSS_TOL (atomics in another order) --
    and against the twin."""
    import torch
    from src import _hip
    from src.photometric import level, level_table
    lib = _hip.lib()
    shapes = [(4, 6, 130), (4, 3, 70), (4, 5, 7), (4, 2, 3), (4, 1, 2)]
    scales, weights = [5.0, 1.0, 0.625, 1.0, 5.0], [0.064, 0.016, 0.004, 0.002, 0.001]
    refs = [reference(3, shp, s, 0.01, wgt, 16384.0) for shp, s, wgt in zip(shapes, scales, weights)]
    assert all(margin_ok(r[3]) for r in refs)

    def launch(groups):
        """groups: lists of level indices, one launch pair per group -> (loss, [(mask, count, dpred)])."""
        bufs = [(dev(r[0]), dev(r[1]), torch.full(r[2].shape, -7.0, device="cuda"), torch.zeros(1, device="cuda"),
                 torch.full(r[0].shape, -7.0, device="cuda")) for r in refs]
        loss = torch.zeros(1, device="cuda")
        for grp in groups:
            table = level_table([level(*bufs[i], scales[i], weights[i]) for i in grp])
            _hip.check(lib.fn2_photometric_masks(table, len(grp), 4, 0.01, 0.5, _hip.stream_ptr()))
            _hip.check(lib.fn2_photometric_loss_grad(table, len(grp), 4, 0.4, 16384.0, _hip.ptr(loss), _hip.stream_ptr()))
        return float(host(loss)[0]), [(host(b[2]), float(host(b[3])[0]), host(b[4])) for b in bufs]

    one_loss, one = launch([[0, 1, 2, 3, 4]])
    five_loss, five = launch([[i] for i in range(5)])
    want_loss = sum(r[4] for r in refs)
    assert abs(one_loss - five_loss) <= LOSS_TOL * abs(five_loss) and abs(one_loss - want_loss) <= LOSS_TOL * abs(want_loss)
    for (m1, c1, g1), (m5, c5, g5), r in zip(one, five, refs):
        np.testing.assert_array_equal(m1, m5)
        np.testing.assert_array_equal(g1, g5)
        assert c1 == c5 == r[2].sum()
        np.testing.assert_array_equal(m1, r[2].astype(np.float32))
        if r[2].any():
            assert np.abs(g1 - r[5]).max() <= GRAD_TOL * np.abs(r[5]).max()
        else:
            assert not g1.any()


@pytest.mark.gpu
def test_quirk_rows_by_hand():
    pred, img, want = quirk_case()
    mask, parts = twin.masks(pred)
    np.testing.assert_array_equal(mask[0], want.astype(bool))      # the twin agrees with the hand-written mask
    L, g, _ = twin.loss_and_grad(img, pred, mask)
    got_loss, got_mask, count, got_g = run(pred, img)
    np.testing.assert_array_equal(got_mask[0], want)
    np.testing.assert_array_equal(got_mask, mask.astype(np.float32))
    assert count == mask.sum()
    check_loss_and_grad(got_loss, got_g, L, g, mask)


# ------------------------------------------------------------------------------------------------ 3. robustness
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 5, 7), (4, 6, 130)])
def test_poisoned_flows_are_clamped(shape):
    """NaN, +-inf and +-1e30 in a few flow components: the call completes with every tap inside its image (guard words behind
    mask and dpred stay), the inputs are unchanged, a poisoned pixel is masked out and gets a zero gradient, and every
    pixel that neither is poisoned nor reads a poisoned partner pixel matches the twin.  The loss is compared only through
    those pixels' gradients: its normaliser counts pixels whose mask is unspecified."""
    import torch
    from src import _hip
    from src.photometric import level, level_table
    n, h, w = shape
    pred, img, check, mask = poisoned_case(shape)
    npix, guard = n * h * w, 64
    d_pred, d_img = dev(pred), dev(img)
    m = torch.full((npix + guard,), -7.0, device="cuda")
    g = torch.full((2 * npix + guard,), -7.0, device="cuda")
    scal = torch.zeros(2, device="cuda")
    table = level_table([level(d_pred, d_img, m[:npix].view(n, h, w), scal[1:], g[:2 * npix].view(n, h, w, 2), 1.0, 1.0)])
    _hip.check(_hip.lib().fn2_photometric_masks(table, 1, n, 1.0 / 64, 0.5, _hip.stream_ptr()))
    _hip.check(_hip.lib().fn2_photometric_loss_grad(table, 1, n, 0.4, 1.0, _hip.ptr(scal), _hip.stream_ptr()))
    got_m, got_g, count = host(m), host(g), float(host(scal)[1])
    assert np.all(got_m[npix:] == -7.0) and np.all(got_g[2 * npix:] == -7.0)
    got_m, got_g = got_m[:npix].reshape(n, h, w), got_g[:2 * npix].reshape(n, h, w, 2)
    assert np.all((got_m == 0) | (got_m == 1)) and count == got_m.sum()
    np.testing.assert_array_equal(got_m[check], mask[check].astype(np.float32))
    assert not got_m[~np.isfinite(pred).all(-1)].any()
    np.testing.assert_array_equal(host(d_pred), pred)              # inputs are only read (NaN == NaN here)
    np.testing.assert_array_equal(host(d_img), img)
    # the twin's gradient under the DEVICE's mask (so that both divide by the same count)
    _, want_g, _ = twin.loss_and_grad(img, pred, got_m)
    assert np.isfinite(got_g).all()
    assert np.abs(got_g - want_g)[check].max() <= GRAD_TOL * np.abs(want_g[check]).max()


# ------------------------------------------------------------------------------------------------ 4. arguments
def level_struct(hip, **kw):
    fake = 0x1000
    return hip.Fn2PhotometricLevel(**dict(dict(pred=fake, img=fake, mask=fake, mask_sum=fake, dpred=fake, h=4, w=5,
                                               scale=1.0, weight=1.0), **kw))


def check_invalid_arguments(hip):
    """Every check sits in front of the launch: the pointers are never followed."""
    lib = hip.lib()
    L = hip.Fn2PhotometricLevel
    ok = lambda **kw: level_struct(hip, **kw)
    masks = lambda table, nl=1, n=2: lib.fn2_photometric_masks(table, nl, n, 0.01, 0.5, None)
    grad = lambda table, nl=1, n=2, q=0.4, acc=0x1000: lib.fn2_photometric_loss_grad(table, nl, n, q, 1.0, acc, None)
    cases = [(lambda f: f(None), b"null level table"), (lambda f: f(ok(), 0), b"n_levels"),
             (lambda f: f((L * 9)(*[ok() for _ in range(9)]), 9), b"n_levels"),
             (lambda f: f(ok(), 1, 3), b"even"), (lambda f: f(ok(), 1, 0), b"even"),
             (lambda f: f(ok(h=0)), b"bad size"), (lambda f: f(ok(w=0)), b"bad size"), (lambda f: f(ok(w=-2)), b"bad size"),
             (lambda f: f(ok(pred=0x1004)), b"aligned"),
             (lambda f: f((L * 3)(ok(), ok(), ok(img=None)), 3), b"level 2")]
    cases += [(lambda f, k=k: f(ok(**{k: None})), b"null pointer") for k in ("pred", "img", "mask", "mask_sum", "dpred")]
    for f in (masks, grad):
        for call, word in cases:
            rc = call(f)
            assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (word, rc, lib.fn2_last_error())
    for kw, word in ((dict(acc=None), b"loss_accum"), (dict(q=0.0), b"q must"), (dict(q=1.5), b"q must"),
                     (dict(q=float("nan")), b"q must")):
        rc = grad(ok(), **kw)
        assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (word, rc, lib.fn2_last_error())
    with pytest.raises(ValueError):
        hip.check(masks(ok(), 1, 3))


@pytest.mark.gpu
def test_invalid_arguments_on_the_device_box():
    import torch
    from src import _hip
    from src.photometric import photometric_loss
    check_invalid_arguments(_hip)
    img, pred = torch.zeros(2, 4, 5, 3, device="cuda"), torch.zeros(2, 4, 5, 2, device="cuda")
    for bad_img, bad_pred in ((img[0], pred[0]), (img, pred[:, :3]), (img[..., :2], pred), (img, img), (img[:1], pred[:1]),
                              (img.cpu(), pred.cpu())):
        with pytest.raises(ValueError):
            photometric_loss(bad_img, bad_pred)
    for kw in (dict(q=0.0), dict(q=2.0), dict(alpha=-1.0), dict(beta=float("nan"))):
        with pytest.raises(ValueError):
            photometric_loss(img, pred, **kw)
