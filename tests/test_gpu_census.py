"""The ternary census data term op by op (csrc/census.hip, src/census.py) against its float64 twin (census_twin.py), with
the exact-arithmetic method of test_gpu_photometric.py.

Inputs: the images are multiples of 1/256 in [0, 1], so G = ((r + g) + b) * 85 is a multiple of 85/256 below 2^8 with 16
significant bits; the flows f = scale * pred are multiples of 1/2 with |component| <= 3 (for the scales 5 and 0.625 multiples
of 2.5, as in test_gpu_photometric.py), so the weight factors are multiples of 1/2, the weights of 1/4, and W, DX, DY are
multiples of 1/1024 below 256: exact in fp32 in any order, with or without contraction.  reference() asserts that on the twin
and the tests compare G, W, DX, DY, V and Mc with assert_array_equal.  Behind them stand sqrtf, divisions and powf: the loss
is held to rel 1e-5, S and dpred to 2e-5 * max|want| per level (DESIGN sections 5, 9 and 15).

The kernels' tile is 8 rows x 32 columns with a 3-pixel halo (14 x 38 staged): (2, 19, 9) is taller than a tile plus halo and
spans three tile rows, (2, 8, 70) and (4, 10, 135) are wider and span three and five tile columns."""
import functools

import numpy as np
import pytest

import census_twin as twin

SHAPES = [(2, 7, 7),      # one interior pixel
          (2, 6, 9),      # no interior: loss and gradient exactly 0
          (2, 9, 6),
          (2, 8, 70),     # crosses a wave, wider than a tile plus halo
          (4, 10, 135),   # two pairs, wider than two waves, two tile rows
          (2, 19, 9)]     # taller than a tile plus halo
SCALES = [1.0, 0.625, 5.0]
GRAD_TOL, LOSS_TOL = 2e-5, 1e-5
WORST = {}                # what the tests of this run saw, printed by each of them


# ------------------------------------------------------------------------------------------------ inputs
def census_case(seed, shape, scale=1.0):
    """(pred [n,h,w,2], img [n,h,w,3], mask [n,h,w] with about 20 % zeros) float32; f = scale * pred exactly, multiples of
    1/2 with |f| <= 3 (|f| <= 1 on the 7 x 7 level, so that its one interior pixel stays valid in most cases)."""
    n, h, w = shape
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    fmax = 1 if shape == (2, 7, 7) else 3
    f = (rng.integers(-2 * fmax, 2 * fmax + 1, (n, h, w, 2)) / 2.0).astype(np.float32)
    f[:, h // 2, w // 2] = 0                                       # (the centre always samples inside)
    if scale != 1.0:
        f = (np.round(f / 2.5) * 2.5).astype(np.float32)           # multiples of 2.5: divisible by 5 and by 0.625 in fp32
    pred = (f / np.float32(scale)).astype(np.float32)
    assert np.array_equal(np.float32(scale) * pred, f) and np.all(f * 2 == np.round(f * 2)) and np.abs(f).max() <= 3
    img = (rng.integers(0, 257, (n, h, w, 3)) / 256.0).astype(np.float32)
    mask = (rng.random((n, h, w)) > 0.2).astype(np.float32)
    mask[:, h // 2, w // 2] = 1
    return pred, img, mask


def warp_exact_ok(parts):
    """G has 16 significant bits below 2^8; W, DX, DY are multiples of 1/1024 below 256: fp32 holds every partial sum."""
    G, ok = parts["G"], True
    ok &= bool(np.all(G * 256 == np.round(G * 256)) and G.min() >= 0 and G.max() <= 255)
    for k in ("W", "DX", "DY"):
        v = parts[k]
        ok &= bool(np.all(v * 1024 == np.round(v * 1024)) and np.abs(v).max() < 256)
        ok &= bool(np.array_equal(v.astype(np.float32).astype(np.float64), v))
    return ok


@functools.lru_cache(maxsize=None)
def reference(seed, shape, scale, weight=1.0, grad_mult=1.0, masked=True, q=0.4):
    """The twin on census_case(seed, shape, scale), computed once: (pred, img, mask or None, L, dpred, parts), with the
    exactness preconditions asserted."""
    pred, img, mask = census_case(seed, shape, scale)
    mask = mask if masked else None
    L, g, parts = twin.loss_and_grad(img, pred, mask, scale, weight, q, grad_mult)
    assert warp_exact_ok(parts)
    return pred, img, mask, L, g, parts


def reach(mc):
    """Pixels within 3 of a pixel with mc = 1: the only ones a gradient can reach."""
    n, h, w = mc.shape
    pad = np.pad(mc > 0, ((0, 0), (3, 3), (3, 3)))
    out = np.zeros((n, h, w), bool)
    for dy in range(7):
        for dx in range(7):
            out |= pad[:, dy:dy + h, dx:dx + w]
    return out


def poisoned_case(shape):
    """census_case with NaN, +-inf and +-1e30 in a few flow components (never the centre pixel)."""
    n, h, w = shape
    pred, img, mask = census_case(21, shape)
    pred = pred.copy()
    rng = np.random.default_rng(22)
    bad = np.zeros((n, h, w), bool)
    for k, v in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30, np.nan, np.inf, 1e30]):
        i, y, x = rng.integers(n), rng.integers(h), rng.integers(w)
        if (y, x) == (h // 2, w // 2):
            x -= 1
        pred[i, y, x, k % 2] = v
        bad[i, y, x] = True
    return pred, img, mask, bad


# ------------------------------------------------------------------------------------------------ device helpers
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(pred, img, mask=None, **kw):
    """census_loss on the device -> (loss, S, count, dpred, {G, W, DX, DY, V, c}) as host values."""
    from src.census import census_loss
    loss, S, count, dpred, bufs = census_loss(dev(img), dev(pred), None if mask is None else dev(mask), **kw)
    return float(host(loss)[0]), host(S), float(host(count)[0]), host(dpred), {k: host(v) for k, v in bufs.items()}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))
    print("worst so far: " + ", ".join("%s %.3e" % kv for kv in sorted(WORST.items())))


def check_warp(bufs, count, parts):
    for k in ("G", "W", "DX", "DY"):
        np.testing.assert_array_equal(bufs[k], parts[k].astype(np.float32), err_msg=k)
    np.testing.assert_array_equal(bufs["V"], parts["V"].astype(np.float32))
    assert count == parts["Mc"]


def check_loss_S_and_grad(got_loss, got_S, got_g, L, g, parts):
    if parts["Mc"] == 0:
        assert got_loss == 0.0 and not got_g.any()                 # exactly
        if min(got_S.shape[1:3]) < twin.PATCH:
            assert not got_S.any()
        return
    S = parts["S"]
    s_err, g_err = np.abs(got_S - S).max() / np.abs(S).max(), np.abs(got_g - g).max() / np.abs(g).max()
    print("loss %.9g, twin %.9g (rel %.3e); worst S error %.3e, worst gradient error %.3e of the largest"
          % (got_loss, L, abs(got_loss - L) / abs(L), s_err, g_err))
    note("loss", abs(got_loss - L) / abs(L)), note("S", s_err), note("dpred", g_err)
    assert abs(got_loss - L) <= LOSS_TOL * abs(L), (got_loss, L)
    assert s_err <= GRAD_TOL and g_err <= GRAD_TOL
    assert not got_g[~parts["V"]].any()                            # no gradient where the sample left the partner frame
    assert not got_g[~reach(parts["mc"])].any()                    # ... nor farther than 3 from every counted pixel
    assert np.isfinite(got_S).all() and not got_S[:, ~twin.interior(*got_S.shape[1:3])].any()


# ------------------------------------------------------------------------------------------------ 1. the warp pass
@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_grey_values_warp_and_count_are_exact(shape, scale):
    pred, img, mask, _, _, parts = reference(0, shape, scale)
    if shape == (2, 7, 7):
        assert parts["Mc"] >= 1
    if min(shape[1:]) < twin.PATCH:
        assert parts["Mc"] == 0
    _, _, count, _, bufs = run(pred, img, mask, scale=scale)
    check_warp(bufs, count, parts)
    assert parts["V"].any() and not parts["V"].all()


# ------------------------------------------------------------------------------------------------ 2. loss, S and gradient
@pytest.mark.gpu
@pytest.mark.parametrize("grad_mult", [1.0, 16384.0])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_distance_and_gradient_match_the_twin(shape, scale, grad_mult):
    pred, img, mask, L, g, parts = reference(0, shape, scale, 0.064, grad_mult)
    got_loss, got_S, count, got_g, bufs = run(pred, img, mask, scale=scale, weight=0.064, grad_mult=grad_mult)
    check_warp(bufs, count, parts)
    check_loss_S_and_grad(got_loss, got_S, got_g, L, g, parts)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 7), (4, 10, 135), (2, 19, 9)])
def test_without_a_mask_every_valid_interior_pixel_counts(shape):
    pred, img, _, L, g, parts = reference(1, shape, 1.0, 1.0, 1.0, False)
    assert parts["Mc"] == (parts["V"] & twin.interior(*shape[1:])[None]).sum() >= 1
    got_loss, got_S, count, got_g, bufs = run(pred, img)
    check_warp(bufs, count, parts)
    check_loss_S_and_grad(got_loss, got_S, got_g, L, g, parts)


@pytest.mark.gpu
def test_five_levels_in_one_launch_equal_five_launches():
    """One table of five levels (different sizes, scales and weights, one without an interior) against the same levels one
    launch each: every buffer bit for bit (nothing in a pixel depends on the table), the loss to LOSS_TOL (atomics in
    another order) -- and against the twin."""
    import torch
    from src import _hip
    from src.census import level, level_table
    lib = _hip.lib()
    shapes = [(4, 10, 135), (4, 19, 9), (4, 8, 70), (4, 7, 7), (4, 6, 9)]
    scales, weights = [5.0, 1.0, 0.625, 1.0, 5.0], [0.064, 0.016, 0.004, 0.002, 0.001]
    refs = [reference(3, shp, s, wgt, 16384.0) for shp, s, wgt in zip(shapes, scales, weights)]

    def launch(groups):
        bufs = []
        for pred, img, mask, _, _, _ in refs:
            n, h, w = mask.shape
            junk = lambda *shape: torch.full(shape, -7.0, device="cuda")
            bufs.append(dict(pred=dev(pred), img=dev(img), mask=dev(mask), dpred=junk(n, h, w, 2), grey=junk(n, h, w),
                             warp=junk(3, n, h, w), valid=junk(n, h, w), coef=junk(2, n, h, w),
                             count=torch.zeros(1, device="cuda")))
        loss = torch.zeros(1, device="cuda")
        for grp in groups:
            table = level_table([level(scale=scales[i], weight=weights[i], **bufs[i]) for i in grp])
            _hip.check(lib.fn2_census_warp(table, len(grp), 4, _hip.stream_ptr()))
            _hip.check(lib.fn2_census_cost(table, len(grp), 4, 0.4, _hip.ptr(loss), _hip.stream_ptr()))
            _hip.check(lib.fn2_census_grad(table, len(grp), 4, 16384.0, _hip.stream_ptr()))
        return float(host(loss)[0]), [{k: host(v) for k, v in b.items()} for b in bufs]

    one_loss, one = launch([[0, 1, 2, 3, 4]])
    five_loss, five = launch([[i] for i in range(5)])
    want_loss = sum(r[3] for r in refs)
    assert abs(one_loss - five_loss) <= LOSS_TOL * abs(five_loss) and abs(one_loss - want_loss) <= LOSS_TOL * abs(want_loss)
    for b1, b5, (_, _, _, L, g, parts) in zip(one, five, refs):
        for k in b1:
            np.testing.assert_array_equal(b1[k], b5[k], err_msg=k)
        check_warp(dict(G=b1["grey"], W=b1["warp"][0], DX=b1["warp"][1], DY=b1["warp"][2], V=b1["valid"]),
                   float(b1["count"][0]), parts)
        if parts["Mc"]:
            assert np.abs(b1["dpred"] - g).max() <= GRAD_TOL * np.abs(g).max()
            assert np.abs(b1["coef"][0] - parts["S"]).max() <= GRAD_TOL * np.abs(parts["S"]).max()
        else:
            assert not b1["dpred"].any() and not b1["coef"].any()


# ------------------------------------------------------------------------------------------------ 3. robustness
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 8, 70), (4, 10, 135)])
def test_poisoned_flows_are_invalid_and_every_output_is_finite(shape):
    """NaN, +-inf and +-1e30 in a few flow components: V = 0 there, every buffer is finite, the guard words behind the
    buffers stay, the inputs are unchanged, and everything matches the twin on the same flows (the partner's FRAME is
    sampled, never its flow, so the poison does not travel)."""
    import torch
    from src import _hip
    from src.census import level, level_table
    n, h, w = shape
    pred, img, mask, bad = poisoned_case(shape)
    L, g, parts = twin.loss_and_grad(img, pred, mask)
    assert warp_exact_ok(parts) and not parts["V"][bad].any() and parts["Mc"] >= 1 and np.isfinite(g).all()
    npix, guard = n * h * w, 64
    junk = lambda k: torch.full((k * npix + guard,), -7.0, device="cuda")
    d_pred, d_img, d_mask = dev(pred), dev(img), dev(mask)
    raw = dict(dpred=junk(2), grey=junk(1), warp=junk(3), valid=junk(1), coef=junk(2))
    shapes = dict(dpred=(n, h, w, 2), grey=(n, h, w), warp=(3, n, h, w), valid=(n, h, w), coef=(2, n, h, w))
    views = {k: v[:v.numel() - guard].view(shapes[k]) for k, v in raw.items()}
    scal = torch.zeros(2, device="cuda")
    table = level_table([level(pred=d_pred, img=d_img, mask=d_mask, count=scal[1:], scale=1.0, weight=1.0, **views)])
    _hip.check(_hip.lib().fn2_census_warp(table, 1, n, _hip.stream_ptr()))
    _hip.check(_hip.lib().fn2_census_cost(table, 1, n, 0.4, _hip.ptr(scal), _hip.stream_ptr()))
    _hip.check(_hip.lib().fn2_census_grad(table, 1, n, 1.0, _hip.stream_ptr()))
    for k, v in raw.items():
        got = host(v)
        assert np.all(got[-guard:] == -7.0) and np.isfinite(got).all(), k
    got = {k: host(v) for k, v in views.items()}
    np.testing.assert_array_equal(host(d_pred), pred)              # inputs are only read (NaN == NaN here)
    np.testing.assert_array_equal(host(d_img), img)
    assert not got["valid"][bad].any() and not got["dpred"][bad].any()
    loss, count = (float(v) for v in host(scal))
    check_warp(dict(G=got["grey"], W=got["warp"][0], DX=got["warp"][1], DY=got["warp"][2], V=got["valid"]), count, parts)
    check_loss_S_and_grad(loss, got["coef"][0], got["dpred"], L, g, parts)


# ------------------------------------------------------------------------------------------------ 4. arguments
def level_struct(hip, **kw):
    fake = 0x1000
    names = ("pred", "img", "mask", "dpred", "grey", "warp", "valid", "coef", "count")
    return hip.Fn2CensusLevel(**dict(dict({k: fake for k in names}, h=8, w=9, scale=1.0, weight=1.0), **kw))


def check_invalid_arguments(hip):
    """Every check sits in front of the launch: the pointers are never followed."""
    lib = hip.lib()
    L = hip.Fn2CensusLevel
    ok = lambda **kw: level_struct(hip, **kw)
    warp = lambda table, nl=1, n=2: lib.fn2_census_warp(table, nl, n, None)
    cost = lambda table, nl=1, n=2, q=0.4, acc=0x1000: lib.fn2_census_cost(table, nl, n, q, acc, None)
    grad = lambda table, nl=1, n=2: lib.fn2_census_grad(table, nl, n, 1.0, None)
    cases = [(lambda f: f(None), b"null level table"), (lambda f: f(ok(), 0), b"n_levels"),
             (lambda f: f((L * 9)(*[ok() for _ in range(9)]), 9), b"n_levels"),
             (lambda f: f(ok(), 1, 3), b"even"), (lambda f: f(ok(), 1, 0), b"even"),
             (lambda f: f(ok(h=0)), b"bad size"), (lambda f: f(ok(w=0)), b"bad size"), (lambda f: f(ok(w=-2)), b"bad size"),
             (lambda f: f(ok(h=1 << 16, w=1 << 15)), b"too large"),
             (lambda f: f(ok(pred=0x1004)), b"8-byte aligned"), (lambda f: f(ok(dpred=0x1004)), b"8-byte aligned"),
             (lambda f: f(ok(grey=0x1002)), b"4-byte aligned"), (lambda f: f(ok(count=0x1001)), b"4-byte aligned"),
             (lambda f: f((L * 3)(ok(), ok(), ok(img=None)), 3), b"level 2")]
    cases += [(lambda f, k=k: f(ok(**{k: None})), b"null pointer")
              for k in ("pred", "img", "mask", "dpred", "grey", "warp", "valid", "coef", "count")]
    for f in (warp, cost, grad):
        for call, word in cases:
            rc = call(f)
            assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (word, rc, lib.fn2_last_error())
    for kw, word in ((dict(acc=None), b"loss_accum"), (dict(q=0.0), b"q must"), (dict(q=1.5), b"q must"),
                     (dict(q=float("nan")), b"q must")):
        rc = cost(ok(), **kw)
        assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (word, rc, lib.fn2_last_error())
    with pytest.raises(ValueError):
        hip.check(warp(ok(), 1, 3))


@pytest.mark.gpu
def test_invalid_arguments_on_the_device_box():
    import torch
    from src import _hip
    from src.census import census_loss, level
    check_invalid_arguments(_hip)
    img, pred = torch.zeros(2, 8, 9, 3, device="cuda"), torch.zeros(2, 8, 9, 2, device="cuda")
    for bad_img, bad_pred in ((img[0], pred[0]), (img, pred[:, :3]), (img[..., :2], pred), (img, img), (img[:1], pred[:1]),
                              (img.cpu(), pred.cpu())):
        with pytest.raises(ValueError):
            census_loss(bad_img, bad_pred)
    for bad_mask in (torch.zeros(2, 8, 8, device="cuda"), torch.zeros(2, 8, 9), np.zeros((2, 8, 9), np.float32)):
        with pytest.raises(ValueError):
            census_loss(img, pred, bad_mask)
    for kw in (dict(q=0.0), dict(q=2.0), dict(q=float("nan"))):
        with pytest.raises(ValueError):
            census_loss(img, pred, **kw)
    z = lambda *s: torch.zeros(s, device="cuda")
    good = dict(pred=pred, img=img, mask=z(2, 8, 9), dpred=z(2, 8, 9, 2), grey=z(2, 8, 9), warp=z(3, 2, 8, 9), valid=z(2, 8, 9),
                coef=z(2, 2, 8, 9), count=z(1), scale=1.0, weight=1.0)
    level(**good)
    for k, v in (("warp", z(2, 2, 8, 9)), ("coef", z(2, 8, 9)), ("count", z(2)), ("grey", z(2, 8, 9).double()),
                 ("valid", z(2, 8, 9).cpu()), ("dpred", z(2, 8, 9, 4)[..., :2])):
        with pytest.raises(ValueError):
            level(**dict(good, **{k: v}))
