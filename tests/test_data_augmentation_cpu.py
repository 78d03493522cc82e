"""Host side of the SelFlow-style augmentation (src/data_augmentation.py, csrc/selflow_aug.hip) without a device: the
parameter draws, the rectangle arithmetic, the hash of the NumPy twin, argument validation of the two entry points and
the exclusion check that goes with the GPU colour tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import selflow_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 384, 512


@pytest.fixture(scope="module")
def DA():
    from src import data_augmentation
    return data_augmentation


@pytest.fixture(scope="module")
def hip():
    from src import _hip
    return _hip


def f32view(t, word):
    return t.view(np.float32)[:, word]


def densities(t):
    """Density in percent a uniform record was drawn at, from its threshold (exact to 100 / 2^32)."""
    return t[:, twin.THRESHOLD].astype(np.float64) / 2.0 ** 32 * 100.0


# ------------------------------------------------------------------------------------------------ parameter drawing
def test_same_seed_same_table(DA):
    a = DA.draw_interp_params(np.random.default_rng(7), 64, H, W, num_distrib=3)
    b = DA.draw_interp_params(np.random.default_rng(7), 64, H, W, num_distrib=3)
    c = DA.draw_interp_params(np.random.default_rng(8), 64, H, W, num_distrib=3)
    assert a.dtype == np.uint32 and a.shape == (64, DA.PARAM_WORDS) and np.array_equal(a, b) and not np.array_equal(a, c)
    ea, eb = DA.draw_estimation_params(np.random.default_rng(7), 16)
    fa, fb = DA.draw_estimation_params(np.random.default_rng(7), 16)
    assert np.array_equal(ea, fa) and np.array_equal(eb, fb)


def test_record_layout_matches_the_header(DA):
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert int(re.search(r"#define FN2_SELFLOW_PARAM_WORDS (\d+)", header).group(1)) == DA.PARAM_WORDS == twin.PARAM_WORDS
    for name in ("DISTRIB", "THRESHOLD", "KEY0", "KEY1", "N_RECT", "RECTS", "FLIP_LR", "FLIP_UD", "PERM", "COLOUR_ORDER",
                 "D_BRIGHTNESS", "F_SATURATION", "D_HUE", "F_CONTRAST"):
        value = int(re.search(r"FN2_SF_%s = (\d+)" % name, header).group(1))
        assert getattr(DA, name) == value == getattr(twin, name), name
    assert DA.CHANNEL_PERMUTATIONS == twin.PERMS


def test_every_field_in_the_reference_range(DA):
    n = 3000
    t = DA.draw_interp_params(np.random.default_rng(1), n, H, W, num_distrib=3)
    i32 = t.view(np.int32)
    assert set(np.unique(t[:, twin.DISTRIB])) == {0, 1, 2}
    assert set(np.unique(t[:, twin.FLIP_LR])) == {0, 1} and set(np.unique(t[:, twin.FLIP_UD])) == {0, 1}
    assert set(np.unique(t[:, twin.PERM])) == set(range(6))
    assert set(np.unique(i32[:, twin.COLOUR_ORDER])) == {0, 1, 2, 3}
    for word, lo, hi in ((twin.D_BRIGHTNESS, -0.2, 0.2), (twin.F_SATURATION, 0.5, 1.5), (twin.D_HUE, -0.2, 0.2),
                         (twin.F_CONTRAST, 0.2, 1.4)):
        v = f32view(t, word)
        assert v.min() >= np.float32(lo) and v.max() < np.float32(hi), (word, v.min(), v.max())
        assert v.min() < lo + 0.05 * (hi - lo) and v.max() > hi - 0.05 * (hi - lo)  # the whole range is used
    uni = t[t[:, twin.DISTRIB] == 1]
    d = densities(uni)
    assert d.min() >= 0.01 - 1e-6 and d.max() < 90.0 and (d < 1).any() and (d > 75).any()
    assert (uni[:, twin.N_RECT] == 0).all()
    inv = i32[t[:, twin.DISTRIB] == 2]
    assert set(np.unique(inv[:, twin.N_RECT])) == {2, 3}
    for rec in inv:
        for k in range(3):
            y0, x0, rh, rw = rec[twin.RECTS + 4 * k:twin.RECTS + 4 * k + 4]
            if k >= rec[twin.N_RECT]:
                assert (y0, x0, rh, rw) == (0, 0, 0, 0)
                continue
            assert 0 <= y0 and 0 <= x0 and rh >= 0 and rw >= 0 and y0 + rh <= H and x0 + rw <= W, (y0, x0, rh, rw)
    keep = t[t[:, twin.DISTRIB] == 0]
    assert (keep[:, twin.THRESHOLD] == 0).all() and (keep[:, twin.N_RECT] == 0).all()
    assert (t[:, 25:] == 0).all()  # reserved words
    fast = DA.draw_interp_params(np.random.default_rng(2), 200, H, W, fast_mode=True)
    assert (fast.view(np.int32)[:, twin.COLOUR_ORDER] == 0).all()
    default = DA.draw_interp_params(np.random.default_rng(3), 500, H, W)
    assert set(np.unique(default[:, twin.DISTRIB])) == {0, 1}


def test_switches_of_sample_sparse_flow(DA):
    rng = np.random.default_rng(4)
    assert (DA.draw_interp_params(rng, 300, H, W, invalid_like=1)[:, twin.DISTRIB] == 2).all()
    assert (DA.draw_interp_params(rng, 300, H, W, num_distrib=1)[:, twin.DISTRIB] == 0).all()
    dense = DA.draw_interp_params(rng, 2000, H, W, min_val=1)
    d = densities(dense[dense[:, twin.DISTRIB] == 1])
    assert len(d) > 500 and d.min() >= 10.0 - 1e-6 and d.max() < 90.0
    ff = DA.draw_interp_params(rng, 2000, H, W, min_val=1, ff_like=1)
    d = densities(ff[ff[:, twin.DISTRIB] == 1])
    assert len(d) > 500 and d.min() >= 65.0 - 1e-6 and d.max() < 85.0
    for _ in range(2000):
        assert 65.0 <= DA.get_sampling_density(rng, 1, ff_like=1) < 85.0
        assert 10.0 <= DA.get_sampling_density(rng, 1) < 90.0
        assert 0.01 <= DA.get_sampling_density(rng, 0, ff_like=1) < 10.0  # ff_like narrows the dense case only
    val = DA.draw_validation_params(rng, 100, H, W)  # the reference's validation defaults: invalid-like, dense
    assert (val[:, twin.DISTRIB] == 2).all() and (val.view(np.int32)[:, twin.COLOUR_ORDER] == -1).all()
    assert (val[:, [twin.FLIP_LR, twin.FLIP_UD, twin.PERM]] == 0).all()
    with pytest.raises(ValueError):
        DA.draw_interp_params(rng, 1, H, W, min_val=2)
    with pytest.raises(ValueError):
        DA.draw_interp_params(rng, 1, H, W, num_distrib=0)


def test_estimation_tables_share_flips_and_permutation(DA):
    a, b = DA.draw_estimation_params(np.random.default_rng(5), 400)
    shared = [twin.FLIP_LR, twin.FLIP_UD, twin.PERM]
    assert np.array_equal(a[:, shared], b[:, shared]) and (a[:, twin.DISTRIB] == 0).all() and (b[:, twin.DISTRIB] == 0).all()
    colour = [twin.COLOUR_ORDER, twin.D_BRIGHTNESS, twin.F_SATURATION, twin.D_HUE, twin.F_CONTRAST]
    assert not np.array_equal(a[:, colour], b[:, colour])  # separate colour records (dataloader.py:101-102)
    assert set(np.unique(a.view(np.int32)[:, twin.COLOUR_ORDER])) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ rectangles
def test_rectangle_arithmetic_by_hand(DA):
    # 25 % of 384 x 512 at 4:3: area 49152, w = sqrt(65536) = 256, h = 256 / (4/3) = 192
    assert DA.crop_size(384, 512, 25.0, 4 / 3) == (192, 256)
    # 1 % of 60 x 60 at 16:9: area 36, w = sqrt(64) = 8, h = 8 / (16/9) = 4.5 -> tf.round is half-to-even: 4, not 5
    assert DA.crop_size(60, 60, 1.0, 16 / 9) == (4, 8)
    # 50 % of 20 x 20 at 3:1: area 200, w = round(sqrt(600) = 24.49) = 24 > 20 -> W - 1 = 19; h = round(24 / 3) = 8 from
    # the UNCLIPPED width
    assert DA.crop_size(20, 20, 50.0, 3.0) == (8, 19)
    # 90 % of 100 x 100 at 4:5: area 9000, w = round(84.85) = 85, h = round(85 / 0.8 = 106.25) = 106 > 100 -> H - 1 = 99
    assert DA.crop_size(100, 100, 90.0, 4 / 5) == (99, 85)
    # at 3:1: w = round(164.3) = 164 -> 99, h = round(54.67) = 55
    assert DA.crop_size(100, 100, 90.0, 3.0) == (55, 99)
    # a side EQUAL to the image is kept (the test is "greater")
    assert DA.crop_size(192, 256, 100.0, 4 / 3) == (192, 256)


def test_offsets_stay_inside(DA):
    rng = np.random.default_rng(6)
    seen_h1 = False
    for _ in range(3000):
        h, w = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        density = float(rng.uniform(0.01, 100.0))
        oy, ox, ch, cw = DA.get_random_offset_and_crop(rng, (h, w), density)
        assert 0 <= ch <= h and 0 <= cw <= w and 0 <= oy <= h - ch and 0 <= ox <= w - cw
        seen_h1 |= ch == h - 1
    assert seen_h1
    # the third hole comes with probability 1/2; the second and third are smaller than the first on average
    counts = [len(DA.invalid_like_rectangles(rng, 50.0, H, W)) for _ in range(2000)]
    assert set(counts) == {2, 3} and abs(np.mean(counts) - 2.5) < 5 * 0.5 / np.sqrt(2000)
    areas = np.array([[r[2] * r[3] for r in DA.invalid_like_rectangles(rng, 50.0, H, W)[:2]] for _ in range(500)])
    frac = areas[:, 1] / (H * W)  # density 50 * 2/3 / U[4, 12) = 2.8 .. 8.3 %
    assert frac.min() > 0.026 and frac.max() < 0.086
    first = areas[:, 0] / (H * W)  # 50 %, less where the 3:1 box is cut to W - 1
    assert first.min() > 0.45 and first.max() < 0.51


# ------------------------------------------------------------------------------------------------ the twin's hash
def _fmix32_int(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def test_hash_constants_and_arithmetic():
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert "x *= 0x%08X" % twin.FMIX_C1 in header and "x *= 0x%08X" % twin.FMIX_C2 in header
    assert "u(i) = fmix32(fmix32(i ^ key0) + key1)" in header
    assert (twin.FMIX_C1, twin.FMIX_C2) == (0x85EBCA6B, 0xC2B2AE35)
    kernel = open(os.path.join(ROOT, "flownet2-tf_amd", "csrc", "selflow_aug.hip")).read()
    assert "0x85EBCA6Bu" in kernel and "0xC2B2AE35u" in kernel
    assert _fmix32_int(0) == 0 and int(twin.fmix32(0)) == 0
    rng = np.random.default_rng(9)
    xs = np.concatenate([rng.integers(0, 1 << 32, 500, dtype=np.uint32), np.array([1, 0xFFFFFFFF, 0x80000000], np.uint32)])
    assert [int(v) for v in twin.fmix32(xs)] == [_fmix32_int(int(v)) for v in xs]
    k0, k1 = 0xDEADBEEF, 0xFFFFFFF0  # the inner sum wraps
    want = [_fmix32_int((_fmix32_int(int(i) ^ k0) + k1) & 0xFFFFFFFF) for i in xs]
    assert [int(v) for v in twin.hash_u(xs, k0, k1)] == want


def test_threshold_arithmetic(DA):
    for fn in (lambda p: twin.threshold_of(p), lambda p: DA.density_threshold(np.float32(p) * np.float32(100.0))):
        assert fn(0.0) == 0
        assert fn(0.25) == 1 << 30
        assert fn(1.0) == (1 << 32) - 1 and fn(1.5) == (1 << 32) - 1
    # a tiny p: density 1e-6 % -> p = float32(1e-6) / 100 in float32, floor(p * 2^32)
    p = np.float32(1e-6) / np.float32(100.0)
    num, den = float(p).as_integer_ratio()
    assert DA.density_threshold(1e-6) == twin.threshold_of(p) == (num << 32) // den == 42
    assert DA.density_threshold(25.0) == 1 << 30 and DA.density_threshold(100.0) == (1 << 32) - 1
    h, w = 96, 128
    assert not twin.uniform_mask(h, w, 0, 1, 2).any()  # u < 0 never holds
    assert twin.uniform_mask(h, w, (1 << 32) - 1, 1, 2).sum() >= h * w - 1


@pytest.mark.parametrize("p", [0.01, 0.25, 0.9])
def test_hash_is_bernoulli_enough(p):
    h, w = 96, 128
    for key0, key1 in ((0x243F6A88, 0x85A308D3), (1, 0), (0xFFFFFFFF, 0x9E3779B9)):
        m = twin.uniform_mask(h, w, twin.threshold_of(p), key0, key1)
        n = h * w
        assert abs(int(m.sum()) - p * n) <= 5 * np.sqrt(n * p * (1 - p)), (p, key0, m.sum())
        q = p * p + (1 - p) * (1 - p)
        for name, agree in (("horizontal", m[:, 1:] == m[:, :-1]), ("vertical", m[1:] == m[:-1])):
            sd = np.sqrt(q * (1 - q) / agree.size)
            assert abs(agree.mean() - q) <= 5 * sd, (p, key0, name, agree.mean(), q, sd)


def test_twin_mask_rules():
    rec = twin.empty_params(1)[0]
    rec[twin.DISTRIB] = 2
    rec[twin.N_RECT] = 2
    rec.view(np.int32)[twin.RECTS:twin.RECTS + 8] = (0, 0, 2, 3, 3, 4, 5, 5)
    m = twin.resampled_mask(rec, 5, 7)
    want = np.ones((5, 7), bool)
    want[0:2, 0:3] = False
    want[3:5, 4:7] = False
    assert np.array_equal(m, want)
    assert twin.keeps_resampled(2, 96 * 128) and not twin.keeps_resampled(1, 96 * 128) and not twin.keeps_resampled(0, 100)


# ------------------------------------------------------------------------------------------------ the C surface
def test_argument_validation_without_gpu(hip):
    lib = hip.lib()
    bad, p = hip.ERR_INVALID_ARGUMENT, C.c_void_p(4096)  # never dereferenced: every call below fails validation first
    assert lib.fn2_selflow_workspace_bytes(8, 384, 512) >= 8 * 4 + 2 * 8 * 3 * 4
    assert lib.fn2_selflow_workspace_bytes(8, 384, 512) == lib.fn2_selflow_workspace_bytes(8, 512, 384)
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 15)):
        assert lib.fn2_selflow_workspace_bytes(n, h, w) == -1
        assert lib.fn2_selflow_stats(p, None, p, None, p, 1 << 20, n, h, w, None) == bad and b"bad size" in lib.fn2_last_error()
        assert lib.fn2_selflow_apply(p, None, None, None, None, None, p, None, None, None, None, None, p, None, p, 1 << 20,
                                     n, h, w, None) == bad and b"bad size" in lib.fn2_last_error()
    need = lib.fn2_selflow_workspace_bytes(2, 8, 8)
    rc = lib.fn2_selflow_stats(p, None, None, None, p, need, 2, 8, 8, None)
    assert rc == bad and b"null" in lib.fn2_last_error()
    with pytest.raises(ValueError):
        hip.check(rc)
    assert lib.fn2_selflow_stats(p, None, p, None, None, need, 2, 8, 8, None) == bad
    assert lib.fn2_selflow_stats(p, p, p, None, p, need, 2, 8, 8, None) == bad and b"params_b" in lib.fn2_last_error()
    assert lib.fn2_selflow_stats(p, None, p, None, p, need - 1, 2, 8, 8, None) == bad and b"workspace" in lib.fn2_last_error()
    assert lib.fn2_selflow_stats(p, None, p, None, C.c_void_p(4100), need, 2, 8, 8, None) == bad

    def apply(ins, outs, params=p, params_b=None, ws=p, ws_bytes=need):
        return lib.fn2_selflow_apply(*ins, *outs, params, params_b, ws, ws_bytes, 2, 8, 8, None)

    none6 = [None] * 6
    assert apply([p] * 6, none6) == bad and b"no output" in lib.fn2_last_error()
    assert apply(none6, [p] + [None] * 5) == bad and b"without its input" in lib.fn2_last_error()
    assert apply([p] * 6, [p] * 6, params=None) == bad and b"null" in lib.fn2_last_error()
    assert apply([p] * 6, [p] * 6, ws=None) == bad
    assert apply([p] * 6, [p] * 6) == bad and b"params_b" in lib.fn2_last_error()  # image_b without its colour records
    assert apply([p] * 6, [p] * 6, params_b=p, ws_bytes=need - 1) == bad and b"workspace" in lib.fn2_last_error()
    odd = C.c_void_p(4100)
    assert apply([p, None, p, odd, p, p], [p, None, p, p, p, p]) == bad and b"aligned" in lib.fn2_last_error()
    with pytest.raises(ValueError):
        hip.check(apply([p, None, p, p, p, p], [p, None, p, p, p, odd]))


def test_python_surface_rejects_bad_tables(DA):
    with pytest.raises(ValueError):
        DA._table(np.zeros((2, 31), np.uint32), 2)
    with pytest.raises(ValueError):
        DA._table(np.zeros((2, DA.PARAM_WORDS), np.int32), 2)
    with pytest.raises(ValueError):
        DA.set_rectangles(DA.empty_params(1)[0], [(0, 0, 1, 1)] * 4)


# ------------------------------------------------------------------------------------------------ exclusion check
def test_no_pixel_near_the_hsv_discontinuity_in_the_gpu_colour_cases():
    """At max channel = 0 with a negative channel the saturation jumps, so float32 and float64 may take different
    branches there; the GPU colour test may exclude such pixels.  With its seeds there are none."""
    cases = twin.colour_cases()
    assert sorted({int(o) for _, _, t in cases for o in t.view(np.int32)[:, twin.COLOUR_ORDER]}) == [0, 1, 2, 3]
    for name, img, table in cases:
        out = twin.apply(table, image_a=img)
        assert out["hazards"].shape == img.shape[:3]
        assert out["hazards"].mean() == 0.0, (name, int(out["hazards"].sum()))
        res = out["image_a"]
        assert (res == 0.0).any() and (res == 1.0).any(), name  # values clip at both ends
    # and the counter does count: an exactly black pixel in front of a chain that starts with the hue op
    img = np.full((1, 2, 2, 3), 0.5, np.float32)
    img[0, 0, 0] = 0.0
    table = twin.empty_params(1)
    twin.set_colour(table[0], 3, 0.1, 0.7, 0.1, 0.9)
    assert int(twin.apply(table, image_a=img)["hazards"].sum()) == 1


def test_twin_colour_ops_on_known_pixels():
    rgb = np.array([[[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 1], [0.5, 0.5, 0.5], [0, 0, 0], [1, 0, 0.5]]], np.float64)
    h, s, v = twin.rgb_to_hsv(rgb)
    assert np.allclose(h[0], [0, 1 / 3, 2 / 3, 0.5, 0, 0, 11 / 12]) and np.allclose(s[0], [1, 1, 1, 1, 0, 0, 1])
    assert np.allclose(v[0], [1, 1, 1, 1, 0.5, 0, 1])
    assert np.allclose(twin.hsv_to_rgb(h, s, v), rgb)
    # dh exactly 6 is case 0: red
    assert np.allclose(twin.hsv_to_rgb(np.array([1.0]), np.array([1.0]), np.array([1.0])), [[1, 0, 0]])
    # cyan + half a turn of hue = red; contrast keeps the channel means; no clipping between the ops
    table = twin.empty_params(1)
    twin.set_colour(table[0], 3, 0.0, 1.0, 0.5, 1.0)
    out, _ = twin.colour_chain(np.array([[[0, 1, 1]]], np.float32), table[0])
    assert np.allclose(out, [[[1, 0, 0]]])
    twin.set_colour(table[0], 0, 0.5, 1.0, 0.0, 2.0)   # B then C: x + 0.5 would clip at 1 if clipped in between
    out, _ = twin.colour_chain(np.array([[[0.9, 0.9, 0.9], [0.3, 0.3, 0.3]]], np.float32), table[0])
    assert np.allclose(out, np.clip((np.array([1.4, 0.8]) - 1.1) * 2 + 1.1, 0, 1)[None, :, None] * np.ones(3))
