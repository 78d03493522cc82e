"""Without a GPU: the references and checks of tests/test_gpu_net_inputs.py against the loop forms and an fp32 emulation
of the kernels (a check that never fails proves nothing: a few wrong emulations have to be caught too), and the argument
checks of fn2_stack_input, fn2_fusion_input and their _pf forms, which refuse a call before anything is launched."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ops as rops
import test_gpu_net_inputs as G
from test_gpu_net_inputs import F32, SENTINEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ (a) the references
@pytest.mark.parametrize("scale", G.RESIZE_SCALES + [1.0])
@pytest.mark.parametrize("c,small,size,n", G.RESIZE_CASES + [(2, (112, 256), (448, 1024), 1)])
def test_resize_emulation_holds_both_bounds(c, small, size, n, scale):
    """The kernel's arithmetic without fused multiply-adds (fp32 NumPy) stays inside both bounds at every GPU case; the
    kernel's fused form rounds less often."""
    rng = np.random.default_rng(6000 + size[0] + size[1] + c)
    x = rng.standard_normal((n,) + small + (c,)).astype(F32)
    got = G.resize_ref1(x, size, scale, F32)
    assert got.dtype == F32 and got.shape == (n,) + size + (c,)
    G.check_resize(got, x, size, scale)
    if small == size and scale == 1.0:
        assert np.array_equal(G.bits(got), G.bits(x))


@pytest.mark.parametrize("scale", G.RESIZE_SCALES)
@pytest.mark.parametrize("c,small,size", G.DYADIC_CASES)
def test_dyadic_resize_is_exact_and_tells_the_order_of_operations(c, small, size, scale):
    """On the dyadic cases the fp32 emulation IS the rounded float64 value; with the taps scaled before the interpolation
    (inside both error bounds: one more rounding of u M |scale|) it is not."""
    x = G.dyadic_input(np.random.default_rng(8000 + c + size[1]), (2,) + small + (c,))
    want = G.resize_exact(x, size, scale)
    assert np.array_equal(G.bits(G.resize_ref1(x, size, scale, F32)), G.bits(want))
    first = G.resize_ref1((x * F32(scale)).astype(F32), size, 1.0, F32)
    G.check_resize(first, x, size, scale)
    assert np.array_equal(G.bits(first), G.bits(want)) == (scale == 20.0)   # 20 * a small integer is exact either way


def stack_buffer(a, b, flow, pad, cs, c0, warp=rops.flow_warp, k10=0.05):
    """What fn2_stack_input leaves in a sentinel-filled f32 buffer, in fp32 NumPy."""
    n, h, w, _ = a.shape
    raw = np.full((n, h + 2 * pad, w + 2 * pad, cs * 4), SENTINEL, np.uint8)
    warped = warp(b, flow)
    d = (a - warped).astype(F32)
    with np.errstate(invalid="ignore"):
        slot = np.concatenate([a, b, warped, flow[..., :1] * F32(0.05), flow[..., 1:] * F32(k10),
                               np.sqrt((d * d).sum(-1, dtype=F32))[..., None], np.zeros((n, h, w, 4), F32)], -1).astype(F32)
    raw.view(F32)[:, pad:pad + h, pad:pad + w, c0:c0 + 16] = slot
    return raw


def fusion_buffer(a, b, sd, css, pad, cs, c0, swap=False):
    n, h, w, _ = a.shape
    raw = np.full((n, h + 2 * pad, w + 2 * pad, cs * 4), SENTINEL, np.uint8)
    err = [G.warp_and_error(a, b, f)[2].astype(F32)[..., None] for f in ((css, sd) if swap else (sd, css))]
    with np.errstate(over="ignore"):
        norms = [G.flow_norm(f).astype(F32)[..., None] for f in (sd, css)]
    view = raw.view(F32)[:, pad:pad + h, pad:pad + w, c0:c0 + 16]
    view[...] = np.concatenate([a, np.zeros((n, h, w, 4), F32)] + norms + err + [np.zeros((n, h, w, 5), F32)], -1)
    view[..., 3:5].view(np.uint32)[...] = G.bits(sd)      # the flows as bits: a NaN's payload survives
    view[..., 5:7].view(np.uint32)[...] = G.bits(css)
    return raw


@pytest.mark.parametrize("shape", G.PLAIN_SHAPES)
def test_references_on_the_planted_pixels(shape):
    """Every plant lands in the first and the last image with the validity it was made for; oracle.ops.flow_warp takes the
    planted flows (NaN, +-inf, +-1e30 among them) without a warning and agrees with the per-pixel loops bit for bit; the
    emulated buffers pass the GPU file's checks."""
    n, h, w = shape
    rng = np.random.default_rng(11)
    a, b = G.images(rng, n, h, w, 255.0)
    base = G.random_flow(rng, n, h, w)
    names = set()
    for rnd in G.plant_rounds(h, w):
        flow = G.planted(base, rnd)
        G.check_plants(flow, rnd)
        names |= {v[0] for v in rnd.values()}
        with np.errstate(all="raise", under="ignore"):
            vec = rops.flow_warp(b, flow)
        assert np.array_equal(G.bits(vec), G.bits(rops.flow_warp_loops(b, flow)))
        assert (vec[~G.warp_valid(flow)] == 0).all()
        for pad, (cs, c0) in ((0, (16, 0)), (3, (32, 16))):
            slot = G.slot_of(stack_buffer(a, b, flow, pad, cs, c0), n, h, w, pad, cs, c0).view(F32)
            G.check_stack_slot(slot, a, b, flow)
    assert names == {p[0] for p in G.plant_list(h, w)} and len(names) == 10
    nans = []
    for rnd_sd, rnd_css in G.pair_rounds(h, w):
        sd, css = G.planted(base, rnd_sd), G.planted(base[..., ::-1].copy(), rnd_css)
        G.check_plants(sd, rnd_sd)
        G.check_plants(css, rnd_css)
        slot = G.slot_of(fusion_buffer(a, b, sd, css, 1, 32, 16), n, h, w, 1, 32, 16).view(F32)
        G.check_fusion_slot(slot, a, b, sd, css)
        nans += list(G.bits(sd)[np.isnan(sd)]) + list(G.bits(css)[np.isnan(css)])
    assert len(nans) >= 2 and set(nans) == {0x7FC12345}             # the planted NaN keeps its payload


def test_plants_disagree_between_the_two_fusion_flows():
    """One warp is valid where the other is not, in at least one round of every shape with room for it."""
    for _, h, w in G.PLAIN_SHAPES:
        mixed = 0
        for rnd_sd, rnd_css in G.pair_rounds(h, w):
            mixed += sum(1 for k in rnd_sd if k in rnd_css and rnd_sd[k][3] != rnd_css[k][3])
        assert mixed > 0, (h, w)


def test_checks_catch_wrong_arithmetic():
    """Emulations that are wrong in the ways a kernel can be: swapped bilinear weights, `x2 <= W-1` for `x2 < W`, a wrong
    factor in channel 10, the two difference norms exchanged, a write into the border, an unwritten pixel."""
    n, h, w = 2, 9, 11
    rng = np.random.default_rng(12)
    a, b = G.images(rng, n, h, w, 255.0)
    flow = G.planted(G.random_flow(rng, n, h, w), G.plant_rounds(h, w)[0])
    css = G.planted(G.random_flow(rng, n, h, w), G.plant_rounds(h, w, 4)[0])
    check = lambda raw: G.check_stack_slot(G.slot_of(raw, n, h, w, 1, 16, 0).view(F32), a, b, flow)
    check(stack_buffer(a, b, flow, 1, 16, 0))

    def swapped(img, f):   # cTR and cBL exchanged
        valid, _, _, xL, xR, yT, yB, al, be = rops._warp_coords(f)
        al, be, k = al[..., None], be[..., None], np.arange(n)[:, None, None]
        out = ((1 - al) * (1 - be) * img[k, yT, xL] + (1 - al) * be * img[k, yT, xR] + al * (1 - be) * img[k, yB, xL]
               + al * be * img[k, yB, xR])
        return np.where(valid[..., None], out, 0).astype(F32)

    def strict(img, f):    # x2 <= W-1, y2 <= H-1
        out = rops.flow_warp(img, f)
        with np.errstate(invalid="ignore"):
            x2 = np.arange(w, dtype=F32)[None, None, :] + f[..., 0]
            out[x2 > F32(w - 1)] = 0
        return out

    assert not np.array_equal(swapped(b, flow), rops.flow_warp(b, flow))
    for wrong in (dict(warp=swapped), dict(warp=strict), dict(k10=0.5)):
        with pytest.raises(AssertionError):
            check(stack_buffer(a, b, flow, 1, 16, 0, **wrong))
    fcheck = lambda raw: G.check_fusion_slot(G.slot_of(raw, n, h, w, 1, 16, 0).view(F32), a, b, flow, css)
    fcheck(fusion_buffer(a, b, flow, css, 1, 16, 0))
    with pytest.raises(AssertionError):
        fcheck(fusion_buffer(a, b, flow, css, 1, 16, 0, swap=True))
    raw = stack_buffer(a, b, flow, 1, 16, 0)
    raw[0, 0, 3, 5] = 0
    with pytest.raises(AssertionError, match="border"):
        check(raw)
    raw = stack_buffer(a, b, flow, 1, 16, 0)
    raw[1, 4, 4] = SENTINEL
    with pytest.raises(AssertionError, match="not written"):
        check(raw)
    raw = stack_buffer(a, b, flow, 1, 32, 16)
    raw[1, 4, 4, 8] = 0
    with pytest.raises(AssertionError, match="neighbouring"):
        G.slot_of(raw, n, h, w, 1, 32, 16)


def test_stored_formats_on_the_host():
    """The host conversions the GPU file compares stored bytes with: bf16 / f16 round to nearest even, f16x2 = 8 hi parts
    then 8 lo parts per group of 8 channels with hi + lo within 2^-22 relative of the value."""
    v = np.random.default_rng(13).standard_normal((3, 16)).astype(F32) * 100
    v[0, :3] = (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 65504.0)          # ties: to even (down, then up) in bf16
    b = G.stored(v, "bf16").view(np.uint16)
    assert b.shape == (3, 16) and b[0, 0] == 0x3F80 and b[0, 1] == 0x3F82
    assert np.array_equal(G.stored(v, "f16").view(np.float16), v.astype(np.float16))
    x2 = G.stored(v, "f16x2").view(np.float16).reshape(3, 2, 2, 8)   # [.., group, hi|lo, 8]
    back = (x2[:, :, 0].astype(np.float64) + x2[:, :, 1].astype(np.float64)).reshape(3, 16)
    assert np.array_equal(x2[:, :, 0].reshape(3, 16), v.astype(np.float16))
    np.testing.assert_allclose(back, v, rtol=2.0 ** -21, atol=2.0 ** -24)


# ------------------------------------------------------------------------------------------------ (b) argument checks
@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


ENTRY_POINTS = {   # name -> (channels of the view, the flow-like pointers, has predict_flow2 sizes)
    "fn2_stack_input": (12, ("flow",), False),
    "fn2_stack_input_pf": (12, ("pf", "flow_out"), True),
    "fn2_fusion_input": (11, ("flow_sd", "flow_css"), False),
    "fn2_fusion_input_pf": (11, ("pf_sd", "flow_sd_out", "pf_css", "flow_css_out"), True),
}


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_entry_points_are_exported_and_validate_without_a_device(hip, name):
    """Invalid calls only: each is refused with FN2_ERR_INVALID_ARGUMENT and a message that names the op, before anything
    is launched.  Host memory stands in for the pointers."""
    lib = hip.lib()
    channels, flows, has_pf = ENTRY_POINTS[name]
    assert name in hip.PROTOTYPES and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert "int %s(" % name in header
    store = (C.c_char * 8192)()
    base = (C.addressof(store) + 255) & ~255
    slots = {key: base + 256 * k for k, key in enumerate(("a", "b", "data") + flows)}
    op = name[len("fn2_"):].encode()

    def call(dtype=hip.FN2_F32, n=1, c=channels, cs=16, c0=0, h=10, w=12, pad=3, view=True, pf_h=2, pf_w=3, **ptrs):
        p = dict(slots, **ptrs)
        t = hip.Fn2Tensor(p["data"], dtype, n, h, w, c, cs, c0)
        tv = C.byref(t) if view else None
        if name == "fn2_stack_input":
            return lib.fn2_stack_input(p["a"], p["b"], p["flow"], tv, pad, None)
        if name == "fn2_stack_input_pf":
            return lib.fn2_stack_input_pf(p["a"], p["b"], p["pf"], pf_h, pf_w, 20.0, p["flow_out"], tv, pad, None)
        if name == "fn2_fusion_input":
            return lib.fn2_fusion_input(p["a"], p["b"], p["flow_sd"], p["flow_css"], tv, pad, None)
        return lib.fn2_fusion_input_pf(p["a"], p["b"], p["pf_sd"], 20.0, p["flow_sd_out"], p["pf_css"], 0.05, p["flow_css_out"],
                                       pf_h, pf_w, tv, pad, None)

    inputs = [f for f in flows if not f.endswith("_out")]           # a flow_out may be NULL; an input may not
    cases = [({key: None}, b"null") for key in ["a", "b", "data"] + inputs]
    cases += [(dict(view=False), b"null"),
              (dict(c=channels + 1), b"%d channels" % channels), (dict(c=23 - channels), b"%d channels" % channels),
              (dict(n=0), b"n >= 1"), (dict(cs=12), b"8-aligned"), (dict(cs=20), b"8-aligned"), (dict(cs=32, c0=4), b"8-aligned"),
              (dict(cs=32, c0=12), b"8-aligned"), (dict(c0=8), b"8-aligned"), (dict(cs=32, c0=24), b"8-aligned"),
              (dict(cs=32, c0=-8), b"8-aligned"), (dict(dtype=4), b"dtype"), (dict(dtype=-1), b"dtype"),
              (dict(pad=5), op + b": bad border"), (dict(pad=6, w=40), op + b": bad border"), (dict(pad=-1), op + b": bad border"),
              (dict(data=slots["data"] + 8), b"16-byte"), (dict(data=slots["data"] + 4), b"16-byte"),
              (dict(a=slots["a"] + 2), b"4-byte"), (dict(b=slots["b"] + 1), b"4-byte")]
    cases += [({key: slots[key] + 4}, b"8-byte") for key in flows]
    if has_pf:
        cases += [(dict(pf_h=0), b"bad size"), (dict(pf_w=0), b"bad size"), (dict(pf_h=-3), b"bad size")]
    for kw, word in cases:
        rc = call(**kw)
        msg = lib.fn2_last_error()
        assert rc == hip.ERR_INVALID_ARGUMENT and word in msg and msg.startswith(op + b":"), (kw, msg)
        with pytest.raises(ValueError):
            hip.check(rc)
