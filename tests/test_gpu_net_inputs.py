"""The kernels between the sub-networks of the stacked models, op by op through the C ABI: fn2_stack_input (warp +
brightness error + 12-channel concat, flownet_cs.py:21-36), fn2_fusion_input (ChannelNorm x4 + warp x2 + 11-channel
concat, flownet2.py:25-47), their _pf forms, which interpolate the full-resolution flow from predict_flow2 themselves,
and fn2_resize_bilinear_f32, the launch those forms replace.

The references are plain NumPy on the CPU (this module; tests/test_net_inputs_cpu.py checks them against the loop
forms without a device):
  warp              oracle.ops.flow_warp: fp32, the kernel's own validity and truncation decisions
  brightness error  oracle.nn.channel_norm(a - warped) in float64; the norms of fusion likewise
  flow channels     float32(flow) * float32(0.05): one multiply, nothing to contract
  resize            (1) the interpolation in float64 at the kernel's own fp32 coordinates, (2) the oracle's resize at
                    the ideal float64 coordinates

Bounds (u = 2^-24, the unit roundoff of fp32):
  warp        rtol 1e-6, atol 1e-6 * max|b|: four products whose coefficients sum to 1 -- a few u * max|b| in the kernel
              (fused multiply-adds) and in the fp32 reference each; the bound test_flow_warp_matches_oracle accepts
  errors      rtol 1e-6, atol 2e-6 * max(|a|, |b|): the norm is 1-Lipschitz in the warped value, so the warp's 1e-6 enters
              at most sqrt(3) times; the factor 2 covers that and the fp32 sum and square root
  flow norms  rtol 1e-6: two squares, a sum, a square root = 2.5 u relative
  resize (1)  8 u (M + D) |scale|: three interpolations of at most (M + D) each and the multiply, arithmetic rounding only
  resize (2)  (4 u ((in_h - 1) D_y + (in_w - 1) D_x) + 8 u M) |scale|: as (1) plus the fp32 coordinate error, 2 u relative
              on a coordinate below in - 1, times the local slope (the interpolant is continuous across the knots)
with M = max|x| and D the largest difference between adjacent input pixels.  Everything else is bit for bit."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import nn as rnn
from oracle import ops as rops

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
F32 = np.float32
U = 2.0 ** -24
PAYLOAD_NAN = np.array([0x7FC12345], np.uint32).view(F32)[0]   # a quiet NaN that carries a payload

PLAIN_SHAPES = [(2, 9, 11), (3, 1, 5), (1, 7, 1), (1, 33, 70)]
PADS = [0, 1, 3]
VIEWS = [(16, 0), (32, 16)]                                     # (cs, c0): the engine's, and a slot inside a wider buffer
DTYPE_CASES = [((2, 9, 11), 3), ((1, 33, 70), 1)]               # (shape, pad)
PF_SIZES = [((8, 12), (32, 48)), ((5, 7), (18, 26)), ((5, 7), (19, 27)), ((1, 1), (4, 6)), ((3, 4), (1, 8))]
PF_SCALES = [20.0, 0.05, 1.0]
# c; (in_h, in_w) -> (out_h, out_w); n
RESIZE_CASES = [
    (2, (5, 7), (19, 26), 2),            # 1 two-channel kernel
    (2, (96, 128), (384, 512), 2),       # 2 the engine's size
    (2, (4, 300), (6, 1026), 2),         # 3 second x-block, one live lane
    (2, (3, 2), (65538, 2), 1),          # 4 the row count forces the generic kernel
    (2, (5, 7), (19, 27), 2),            # 5 odd width forces the generic kernel
    (3, (9, 13), (4, 6), 2),             # 6 downscale through the generic kernel
    (1, (9, 13), (4, 6), 2),
    (2, (6, 8), (6, 8), 2),              # 7 identity
    (2, (1, 1), (4, 6), 2),              # 8 one-pixel input
    (2, (6, 8), (1, 1), 2),              # 9 one-pixel output
]
RESIZE_SCALES = [20.0, 0.05]
# Sizes whose fp32 coordinates are exact multiples of 1/2 (scales 5/10, 15/15, 7/14): on small integers every operation
# of the interpolation is exact, so the output is ONE rounding -- of the final multiply by `scale` -- and any other order
# of the operations shows in the last bit.  (An even output width admits integer x scales only: (w_in - 1) / odd.)
DYADIC_CASES = [(2, (6, 16), (11, 16)),   # two-channel kernel
                (2, (6, 8), (11, 15)), (3, (6, 8), (11, 15))]   # generic kernel, half weights on both axes


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ inputs
def images(rng, n, h, w, top):
    return ((rng.random((n, h, w, 3)) * top).astype(F32), (rng.random((n, h, w, 3)) * top).astype(F32))


def random_flow(rng, n, h, w):
    """N(0, 4^2): at these sizes a large share of the pixels leaves the image."""
    return (rng.standard_normal((n, h, w, 2)) * 4).astype(F32)


def plant_list(h, w, nan=np.nan):
    """(name, place(y, x) -> (u, v) or None, valid): the flows the kernels' branches turn on.  place answers None where the
    pixel cannot carry the plant: float32(x) + u has to BE the target coordinate.  `valid` is what the reference rules
    (flow_warp.cu.cc:80) say of the warp there.  float32(w - 2^-20) is w itself from w = 16 on (an invalid pixel then: x2 == w),
    so the largest fp32 below w is planted too."""
    def at_x(tx):
        tx = F32(tx)

        def place(y, x):
            u = F32(np.float64(tx) - x)
            return (u, F32(0)) if F32(F32(x) + u) == tx else None
        return place

    def at_y(ty):
        ty = F32(ty)

        def place(y, x):
            v = F32(np.float64(ty) - y)
            return (F32(0), v) if F32(F32(y) + v) == ty else None
        return place

    def raw(u, v, x0=False):
        return lambda y, x: (F32(u), F32(v)) if (x == 0 or not x0) else None

    below = F32(w - 2.0 ** -20)
    return [("x2 == W-1", at_x(w - 1), True),
            ("x2 = W - 2^-20", at_x(below), bool(below < F32(w))),
            ("x2 = largest fp32 below W", at_x(np.nextafter(F32(w), F32(0))), True),
            ("x2 = -0.0", raw(-0.0, 0.0, x0=True), True),
            ("x2 = -1e-7", raw(-1e-7, 0.0, x0=True), False),
            ("y2 == H-1", at_y(h - 1), True),
            ("(NaN, 0)", raw(nan, 0.0), False),
            ("(+inf, -inf)", raw(np.inf, -np.inf), False),
            ("(1e30, -1e30)", raw(1e30, -1e30), False),
            ("(0, 0)", raw(0.0, 0.0), True)]


def plant_rounds(h, w, rotate=0, nan=np.nan):
    """Every plant on a pixel of its own: a list of rounds {(y, x): (name, u, v, valid)}; a shape with fewer pixels than plants
    takes several rounds, one launch each."""
    todo = plant_list(h, w, nan)
    todo = todo[rotate:] + todo[:rotate]
    rounds = []
    while todo:
        taken, rest = {}, []
        for name, place, valid in todo:
            for y, x in itertools.product(range(h), range(w)):
                uv = place(y, x) if (y, x) not in taken else None
                if uv is not None:
                    taken[(y, x)] = (name, uv[0], uv[1], valid)
                    break
            else:
                rest.append((name, place, valid))
        assert taken, "a plant no pixel can carry"
        rounds.append(taken)
        todo = rest
    return rounds


def planted(flow, rnd):
    """`flow` with one round planted in the first AND the last image of the batch."""
    f = flow.copy()
    for (y, x), (_, u, v, _) in rnd.items():
        for n in {0, f.shape[0] - 1}:
            f[n, y, x] = (u, v)
    return f


def check_plants(flow, rnd):
    """The reference's validity on the planted pixels is the one the plant was made for."""
    valid = warp_valid(flow)
    for (y, x), (name, _, _, want) in rnd.items():
        for n in {0, flow.shape[0] - 1}:
            assert bool(valid[n, y, x]) == want, (name, n, y, x)


def pair_rounds(h, w):
    """Rounds for the two flows of fusion: the same plants four places apart, so one warp is valid where the other is not."""
    return list(itertools.zip_longest(plant_rounds(h, w, 0, PAYLOAD_NAN), plant_rounds(h, w, 4, PAYLOAD_NAN), fillvalue={}))


# ------------------------------------------------------------------------------------------------ references
def warp_valid(flow):
    """flow_warp.cu.cc:45-46, :80 in fp32: NaN fails every comparison."""
    n, h, w, _ = flow.shape
    with np.errstate(invalid="ignore"):
        x2 = (np.arange(w, dtype=F32)[None, None, :] + flow[..., 0]).astype(F32)
        y2 = (np.arange(h, dtype=F32)[None, :, None] + flow[..., 1]).astype(F32)
        return (x2 >= 0) & (y2 >= 0) & (x2 < F32(w)) & (y2 < F32(h))


def warp_and_error(a, b, flow):
    """(valid, warp(b, flow) fp32, |a - warp| float64 [n, h, w])"""
    warped = rops.flow_warp(b, flow)
    err = rnn.channel_norm(a.astype(np.float64) - warped.astype(np.float64))[..., 0]
    return warp_valid(flow), warped, err


def flow_norm(flow):
    with np.errstate(invalid="ignore", over="ignore"):
        return rnn.channel_norm(flow.astype(np.float64))[..., 0]


def resize_axis(n_in, n_out):
    """The kernel's own fp32 coordinates: sy = float32(in-1)/float32(out-1), src = float32(y)*sy, floor, min(lo+1, in-1)."""
    s = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = (np.arange(n_out, dtype=F32) * s).astype(F32)
    lo = np.floor(src).astype(np.int64)
    assert lo.min() >= 0 and lo.max() <= n_in - 1
    return lo, np.minimum(lo + 1, n_in - 1), (src - lo.astype(F32)).astype(F32)


def resize_ref1(x, size, scale, dtype=np.float64):
    """Reference 1: the interpolation in `dtype` at the fp32 coordinates, times float32(scale) last.  dtype=float32 is the
    non-fused emulation of the kernel."""
    x = np.asarray(x, dtype)
    ylo, yhi, ly = resize_axis(x.shape[1], size[0])
    xlo, xhi, lx = resize_axis(x.shape[2], size[1])
    ly = ly.astype(dtype)[None, :, None, None]
    lx = lx.astype(dtype)[None, None, :, None]
    tl, tr = x[:, ylo][:, :, xlo], x[:, ylo][:, :, xhi]
    bl, br = x[:, yhi][:, :, xlo], x[:, yhi][:, :, xhi]
    top = (tl + (tr - tl) * lx).astype(dtype)
    bot = (bl + (br - bl) * lx).astype(dtype)
    return ((top + (bot - top) * ly).astype(dtype) * dtype(F32(scale))).astype(dtype)


def resize_ref2(x, size, scale):
    """Reference 2: the oracle's resize of scale * x at the ideal float64 coordinates."""
    return rnn.resize_bilinear_align_corners(np.float64(F32(scale)) * np.asarray(x, np.float64), size)


def dyadic_input(rng, shape):
    return rng.integers(-64, 65, shape).astype(F32)


def resize_exact(x, size, scale):
    """For DYADIC_CASES on dyadic_input: float64 holds every intermediate and the product exactly, the cast rounds once."""
    for n_in, n_out in zip(x.shape[1:3], size):
        assert np.array_equal(resize_axis(n_in, n_out)[2] * 2 % 1, np.zeros(n_out))
    return resize_ref1(x, size, scale).astype(F32)


def resize_bounds(x, scale):
    """(bound against reference 1, bound against reference 2), see the module docstring."""
    x = np.asarray(x, np.float64)
    m = np.abs(x).max()
    dy = np.abs(np.diff(x, axis=1)).max() if x.shape[1] > 1 else 0.0
    dx = np.abs(np.diff(x, axis=2)).max() if x.shape[2] > 1 else 0.0
    s = abs(float(F32(scale)))
    return (8 * U * (m + max(dx, dy)) * s,
            (4 * U * ((x.shape[1] - 1) * dy + (x.shape[2] - 1) * dx) + 8 * U * m) * s)


def check_resize(got, x, size, scale):
    b1, b2 = resize_bounds(x, scale)
    e1 = np.abs(got.astype(np.float64) - resize_ref1(x, size, scale)).max()
    e2 = np.abs(got.astype(np.float64) - resize_ref2(x, size, scale)).max()
    print("resize %s -> %s scale %g: err vs fp32-coordinate reference %.3e (bound %.3e), vs ideal %.3e (bound %.3e)"
          % (x.shape, tuple(size), scale, e1, b1, e2, b2))
    assert e1 <= b1 and e2 <= b2


# ------------------------------------------------------------------------------------------------ checks on a written buffer
def slot_of(raw, n, h, w, pad, cs, c0, esz=4):
    """raw: the buffer's bytes [n, hp, wp, cs * esz].  Asserts that the border, and the channels of the interior outside the
    16-channel slot, keep the sentinel and that every interior pixel was written; returns the slot's bytes [n, h, w, 16 * esz].
    (A split-fp16 group of 8 channels is 32 contiguous bytes, so a slot at c0 % 8 == 0 is a byte range for every format.)"""
    assert raw.dtype == np.uint8 and raw.shape == (n, h + 2 * pad, w + 2 * pad, cs * esz)
    inner = np.zeros(raw.shape[:3], bool)
    inner[:, pad:pad + h, pad:pad + w] = True
    assert (raw[~inner] == SENTINEL).all(), "the border was written"
    px = raw[:, pad:pad + h, pad:pad + w]
    assert (px[..., :c0 * esz] == SENTINEL).all() and (px[..., (c0 + 16) * esz:] == SENTINEL).all(), "a neighbouring channel was written"
    slot = px[..., c0 * esz:(c0 + 16) * esz]
    assert not (slot == SENTINEL).all(axis=-1).any(), "an interior pixel was not written"
    return np.ascontiguousarray(slot)


def close(got, want, rtol, atol, where=None):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if where is not None:
        got, want = got[where], want[where]
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol)


def check_stack_slot(slot, a, b, flow):
    """slot: fp32 [n, h, w, 16] = [a | b | warp(b, flow) | 0.05 * flow | brightness error | 0 0 0 0]."""
    valid, warped, err = warp_and_error(a, b, flow)
    peak_b = float(np.abs(b).max())
    peak = max(peak_b, float(np.abs(a).max()))
    assert np.array_equal(bits(slot[..., 0:3]), bits(a)) and np.array_equal(bits(slot[..., 3:6]), bits(b))
    assert (slot[..., 6:9][~valid] == 0).all()                                  # exactly 0 where the warp leaves the image
    close(slot[..., 6:9], warped, 1e-6, 1e-6 * peak_b, valid)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(bits(slot[..., 9:11]), bits(flow * F32(0.05)))    # one fp32 multiply
    close(slot[..., 11], err, 1e-6, 2e-6 * peak)
    close(slot[..., 11], rnn.channel_norm(a.astype(np.float64))[..., 0], 1e-6, 2e-6 * peak, ~valid)   # invalid: |a|
    assert (bits(slot[..., 12:16]) == 0).all()                                  # +0, bit for bit


def check_norm(got, flow):
    """ChannelNorm of a flow: rtol 1e-6 where it is finite, exactly 0 for a zero flow, NaN / inf for a NaN / inf flow."""
    want = flow_norm(flow)
    fin = np.isfinite(want)
    close(got, want, 1e-6, 0.0, fin)
    zero = (flow == 0).all(-1)
    assert (got[zero] == 0).all()
    nan = np.isnan(flow).any(-1)
    inf = np.isinf(flow).any(-1) & ~nan
    assert np.isnan(got[nan]).all() and np.isposinf(got[inf]).all()
    assert fin.sum() + nan.sum() + inf.sum() == fin.size


def check_fusion_slot(slot, a, b, sd, css):
    """slot: fp32 [n, h, w, 16] = [a | sd | css | |sd| | |css| | |a - warp(b, sd)| | |a - warp(b, css)| | 0 0 0 0 0]."""
    peak = max(float(np.abs(b).max()), float(np.abs(a).max()))
    assert np.array_equal(bits(slot[..., 0:3]), bits(a))
    assert np.array_equal(bits(slot[..., 3:5]), bits(sd)) and np.array_equal(bits(slot[..., 5:7]), bits(css))   # NaN payloads too
    check_norm(slot[..., 7], sd)
    check_norm(slot[..., 8], css)
    norm_a = rnn.channel_norm(a.astype(np.float64))[..., 0]
    for ch, flow in ((9, sd), (10, css)):
        valid, _, err = warp_and_error(a, b, flow)
        close(slot[..., ch], err, 1e-6, 2e-6 * peak)
        close(slot[..., ch], norm_a, 1e-6, 2e-6 * peak, ~valid)
    assert (bits(slot[..., 11:16]) == 0).all()


# ------------------------------------------------------------------------------------------------ launches
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Launcher:
    """The four entry points on sentinel-filled buffers; every method returns the buffer's bytes [n, hp, wp, cs * esz]."""

    def __init__(self, a, b, pad=0, cs=16, c0=0, dtype="f32"):
        from src import _hip
        from src.engine import _CODE, _DT
        self.hip, self.lib = _hip, _hip.lib()
        self.n, self.h, self.w = a.shape[:3]
        self.pad, self.cs, self.c0, self.code, self.tdt = pad, cs, c0, _CODE[dtype], _DT[dtype]
        self.a, self.b = dev(a), dev(b)

    def _out(self, c):
        t = torch.empty((self.n, self.h + 2 * self.pad, self.w + 2 * self.pad, self.cs), dtype=self.tdt, device="cuda")
        t.view(torch.uint8).fill_(SENTINEL)
        return t, self.hip.view(t, c, self.c0, self.code)

    def _done(self, t):
        torch.cuda.synchronize()
        return t.view(torch.uint8).cpu().numpy().reshape(t.shape[:3] + (-1,))

    def flow_buffer(self):
        t = torch.empty((self.n, self.h, self.w, 2), dtype=torch.float32, device="cuda")
        t.view(torch.uint8).fill_(SENTINEL)
        return t

    def stack(self, flow):
        t, v = self._out(12)
        p = self.hip.ptr
        self.hip.check(self.lib.fn2_stack_input(p(self.a), p(self.b), p(flow), C.byref(v), self.pad, self.hip.stream_ptr()))
        return self._done(t)

    def fusion(self, sd, css):
        t, v = self._out(11)
        p = self.hip.ptr
        self.hip.check(self.lib.fn2_fusion_input(p(self.a), p(self.b), p(sd), p(css), C.byref(v), self.pad, self.hip.stream_ptr()))
        return self._done(t)

    def stack_pf(self, pf, scale, flow_out):
        t, v = self._out(12)
        p = self.hip.ptr
        self.hip.check(self.lib.fn2_stack_input_pf(p(self.a), p(self.b), p(pf), pf.shape[1], pf.shape[2], scale,
                                                   None if flow_out is None else p(flow_out), C.byref(v), self.pad,
                                                   self.hip.stream_ptr()))
        return self._done(t)

    def fusion_pf(self, pf_sd, scale_sd, out_sd, pf_css, scale_css, out_css):
        t, v = self._out(11)
        p = self.hip.ptr
        opt = lambda x: None if x is None else p(x)
        self.hip.check(self.lib.fn2_fusion_input_pf(p(self.a), p(self.b), p(pf_sd), scale_sd, opt(out_sd), p(pf_css), scale_css,
                                                    opt(out_css), pf_sd.shape[1], pf_sd.shape[2], C.byref(v), self.pad,
                                                    self.hip.stream_ptr()))
        return self._done(t)

    def slot(self, raw, esz=4):
        return slot_of(raw, self.n, self.h, self.w, self.pad, self.cs, self.c0, esz)


def run_resize(x, size, scale):
    """fn2_resize_bilinear_f32 into a sentinel-filled buffer with a guard behind it: every element written, none beyond."""
    from src import _hip
    n, ih, iw, c = x.shape
    count = n * size[0] * size[1] * c
    out = torch.empty(count + 64, dtype=torch.float32, device="cuda")
    out.view(torch.uint8).fill_(SENTINEL)
    dx = dev(x)
    _hip.check(_hip.lib().fn2_resize_bilinear_f32(_hip.ptr(dx), _hip.ptr(out), n, ih, iw, c, size[0], size[1], scale,
                                                  _hip.stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    sentinel = np.frombuffer(bytes([SENTINEL] * 4), np.uint32)[0]
    assert (got[count:].view(np.uint32) == sentinel).all(), "written beyond the output"
    assert not (got[:count].view(np.uint32) == sentinel).any(), "an element was not written"
    return got[:count].reshape(n, size[0], size[1], c)


# ------------------------------------------------------------------------------------------------ 1. plain forms, f32
@pytest.mark.parametrize("cs,c0", VIEWS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_stack_input_matches_the_references(shape, pad, cs, c0):
    """fn2_stack_input, f32 output, against the module's references under the module's bounds: pass-through and flow
    channels bit for bit, the warp exactly 0 where the reference rules call it invalid, the brightness error |a| there,
    the tail +0, border and neighbouring channels untouched, every interior pixel written.  The planted flows sit in the
    first and the last image; a shape with fewer pixels than plants takes them in several launches."""
    n, h, w = shape
    rng = np.random.default_rng(1000 + 97 * h + w)
    for top in (1.0, 255.0):
        a, b = images(rng, n, h, w, top)
        run = Launcher(a, b, pad, cs, c0)
        base = random_flow(rng, n, h, w)
        print("%s top %g: %.0f%% of the random flows leave the image" % (shape, top, 100 * (1 - warp_valid(base).mean())))
        for rnd in plant_rounds(h, w):
            flow = planted(base, rnd)
            check_plants(flow, rnd)
            slot = run.slot(run.stack(dev(flow))).view(F32)
            check_stack_slot(slot, a, b, flow)


@pytest.mark.parametrize("cs,c0", VIEWS)
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_fusion_input_matches_the_references(shape, pad, cs, c0):
    """fn2_fusion_input likewise; the plants go into flow_sd and flow_css independently (four places apart, with a NaN
    that carries a payload), so one warp is valid where the other is not, and the flows pass through bit for bit."""
    n, h, w = shape
    rng = np.random.default_rng(2000 + 97 * h + w)
    for top in (1.0, 255.0):
        a, b = images(rng, n, h, w, top)
        run = Launcher(a, b, pad, cs, c0)
        base_sd, base_css = random_flow(rng, n, h, w), random_flow(rng, n, h, w)
        for rnd_sd, rnd_css in pair_rounds(h, w):
            sd, css = planted(base_sd, rnd_sd), planted(base_css, rnd_css)
            check_plants(sd, rnd_sd)
            check_plants(css, rnd_css)
            slot = run.slot(run.fusion(dev(sd), dev(css))).view(F32)
            check_fusion_slot(slot, a, b, sd, css)


def test_stack_warp_against_the_flow_warp_kernel():
    """Recorded, not asserted: whether channels 6..8 of fn2_stack_input carry the bits of fn2_flow_warp_f32(b, flow).  warp3
    writes the same expression, but what is contracted into fused multiply-adds is the compiler's choice per kernel.  What
    IS asserted is the bound both are held to against the fp32 reference."""
    from src import _hip
    n, h, w = 1, 33, 70
    rng = np.random.default_rng(5)
    a, b = images(rng, n, h, w, 255.0)
    flow = planted(random_flow(rng, n, h, w), plant_rounds(h, w)[0])
    run = Launcher(a, b)
    d_flow = dev(flow)
    slot = run.slot(run.stack(d_flow)).view(F32)
    out = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda")
    _hip.check(_hip.lib().fn2_flow_warp_f32(_hip.ptr(run.b), _hip.ptr(d_flow), _hip.ptr(out), n, h, w, 3, _hip.stream_ptr()))
    torch.cuda.synchronize()
    warp = out.cpu().numpy()
    same = np.array_equal(bits(slot[..., 6:9]), bits(warp))
    print("stack_input channels 6..8 vs fn2_flow_warp_f32: bit-equal %s, %d of %d values differ, max |diff| %.3e"
          % (same, int((bits(slot[..., 6:9]) != bits(warp)).sum()), warp.size, float(np.abs(slot[..., 6:9] - warp).max())))
    valid, want, _ = warp_and_error(a, b, flow)
    for got in (slot[..., 6:9], warp):
        assert (got[~valid] == 0).all()
        close(got, want, 1e-6, 1e-6 * float(np.abs(b).max()), valid)


# ------------------------------------------------------------------------------------------------ 2. the other formats
def stored(slot32, dtype):
    """The bytes a 16-bit or split-fp16 buffer holds for the fp32 values [..., 16]: torch's round-to-nearest .to() for
    bf16 and f16; per group of 8 channels 8 fp16 hi parts, then 8 lo parts (lo = fp16(v - hi)) for f16x2."""
    from src.engine import _DT
    from src.weights import split_f16x2
    if dtype == "f16x2":
        return np.ascontiguousarray(split_f16x2(slot32)).view(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(slot32)).to(_DT[dtype]).view(torch.uint8).numpy()


@pytest.mark.parametrize("cs,c0", VIEWS)
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f16x2"])
@pytest.mark.parametrize("shape,pad", DTYPE_CASES)
def test_other_formats_store_the_conversion_of_the_f32_output(shape, pad, dtype, cs, c0):
    """Finite flows (|v| < 6e4, fp16's range): the bytes a bf16, f16 or f16x2 launch stores are the host conversion of the
    f32 launch's own output -- which catches a wrong group layout, a wrong rounding or a channel shifted by the 8-channel
    split, whatever the warp computes."""
    n, h, w = shape
    esz = 4 if dtype == "f16x2" else 2
    rng = np.random.default_rng(3000 + h)
    a, b = images(rng, n, h, w, 255.0)
    sd, css = random_flow(rng, n, h, w), random_flow(rng, n, h, w)
    sd[0, 0, 0], css[-1, -1, -1] = (4.5e4, -4.5e4), (-5.9e4, 1e-3)      # norms below fp16's 65504 too
    f32, low = Launcher(a, b, pad, cs, c0), Launcher(a, b, pad, cs, c0, dtype)
    d_sd, d_css = dev(sd), dev(css)
    for want, got in ((f32.stack(d_sd), low.stack(d_sd)), (f32.fusion(d_sd, d_css), low.fusion(d_sd, d_css))):
        want = stored(f32.slot(want).view(F32), dtype)
        got = low.slot(got, esz)
        assert got.shape == want.shape and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ 3. the grid-stride loop
BIG = (1, 1025, 1025)     # 1,050,625 pixels: 2,049 more than the 4096 x 256 lanes of the capped grid


def big_flow(rng, rotate=0):
    """The plants, and invalid flows on the last 2,049 pixels -- the ones only the second trip of the loop reaches."""
    n, h, w = BIG
    rnd = plant_rounds(h, w, rotate)[0]
    flow = planted(random_flow(rng, n, h, w), rnd)
    check_plants(flow, rnd)
    tail = flow.reshape(-1, 2)[-2049:]
    for k, uv in enumerate([(np.nan, 0.0), (np.inf, -np.inf), (1e30, -1e30), (2048.0, 0.0)]):
        tail[(k + rotate) % 4::4] = uv
    assert not warp_valid(flow).reshape(-1)[-2049:].any()
    return flow


def test_stack_input_beyond_the_grid_cap():
    n, h, w = BIG
    assert n * h * w - 4096 * 256 == 2049
    rng = np.random.default_rng(41)
    a, b = images(rng, n, h, w, 1.0)
    flow = big_flow(rng)
    run = Launcher(a, b, pad=1)
    check_stack_slot(run.slot(run.stack(dev(flow))).view(F32), a, b, flow)


def test_fusion_input_beyond_the_grid_cap():
    n, h, w = BIG
    rng = np.random.default_rng(42)
    a, b = images(rng, n, h, w, 1.0)
    sd, css = big_flow(rng), big_flow(rng, 5)
    run = Launcher(a, b, pad=1)
    check_fusion_slot(run.slot(run.fusion(dev(sd), dev(css))).view(F32), a, b, sd, css)


# ------------------------------------------------------------------------------------------------ 4. the _pf forms
def predict_flow2(rng, n, ph, pw, h, w, scale):
    """predict_flow2 values such that about a third of scale * (their interpolation) leaves the h x w image: per axis a
    normal displacement of sigma 0.3 * extent (the interpolation takes some of it away)."""
    return (rng.standard_normal((n, ph, pw, 2)) * np.array([0.3 * w, 0.3 * h]) / scale).astype(F32)


def check_flow_out(got, pf, size, scale):
    """flow_out against fn2_resize_bilinear_f32: bit for bit where that launch takes the two-channel kernel (even width:
    the project's own claim, fn2_common.h:83-92); under the resize bounds against both references in every case."""
    assert not (bits(got) == 0x5A5A5A5A).any()
    check_resize(got, pf, size, scale)
    if size[1] % 2 == 0:
        assert np.array_equal(bits(got), bits(run_resize(pf, size, scale)))


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f16x2"])
@pytest.mark.parametrize("scale", PF_SCALES)
@pytest.mark.parametrize("small,size", PF_SIZES)
def test_stack_input_pf(small, size, scale, dtype):
    """(a) the 16-channel output equals the plain form fed with the flow_out the _pf launch wrote, byte for byte;
    (b) flow_out is the resize launch's output; (c) flow_out = NULL gives the same bytes.  f32: the plain form is held to
    the references at these sizes too."""
    n, (ph, pw), (h, w) = 2, small, size
    rng = np.random.default_rng(4001 + 31 * h + w)
    a, b = images(rng, n, h, w, 1.0)
    pf = predict_flow2(rng, n, ph, pw, h, w, scale)
    run = Launcher(a, b, pad=1, cs=32, c0=16, dtype=dtype)
    d_pf, flow_out = dev(pf), run.flow_buffer()
    got = run.stack_pf(d_pf, scale, flow_out)
    plain = run.stack(flow_out)
    assert np.array_equal(got, plain)                                        # (a)
    flow = flow_out.cpu().numpy()
    print("%.0f%% of the interpolated flows leave the image" % (100 * (1 - warp_valid(flow).mean())))
    check_flow_out(flow, pf, size, scale)                                    # (b)
    assert np.array_equal(run.stack_pf(d_pf, scale, None), got)              # (c)
    slot = run.slot(got, 4 if dtype in ("f32", "f16x2") else 2)
    if dtype == "f32":
        check_stack_slot(slot.view(F32), a, b, flow)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "f16x2"])
@pytest.mark.parametrize("scale", PF_SCALES)
@pytest.mark.parametrize("small,size", PF_SIZES)
def test_fusion_input_pf(small, size, scale, dtype):
    """As test_stack_input_pf, with a scale of its own per flow; (c) also with one of the two flow_out pointers only."""
    n, (ph, pw), (h, w) = 2, small, size
    scale_css = PF_SCALES[(PF_SCALES.index(scale) + 1) % len(PF_SCALES)]
    rng = np.random.default_rng(5000 + 31 * h + w)
    a, b = images(rng, n, h, w, 1.0)
    pf_sd, pf_css = predict_flow2(rng, n, ph, pw, h, w, scale), predict_flow2(rng, n, ph, pw, h, w, scale_css)
    run = Launcher(a, b, pad=1, cs=32, c0=16, dtype=dtype)
    d_sd, d_css, out_sd, out_css = dev(pf_sd), dev(pf_css), run.flow_buffer(), run.flow_buffer()
    got = run.fusion_pf(d_sd, scale, out_sd, d_css, scale_css, out_css)
    assert np.array_equal(got, run.fusion(out_sd, out_css))                  # (a)
    sd, css = out_sd.cpu().numpy(), out_css.cpu().numpy()
    check_flow_out(sd, pf_sd, size, scale)                                   # (b)
    check_flow_out(css, pf_css, size, scale_css)
    assert np.array_equal(run.fusion_pf(d_sd, scale, None, d_css, scale_css, None), got)   # (c)
    only = run.flow_buffer()
    assert np.array_equal(run.fusion_pf(d_sd, scale, None, d_css, scale_css, only), got)
    assert torch.equal(only, out_css)
    slot = run.slot(got, 4 if dtype in ("f32", "f16x2") else 2)
    if dtype == "f32":
        check_fusion_slot(slot.view(F32), a, b, sd, css)


# ------------------------------------------------------------------------------------------------ 5. the resize alone
@pytest.mark.parametrize("scale", RESIZE_SCALES)
@pytest.mark.parametrize("c,small,size,n", RESIZE_CASES)
def test_resize_bilinear_matches_both_references(c, small, size, n, scale):
    """Every branch of fn2_resize_bilinear_f32 (RESIZE_CASES) under the two bounds of the module docstring; every element
    of the output written and none behind it."""
    rng = np.random.default_rng(6000 + size[0] + size[1] + c)
    x = rng.standard_normal((n,) + small + (c,)).astype(F32)
    check_resize(run_resize(x, size, scale), x, size, scale)


@pytest.mark.parametrize("scale", RESIZE_SCALES)
@pytest.mark.parametrize("c,small,size", DYADIC_CASES)
def test_resize_bilinear_is_exact_on_dyadic_inputs(c, small, size, scale):
    """Small integers at half-pixel coordinates: the interpolation is exact whether fused or not, the multiply by `scale`
    rounds once, and the result is the correctly rounded float64 value bit for bit -- in the resize launch and, for two
    channels, in the flow_out of both _pf forms.  Scaling the taps before the interpolation would round four times."""
    rng = np.random.default_rng(8000 + c + size[1])
    x = dyadic_input(rng, (2,) + small + (c,))
    want = resize_exact(x, size, scale)
    assert np.array_equal(bits(run_resize(x, size, scale)), bits(want))
    if c == 2:
        a, b = images(rng, 2, size[0], size[1], 1.0)
        run = Launcher(a, b)
        out, out_sd, out_css, d_x = run.flow_buffer(), run.flow_buffer(), run.flow_buffer(), dev(x)
        run.stack_pf(d_x, scale, out)
        run.fusion_pf(d_x, scale, out_sd, d_x, scale, out_css)
        for got in (out, out_sd, out_css):
            assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_resize_bilinear_identity_returns_the_input():
    """Same size, scale 1: every weight is 0, so the input comes back bit for bit."""
    x = np.random.default_rng(7).standard_normal((2, 6, 8, 2)).astype(F32)
    assert np.array_equal(bits(run_resize(x, (6, 8), 1.0)), bits(x))
