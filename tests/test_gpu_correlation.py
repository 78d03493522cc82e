"""The cost-volume kernels op by op on the C ABI: corr3_kernel, corr2_kernel, corr_mfma_kernel<.., 1>, the generic
forward kernel and both gradient kernels, at every input / output type and view form they accept, against a float64
NumPy restatement of the formula in include/flownet2_hip.h.

Exact tests use dyadic inputs (multiples of 1/2, plus a split-fp16 lo part of 0 or +-2^-13) under a keep-mask, so
that every partial sum is exactly representable in fp32 in any order: the comparison is assert_array_equal.  Bounded
tests (Gaussian data) assert |got - ref| <= (C + 4) 2^-24 S / C with S = sum_c |a_c| |b_c|, a derived margin (see
_assert_bounded).  Every test first asserts the kernel it means to run through the host-only name queries.

The case tables (EXACT_FUSED, EXACT_OP, EXACT_WS, EXACT_GRAD) are plain data: tests/test_correlation_dispatch_cpu.py
reads them without a GPU to show which kernels the exact tests cover."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

CODE = {"f32": 0, "bf16": 1, "f16": 2, "f16x2": 3}
TNAME = {"f32": "float", "bf16": "__bf16", "f16": "_Float16", "f16x2": "fn2::x2_t"}
TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SMALLEST_C = {"f16x2": 32, "f32": 32, "bf16": 64, "f16": 64}    # one 128-byte channel line
SLAB_C = {"f16x2": 16, "f32": 16, "bf16": 32, "f16": 32}        # one 64-byte slab: corr_mfma_kernel<.., 1>
ACT_NONE, ACT_LEAKY = 0, 1
SENT32, SENT16 = 0xFFC0BEEF, 0xFFC1  # NaN bit patterns: an element that keeps its sentinel shows up as a NaN


def kname(family, dt, out, lines):
    return "%s_kernel<%s, %s, %d>" % (family, TNAME[dt], TNAME[out], lines)


# ------------------------------------------------------------------------------------------- float64 reference
def corr_sums(a, b, md, s2, k=1, s1=1, pad=None):
    """S[n,y,x,(p+gr)*gw+(o+gr)] = sum_{j,i,c} A0[n,y1+j,x1+i,c] * B0[n,y1+j+s2*p,x1+i+s2*o,c] in float64, with
    (y1, x1) = (y, x) * s1 + md - pad and A0 / B0 the inputs, zero outside the image.  The op divides S by k*k*C."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    pad = md if pad is None else pad
    N, H, W, Cn = a.shape
    kr = (k - 1) // 2
    oh = -(-(H + 2 * pad - 2 * (md + kr)) // s1)
    ow = -(-(W + 2 * pad - 2 * (md + kr)) // s1)
    gr = md // s2
    gw = 2 * gr + 1
    ext = pad + md + k  # zero margin wide enough for every displaced read
    A0 = np.zeros((N, H + 2 * ext, W + 2 * ext, Cn))
    B0 = np.zeros_like(A0)
    A0[:, ext:ext + H, ext:ext + W] = a
    B0[:, ext:ext + H, ext:ext + W] = b
    y0 = x0 = ext + md - pad
    out = np.zeros((N, oh, ow, gw * gw))
    for pi in range(gw):
        for oi in range(gw):
            dy, dx = (pi - gr) * s2, (oi - gr) * s2
            acc = np.zeros((N, oh, ow))
            for j in range(k):
                for i in range(k):
                    ya, xa = y0 + j, x0 + i
                    pa = A0[:, ya:ya + (oh - 1) * s1 + 1:s1, xa:xa + (ow - 1) * s1 + 1:s1]
                    pb = B0[:, ya + dy:ya + dy + (oh - 1) * s1 + 1:s1, xa + dx:xa + dx + (ow - 1) * s1 + 1:s1]
                    acc += np.einsum("nyxc,nyxc->nyx", pa, pb)
            out[..., pi * gw + oi] = acc
    return out


def out_shape(shape, args):
    """(N, oh, ow, D) of the op for an input shape and (k, md, s1, s2, pad)."""
    k, md, s1, s2, pad = args
    kr = (k - 1) // 2
    oh = -(-(shape[1] + 2 * pad - 2 * (md + kr)) // s1)
    ow = -(-(shape[2] + 2 * pad - 2 * (md + kr)) // s1)
    return (shape[0], oh, ow, (2 * (md // s2) + 1) ** 2)


def outside_mask(H, W, md, s2):
    """[H, W, D] True where the displaced pixel (y + s2 p, x + s2 o) lies outside the image (k = 1, s1 = 1, pad = md)."""
    gr = md // s2
    d = (np.arange(2 * gr + 1) - gr) * s2
    yo = (np.arange(H)[:, None] + d[None, :] < 0) | (np.arange(H)[:, None] + d[None, :] >= H)   # [H, gw]
    xo = (np.arange(W)[:, None] + d[None, :] < 0) | (np.arange(W)[:, None] + d[None, :] >= W)   # [W, gw]
    return (yo[:, None, :, None] | xo[None, :, None, :]).reshape(H, W, -1)


def grad_sums(g, a, b, md, s2):
    """kernel 1, stride_1 1, pad = md (the comment above correlation_grad_tiled_kernel in ops.hip), float64, undivided:
    SA[n,y,x,c] = sum_{p,o} g[n,y,x,(p,o)] B0[n,y+s2 p,x+s2 o,c],  SB[n,y,x,c] = sum_{p,o} g[n,y-s2 p,x-s2 o,(p,o)] A0[..same..,c]."""
    g, a, b = (np.asarray(t, np.float64) for t in (g, a, b))
    N, H, W, Cn = a.shape
    gr = md // s2
    gw = 2 * gr + 1
    A0 = np.zeros((N, H + 2 * md, W + 2 * md, Cn))
    B0 = np.zeros_like(A0)
    A0[:, md:md + H, md:md + W] = a
    B0[:, md:md + H, md:md + W] = b
    SA, SB0 = np.zeros_like(a), np.zeros_like(A0)
    for pi in range(gw):
        for oi in range(gw):
            dy, dx = (pi - gr) * s2, (oi - gr) * s2
            gd = g[..., pi * gw + oi][..., None]
            SA += gd * B0[:, md + dy:md + dy + H, md + dx:md + dx + W]
            SB0[:, md + dy:md + dy + H, md + dx:md + dx + W] += gd * a
    return SA, SB0[:, md:md + H, md:md + W]


# ------------------------------------------------------------------------------------------- inputs
def keep_fraction(Cn):
    """At most ~64 non-zero channels per pixel on average whatever C is (the exactness precondition is asserted)."""
    return 0.25 if Cn >= 256 else min(0.75, 64.0 / Cn)


@functools.lru_cache(maxsize=None)
def dyadic(shape, seed, lo=False):
    """float64 values hi + lo under a random keep-mask: hi a multiple of 1/2 with |hi| <= 2, lo in {0, +-2^-13} (a normal
    fp16, below half an ulp of any non-zero hi) when `lo`, else 0."""
    rng = np.random.default_rng(seed)
    keep = rng.random(shape) < keep_fraction(shape[-1])
    x = rng.integers(-4, 5, shape) / 2.0
    if lo:
        x = x + rng.integers(-1, 2, shape) * 2.0 ** -13 * (x != 0)  # never alone: it would be a hi part, and 2^-26 products
    x = x * keep
    x.setflags(write=False)
    return x


def split_parts(x):
    """Split-fp16 parts of fp32-representable values, element by element: hi = fp16(x), lo = fp16(x - hi)."""
    x32 = np.asarray(x, np.float32)
    hi = x32.astype(np.float16)
    lo = (x32 - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def round_to(dt, x):
    """x rounded to the input type on the host, as float64."""
    x32 = np.asarray(x, np.float32)
    if dt == "f32":
        return x32.astype(np.float64)
    if dt == "f16x2":
        hi, lo = split_parts(x32)
        return hi.astype(np.float64) + lo.astype(np.float64)
    return torch.from_numpy(x32).to(TORCH[dt]).double().numpy()


def assert_exact_preconditions(dt, a, b, lo):
    """The reference-side preconditions of an exact test."""
    for x in (a, b):
        assert np.array_equal(round_to(dt, x), x), "a value does not survive the cast to %s" % dt
    if lo:
        assert dt == "f16x2"
        for x in (a, b):
            assert (split_parts(x)[1] != 0).mean() >= 0.10
    nz = max(int((a != 0).sum(-1).max()), int((b != 0).sum(-1).max()))
    assert nz * np.abs(a).max() * np.abs(b).max() * 2.0 ** 14 < 2.0 ** 24, nz


@functools.lru_cache(maxsize=None)
def fused_reference(dt, shape, md, s2, lo, seed):
    """(a, b, exact float64 sums the kernel family computes).  corr2 / corr3 on split fp16 form
    hi*hi + hi*lo + lo*hi; with lo == 0 (every other type, and the corr_mfma cases) that is the plain product."""
    a, b = dyadic(shape, seed, lo), dyadic(shape, seed + 1, lo)
    assert_exact_preconditions(dt, a, b, lo)
    if lo:
        (ah, al), (bh, bl) = split_parts(a), split_parts(b)
        S = corr_sums(ah, bh, md, s2) + corr_sums(ah, bl, md, s2) + corr_sums(al, bh, md, s2)
    else:
        S = corr_sums(a, b, md, s2)
    assert np.array_equal(S.astype(np.float32), S)  # the sums themselves are fp32 numbers
    S.setflags(write=False)
    return a, b, S


# ------------------------------------------------------------------------------------------- device buffers
def _lib():
    from src import _hip
    return _hip, _hip.lib()


def _up8(n):
    return (n + 7) // 8 * 8


def _storage(dt, logical):
    """Logical fp32 [N, H, W, cs] (NaN allowed) -> flat CPU torch tensor in the storage layout of `dt`."""
    from src import weights as W
    x32 = np.ascontiguousarray(logical, np.float32)
    if dt == "f32":
        return torch.from_numpy(x32).reshape(-1)
    if dt == "f16x2":
        assert x32.shape[-1] % 8 == 0
        return torch.from_numpy(W.split_f16x2(x32)).reshape(-1)  # fp16, two per logical element
    return torch.from_numpy(x32).to(TORCH[dt]).reshape(-1)


def _guarded(dt, body_flat, guard_elems):
    """[NaN guard | body | NaN guard] on the device; returns (buffer, byte offset of the body)."""
    per = 2 if dt == "f16x2" else 1  # storage items per logical element
    g = guard_elems * per
    buf = torch.full((g + body_flat.numel() + g,), float("nan"), dtype=body_flat.dtype)
    buf[g:g + body_flat.numel()] = body_flat
    return buf.cuda(), g * body_flat.element_size()


class FeatureView:
    """A feature tensor as channels [c0, c0 + C) of a [N, H, W, cs] buffer.  Every other channel is NaN (both halves for
    split fp16), and the buffer sits between two NaN guard regions of at least one image row."""

    def __init__(self, dt, x, cs=None, c0=0):
        _hip, _ = _lib()
        N, H, W, Cn = x.shape
        cs = Cn if cs is None else cs
        full = np.full((N, H, W, cs), np.nan, np.float32)
        full[..., c0:c0 + Cn] = x
        self.buf, off = _guarded(dt, _storage(dt, full), _up8(W * cs))
        self.t = _hip.Fn2Tensor(self.buf.data_ptr() + off, CODE[dt], N, H, W, Cn, cs, c0)


class OutputView:
    """Channels [c0, c0 + D) of a sentinel-filled [N, H, W, cs] buffer between sentinel guards."""

    def __init__(self, dt, N, H, W, D, cs, c0):
        _hip, _ = _lib()
        self.dt, self.shape, self.D, self.cs, self.c0 = dt, (N, H, W), D, cs, c0
        self.total = N * H * W * cs
        self.guard = _up8(W * cs)
        n_log = self.guard + _up8(self.total) + self.guard
        if dt == "f32":
            self.buf = torch.full((n_log,), SENT32 - (1 << 32), dtype=torch.int32).cuda()
            esz = 4
        else:
            self.buf = torch.full((n_log * (2 if dt == "f16x2" else 1),), SENT16 - (1 << 16), dtype=torch.int16).cuda()
            esz = 4 if dt == "f16x2" else 2
        assert self.buf.data_ptr() % 32 == 0
        self.t = _hip.Fn2Tensor(self.buf.data_ptr() + self.guard * esz, CODE[dt], N, H, W, D, cs, c0)

    def read(self):
        """Checks the sentinels (as integers) and returns the slice: float32 [N, H, W, D] for f32 / bf16 / f16 (the 16-bit
        values widened exactly), (hi, lo) float16 arrays for split fp16.  Every element inside must have been written:
        the sentinels are NaNs, and the slice must hold none."""
        N, H, W = self.shape
        raw = self.buf.cpu().numpy()
        if self.dt == "f16x2":
            # split-fp16 storage is grouped by address: 8 hi halves then 8 lo halves per 32 bytes; logical element e of the
            # allocation owns hi[e] and lo[e], wherever a view's channel stride puts the group boundaries
            phys = raw.view(np.uint16).reshape(-1, 2, 8)
            planes = [phys[:, 0, :].reshape(-1), phys[:, 1, :].reshape(-1)]
        else:
            planes = [raw.view(np.uint32 if self.dt == "f32" else np.uint16)]
        sent = SENT32 if self.dt == "f32" else SENT16
        got = []
        for bits in planes:
            assert np.all(bits[:self.guard] == sent) and np.all(bits[self.guard + self.total:] == sent), "guard written"
            body = bits[self.guard:self.guard + self.total].reshape(N, H, W, self.cs)
            assert np.all(body[..., :self.c0] == sent) and np.all(body[..., self.c0 + self.D:] == sent), \
                "bytes outside the output slice changed"
            inside = np.ascontiguousarray(body[..., self.c0:self.c0 + self.D])
            if self.dt == "f32":
                val = inside.view(np.float32)
            elif self.dt == "bf16":
                val = (inside.astype(np.uint32) << 16).view(np.float32)
            else:
                val = inside.view(np.float16)
            assert not np.isnan(val).any(), "an element of the slice was not written (or is NaN)"
            got.append(val)
        if self.dt == "f16x2":
            return got[0], got[1]
        return got[0].astype(np.float32)


def expected_in(dt, ref32):
    """The fp32 reference as the output type stores it: torch's round-to-nearest-even cast for bf16 / f16, the split
    (W.split_f16x2's arithmetic, element by element) for split fp16."""
    if dt == "f32":
        return ref32
    if dt == "f16x2":
        return split_parts(ref32)
    return torch.from_numpy(ref32).to(TORCH[dt]).float().numpy()


def joined(dt, got):
    """Device output of any type as float64 values."""
    if dt == "f16x2":
        return got[0].astype(np.float64) + got[1].astype(np.float64)
    return got.astype(np.float64)


def fused_kernel_name(va, vb, vo, md, s2):
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.fn2_correlation_fused_kernel_name(C.byref(va), C.byref(vb), C.byref(vo), md, s2, buf, 128)
    assert rc == 0, lib.fn2_last_error()
    return buf.value.decode()


def op_kernel_name(shape, args, ws):
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.fn2_correlation_f32_kernel_name(*shape, *args, int(ws), buf, 128)
    assert rc == 0, lib.fn2_last_error()
    return buf.value.decode()


def grad_kernel_name(shape, args):
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.fn2_correlation_grad_f32_kernel_name(*shape, *args, buf, 128)
    assert rc == 0, lib.fn2_last_error()
    return buf.value.decode()


def run_fused(case, a, b, act=ACT_NONE):
    """One fn2_correlation_fused call of a case (see EXACT_FUSED) on the given logical inputs; asserts the kernel first."""
    _hip, lib = _lib()
    assert "FN2_CORR3_DBG" not in os.environ
    dt, out = case["dt"], case["out"]
    N, H, W, Cn = case["shape"]
    md, s2 = case["attrs"]
    D = (2 * (md // s2) + 1) ** 2
    if case.get("halves"):  # a and b are the batch halves of one [2N, H, W, C] buffer (the engine's fused towers)
        both = FeatureView(dt, np.concatenate([a, b], 0))
        ta = _hip.Fn2Tensor(both.t.data, CODE[dt], N, H, W, Cn, Cn, 0)
        tb = _hip.Fn2Tensor(both.t.data + N * H * W * Cn * (2 if dt in ("bf16", "f16") else 4), CODE[dt], N, H, W, Cn, Cn, 0)
        keep = (both,)
    else:
        (a_extra, a_c0), (b_extra, b_c0) = case["a_view"] or (0, 0), case["b_view"] or (0, 0)
        av, bv = FeatureView(dt, a, Cn + a_extra, a_c0), FeatureView(dt, b, Cn + b_extra, b_c0)
        ta, tb, keep = av.t, bv.t, (av, bv)
    cs, c0 = case["out_view"] or (D, 0)
    ov = OutputView(out, N, H, W, D, cs, c0)
    assert fused_kernel_name(ta, tb, ov.t, md, s2) == case["kernel"]
    _hip.check(lib.fn2_correlation_fused(C.byref(ta), C.byref(tb), C.byref(ov.t), md, s2, act, _hip.stream_ptr()))
    torch.cuda.synchronize()
    del keep
    return ov.read()


def fcase(kernel_family, dt, shape_hw, Cn, attrs=(20, 2), out=None, out_view=None, a_view=None, b_view=None, N=2,
          corr3="1", lo=None, lines=None, halves=False, tag=""):
    """A fused case.  a_view / b_view are (extra channels, c0); out_view is (cs, c0); corr3 is FN2_CORR3's value."""
    out = out or "f32"
    esz = 2 if dt in ("bf16", "f16") else 4
    lines = lines or Cn * esz // (64 if kernel_family == "corr_mfma" else 128)
    lo = (dt == "f16x2" and kernel_family != "corr_mfma") if lo is None else lo
    ident = "%s-%s-%s-%dx%dx%dx%d-md%d-s%d-%s%s" % (kernel_family, dt, out, N, shape_hw[0], shape_hw[1], Cn, attrs[0], attrs[1],
                                                  "dense" if out_view is None else "cs%d.c0%d" % out_view, tag)
    return dict(id=ident, family=kernel_family, dt=dt, out=out, shape=(N, shape_hw[0], shape_hw[1], Cn), attrs=attrs,
                out_view=out_view, a_view=a_view, b_view=b_view, corr3=corr3, lo=lo, halves=halves,
                kernel=kname(kernel_family, dt, out, lines))


IN16 = ("f16x2", "bf16", "f16")
ALL = ("f32", "f16x2", "bf16", "f16")
AV, BV = (16, 8), (32, 16)  # a: cs = C + 16, c0 = 8;  b: cs = C + 32, c0 = 16


def _exact_fused_cases():
    cs = []
    # ---- corr3: (20, 2), H % 4 == 0
    for dt in IN16:
        c = SMALLEST_C[dt]
        cs += [fcase("corr3", dt, (4, 7), c),                 # image smaller than the displacement range both ways
               fcase("corr3", dt, (8, 64), c),                # exactly one x block
               fcase("corr3", dt, (8, 65), c),                # the second block holds one pixel
               fcase("corr3", dt, (12, 130), c, N=1),         # three blocks, the last ragged
               fcase("corr3", dt, (44, 33), c, N=1)]          # rows 20..23 use all 21 displacement rows; 8 / 8 / 5-row chunks
        cs += [fcase("corr3", dt, (8, 65), c * m) for m in (2, 4, 8)]   # every nl in {1, 2, 4, 8}
        same_view = (456, 8) if dt == "f16x2" else None                # split-fp16 out on corr3: group-aligned views only
        cs += [fcase("corr3", dt, (8, 65), c, out=dt, out_view=same_view),
               fcase("corr3", dt, (8, 65), c, out=dt, out_view=(480, 32) if dt == "f16x2" else (473, 32)),
               fcase("corr3", dt, (8, 65), c, out_view=(473, 32)),
               fcase("corr3", dt, (8, 65), c, a_view=AV, b_view=BV, tag="-views"),
               fcase("corr3", dt, (8, 65), c, halves=True, tag="-halves")]
    # ---- corr2
    for dt in ALL:
        c = SMALLEST_C[dt]
        cs += [fcase("corr2", dt, (6, 65), c), fcase("corr2", dt, (9, 70), c)]   # H % 4 != 0
        if dt != "f32":
            cs.append(fcase("corr2", dt, (8, 65), c, corr3="0", tag="-FN2_CORR3=0"))
        # lo = md - (md / s2) * s2 != 0; the widest window that fits; 41 x 41 displacements; a narrow band
        cs += [fcase("corr2", dt, (6, 70), c, attrs=at, N=1) for at in ((21, 2), (5, 3), (24, 2), (20, 1), (4, 1))]
        cs += [fcase("corr2", dt, (6, 65), c, out=dt, out_view=(473, 32)),
               fcase("corr2", dt, (6, 65), c, a_view=AV, b_view=BV, out_view=(473, 32), tag="-views")]
    # split-fp16 out that is not group aligned takes corr2's element-wise stores, even where corr3 serves the geometry
    cs += [fcase("corr2", "f16x2", (8, 65), 32, out="f16x2", out_view=v) for v in (None, (473, 32), (450, 9))]
    # ---- corr_mfma, one 64-byte slab.  Split-fp16 input is joined to fp32 operands there: exact with lo == 0 only, and
    # the launch wants every split-fp16 view group aligned (the output stride included)
    for dt in ALL:
        c = SLAB_C[dt]
        dense = (448, 0) if dt == "f16x2" else None
        cs += [fcase("corr_mfma", dt, (6, 65), c, attrs=at, out_view=dense) for at in ((20, 2), (21, 2))]
        cs += [fcase("corr_mfma", dt, (6, 65), c, out=dt, out_view=(456, 8) if dt == "f16x2" else (473, 32)),
               fcase("corr_mfma", dt, (6, 65), c, a_view=AV, b_view=BV, out_view=(480, 32) if dt == "f16x2" else (473, 32),
                     tag="-views")]
    return cs


EXACT_FUSED = _exact_fused_cases()

# the fp32 op surface: (shape, (k, md, s1, s2, pad), kernel)
EXACT_OP = [
    ((1, 12, 14, 8), (3, 2, 2, 1, 3), "correlation_generic_kernel"),    # k = 3, s1 = 2, pad != md; k*k*C = 72
    ((1, 8, 8, 5), (1, 3, 1, 3, 3), "correlation_generic_kernel"),      # C = 5
    ((2, 8, 70, 96), (1, 20, 1, 2, 20), "correlation_generic_kernel"),  # three 128-byte lines: no matrix-core kernel takes it
    ((2, 6, 65, 32), (1, 20, 1, 2, 20), "corr2_kernel<float, float, 1>"),
    ((2, 6, 65, 16), (1, 20, 1, 2, 20), "corr_mfma_kernel<float, float, 1>"),
]
# fn2_correlation_f32_ws with a sufficient workspace: corr3 on split-fp16 copies
EXACT_WS = [((2, 8, 65, 32), "corr3_kernel<fn2::x2_t, float, 1>"), ((2, 8, 65, 256), "corr3_kernel<fn2::x2_t, float, 8>")]
ATTRS_C = (1, 20, 1, 2, 20)  # the FlowNetC call site
TILED = "correlation_grad_tiled_kernel<true, 16, 10, 2>"  # grad_a; grad_b is the <false, ..> instantiation of the same launch
EXACT_GRAD = [
    ((2, 5, 16, 8), ATTRS_C, TILED),      # one full tile, a partly filled lane block
    ((1, 5, 17, 256), ATTRS_C, TILED),    # the second tile holds one pixel
    ((1, 5, 37, 300), ATTRS_C, TILED),    # three tiles, two channel blocks, C not a power of two
    ((1, 44, 17, 8), ATTRS_C, TILED),     # rows 20..23 see all 21 displacement rows
    ((1, 44, 37, 8), ATTRS_C, TILED),
    ((1, 6, 7, 2), (3, 2, 2, 1, 3), "correlation_grad_kernel"),   # k = 3, s1 = 2
    ((2, 5, 6, 4), (1, 4, 1, 1, 4), "correlation_grad_kernel"),   # s2 = 1, md = 4
]


@pytest.fixture(autouse=True)
def _corr3_switch_unset(monkeypatch):
    assert "FN2_CORR3_DBG" not in os.environ  # corr3's ablation bits: results are wrong when set
    monkeypatch.delenv("FN2_CORR3", raising=False)


# ------------------------------------------------------------------------------------------- CPU checks of the helpers
def test_reference_agrees_with_the_oracle():
    from oracle import ops as ref
    for shape, args in (((2, 6, 9, 8), (1, 20, 1, 2, 20)), ((1, 7, 9, 4), (1, 5, 1, 3, 5)), ((1, 12, 14, 8), (3, 2, 2, 1, 3)),
                        ((1, 8, 8, 5), (1, 3, 1, 3, 3))):
        a, b = dyadic(shape, 1), dyadic(shape, 2)
        k, md, s1, s2, pad = args
        want = ref.correlation(a, b, *args)
        np.testing.assert_allclose(corr_sums(a, b, md, s2, k, s1, pad) / (k * k * shape[3]), want, rtol=1e-6, atol=1e-7)
    shape = (1, 5, 18, 8)
    a, b, g = dyadic(shape, 3), dyadic(shape, 4), dyadic(shape[:3] + (441,), 5)
    SA, SB = grad_sums(g, a, b, 20, 2)
    da, db = ref.correlation_grad(g, a, b, *ATTRS_C)
    np.testing.assert_allclose(SA / 8, da, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(SB / 8, db, rtol=1e-6, atol=1e-7)


def test_dyadic_inputs_have_the_stated_properties():
    from src import weights as W
    x = dyadic((1, 8, 70, 256), 0, True)
    x32 = x.astype(np.float32)
    assert np.array_equal(x32, x)
    assert np.array_equal(W.join_f16x2(W.split_f16x2(x32)), x32)  # the split round-trips exactly
    hi, lo = split_parts(x32)
    assert np.array_equal(W.split_f16x2(x32).reshape(-1, 2, 8)[:, 1].reshape(x.shape), lo)  # split_parts is W.split_f16x2
    assert 0.10 <= (lo != 0).mean() <= 0.20
    assert np.all(np.isin(np.abs(lo.astype(np.float64)), (0.0, 2.0 ** -13)))
    assert_exact_preconditions("f16x2", x, dyadic((1, 8, 70, 256), 1, True), True)


# ------------------------------------------------------------------------------------------- exact forward tests
def _compare_exact(case, got, ref32):
    N, H, W, _ = case["shape"]
    want = expected_in(case["out"], ref32)
    outside = np.broadcast_to(outside_mask(H, W, *case["attrs"]), ref32.shape)
    if case["out"] == "f16x2":
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        assert np.all(got[0][outside] == 0) and np.all(got[1][outside] == 0)
    else:
        np.testing.assert_array_equal(got, want)
        assert np.all(got[outside] == 0)  # displacements that fall outside the image


@gpu
@pytest.mark.parametrize("case", EXACT_FUSED, ids=[c["id"] for c in EXACT_FUSED])
def test_fused_exact(case, monkeypatch):
    if case["corr3"] != "1":
        monkeypatch.setenv("FN2_CORR3", case["corr3"])
    md, s2 = case["attrs"]
    a, b, S = fused_reference(case["dt"], case["shape"], md, s2, case["lo"], 11)
    Cn = case["shape"][3]
    assert Cn & (Cn - 1) == 0  # 1 / C is exact
    ref32 = (S / Cn).astype(np.float32)
    assert np.array_equal(ref32, S / Cn)
    if case["shape"][0] > 1:
        assert not np.array_equal(ref32[0], ref32[1])  # the two images hold different data
    _compare_exact(case, run_fused(case, a, b), ref32)


def _run_op(shape, args, a, b, ws=None, ws_bytes=0, use_ws_entry=False):
    _hip, lib = _lib()
    assert "FN2_CORR3_DBG" not in os.environ
    k, md, s1, s2, pad = args
    N, H, W, Cn = shape
    ta = torch.from_numpy(np.asarray(a, np.float32)).cuda()
    tb = torch.from_numpy(np.asarray(b, np.float32)).cuda()
    out = torch.full(out_shape(shape, args), float("nan"), dtype=torch.float32, device="cuda")
    if use_ws_entry:
        _hip.check(lib.fn2_correlation_f32_ws(_hip.ptr(ta), _hip.ptr(tb), _hip.ptr(out), N, H, W, Cn, *args,
                                              None if ws is None else _hip.ptr(ws), ws_bytes, _hip.stream_ptr()))
    else:
        _hip.check(lib.fn2_correlation_f32(_hip.ptr(ta), _hip.ptr(tb), _hip.ptr(out), N, H, W, Cn, *args, _hip.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize("shape,args,kernel", EXACT_OP)
def test_op_surface_exact(shape, args, kernel):
    """fn2_correlation_f32 on dyadic fp32 data: float32(S) / float32(k*k*C), one correctly rounded division of the exact
    sum (exact outright when k*k*C is a power of two)."""
    k, md, s1, s2, pad = args
    assert op_kernel_name(shape, args, False) == kernel
    a, b = dyadic(shape, 21), dyadic(shape, 22)
    assert_exact_preconditions("f32", a, b, False)
    S = corr_sums(a, b, md, s2, k, s1, pad)
    assert np.array_equal(S.astype(np.float32), S) and np.abs(S).max() > 0
    want = S.astype(np.float32) / np.float32(k * k * shape[3])
    np.testing.assert_array_equal(_run_op(shape, args, a, b), want)


@gpu
@pytest.mark.parametrize("shape,kernel", EXACT_WS)
def test_workspace_entry_exact_and_its_fallbacks(shape, kernel):
    """fn2_correlation_f32_ws: with a sufficient workspace the fp32 features become split fp16 without loss (asserted: they
    carry 22 significant bits at most) and corr3 forms hi*hi + hi*lo + lo*hi exactly; with a NULL workspace, or one a byte
    too small, the call is fn2_correlation_f32, bit for bit."""
    from src import weights as W
    _hip, lib = _lib()
    assert op_kernel_name(shape, ATTRS_C, True) == kernel
    assert op_kernel_name(shape, ATTRS_C, False) == "corr2_kernel<float, float, %d>" % (shape[3] // 32)
    a, b = dyadic(shape, 31, True), dyadic(shape, 32, True)
    assert_exact_preconditions("f16x2", a, b, True)
    for x in (a, b):
        x32 = x.astype(np.float32)
        assert np.array_equal(x32, x) and np.array_equal(W.join_f16x2(W.split_f16x2(x32)), x32)
    (ah, al), (bh, bl) = split_parts(a), split_parts(b)
    S = corr_sums(ah, bh, 20, 2) + corr_sums(ah, bl, 20, 2) + corr_sums(al, bh, 20, 2)
    want = (S / shape[3]).astype(np.float32)
    assert np.array_equal(want, S / shape[3])
    need = int(lib.fn2_correlation_workspace_bytes(*shape, *ATTRS_C))
    assert need == 2 * 4 * int(np.prod(shape))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    np.testing.assert_array_equal(_run_op(shape, ATTRS_C, a, b, ws, need, True), want)
    plain = _run_op(shape, ATTRS_C, a, b)
    assert np.array_equal(_run_op(shape, ATTRS_C, a, b, None, need, True).view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(_run_op(shape, ATTRS_C, a, b, ws, need - 1, True).view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------------------------------- bounded tests
def _gauss(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _assert_bounded(dt, got, a, b, md, s2, k=1, s1=1, pad=None):
    """|got - ref| <= (C + 4) 2^-24 S / C per element, S = sum_c |a_c| |b_c| in float64 on the inputs as the input type
    holds them.  Derived, not measured: any fp32 summation order of exact products costs (C - 1) u S (u = 2^-24); the
    lo*lo term corr2 / corr3 drop on split fp16 is at most 2^-22 S = 4 u S, and the paths that do not drop it round each
    product of two fp32 operands instead (u S); the final division rounds once more (u S).  Returns max error / bound."""
    ar, br = round_to(dt, a), round_to(dt, b)
    n = k * k * a.shape[3]
    ref = corr_sums(ar, br, md, s2, k, s1, pad) / n
    S = corr_sums(np.abs(ar), np.abs(br), md, s2, k, s1, pad)
    bound = (n + 4) * 2.0 ** -24 * S / n
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err[S > 0] / bound[S > 0]).max())
    assert np.all(err <= bound), ratio
    assert np.all(got[S == 0] == 0)
    return ratio


BOUNDED_FUSED = ([fcase("corr3", dt, (8, 65), SMALLEST_C[dt]) for dt in IN16] +
                 [fcase("corr2", dt, (6, 65), SMALLEST_C[dt]) for dt in ALL] +
                 [fcase("corr_mfma", dt, (6, 65), SLAB_C[dt], out_view=(448, 0) if dt == "f16x2" else None) for dt in ALL])


@gpu
@pytest.mark.parametrize("case", BOUNDED_FUSED, ids=[c["id"] for c in BOUNDED_FUSED])
def test_fused_bounded_gaussian(case):
    """Gaussian data under the derived bound of _assert_bounded.  Largest observed error / bound on an MI355X:
    corr3 f16x2 0.047, bf16 0.018, f16 0.020; corr2 f32 0.118, f16x2 0.047, bf16 0.018, f16 0.019;
    corr_mfma f32 0.172, f16x2 0.181, bf16 0.040, f16 0.041.  The bound stays the assertion."""
    a, b = _gauss(case["shape"], 41), _gauss(case["shape"], 42)
    dt = case["dt"]
    got = run_fused(case, round_to(dt, a), round_to(dt, b))
    print("%s: max error / bound = %.4f" % (case["id"], _assert_bounded(dt, got, a, b, *case["attrs"])))


@gpu
def test_corr_mfma_split_fp16_with_lo_parts_bounded():
    """corr_mfma_kernel multiplies the joined fp32 values of split-fp16 features, so lo-carrying dyadic inputs are not
    exact there (the lo*lo products need more than 24 bits): the derived bound holds.  Observed error / bound: 0.033."""
    case = fcase("corr_mfma", "f16x2", (6, 65), 16, out_view=(448, 0), lo=True)
    a, b = dyadic(case["shape"], 43, True), dyadic(case["shape"], 44, True)
    assert (split_parts(a)[1] != 0).mean() >= 0.10
    print("corr_mfma f16x2 with lo parts: max error / bound = %.4f" % _assert_bounded("f16x2", run_fused(case, a, b), a, b, 20, 2))


@gpu
def test_generic_kernel_bounded_gaussian():
    """The thread-per-element forward kernel on Gaussian fp32 data, C = 96.  Observed error / bound: 0.021."""
    shape, args = (2, 6, 65, 96), ATTRS_C
    assert op_kernel_name(shape, args, False) == "correlation_generic_kernel"
    a, b = _gauss(shape, 45), _gauss(shape, 46)
    print("generic f32 C=96: max error / bound = %.4f" % _assert_bounded("f32", _run_op(shape, args, a, b), a, b, 20, 2))


# ------------------------------------------------------------------------------------------- LeakyReLU
def _ulp(dt, v):
    """One unit in the last place of the output type at |v| (0 for fp32: its roundings are in the bound already)."""
    if dt == "f32":
        return np.zeros_like(v)
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -60)))
    if dt == "bf16":
        return 2.0 ** (e - 7)
    if dt == "f16":
        return np.maximum(2.0 ** (e - 10), 2.0 ** -24)
    return np.maximum(2.0 ** (e - 21), 2.0 ** -24)  # hi carries 11 bits, lo the next 11; fp16's smallest step below


LEAKY = [fcase("corr3", "f16x2", (8, 65), 32, out="f16x2", out_view=(480, 32)),  # the engine's call
         fcase("corr3", "bf16", (8, 65), 64, out="bf16", out_view=(473, 32)),
         fcase("corr3", "f16", (8, 65), 64, out_view=(473, 32)),
         fcase("corr2", "f32", (6, 65), 32, out_view=(473, 32)),
         fcase("corr2", "f16x2", (6, 65), 32, out="f16x2", out_view=(480, 32)),
         fcase("corr2", "f16", (6, 65), 64, out="f16", out_view=(473, 32)),
         fcase("corr_mfma", "bf16", (6, 65), 32, out="bf16", out_view=(473, 32)),
         fcase("corr_mfma", "f32", (6, 65), 16, out_view=(473, 32)),
         fcase("corr_mfma", "f16x2", (6, 65), 16, out="f16x2", out_view=(480, 32))]


@gpu
@pytest.mark.parametrize("case", LEAKY, ids=[c["id"] for c in LEAKY])
def test_fused_leaky_relu(case):
    """act = FN2_ACT_LEAKY on top of the exact pre-activation value x: the device computes 0.55f*x + 0.45f*|x| (possibly
    contracted) -- three roundings, one spare: 4 * 2^-24 |x| around the float64 value of that expression with the float32
    constants, plus one unit in the last place of a 16-bit / split-fp16 output type."""
    md, s2 = case["attrs"]
    a, b, S = fused_reference(case["dt"], case["shape"], md, s2, case["lo"], 11)
    x = S / case["shape"][3]
    assert np.array_equal(x.astype(np.float32), x)
    want = float(np.float32(0.55)) * x + float(np.float32(0.45)) * np.abs(x)
    got = joined(case["out"], run_fused(case, a, b, ACT_LEAKY))
    assert (got < 0).any() and (got > 0).any()
    tol = 4 * 2.0 ** -24 * np.abs(x) + _ulp(case["out"], want)
    err = np.abs(got - want)
    assert np.all(err <= tol), float((err - tol).max())
    assert np.all(got[x == 0] == 0)
    assert np.array_equal(np.sign(got), np.sign(x))


# ------------------------------------------------------------------------------------------- backward
def _run_grad(shape, args, g, a, b):
    _hip, lib = _lib()
    N, H, W, Cn = shape
    tg, ta, tb = (torch.from_numpy(np.asarray(t, np.float32)).cuda() for t in (g, a, b))
    da = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    db = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    _hip.check(lib.fn2_correlation_grad_f32(_hip.ptr(tg), _hip.ptr(ta), _hip.ptr(tb), _hip.ptr(da), _hip.ptr(db),
                                            N, H, W, Cn, *args, _hip.stream_ptr()))
    torch.cuda.synchronize()
    return da.cpu().numpy(), db.cpu().numpy()


def small_ints(shape, seed):
    """Gradient tensor: integers in [-3, 3] under a keep-mask of one half."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, shape) * (rng.random(shape) < 0.5)).astype(np.float64)


@gpu
@pytest.mark.parametrize("shape,args,kernel", EXACT_GRAD)
def test_correlation_grad_exact(shape, args, kernel):
    """fn2_correlation_grad_f32 on dyadic data: float32(S) / float32(k*k*C) with S the exact float64 sum.  The tiled
    kernels against the formula in ops.hip's comment; the thread-per-element kernel against the window sums of
    oracle.ops.correlation_grad_loops (its quotients turned back into the exact sums, which are multiples of 1/2)."""
    from oracle import ops as ref
    k, md, s1, s2, pad = args
    assert grad_kernel_name(shape, args) == kernel
    a, b = dyadic(shape, 51), dyadic(shape, 52)
    g = small_ints(out_shape(shape, args), 53)
    D = g.shape[-1]
    # every sum has at most D * k * k window terms of |g| <= 3 times |value| <= 2, in units of 1/2: far below 2^24
    assert D * k * k * np.abs(g).max() * max(np.abs(a).max(), np.abs(b).max()) * 2 < 2.0 ** 24
    n = float(k * k * shape[3])
    if kernel == TILED:
        SA, SB = grad_sums(g, a, b, md, s2)
    else:
        qa, qb = ref.correlation_grad_loops(g, a, b, *args)
        SA, SB = np.rint(qa.astype(np.float64) * n * 2) / 2, np.rint(qb.astype(np.float64) * n * 2) / 2
        assert np.abs(qa * n - SA).max() < 2.0 ** -10 and np.abs(qb * n - SB).max() < 2.0 ** -10
    assert np.abs(SA).max() > 0 and np.abs(SB).max() > 0
    da, db = _run_grad(shape, args, g, a, b)
    np.testing.assert_array_equal(da, SA.astype(np.float32) / np.float32(n))
    np.testing.assert_array_equal(db, SB.astype(np.float32) / np.float32(n))


ADJOINT_OP = [
    ((1, 6, 20, 32), ATTRS_C, False, "corr2_kernel<float, float, 1>", TILED),
    ((1, 8, 20, 32), ATTRS_C, True, "corr3_kernel<fn2::x2_t, float, 1>", TILED),
    ((1, 6, 20, 16), ATTRS_C, False, "corr_mfma_kernel<float, float, 1>", TILED),
    ((1, 5, 6, 4), (1, 4, 1, 1, 4), False, "correlation_generic_kernel", "correlation_grad_kernel"),
]


def _assert_adjoint(out, g, a, da, b, db):
    lhs = float((out.astype(np.float64) * g).sum())
    assert lhs != 0
    assert float((a * da.astype(np.float64)).sum()) == lhs
    assert float((b * db.astype(np.float64)).sum()) == lhs


@gpu
@pytest.mark.parametrize("shape,args,ws,fwd,bwd", ADJOINT_OP)
def test_adjoint_identity_op_surface(shape, args, ws, fwd, bwd):
    """<corr(a, b), g> = <a, dA> = <b, dB>: with dyadic a, b, g and a power-of-two C every device value is exact, so the
    three float64 sums are equal, not close.  Needs no oracle."""
    _, lib = _lib()
    assert op_kernel_name(shape, args, ws) == fwd and grad_kernel_name(shape, args) == bwd
    a, b = dyadic(shape, 61), dyadic(shape, 62)
    g = small_ints(out_shape(shape, args), 63)
    if ws:
        need = int(lib.fn2_correlation_workspace_bytes(*shape, *args))
        out = _run_op(shape, args, a, b, torch.empty(need, dtype=torch.uint8, device="cuda"), need, True)
    else:
        out = _run_op(shape, args, a, b)
    da, db = _run_grad(shape, args, g, a, b)
    _assert_adjoint(out, g, a, da, b, db)


@gpu
def test_adjoint_identity_fused_split_fp16():
    """The same identity with the forward taken from fn2_correlation_fused on split fp16 (lo = 0)."""
    case = fcase("corr3", "f16x2", (8, 20), 32, N=1, lo=False)
    shape = case["shape"]
    assert grad_kernel_name(shape, ATTRS_C) == TILED
    a, b = dyadic(shape, 61), dyadic(shape, 62)
    g = small_ints(shape[:3] + (441,), 63)
    out = run_fused(case, a, b)
    da, db = _run_grad(shape, ATTRS_C, g, a, b)
    _assert_adjoint(out, g, a, da, b, db)
