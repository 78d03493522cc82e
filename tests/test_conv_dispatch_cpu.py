"""Which kernel fn2_conv2d and fn2_flow_head5 launch, asserted without a device: fn2_conv2d_kernel_name and
fn2_flow_head5_kernel_name are host-only (they walk the launch entries up to the launch site, write the instantiation and
call no HIP runtime function), so every query here returns 0 on dummy pointers.  A launch attempt would not: without a
device it fails with FN2_ERR_HIP -- a launch site that misses the name-sink check shows up as that code.

The expected names are the instantiations of the launch tables (conv.hip: launch_conv, fn2_conv2d's flow-head branch;
conv2.hip: launch2, launch_halo, launch_rowrun, launch_head5, launch_head5_strip) written out, in the form rocprofv3
prints them minus "void fn2::", the argument list and the defaulted trailing template arguments (bench.py matches them
as prefixes of the profiles/*_kernel_stats.csv rows, which carry all thirteen of conv_igemm2_kernel's)."""
import ctypes as C

import pytest

F32, BF16, F16, X2 = 0, 1, 2, 3
TYPE = {F32: "float", BF16: "__bf16", F16: "_Float16", X2: "fn2::x2_t"}
OK, INVALID, UNSUPPORTED, HIP = 0, -1, -2, -3
DUMMY = 0x1000  # non-null, never dereferenced


def _lib():
    from src import _hip
    return _hip, _hip.lib()


def _desc(dt_in, dt_out, n, h, w, cin, cout, k=3, stride=1, pad=1, kind=0, cin_pad=None, layout=None, in_cs=None, act=0):
    """A descriptor as the engine would fill it for this geometry: plan from fn2_conv2d_plan, dense views, dummy pointers."""
    _hip, lib = _lib()
    cin_pad = cin if cin_pad is None else cin_pad
    plan = _hip.conv_plan(dt_in, cin_pad, cout)
    d = _hip.Fn2ConvDesc()
    if kind == 0:
        oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        taps = k * k
    elif kind == 2:
        oh, ow = (h - k) // stride + 1, (w - k) // stride + 1
        taps = k          # a kernel row is one tap of cin_pad channels
    else:
        oh, ow, taps = 2 * h, 2 * w, 4
    d.inp = _hip.Fn2Tensor(DUMMY, dt_in, n, h, w, cin, cin_pad if in_cs is None else in_cs, 0)
    d.out = _hip.Fn2Tensor(DUMMY, dt_out, n, oh, ow, cout, (cout + 7) // 8 * 8, 0)
    d.wgt = DUMMY
    d.kind, d.kh, d.kw, d.stride, d.pad, d.act = kind, k, k, stride, pad, act
    d.cin_pad = cin_pad
    d.cout_pad = -(-cout // plan.cout_tile) * plan.cout_tile
    d.kpad = -(-taps * cin_pad // plan.kstep_elems) * plan.kstep_elems
    d.wgt_layout = plan.layout if layout is None else layout
    d.out_scale = 1.0
    return d


def _query(d):
    _, lib = _lib()
    buf = C.create_string_buffer(256)
    rc = lib.fn2_conv2d_kernel_name(C.byref(d), buf, 256)
    return rc, buf.value.decode()


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in ("FN2_CONV_DBG", "FN2_KG", "FN2_KG2_MAX", "FN2_KG3_MAX", "FN2_BP64_MIN", "FN2_RING_MAX", "FN2_M16_MIN",
              "FN2_DEEP_MIN", "FN2_DEEP_MAX", "FN2_RING_SPLIT", "FN2_WREG_RING", "FN2_WREG_FEED", "FN2_H5_STRIP",
              "FN2_H5_DBG", "FN2_SPLIT_MINBLOCKS"):
        monkeypatch.delenv(k, raising=False)


# ---- the generic kernel (wgt_layout 0: 24 channels per tap are no whole 128-byte lines) -------------------------------
@pytest.mark.parametrize("dt, cout, shape", [(F32, 128, "4, 2, 2"), (F32, 64, "4, 1, 4"), (F32, 32, "2, 1, 4"),
                                             (F32, 16, "1, 1, 4"), (BF16, 64, "4, 1, 4"), (F16, 16, "1, 1, 4")])
def test_generic_kernel_per_tile_and_type(dt, cout, shape):
    d = _desc(dt, dt, 1, 16, 16, 24, cout)
    assert d.wgt_layout == 0
    assert _query(d) == (OK, "conv_igemm_kernel<%s, %s, %s>" % (TYPE[dt], TYPE[dt], shape))


def test_generic_kernel_fp32_output_of_a_16_bit_layer():
    assert _query(_desc(BF16, F32, 1, 16, 16, 24, 64)) == (OK, "conv_igemm_kernel<__bf16, float, 4, 1, 4>")


# ---- the dot-product flow head: 3x3, stride 1, pad 1, two fp32 outputs ------------------------------------------------
@pytest.mark.parametrize("dt", [F32, BF16, F16, X2])
@pytest.mark.parametrize("hw", [(16, 16), (96, 128)])   # (split fp16: block per pixel up to 4096 pixels -- the same kernel)
def test_flow_head_kernel(dt, hw):
    d = _desc(dt, F32, 1, hw[0], hw[1], 64, 2)
    assert d.wgt_layout == 0
    assert _query(d) == (OK, "flow_head_kernel<%s>" % TYPE[dt])


def test_two_outputs_that_are_no_flow_head_run_the_generic_kernel():
    # (a LeakyReLU on the two outputs: not the head path; cout == 2 plans the 16-row tile of the generic kernel)
    assert _query(_desc(F32, F32, 1, 16, 16, 24, 2, act=1)) == (OK, "conv_igemm_kernel<float, float, 1, 1, 4>")


# ---- the LDS-DMA kernels --------------------------------------------------------------------------------------------
def test_plain_igemm2_64_cout_tile():
    # fp32, 64 -> 64 channels, 1x1: 64 x 128 tiles, two stages, one K group
    assert _query(_desc(F32, F32, 1, 16, 16, 64, 64, k=1, pad=0)) == (OK, "conv_igemm2_kernel<float, float, 1, 4, 2, 1, 2, 1, false>")


def test_fp32_128_cout_on_a_small_map_takes_two_k_groups():
    # fp32, cin_pad 64 -> 128 outputs on a 16x16 map: 4 blocks of 128 x 64, under the 96 of FN2_KG2_MAX
    assert _query(_desc(F32, F32, 1, 16, 16, 64, 128)) == (OK, "conv_igemm2_kernel<float, float, 2, 2, 2, 1, 2, 2, false>")


def test_k_groups_on_the_6x8_level_and_their_switch(monkeypatch):
    d = _desc(X2, X2, 1, 6, 8, 1024, 512)    # conv6-like: 1 x 4 blocks of 128 x 64
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 2, 2, 2, 1, 2, 2, false>")
    monkeypatch.setenv("FN2_KG", "0")        # no groups: under FN2_BP64_MIN's 96 blocks the full 128 x 128 tile
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 2, 2, 2, 2, 2, 1, false>")


def test_three_slot_ring_on_a_one_round_grid():
    # conv3_1 at batch 4: 12288 pixels / 64 x 2 cout tiles = 384 blocks (384 .. FN2_RING_MAX = 512), no split-K
    d = _desc(X2, X2, 4, 48, 64, 256, 256)
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 2, 2, 2, 1, 3, 1, false>")


def test_halo_kernel_and_fragment_order_weights():
    # the same layer at batch 8: 768 blocks -- stride 1, tiles inside image rows: the halo kernel; with its weights in
    # fragment order (wgt_layout 2) the register-operand instantiation, two stages, no slab
    d = _desc(X2, X2, 8, 48, 64, 256, 256)
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 2, 2, 2, 1, 3>")
    d.wgt_layout = 2
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 4, 1, 1, 2, 2, 1, false, true, false>")


def test_fragment_order_ring_with_feeder_waves():
    d = _desc(X2, X2, 4, 48, 64, 256, 256, layout=2)    # 384 blocks: the ring form; FN2_WREG_FEED 1: eight waves
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 4, 1, 1, 2, 3, 1, false, true, false, false, true>")


def test_rowrun_stem():
    # FlowNetS conv1 on the packed pair: 7x7 stride 2 over [n, 128 + 6, 256 + 6, 8], run = 7 * 8 -> 64 channels
    d = _desc(X2, X2, 1, 134, 262, 8, 64, k=7, stride=2, pad=0, kind=2, cin_pad=64, in_cs=8)
    assert _query(d) == (OK, "conv_rowrun_kernel<fn2::x2_t, 2>")


def test_transposed_conv_kind_1():
    # deconv5 at batch 1: 48 pixels x 4 phases x 4 cout tiles = 16 blocks: two K groups
    d = _desc(X2, X2, 1, 6, 8, 1024, 512, k=4, stride=2, pad=1, kind=1)
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 2, 2, 2, 1, 2, 2, false>")
    # fuse_deconv1 at batch 4: 128 -> 32 channels on 96 x 128 phase maps, 1536 blocks of 32 x 128 inside image rows --
    # the 2x2-tap halo form
    d = _desc(X2, X2, 4, 96, 128, 128, 32, k=4, stride=2, pad=1, kind=1)
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 1, 1, 2>")


def test_riding_head_and_workspace_do_not_launch():
    """A descriptor that carries a workspace, a riding upsample_flow and a riding head is still answered host-only, with
    the name of the convolution's own launch."""
    _hip, _ = _lib()
    d = _desc(X2, X2, 1, 6, 8, 1024, 512, k=4, stride=2, pad=1, kind=1)
    d.out.cs = 776   # room for the two flow channels behind the 512 outputs
    h = _desc(X2, F32, 1, 6, 8, 1024, 2)
    d.head = C.addressof(h)
    d.up_src, d.up_w, d.up_c0 = DUMMY, DUMMY, 768
    d.workspace, d.workspace_bytes = DUMMY, 1 << 30
    assert _query(d) == (OK, "conv_igemm2_kernel<fn2::x2_t, fn2::x2_t, 2, 2, 2, 1, 2, 2, false>")


# ---- refusals: the query returns what fn2_conv2d returns, and no name ---------------------------------------------------
def _bad_kind(d): d.kind = 7
def _bad_layout(d): d.wgt_layout = 1 - d.wgt_layout
def _bad_kpad(d): d.kpad = 8
def _bad_batch(d): d.out.n = 2
def _bad_out(d): d.out.h += 1
def _null_weight(d): d.wgt = None
def _frag_f32(d): d.wgt_layout = 2


@pytest.mark.parametrize("spoil", [_bad_kind, _bad_layout, _bad_kpad, _bad_batch, _bad_out, _null_weight, _frag_f32])
def test_refused_descriptor_same_code_no_name(spoil):
    _, lib = _lib()
    d = _desc(F32, F32, 1, 16, 16, 64, 128)
    assert _query(d)[0] == OK
    spoil(d)
    rc, name = _query(d)
    assert rc in (INVALID, UNSUPPORTED) and name == ""
    assert lib.fn2_conv2d(C.byref(d), None) == rc   # (refused in front of any launch: safe without a device)
    buf = C.create_string_buffer(8)
    assert lib.fn2_conv2d_kernel_name(None, buf, 8) == INVALID and lib.fn2_conv2d_kernel_name(C.byref(d), None, 0) == INVALID


# ---- fn2_flow_head5 ------------------------------------------------------------------------------------------------
HEAD5_TILE = "conv_igemm2_kernel<fn2::x2_t, float, 1, 4, 2, 2, 2, 1, false, false, false, true>"


def _head5(cin_pad, c=None, dt=X2, c0=0, kpad=None, cs=None, ring_w=DUMMY):
    _hip, lib = _lib()
    x = _hip.Fn2Tensor(DUMMY, dt, 1, 256, 256, cin_pad - 14 if c is None else c, cin_pad if cs is None else cs, c0)
    args = (C.byref(x), DUMMY, cin_pad, cin_pad if kpad is None else kpad, C.c_float(1.0), DUMMY, DUMMY, 1, ring_w, DUMMY)
    buf = C.create_string_buffer(256)
    rc = lib.fn2_flow_head5_kernel_name(*args, buf, 256)
    return rc, buf.value.decode(), args


def test_head5_strip_and_tile_forms(monkeypatch):
    assert _head5(96)[:2] == (OK, "head5_strip_kernel<1>")     # the fusion net's concat0: 82 channels, three lines
    assert _head5(192)[:2] == (OK, "head5_strip_kernel<2>")    # concat1: 162 channels, six lines
    assert _head5(64)[:2] == (OK, HEAD5_TILE)
    assert _head5(96, ring_w=None)[:2] == (OK, "head5_strip_kernel<1>")
    monkeypatch.setenv("FN2_H5_STRIP", "0")
    assert _head5(96)[:2] == (OK, HEAD5_TILE)
    assert _head5(192)[:2] == (OK, HEAD5_TILE)


@pytest.mark.parametrize("bad", [dict(dt=F32), dict(dt=BF16), dict(c0=4, cs=104), dict(cs=100), dict(kpad=128),
                                 dict(cin_pad=80), dict(c=100)])
def test_head5_refusals_equal_the_launch_entry(bad):
    _, lib = _lib()
    rc, name, args = _head5(bad.pop("cin_pad", 96), **bad)
    assert rc == INVALID and name == ""
    assert lib.fn2_flow_head5(*args, None) == rc    # (refused in front of the launch)
