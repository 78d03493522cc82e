"""fn2_conv2d kind 5 with the per-phase tap walk (conv_halo_kernel, PT): each column phase of
the merged transposed conv multiplies only the two window columns it has weights for -- 16 outputs as two 16-row tiles
on the 16x16x32 instruction, 32 outputs as two 32-row tiles in one block.  Against the oracle's conv2d_transpose with
bias and LeakyReLU (the fp32 accumulation-order bound of test_gpu_conv.py, 2e-5) and against the four-phase kind-1
launch of the same layer (1e-5), written into a channel slice of a wider buffer whose other channels must stay as they
were, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nn as refnn
from test_gpu_conv import _from_dev, _to_dev, rnd, run_conv

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
C0, CS = 64, 96          # the layer writes channels [64, 64 + Cout) of a 96-channel buffer
UP_C0 = 80               # the riding upsample's two channels

CASES = [
    # cin, cout, N, H, W, up
    (32, 16, 2, 2, 128, False),    # one channel block; both rows are border rows; two images (no read across the image seam)
    (96, 16, 1, 3, 128, False),    # three channel blocks: an odd count in the two-buffer loop
    (162, 16, 2, 3, 256, False),   # the real layer's padded tail channels; two tiles per row (window columns cross the tile edge)
    (128, 32, 1, 3, 128, False),   # 32 outputs: two 32-row tiles in one block
    (64, 32, 2, 2, 256, False),
    (32, 16, 2, 2, 128, True),     # fuse_upsample_flow1to0 riding on the launch (fn2_conv_desc.up_src)
]


@pytest.mark.parametrize("cin,cout,N,H,W,up", CASES)
def test_deconv_phase_taps(cin, cout, N, H, W, up):
    from src import _hip, weights as Wt
    lib = _hip.lib()
    x = rnd((N, H, W, cin), 190)
    w = rnd((4, 4, cout, cin), 191, (2.0 / (4 * cin)) ** 0.5)
    b = rnd((cout,), 192, 0.5)
    want = refnn.conv2d_transpose(x, w, activation=refnn.leaky_relu, bias=b)
    cs = (cin + 31) // 32 * 32
    xp = np.zeros((N, H, W, cs), np.float32)
    xp[..., :cin] = x
    xin = _to_dev(xp, "f16x2")
    plan = _hip.conv_plan(3, cs, cout)
    assert plan.layout == 1 and plan.cout_tile == 32
    packed, cin_pad, cout_pad, kpad = Wt.pack_deconv_merged(w, plan.cout_tile, plan.kstep_elems, cs, plan.layout)
    k2 = int(np.floor(np.log2(1024.0 / np.abs(packed).max())))
    wdev = Wt.packed_to_device(packed * 2.0 ** k2, plan.wgt_dtype, "cuda")
    bd = torch.from_numpy(b).cuda()
    out = _to_dev(np.full((N, 2 * H, 2 * W, CS), SENTINEL, np.float32), "f16x2")
    d = _hip.Fn2ConvDesc()
    d.inp, d.out = _hip.view(xin, cin, 0, 3), _hip.view(out, cout, C0, 3)
    d.wgt, d.bias = wdev.data_ptr(), bd.data_ptr()
    d.kind, d.kh, d.kw, d.stride, d.pad, d.act = 5, 4, 4, 2, 1, 1
    d.cin_pad, d.cout_pad, d.kpad, d.wgt_layout, d.out_scale = cin_pad, cout_pad, kpad, plan.layout, 2.0 ** -k2
    if up:
        flow = rnd((N, H, W, 2), 193, 3.0)
        uw = rnd((4, 4, 2, 2), 194, 0.5)
        ub = np.array([0.375, -1.25], np.float32)
        fd, uwd, ubd = torch.from_numpy(flow).cuda(), torch.from_numpy(uw).cuda(), torch.from_numpy(ub).cuda()
        d.up_src, d.up_w, d.up_bias, d.up_c0 = fd.data_ptr(), uwd.data_ptr(), ubd.data_ptr(), UP_C0
    name = C.create_string_buffer(256)
    _hip.check(lib.fn2_conv2d_kernel_name(C.byref(d), name, 256))
    assert name.value.decode() == "conv_halo_kernel<fn2::x2_t, 1, 4, %d, 1, 3, 1>" % (cout // 16), name.value
    _hip.check(lib.fn2_conv2d(C.byref(d), _hip.stream_ptr()))
    torch.cuda.synchronize()
    res = _from_dev(out, 3)
    got = res[..., C0:C0 + cout]
    base = run_conv(x, w, b, "deconv", 4, 2, 1, True, "f16x2")
    print("cin %d cout %d: max |got - oracle| %.3e, max |got - four-phase| %.3e (max |oracle| %.2f)"
          % (cin, cout, np.abs(got - want).max(), np.abs(got - base).max(), np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(got, base, rtol=1e-5, atol=1e-5)
    touched = np.zeros(CS, bool)
    touched[C0:C0 + cout] = True
    if up:
        touched[UP_C0:UP_C0 + 2] = True
        upw = refnn.conv2d_transpose(flow, uw, bias=ub)
        print("riding upsample: max |got - oracle| %.3e" % np.abs(res[..., UP_C0:UP_C0 + 2] - upw).max())
        np.testing.assert_allclose(res[..., UP_C0:UP_C0 + 2], upw, rtol=1e-5, atol=1e-5)
    assert np.array_equal(res[..., ~touched], np.full_like(res[..., ~touched], SENTINEL))
