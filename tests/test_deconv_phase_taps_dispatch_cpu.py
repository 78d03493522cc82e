"""Which instantiation a kind-5 transposed conv launches, asked without a device (fn2_conv2d_kernel_name is host-only, as in
test_conv_dispatch_cpu.py): the per-phase tap walk by default, the all-columns walk with FN2_CONV_DBG bit 128 and for
launches whose epilogue the 16-output form does not have (accumulate)."""
import pytest

from test_conv_dispatch_cpu import OK, X2, _desc, _query


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    monkeypatch.delenv("FN2_CONV_DBG", raising=False)


def _merged(cout, n=4, h=192, w=256, cin=192):
    d = _desc(X2, X2, n, h, w, cin, cout, k=4, stride=2, pad=1, kind=5)
    d.cout_pad = 2 * cout
    d.kpad = 6 * cin
    return d


def test_sixteen_outputs_take_two_16_row_tiles(monkeypatch):
    d = _merged(16)                                   # fuse_deconv0 at batch 4
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 1, 1, 3, 1>")
    monkeypatch.setenv("FN2_CONV_DBG", "128")         # A/B: every phase walks all three window columns
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 1, 1, 3>")


def test_thirty_two_outputs_take_both_phases_in_one_block(monkeypatch):
    d = _merged(32, h=96, w=128, cin=128)             # fuse_deconv1 at batch 4
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 2, 1, 3, 1>")
    monkeypatch.setenv("FN2_CONV_DBG", "128")         # one 32-row tile (= one column phase) per block
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 1, 1, 3>")


def test_accumulating_sixteen_output_launch_keeps_the_all_columns_walk():
    d = _merged(16)
    d.accumulate = 1
    assert _query(d) == (OK, "conv_halo_kernel<fn2::x2_t, 1, 4, 1, 1, 3>")
