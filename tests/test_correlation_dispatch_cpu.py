"""Which device kernel a cost-volume call takes, and what fn2_correlation_fused refuses, without a GPU: the host-only
queries fn2_correlation_fused_kernel_name / fn2_correlation_f32_kernel_name / fn2_correlation_grad_f32_kernel_name run
the same checks and the same selection code as the launches and launch nothing."""
import ctypes as C
import itertools

import pytest

import test_gpu_correlation as G

DTYPES = ("f32", "bf16", "f16", "f16x2")
OK, INVALID, UNSUPPORTED = 0, -1, -2
DUMMY = 0x1000  # non-null, never dereferenced: the queries and the argument checks touch no device memory


def _lib():
    from src import _hip
    return _hip, _hip.lib()


def _tensor(dt, n, h, w, c, cs=None, c0=0, data=DUMMY):
    _hip, _ = _lib()
    return _hip.Fn2Tensor(data, G.CODE[dt], n, h, w, c, c if cs is None else cs, c0)


def _fused_query(a, b, out, md, s2):
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.fn2_correlation_fused_kernel_name(C.byref(a), C.byref(b), C.byref(out), md, s2, buf, 128)
    return rc, buf.value.decode()


def _op_query(shape, args, ws):
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    rc = lib.fn2_correlation_f32_kernel_name(*shape, *args, int(ws), buf, 128)
    return rc, buf.value.decode()


# ---- the documented rule, stated once (include/flownet2_hip.h, DESIGN.md "Cost-volume dispatch") ----------------------
# bytes of one pixel's channels -> what the matrix-core kernels make of them
#   128, 256, 512, 1024   NL = 1, 2, 4, 8 lines of 128 bytes: corr2_kernel, or corr3_kernel under the conditions below
#   64                    one slab: corr_mfma_kernel<.., 1>
#   anything else         no matrix-core kernel: FN2_ERR_UNSUPPORTED on the fused entry, correlation_generic_kernel on the op
#                         surface
LINES_OF_BYTES = {128: 1, 256: 2, 512: 4, 1024: 8}
WIDEST_MD = 24  # the B window of a 64-pixel block, 64 + 2 * md pixels, has 112 LDS rows


def expected_fused(dt, c, h, md, s2, out, cs, c0, corr3_enabled):
    """(status, kernel) of fn2_correlation_fused for dense a / b views."""
    row = c * (2 if dt in ("bf16", "f16") else 4)
    if md > WIDEST_MD:
        return UNSUPPORTED, ""
    if row in LINES_OF_BYTES:
        corr3 = (corr3_enabled and dt != "f32" and (md, s2) == (20, 2) and h % 4 == 0 and
                 (out != "f16x2" or (cs % 8 == 0 and c0 % 8 == 0)))
        return OK, G.kname("corr3" if corr3 else "corr2", dt, out, LINES_OF_BYTES[row])
    if row == 64:
        if dt == "f16x2" and cs % 8 != 0:  # corr_mfma wants every split-fp16 view group aligned, the output stride included
            return INVALID, ""
        return OK, G.kname("corr_mfma", dt, out, 1)
    return UNSUPPORTED, ""


def expected_op(c, h, args, ws, corr3_enabled):
    """Kernel of fn2_correlation_f32 (ws False) / fn2_correlation_f32_ws with a sufficient workspace (ws True)."""
    k, md, s1, s2, pad = args
    if k != 1 or s1 != 1 or pad != md or md > WIDEST_MD:
        return "correlation_generic_kernel"
    if ws and corr3_enabled and (md, s2) == (20, 2) and h % 4 == 0 and 4 * c in LINES_OF_BYTES:
        return G.kname("corr3", "f16x2", "f32", LINES_OF_BYTES[4 * c])  # on split-fp16 copies in the workspace
    st, name = expected_fused("f32", c, h, md, s2, "f32", 0, 0, False)
    return name if st == OK else "correlation_generic_kernel"


CHANNELS = (16, 32, 48, 64, 96, 128, 256, 512)
HEIGHTS = (6, 8)
ATTRS = ((20, 2), (20, 1), (21, 2), (5, 3), (24, 2), (25, 2), (4, 1))
OUT_VIEWS = ((441, 0), (448, 0), (473, 32), (456, 8), (450, 9))  # (cs, c0) around the 441 channels of (20, 2)


def _out_view(md, s2, cs, c0):
    """The grid's (cs, c0) for a cost volume of D channels: strides grow by D - 441 where D > 441 (a multiple of 8 for
    every attribute set here, so the alignment classes stay), and the smaller volumes fit as they are."""
    d = (2 * (md // s2) + 1) ** 2
    grow = max(0, d - 441)
    assert grow % 8 == 0
    return d, cs + grow, c0


@pytest.mark.parametrize("corr3_env", [None, "0", "1"])
@pytest.mark.parametrize("dt", DTYPES)
def test_fused_dispatch_table(dt, corr3_env, monkeypatch):
    if corr3_env is None:
        monkeypatch.delenv("FN2_CORR3", raising=False)
    else:
        monkeypatch.setenv("FN2_CORR3", corr3_env)
    seen = {}
    for c, h, (md, s2), same, (cs, c0) in itertools.product(CHANNELS, HEIGHTS, ATTRS, (True, False), OUT_VIEWS):
        out = dt if same else "f32"
        d, cs, c0 = _out_view(md, s2, cs, c0)
        a, b, o = _tensor(dt, 2, h, 70, c), _tensor(dt, 2, h, 70, c), _tensor(out, 2, h, 70, d, cs, c0)
        want = expected_fused(dt, c, h, md, s2, out, cs, c0, corr3_env != "0")
        got = _fused_query(a, b, o, md, s2)
        assert got == want, (dt, c, h, md, s2, out, cs, c0, got, want)
        seen[want[1].split("<")[0] or want[0]] = seen.get(want[1].split("<")[0] or want[0], 0) + 1
    # the rows the table must show
    assert ("corr3_kernel" in seen) == (dt != "f32" and corr3_env != "0")
    assert {"corr2_kernel", "corr_mfma_kernel", UNSUPPORTED} <= set(seen)
    assert (INVALID in seen) == (dt == "f16x2")


def test_fused_dispatch_named_rows(monkeypatch):
    monkeypatch.delenv("FN2_CORR3", raising=False)

    def q(dt, c, h=8, attrs=(20, 2), out=None, view=(441, 0)):
        d, cs, c0 = _out_view(*attrs, *view)
        return _fused_query(_tensor(dt, 2, h, 70, c), _tensor(dt, 2, h, 70, c), _tensor(out or dt, 2, h, 70, d, cs, c0), *attrs)

    # corr3: 16-bit or split fp16, (20, 2), H % 4 == 0, 1 / 2 / 4 / 8 lines
    assert q("f16x2", 256, view=(456, 8)) == (OK, "corr3_kernel<fn2::x2_t, fn2::x2_t, 8>")
    assert q("bf16", 64) == (OK, "corr3_kernel<__bf16, __bf16, 1>")
    assert q("f16", 512, out="f32", view=(473, 32)) == (OK, "corr3_kernel<_Float16, float, 8>")
    assert q("f16x2", 64, out="f32", view=(450, 9)) == (OK, "corr3_kernel<fn2::x2_t, float, 2>")
    # .. with split-fp16 out only when cs and c0 are multiples of 8, else corr2's element-wise stores
    for view in ((441, 0), (473, 32), (450, 9)):
        assert q("f16x2", 256, view=view) == (OK, "corr2_kernel<fn2::x2_t, fn2::x2_t, 8>")
    # .. not for fp32 features, another height class or other attributes
    assert q("f32", 256) == (OK, "corr2_kernel<float, float, 8>")
    assert q("f16", 64, h=6) == (OK, "corr2_kernel<_Float16, _Float16, 1>")
    assert q("bf16", 128, attrs=(21, 2)) == (OK, "corr2_kernel<__bf16, __bf16, 2>")
    assert q("f16x2", 32, attrs=(24, 2), view=(448, 0)) == (OK, "corr2_kernel<fn2::x2_t, fn2::x2_t, 1>")
    # corr_mfma_kernel<.., 1>: one 64-byte slab
    assert q("bf16", 32) == (OK, "corr_mfma_kernel<__bf16, __bf16, 1>")
    assert q("f16", 32, out="f32") == (OK, "corr_mfma_kernel<_Float16, float, 1>")
    assert q("f16x2", 16, view=(448, 0)) == (OK, "corr_mfma_kernel<fn2::x2_t, fn2::x2_t, 1>")
    assert q("f32", 16) == (OK, "corr_mfma_kernel<float, float, 1>")
    # FN2_ERR_UNSUPPORTED
    assert q("bf16", 96)[0] == UNSUPPORTED and q("f16", 96)[0] == UNSUPPORTED
    assert q("f16x2", 48, view=(448, 0))[0] == UNSUPPORTED
    for dt in DTYPES:
        assert q(dt, 64, attrs=(25, 2), view=(448, 0))[0] == UNSUPPORTED
    # the same inputs on the op surface: the generic kernel
    assert _op_query((2, 8, 70, 96), (1, 20, 1, 2, 20), False) == (OK, "correlation_generic_kernel")
    assert _op_query((2, 8, 70, 48), (1, 20, 1, 2, 20), True) == (OK, "correlation_generic_kernel")
    assert _op_query((2, 8, 70, 64), (1, 25, 1, 2, 25), True) == (OK, "correlation_generic_kernel")
    # FN2_CORR3=0 turns every corr3 row into corr2
    monkeypatch.setenv("FN2_CORR3", "0")
    assert q("f16x2", 256, view=(456, 8)) == (OK, "corr2_kernel<fn2::x2_t, fn2::x2_t, 8>")
    assert q("bf16", 64) == (OK, "corr2_kernel<__bf16, __bf16, 1>")
    assert _op_query((2, 8, 70, 256), (1, 20, 1, 2, 20), True) == (OK, "corr2_kernel<float, float, 8>")


@pytest.mark.parametrize("corr3_env", [None, "0"])
def test_op_surface_dispatch_table(corr3_env, monkeypatch):
    if corr3_env is None:
        monkeypatch.delenv("FN2_CORR3", raising=False)
    else:
        monkeypatch.setenv("FN2_CORR3", corr3_env)
    _, lib = _lib()
    attr_sets = [(1, md, 1, s2, md) for md, s2 in ATTRS] + [(3, 2, 2, 1, 3), (1, 3, 1, 3, 3), (1, 20, 2, 2, 20), (1, 4, 1, 1, 6)]
    seen = set()
    for c, h, args, ws in itertools.product(CHANNELS + (5,), HEIGHTS + (12,), attr_sets, (False, True)):
        shape = (2, h, 70, c)
        want = expected_op(c, h, args, ws, corr3_env != "0")
        assert _op_query(shape, args, ws) == (OK, want), (shape, args, ws)
        # a workspace is asked for exactly where it changes the kernel
        need = lib.fn2_correlation_workspace_bytes(*shape, *args)
        assert (need > 0) == want.startswith("corr3_kernel") or not ws
        if ws and want.startswith("corr3_kernel"):
            assert need == 2 * 4 * 2 * h * 70 * c
        seen.add(want.split("<")[0])
    assert seen == ({"corr2_kernel", "corr_mfma_kernel", "correlation_generic_kernel"} |
                    ({"corr3_kernel"} if corr3_env is None else set()))


@pytest.mark.parametrize("corr3_env", [None, "0"])
@pytest.mark.parametrize("h", [47, 48])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_engine_reports_the_kernel_the_library_picks(dtype_name, h, corr3_env, monkeypatch):
    """The engine names its correlation launch by this query on the launch's own arguments (Engine.kernel_name); for
    the engine's call shape -- C = 256 features, the 441 channels behind conv_redir's 32 in the concat buffer, same-type
    output -- the library's answer is the documented rule's."""
    if corr3_env is None:
        monkeypatch.delenv("FN2_CORR3", raising=False)
    else:
        monkeypatch.setenv("FN2_CORR3", corr3_env)
    cs = 512 if dtype_name in ("bf16", "f16") else 480  # Engine._buf: the 473 channels rounded up to whole 128-byte lines
    a, b = _tensor(dtype_name, 4, h, 64, 256), _tensor(dtype_name, 4, h, 64, 256)
    out = _tensor(dtype_name, 4, h, 64, 441, cs, 32)
    want = expected_fused(dtype_name, 256, h, 20, 2, dtype_name, cs, 32, corr3_env is None)
    assert want[0] == OK and want[1].startswith("corr3_kernel" if (corr3_env is None and dtype_name != "f32" and h == 48)
                                                else "corr2_kernel")
    assert _fused_query(a, b, out, 20, 2) == want
    import types
    from src.engine import Engine
    _hip, lib = _lib()
    launch_args = (C.byref(a), C.byref(b), C.byref(out), 20, 2, _hip.ACT_LEAKY)   # Engine._net_c's op, without the stream
    assert Engine.kernel_name(types.SimpleNamespace(lib=lib), lib.fn2_correlation_fused, launch_args) == want[1]


# ---- validation of fn2_correlation_fused (dummy pointers: nothing launches) ------------------------------------------
def _fused_call(a, b, out, md=20, s2=2):
    """fn2_correlation_fused on arguments it must refuse.  The query goes first: a call it accepts is never made (the
    pointers are dummies), and where it refuses, the launch entry returns the same code."""
    _, lib = _lib()
    byref = lambda t: None if t is None else C.byref(t)
    buf = C.create_string_buffer(128)
    rcq = lib.fn2_correlation_fused_kernel_name(byref(a), byref(b), byref(out), md, s2, buf, 128)
    assert rcq != OK and buf.value == b""
    rc = lib.fn2_correlation_fused(byref(a), byref(b), byref(out), md, s2, 0, None)
    assert rc == rcq
    return rc, lib.fn2_last_error().decode()


def _good(dt="f16x2", out=None, c=64):
    return _tensor(dt, 2, 8, 70, c), _tensor(dt, 2, 8, 70, c), _tensor(out or dt, 2, 8, 70, 441, 448, 0)


def test_fused_validation():
    _, lib = _lib()
    a, b, o = _good()
    assert _fused_query(a, b, o, 20, 2)[0] == OK  # the starting point of every case below is a valid call
    # null tensor / null data
    for args in ((None, b, o), (a, None, o), (a, b, None)):
        rc, msg = _fused_call(*args)
        assert rc == INVALID and "null tensor" in msg
    rc, msg = _fused_call(_tensor("f16x2", 2, 8, 70, 64, data=None), b, o)
    assert rc == INVALID and "null tensor" in msg
    assert lib.fn2_correlation_fused_kernel_name(C.byref(a), C.byref(b), C.byref(o), 20, 2, None, 0) == INVALID
    # a / b dtype mismatch
    rc, msg = _fused_call(_tensor("f32", 2, 8, 70, 64), b, o)
    assert rc == INVALID and "dtype mismatch" in msg
    # a / b shape mismatch, each dimension
    for shp in ((1, 8, 70, 64), (2, 4, 70, 64), (2, 8, 69, 64), (2, 8, 70, 32)):
        rc, msg = _fused_call(a, _tensor("f16x2", *shp), o)
        assert rc == INVALID and "same shape" in msg
    # output spatial mismatch
    for n, h, w in ((1, 8, 70), (2, 4, 70), (2, 8, 71)):
        rc, msg = _fused_call(a, b, _tensor("f16x2", n, h, w, 441, 448, 0))
        assert rc == INVALID and "output spatial mismatch" in msg
    # out.c != gw * gw
    rc, msg = _fused_call(a, b, _tensor("f16x2", 2, 8, 70, 440, 448, 0))
    assert rc == INVALID and "441 channels" in msg
    rc, msg = _fused_call(a, b, o, 20, 1)
    assert rc == INVALID and "1681 channels" in msg
    # a slice that leaves its buffer, on each of a, b and out
    for args in ((_tensor("f16x2", 2, 8, 70, 64, 64, 8), b, o), (a, _tensor("f16x2", 2, 8, 70, 64, 72, 16), o),
                 (a, b, _tensor("f16x2", 2, 8, 70, 441, 448, 8)), (a, b, _tensor("f16x2", 2, 8, 70, 441, 440, 0))):
        rc, msg = _fused_call(*args)
        assert rc == INVALID and "outside the buffer" in msg
    # a feature view whose cs or c0 is not 16-byte aligned
    for dt, cs, c0 in (("f16x2", 70, 0), ("f16x2", 72, 2), ("bf16", 68, 0), ("bf16", 72, 4), ("f32", 66, 0), ("f16", 80, 12)):
        rc, msg = _fused_call(_tensor(dt, 2, 8, 70, 64, cs, c0), _tensor(dt, 2, 8, 70, 64), _tensor(dt, 2, 8, 70, 441, 448, 0))
        assert rc == INVALID and "16-byte aligned" in msg, (dt, cs, c0)
        rc, msg = _fused_call(_tensor(dt, 2, 8, 70, 64), _tensor(dt, 2, 8, 70, 64, cs, c0), _tensor(dt, 2, 8, 70, 441, 448, 0))
        assert rc == INVALID and "16-byte aligned" in msg, (dt, cs, c0)
    # bf16 in with f16 out (and the other mixed pairs)
    for dt, out in (("bf16", "f16"), ("f16", "bf16"), ("f32", "f16x2"), ("f16x2", "f16"), ("f32", "bf16")):
        rc, msg = _fused_call(*_good(dt, out))
        assert rc == INVALID and "bad output dtype" in msg
    # split-fp16 views that are not group (8) aligned on the corr_mfma path (C = 16: one slab); 16-byte alignment alone
    # (multiples of 4 channels) passes the earlier check
    m = lambda cs=16, c0=0: _tensor("f16x2", 2, 8, 70, 16, cs, c0)
    mo = lambda cs=448: _tensor("f16x2", 2, 8, 70, 441, cs, 0)
    assert _fused_query(m(), m(), mo(), 20, 2) == (OK, "corr_mfma_kernel<fn2::x2_t, fn2::x2_t, 1>")
    for args in ((m(20, 0), m(), mo()), (m(24, 4), m(), mo()), (m(), m(28, 0), mo()), (m(), m(24, 4), mo()), (m(), m(), mo(444))):
        rc, msg = _fused_call(*args)
        assert rc == INVALID and "group (8) aligned" in msg
    # FN2_ERR_UNSUPPORTED carries its own text
    rc, msg = _fused_call(*_good("bf16", c=96))
    assert rc == UNSUPPORTED and "not covered" in msg


def test_op_surface_and_grad_queries_return_the_launch_errors():
    _, lib = _lib()
    buf = C.create_string_buffer(128)
    assert lib.fn2_correlation_f32_kernel_name(2, 8, 8, 4, 2, 2, 1, 1, 2, 0, buf, 128) == INVALID   # even kernel size
    assert b"kernel_size must be odd" in lib.fn2_last_error()
    assert lib.fn2_correlation_f32_kernel_name(1, 4, 4, 4, 1, 8, 1, 1, 0, 0, buf, 128) == INVALID   # window does not fit
    assert lib.fn2_correlation_f32_kernel_name(0, 4, 4, 4, 1, 2, 1, 1, 2, 0, buf, 128) == INVALID
    assert lib.fn2_correlation_f32_kernel_name(1, 4, 4, 4, 1, 2, 1, 1, 2, 0, None, 0) == INVALID
    assert lib.fn2_correlation_grad_f32_kernel_name(1, 4, 4, 0, 1, 2, 1, 1, 2, buf, 128) == INVALID
    assert lib.fn2_correlation_grad_f32_kernel_name(1, 4, 4, 4, 2, 2, 1, 1, 2, buf, 128) == INVALID
    assert lib.fn2_correlation_grad_f32_kernel_name(1, 4, 4, 4, 1, 20, 1, 2, 20, buf, 128) == OK
    assert buf.value == b"correlation_grad_tiled_kernel<true, 16, 10, 2>"
    for args in ((1, 20, 1, 1, 20), (1, 18, 1, 2, 18), (3, 20, 1, 2, 21), (1, 20, 2, 2, 20)):
        assert lib.fn2_correlation_grad_f32_kernel_name(1, 8, 8, 4, *args, buf, 128) == OK, args
        assert buf.value == b"correlation_grad_kernel", args


# ---- what the exact GPU tests cover, by kernel name --------------------------------------------------------------------
def test_exact_gpu_cases_take_the_kernels_they_name_and_cover_every_family(monkeypatch):
    """Every case of tests/test_gpu_correlation.py's exact tables resolves here, without a device, to the kernel it names;
    together they run corr3_kernel, corr2_kernel and corr_mfma_kernel<.., 1> on every input type each accepts, with every
    NL, the generic forward kernel and both gradient kernels."""
    ids = [c["id"] for c in G.EXACT_FUSED]
    assert len(set(ids)) == len(ids)
    covered = set()
    for case in G.EXACT_FUSED:
        if case["corr3"] == "1":
            monkeypatch.delenv("FN2_CORR3", raising=False)
        else:
            monkeypatch.setenv("FN2_CORR3", case["corr3"])
        n, h, w, c = case["shape"]
        md, s2 = case["attrs"]
        d = (2 * (md // s2) + 1) ** 2
        (ae, a0), (be, b0) = case["a_view"] or (0, 0), case["b_view"] or (0, 0)
        cs, c0 = case["out_view"] or (d, 0)
        got = _fused_query(_tensor(case["dt"], n, h, w, c, c + ae, a0), _tensor(case["dt"], n, h, w, c, c + be, b0),
                           _tensor(case["out"], n, h, w, d, cs, c0), md, s2)
        assert got == (OK, case["kernel"]), case["id"]
        assert case["kernel"].startswith(case["family"] + "_kernel<" + G.TNAME[case["dt"]] + ", ")
        covered.add((case["family"], case["dt"], int(case["kernel"].rstrip(">").split(", ")[-1])))
    monkeypatch.delenv("FN2_CORR3", raising=False)
    for dt in ("f16x2", "bf16", "f16"):
        assert {("corr3", dt, nl) for nl in (1, 2, 4, 8)} <= covered
    for dt in DTYPES:
        assert ("corr2", dt, 1) in covered and ("corr_mfma", dt, 1) in covered
    assert not any(f == "corr3" and dt == "f32" for f, dt, _ in covered)
    # output types: same and fp32 for every family and input type
    for fam, dt in [("corr3", d) for d in ("f16x2", "bf16", "f16")] + [(f, d) for f in ("corr2", "corr_mfma") for d in DTYPES]:
        outs = {c["out"] for c in G.EXACT_FUSED if c["family"] == fam and c["dt"] == dt}
        assert outs == {dt, "f32"}, (fam, dt, outs)
    op = set()
    for shape, args, kernel in G.EXACT_OP:
        assert _op_query(shape, args, False) == (OK, kernel)
        op.add(kernel)
    for shape, kernel in G.EXACT_WS:
        assert _op_query(shape, G.ATTRS_C, True) == (OK, kernel)
        op.add(kernel.split("<")[0])
    assert {"correlation_generic_kernel", "corr2_kernel<float, float, 1>", "corr_mfma_kernel<float, float, 1>",
            "corr3_kernel"} <= op
    grads = set()
    for shape, args, kernel in G.EXACT_GRAD:
        buf = C.create_string_buffer(128)
        assert _lib()[1].fn2_correlation_grad_f32_kernel_name(*shape, *args, buf, 128) == OK
        assert buf.value.decode() == kernel
        grads.add(kernel)
    assert grads == {G.TILED, "correlation_grad_kernel"}


def test_corr_mfma_wider_instantiations_need_a_2_gib_b_buffer():
    """corr_mfma_kernel's NS = 2, 4, 8, 16 are exactly the channel rows corr2 takes first (NL = 1, 2, 4, 8): they are
    reached only where corr2 declines for its 31-bit DMA range, a B buffer of 2 GiB or more."""
    for dt, esz in (("f32", 4), ("f16x2", 4), ("bf16", 2), ("f16", 2)):
        for ns in (2, 4, 8, 16):
            c = ns * 64 // esz
            small = _fused_query(_tensor(dt, 1, 6, 70, c), _tensor(dt, 1, 6, 70, c), _tensor("f32", 1, 6, 70, 441, 448, 0), 20, 2)
            assert small == (OK, G.kname("corr2", dt, "f32", ns // 2))
            w = -(-(1 << 31) // (6 * c * esz))  # the narrowest 6-row image whose B buffer reaches 2 GiB
            big = _fused_query(_tensor(dt, 1, 6, w, c), _tensor(dt, 1, 6, w, c), _tensor("f32", 1, 6, w, 441, 448, 0), 20, 2)
            assert big == (OK, G.kname("corr_mfma", dt, "f32", ns)), (dt, ns, big)
            less = _fused_query(_tensor(dt, 1, 6, w - 1, c), _tensor(dt, 1, 6, w - 1, c), _tensor("f32", 1, 6, w - 1, 441, 448, 0), 20, 2)
            assert less == (OK, G.kname("corr2", dt, "f32", ns // 2))
