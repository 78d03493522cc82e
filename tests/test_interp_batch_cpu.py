"""FlowNetS_interp list inference without a GPU: the uint8 twin of adapt_x_matches, the list-line dispatch, the CLI
parser and fn2_pack_interp_u8's argument checks."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    from src.flownet_s_interp.flownet_s_interp import FlowNetS_interp
    from src.net import Mode
    return FlowNetS_interp(mode=Mode.TEST)


@pytest.mark.parametrize("image,mask,flags", [("bytes", 255, (True, True)), ("bytes", 1, (True, False)),
                                              ("01", 255, (False, True)), ("01", 1, (False, False))])
@pytest.mark.parametrize("shape", [(100, 150), (128, 192)])
def test_adapt_x_matches_u8_agrees_with_adapt_x_matches(image, mask, flags, shape):
    net = _net()
    rng = np.random.default_rng(4)
    h, w = shape
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if image == "bytes" else (rng.random((h, w, 3)) < 0.5).astype(np.uint8)
    m = (rng.random((h, w)) > 0.9).astype(np.uint8) * mask
    sf = rng.standard_normal((h, w, 2)).astype(np.float32) * (m > 0)[..., None]
    fa, fm, fsf, finfo = net.adapt_x_matches(img, m, sf)
    ua, um, usf, uinfo, scale = net.adapt_x_matches_u8(img, m, sf)
    assert scale == flags and uinfo == finfo
    assert finfo == (None if shape == (128, 192) else (1, 100, 150, 3))
    assert ua.shape == fa.shape == (1, 128, 192, 3) and um.shape == fm.shape == (1, 128, 192, 1) and usf.shape == fsf.shape
    assert ua.dtype == np.uint8 and um.dtype == np.uint8 and usf.dtype == np.float32
    assert ua.flags["C_CONTIGUOUS"] and um.flags["C_CONTIGUOUS"] and usf.flags["C_CONTIGUOUS"]
    # the device's conversion: the table float32(float64(i) / 255.0) where the flag is set, float32(i) where it is not
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    raw = np.arange(256, dtype=np.float32)
    assert np.array_equal((lut if scale[0] else raw)[ua], fa)
    assert np.array_equal((lut if scale[1] else raw)[um], fm)
    assert np.array_equal(usf, fsf)


def test_adapt_x_matches_u8_rejects_what_it_cannot_take():
    net = _net()
    img = np.zeros((20, 30, 3), np.uint8)
    sf = np.zeros((20, 30, 2), np.float32)
    with pytest.raises(AssertionError, match="Mask has invalid dimensions"):
        net.adapt_x_matches_u8(img, np.zeros((20, 31), np.uint8), sf)
    with pytest.raises(AssertionError, match="Mask has invalid dimensions"):
        net.adapt_x_matches(img, np.zeros((20, 31), np.uint8), sf)
    with pytest.raises(ValueError):
        net.adapt_x_matches_u8(img.astype(np.float32), np.zeros((20, 30), np.uint8), sf)
    with pytest.raises(ValueError):
        net.adapt_x_matches_u8(img, np.zeros((20, 30), np.float32), sf)


def test_matches_line_fields_dispatch():
    from src.net import matches_line_fields
    p = ["I1", "MM", "SF", "GT", "OCC", "INV", "I2"]
    none = dict(gt=None, occ=None, inv=None, image_b=None)
    base = dict(image="I1", matches="MM", sparse="SF")
    assert matches_line_fields(p[:3]) == {**base, **none}
    assert matches_line_fields(p[:4]) == {**base, **none, "gt": "GT"}
    # 5 and 6 fields: the last one is the second image (the reference's `... GT OCC` / `... GT OCC INV` branches are shadowed)
    assert matches_line_fields(["I1", "MM", "SF", "GT", "X"]) == {**base, **none, "gt": "GT", "image_b": "X"}
    assert matches_line_fields(["I1", "MM", "SF", "GT", "OCC", "X"]) == {**base, **none, "gt": "GT", "occ": "OCC", "image_b": "X"}
    assert matches_line_fields(p) == {**base, "gt": "GT", "occ": "OCC", "inv": "INV", "image_b": "I2"}
    for bad in (p[:2], p + ["extra"], p[:1], []):
        with pytest.raises(AssertionError, match="More paths than expected"):
            matches_line_fields(bad)


def test_test_batch_rejects_unknown_input_types_only(tmp_path):
    net = _net()
    lst = tmp_path / "l.txt"
    lst.write_text("a b\n")
    with pytest.raises(NotImplementedError):
        net.test_batch(None, str(lst), str(tmp_path), input_type="image_triplets")
    net.weights = {}  # (keeps the call from building seeded weights: the line check comes first)
    with pytest.raises(AssertionError, match="More paths than expected"):
        net.test_batch(None, str(lst), str(tmp_path), input_type="image_matches", log_metrics2file=False)


def test_net_test_signature_gains_the_mask_paths():
    from src.net import Net
    names = list(inspect.signature(Net.test).parameters)
    assert names[-3:] == ["occ_mask", "inv_mask", "variational_refinement"]
    sig = inspect.signature(Net.test)
    assert sig.parameters["occ_mask"].default is None and sig.parameters["inv_mask"].default is None


def test_cli_parser_list_form():
    from src.flownet_s_interp.test import build_parser, is_list
    p = build_parser()
    f = p.parse_args(["--input_a", "val.txt", "--out", "o"])          # a list needs neither --matches_a nor --sparse_flow
    assert f.matches_a is None and f.sparse_flow is None and is_list(f.input_a)
    assert f.input_type == "image_matches" and f.occ_mask is None and f.inv_mask is None
    assert f.accumulate_metrics is True and f.log_metrics2file is False
    assert (f.width, f.height, f.batch_size) == (1024, 436, 8)
    f = p.parse_args(["--input_a", "a.png", "--matches_a", "m.png", "--sparse_flow", "s.flo", "--out", "o", "--occ_mask", "occ.png",
                      "--inv_mask", "inv.png", "--accumulate_metrics", "false", "--log_metrics2file", "true", "--width", "512",
                      "--height", "384", "--batch_size", "4", "--input_type", "image_pairs"])
    assert not is_list(f.input_a) and (f.occ_mask, f.inv_mask) == ("occ.png", "inv.png")
    assert f.accumulate_metrics is False and f.log_metrics2file is True
    assert (f.width, f.height, f.batch_size, f.input_type) == (512, 384, 4, "image_pairs")


def test_engine_option_belongs_to_the_interp_model():
    from src.engine import Engine
    assert inspect.signature(Engine.__init__).parameters["interp_u8_inputs"].default is False
    assert hasattr(Engine, "set_inputs_interp_u8")


@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


def test_pack_interp_u8_is_exported_and_validates_without_a_device(hip):
    lib = hip.lib()
    assert "fn2_pack_interp_u8" in hip.PROTOTYPES and hasattr(lib, "fn2_pack_interp_u8")
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    assert "int fn2_pack_interp_u8(" in header
    # host memory stands in for the pointers: every call below is refused before anything is launched
    store = (C.c_char * 4096)()
    base = (C.addressof(store) + 255) & ~255
    img, mask, sparse, lut, flags, out = (base + 256 * k for k in range(6))

    def call(img=img, mask=mask, sparse=sparse, lut=lut, flags=flags, data=out, dtype=hip.FN2_F32, c=6, cs=8, c0=0, h=10,
             w=12, pad=3, view=True):
        t = hip.Fn2Tensor(data, dtype, 1, h, w, c, cs, c0)
        return lib.fn2_pack_interp_u8(img, mask, sparse, lut, flags, C.byref(t) if view else None, pad, None)

    for kw, word in ((dict(img=None), b"null"), (dict(mask=None), b"null"), (dict(sparse=None), b"null"),
                     (dict(lut=None), b"null"), (dict(flags=None), b"null"), (dict(view=False), b"null"),
                     (dict(data=None), b"null"), (dict(dtype=7), b"dtype"), (dict(c=3), b"6 channels"),
                     (dict(cs=12), b"8-channel"), (dict(cs=16, c0=4), b"8-channel"), (dict(c0=8), b"8-channel"),
                     (dict(pad=5), b"border"), (dict(pad=-1), b"border"), (dict(sparse=sparse + 4), b"8-byte"),
                     (dict(data=out + 8), b"16-byte")):
        rc = call(**kw)
        assert rc == hip.ERR_INVALID_ARGUMENT and word in lib.fn2_last_error(), (kw, lib.fn2_last_error())
        with pytest.raises(ValueError):
            hip.check(rc)


class _StubEngine:
    """Stands in for the HIP engine: records what Net._infer_matches hands it and returns the sparse flow as the flow."""

    def __init__(self, n, h, w):
        import torch
        self.shape, self.calls, self.torch = (n, h, w), [], torch
        self.outputs = {}

    def set_inputs_interp_u8(self, a, m, sf, flags):
        assert a.shape == self.shape + (3,) and m.shape == self.shape and sf.shape == self.shape + (2,)
        assert a.dtype == np.uint8 and m.dtype == np.uint8 and sf.dtype == np.float32 and flags.shape == (self.shape[0], 2)
        self.calls.append((a.copy(), m.copy(), np.array(flags)))
        self.outputs = {"flow": self.torch.from_numpy(sf.copy())}

    def launch(self):
        pass


def test_test_batch_image_matches_groups_lines_by_padded_size(tmp_path, monkeypatch):
    """The host side of the list path with a stub engine: `batch_size` lines per chunk, one launch per padded size,
    short groups padded with zero samples, 0/255 and 0/1 masks in one launch, flows cropped and written per line."""
    from PIL import Image
    from src import flowlib
    net = _net()
    net.weights = {}
    engines = {}

    def engine(batch, height, width, uint8_inputs=False, interp_u8_inputs=False):
        assert interp_u8_inputs and not uint8_inputs
        return engines.setdefault((batch, height, width), _StubEngine(batch, height, width))

    monkeypatch.setattr(net, "engine", engine)
    rng = np.random.default_rng(1)
    seq = tmp_path / "seq"
    seq.mkdir()
    lines, want = [], []
    for k, (nf, h, w, top) in enumerate([(3, 100, 150, 255), (4, 100, 150, 1), (4, 60, 150, 255)]):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        m = (rng.random((h, w)) > 0.5).astype(np.uint8) * top
        sf = rng.standard_normal((h, w, 2)).astype(np.float32)
        p = [str(seq / ("f%d%s" % (k, s))) for s in (".png", "_m.png", "_sf.flo", "_gt.flo")]
        Image.fromarray(img).save(p[0])
        Image.fromarray(m).save(p[1])
        flowlib.write_flow(sf, p[2])
        flowlib.write_flow(sf + 1, p[3])
        lines.append(" ".join(p[:nf]))
        want.append((img, m, sf))
    lst = tmp_path / "v.txt"
    lst.write_text("\n".join(lines) + "\n")
    flows = net.test_batch(None, str(lst), str(tmp_path / "out"), input_type="image_matches", save_image=False,
                           accumulate_metrics=True, batch_size=2)
    assert sorted(engines) == [(2, 64, 192), (2, 128, 192)]
    big, small = engines[(2, 128, 192)], engines[(2, 64, 192)]
    assert len(big.calls) == 1 and len(small.calls) == 1
    a, m, flags = big.calls[0]
    assert flags.tolist() == [[1, 1], [1, 0]]                     # the 0/255 and the 0/1 mask share the launch
    assert np.array_equal(a[0, :100, :150], want[0][0]) and np.array_equal(m[1, :100, :150], want[1][1])
    assert not a[:, 100:].any() and not a[:, :, 150:].any()
    a, m, flags = small.calls[0]
    assert flags.tolist() == [[1, 1], [0, 0]] and not a[1].any() and not m[1].any()   # short group: a zero sample
    for (img, _, sf), flow, k in zip(want, flows, range(3)):
        assert np.array_equal(flow, sf)
        assert np.array_equal(flowlib.read_flow(str(tmp_path / "out" / "seq" / ("f%d_flow.flo" % k))), flow)
    log = (tmp_path / "out" / "v_metrics.log").read_text()
    assert log.count("MPI-Sintel Flow Error Metrics") == 3 and "f0" not in log.replace("f0_", "") and "(AVERAGE)" in log
