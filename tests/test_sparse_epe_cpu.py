"""Sparse ground truth without a GPU: the float64 twin of the sparse EPE checked against torch autograd of its own forward and
a case worked by hand, the exported symbols and every argument check that has to come before any device use (library,
wrapper, trainer, loader, CLI), the 16-bit PNG codec against an independent encoder, KITTI's flow format, its metrics, and
the crop window of the loader."""
import inspect
import math
import os
import struct
import zlib

import numpy as np
import pytest

import sparse_epe_twin as twin
from test_gpu_sparse_epe import PATTERNS, SHAPES, case, check_invalid_arguments, five_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("shape", [(2, 5, 7), (3, 4, 5), (2, 3, 70)])
def test_twin_gradient_is_autograd_of_its_forward(shape):
    """M and the mask are constants; pixels with pred == label (sqrt has no derivative at 0) are moved off the label."""
    import torch
    pred, label = case(9, shape, "half")
    same = (pred == label).all(axis=-1)
    pred[same, 0] += 0.5
    L, g, m = twin.loss_and_grad(pred, label, 0.064, grad_mult=3.0)
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    Lt = twin.torch_loss(p, label, 0.064)
    Lt.backward()
    assert 0 < m < same.size and L > 0
    assert abs(float(Lt.detach()) - L) <= 1e-12 * L
    np.testing.assert_allclose(3.0 * p.grad.numpy(), g, rtol=1e-12, atol=1e-15)
    assert not g[~twin.valid_mask(label)].any()


def test_twin_on_a_case_worked_by_hand():
    """n 1, h 2, w 3, weight 0.5, grad_mult 4.  Labels: (0,0) NaN in u, (1,2) inf in v, so M = 4 and weight h w / M = 0.75.
      (0,1): d = (3, 4), e = 5      (0,2): d = (0, 0), e = 0      (1,0): d = (-6, 8), e = 10      (1,1): d = (0, -2), e = 2
    L = 0.75 * 17;  dpred = 4 * 0.75 * d / e."""
    pred = np.zeros((1, 2, 3, 2), np.float32)
    label = np.zeros((1, 2, 3, 2), np.float32)
    label[0, 0, 0] = (np.nan, 1.0)
    label[0, 1, 2] = (2.0, np.inf)
    pred[0, 0, 0], pred[0, 1, 2] = (5.0, 5.0), (7.0, 7.0)           # read by nothing
    pred[0, 0, 1], label[0, 0, 1] = (4.0, 6.0), (1.0, 2.0)
    pred[0, 0, 2], label[0, 0, 2] = (1.5, -2.0), (1.5, -2.0)
    pred[0, 1, 0], label[0, 1, 0] = (-5.0, 8.0), (1.0, 0.0)
    pred[0, 1, 1], label[0, 1, 1] = (3.0, 0.0), (3.0, 2.0)
    L, g, m = twin.loss_and_grad(pred, label, 0.5, grad_mult=4.0)
    assert m == 4 and L == pytest.approx(0.75 * 17.0, rel=1e-15)
    want = np.zeros((1, 2, 3, 2))
    want[0, 0, 1] = (3 * 0.6, 3 * 0.8)
    want[0, 1, 0] = (3 * -0.6, 3 * 0.8)
    want[0, 1, 1] = (0.0, -3.0)
    np.testing.assert_allclose(g, want, rtol=1e-15, atol=0)
    # full validity is average_endpoint_error: weight / n * sum e
    pred, label = case(0, (3, 4, 5), "all")
    L, g, m = twin.loss_and_grad(pred, label, 0.064)
    d = pred.astype(np.float64) - label
    assert m == 60 and L == pytest.approx(float(np.float32(0.064)) / 3 * np.sqrt((d * d).sum(-1)).sum(), rel=1e-14)
    # no ground truth at all
    L, g, m = twin.loss_and_grad(*case(0, (2, 5, 7), "none"), 0.064)
    assert (L, m) == (0.0, 0) and not g.any()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("shape", SHAPES)
def test_preconditions_of_the_gpu_op_tests_hold(shape, pattern):
    """Every difference the kernel forms in fp32 is exact on these inputs, and the patterns are what their names say."""
    pred, label = case(1, shape, pattern)
    valid = twin.valid_mask(label)
    assert np.all(pred * 2 == np.round(pred * 2)) and np.abs(pred).max() <= 8
    assert np.all(label[valid] * 2 == np.round(label[valid] * 2)) and (not valid.any() or np.abs(label[valid]).max() <= 8)
    n = valid.size
    want = {"all": n, "none": 0, "one": 1}.get(pattern)
    assert want is None or valid.sum() == want
    if pattern == "u_only":
        assert np.isfinite(label[..., 1]).all() and np.isnan(label[..., 0]).sum() == n - valid.sum()
    if pattern == "v_only":
        assert np.isfinite(label[..., 0]).all() and np.isnan(label[..., 1]).sum() == n - valid.sum()
    if pattern == "inf":
        assert not np.isnan(label).any() and (n < 8 or (np.isposinf(label).any() and np.isneginf(label).any()))
    if shape == (4, 6, 130):
        assert n > 256 * 4 and (pattern in ("all", "none", "one") or 0 < valid.sum() < n)   # several blocks, mixed
        assert pattern != "all" or ((pred == label).all(-1).sum() > 0)
    assert all(0 < twin.valid_mask(l).sum() < l[..., 0].size or l.shape[1:3] == (1, 1) for _, l, _ in five_levels(3))


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


def test_entry_points_are_exported_declared_and_validate_without_a_device(hip):
    import ctypes as C
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    for name, nargs in (("fn2_sparse_epe_count", 4), ("fn2_sparse_epe_loss_grad", 6)):
        assert name in hip.PROTOTYPES and hasattr(lib, name) and ("int %s(" % name) in header
        res, args = hip.PROTOTYPES[name]
        assert res is C.c_int and len(args) == nargs and args[0] == C.POINTER(hip.Fn2SparseEpeLevel)
    assert hip.PROTOTYPES["fn2_sparse_epe_loss_grad"][1][3] is C.c_float
    assert [f[0] for f in hip.Fn2SparseEpeLevel._fields_] == ["pred", "label", "dpred", "count", "h", "w", "weight"]
    assert "} fn2_sparse_epe_level;" in header and "its own M" in header
    assert "sparse_epe.hip" in open(os.path.join(ROOT, "flownet2-tf_amd", "csrc", "Makefile")).read()
    check_invalid_arguments(hip)


# ------------------------------------------------------------------------------------------------ Python surface
def test_wrapper_rejects_bad_arguments_before_touching_a_device(monkeypatch):
    import torch
    from src import _hip, sparse_epe
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was asked for"))
    z = torch.zeros
    with pytest.raises(ValueError, match="device tensor"):
        sparse_epe.sparse_epe_loss(z(2, 4, 5, 2), z(2, 4, 5, 2), 1.0)
    with pytest.raises(ValueError, match="device tensor"):
        sparse_epe.sparse_epe_loss(z(2, 4, 5, 2).numpy(), z(2, 4, 5, 2).numpy(), 1.0)
    for p, l, word in ((z(4, 5, 2), z(4, 5, 2), "rank 4"), (z(2, 4, 5, 3), z(2, 4, 5, 3), "2 channels"),
                       (z(2, 4, 5, 2), z(2, 4, 6, 2), "same shape"), (z(2, 0, 5, 2), z(2, 0, 5, 2), "empty"),
                       (z(2, 4, 5, 2, dtype=torch.int32), z(2, 4, 5, 2), "floating-point")):
        with pytest.raises(ValueError, match=word):
            sparse_epe.sparse_epe_loss(p, l, 1.0)
    nan, inf = float("nan"), float("inf")
    for w, gm in ((-1.0, 1.0), (nan, 1.0), (inf, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, nan), (1.0, inf)):
        with pytest.raises(ValueError):
            sparse_epe.check_constants(w, gm)
    assert sparse_epe.check_constants(0, 16384) == (0.0, 16384.0)
    with pytest.raises(ValueError, match="device tensors only"):
        sparse_epe.level(z(2, 4, 5, 2), z(2, 4, 5, 2), z(2, 4, 5, 2), z(1, dtype=torch.int32), 1.0)
    with pytest.raises(ValueError, match="levels"):
        sparse_epe.level_table([])
    with pytest.raises(ValueError, match="levels"):
        sparse_epe.level_table([None] * 9)
    assert "import src.smoothness, src.sparse_epe" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_trainer_arguments_are_checked_before_the_engine_is_built(monkeypatch):
    from src import trainer
    monkeypatch.setattr(trainer, "Engine", lambda *a, **k: pytest.fail("the engine was asked for"))
    make = lambda **kw: trainer.FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128, sparse_gt=True), **kw))
    with pytest.raises(ValueError, match="unsupervised"):
        make(unsupervised=True)
    for mode in ("hard", "edges"):
        with pytest.raises(ValueError, match="mining"):
            make(model="FlowNetS_interp", add_hard_flow_mining=mode)
    for model in ("FlowNetS_interp", "FlowNet2"):
        with pytest.raises(ValueError, match="not %s" % model):
            make(model=model)
    assert inspect.signature(trainer.FlowNetSTrainer.__init__).parameters["sparse_gt"].default is False
    assert list(inspect.signature(trainer.FlowNetSTrainer.evaluate_sparse).parameters) == ["self", "batches", "max_batches"]


@pytest.mark.parametrize("model", ["flownet_s", "flownet_sd", "flownet_c", "flownet_cs", "flownet_css"])
def test_cli_flags_and_their_checks(model, tmp_path, monkeypatch):
    import importlib
    from src.flownet_s import train as cli
    mod = importlib.import_module("src.%s.train" % model)
    assert mod.parse_and_run is cli.parse_and_run                  # one CLI for the five models
    base = ["--list", "l.txt", "--out", str(tmp_path)]
    parse = lambda extra: cli.build_parser().parse_args(base + extra)
    flags = parse([])
    assert (flags.sparse_gt, flags.crop) == (False, False) and cli.sparse_kwargs(flags) == ({}, {})
    assert cli.sparse_kwargs(parse(["--sparse_gt", "--no-augment"])) == (dict(sparse_gt=True), dict(sparse_gt=True))
    for aug in ("selflow", "pair"):
        got = cli.sparse_kwargs(parse(["--sparse_gt", "--crop", "--augmentation", aug, "--height", "128", "--width", "192"]))
        assert got == (dict(sparse_gt=True), dict(sparse_gt=True, crop=(128, 192)))
    assert cli.sparse_kwargs(parse(["--crop", "--no-augment"])) == ({}, dict(crop=(384, 512)))
    assert cli.sparse_kwargs(parse(["--crop", "--unsupervised", "--augmentation", "pair"])) == ({}, dict(crop=(384, 512)))
    # refused before torch or the device are touched: the trainer is never reached
    from src import trainer
    monkeypatch.setattr(trainer, "FlowNetSTrainer", lambda *a, **k: pytest.fail("the trainer was asked for"))
    for extra, word in ((["--sparse_gt"], "--no-augment"), (["--sparse_gt", "--augmentation", "plugin"], "--no-augment"),
                        (["--crop"], "own crop"), (["--crop", "--augmentation", "plugin"], "own crop"),
                        (["--sparse_gt", "--unsupervised", "--no-augment"], "--unsupervised"),
                        (["--crop", "--no-augment", "--height", "0"], ">= 1")):
        with pytest.raises(ValueError, match=word):
            cli.main(parse(extra))
    flags = parse(["--sparse_gt", "--no-augment"])
    flags.model = "FlowNet2"
    with pytest.raises(ValueError, match="covers"):
        cli.main(flags)
    assert not os.listdir(str(tmp_path))


# ------------------------------------------------------------------------------------------------ 16-bit PNG codec
def png_chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload) & 0xFFFFFFFF)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def encode_png(image, filters, depth=16, colour=2, interlace=0, idat_pieces=1):
    """An encoder of its own, byte by byte from the PNG specification: row y is filtered with filters[y % len(filters)]."""
    h, w = image.shape[:2]
    raw = [list(image[y].astype(">u2" if depth == 16 else np.uint8).tobytes()) for y in range(h)]
    bpp = len(raw[0]) // w
    data = bytearray()
    for y, row in enumerate(raw):
        ft = filters[y % len(filters)]
        up = raw[y - 1] if y else [0] * len(row)
        data.append(ft)
        for i, x in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            pred = (0, a, up[i], (a + up[i]) // 2, paeth(a, up[i], c))[ft]
            data.append((x - pred) & 255)
    z = zlib.compress(bytes(data))
    cut = [len(z) * k // idat_pieces for k in range(idat_pieces + 1)]
    return (b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
            + png_chunk(b"tEXt", b"Comment\x00an ancillary chunk in between")
            + b"".join(png_chunk(b"IDAT", z[cut[k]:cut[k + 1]]) for k in range(idat_pieces)) + png_chunk(b"IEND", b""))


def picture(seed, h=7, w=9):
    """Smooth ramps plus noise in every byte: filters predict well in places and wrap around in others."""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(h)[:, None, None] * 4099 + np.arange(w)[None, :, None] * 977 + np.arange(3)[None, None, :] * 21001)
    return ((ramp + rng.integers(0, 700, size=(h, w, 3))) % 65536).astype(np.uint16)


@pytest.mark.parametrize("filters", [(0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0), (1, 4)])
def test_png_reader_decodes_every_row_filter(filters, tmp_path):
    from src import png16
    img = picture(len(filters) * 10 + filters[0])
    path = tmp_path / "f.png"
    path.write_bytes(encode_png(img, filters))
    got = png16.read_rgb16(str(path))
    assert got.dtype == np.uint16 and np.array_equal(got, img)


def test_png_reader_takes_several_idat_chunks_and_its_own_writer(tmp_path):
    from src import png16
    img = picture(3, 12, 5)
    path = tmp_path / "two.png"
    path.write_bytes(encode_png(img, (4, 1), idat_pieces=2))
    assert np.array_equal(png16.read_rgb16(str(path)), img)
    path.write_bytes(encode_png(img, (3,), idat_pieces=5))
    assert np.array_equal(png16.read_rgb16(str(path)), img)
    own = tmp_path / "own.png"
    png16.write_rgb16(str(own), img)
    assert np.array_equal(png16.read_rgb16(str(own)), img)
    # the writer's file is a PNG to another decoder too (Pillow keeps 8 of the 16 bits: size and mode are what it can tell)
    from PIL import Image
    with Image.open(str(own)) as im:
        assert im.size == (5, 12) and im.format == "PNG"
    with pytest.raises(ValueError, match="uint16"):
        png16.write_rgb16(str(own), img.astype(np.int32))


def test_png_reader_refuses_what_it_does_not_read(tmp_path):
    from src import png16
    img = picture(4)
    good = encode_png(img, (0,))
    cases = {"eight.png": (encode_png((img >> 8).astype(np.uint8), (0,), depth=8), "bit depth 8"),
             "palette.png": (encode_png((img >> 8).astype(np.uint8)[:, :, :1], (0,), depth=8, colour=3), "colour type 3"),
             "grey16.png": (encode_png(img[:, :, :1], (0,), colour=0), "colour type 0"),
             "interlaced.png": (encode_png(img, (0,), interlace=1), "interlaced"),
             "truncated.png": (good[:len(good) - 30], "truncated"),
             "no_iend.png": (good[:len(good) - 12], "truncated"),
             "short.png": (good[:20], "truncated"),
             "not.png": (b"P6\n" + good, "signature")}
    crc = bytearray(good)
    crc[good.index(b"IDAT") + 9] ^= 0x40                            # one bit inside the image data
    cases["crc.png"] = (bytes(crc), "CRC")
    h, w = img.shape[:2]
    rows = bytearray(b"".join(b"\x00" + img[y].astype(">u2").tobytes() for y in range(h)))
    rows[0] = 7                                                     # a filter type that does not exist
    cases["filter7.png"] = (b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0))
                            + png_chunk(b"IDAT", zlib.compress(bytes(rows))) + png_chunk(b"IEND", b""), "filter 7")
    cases["fewrows.png"] = (b"\x89PNG\r\n\x1a\n" + png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h + 1, 16, 2, 0, 0, 0))
                            + png_chunk(b"IDAT", zlib.compress(bytes(rows))) + png_chunk(b"IEND", b""), "truncated")
    for name, (data, word) in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises(ValueError, match=word) as err:
            png16.read_rgb16(str(path))
        assert name in str(err.value)                               # the message names the file


# ------------------------------------------------------------------------------------------------ KITTI flow files
def test_flow_png_round_trip_is_exact(tmp_path):
    from src import flowlib
    rng = np.random.default_rng(8)
    flow = rng.integers(-511 * 64, 511 * 64 + 1, size=(11, 13, 2)) / 64.0
    flow[0, 0], flow[0, 1] = (-511.0, 511.0), (0.0, 1 / 64.0)
    flow[2, 3] = (np.nan, 1.0)
    flow[4, 5] = (2.0, np.inf)
    flow[6, 7] = (np.nan, np.nan)
    path = str(tmp_path / "gt.png")
    flowlib.write_flow_png(flow, path)
    got = flowlib.read_flow_png(path)
    assert got.shape == (11, 13, 3) and got.dtype == np.float64
    valid = np.isfinite(flow).all(-1)
    assert valid.sum() == 11 * 13 - 3 and np.array_equal(got[..., 2], valid.astype(np.float64))
    assert np.array_equal(got[valid][:, :2], flow[valid])
    assert not got[~valid].any()                                    # invalid pixels come back 0, 0, 0
    from src import png16
    raw = png16.read_rgb16(path)
    assert not raw[~valid].any() and raw[0, 0].tolist() == [32768 - 511 * 64, 32768 + 511 * 64, 1]
    # an explicit mask: a finite pixel can be declared invalid, a non-finite one cannot be declared valid
    mask = np.ones((11, 13), bool)
    mask[1, 1] = False
    flowlib.write_flow_png(flow.astype(np.float32), path, valid=mask)
    got = flowlib.read_flow_png(path)
    assert got[1, 1].tolist() == [0, 0, 0] and got[2, 3].tolist() == [0, 0, 0] and got[0, 1].tolist() == [0.0, 1 / 64.0, 1.0]
    # the devkit's clip and truncation
    flowlib.write_flow_png(np.array([[[600.0, -600.0], [1 / 128.0, -1 / 128.0]]]), path)
    assert png16.read_rgb16(path)[0].tolist() == [[65535, 0, 1], [32768, 32767, 1]]
    with pytest.raises(ValueError, match=r"\(H, W, 2\)"):
        flowlib.write_flow_png(np.zeros((3, 4, 3)), path)


def test_read_sparse_flow_on_a_png_and_on_a_flo(tmp_path):
    from src import flowlib
    flow = np.array([[[1.5, -2.0], [np.nan, np.nan], [0.0, 0.0]], [[3.25, 4.0], [-1.0, 1.0], [np.nan, np.nan]]])
    png = str(tmp_path / "gt.PNG")
    flowlib.write_flow_png(flow, png)
    got = flowlib.read_sparse_flow(png)
    assert got.dtype == np.float32 and got.shape == (2, 3, 2)
    np.testing.assert_array_equal(got, flow.astype(np.float32))     # (NaN equals NaN here; a valid 0, 0 stays 0, 0)
    flo = str(tmp_path / "gt.flo")
    dense = np.nan_to_num(flow, nan=1e10).astype(np.float32)
    dense[1, 2] = (2.0, -1e10)                                      # one component is enough
    flowlib.write_flow(dense, flo)
    got = flowlib.read_sparse_flow(flo)
    want = flow.astype(np.float32)
    np.testing.assert_array_equal(got, want)
    assert np.isnan(got[0, 1]).all() and np.isnan(got[1, 2]).all() and got.dtype == np.float32
    np.testing.assert_array_equal(flowlib.read_flow(flo), dense)    # read_flow is what it was


def test_kitti_metrics_on_a_case_worked_by_hand():
    """2 x 3.  gt magnitudes and errors:
      (0,0) gt (100, 0), err 5 = exactly 5 %, > 3      not an outlier
      (0,1) gt (10, 0),  err exactly 3                 not an outlier
      (0,2) gt (10, 0),  err 4 > 3 and > 0.5           outlier
      (1,0) gt (200, 0), err 6 > 3 but 3 % of 200      not an outlier
      (1,1) gt (0, 0),   err 3.5 > 3 and > 0           outlier
      (1,2) no ground truth
    epe = (5 + 3 + 4 + 6 + 3.5) / 5 = 4.3, Fl-all = 2 / 5, valid share 5 / 6."""
    from src import flowlib
    gt = np.array([[[100.0, 0], [10, 0], [10, 0]], [[200, 0], [0, 0], [np.nan, 1]]])
    est = np.array([[[105.0, 0], [10, 3], [10, -4]], [[194, 0], [0, 3.5], [1e9, 1e9]]])
    m = flowlib.kitti_metrics(est, gt)
    assert set(m) == {"epe", "fl_all", "valid_share"}
    assert m["epe"] == pytest.approx(4.3, rel=1e-15) and m["fl_all"] == 0.4 and m["valid_share"] == pytest.approx(5 / 6)
    mask = np.ones((2, 3), bool)
    mask[0, 2] = False
    m = flowlib.kitti_metrics(est.astype(np.float32), gt.astype(np.float32), valid=mask)   # a non-finite pixel never counts
    assert m["epe"] == pytest.approx(17.5 / 4) and m["fl_all"] == 0.25 and m["valid_share"] == pytest.approx(4 / 6)
    m = flowlib.kitti_metrics(est, np.full((2, 3, 2), np.nan))
    assert math.isnan(m["epe"]) and math.isnan(m["fl_all"]) and m["valid_share"] == 0.0
    m = flowlib.kitti_metrics(est, gt, valid=np.zeros((2, 3), bool))
    assert math.isnan(m["epe"]) and m["valid_share"] == 0.0
    assert not hasattr(flowlib, "flow_error_image")


# ------------------------------------------------------------------------------------------------ loader and crop
def test_crop_window_arithmetic():
    from src import dataloader as D
    assert D.crop_window((140, 200, 3), (128, 192), "centre", None) == (6, 4)
    assert D.crop_window((128, 192), (128, 192), "centre", None) == (0, 0)
    assert D.crop_window((129, 193), (128, 192), "centre", None) == (0, 0)
    a, b = np.random.default_rng([5, 0xC809]), np.random.default_rng([5, 0xC809])
    wa = [D.crop_window((375, 1242), (320, 1152), "random", a) for _ in range(200)]
    wb = [D.crop_window((375, 1242), (320, 1152), "random", b) for _ in range(200)]
    assert wa == wb                                                 # the same seed gives the same windows
    ys, xs = {w[0] for w in wa}, {w[1] for w in wa}
    assert min(ys) == 0 and max(ys) == 55 and min(xs) >= 0 and max(xs) <= 90 and len(xs) > 40   # every position, none outside
    assert D.crop_window((128, 192), (128, 192), "random", a) == (0, 0)
    for shape in ((127, 192), (128, 191)):
        with pytest.raises(ValueError, match="frame_17.png.*smaller than the crop 128x192"):
            D.crop_window(shape, (128, 192), "random", a, "frame_17.png")
    for crop, mode in (((128,), "random"), ((0, 5), "random"), ("ab", "random"), ((128, 192), "center")):
        with pytest.raises(ValueError, match="crop"):
            D.check_crop(crop, mode)
    assert D.check_crop(None, "centre") is None and D.check_crop([128.0, 192], "random") == (128, 192)


@pytest.fixture
def kitti_like(tmp_path):
    """Seven samples of differing sizes: PNG frames whose pixels tell sample, row and column, and KITTI flow PNGs."""
    from PIL import Image
    from src import flowlib
    rows = []
    for k in range(7):
        h, w = 20 + k % 3, 30 + k % 4
        yy, xx = np.mgrid[0:h, 0:w]
        for j in (0, 1):
            Image.fromarray(np.stack([np.full((h, w), 10 * k + j), yy, xx], -1).astype(np.uint8)).save(
                str(tmp_path / ("%d_%d.png" % (k, j))))
        flow = np.stack([yy + k / 64.0, -xx.astype(np.float64)], -1)
        flow[(yy + xx) % 3 == 0] = np.nan
        flowlib.write_flow_png(flow, str(tmp_path / ("%d_flow.png" % k)))
        rows.append([str(tmp_path / ("%d_%d.png" % (k, 0))), str(tmp_path / ("%d_%d.png" % (k, 1))),
                     str(tmp_path / ("%d_flow.png" % k))])
    lst = tmp_path / "kitti.txt"
    lst.write_text("".join(" ".join(r) + "\n" for r in rows))
    return str(lst), rows


def host_loader(monkeypatch):
    """load_batches with its one device call answered by the host: the batches are CPU tensors."""
    import torch
    from src import dataloader as D
    monkeypatch.setattr(D.P._hip, "require_device", lambda: torch.device("cpu"))
    return D


def sample_ids(batches):
    return [[int(round(float(a[i, 0, 0, 0]) * 255)) // 10 for i in range(a.shape[0])] for a, _, _ in batches]


def test_loader_crops_sparse_samples_into_batches(kitti_like, monkeypatch):
    D = host_loader(monkeypatch)
    lst, rows = kitti_like
    kw = dict(batch_size=2, data_augmentation=False, seed=3, epochs=2, sparse_gt=True)
    with pytest.raises(ValueError):                                 # differing sizes do not stack
        list(D.load_batches(lst, **kw))
    got = list(D.load_batches(lst, crop=(16, 24), **kw))
    assert len(got) == 6
    perm = np.random.default_rng(3)                                  # a restatement of the draws: one permutation per epoch
    want = [list(p[:2]) + list(p[2:4]) + list(p[4:6]) for p in (perm.permutation(7), perm.permutation(7))]
    assert sum(sample_ids(got), []) == [int(v) for v in sum(want, [])]
    # one window per sample READ, in reading order: the seventh sample of an epoch is cut too, then left over
    win = np.random.default_rng([3, 0xC809])
    perm = np.random.default_rng(3)
    windows = [[D.crop_window((20 + k % 3, 30 + k % 4), (16, 24), "random", win) for k in perm.permutation(7)][:6]
               for _ in range(2)]
    windows = iter(sum(windows, []))
    for a, b, f in got:
        assert tuple(a.shape) == (2, 16, 24, 3) and tuple(b.shape) == (2, 16, 24, 3) and tuple(f.shape) == (2, 16, 24, 2)
        for i in range(2):
            k = int(round(float(a[i, 0, 0, 0]) * 255)) // 10
            y0, x0 = next(windows)
            rows_, cols = np.mgrid[y0:y0 + 16, x0:x0 + 24]
            np.testing.assert_array_equal(np.round(a[i, :, :, 1].numpy() * 255), rows_)   # the window drawn, in both frames
            np.testing.assert_array_equal(np.round(b[i, :, :, 2].numpy() * 255), cols)
            assert int(round(float(b[i, 0, 0, 0]) * 255)) == 10 * k + 1
            nan = (rows_ + cols) % 3 == 0                           # and in the flow: NaN stays with its pixel
            fi = f[i].numpy()
            assert np.array_equal(np.isnan(fi).all(-1), nan) and np.array_equal(np.isnan(fi).any(-1), nan)
            np.testing.assert_array_equal(fi[~nan][:, 0], (rows_ + k / 64.0)[~nan].astype(np.float32))
            np.testing.assert_array_equal(fi[~nan][:, 1], -cols[~nan].astype(np.float32))
    centre = list(D.load_batches(lst, crop=(16, 24), crop_mode="centre", **kw))
    assert sample_ids(centre) == sample_ids(got)                    # the sample order does not depend on the crop
    for a, _, _ in centre:
        for i in range(2):
            k = int(round(float(a[i, 0, 0, 0]) * 255)) // 10
            assert round(float(a[i, 0, 0, 1]) * 255) == (20 + k % 3 - 16) // 2 and round(float(a[i, 0, 0, 2]) * 255) == (30 + k % 4 - 24) // 2
    with pytest.raises(ValueError, match=r"_0\.png.*smaller than the crop 21x24"):
        list(D.load_batches(lst, crop=(21, 24), **kw))


def test_sample_order_and_augmentation_draws_do_not_depend_on_the_crop(tmp_path, monkeypatch):
    """Equal-sized samples: without a crop the order is today's (the permutation draws restated), and under 'selflow' the
    augmentation tables are the same with and without a crop, while the windows are the same with and without augmentation."""
    from PIL import Image
    from src import data_augmentation as DA, flowlib
    D = host_loader(monkeypatch)
    rows = []
    for k in range(5):
        yy, xx = np.mgrid[0:20, 0:30]
        for j in (0, 1):
            Image.fromarray(np.stack([np.full((20, 30), 10 * k + j), yy, xx], -1).astype(np.uint8)).save(
                str(tmp_path / ("%d_%d.ppm" % (k, j))))
        flowlib.write_flow(np.zeros((20, 30, 2), np.float32), str(tmp_path / ("%d.flo" % k)))
        rows.append("%s %s %s\n" % (tmp_path / ("%d_0.ppm" % k), tmp_path / ("%d_1.ppm" % k), tmp_path / ("%d.flo" % k)))
    lst = tmp_path / "l.txt"
    lst.write_text("".join(rows))
    plain = list(D.load_batches(str(lst), 2, data_augmentation=False, seed=7, epochs=3))
    ref = np.random.default_rng(7)
    want = [[int(v) for v in ref.permutation(5)[:4]] for _ in range(3)]
    assert sum(sample_ids(plain), []) == sum(want, [])
    assert all(tuple(a.shape) == (2, 20, 30, 3) and f.dtype.is_floating_point for a, _, f in plain)
    seen = []

    def record(image1, image2, gt_flow, params=None, **kw):
        seen.append((image1.copy(), params[0].copy(), params[1].copy()))
        return image1, image2, gt_flow

    monkeypatch.setattr(DA, "augment_all_estimation", record)
    list(D.load_batches(str(lst), 2, seed=7, epochs=2, augmentation="selflow"))
    uncropped, seen[:] = list(seen), []
    list(D.load_batches(str(lst), 2, seed=7, epochs=2, augmentation="selflow", crop=(16, 24)))
    cropped = list(seen)
    windows_no_aug = [np.round(a[:, 0, 0, 1:].numpy() * 255) for a, _, _ in
                      D.load_batches(str(lst), 2, data_augmentation=False, seed=7, epochs=2, crop=(16, 24))]
    assert len(uncropped) == len(cropped) == len(windows_no_aug) == 4
    for (ia, ta, tb), (ic, tc, td), wn in zip(uncropped, cropped, windows_no_aug):
        np.testing.assert_array_equal(ta, tc)
        np.testing.assert_array_equal(tb, td)
        np.testing.assert_array_equal(ia[:, 0, 0, 0], ic[:, 0, 0, 0])     # the same samples
        np.testing.assert_array_equal(np.round(ic[:, 0, 0, 1:] * 255), wn)   # the same windows
    assert len({tuple(w.reshape(-1)) for w in windows_no_aug}) > 1


def test_loader_refusals_come_before_any_file_or_device(tmp_path):
    from src import dataloader as D
    missing = str(tmp_path / "missing.txt")
    for kw, word in ((dict(sparse_gt=True), "plugin augmentation"), (dict(sparse_gt=True, augmentation="plugin"), "plugin"),
                     (dict(crop=(8, 8)), "own crop"), (dict(crop=(8, 8), data_augmentation=False, crop_mode="middle"), "crop_mode"),
                     (dict(crop=(8,), data_augmentation=False), "crop must be")):
        with pytest.raises(ValueError, match=word):
            next(D.load_batches(missing, 1, **kw))
    for kw, word in ((dict(sparse_gt=True), "dense"), (dict(crop=(8, 8)), "share one size")):
        with pytest.raises(ValueError, match=word):
            next(D.load_batches(str(tmp_path / "x.tfrecords"), 1, data_augmentation=False, **kw))
    sig = inspect.signature(D.load_batches).parameters
    assert (sig["sparse_gt"].default, sig["crop"].default, sig["crop_mode"].default) == (False, None, "random")
