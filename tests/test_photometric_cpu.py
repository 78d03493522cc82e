"""The occlusion-aware photometric loss without a GPU: the float64 twin checked against torch autograd of its own forward
and against a case worked by hand, the preconditions of the GPU tests, the exported symbols, and every argument check of
the library, the wrapper, the trainer, the list reader and the CLI that has to come before any device use."""
import ctypes as C
import os

import numpy as np
import pytest

import photometric_twin as twin
from test_gpu_photometric_train import BAND_CAP, CONFIGS, FRAME_SEED, IDS, frames, level_scale, slots, twin_levels
from test_gpu_photometric import (SCALES, SHAPES, check_invalid_arguments, margin_ok, poisoned_case, quirk_case, reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("shape,scale", [((2, 5, 7), 1.0), ((4, 6, 9), 0.625), ((2, 3, 70), 5.0)])
def test_twin_gradient_is_autograd_of_its_forward(shape, scale):
    """Random (non-dyadic) inputs: dL/dpred of torch_loss by autograd against the analytic formula, and the two forwards."""
    import torch
    n, h, w = shape
    rng = np.random.default_rng(5)
    img = rng.random((n, h, w, 3))
    pred = (rng.standard_normal((n, h, w, 2)) * 1.2 / scale).astype(np.float32)
    mask, parts = twin.masks(pred, scale)
    assert mask.any() and not mask.all() and parts["occ"].any() and not parts["valid"].all()
    L, g, _ = twin.loss_and_grad(img, pred, mask, scale, weight=0.064, q=0.4, grad_mult=3.0)
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    Lt = twin.torch_loss(img, p, mask, scale, weight=0.064, q=0.4)
    Lt.backward()
    assert abs(float(Lt.detach()) - L) <= 1e-12 * abs(L)
    np.testing.assert_allclose(3.0 * p.grad.numpy(), g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    assert not g[~mask].any() and np.abs(g[mask]).min() > 0


def test_twin_on_a_case_worked_by_hand():
    """2 slots of 2 x 3.  Partner frame B[y][x] = [[0, .25, .5], [1, 1.25, 1.5]] in channel 0, twice that in channel 1, 0 in
    channel 2; own frame 0.  scale 2, pred (.25, .25) at pixel (0, 0) of slot 0, 0 elsewhere.  Valid pixels: row 0, columns 0
    and 1 of either slot (X < 2, Y < 1); none occluded (|f|^2 = .5 <= .505), so M = 4.
      slot 0 (0,0): X = Y = .5, four weights of 1/4: warp = (.625, 1.25, 0), d = -warp;
                    d warp/dX = .5 (.25 - 0) + .5 (1.25 - 1) = .25 (x2 in channel 1), d warp/dY = .5 (1) + .5 (1) = 1 (x2)
      slot 0 (0,1): X = 1, Y = 0, weight 1 on B[0][1]: d = (-.25, -.5, 0); d warp/dX = B[0][2] - B[0][1] = .25 (x2),
                    d warp/dY = B[1][1] - B[0][1] = 1 (x2)
      slot 1: the partner frame is 0, so warp = 0 and every tap difference is 0: d = own value, gradient 0."""
    q, wgt, gm, s = 0.4, 0.064, 16384.0, 2.0
    B = np.array([[0, .25, .5], [1, 1.25, 1.5]])
    img = np.zeros((2, 2, 3, 3))
    img[1, :, :, 0], img[1, :, :, 1] = B, 2 * B
    pred = np.zeros((2, 2, 3, 2), np.float32)
    pred[0, 0, 0] = (0.25, 0.25)
    mask, parts = twin.masks(pred, s)
    want_mask = np.zeros((2, 2, 3), bool)
    want_mask[:, 0, :2] = True
    np.testing.assert_array_equal(mask, want_mask)
    np.testing.assert_array_equal(parts["X"][0, 0], np.float32([0.5, 1, 2]))
    L, g, d = twin.loss_and_grad(img, pred, mask, s, wgt, q, gm)
    np.testing.assert_array_equal(d[0, 0, 0], [-0.625, -1.25, 0])
    np.testing.assert_array_equal(d[0, 0, 1], [-0.25, -0.5, 0])
    psi = lambda v: (abs(v) + 0.01) ** q
    dpsi = lambda v: q * (abs(v) + 0.01) ** (q - 1)
    den = 2 * 4 + 1e-6
    total = (psi(.625) + psi(1.25) + psi(0)) + (psi(.25) + psi(.5) + psi(0)) + 3 * psi(0) + (psi(.25) + psi(.5) + psi(0))
    assert L == pytest.approx(wgt * total / den, rel=1e-14)
    k = gm * wgt * s / den
    want = np.zeros((2, 2, 3, 2))
    want[0, 0, 0] = (k * (dpsi(.625) * .25 + dpsi(1.25) * .5), k * (dpsi(.625) * 1 + dpsi(1.25) * 2))
    want[0, 0, 1] = (k * (dpsi(.25) * .25 + dpsi(.5) * .5), k * (dpsi(.25) * 1 + dpsi(.5) * 2))
    np.testing.assert_allclose(g, want, rtol=1e-14, atol=0)
    # a level without a valid pixel: loss and gradient exactly 0
    L0, g0, _ = twin.loss_and_grad(np.ones((2, 1, 1, 3)), np.zeros((2, 1, 1, 2)), twin.masks(np.zeros((2, 1, 1, 2)))[0])
    assert L0 == 0.0 and not g0.any()


@pytest.mark.parametrize("shape", SHAPES)
def test_preconditions_of_the_gpu_op_tests_hold(shape):
    """reference() asserts exactness; here also the margins with alpha = 0.01 for every case the GPU tests use, that fp32
    arithmetic in NumPy's order gives the same masks, and which shapes have no valid pixel."""
    from test_gpu_occlusion import occlusion_ref
    for scale in SCALES:
        pred, img, mask, parts, L, g = reference(0, shape, scale, 1.0 / 64)
        pred, img, mask, parts, L, g = reference(0, shape, scale, 0.01, 0.064, 1.0)
        assert margin_ok(parts) and reference(0, shape, scale, 0.01, 0.064, 16384.0)[5].shape == pred.shape
        f = parts["f"].astype(np.float32)
        f32 = occlusion_ref(f[0::2], f[1::2], np.float32(0.01), np.float32(0.5), np.float32)
        assert np.array_equal(f32[0][..., 0], parts["occ"][0::2]) and np.array_equal(f32[1][..., 0], parts["occ"][1::2])
        assert mask.any() == (shape in SHAPES[:3]) and (L == 0.0) == (not mask.any())
    for seed in (0, 1):
        _, _, mask, parts, _, _ = reference(seed, shape, 1.0, 0.01)
        assert margin_ok(parts)
        if shape in SHAPES[:3]:
            assert mask.any() and not mask.all() and parts["occ"].any()
    if shape in ((2, 5, 7), (4, 6, 130)):
        poisoned_case(shape)


def test_five_level_and_quirk_cases_hold_on_the_twin():
    for shp, s, wgt in zip([(4, 6, 130), (4, 3, 70), (4, 5, 7), (4, 2, 3), (4, 1, 2)], [5.0, 1.0, 0.625, 1.0, 5.0],
                           [0.064, 0.016, 0.004, 0.002, 0.001]):
        assert margin_ok(reference(3, shp, s, 0.01, wgt, 16384.0)[3])
    pred, img, want = quirk_case()
    mask, parts = twin.masks(pred)
    np.testing.assert_array_equal(mask[0], want.astype(bool))
    assert mask[1].any() and parts["occ"][1].any()                 # the partner slot sees the hand-placed flows as occlusions
    assert float((np.abs(parts["d"] - parts["t"]) / (1 + parts["t"])).min()) > 2.0 ** -18


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c[4] == "f32"], ids=[i for i in IDS if i.endswith("f32")])
def test_seeded_trainer_inputs_stay_inside_the_band_cap(cfg):
    """The GPU trainer tests on the CPU, with the oracle's predictions standing in for the engine's (they differ by fp32
    rounding): the band around the thresholds holds at most 1 % of the mask pixels, both mask values occur, and no unmasked
    residual lies at the kink of psi."""
    from oracle import models as refm
    from oracle import ops as refo
    from src import weights as W
    model, n, h, w, _ = cfg
    A, B = slots(*frames(n // 2, h, w, FRAME_SEED))
    out = refm.MODELS[model](W.init_weights(model, 1234), {"input_a": A, "input_b": B})
    preds = {k: np.asarray(out[k], np.float32) for k in ("predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3",
                                                         "predict_flow2")}
    lv = twin_levels(model, w, preds)
    in_band = sum(int(band.sum()) for _, _, band in lv.values())
    total = sum(band.size for _, _, band in lv.values())
    print("%s: %d of %d mask pixels in the band; unmasked share per level %s"
          % (cfg, in_band, total, ["%.2f" % m.mean() for m, _, _ in lv.values()]))
    assert in_band <= BAND_CAP * total
    assert any(m.any() and not m.all() for m, _, _ in lv.values())
    for name, (mask, _, _) in lv.items():
        if min(mask.shape[1:3]) == 1:                              # a 1-high level: nothing valid, its frames are never formed
            assert not mask.any()
            continue
        img = np.asarray(refo.downsample(A, list(mask.shape[1:3])), np.float32)
        d = twin.loss_and_grad(img, preds[name], mask, level_scale(model, mask.shape[2], w))[2]
        assert not mask.any() or np.abs(d[mask]).min() > 1e-6


# ------------------------------------------------------------------------------------------------ the library
@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


def test_entry_points_are_exported_declared_and_validate_without_a_device(hip):
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    for name in ("fn2_photometric_masks", "fn2_photometric_loss_grad"):
        assert name in hip.PROTOTYPES and hasattr(lib, name) and ("int %s(" % name) in header
    assert "utils.py:354-395" in header and "utils.py:453-538" in header
    check_invalid_arguments(hip)


def test_level_struct_matches_the_header_layout(hip):
    """fn2_photometric_level: five pointers, two int32, two floats: 56 bytes."""
    L = hip.Fn2PhotometricLevel
    assert C.sizeof(L) == 56 and (L.h.offset, L.w.offset, L.scale.offset, L.weight.offset) == (40, 44, 48, 52)


# ------------------------------------------------------------------------------------------------ Python surface
def test_wrapper_rejects_bad_arguments_before_touching_a_device(monkeypatch):
    import torch
    from src import _hip, photometric
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was asked for"))
    img, pred = torch.zeros(2, 4, 5, 3), torch.zeros(2, 4, 5, 2)
    with pytest.raises(ValueError, match="device tensor"):
        photometric.photometric_loss(img, pred)
    with pytest.raises(ValueError, match="device tensor"):
        photometric.photometric_loss(img.numpy(), pred.numpy())
    z = torch.zeros
    for i, p, word in ((z(4, 5, 3), z(4, 5, 2), "rank 4"), (z(2, 4, 5, 2), z(2, 4, 5, 2), "3 channels"),
                       (z(2, 4, 5, 3), z(2, 4, 5, 3), "2 channels"), (z(2, 4, 5, 3), z(2, 4, 6, 2), "same batch"),
                       (z(3, 4, 5, 3), z(3, 4, 5, 2), "even"), (z(2, 0, 5, 3), z(2, 0, 5, 2), "empty")):
        with pytest.raises(ValueError, match=word):
            photometric.photometric_loss(i, p)
    for bad in (dict(q=0.0), dict(q=1.5), dict(q=float("nan")), dict(alpha=-0.1), dict(beta=float("nan"))):
        with pytest.raises(ValueError):
            photometric.check_constants(**dict(dict(alpha=0.01, beta=0.5, q=0.4), **bad))
    assert photometric.check_constants(0.01, 0.5, 0.4) == (0.01, 0.5, 0.4)


def test_trainer_arguments_are_checked_before_the_engine_is_built(monkeypatch):
    from src import trainer
    monkeypatch.setattr(trainer, "Engine", lambda *a, **k: pytest.fail("the engine was asked for"))
    make = lambda **kw: trainer.FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128, unsupervised=True), **kw))
    for kw, word in ((dict(batch=3), "even"), (dict(model="FlowNet2"), "FlowNet2"), (dict(model="FlowNetS_interp"), "interp"),
                     (dict(add_hard_flow_mining="hard"), "mining"), (dict(add_hard_flow_mining="edges"), "mining"),
                     (dict(photometric_q=0.0), "q must"), (dict(occ_alpha=-1.0), ">= 0")):
        with pytest.raises(ValueError, match=word):
            make(**kw)
    import inspect
    sig = inspect.signature(trainer.FlowNetSTrainer.__init__).parameters
    assert sig["unsupervised"].default is False and (sig["photometric_q"].default, sig["occ_alpha"].default,
                                                     sig["occ_beta"].default) == (0.4, 0.01, 0.5)


def test_supervised_and_unsupervised_steps_do_not_mix():
    from src.trainer import FlowNetSTrainer
    tr = object.__new__(FlowNetSTrainer)                            # the mode check comes first: nothing else is looked at
    tr.unsupervised = True
    for call in (lambda: tr.train_step(None, None, None), lambda: tr.forward_backward(None, None, None)):
        with pytest.raises(ValueError, match="supervised"):
            call()
    tr.unsupervised = False
    for call in (lambda: tr.train_step_unsupervised(None, None), lambda: tr.forward_backward_unsupervised(None, None)):
        with pytest.raises(ValueError, match="unsupervised"):
            call()


def test_read_list_takes_two_fields_only_when_asked(tmp_path):
    from src.dataloader import load_batches, read_list
    two, three, mixed = tmp_path / "two.txt", tmp_path / "three.txt", tmp_path / "mixed.txt"
    two.write_text("a.ppm b.ppm\n\nc.ppm d.ppm\n")
    three.write_text("a.ppm b.ppm f.flo\n")
    mixed.write_text("a.ppm b.ppm f.flo\nc.ppm d.ppm\n")
    assert read_list(str(three)) == [["a.ppm", "b.ppm", "f.flo"]]
    with pytest.raises(ValueError, match="image_a image_b flow.flo"):
        read_list(str(two))
    with pytest.raises(ValueError):
        read_list(str(mixed))
    assert read_list(str(two), allow_unlabeled=True) == [["a.ppm", "b.ppm"], ["c.ppm", "d.ppm"]]
    assert len(read_list(str(mixed), allow_unlabeled=True)) == 2
    bad = tmp_path / "bad.txt"
    bad.write_text("a.ppm\n")
    with pytest.raises(ValueError):
        read_list(str(bad), allow_unlabeled=True)
    with pytest.raises(ValueError, match="data_augmentation=False"):
        next(load_batches(str(two), 1, allow_unlabeled=True))      # both augmentations transform a ground truth
    with pytest.raises(ValueError, match="image_a image_b flow.flo"):
        next(load_batches(str(two), 1, data_augmentation=False))   # the default still wants three fields


@pytest.mark.parametrize("model", ["flownet_s", "flownet_sd", "flownet_c", "flownet_cs", "flownet_css"])
def test_cli_flags_and_their_checks(model, tmp_path):
    import importlib
    from src.flownet_s import train as cli
    mod = importlib.import_module("src.%s.train" % model)
    assert mod.parse_and_run is cli.parse_and_run                  # one CLI for the five models
    base = ["--list", "l.txt", "--out", str(tmp_path)]
    flags = cli.build_parser().parse_args(base)
    assert flags.unsupervised is False and (flags.photometric_q, flags.occ_alpha, flags.occ_beta) == (0.4, 0.01, 0.5)
    assert cli.unsupervised_kwargs(flags) == {}
    flags = cli.build_parser().parse_args(base + ["--unsupervised", "--no-augment", "--photometric_q", "0.5", "--occ_alpha",
                                                  "0.02", "--occ_beta", "1", "--batch", "4"])
    assert cli.unsupervised_kwargs(flags) == dict(unsupervised=True, photometric_q=0.5, occ_alpha=0.02, occ_beta=1.0)
    flags = cli.build_parser().parse_args(base + ["--unsupervised"])
    with pytest.raises(ValueError, match="brightness constancy"):
        cli.main(flags)                                            # raised before torch or the device are touched
    assert not os.listdir(str(tmp_path))
    with pytest.raises(ValueError, match="even"):
        cli.main(cli.build_parser().parse_args(base + ["--unsupervised", "--no-augment", "--batch", "3"]))
    with pytest.raises(ValueError, match="q must"):
        cli.main(cli.build_parser().parse_args(base + ["--unsupervised", "--no-augment", "--photometric_q", "0"]))
