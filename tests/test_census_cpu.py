"""The ternary census data term without a GPU: the float64 twin checked against torch autograd of its own forward and
against a level worked by hand, the preconditions of the GPU tests, the exported symbols, and every argument check of the
library, the wrapper, the trainer and the CLI that has to come before any device use."""
import ctypes as C
import os

import numpy as np
import pytest

import census_twin as twin
from test_gpu_census import SCALES, SHAPES, check_invalid_arguments, poisoned_case, reach, reference, warp_exact_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize("shape,scale", [((2, 7, 7), 1.0), ((2, 8, 11), 0.625), ((2, 9, 14), 5.0)])
def test_twin_gradient_is_autograd_of_its_forward(shape, scale):
    """Random (non-dyadic) inputs and a random mask: dL/dpred of torch_loss by autograd against the scattered analytic
    gradient, and the two forwards."""
    import torch
    n, h, w = shape
    rng = np.random.default_rng(5)
    img = rng.random((n, h, w, 3)).astype(np.float32)
    pred = (rng.standard_normal((n, h, w, 2)) * 0.8 / scale).astype(np.float32)
    pred[:, h // 2, w // 2] = 0.25 / scale
    mask = (rng.random((n, h, w)) > 0.2).astype(np.float32)
    mask[:, h // 2, w // 2] = 1
    L, g, parts = twin.loss_and_grad(img, pred, mask, scale, weight=0.064, q=0.4, grad_mult=3.0)
    assert parts["Mc"] >= 1 and not parts["V"].all()
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    Lt = twin.torch_loss(img, p, mask, scale, weight=0.064, q=0.4)
    Lt.backward()
    assert abs(float(Lt.detach()) - L) <= 1e-12 * abs(L)
    np.testing.assert_allclose(3.0 * p.grad.numpy(), g, rtol=1e-9, atol=1e-12 * np.abs(g).max())
    assert np.abs(g).max() > 0 and not g[~parts["V"]].any() and not g[~reach(parts["mc"])].any()


def test_twin_on_a_level_worked_by_hand():
    """2 slots of 7 x 7, zero flow, scale 2: X = x, Y = y, every tap weight is 1 on the pixel itself, V = (x < 6 and y < 6),
    one interior pixel q = (3, 3) per slot, Mc = 2.  Slot 0 is a uniform frame, rgb = (.25, .25, .125): G = .625 * 85 =
    53.125; slot 1 is black but for pixel (2, 2) = (.5, .25, .25): G = 85.
      slot 0: a = 0 for every d (uniform frame); W = slot 1's G, so b = n(85) at d = (-1, -1) and 0 elsewhere:
              S = e / (0.1 + e), e = n(85)^2, n(85) = 85 / sqrt(0.81 + 7225)
              DX(y, x) = G1(y, x+1) - G1(y, x), DY(y, x) = G1(y+1, x) - G1(y, x): (DX, DY) = (-85, -85) at (2, 2).
              The one live term pushes on W(2, 2) with c k and pulls on W(3, 3) with -c k; DX = DY = 0 at (3, 3), so the
              gradient is dpred(2, 2) = coef * c * k * (-85, -85) and 0 at every other pixel.
      slot 1: a = n(85) at d = (-1, -1); W = slot 0's uniform grey, b = 0: the same e and S; DX = DY = 0 everywhere, gradient 0."""
    q, wgt, gm, s = 0.4, 0.064, 16384.0, 2.0
    img = np.zeros((2, 7, 7, 3), np.float32)
    img[0] = (0.25, 0.25, 0.125)                                   # G = 0.625 * 85 = 53.125
    img[1, 2, 2] = (0.5, 0.25, 0.25)
    pred = np.zeros((2, 7, 7, 2), np.float32)
    L, g, parts = twin.loss_and_grad(img, pred, None, s, wgt, q, gm)
    assert parts["G"][0, 0, 0] == 53.125 and parts["G"][1, 2, 2] == 85.0 and parts["G"][1].sum() == 85.0
    want_V = np.zeros((7, 7), bool)
    want_V[:6, :6] = True
    np.testing.assert_array_equal(parts["V"], np.stack([want_V, want_V]))
    np.testing.assert_array_equal(parts["mc"].nonzero(), ([0, 1], [3, 3], [3, 3]))
    assert parts["Mc"] == 2
    n85 = 85.0 / np.sqrt(0.81 + 85.0 ** 2)
    e = n85 ** 2
    S = e / (0.1 + e)
    np.testing.assert_allclose(parts["S"][:, 3, 3], [S, S], rtol=1e-14)
    assert np.count_nonzero(parts["S"]) == 2
    den = 2 * 2 + 1e-6
    assert L == pytest.approx(wgt * 2 * (S + 0.01) ** q / den, rel=1e-14)
    c = q * (S + 0.01) ** (q - 1)
    k = (-2 * (0 - n85) * 0.1 / (0.1 + e) ** 2) * 0.81 / (0.81 + 85.0 ** 2) ** 1.5
    want = np.zeros((2, 7, 7, 2))
    want[0, 2, 2] = gm * wgt * s / den * c * k * np.array([-85.0, -85.0])
    np.testing.assert_allclose(g, want, rtol=1e-13, atol=0)
    assert g[0, 2, 2, 0] < 0                                       # moving the sample off the bright pixel lowers the distance
    # a masked interior pixel: nothing is counted, loss and gradient exactly 0
    mask = np.ones((2, 7, 7), np.float32)
    mask[:, 3, 3] = 0
    L0, g0, p0 = twin.loss_and_grad(img, pred, mask, s, wgt, q, gm)
    assert L0 == 0.0 and not g0.any() and p0["Mc"] == 0


@pytest.mark.parametrize("shape", [(2, 6, 9), (2, 9, 6), (2, 1, 1), (4, 5, 40)])
def test_a_level_without_an_interior_gives_zero(shape):
    n, h, w = shape
    rng = np.random.default_rng(3)
    img, pred = rng.random((n, h, w, 3)).astype(np.float32), rng.standard_normal((n, h, w, 2)).astype(np.float32)
    L, g, parts = twin.loss_and_grad(img, pred)
    assert L == 0.0 and not g.any() and parts["Mc"] == 0 and not parts["S"].any() and not twin.interior(h, w).any()
    import torch
    p = torch.tensor(pred.astype(np.float64), requires_grad=True)
    twin.torch_loss(img, p).backward()
    assert not p.grad.numpy().any()


@pytest.mark.parametrize("shape", SHAPES)
def test_preconditions_of_the_gpu_op_tests_hold(shape):
    """reference() asserts the exactness of G, W, DX, DY; here for every case the GPU tests use, with the counts they
    rely on."""
    for scale in SCALES:
        for gm in (1.0, 16384.0):
            pred, img, mask, L, g, parts = reference(0, shape, scale, 0.064, gm)
            assert (parts["Mc"] == 0) == (min(shape[1:]) < twin.PATCH) and (L == 0.0) == (parts["Mc"] == 0)
        assert reference(0, shape, scale)[5]["V"].any()
    if shape in ((2, 7, 7), (4, 10, 135), (2, 19, 9)):
        parts = reference(1, shape, 1.0, 1.0, 1.0, False)[5]
        assert parts["Mc"] == (parts["V"] & twin.interior(*shape[1:])[None]).sum() >= 1
    if shape in ((2, 8, 70), (4, 10, 135)):
        pred, img, mask, bad = poisoned_case(shape)
        L, g, parts = twin.loss_and_grad(img, pred, mask)
        assert warp_exact_ok(parts) and not parts["V"][bad].any() and parts["Mc"] >= 1 and np.isfinite(g).all()
        assert np.isfinite(L) and bad.sum() >= 6


def test_five_level_case_holds_on_the_twin():
    for shp, s, wgt in zip([(4, 10, 135), (4, 19, 9), (4, 8, 70), (4, 7, 7), (4, 6, 9)], [5.0, 1.0, 0.625, 1.0, 5.0],
                           [0.064, 0.016, 0.004, 0.002, 0.001]):
        parts = reference(3, shp, s, wgt, 16384.0)[5]
        assert (parts["Mc"] >= 1) == (min(shp[1:]) >= twin.PATCH)


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
    for name in ("fn2_census_warp", "fn2_census_cost", "fn2_census_grad"):
        assert name in hip.PROTOTYPES and hasattr(lib, name) and ("int %s(" % name) in header
    _i, _p, _f = C.c_int, C.c_void_p, C.c_float
    T = C.POINTER(hip.Fn2CensusLevel)
    assert hip.PROTOTYPES["fn2_census_warp"] == (_i, [T, _i, _i, _p])
    assert hip.PROTOTYPES["fn2_census_cost"] == (_i, [T, _i, _i, _f, _p, _p])
    assert hip.PROTOTYPES["fn2_census_grad"] == (_i, [T, _i, _i, _f, _p])
    assert "fn2_census_level" in header and "utils.py:378-395" in header
    check_invalid_arguments(hip)


def test_level_struct_matches_the_header_layout(hip):
    """fn2_census_level: nine pointers, two int32, two floats: 88 bytes; fn2_photometric_level is untouched."""
    L = hip.Fn2CensusLevel
    assert [f[0] for f in L._fields_] == ["pred", "img", "mask", "dpred", "grey", "warp", "valid", "coef", "count", "h", "w",
                                          "scale", "weight"]
    assert C.sizeof(L) == 88 and (L.count.offset, L.h.offset, L.w.offset, L.scale.offset, L.weight.offset) == (64, 72, 76, 80, 84)
    assert C.sizeof(hip.Fn2PhotometricLevel) == 56


# ------------------------------------------------------------------------------------------------ Python surface
def test_wrapper_rejects_bad_arguments_before_touching_a_device(monkeypatch):
    import torch
    from src import _hip, census
    monkeypatch.setattr(_hip, "lib", lambda: pytest.fail("the library was asked for"))
    img, pred = torch.zeros(2, 8, 9, 3), torch.zeros(2, 8, 9, 2)
    with pytest.raises(ValueError, match="device tensor"):
        census.census_loss(img, pred)
    with pytest.raises(ValueError, match="device tensor"):
        census.census_loss(img.numpy(), pred.numpy())
    with pytest.raises(ValueError, match="device tensor"):
        census.census_loss(img, pred, np.ones((2, 8, 9), np.float32))
    z = torch.zeros
    for i, p, word in ((z(8, 9, 3), z(8, 9, 2), "rank 4"), (z(2, 8, 9, 2), z(2, 8, 9, 2), "3 channels"),
                       (z(2, 8, 9, 3), z(2, 8, 9, 3), "2 channels"), (z(2, 8, 9, 3), z(2, 8, 10, 2), "same batch"),
                       (z(3, 8, 9, 3), z(3, 8, 9, 2), "even"), (z(2, 0, 9, 3), z(2, 0, 9, 2), "empty")):
        with pytest.raises(ValueError, match=word):
            census.census_loss(i, p)
    with pytest.raises(ValueError, match=r"mask .* must be"):
        census.census_loss(img, pred, z(2, 8, 8))
    assert (census.RADIUS, census.PATCH) == (twin.R, twin.PATCH) == (3, 7)
    for term, unsup in (("ssim", True), ("", True), (None, True), ("census", False)):
        with pytest.raises(ValueError, match="data_term"):
            census.check_data_term(term, unsup)
    assert census.check_data_term("census", True) == "census" and census.check_data_term("photometric", False) == "photometric"


def test_trainer_arguments_are_checked_before_the_engine_is_built(monkeypatch):
    import inspect
    from src import trainer
    monkeypatch.setattr(trainer, "Engine", lambda *a, **k: pytest.fail("the engine was asked for"))
    make = lambda **kw: trainer.FlowNetSTrainer({}, **dict(dict(batch=2, height=64, width=128), **kw))
    for kw, word in ((dict(unsupervised=True, data_term="ssim"), "data_term"), (dict(data_term="census"), "unsupervised=True"),
                     (dict(data_term="census", sparse_gt=True), "unsupervised=True"),
                     (dict(unsupervised=True, data_term="census", batch=3), "even"),
                     (dict(unsupervised=True, data_term="census", model="FlowNet2"), "FlowNet2"),
                     (dict(unsupervised=True, data_term="census", photometric_q=0.0), "q must")):
        with pytest.raises(ValueError, match=word):
            make(**kw)
    assert inspect.signature(trainer.FlowNetSTrainer.__init__).parameters["data_term"].default == "photometric"


def test_stage_for_picks_the_census_stage_only_when_asked():
    import types
    from src import loss_stages
    tr = lambda **kw: types.SimpleNamespace(**dict(dict(unsupervised=True, data_term="photometric", loss_terms={}), **kw))
    assert type(loss_stages.stage_for(tr())) is loss_stages.Photometric
    st = loss_stages.stage_for(tr(data_term="census"))
    assert type(st) is loss_stages.Census and st.kind == "census" and isinstance(st, loss_stages.Photometric)


@pytest.mark.parametrize("model", ["flownet_s", "flownet_sd", "flownet_c", "flownet_cs", "flownet_css"])
def test_cli_flag_and_its_checks(model, tmp_path):
    import importlib
    from src.flownet_s import train as cli
    mod = importlib.import_module("src.%s.train" % model)
    assert mod.parse_and_run is cli.parse_and_run                  # one CLI for the five models
    base = ["--list", "l.txt", "--out", str(tmp_path)]
    assert cli.build_parser().parse_args(base).data_term == "photometric"
    unsup = base + ["--unsupervised", "--no-augment"]
    assert "data_term" not in cli.unsupervised_kwargs(cli.build_parser().parse_args(unsup))
    assert "data_term" not in cli.unsupervised_kwargs(cli.build_parser().parse_args(unsup + ["--data_term", "photometric"]))
    flags = cli.build_parser().parse_args(unsup + ["--data_term", "census", "--smoothness_weight", "0.5"])
    assert cli.unsupervised_kwargs(flags) == dict(unsupervised=True, photometric_q=0.4, occ_alpha=0.01, occ_beta=0.5,
                                                  data_term="census", smoothness_weight=0.5, smoothness_order=1,
                                                  edge_lambda=150.0)
    with pytest.raises(ValueError, match="needs --unsupervised"):
        cli.main(cli.build_parser().parse_args(base + ["--data_term", "census"]))   # before torch or the device are touched
    with pytest.raises(ValueError, match="needs --unsupervised"):
        cli.main(cli.build_parser().parse_args(base + ["--no-augment", "--sparse_gt", "--data_term", "census"]))
    assert not os.listdir(str(tmp_path))
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--data_term", "ssim"])
