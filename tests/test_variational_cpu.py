"""Variational refinement without a GPU: the fixture file, the parameter tables against the reference binary's
values, the dataset argument of calc_variational_inference_map, the interp CLI flag and the no-CPU-path error."""
import os

import numpy as np
import pytest
import torch

CASES = ["full", "crop", "crop_net", "crop_o1s1", "crop_o1s30", "crop_kitti"]


def test_fixture_holds_every_case_with_finite_data(golden_dir):
    with np.load(os.path.join(golden_dir, "variational_golden.npz")) as z:
        assert list(z["cases"]) == CASES
        assert tuple(z["crop"]) == (100, 130, 190, 254) and int(z["grid_step"]) == 4
        # outputs on every 4th row / column plus the last ones: 384x512 -> 97x129, 190x254 -> 49x65
        for name in CASES:
            out = z[name + "_out"]
            shape = (97, 129, 2) if name == "full" else (49, 65, 2)
            assert out.shape == shape and out.dtype == np.float32 and np.isfinite(out).all()
            assert z[name + "_params"].shape == (8,)
        assert z["full_q"].shape == (384, 512, 2) and z["full_q"].dtype == np.int8
        assert z["crop_q"].shape == (190, 254, 2) and z["crop_q"].dtype == np.int8
        for q in (z["full_q"], z["crop_q"]):  # N(0, 0.75 px) in half pixels
            assert 1.25 < float(q.astype(np.float64).std()) < 1.75
        assert z["crop_net_init"].shape == (190, 254, 2) and np.isfinite(z["crop_net_init"]).all()
        assert z["crop_kitti_params"][4] == 2 and abs(z["crop_kitti_params"][3] - 1.7) < 1e-6
        assert os.path.getsize(os.path.join(golden_dir, "variational_golden.npz")) < 600_000


def test_fixture_outputs_move_the_init_but_not_far(golden_dir):
    from src.flowlib import read_flow
    gt = read_flow(os.path.join(golden_dir, "samples", "0flow.flo")).astype(np.float32)
    with np.load(os.path.join(golden_dir, "variational_golden.npz")) as z:
        init = gt + z["full_q"].astype(np.float32) * np.float32(0.5)
        grid = init[np.unique(np.r_[np.arange(0, 384, 4), 383])][:, np.unique(np.r_[np.arange(0, 512, 4), 511])]
        d = float(np.abs(z["full_out"] - grid).mean())
        assert 0.05 < d < 5.0, d


def test_defaults_and_presets_are_the_binary_values():
    from src import variational as V
    # variational.c:85-98
    assert V.DEFAULTS == dict(alpha=1.0, gamma=0.71, delta=0.0, sigma=1.0, niter_outer=5, niter_inner=1,
                              niter_solver=30, sor_omega=1.9)
    # variational_main.cpp:63-84
    assert V.PRESETS["sintel"] == dict(niter_outer=5, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1)
    assert V.PRESETS["kitti"] == dict(niter_outer=2, alpha=1.0, gamma=0.77, delta=0.0, sigma=1.7)
    assert V.PRESETS["middlebury"] == dict(niter_outer=25, alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1)
    p = V.params_for("kitti", niter_solver=10)
    assert p["niter_outer"] == 2 and p["sigma"] == 1.7 and p["niter_solver"] == 10 and p["sor_omega"] == 1.9
    assert V.params_for(None) == V.DEFAULTS
    with pytest.raises(ValueError):
        V.params_for("sintel2")
    with pytest.raises(TypeError):
        V.params_for(None, beta=2.0)
    with pytest.raises(ValueError):
        V.params_for(None, niter_outer=-1)
    with pytest.raises(ValueError):
        V.params_for(None, sigma=0.0)


@pytest.mark.parametrize("dataset", ["sintel", "kitti", "middlebury", "", "anything"])
def test_dataset_argument_maps_to_defaults(dataset):
    from src import variational as V
    assert V.binary_params(dataset) == V.DEFAULTS


def test_interp_cli_parses_variational_refinement():
    from src.flownet_s_interp.test import build_parser
    base = ["--input_a", "a.png", "--matches_a", "m.png", "--sparse_flow", "s.flo", "--out", "o"]
    p = build_parser()
    assert p.parse_args(base).variational_refinement is False
    assert p.parse_args(base + ["--variational_refinement", "true"]).variational_refinement is True
    assert p.parse_args(base + ["--variational_refinement", "0"]).variational_refinement is False
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--variational_refinement", "maybe"])


def test_refine_on_cpu_tensors_raises_clear_error():
    from src.variational import refine
    flow = torch.zeros(8, 12, 2)
    img = torch.zeros(8, 12, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ROCm device"):
        refine(flow, img, img)
    with pytest.raises(TypeError):
        refine(flow.numpy(), img, img)


def test_net_signatures_take_the_flag():
    import inspect
    from src.net import Net
    sig = inspect.signature(Net.test)
    assert list(sig.parameters)[-1] == "variational_refinement"
    assert sig.parameters["variational_refinement"].default is False
    assert inspect.signature(Net.test_batch).parameters["variational_refinement"].default is False
