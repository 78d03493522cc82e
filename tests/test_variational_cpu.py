"""Variational refinement without a GPU: the fixture file, the parameter tables against the reference binary's
values, the dataset argument of calc_variational_inference_map, the interp CLI flag and the no-CPU-path error."""
import os
import sys

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


# variational_edges_golden.npz: case -> (H, W) and the parameters that differ from the defaults
EDGE_CASES = {
    "delta": ((48, 64), dict(delta=0.5, niter_outer=2)),
    "delta_only": ((48, 64), dict(delta=1.0, gamma=0.0, niter_outer=2)),
    "inner2": ((48, 64), dict(niter_inner=2, niter_outer=2, niter_solver=10)),
    "inner3": ((48, 64), dict(niter_inner=3, niter_outer=1, niter_solver=5)),
    "sig03": ((48, 64), dict(sigma=0.3, niter_outer=1)),
    "sig066": ((48, 64), dict(sigma=0.66, niter_outer=1)),
    "sig3": ((48, 64), dict(sigma=3.0, niter_outer=2)),
    "sig10": ((63, 63), dict(sigma=10.0, niter_outer=2)),
    "min9": ((9, 9), dict(niter_outer=2)),
    "w2": ((33, 2), dict(sigma=0.3, niter_outer=1)),
    "w3": ((33, 3), dict(sigma=0.3, niter_outer=1)),
    "w4": ((33, 4), dict(sigma=0.5, niter_outer=1)),
    "h4": ((4, 33), dict(sigma=0.5, niter_outer=1)),
    "h5": ((5, 33), dict(sigma=0.5, niter_outer=1)),
    "col": ((40, 1), dict(sigma=0.3, niter_outer=2, niter_solver=10)),
    "h600": ((600, 12), dict(niter_outer=2)),
    "tall": ((1100, 12), dict(niter_outer=2)),
    "far": ((48, 64), dict(niter_outer=2)),
    "omega1": ((48, 64), dict(sor_omega=1.0, niter_outer=2)),
    "alpha3": ((48, 64), dict(alpha=3.0, niter_outer=2)),
    "far_edge": ((48, 64), dict(niter_outer=1)),  # not in the issue's table: `far` with ten inits ON the border
}
EDGE_SPREAD_CAP = 1e-3  # px


def _edges_generator(golden_dir):
    if golden_dir not in sys.path:
        sys.path.insert(0, golden_dir)
    import make_golden_variational_edges as gen
    return gen


def test_edges_fixture_holds_the_table_with_finite_well_conditioned_data(golden_dir):
    from src import variational as V
    path = os.path.join(golden_dir, "variational_edges_golden.npz")
    assert os.path.getsize(path) < 600_000
    keys = ("alpha", "gamma", "delta", "sigma", "niter_outer", "niter_inner", "niter_solver", "sor_omega")
    with np.load(path) as z:
        assert list(z["cases"]) == list(EDGE_CASES)
        assert [tuple(s) for s in z["shapes"]] == [v[0] for v in EDGE_CASES.values()]
        assert tuple(z["origin"]) == (100, 130)
        for k in z.files:
            if z[k].dtype.kind in "fi":
                assert np.isfinite(z[k]).all(), k
        for name, (shape, over) in EDGE_CASES.items():
            out = z[name + "_out"]  # the full pixel grid
            assert out.shape == shape + (2,) and out.dtype == np.float32
            want = dict(V.DEFAULTS, **over)
            assert z[name + "_params"].tolist() == [float(want[k]) for k in keys], name
            q = z["q_%dx%d" % shape]
            assert q.shape == shape + (2,) and q.dtype == np.int8
        assert z["far_off"].shape == (48, 64, 2) and z["far_off"].dtype == np.int8
        assert int((np.abs(z["far_off"].astype(int)) >= 59).sum()) > 48 * 64 * 2 // 3  # about half are +-30 px
        for name in list(EDGE_CASES) + ["crop"]:
            s = z[name + "_spread"]
            assert s.shape == (3,) and (s >= 0).all() and s[0] <= s[1] <= s[2], name
        for name in EDGE_CASES:  # the yardstick `crop` is not stored here and not held to the cap
            assert z[name + "_spread"][2] <= EDGE_SPREAD_CAP, name


def test_edges_generator_tables_and_input_helper(golden_dir):
    gen = _edges_generator(golden_dir)
    from src import variational as V
    assert gen.CASE_NAMES == list(EDGE_CASES) and gen.SPREAD_CAP == EDGE_SPREAD_CAP
    for name, (shape, over) in EDGE_CASES.items():
        assert gen.case_params(name) == dict(V.DEFAULTS, **over), name
    samples = gen.load_samples(os.path.join(golden_dir, "samples"))
    with np.load(os.path.join(golden_dir, gen.FIXTURE)) as z:
        arrays = {k: z[k] for k in z.files}
    for name, (shape, _) in EDGE_CASES.items():
        a, b, init, p = gen.case_inputs(name, samples, arrays)
        assert a.shape == b.shape == shape + (3,) and a.dtype == b.dtype == np.uint8, name
        assert init.shape == shape + (2,) and init.dtype == np.float32 and np.isfinite(init).all(), name
    # tall: the 12-column strips at x = 100, 250, 400 stacked vertically; rows 384.. come from the second strip
    a, b, init, _ = gen.case_inputs("tall", samples, arrays)
    assert np.array_equal(a[:384], samples[0][:, 100:112]) and np.array_equal(a[384:768], samples[0][:, 250:262])
    assert np.array_equal(b[768:], samples[1][:332, 400:412])
    gt = np.concatenate([samples[2][:, x:x + 12] for x in (100, 250, 400)])[:1100]
    assert np.array_equal(init, gt + arrays["q_1100x12"].astype(np.float32) * np.float32(0.5))
    # far: the 48x64 crop's init moved by +-30 px in about half of its components
    _, _, base, _ = gen.case_inputs("delta", samples, arrays)
    a, _, far, _ = gen.case_inputs("far", samples, arrays)
    assert np.array_equal(a, samples[0][100:148, 130:194])
    assert np.array_equal(far - base, arrays["far_off"].astype(np.float32) * np.float32(0.5))
    moved = np.abs(far - base) > 29
    assert 0.35 < float(moved.mean()) < 0.65
    # no init points exactly at the frame's border, where the reference's in-image mask switches ...
    on_border = {}
    for name, (shape, _) in EDGE_CASES.items():
        init = gen.case_inputs(name, samples, arrays)[2]
        jj, ii = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float32)
        xx, yy = ii + init[..., 0], jj + init[..., 1]
        inside = (xx >= 0) & (xx <= shape[1] - 1) & (yy >= 0) & (yy <= shape[0] - 1)
        on_border[name] = [(xx == shape[1] - 1) & inside, (xx == 0) & inside, (yy == shape[0] - 1) & inside,
                           (yy == 0) & inside]
        if name != "far_edge":
            assert not np.any(on_border[name]), name
    # ... but far_edge's pinned pixels, which are `far` elsewhere: each points at the last column, the first column,
    # the last row or the first row with its other coordinate inside, so the mask's `<=` alone decides it
    pins = gen.edge_pins((48, 64))
    assert int(pins.sum()) == len(gen.EDGE_PINS) == 10
    assert [int(m.sum()) for m in on_border["far_edge"]] == [4, 2, 2, 2]
    assert np.array_equal(np.any(on_border["far_edge"], 0), pins)
    edge = gen.case_inputs("far_edge", samples, arrays)[2]
    assert np.array_equal(edge[~pins], far[~pins])


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
