"""The forward-backward occlusion check without a GPU: the NumPy restatement of the reference's tf_warp that the GPU
tests compare against (test_gpu_occlusion.tf_warp_ref) checked independently, the preconditions of those tests, the CLI
flag, the argument checks of the two entry points and the list-level checks that come before any device use."""
import os

import numpy as np
import pytest

from test_gpu_occlusion import (LARGER, SHAPES, check_invalid_arguments, dyadic_flows, occlusion_exact_ok, occlusion_ref,
                                poisoned_case, quirk_cases, tf_warp_ref)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tf_warp_ref_agrees_with_grid_sample_in_the_interior():
    """Where the coordinate is >= 0 and all four taps are interior (x <= W - 2, y <= H - 2: no clamp acts), tf_warp is the
    ordinary bilinear sample -- torch's grid_sample with align_corners=True on pixel coordinates."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    n, h, w, c = 2, 13, 17, 3
    img = rng.standard_normal((n, h, w, c))
    flow = rng.uniform(-4, 4, (n, h, w, 2))
    gx, gy = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    x, y = gx[None] + flow[..., 0], gy[None] + flow[..., 1]
    inside = (x >= 0) & (y >= 0) & (np.floor(x) + 1 <= w - 1) & (np.floor(y) + 1 <= h - 1)
    assert 0.3 < inside.mean() < 0.95
    grid = torch.from_numpy(np.stack([2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1], -1))
    want = F.grid_sample(torch.from_numpy(img).permute(0, 3, 1, 2), grid, mode="bilinear", padding_mode="zeros",
                         align_corners=True).permute(0, 2, 3, 1).numpy()
    got = tf_warp_ref(img, flow)
    assert np.abs(got - want)[inside].max() < 1e-6
    assert np.abs(got - want)[~inside].max() > 1e-3        # ... and it is something else outside: the quirks below


def test_tf_warp_ref_quirk_rows_by_hand():
    img, flow, want = quirk_cases()
    np.testing.assert_array_equal(tf_warp_ref(img, flow), want)
    np.testing.assert_array_equal(tf_warp_ref(img, flow, np.float32).astype(np.float64), want)
    # a 1-wide and a 1-high image warp to exactly 0 whatever the flow
    for shape in ((2, 9, 1), (1, 1, 9), (1, 1, 1)):
        fw, _ = dyadic_flows(0, shape)
        assert not tf_warp_ref(np.ones(shape + (2,)), fw).any()


@pytest.mark.parametrize("shape", SHAPES)
def test_preconditions_of_the_gpu_tests_hold(shape):
    """What the GPU tests assert on their float64 reference before they compare: exactness, the margin to the threshold with
    the reference's constants, both mask values at the larger shapes -- and that fp32 arithmetic on these inputs, in
    NumPy's order, gives the float64 masks."""
    for seed in range(4):
        fw, bw = dyadic_flows(seed, shape)
        for alpha in (1.0 / 64, 0.01):
            want_fw, want_bw, parts = occlusion_ref(fw, bw, alpha, 0.5)
            occlusion_exact_ok(fw, bw, parts)
            f32 = occlusion_ref(fw, bw, np.float32(alpha), np.float32(0.5), np.float32)
            assert np.array_equal(f32[0], want_fw) and np.array_equal(f32[1], want_bw)
        d_fw, t_fw, d_bw, t_bw = parts[:4]
        assert min(float((np.abs(d_fw - t_fw) / (1 + t_fw)).min()), float((np.abs(d_bw - t_bw) / (1 + t_bw)).min())) > 2.0 ** -18
        if shape in LARGER:
            assert want_fw.any() and not want_fw.all() and want_bw.any() and not want_bw.all()
    if shape in ((2, 5, 7), (2, 6, 130)):
        poisoned_case(shape, 1.0 / 64, 0.5)


@pytest.mark.parametrize("model", ["flownet_s", "flownet_sd", "flownet_c", "flownet_cs", "flownet_css", "flownet2"])
def test_cli_accepts_occlusions(model):
    import importlib
    parser = importlib.import_module("src.%s.test" % model).build_parser()
    base = ["--input_a", "a.png", "--input_b", "b.png", "--out", "o"]
    assert parser.parse_args(base).occlusions is False
    assert parser.parse_args(base + ["--occlusions", "true"]).occlusions is True
    assert parser.parse_args(base + ["--occlusions", "no"]).occlusions is False
    assert parser.parse_args(base + ["--occlusions"]).occlusions is True
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--occlusions", "perhaps"])


def _net():
    from src.flownet_s.flownet_s import FlowNetS
    from src.net import Mode
    net = FlowNetS(mode=Mode.TEST)
    net.weights = {}  # (keeps a call that gets that far from building seeded weights)
    return net


def test_list_checks_come_before_any_device_use(tmp_path, monkeypatch):
    net = _net()
    monkeypatch.setattr(net, "engine", lambda *a, **k: pytest.fail("the engine was asked for"))
    lst = tmp_path / "l.txt"
    lst.write_text("a.png b.png\n")
    for kw in (dict(occlusions=True), dict(occlusions_for_metrics=True)):
        with pytest.raises(ValueError, match="image_matches"):
            net.test_batch(None, str(lst), str(tmp_path / "o"), input_type="image_matches", **kw)
        with pytest.raises(ValueError, match="even"):
            net.test_batch(None, str(lst), str(tmp_path / "o"), batch_size=3, **kw)
    with pytest.raises(ValueError, match="image_matches"):
        net.test(None, "a.png", matches_a_path="m.png", sparse_flow_path="s.flo", input_type="image_matches", occlusions=True)
    with pytest.raises(ValueError, match="even"):
        net._infer_pairs([["a.png", "b.png"]], 3, bidirectional=True)
    assert not (tmp_path / "o").exists()                       # refused before the log file was opened


def test_new_arguments_default_to_off():
    import inspect
    from src.net import Net
    for fn, names in ((Net.test, ("occlusions",)), (Net.test_batch, ("occlusions", "occlusions_for_metrics")),
                      (Net._infer_pairs, ("bidirectional",))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is False


def test_shape_rules_need_no_device():
    from src.occlusion import occlusion, tf_warp
    f = np.zeros((1, 4, 5, 2), np.float32)
    for bad_fw, bad_bw in ((f[0], f[0]), (f, f[:, :3]), (f[..., :1], f[..., :1])):
        with pytest.raises(ValueError):
            occlusion(bad_fw, bad_bw)
    with pytest.raises(ValueError):
        tf_warp(np.zeros((4, 5, 3), np.float32), f)
    with pytest.raises(ValueError):
        tf_warp(np.zeros((1, 4, 5, 3), np.float32), np.zeros((1, 4, 5, 3), np.float32))


@pytest.fixture(scope="module")
def hip():
    from src import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "flownet2-tf_amd", "csrc"), "-j4"], check=True)
    return _hip


def test_entry_points_are_exported_and_validate_without_a_device(hip):
    lib = hip.lib()
    header = open(os.path.join(ROOT, "include", "flownet2_hip.h")).read()
    for name in ("fn2_tf_warp_f32", "fn2_fb_occlusion"):
        assert name in hip.PROTOTYPES and hasattr(lib, name) and ("int %s(" % name) in header
    check_invalid_arguments(hip)   # host memory stands in for the pointers: every call is refused before a launch
