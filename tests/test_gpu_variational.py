"""EpicFlow variational refinement on the GPU (src/variational.py, fn2_variational_refine) against the reference
binary's outputs in tests/golden/variational_golden.npz (make_golden_variational.py; stored on a grid of every 4th
row and column plus the last ones), and its use by Net.test / Net.test_batch.  The solver keeps the reference's
lexicographic SOR order: a red-black sweep fails the EPE bounds."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ["full", "crop", "crop_net", "crop_o1s1", "crop_o1s30", "crop_kitti"]
MEAN_TOL, P999_TOL = 1e-4, 2e-3
PARAM_KEYS = ("alpha", "gamma", "delta", "sigma", "niter_outer", "niter_inner", "niter_solver", "sor_omega")


@pytest.fixture(scope="module")
def gold(golden_dir):
    """The fixture plus the committed sample frames and ground truth it was made from (see its generator)."""
    from src.flowlib import read_flow
    from src.net import imread
    with np.load(os.path.join(golden_dir, "variational_golden.npz")) as z:
        g = {k: z[k] for k in z.files}
    samples = os.path.join(golden_dir, "samples")
    a, b = imread(os.path.join(samples, "0img0.ppm")), imread(os.path.join(samples, "0img1.ppm"))
    gt = read_flow(os.path.join(samples, "0flow.flo")).astype(np.float32)
    y0, x0, h, w = (int(v) for v in g["crop"])
    crop = (slice(y0, y0 + h), slice(x0, x0 + w))
    g["full_img_a"], g["full_img_b"] = a, b
    g["crop_img_a"], g["crop_img_b"] = np.ascontiguousarray(a[crop]), np.ascontiguousarray(b[crop])
    g["full_init"] = init_from(gt, g["full_q"])
    g["crop_init"] = init_from(np.ascontiguousarray(gt[crop]), g["crop_q"])
    g["crop_net_init"] = g["crop_net_init"].astype(np.float32)
    return g


def init_from(gt, q):
    """make_golden_variational.init_from: ground truth + q / 2, one float32 rounding."""
    return gt.astype(np.float32) + q.astype(np.float32) * np.float32(0.5)


def on_grid(flow, step):
    """The pixels the fixture stores outputs for: every `step`-th row and column and the last ones."""
    h, w = flow.shape[:2]
    rows = np.unique(np.r_[np.arange(0, h, step), h - 1])
    cols = np.unique(np.r_[np.arange(0, w, step), w - 1])
    return flow[rows][:, cols]


def case_inputs(gold, name):
    frames = "full" if name == "full" else "crop"
    init = gold[(name if name in ("full", "crop_net") else frames) + "_init"]
    p = dict(zip(PARAM_KEYS, gold[name + "_params"].tolist()))
    for k in ("niter_outer", "niter_inner", "niter_solver"):
        p[k] = int(p[k])
    return gold[frames + "_img_a"], gold[frames + "_img_b"], init, p


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def epe_stats(got, want):
    e = np.sqrt(((got.astype(np.float64) - want) ** 2).sum(-1))
    return float(e.mean()), float(np.percentile(e, 99.9)), float(e.max())


@pytest.mark.parametrize("name", CASES)
def test_matches_reference_binary(gold, name):
    from src.variational import refine
    a, b, init, p = case_inputs(gold, name)
    got = refine(dev(init), dev(a), dev(b), **p).cpu().numpy()
    assert got.shape == init.shape and np.isfinite(got).all()
    mean, p999, mx = epe_stats(on_grid(got, int(gold["grid_step"])), gold[name + "_out"])
    print("%s: EPE vs reference mean %.2e  p99.9 %.2e  max %.2e px" % (name, mean, p999, mx))
    assert mean < MEAN_TOL and p999 < P999_TOL


def test_kitti_preset_is_the_binary_preset(gold):
    from src.variational import refine
    a, b, init, p = case_inputs(gold, "crop_kitti")
    got = refine(dev(init), dev(a), dev(b), preset="kitti").cpu().numpy()
    want = refine(dev(init), dev(a), dev(b), **p).cpu().numpy()
    assert np.array_equal(got, want)


def test_batch_equals_single_calls(gold):
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    net_init = gold["crop_net_init"]
    pairs = [(a, b, init), (a, b, net_init), (b, a, -init)]
    singles = [refine(dev(f), dev(x), dev(y)).cpu().numpy() for x, y, f in pairs]
    batch = refine(dev(np.stack([p[2] for p in pairs])), dev(np.stack([p[0] for p in pairs])),
                   dev(np.stack([p[1] for p in pairs]))).cpu().numpy()
    for i, s in enumerate(singles):
        assert np.array_equal(batch[i], s), i


def test_padded_frames_read_in_place(gold):
    """The 254x190 crop read from the 256x192 buffer adapt_x_u8 makes (row pitch 768 bytes) gives the bits of a
    contiguous crop."""
    from src.net import Net
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    pa, pb, info, _ = Net().adapt_x_u8(a, b)
    assert pa.shape == (1, 192, 256, 3) and info is not None
    h, w = a.shape[:2]
    va, vb = dev(pa)[:, :h, :w], dev(pb)[:, :h, :w]
    assert not va.is_contiguous()
    got = refine(dev(init)[None], va, vb).cpu().numpy()
    want = refine(dev(init)[None], dev(a)[None], dev(b)[None]).cpu().numpy()
    assert np.array_equal(got, want)


def test_padded_flow_updated_in_place(gold):
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    h, w = init.shape[:2]
    buf = torch.full((192, 256, 2), 7.0, device="cuda")
    buf[:h, :w] = dev(init)
    view = buf[:h, :w]
    out = refine(view, dev(a), dev(b), inplace=True)
    assert out is view
    want = refine(dev(init), dev(a), dev(b)).cpu().numpy()
    assert np.array_equal(buf[:h, :w].cpu().numpy(), want)
    assert bool((buf[h:] == 7.0).all()) and bool((buf[:, w:] == 7.0).all())


def test_zero_iterations_leave_flow(gold):
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    for kw in (dict(niter_outer=0), dict(niter_inner=0)):
        assert np.array_equal(refine(dev(init), dev(a), dev(b), **kw).cpu().numpy(), init)
    # niter_solver = 0: the system is built, no SOR sweep runs, du stays 0 (solver.c slow path semantics)
    assert np.array_equal(refine(dev(init), dev(a), dev(b), niter_solver=0).cpu().numpy(), init + 0.0)


def test_thin_images_take_the_readable_solver(gold):
    """w < 2 or h < 2: sor_coupled's slow path; the result is finite and moves the flow."""
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    for sl in ((slice(0, 40), slice(0, 1)), (slice(0, 1), slice(0, 60))):
        f = init[sl]
        got = refine(dev(f), dev(a[sl]), dev(b[sl])).cpu().numpy()
        assert got.shape == f.shape and np.isfinite(got).all()


def _seeded_flownet_s():
    from src import weights as W
    from src.flownet_s.flownet_s import FlowNetS
    from src.net import Mode
    net = FlowNetS(mode=Mode.TEST)
    net.weights = W.init_weights("FlowNetS", 1234)
    return net


def test_net_test_refines_the_cropped_flow(golden_dir, tmp_path):
    from src.net import imread
    from src.variational import refine
    pa = os.path.join(golden_dir, "samples", "0img0.ppm")
    pb = os.path.join(golden_dir, "samples", "0img1.ppm")
    net = _seeded_flownet_s()
    kw = dict(out_path=str(tmp_path), save_image=False, save_flo=False, compute_metrics=False)
    plain = net.test(None, pa, pb, **kw)
    again = net.test(None, pa, pb, variational_refinement=False, **kw)
    assert np.array_equal(plain, again)
    refined = net.test(None, pa, pb, variational_refinement=True, **kw)
    want = refine(dev(plain), dev(imread(pa)), dev(imread(pb))).cpu().numpy()
    assert refined.shape == plain.shape
    assert np.array_equal(refined, want)
    assert not np.array_equal(refined, plain)


def test_test_batch_writes_refined_flows(golden_dir, tmp_path):
    from src.flowlib import read_flow
    from src.net import imread
    from src.variational import refine
    pa = os.path.join(golden_dir, "samples", "0img0.ppm")
    pb = os.path.join(golden_dir, "samples", "0img1.ppm")
    lst = tmp_path / "pairs.txt"
    lst.write_text("%s %s\n%s %s\n" % (pa, pb, pb, pa))
    net = _seeded_flownet_s()
    kw = dict(save_image=False, save_flo=True, compute_metrics=False, log_metrics2file=False, batch_size=2)
    plain = net.test_batch(None, str(lst), str(tmp_path / "off"), **kw)
    refined = net.test_batch(None, str(lst), str(tmp_path / "on"), variational_refinement=True, **kw)
    for (x, y), f0, f1 in zip(((pa, pb), (pb, pa)), plain, refined):
        want = refine(dev(f0), dev(imread(x)), dev(imread(y))).cpu().numpy()
        assert np.array_equal(f1, want)
        name = os.path.splitext(os.path.basename(x))[0]
        written = read_flow(str(tmp_path / "on" / "samples" / (name + "_flow.flo")))
        assert np.array_equal(written, want)


def test_calc_variational_inference_map_round_trip(gold, tmp_path):
    from PIL import Image
    from src.flowlib import read_flow, write_flow
    from src.variational import calc_variational_inference_map
    a, b, init, _ = case_inputs(gold, "crop")
    ia, ib = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    Image.fromarray(a).save(ia)
    Image.fromarray(b).save(ib)
    fi, fo = str(tmp_path / "in.flo"), str(tmp_path / "out.flo")
    write_flow(init, fi)
    calc_variational_inference_map(ia, ib, fi, fo, "sintel")
    got = read_flow(fo)
    assert got.shape == init.shape
    mean, p999, _ = epe_stats(on_grid(got, int(gold["grid_step"])), gold["crop_out"])
    assert mean < MEAN_TOL and p999 < P999_TOL


def test_bad_arguments_raise_before_launch(gold):
    from src.variational import refine
    a, b, init, _ = case_inputs(gold, "crop")
    fa, ta, tb = dev(init), dev(a), dev(b)
    with pytest.raises(TypeError):
        refine(fa.double(), ta, tb)
    with pytest.raises(TypeError):
        refine(fa, ta.float(), tb)
    with pytest.raises(TypeError):
        refine(init, ta, tb)
    with pytest.raises(ValueError):
        refine(fa[..., :1], ta, tb)
    with pytest.raises(ValueError):
        refine(fa, ta[:-1], tb)
    with pytest.raises(ValueError):
        refine(fa, ta, tb[..., :2])
    with pytest.raises(ValueError):
        refine(fa[None].expand(2, -1, -1, -1), ta, tb)
    with pytest.raises(ValueError):
        refine(fa, ta, tb, sigma=0.0)
    with pytest.raises(ValueError):
        refine(fa, ta, tb, niter_solver=-1)
    with pytest.raises(ValueError):
        refine(fa, ta, tb, preset="nope")
    with pytest.raises(TypeError):
        refine(fa, ta, tb, beta=1.0)
    torch.cuda.synchronize()
