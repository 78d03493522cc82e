"""FlowNetS_interp from the bytes its input files hold: fn2_pack_interp_u8 against fn2_pack_pair on host-prepared floats
(bit for bit), the engine option and its captured plan, FlowNetS_interp.model on uint8 inputs, Net.test_batch over
'image_matches' list files (outputs, metrics log, variational refinement) and the list form of the CLI.

Bounds: the kernel and the engine do the arithmetic of the float path operation for operation -- same table, same fp32
multiply -- so those comparisons are exact.  Against the fp64 oracle the bound is the suite's: mean EPE < 1e-3 px
(EPE_TOL of tests/test_gpu_models.py, BASELINE's north star)."""
import os

import numpy as np
import pytest
import torch

from oracle import models as refm

pytestmark = pytest.mark.gpu

EPE_TOL = 1e-3  # px
SENTINEL = 0x5A


def epe(x, y):
    d = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return float(np.sqrt((d * d).sum(-1)).mean())


def sample(rng, h, w, image="bytes", mask="255"):
    """One (image, mask, sparse flow, dense flow) set as the files hold it: uint8 image (values 0..255, or 0/1), uint8 mask
    (0/255 as a PNG mask is written, or 0/1), fp32 sparse flow = dense flow on the matches."""
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8) if image == "bytes" else (rng.random((h, w, 3)) < 0.5).astype(np.uint8)
    m = (rng.random((h, w)) > 0.9).astype(np.uint8) * (255 if mask == "255" else 1)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    dense = np.stack([6 * np.sin(xx / 23) + 2, 4 * np.cos(yy / 17) - 1], -1).astype(np.float32)
    dense += rng.standard_normal((h, w, 2)).astype(np.float32) * 0.25
    return img, m, dense * (m > 0)[..., None].astype(np.float32), dense


def _net(dtype="f16x2"):
    from src.flownet_s_interp.flownet_s_interp import FlowNetS_interp
    from src.net import Mode
    return FlowNetS_interp(mode=Mode.TEST, dtype=dtype)


def float_inputs(net, sets):
    """adapt_x_matches (the host float path) on each set, stacked: (a, m, sf) fp32."""
    parts = [net.adapt_x_matches(img, m, sf)[:3] for img, m, sf, _ in sets]
    return tuple(np.concatenate([p[k] for p in parts], 0) for k in range(3))


def u8_inputs(net, sets):
    parts = [net.adapt_x_matches_u8(img, m, sf) for img, m, sf, _ in sets]
    return (tuple(np.concatenate([p[k] for p in parts], 0) for k in range(3)), [p[4] for p in parts])


# ---------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("dtype", ["f32", "f16x2", "bf16", "f16"])
def test_pack_interp_u8_writes_the_bytes_pack_pair_writes(dtype):
    """A ragged pixel count (3 x 37 x 53), pad 3; in one batch a 0..255 image with a 0/255 mask (both divided), a 0..255
    image with a 0/1 mask (mask not divided) and a 0/1 image (not divided).  The interior equals fn2_pack_pair on
    adapt_x_matches' floats with in_b = [0.05 * sf | m] byte for byte; the border keeps what the buffer held; the two
    padding channels hold the zeros of the group store."""
    import ctypes as C
    from src import _hip
    from src.engine import _CODE, _DT
    net = _net()
    rng = np.random.default_rng(31)
    n, h, w, pad = 3, 37, 53, 3
    sets = [sample(rng, h, w), sample(rng, h, w, mask="1"), sample(rng, h, w, image="01")]
    want_flags = [(True, True), (True, False), (False, True)]
    a = np.zeros((n, h, w, 3), np.float32)
    b = np.zeros((n, h, w, 3), np.float32)
    img8, m8, sf32 = np.zeros((n, h, w, 3), np.uint8), np.zeros((n, h, w), np.uint8), np.zeros((n, h, w, 2), np.float32)
    for i, (img, m, sf, _) in enumerate(sets):
        fa, fm, fsf, _ = net.adapt_x_matches(img, m, sf, divisor=1)
        a[i] = fa[0]
        b[i] = np.concatenate([fsf[0] * np.float32(0.05), fm[0]], -1)
        ua, um, usf, info, scale = net.adapt_x_matches_u8(img, m, sf, divisor=1)
        assert info is None and scale == want_flags[i]
        img8[i], m8[i], sf32[i] = ua[0], um[0, :, :, 0], usf[0]
    assert a[2].max() == 1.0 and b[1, :, :, 2].max() == 1.0 and b[0, :, :, 2].max() == 1.0

    def stem():
        t = torch.empty((n, h + 2 * pad, w + 2 * pad, 8), dtype=_DT[dtype], device="cuda")
        t.view(torch.uint8).fill_(SENTINEL)
        return t

    lib = _hip.lib()
    dev = lambda x: torch.from_numpy(x).cuda()
    ref, got = stem(), stem()
    da, db = dev(a), dev(b)
    v = _hip.view(ref, 6, 0, _CODE[dtype])
    _hip.check(lib.fn2_pack_pair(_hip.ptr(da), _hip.ptr(db), C.byref(v), pad, _hip.stream_ptr()))
    d_img, d_m, d_sf = dev(img8), dev(m8), dev(sf32)
    lut = dev((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32))
    flags = dev(np.array(want_flags, np.uint8))
    v2 = _hip.view(got, 6, 0, _CODE[dtype])
    _hip.check(lib.fn2_pack_interp_u8(_hip.ptr(d_img), _hip.ptr(d_m), _hip.ptr(d_sf), _hip.ptr(lut), _hip.ptr(flags),
                                      C.byref(v2), pad, _hip.stream_ptr()))
    torch.cuda.synchronize()
    rb, gb = ref.view(torch.uint8).cpu().numpy(), got.view(torch.uint8).cpu().numpy()   # [n, hp, wp, bytes per pixel]
    assert np.array_equal(gb, rb)
    inner = np.zeros(gb.shape[:3], bool)
    inner[:, pad:pad + h, pad:pad + w] = True
    assert (gb[~inner] == SENTINEL).all()                         # the border is never written
    assert not (gb[inner] == SENTINEL).all(axis=-1).any()         # every interior pixel is
    if dtype == "f16x2":   # a group is 8 fp16 hi parts then 8 fp16 lo parts
        halves = got.view(torch.float16)[:, pad:pad + h, pad:pad + w].cpu().numpy()
        assert (halves[..., [6, 7, 14, 15]] == 0).all()
    else:
        assert (got[:, pad:pad + h, pad:pad + w, 6:].float().cpu().numpy() == 0).all()


# ---------------------------------------------------------------------------------------------- 2. the engine
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_engine_interp_u8_inputs_equal_the_float_engine(dtype):
    from src import weights as W
    from src.engine import Engine
    net = _net(dtype)
    wts = W.init_weights("FlowNetS_interp", 17)
    rng = np.random.default_rng(5)
    first = [sample(rng, 64, 128), sample(rng, 64, 128, mask="1")]
    second = [sample(rng, 64, 128, image="01"), sample(rng, 64, 128)]
    feng = Engine("FlowNetS_interp", wts, 2, 64, 128, dtype)
    ueng = Engine("FlowNetS_interp", wts, 2, 64, 128, dtype, interp_u8_inputs=True)
    assert any(fn is ueng.lib.fn2_pack_interp_u8 for _, fn, _ in ueng.ops)
    assert not any(fn is ueng.lib.fn2_pack_pair for _, fn, _ in ueng.ops)
    assert not any(fn is feng.lib.fn2_pack_interp_u8 for _, fn, _ in feng.ops)
    want = []
    for sets in (first, second):
        feng.set_inputs_interp(*float_inputs(net, sets))
        feng.launch()
        want.append(feng.outputs["flow"].clone())
    assert not torch.equal(want[0], want[1])
    (u1, flags1), (u2, flags2) = u8_inputs(net, first), u8_inputs(net, second)
    assert flags1 == [(True, True), (True, False)] and flags2 == [(False, True), (True, True)]
    ueng.set_inputs_interp_u8(*u1, flags1)
    ueng.launch()
    assert torch.equal(ueng.outputs["flow"], want[0])
    ueng.capture()
    ueng.set_inputs_interp_u8(*u2, flags2)     # other inputs and other flags through the captured plan ...
    ueng.launch()
    torch.cuda.synchronize()
    assert torch.equal(ueng.outputs["flow"], want[1])
    ueng.set_inputs_interp_u8(*u1, flags1)     # ... and back
    ueng.launch()
    torch.cuda.synchronize()
    assert torch.equal(ueng.outputs["flow"], want[0])
    # one pair of flags for every sample
    ueng.set_inputs_interp_u8(*u8_inputs(net, [second[1], first[0]])[0], (True, True))
    ueng.launch()
    feng.set_inputs_interp(*float_inputs(net, [second[1], first[0]]))
    feng.launch()
    assert torch.equal(ueng.outputs["flow"], feng.outputs["flow"])
    with pytest.raises(ValueError):
        feng.set_inputs_interp_u8(*u1, flags1)                                    # built without the option
    with pytest.raises(ValueError):
        ueng.set_inputs_interp_u8(u1[0].astype(np.float32), u1[1], u1[2], flags1)  # not bytes
    with pytest.raises(ValueError):
        ueng.set_inputs_interp_u8(u1[0], u1[1], u1[2].astype(np.float64), flags1)
    with pytest.raises(ValueError):
        ueng.set_inputs_interp_u8(u1[0][:1], u1[1], u1[2], flags1)                 # wrong shape
    with pytest.raises(ValueError):
        Engine("FlowNetS", W.init_weights("FlowNetS", 1), 1, 64, 64, dtype, interp_u8_inputs=True)


# ---------------------------------------------------------------------------------------------- 3. the model
@pytest.mark.parametrize("dtype", ["f32", "f16x2"])
def test_model_on_uint8_inputs_matches_oracle(dtype):
    net = _net(dtype)
    wts = net.load_weights(None, seed=21)
    rng = np.random.default_rng(9)
    sets = [sample(rng, 128, 192), sample(rng, 128, 192, mask="1")]
    a, m, sf = float_inputs(net, sets)
    want = refm.flownet_s_interp(wts, {"input_a": a, "matches_a": m, "sparse_flow": sf})["flow"]
    (ua, um, usf), flags = u8_inputs(net, sets)
    got = net.model({"input_a": ua, "matches_a": um, "sparse_flow": usf})          # flags from the samples' maxima
    e = epe(got["flow"].float().cpu().numpy(), want)
    print("FlowNetS_interp %s uint8 inputs: mean EPE vs oracle %.3e px" % (dtype, e))
    assert e < EPE_TOL
    assert any(k[5] for k in net._engines)                                          # the uint8 engine ran
    again = net.model({"input_a": ua, "matches_a": um, "sparse_flow": usf, "scale": flags}, is_training=False)
    assert set(again) == {"flow"} and torch.equal(again["flow"], got["flow"])
    old = net.model({"input_a": a, "matches_a": m, "sparse_flow": sf})              # float inputs: the float path
    assert torch.equal(old["flow"], got["flow"])


# ---------------------------------------------------------------------------------------------- 4.-6. list files
H0, W0 = 100, 150   # padded to 128 x 192


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    """Five lines in two sizes and four layouts, batch_size 2 -> chunks [3 fields | 4 fields, 0/1 mask], [5 fields,
    60 x 150 | 7 fields], [4 fields]: two sizes in one chunk, short groups, mixed scale flags in one launch."""
    from PIL import Image
    from src import flowlib
    root = tmp_path_factory.mktemp("interp_list")
    seq = root / "seq_a"
    seq.mkdir()
    rng = np.random.default_rng(77)
    recs = []
    spec = [(3, H0, W0, "255"), (4, H0, W0, "1"), (5, 60, W0, "255"), (7, H0, W0, "255"), (4, H0, W0, "255")]
    for k, (nf, h, w, mk) in enumerate(spec):
        img, m, sf, dense = sample(rng, h, w, mask=mk)
        img2 = np.roll(img, (1, -2), (0, 1))
        name = "frame_%04d" % (k + 1)
        p = {key: str(seq / (name + suffix)) for key, suffix in
             (("image", ".png"), ("matches", "_mask.png"), ("sparse", "_sparse.flo"), ("gt", "_gt.flo"),
              ("occ", "_occ.png"), ("inv", "_inv.png"), ("image_b", "_next.png"))}
        Image.fromarray(img).save(p["image"])
        Image.fromarray(img2).save(p["image_b"])
        Image.fromarray(m).save(p["matches"])
        flowlib.write_flow(sf, p["sparse"])
        flowlib.write_flow(dense + np.float32(0.5), p["gt"])
        occ = (rng.random((h, w)) > 0.8).astype(np.uint8) * 255
        inv = (rng.random((h, w)) > 0.97).astype(np.uint8) * 255
        Image.fromarray(occ).save(p["occ"])
        Image.fromarray(inv).save(p["inv"])
        order = {3: ("image", "matches", "sparse"), 4: ("image", "matches", "sparse", "gt"),
                 5: ("image", "matches", "sparse", "gt", "image_b"),
                 7: ("image", "matches", "sparse", "gt", "occ", "inv", "image_b")}[nf]
        recs.append(dict(name=name, nf=nf, paths=p, line=" ".join(p[key] for key in order), img=img, img2=img2, m=m, sf=sf,
                         occ=occ, inv=inv))
    lst = root / "interp_val.txt"
    lst.write_text("\n".join(r["line"] for r in recs) + "\n")
    return dict(root=root, list=str(lst), recs=recs)


@pytest.fixture(scope="module")
def plain_run(listing):
    net = _net("f16x2")
    out = listing["root"] / "out"
    flows = net.test_batch(None, listing["list"], str(out), input_type="image_matches", accumulate_metrics=True,
                           batch_size=2)
    return net, out, flows


def test_test_batch_image_matches_outputs_and_metrics(listing, plain_run):
    from src import flowlib
    net, out, flows = plain_run
    recs = listing["recs"]
    assert len(flows) == len(recs)
    assert {k[:3] for k in net._engines if k[5]} == {(2, 128, 192), (2, 64, 192)}   # one engine per padded size
    for r, flow in zip(recs, flows):
        a, m, sf, info = net.adapt_x_matches(r["img"], r["m"], r["sf"])
        want = refm.flownet_s_interp(net.weights, {"input_a": a, "matches_a": m, "sparse_flow": sf})["flow"][0]
        want = want[:info[1], :info[2]]
        assert flow.shape == r["img"].shape[:2] + (2,) and flow.dtype == np.float32
        e = epe(flow, want)
        print("%s (%d fields): mean EPE vs oracle %.3e px" % (r["name"], r["nf"], e))
        assert e < EPE_TOL
        assert np.array_equal(flowlib.read_flow(str(out / "seq_a" / (r["name"] + "_flow.flo"))), flow)
        assert (out / "seq_a" / (r["name"] + "_viz.png")).exists()
        assert (out / "seq_a" / (r["name"] + "_viz_norm_gt_max_motion.png")).exists()
    log = (out / "interp_val_metrics.log").read_text()
    with_gt = [r for r in recs if r["nf"] >= 4]
    assert log.count("MPI-Sintel Flow Error Metrics") == len(with_gt) + 1 and log.count("(AVERAGE)") == 1
    assert recs[0]["name"] not in log
    for r, flow in zip(recs, flows):
        if r["nf"] < 4:
            continue
        gt = flowlib.read_flow(r["paths"]["gt"])
        masks = dict(occ_mask=r["occ"], inv_mask=r["inv"]) if r["nf"] == 7 else {}
        m, *_ = flowlib.compute_all_metrics(flow, gt, **masks)
        assert r["name"] in log and ("%.4f" % m["EPEall"]) in log
        if r["nf"] == 7:   # the occlusion and invalid masks were consumed: the unmatched row is that of the masks
            assert np.isfinite(m["EPEumat"]) and m["EPEumat"] > 0
            block = log[log.index(r["name"]):]
            umt = [ln for ln in block.splitlines() if ln.startswith("(umt)")][0]
            assert ("%.4f" % m["EPEumat"]) in umt and np.isfinite(float(umt.split()[-1]))
    assert np.isfinite(net.last_average_metrics["EPEall"])


def test_test_batch_image_matches_refines_lines_with_a_second_image(listing, plain_run):
    from src import flowlib
    from src.variational import refine
    net, _, plain = plain_run
    out = listing["root"] / "refined"
    refined = net.test_batch(None, listing["list"], str(out), input_type="image_matches", save_image=False,
                             compute_metrics=False, log_metrics2file=False, variational_refinement=True, batch_size=2)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    seen = set()
    for r, f0, f1 in zip(listing["recs"], plain, refined):
        if r["nf"] in (5, 7):
            want = refine(dev(f0), dev(r["img"]), dev(r["img2"])).cpu().numpy()
            assert np.array_equal(f1, want) and not np.array_equal(f1, f0)
        else:   # no second image on the line: nothing to refine on
            assert np.array_equal(f1, f0)
        assert np.array_equal(flowlib.read_flow(str(out / "seq_a" / (r["name"] + "_flow.flo"))), f1)
        seen.add(r["nf"])
    assert seen == {3, 4, 5, 7}


def test_cli_list_form_writes_what_test_batch_writes(listing, plain_run):
    from src import flowlib
    from src.flownet_s_interp import test as cli
    _, out, flows = plain_run
    cli_out = listing["root"] / "cli"
    cli.FLAGS = cli.build_parser().parse_args(["--input_a", listing["list"], "--out", str(cli_out), "--dtype", "f16x2",
                                               "--no_deconv_biases", "true", "--batch_size", "2",
                                               "--log_metrics2file", "true"])
    cli.main()
    ours = sorted(os.listdir(out / "seq_a"))
    assert sorted(os.listdir(cli_out / "seq_a")) == ours and len(ours) == 3 * len(flows)
    for r, flow in zip(listing["recs"], flows):
        assert np.array_equal(flowlib.read_flow(str(cli_out / "seq_a" / (r["name"] + "_flow.flo"))), flow)
    strip = lambda text: [ln for ln in text.splitlines() if not ln.startswith("Today is")]
    assert strip((cli_out / "interp_val_metrics.log").read_text()) == strip((out / "interp_val_metrics.log").read_text())


def test_single_frame_test_takes_the_uint8_path_and_prints_the_metrics_block(listing, capsys):
    from src import flowlib
    r = listing["recs"][3]
    net = _net("f16x2")
    p = r["paths"]
    flow = net.test(None, p["image"], matches_a_path=p["matches"], sparse_flow_path=p["sparse"], input_type="image_matches",
                    out_path=str(listing["root"] / "single"), gt_flow=p["gt"], occ_mask=p["occ"], inv_mask=p["inv"],
                    save_image=False)
    assert any(k[5] for k in net._engines) and not any(not k[5] for k in net._engines)
    text = capsys.readouterr().out
    m, *_ = flowlib.compute_all_metrics(flow, flowlib.read_flow(p["gt"]), occ_mask=r["occ"], inv_mask=r["inv"])
    assert "MPI-Sintel Flow Error Metrics" in text and r["name"] in text
    assert ("%.4f" % m["EPEall"]) in text and ("%.4f" % m["EPEumat"]) in text and m["EPEumat"] > 0
    a, mm, sf, info = net.adapt_x_matches(r["img"], r["m"], r["sf"])
    old = net.model({"input_a": a, "matches_a": mm, "sparse_flow": sf})["flow"][0, :info[1], :info[2]].cpu().numpy()
    assert np.array_equal(flow, old)
