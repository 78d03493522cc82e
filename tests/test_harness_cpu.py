"""The inference harness without a GPU (src/net.py, the classic CLIs): Net.test is the one-line case of Net.test_batch,
the four input adaptors pad alike, and the six `python -m src.<model>.test` entry points differ in their default
checkpoint alone."""
import importlib
import inspect

import numpy as np
import pytest

H, W = 70, 100            # pads to 128 x 128: the smallest size at which pad, crop and grouping all act


class _StubEngine:
    """Stands in for the HIP engine: records what it is handed; the flow is a fixed function of the inputs."""

    def __init__(self):
        self.inputs, self.launches, self.outputs = [], 0, {}

    def _set(self, flow, *arrays):
        import torch
        self.inputs.append(tuple(np.array(x) for x in arrays))
        self.outputs = {"flow": torch.from_numpy(np.ascontiguousarray(flow, np.float32))}

    def set_inputs_u8(self, a, b, scale=(True, True)):
        assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 4
        f = a[..., :2].astype(np.float32) - b[..., 1:].astype(np.float32) / 8
        self._set(f * (2.0 if scale[0] else 1.0) + (0.5 if scale[1] else 0.0), a, b)

    def set_inputs_interp_u8(self, a, m, sf, flags):
        m = m[..., 0] if m.ndim == 4 else m               # [N,H,W,1] or [N,H,W], as Engine.set_inputs_interp_u8 takes them
        fl = np.asarray(flags, bool).reshape(-1, 2)
        assert a.dtype == np.uint8 and m.dtype == np.uint8 and sf.dtype == np.float32 and len(fl) == len(a)
        f = sf + a[..., :2].astype(np.float32) / 16 + m[..., None].astype(np.float32) / 32
        self._set(f * np.where(fl[:, 0], 2.0, 1.0)[:, None, None, None] + np.where(fl[:, 1], 0.5, 0.0)[:, None, None, None],
                  a, m, sf)

    def launch(self):
        self.launches += 1


def _stubbed(net, monkeypatch):
    """`net` with seeded-weight construction and the engine replaced; returns ({engine key: stub}, [keys as requested])."""
    net.weights = {}
    engines, asked = {}, []

    def engine(batch, height, width, uint8_inputs=False, interp_u8_inputs=False):
        key = (batch, height, width, bool(uint8_inputs), bool(interp_u8_inputs))
        asked.append(key)
        return engines.setdefault(key, _StubEngine())

    monkeypatch.setattr(net, "engine", engine)
    return engines, asked


def _frames(tmp_path):
    from PIL import Image
    from src import flowlib
    rng = np.random.default_rng(12)
    seq = tmp_path / "seq"
    seq.mkdir()
    a = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    b = np.roll(a, (1, -2), (0, 1))
    m = (rng.random((H, W)) > 0.8).astype(np.uint8) * 255
    sf = rng.standard_normal((H, W, 2)).astype(np.float32) * (m > 0)[..., None]
    p = {k: str(seq / ("frame_0001" + s)) for k, s in (("a", ".png"), ("b", "_next.png"), ("m", "_mask.png"), ("sf", "_sparse.flo"))}
    Image.fromarray(a).save(p["a"])
    Image.fromarray(b).save(p["b"])
    Image.fromarray(m).save(p["m"])
    flowlib.write_flow(sf, p["sf"])
    return p


@pytest.mark.parametrize("input_type", ["image_pairs", "image_matches"])
def test_single_run_is_the_one_line_list(input_type, tmp_path, monkeypatch):
    from src.flownet_s.flownet_s import FlowNetS
    from src.flownet_s_interp.flownet_s_interp import FlowNetS_interp
    from src.net import Mode
    p = _frames(tmp_path)
    lst = tmp_path / "one.txt"
    if input_type == "image_pairs":
        cls, line = FlowNetS, [p["a"], p["b"]]
        single_kw = dict(input_b_path=p["b"])
        key = (1, 128, 128, True, False)
    else:
        cls, line = FlowNetS_interp, [p["a"], p["m"], p["sf"]]
        single_kw = dict(matches_a_path=p["m"], sparse_flow_path=p["sf"])
        key = (1, 128, 128, False, True)
    lst.write_text(" ".join(line) + "\n")

    one = cls(mode=Mode.TEST)
    engines1, asked1 = _stubbed(one, monkeypatch)
    flow1 = one.test(None, p["a"], out_path=str(tmp_path / "single"), input_type=input_type, **single_kw)
    many = cls(mode=Mode.TEST)
    engines2, asked2 = _stubbed(many, monkeypatch)
    flows = many.test_batch(None, str(lst), str(tmp_path / "list"), input_type=input_type, batch_size=1,
                            log_metrics2file=False)

    assert len(flows) == 1 and flow1.shape == (H, W, 2) and flow1.dtype == np.float32
    assert np.array_equal(flow1, flows[0]) and np.abs(flow1).max() > 1
    for name in ("frame_0001_flow.flo", "frame_0001_viz.png"):
        got = (tmp_path / "single" / "seq" / name).read_bytes()
        assert got == (tmp_path / "list" / "seq" / name).read_bytes() and len(got) > 100
    assert set(asked1) == set(asked2) == {key} and list(engines1) == list(engines2) == [key]
    assert engines1[key].launches == 1 and engines2[key].launches == 1


def _adaptor_calls(net, h, w):
    """(name, padded arrays, info) of each of the four adaptors on an h x w input."""
    rng = np.random.default_rng(5)
    a = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)
    b = rng.integers(1, 256, (h, w, 3)).astype(np.uint8)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    sf = (rng.random((h, w, 2)) + 1).astype(np.float32)
    r = net.adapt_x(a, b)
    yield "adapt_x", r[:2], r[2]
    r = net.adapt_x_u8(a, b)
    yield "adapt_x_u8", r[:2], r[2]
    r = net.adapt_x_matches(a, m, sf)
    yield "adapt_x_matches", r[:3], r[3]
    r = net.adapt_x_matches_u8(a, m, sf)
    yield "adapt_x_matches_u8", r[:3], r[3]


def test_the_four_adaptors_pad_alike():
    from src.net import Net
    net = Net()
    seen = []
    for name, arrays, info in _adaptor_calls(net, H, W):
        assert info == (1, H, W, 3), name
        for x in arrays:
            assert x.shape[:3] == (1, 128, 128), name
            assert x[:, :H, :W].all(), name                                   # (the inputs hold no zero)
            assert not x[:, H:].any() and not x[:, :, W:].any(), name         # everything outside the original is zero
        seen.append(name)
    assert seen == ["adapt_x", "adapt_x_u8", "adapt_x_matches", "adapt_x_matches_u8"]
    for name, arrays, info in _adaptor_calls(net, 64, 128):
        assert info is None, name
        assert all(x.shape[:3] == (1, 64, 128) for x in arrays), name


# ---- the six classic CLIs: the table below is what the six files held before they shared one parser ---------------
_STR2BOOL = "str2bool"
# dest: (option string, type, default, required, nargs, const, choices)
CLASSIC_OPTIONS = {
    "input_a": ("--input_a", str, None, True, None, None, None),
    "input_b": ("--input_b", str, None, True, None, None, None),
    "out": ("--out", str, None, True, None, None, None),
    "checkpoint": ("--checkpoint", str, "<per model>", False, None, None, None),
    "dtype": ("--dtype", str, "f32", False, None, None, ["f32", "bf16", "f16", "f16x2"]),
    "occlusions": ("--occlusions", _STR2BOOL, False, False, "?", True, None),
}
CLASSIC = {
    "flownet_c": ("FlowNetC", "./checkpoints/FlowNetC/flownet-C.ckpt-0"),
    "flownet_cs": ("FlowNetCS", "./checkpoints/FlowNetCS/flownet-CS.ckpt-0"),
    "flownet_css": ("FlowNetCSS", "./checkpoints/FlowNetCSS/flownet-CSS.ckpt-0"),
    "flownet_s": ("FlowNetS", "./checkpoints/FlowNetS/flownet-S.ckpt-0"),
    "flownet_sd": ("FlowNetSD", "./checkpoints/FlowNetSD/flownet-SD.ckpt-0"),
    "flownet2": ("FlowNet2", "./checkpoints/FlowNet2/flownet-2.ckpt-0"),
}
CLASSIC_HELP = {
    "input_a": "Path to first image",
    "input_b": "Path to second image",
    "out": "Path to output flow result",
    "checkpoint": ".npz weights keyed by the reference variable names",
    "dtype": None,
    "occlusions": "also run the pair backwards in the same launch and write the forward-backward occlusion masks "
                  "(<name>_occ.png, <name>_occ_bw.png) and the backward flow (<name>_flow_bw.flo)",
}


@pytest.mark.parametrize("model", sorted(CLASSIC))
def test_classic_cli_parser_and_main(model, monkeypatch):
    from src.net import Net, str2bool
    cls_name, checkpoint = CLASSIC[model]
    cli = importlib.import_module("src.%s.test" % model)
    cls = getattr(importlib.import_module("src.%s.%s" % (model, model)), cls_name)
    actions = {a.dest: a for a in cli.build_parser()._actions if a.dest != "help"}
    assert list(actions) == list(CLASSIC_OPTIONS)
    for dest, (flag, typ, default, required, nargs, const, choices) in CLASSIC_OPTIONS.items():
        a = actions[dest]
        assert a.option_strings == [flag], dest
        assert a.type is (str2bool if typ is _STR2BOOL else typ), dest
        assert a.default == (checkpoint if dest == "checkpoint" else default), dest
        assert (a.required, a.nargs, a.const, a.choices, a.help) == (required, nargs, const, choices, CLASSIC_HELP[dest]), dest

    calls = []
    monkeypatch.setattr(cls, "test", lambda self, *args, **kw: calls.append((self, args, kw)))
    monkeypatch.setattr(cli, "FLAGS", cli.build_parser().parse_args(["--input_a", "a.png", "--input_b", "b.png", "--out", "o",
                                                                    "--dtype", "f16x2", "--occlusions"]))
    cli.main()
    (net, args, kw), = calls
    assert type(net) is cls and net.dtype == "f16x2"
    passed = inspect.signature(Net.test).bind(net, *args, **kw).arguments
    passed.pop("self")
    assert dict(passed) == dict(checkpoint=checkpoint, input_a_path="a.png", input_b_path="b.png", out_path="o",
                                occlusions=True)
