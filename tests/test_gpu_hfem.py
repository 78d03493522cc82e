"""Device-side hard-example mining: fn2_hfem_hard_weights / fn2_hfem_edge_weights op by op against the NumPy twin
(exact), and the captured FlowNetS_interp train step in the three loss modes against the float64 oracle."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import hfem_twin as twin

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 5), (1, 3, 5), (2, 7, 9), (2, 33, 65), (3, 64, 96)]  # 5, 15, 126, 4290 (> one tile + tail), 18432 pixels


# ---------------------------------------------------------------------------------------------------- value patterns
def _equal(n, rng):
    return np.full(n, 3.0, np.float32)


def _two_values(n, rng):
    """Half the pixels (the even ones) hold the larger value: every k up to n / 2 cuts inside that tie group."""
    return np.where(np.arange(n) % 2 == 0, 2.0, 1.0).astype(np.float32)


def _low_byte(n, rng):
    """Keys that differ in their lowest byte only: 1 + j * 2^-23, j < 256 (each value many times over at the larger sizes)."""
    j = rng.integers(0, 256, n)
    return (1.0 + j * 2.0 ** -23).astype(np.float32)


def _top_byte(n, rng):
    return np.array([2.0 ** -20, 1.0, 2.0 ** 20], np.float32)[rng.integers(0, 3, n)]


def _zeros(n, rng):
    """Mostly exact zeros (prediction == label), a fifth of the pixels off."""
    return np.where(np.arange(n) % 5 == 2, 1.5, 0.0).astype(np.float32)


def _inf(n, rng):
    v = ((np.arange(n) % 7) * 0.25).astype(np.float32)
    v[1::4] = np.inf
    return v


def _one_nan(n, rng):
    v = ((np.arange(n) % 11) * 0.5).astype(np.float32)
    v[n // 2] = np.nan
    return v


def _distinct(n, rng):
    """n distinct values of 12 significant bits in random order: mantissas 2048..4095 over as many exponents as needed."""
    j = rng.permutation(n)
    return np.ldexp((2048 + j % 2048).astype(np.float64), j // 2048 - 11).astype(np.float32)


PATTERNS = {"equal": _equal, "two_values": _two_values, "low_byte": _low_byte, "top_byte": _top_byte, "zeros": _zeros,
            "inf": _inf, "one_nan": _one_nan, "distinct": _distinct}


def _pred_of(v, shape):
    """label = 0, pred = (+-v, 0): the difference is exact and dy = 0, so EPE = sqrt(round(v^2)) -- |v| exactly when v^2 is
    exact (12 significant bits) and, in binary floating point with a correctly rounded square and root, for every other
    v too (the low-byte pattern needs 24 bits); the tests assert epe == |v| before they look at the weights."""
    sign = np.where(np.arange(v.size) % 3 == 1, -1.0, 1.0).astype(np.float32)
    pred = np.zeros(tuple(shape) + (2,), np.float32)
    pred[..., 0] = (sign * v).reshape(shape)
    return pred


def _run_levels(levels):
    """levels: [(pred [..,2], label, k, hard_weight)] as NumPy -> [(epe, weight)] from ONE fn2_hfem_hard_weights launch."""
    from src import _hip
    dev, table, keep = torch.device("cuda"), [], []
    for pred, label, k, hw in levels:
        p, l = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
        npix = pred.size // 2
        # (canaries behind the maps: the kernel must not write past npix)
        e, w = torch.full((npix + 64,), -7.0, device=dev), torch.full((npix + 64,), -7.0, device=dev)
        keep.append((p, l, e, w, npix))
        table.append(_hip.Fn2HfemLevel(p.data_ptr(), l.data_ptr(), e.data_ptr(), w.data_ptr(), npix, int(k), float(hw)))
    arr = (_hip.Fn2HfemLevel * len(table))(*table)
    _hip.check(_hip.lib().fn2_hfem_hard_weights(arr, len(table), _hip.stream_ptr()))
    out = []
    for p, l, e, w, npix in keep:
        e, w = e.cpu().numpy(), w.cpu().numpy()
        assert (e[npix:] == -7.0).all() and (w[npix:] == -7.0).all()
        out.append((e[:npix], w[:npix]))
    return out


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hard_weights_are_the_stable_topk_mask(shape, pattern):
    from src.losses import hard_example_weights
    npix = int(np.prod(shape))
    v = PATTERNS[pattern](npix, np.random.default_rng(npix))
    pred, label = _pred_of(v, shape), np.zeros(tuple(shape) + (2,), np.float32)
    hw = np.float32(2.5)
    for k in sorted({0, 1, npix - 1, npix}):
        (epe, weight), = _run_levels([(pred, label, k, hw)])
        np.testing.assert_array_equal(epe, np.abs(v))  # (NaN == NaN here)
        want = np.where(twin.stable_topk_mask(np.abs(v), k), hw, np.float32(0))
        np.testing.assert_array_equal(weight, want, err_msg="k = %d" % k)
    # the public op, with its own k and weight
    for perc in (33, 50):
        k = twin.oracle_hard_k(npix, perc)
        weight, epe = hard_example_weights(torch.from_numpy(label).cuda(), torch.from_numpy(pred).cuda(), perc_hfem=perc,
                                           lambda_w=2.0, return_epe=True)
        assert weight.shape == epe.shape == tuple(shape) and weight.dtype == torch.float32
        np.testing.assert_array_equal(epe.cpu().numpy().reshape(-1), np.abs(v))
        want = np.where(twin.stable_topk_mask(np.abs(v), k), twin.hard_weight(npix, k, 2.0), np.float32(0))
        np.testing.assert_array_equal(weight.cpu().numpy().reshape(-1), want, err_msg="perc = %d" % perc)


def test_five_levels_in_one_launch_equal_five_launches():
    rng = np.random.default_rng(17)
    levels = []
    for i, shape in enumerate(SHAPES):
        npix = int(np.prod(shape))
        v = np.round(rng.random(npix) * 16).astype(np.float32) / 4  # 65 values: ties at every size
        levels.append((_pred_of(v, shape), np.zeros(tuple(shape) + (2,), np.float32), twin.oracle_hard_k(npix, 50),
                       np.float32(1.5 + i)))
    together = _run_levels(levels)
    for lvl, (epe, weight) in zip(levels, together):
        (epe1, weight1), = _run_levels([lvl])
        np.testing.assert_array_equal(epe, epe1)
        np.testing.assert_array_equal(weight, weight1)
        np.testing.assert_array_equal(weight, np.where(twin.stable_topk_mask(epe, lvl[2]), lvl[3], np.float32(0)))


@pytest.mark.parametrize("shape", [(2, 33, 65), (3, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_random_flows_select_on_the_returned_epe(shape):
    """Float predictions against float labels: epe within 1e-6 relative of NumPy's fp32 (one rounding of the sum may
    differ with a fused multiply-add), and the weights exactly the twin's mask of the epe the kernel returned."""
    rng = np.random.default_rng(23)
    pred = rng.standard_normal(tuple(shape) + (2,)).astype(np.float32)
    label = rng.standard_normal(tuple(shape) + (2,)).astype(np.float32)
    npix = int(np.prod(shape))
    d = pred - label
    want_epe = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).reshape(-1)
    for perc in (33, 50):
        k = twin.oracle_hard_k(npix, perc)
        hw = twin.hard_weight(npix, k, 2.0)
        (epe, weight), = _run_levels([(pred, label, k, hw)])
        np.testing.assert_allclose(epe, want_epe, rtol=1e-6, atol=0)
        np.testing.assert_array_equal(weight, np.where(twin.stable_topk_mask(epe, k), hw, np.float32(0)))


@pytest.mark.parametrize("npix", [15, 4290])
def test_edge_weights_round_product_and_sum_separately(npix):
    from src import _hip
    rng = np.random.default_rng(npix)
    e = rng.random(npix).astype(np.float32)
    for lam in (2.0, 0.3):
        src = torch.from_numpy(e).cuda()
        out = torch.full((npix + 64,), -7.0, device="cuda")
        _hip.check(_hip.lib().fn2_hfem_edge_weights(_hip.ptr(src), lam, _hip.ptr(out), npix, _hip.stream_ptr()))
        got = out.cpu().numpy()
        assert (got[npix:] == -7.0).all()
        np.testing.assert_array_equal(got[:npix], np.float32(1) + np.float32(lam) * e)


# ------------------------------------------------------------------------------------------------- the captured step
def _interp_batch(seed):
    from test_gpu_train import data
    a, _, gt = data(2, 128, 128, seed)
    rng = np.random.default_rng(seed + 1)
    matches = (rng.random((2, 128, 128, 1)) < 0.05).astype(np.float32)
    sparse = (gt * matches).astype(np.float32)
    edges = rng.random((2, 128, 128, 1)).astype(np.float32)
    return a, matches, sparse, gt, edges


def _snapshot(tr, loss):
    from test_gpu_train import device_signs
    torch.cuda.synchronize()
    return dict(loss=float(loss.item()), signs=device_signs(tr),
                dw={id(rec): rec["dw"].cpu().numpy().copy() for rec in tr.eng.layers})


@pytest.fixture(scope="module", params=["", "hard", "edges"])
def steps(request):
    """Two captured steps (different batches) and one eager step from the same start, run once per loss mode; the tests
    below compare what they left against the oracle.  Batch 1 has the seeds of test_flownet_s_interp_gradients_match_oracle."""
    import os
    from src import weights as W
    from src.flownet_s.train import unpack_weights
    from src.trainer import FlowNetSTrainer
    mode = request.param
    wts = W.init_weights("FlowNetS_interp", 9)
    b1, b2 = _interp_batch(4), _interp_batch(40)
    make = lambda: FlowNetSTrainer(wts, 2, 128, 128, dtype="f32", model="FlowNetS_interp", add_hard_flow_mining=mode,
                                   lambda_weight=2.0, hard_examples_perc=50)
    old = os.environ.get("FN2_TRAIN_GRAPH")
    try:
        os.environ["FN2_TRAIN_GRAPH"] = "1"
        tr = make()
        s1 = _snapshot(tr, tr.train_step_interp(*b1[:4], edges=b1[4]))
        captured = getattr(tr, "_step_graphs", None) is not None
        w1 = unpack_weights(tr)
        s2 = _snapshot(tr, tr.train_step_interp(*b2[:4], edges=b2[4]))
        os.environ["FN2_TRAIN_GRAPH"] = "0"
        eager = make()
        eager_loss = float(eager.train_step_interp(*b1[:4], edges=b1[4]).item())
        eager_captured = getattr(eager, "_step_graphs", None) is not None
    finally:
        if old is None:
            os.environ.pop("FN2_TRAIN_GRAPH", None)
        else:
            os.environ["FN2_TRAIN_GRAPH"] = old
    return types.SimpleNamespace(mode=mode, tr=tr, wts=wts, w1=w1, b1=b1, b2=b2, s1=s1, s2=s2, captured=captured,
                                 eager_loss=eager_loss, eager_captured=eager_captured)


def _check_against_oracle(st, weights, batch, snap):
    from oracle import train as reft
    from test_gpu_train import packed_grad
    a, matches, sparse, gt, edges = batch
    b_equiv = np.concatenate([sparse * np.float32(0.05), matches], axis=3)
    want_loss, grads, _ = reft.flownet_s_loss_and_grads(weights, a, b_equiv, gt, signs=snap["signs"], add_hfem=st.mode,
                                                        lambda_w=2.0, perc_hfem=50,
                                                        edges=edges if st.mode == "edges" else None)
    print("mode %r: loss %.8g, oracle %.8g" % (st.mode, snap["loss"], want_loss))
    assert abs(snap["loss"] - want_loss) < 2e-5 * abs(want_loss), (snap["loss"], want_loss)
    worst = 0.0
    for rec in st.tr.eng.layers:
        name = f"{rec['scope']}/{rec['name']}"
        got = snap["dw"][id(rec)]
        want = (grads[name + "/weights"].astype(np.float32).reshape(-1) if rec["kind"] == "upflow"
                else packed_grad(rec, grads[name + "/weights"]).reshape(-1))
        worst = max(worst, np.abs(got - want).max() / (np.abs(want).max() + 1e-12))
    print("mode %r: worst relative gradient error %.3e" % (st.mode, worst))
    # the tolerances of test_flownet_s_interp_gradients_match_oracle ('hard': a pixel within fp32 rounding of the cut)
    assert worst < (2e-5 if st.mode != "hard" else 2e-3), worst


def test_captured_interp_step_matches_oracle(steps):
    assert steps.captured, "train_step_interp did not capture the step"
    _check_against_oracle(steps, steps.wts, steps.b1, steps.s1)


def test_second_replay_with_other_inputs_matches_oracle(steps):
    """The replay reads this step's labels, weights and edge maps, not the first step's."""
    assert steps.tr.step_count == 2
    _check_against_oracle(steps, steps.w1, steps.b2, steps.s2)


def test_eager_interp_step_gives_the_same_loss(steps):
    assert not steps.eager_captured
    assert abs(steps.eager_loss - steps.s1["loss"]) <= 2e-5 * abs(steps.s1["loss"]), (steps.eager_loss, steps.s1["loss"])


def test_edges_choice_is_fixed_by_the_capture():
    from src import weights as W
    from src.trainer import FlowNetSTrainer
    a, matches, sparse, gt, edges = _interp_batch(4)
    tr = FlowNetSTrainer(W.init_weights("FlowNetS_interp", 9), 2, 128, 128, dtype="f32", model="FlowNetS_interp",
                         add_hard_flow_mining="edges")
    tr.train_step_interp(a, matches, sparse, gt)  # no edge map: plain AEPE weights, as on the eager path
    assert tr._step_graphs is not None and tr._mining is None
    with pytest.raises(ValueError, match="edge map"):
        tr.train_step_interp(a, matches, sparse, gt, edges=edges)


def test_interp_cli_trains_through_the_captured_step(tmp_path):
    from src import tfrecord
    from src.flownet_s_interp import train as cli
    rng = np.random.default_rng(11)
    path = str(tmp_path / "interp.tfrecords")
    with tfrecord.TFRecordWriter(path) as w:
        for _ in range(4):
            img = rng.random((128, 192, 3))
            flow = np.clip(rng.standard_normal((128, 192, 2)) * 3, -20, 20).astype(np.float32)
            m = (rng.random((128, 192, 1)) < 0.05).astype(np.float64)
            w.write(tfrecord.encode_sample(img, flow=flow, matches_a=m, sparse_flow=(flow * m).astype(np.float32),
                                           edges_a=rng.random((128, 192, 1)).astype(np.float32)))
    flags = types.SimpleNamespace(records=path, out=str(tmp_path / "ck"), checkpoint=None, ckpt_format="npz", steps=2,
                                  batch=2, dtype="f16x2", height=128, width=192, add_hard_flow_mining="hard",
                                  lambda_weight=2.0, hard_examples_perc=50, seed=3, log_every=1, save_every=10)
    tr = cli.main(flags)
    assert tr.step_count == 2 and np.isfinite(float(tr.loss_dev.item()))
    assert getattr(tr, "_step_graphs", None) is not None and tr._mining == "hard"
