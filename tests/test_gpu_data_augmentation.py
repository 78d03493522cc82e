"""fn2_selflow_stats + fn2_selflow_apply (csrc/selflow_aug.hip) through src/data_augmentation.py against the NumPy twin
(tests/selflow_twin.py): bit for bit wherever data is moved or sampled, to the op-level bar of 1e-5 absolute (DESIGN
section 2) against float64 for the colour arithmetic on values in [0, 1]."""
import numpy as np
import pytest

import selflow_twin as twin

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def DA():
    from src import data_augmentation
    return data_augmentation


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    return np.array_equal(bits(got.cpu().numpy()), bits(want))


def inputs(rng, n, h, w):
    """(image, matches, sparse_flow, edges, flow) as float32 host arrays, a DeepMatching-like sparse mask."""
    img = rng.random((n, h, w, 3), dtype=np.float32)
    flow = (rng.standard_normal((n, h, w, 2)) * 4).astype(np.float32)
    matches = (rng.random((n, h, w, 1)) < 0.3).astype(np.float32)
    sparse = (flow + np.float32(0.25)) * matches  # not the ground truth: a pass-through is told from a re-sampling
    edges = rng.random((n, h, w, 1), dtype=np.float32)
    return img, matches, sparse.astype(np.float32), edges, flow


NAMES = ("image_a", "matches", "sparse_flow", "edges", "flow")


def run_interp(DA, table, data):
    out = DA.apply_params(table, image_a=data[0], matches=data[1], sparse_flow=data[2], edges=data[3], flow=data[4])
    return dict(zip(NAMES, (out[0], out[2], out[3], out[4], out[5])))


def want_interp(table, data):
    return twin.apply(table, image_a=data[0], matches=data[1], sparse_flow=data[2], edges=data[3], flow=data[4])


# ------------------------------------------------------------------------------------------------ flips, permutation
@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 4, 130)])
def test_flips_and_permutation_bit_for_bit(DA, shape):
    n, h, w = shape
    data = inputs(np.random.default_rng(11), n, h, w)
    flips, perms = set(), set()
    for j in range(6):
        table = DA.empty_params(n)
        for s in range(n):
            f, p = (j + s) % 4, (j + 2 * s) % 6
            table[s, [twin.FLIP_LR, twin.FLIP_UD, twin.PERM]] = (f & 1, f >> 1, p)
            flips.add(f), perms.add(p)
        got, want = run_interp(DA, table, data), want_interp(table, data)
        for name in NAMES:
            assert same_bits(got[name], want[name]), (name, j)
    assert flips == set(range(4)) and perms == set(range(6))


@pytest.mark.parametrize("shape", [(3, 5, 7), (2, 4, 130)])
def test_same_flips_twice_return_the_input(DA, shape):
    n, h, w = shape
    img, matches, sparse, edges, flow = inputs(np.random.default_rng(12), n, h, w)
    for f in range(4):
        table = DA.empty_params(n)
        table[:, [twin.FLIP_LR, twin.FLIP_UD]] = (f & 1, f >> 1)
        once = DA.random_flip_with_flow([img, matches, edges], [sparse, flow], params=table)
        twice = DA.random_flip_with_flow(once[0], once[1], params=table)
        for got, want in zip(twice[0] + twice[1], (img, matches, edges, sparse, flow)):
            assert same_bits(got, want), f
        if f:
            assert not np.array_equal(once[1][1].cpu().numpy(), flow)
        if f == 1:  # flip_lr: u of the mirrored pixel, negated; v kept
            assert np.array_equal(once[1][1].cpu().numpy(), flow[:, :, ::-1] * np.float32([-1, 1]))
    # the stage functions leave the other stages off
    table = DA.empty_params(n)
    table[:, twin.PERM] = 3
    table[:, twin.FLIP_LR] = 1
    swapped = DA.random_channel_swap([img], params=table)[0]
    assert same_bits(swapped, img[..., [1, 2, 0]])


# ------------------------------------------------------------------------------------------------ colour
@pytest.mark.parametrize("index", range(3))
def test_colour_chains_against_float64(DA, index):
    """Every chain order at both shapes within 1e-5 of the float64 twin; the measured maxima are in DESIGN section 13."""
    name, img, table = twin.colour_cases()[index]
    want = twin.apply(table, image_a=img)
    got = DA.apply_params(table, image_a=img)[0]
    again = DA.apply_params(table, image_a=img)[0]
    assert same_bits(got, again.cpu().numpy())  # two runs, the same bits
    keep = ~want["hazards"]
    assert want["hazards"].mean() <= 1e-3
    err = np.abs(got.cpu().numpy().astype(np.float64) - want["image_a"])[keep]
    print("selflow colour %s: max abs error vs float64 = %.3e, excluded %d pixels" % (name, err.max(), (~keep).sum()))
    assert err.max() <= 1e-5, (name, err.max())
    res = got.cpu().numpy()
    assert res.min() == 0.0 and res.max() == 1.0  # clipped once, at both ends
    # distort_colour is the same chain with the permutation switched off
    alone = DA.distort_colour(img, params=table).cpu().numpy()
    plain = table.copy()
    plain[:, twin.PERM] = 0
    assert np.abs(alone - twin.apply(plain, image_a=img)["image_a"]).max() <= 1e-5


def test_hue_does_not_commute_with_an_odd_permutation(DA):
    """The permutation comes BEFORE the colour chain: with the order swapped the result differs by far more than the bar."""
    name, img, table = twin.colour_cases()[0]
    got = DA.apply_params(table, image_a=img)[0].cpu().numpy()
    plain = table.copy()
    plain[:, twin.PERM] = 0
    late = np.stack([twin.apply(plain, image_a=img)["image_a"][s][..., list(twin.PERMS[int(table[s, twin.PERM])])]
                     for s in range(len(img))])
    odd = [s for s in range(len(img)) if int(table[s, twin.PERM]) in (1, 2, 5)]
    assert odd and all(np.abs(got[s] - late[s]).max() > 1e-2 for s in odd)


# ------------------------------------------------------------------------------------------------ re-sampling
def resampling_tables(DA, n, h, w):
    """Tables that put each distrib on each sample; rectangles touching every border, overlapping, one of h - 1 rows."""
    rects = [(0, 0, h - 1, max(w // 7, 1)), (h // 2, w - w // 5 - 1, h - h // 2, w // 5 + 1), (h // 4, w // 10, h // 2, w - w // 5)]
    tables = []
    for shift in range(3):
        t = DA.empty_params(n)
        for s in range(n):
            d = (s + shift) % 3
            t[s, twin.DISTRIB] = d
            t[s, [twin.THRESHOLD, twin.KEY0, twin.KEY1]] = (twin.threshold_of(0.25), 0x1234567 + s, 0x9E3779B9 * (shift + 1) % (1 << 32))
            DA.set_rectangles(t[s], rects[:2 + (s + shift) % 2] if d == 2 else [])
        tables.append(t)
    return tables


def check_resampling(DA, table, data, expect_resampled):
    got, want = run_interp(DA, table, data), want_interp(table, data)
    for name in NAMES:
        assert same_bits(got[name], want[name]), name
    m, sf = got["matches"].cpu().numpy(), got["sparse_flow"].cpu().numpy()
    for s, resampled in enumerate(expect_resampled):
        if resampled:
            assert set(np.unique(m[s])) <= {0.0, 1.0}
            assert np.array_equal(sf[s], np.where(m[s] == 1, data[4][s], np.float32(0)))  # -0.0 == 0.0 here
        else:
            assert np.array_equal(m[s], data[1][s]) and np.array_equal(sf[s], data[2][s])
    return m


@pytest.mark.parametrize("shape", [(3, 9, 37), (2, 96, 128)])
def test_resampling_equals_the_twin(DA, shape):
    n, h, w = shape
    data = inputs(np.random.default_rng(21), n, h, w)
    seen = set()
    for table in resampling_tables(DA, n, h, w):
        m = check_resampling(DA, table, data, [int(d) != 0 for d in table[:, twin.DISTRIB]])
        for s in range(n):
            d = int(table[s, twin.DISTRIB])
            seen.add(d)
            if d == 1:
                assert abs(m[s].mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / (h * w))
            if d == 2:
                assert m[s][h - 1, 0, 0] == 1 and m[s][0, 0, 0] == 0 and m[s][h - 1, w - 1, 0] == 0 and m[s][0, w - 1, 0] == 1
    assert seen == {0, 1, 2}
    # a threshold of 0 sets nothing: the DeepMatching inputs come back
    table = DA.empty_params(n)
    table[:, twin.DISTRIB] = 1
    table[:, [twin.KEY0, twin.KEY1]] = (5, 6)
    check_resampling(DA, table, data, [False] * n)
    # the stage function alone, and the validation form, equal the same twin
    table = resampling_tables(DA, n, h, w)[1]
    m, sf = DA.sample_sparse_flow(data[1], data[2], data[4], params=table)
    want = want_interp(table, data)
    assert same_bits(m, want["matches"]) and same_bits(sf, want["sparse_flow"])
    val = DA.augment_all_interp_validation(*data, params=table)
    assert same_bits(val[1], want["matches"]) and same_bits(val[2], want["sparse_flow"])
    assert val[0] is data[0] and val[3] is data[3] and val[4] is data[4]


def all_but(h, w, k):
    """Rectangles that leave exactly the last k pixels of the last row outside (k <= w)."""
    return [(0, 0, h - 1, w), (h - 1, 0, 1, w - k)]


def test_almost_empty_masks_fall_back(DA):
    """sample_from_distribution keeps a re-sampled mask from 0.01 % of the pixels on, in float32: on 96 x 128 that is 1.2288
    pixels (2 kept, 1 just below); on 100 x 100 one pixel is exactly at the bound (kept: float32 100 * (1 / 10000) ==
    float32 0.01), none is below."""
    for (h, w), kept, dropped in (((96, 128), 2, 1), ((100, 100), 1, 0)):
        assert 100.0 * kept / (h * w) >= 0.01 > 100.0 * dropped / (h * w)
        data = inputs(np.random.default_rng(22), 2, h, w)
        table = DA.empty_params(2)
        table[:, twin.DISTRIB] = 2
        DA.set_rectangles(table[0], all_but(h, w, kept))
        DA.set_rectangles(table[1], all_but(h, w, dropped))
        assert twin.keeps_resampled(kept, h * w) and not twin.keeps_resampled(dropped, h * w)
        m = check_resampling(DA, table, data, [True, False])
        assert m[0].sum() == kept


# ------------------------------------------------------------------------------------------------ composition
def test_augment_all_interp_equals_the_twins_composition(DA):
    n, h, w = 2, 64, 64
    data = inputs(np.random.default_rng(31), n, h, w)
    seen = set()
    for seed in (0, 1, 2):
        table = DA.draw_interp_params(np.random.default_rng(seed), n, h, w, num_distrib=3)
        seen |= {int(d) for d in table[:, twin.DISTRIB]}
        got = dict(zip(NAMES, DA.augment_all_interp(*data, params=table)))
        want = want_interp(table, data)
        for name in NAMES[1:]:
            assert same_bits(got[name], want[name]), (name, seed)
        keep = ~want["hazards"]
        assert (~keep).mean() <= 1e-3
        assert np.abs(got["image_a"].cpu().numpy() - want["image_a"])[keep].max() <= 1e-5, seed
    assert len(seen) >= 2
    # seed= draws the same table as the explicit call
    a = DA.augment_all_interp(*data, seed=5, num_distrib=3)
    b = DA.augment_all_interp(*data, params=DA.draw_interp_params(np.random.default_rng(5), n, h, w, num_distrib=3))
    assert all(same_bits(x, y.cpu().numpy()) for x, y in zip(a, b))


def test_augment_all_estimation_equals_the_twin(DA):
    n, h, w = 2, 64, 64
    rng = np.random.default_rng(32)
    img1, _, _, _, flow = inputs(rng, n, h, w)
    img2 = rng.random((n, h, w, 3), dtype=np.float32)
    for seed in (0, 1):
        ta, tb = DA.draw_estimation_params(np.random.default_rng(seed), n)
        g1, g2, gf = DA.augment_all_estimation(img1, img2, flow, params=(ta, tb))
        want = twin.apply(ta, tb, image_a=img1, image_b=img2, flow=flow)
        assert same_bits(gf, want["flow"])
        keep = ~want["hazards"]
        assert (~keep).mean() <= 1e-3
        assert np.abs(g1.cpu().numpy() - want["image_a"])[keep].max() <= 1e-5
        assert np.abs(g2.cpu().numpy() - want["image_b"])[keep].max() <= 1e-5
        assert not np.array_equal(tb[:, twin.D_HUE], ta[:, twin.D_HUE])  # each image its own colour record


# ------------------------------------------------------------------------------------------------ loader and trainer
@pytest.fixture(scope="module")
def records(tmp_path_factory):
    from src import tfrecord
    rng = np.random.default_rng(41)
    path = str(tmp_path_factory.mktemp("selflow") / "interp.tfrecords")
    samples = []
    with tfrecord.TFRecordWriter(path) as wr:
        for _ in range(2):
            img = rng.random((128, 128, 3))
            flow = np.clip(rng.standard_normal((128, 128, 2)) * 3, -20, 20).astype(np.float32)
            m = (rng.random((128, 128, 1)) < 0.05).astype(np.float64)
            sparse, edges = (flow * m).astype(np.float32), rng.random((128, 128, 1)).astype(np.float32)
            wr.write(tfrecord.encode_sample(img, flow=flow, matches_a=m, sparse_flow=sparse, edges_a=edges))
            samples.append((img.astype(np.float32), m.astype(np.float32), sparse, edges, flow))
    return path, samples


def first_batch(path, **kw):
    from src.dataloader import load_interp_batches
    return [t.cpu().numpy() for t in next(load_interp_batches(path, 2, (128, 128), epochs=1, **kw))]


def test_loader_augmentation_is_seeded_and_off_by_default(records):
    path, samples = records
    a = first_batch(path, seed=3, data_augmentation=True, num_distrib=3)
    b = first_batch(path, seed=3, data_augmentation=True, num_distrib=3)
    c = first_batch(path, seed=4, data_augmentation=True, num_distrib=3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, c))
    assert [x.shape[-1] for x in a] == [3, 1, 2, 1, 2] and 0.0 <= a[0].min() and a[0].max() <= 1.0
    # off: exactly what the loader gave before it had the switch -- the records, batched in the shuffled order
    today = first_batch(path, seed=3)
    off = first_batch(path, seed=3, data_augmentation=False)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(today, off))
    order = [0, 1] if np.array_equal(today[4][0], samples[0][4]) else [1, 0]
    for i in range(5):
        assert np.array_equal(today[i], np.stack([samples[k][i] for k in order]))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, today))
    # the validation form re-samples the matches and leaves image, edges and ground truth alone
    v = first_batch(path, seed=3, data_augmentation=True, split="valid", invalid_like=1, min_val=1)
    assert all(np.array_equal(v[i], today[i]) for i in (0, 3, 4)) and not np.array_equal(v[1], today[1])
    assert np.array_equal(v[2], np.where(v[1] == 1, today[4], np.float32(0)))


def test_pair_loader_selects_the_selflow_augmentation(DA, tmp_path):
    """load_batches(augmentation='selflow') = augment_all_estimation with a table drawn from the loader's stream; the
    plugin stays the default and 'selflow' keeps the frame size (no crop)."""
    from src import tfrecord
    from src.dataloader import load_batches
    rng = np.random.default_rng(51)
    path = str(tmp_path / "pairs.tfrecords")
    a, b = rng.random((2, 64, 96, 3)), rng.random((2, 64, 96, 3))
    flow = rng.standard_normal((2, 64, 96, 2)).astype(np.float32)
    with tfrecord.TFRecordWriter(path) as wr:
        for k in range(2):
            wr.write(tfrecord.encode_sample(a[k], image_b=b[k], flow=flow[k]))
    kw = dict(epochs=1, image_size=(64, 96))
    got = [t.cpu().numpy() for t in next(load_batches(path, 2, seed=7, augmentation="selflow", **kw))]
    again = [t.cpu().numpy() for t in next(load_batches(path, 2, seed=7, augmentation="selflow", **kw))]
    other = [t.cpu().numpy() for t in next(load_batches(path, 2, seed=8, augmentation="selflow", **kw))]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(got, other))
    assert [x.shape for x in got] == [(2, 64, 96, 3), (2, 64, 96, 3), (2, 64, 96, 2)]
    plain = [t.cpu().numpy() for t in next(load_batches(path, 2, data_augmentation=False, seed=7, **kw))]
    # the same stream: shuffle draws first, then the table
    stream = np.random.default_rng(7)
    stream.permutation(2)
    ta, tb = DA.draw_estimation_params(stream, 2)
    want = twin.apply(ta, tb, image_a=plain[0], image_b=plain[1], flow=plain[2])
    assert np.array_equal(bits(got[2]), bits(want["flow"]))
    keep = ~want["hazards"]
    assert (~keep).mean() <= 1e-3
    assert np.abs(got[0] - want["image_a"])[keep].max() <= 1e-5 and np.abs(got[1] - want["image_b"])[keep].max() <= 1e-5
    with pytest.raises(ValueError):
        next(load_batches(path, 2, augmentation="caffe", **kw))


def test_one_training_step_on_an_augmented_batch(records):
    import torch
    from src import weights as W
    from src.dataloader import load_interp_batches
    from src.trainer import FlowNetSTrainer
    path, _ = records
    wts = W.init_weights("FlowNetS_interp", 9)
    tr = FlowNetSTrainer(wts, 2, 128, 128, dtype="f32", model="FlowNetS_interp")
    img, matches, sparse, edges, flow = next(load_interp_batches(path, 2, (128, 128), seed=3, epochs=1,
                                                                 data_augmentation=True))
    loss = tr.forward_backward_interp(img, matches, sparse, flow, edges=edges)
    tr.apply_gradients()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss.item())) and tr.step_count == 1
