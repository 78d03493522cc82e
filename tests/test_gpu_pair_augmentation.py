"""The pair-consistent augmentation of unsupervised training (draw_estimation_params(shared_colour=True),
load_batches(augmentation='pair')) on the device: it draws no new kernel, only other tables for fn2_selflow_apply, so what has
to hold is that EQUAL frames stay equal -- brightness constancy survives -- for every colour chain and flip, that the
independent draws of 'selflow' do not have that property (the test can fail), and that a ground-truth flow is flipped as
before."""
import os

import numpy as np
import pytest

SEEDS = [0, 1, 2, 3]
N, H, W = 8, 12, 20
SAMPLES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "samples")


def frame(seed):
    return np.random.default_rng([seed, 77]).random((N, H, W, 3), dtype=np.float32)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_seeds_cover_every_chain_order_and_both_flips():
    from src import data_augmentation as DA
    tables = [DA.draw_estimation_params(np.random.default_rng(s), N, shared_colour=True)[0] for s in SEEDS]
    t = np.concatenate(tables)
    assert set(t.view(np.int32)[:, DA.COLOUR_ORDER].tolist()) == {0, 1, 2, 3}
    assert {(int(a), int(b)) for a, b in t[:, [DA.FLIP_LR, DA.FLIP_UD]]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert len(set(t[:, DA.PERM].tolist())) == 6


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_equal_frames_stay_equal_under_pair_tables_and_not_under_selflow_tables(seed):
    from src import data_augmentation as DA
    x = frame(seed)
    pair = DA.draw_estimation_params(np.random.default_rng(seed), N, shared_colour=True)
    a, b, f = DA.augment_all_estimation(x, x, None, params=pair)
    a, b = host(a), host(b)
    assert f is None and a.shape == x.shape
    np.testing.assert_array_equal(a, b)
    assert np.isfinite(a).all() and a.min() >= 0.0 and a.max() <= 1.0 and not np.array_equal(a, x)
    own = DA.draw_estimation_params(np.random.default_rng(seed), N)
    a2, b2, _ = DA.augment_all_estimation(x, x, None, params=own)
    a2, b2 = host(a2), host(b2)
    assert not np.array_equal(a2, b2)
    assert all(not np.array_equal(a2[i], b2[i]) for i in range(N))  # every sample's two frames were recoloured apart


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS[:2])
def test_flow_is_flipped_as_under_selflow(seed):
    from src import data_augmentation as DA
    x = frame(seed)
    flow = np.random.default_rng([seed, 78]).standard_normal((N, H, W, 2)).astype(np.float32)
    pair = DA.draw_estimation_params(np.random.default_rng(seed), N, shared_colour=True)
    own = DA.draw_estimation_params(np.random.default_rng(seed + 100), N)
    words = [DA.FLIP_LR, DA.FLIP_UD, DA.PERM]
    for t in own:
        t[:, words] = pair[0][:, words]
    got = host(DA.augment_all_estimation(x, x, flow, params=pair)[2])
    np.testing.assert_array_equal(got, host(DA.augment_all_estimation(x, x, flow, params=own)[2]))
    want = flow.copy()
    for i in range(N):
        if pair[0][i, DA.FLIP_LR]:
            want[i] = want[i, :, ::-1] * np.float32([-1, 1])
        if pair[0][i, DA.FLIP_UD]:
            want[i] = want[i, ::-1] * np.float32([1, -1])
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_loader_yields_pair_batches_from_an_unlabeled_list(tmp_path):
    import torch
    from src.dataloader import load_batches
    lst = tmp_path / "pairs.txt"
    lst.write_text("%s %s\n" % (os.path.join(SAMPLES, "0img0.ppm"), os.path.join(SAMPLES, "0img0.ppm")))
    a, b, f = next(load_batches(str(lst), 1, allow_unlabeled=True, augmentation="pair", seed=4))
    assert f is None and a.is_cuda and a.shape == b.shape and a.shape[0] == 1 and a.shape[3] == 3
    assert torch.equal(a, b)                                       # the same file twice: the frames stay equal
    a2, b2, f2 = next(load_batches(str(lst), 1, allow_unlabeled=True, augmentation="pair", seed=5))
    assert not torch.equal(a, a2)
