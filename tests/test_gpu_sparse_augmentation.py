"""Sparse ground truth through the 'selflow' and 'pair' augmentations (load_batches(sparse_gt=True, augmentation=...)):
fn2_selflow_apply moves a flow pixel whole and flips by negation, so a pixel without ground truth (NaN) stays with its pixel
and reaches no other.  The NaN set of the output is the flipped NaN set of the input, and every other pixel is what the
dense flow gives bit for bit."""
import numpy as np
import pytest

SEEDS = [0, 1, 2, 3]
N, H, W = 8, 12, 20


def inputs(seed):
    rng = np.random.default_rng([seed, 0xC809])
    x = rng.random((N, H, W, 3), dtype=np.float32)
    dense = rng.standard_normal((N, H, W, 2)).astype(np.float32)
    hole = rng.random((N, H, W)) < 0.3
    hole[:, 2:5, 3:9] = True                                        # a region, off-centre so that both flips move it
    hole[:, 0, 0] = True
    hole[:, H - 1, W - 2] = False
    sparse = dense.copy()
    sparse[hole] = np.nan
    sparse[0, 6, 7], sparse[1, 6, 7] = dense[0, 6, 7], dense[1, 6, 7]
    sparse[0, 6, 7, 0] = np.nan                                     # one component is enough to carry no label; the other
    sparse[1, 6, 7, 1] = np.nan                                     # keeps the dense value
    return x, dense, sparse


def flipped(mask, table):
    from src import data_augmentation as DA
    out = mask.copy()
    for i in range(len(mask)):
        if table[i, DA.FLIP_LR]:
            out[i] = out[i][:, ::-1]
        if table[i, DA.FLIP_UD]:
            out[i] = out[i][::-1]
    return out


def test_seeds_cover_both_flips_under_both_kinds_of_table():
    from src import data_augmentation as DA
    for shared in (False, True):
        t = np.concatenate([DA.draw_estimation_params(np.random.default_rng(s), N, shared_colour=shared)[0] for s in SEEDS])
        assert {(int(a), int(b)) for a, b in t[:, [DA.FLIP_LR, DA.FLIP_UD]]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    _, dense, sparse = inputs(0)
    hole = np.isnan(sparse)
    assert np.isfinite(dense).all() and 0.2 < hole.any(-1).mean() < 0.5
    assert not np.array_equal(hole[0], hole[0][:, ::-1]) and not np.array_equal(hole[0], hole[0][::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [False, True], ids=["selflow", "pair"])
@pytest.mark.parametrize("seed", SEEDS)
def test_a_pixel_without_ground_truth_stays_with_its_pixel(seed, shared):
    import torch
    from src import data_augmentation as DA
    x, dense, sparse = inputs(seed)
    y = np.roll(x, 1, 2)
    params = DA.draw_estimation_params(np.random.default_rng(seed), N, shared_colour=shared)
    a0, b0, f0 = DA.augment_all_estimation(x, y, dense, params=params)
    a1, b1, f1 = DA.augment_all_estimation(x, y, sparse, params=params)
    torch.cuda.synchronize()
    f0, f1 = f0.cpu().numpy(), f1.cpu().numpy()
    np.testing.assert_array_equal(a1.cpu().numpy(), a0.cpu().numpy())   # the frames do not see the flow
    np.testing.assert_array_equal(b1.cpu().numpy(), b0.cpu().numpy())
    assert np.isfinite(f0).all()
    for c in (0, 1):                                                # per component: a NaN in u alone stays in u alone
        np.testing.assert_array_equal(np.isnan(f1[..., c]), flipped(np.isnan(sparse[..., c]), params[0]))
    keep = ~np.isnan(f1)
    np.testing.assert_array_equal(f1[keep].view(np.uint32), f0[keep].view(np.uint32))
    assert not np.isinf(f1).any()
