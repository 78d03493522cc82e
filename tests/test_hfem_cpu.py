"""Hard-flow-example mining without a GPU: the rounding of the number of hard pixels, the NumPy twin of the selection
against the oracle's loss, and the argument checks of the Python op and of the library entry points (which run before
any launch)."""
import ctypes as C

import numpy as np
import pytest

import hfem_twin as twin
from oracle import models as refm


@pytest.fixture(scope="module")
def hip():
    from src import _hip
    return _hip


def test_hard_k_is_the_oracles_rounding():
    from src.losses import hard_k
    assert hard_k(15, 50) == 8 and hard_k(5, 50) == 2  # 7.5 and 2.5: half to even
    assert hard_k(7, 0) == 0 and hard_k(7, 100) == 7
    for numel in list(range(1, 70)) + [126, 384, 4290, 18432, 98304, 229376]:
        for perc in (0, 1, 12.5, 25, 33, 50, 66.6, 75, 99, 100):
            want = int(np.round(np.float32(perc / 100) * np.float32(numel)))
            assert hard_k(numel, perc) == want == twin.oracle_hard_k(numel, perc), (numel, perc)
            assert 0 <= want <= numel


@pytest.mark.parametrize("ties", [False, True])
def test_twin_mask_reproduces_the_oracle_loss(ties):
    """(1 + lambda) / N * #pixels / k * sum of the EPE under the twin's mask == average_endpoint_error_hfem 'hard'; with
    ties the sum does not depend on which of the equal values are taken, but the mask must hold exactly k of them."""
    rng = np.random.default_rng(3)
    lab = rng.standard_normal((2, 6, 7, 2))
    pred = rng.standard_normal((2, 6, 7, 2))
    if ties:
        lab, pred = np.round(lab), np.round(pred)
    d = lab - pred
    epe = np.sqrt((d * d).sum(axis=3))
    for perc in (10, 33, 50, 100):
        k = twin.oracle_hard_k(epe.size, perc)
        mask = twin.stable_topk_mask(epe, k)
        assert mask.shape == epe.shape and int(mask.sum()) == k
        got = (1.0 + 2.0) * epe[mask].sum() / 2 * (epe.size / max(k, 1))
        want = refm.average_endpoint_error_hfem(lab, pred, "hard", 2.0, perc)
        assert got == pytest.approx(want, rel=1e-12)


def test_twin_takes_ties_in_index_order_and_nan_first():
    assert twin.stable_topk_mask(np.array([1., 1., 1., 1.]), 2).tolist() == [True, True, False, False]
    assert twin.stable_topk_mask(np.array([1., 2., 1., 2., 2.]), 2).tolist() == [False, True, False, True, False]
    assert twin.stable_topk_mask(np.array([1., np.inf, np.nan, 0.]), 1).tolist() == [False, False, True, False]
    assert twin.stable_topk_mask(np.array([1., np.inf, np.nan, 0.]), 2).tolist() == [False, True, True, False]
    assert not twin.stable_topk_mask(np.ones((2, 3)), 0).any() and twin.stable_topk_mask(np.ones((2, 3)), 6).all()


def test_hard_example_weights_rejects_bad_arguments_before_touching_a_device():
    import torch
    from src.losses import hard_example_weights
    a, b = torch.zeros(1, 3, 5, 2), torch.zeros(1, 3, 5, 2)
    for perc in (-1, 100.5, float("nan")):
        with pytest.raises(ValueError, match="perc_hfem"):
            hard_example_weights(a, b, perc_hfem=perc)
    with pytest.raises(ValueError, match=r"\[N, H, W, 2\]"):
        hard_example_weights(a, torch.zeros(1, 3, 4, 2))
    with pytest.raises(ValueError, match=r"\[N, H, W, 2\]"):
        hard_example_weights(torch.zeros(1, 3, 5, 3), torch.zeros(1, 3, 5, 3))
    with pytest.raises(ValueError, match=r"\[N, H, W, 2\]"):
        hard_example_weights(torch.zeros(3, 5, 2), torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match="device tensors"):
        hard_example_weights(a, b)  # CPU tensors
    with pytest.raises(ValueError, match="device tensors"):
        hard_example_weights(a.numpy(), b.numpy())


def test_library_rejects_bad_level_tables(hip):
    """Every check sits in front of the launch: nothing here reaches a device (the pointers are never followed)."""
    lib = hip.lib()
    L = hip.Fn2HfemLevel
    fake = 0x1000
    ok = lambda **kw: L(**dict(dict(pred=fake, label=fake, epe=fake, weight=fake, npix=8, k=4, hard_weight=1.0), **kw))
    assert lib.fn2_hfem_hard_weights(None, 1, None) == hip.ERR_INVALID_ARGUMENT
    for field in ("pred", "label", "epe", "weight"):
        assert lib.fn2_hfem_hard_weights(ok(**{field: None}), 1, None) == hip.ERR_INVALID_ARGUMENT
        assert b"null pointer" in lib.fn2_last_error()
    assert lib.fn2_hfem_hard_weights(ok(k=9), 1, None) == hip.ERR_INVALID_ARGUMENT  # k > npix
    assert b"k = 9" in lib.fn2_last_error()
    assert lib.fn2_hfem_hard_weights(ok(k=-1), 1, None) == hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_hfem_hard_weights(ok(npix=0, k=0), 1, None) == hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_hfem_hard_weights(ok(), 0, None) == hip.ERR_INVALID_ARGUMENT
    assert b"n_levels" in lib.fn2_last_error()
    table = (L * 9)(*[ok() for _ in range(9)])
    assert lib.fn2_hfem_hard_weights(table, 9, None) == hip.ERR_INVALID_ARGUMENT
    # a bad entry behind good ones is found too
    table = (L * 3)(ok(), ok(), ok(k=9))
    assert lib.fn2_hfem_hard_weights(table, 3, None) == hip.ERR_INVALID_ARGUMENT and b"level 2" in lib.fn2_last_error()
    assert lib.fn2_hfem_edge_weights(None, 2.0, fake, 8, None) == hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_hfem_edge_weights(fake, 2.0, None, 8, None) == hip.ERR_INVALID_ARGUMENT
    assert lib.fn2_hfem_edge_weights(fake, 2.0, fake, 0, None) == hip.ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        hip.check(lib.fn2_hfem_hard_weights(ok(k=9), 1, None))


def test_level_struct_matches_the_header_layout(hip):
    """fn2_hfem_level: four pointers, two int64, one float (padded to 8): 56 bytes, as the C side lays it out."""
    assert C.sizeof(hip.Fn2HfemLevel) == 56
    assert hip.Fn2HfemLevel.npix.offset == 32 and hip.Fn2HfemLevel.k.offset == 40 and hip.Fn2HfemLevel.hard_weight.offset == 48
