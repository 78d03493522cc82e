"""The augmentation the reference's loader trains with (src/data_augmentation.py + dataloader.py:35-113 there) on
the GPU: re-sampling of the match mask and sparse flow, random flips with their flow signs, a random channel
permutation and one of four colour-distortion chains, through two library calls per batch (fn2_selflow_stats,
fn2_selflow_apply; csrc/selflow_aug.hip).

Every random decision is drawn here, per sample (the reference augments before batching), into a table of
PARAM_WORDS 32-bit words per sample (layout: include/flownet2_hip.h, FN2_SF_*); the kernels are deterministic
functions of their inputs and that table.  The draws restate the reference's TensorFlow graph in float32; its random
streams are not reproduced.  `perturbate_dm_matches` and `sample_sparse_grid_like` are never called by the reference
and are not built; `random_crop` is commented out there.
"""
import math

import numpy as np
import torch

from . import _hip

PARAM_WORDS = 32
(DISTRIB, THRESHOLD, KEY0, KEY1, N_RECT, RECTS, FLIP_LR, FLIP_UD, PERM, COLOUR_ORDER, D_BRIGHTNESS, F_SATURATION, D_HUE,
 F_CONTRAST) = 0, 1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 22, 23, 24
DISTRIB_DM, DISTRIB_UNIFORM, DISTRIB_INVALID_LIKE = 0, 1, 2

CHANNEL_PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))  # data_augmentation.py:163-168
ASPECT_RATIOS = (16 / 9, 4 / 3, 3 / 2, 3 / 1, 4 / 5)                                      # :241
DENSE_RANGES = ((10.0, 25.0), (25.0, 50.0), (50.0, 75.0), (75.0, 90.0))                   # case_dense :203-220
SPARSE_RANGES = ((0.01, 1.0), (1.0, 10.0))                                                # case_sparse :193-200
FF_LIKE_RANGE = (65.0, 85.0)
# distort_colour's ranges (:68-73): brightness delta, saturation factor, hue delta, contrast factor
COLOUR_RANGES = {"d_brightness": (-51.0 / 255.0, 51.0 / 255.0), "f_saturation": (0.5, 1.5), "d_hue": (-0.2, 0.2),
                 "f_contrast": (0.2, 1.4)}
MIN_PERCENTAGE = 0.01  # sample_from_distribution :514
_COLOUR_WORDS = [COLOUR_ORDER, D_BRIGHTNESS, F_SATURATION, D_HUE, F_CONTRAST]

_f32 = np.float32


def _uniform32(rng, lo, hi):
    """tf.random_uniform([], lo, hi, float32): u * (hi - lo) + lo in float32, u in [0, 1); never hi itself."""
    lo, hi = _f32(lo), _f32(hi)
    v = _f32(rng.random(dtype=np.float32)) * (hi - lo) + lo
    return v if v < hi else np.nextafter(hi, lo, dtype=np.float32)


def density_threshold(density):
    """The uint32 the hash is compared with: min(floor(p * 2^32), 2^32 - 1), p = density / 100 in float32."""
    p = _f32(density) / _f32(100.0)
    return int(min(max(math.floor(float(p) * 4294967296.0), 0), 4294967295))


def get_sampling_density(rng, dense_or_sparse, num_ranges=(4, 2), ff_like=-1):
    """:193-228.  The range id is drawn in either case, as case_dense does before it looks at ff_like."""
    if dense_or_sparse > 0:
        k = int(rng.integers(num_ranges[0]))
        lo, hi = FF_LIKE_RANGE if ff_like > 0 else DENSE_RANGES[k]
    else:
        lo, hi = SPARSE_RANGES[int(rng.integers(num_ranges[1]))]
    return _uniform32(rng, lo, hi)


def crop_size(height, width, density, aspect_ratio):
    """The rectangle of get_random_offset_and_crop (:238-255) for one aspect ratio, in float32: tf.round is
    round-half-to-even, and a side LARGER than the image becomes size - 1 (not size)."""
    ar = _f32(aspect_ratio)
    bbox_area = (_f32(density) / _f32(100.0)) * _f32(height * width)
    crop_w = int(np.rint(np.sqrt(_f32(bbox_area * ar))))
    crop_h = int(np.rint(_f32(crop_w) / ar))
    if crop_h > height:
        crop_h = height - 1
    if crop_w > width:
        crop_w = width - 1
    return crop_h, crop_w


def get_random_offset_and_crop(rng, image_shape, density):
    """:231-260 -> (offset_h, offset_w, crop_h, crop_w); offsets uniform in [0, size - crop + 1)."""
    height, width = image_shape
    crop_h, crop_w = crop_size(height, width, density, ASPECT_RATIOS[int(rng.integers(len(ASPECT_RATIOS)))])
    off_h = int(rng.integers(0, height - crop_h + 1))
    off_w = int(rng.integers(0, width - crop_w + 1))
    return off_h, off_w, crop_h, crop_w


def _corrupt_once(rng, density, height, width):
    """corrupt_sparse_flow_once (:307-313): a hole at density / U[4, 12)."""
    inv_fraction = _uniform32(rng, 4.0, 12.0)
    return get_random_offset_and_crop(rng, (height, width), _f32(density) / inv_fraction)


def invalid_like_rectangles(rng, density, height, width):
    """sample_sparse_invalid_like (:452-460) + corrupt_sparse_flow_loop (:287-304): one hole at the drawn density, one at
    density * 2/3 / U[4, 12), a third like the second with probability 1/2."""
    rects = [get_random_offset_and_crop(rng, (height, width), density)]
    reduced = _f32(density) * _f32(2 / 3)
    rects.append(_corrupt_once(rng, reduced, height, width))
    if int(rng.integers(2)) > 0:
        rects.append(_corrupt_once(rng, reduced, height, width))
    return rects


def empty_params(n):
    """n records that change nothing: DeepMatching inputs kept, no flip, identity permutation, no colour."""
    t = np.zeros((n, PARAM_WORDS), np.uint32)
    t.view(np.int32)[:, COLOUR_ORDER] = -1
    return t


def set_colour(record, order, d_brightness=0.0, f_saturation=1.0, d_hue=0.0, f_contrast=1.0):
    record.view(np.int32)[COLOUR_ORDER] = order
    record.view(np.float32)[[D_BRIGHTNESS, F_SATURATION, D_HUE, F_CONTRAST]] = (d_brightness, f_saturation, d_hue, f_contrast)


def set_rectangles(record, rects):
    if len(rects) > 3:
        raise ValueError("at most three rectangles, got %d" % len(rects))
    record[N_RECT] = len(rects)
    record.view(np.int32)[RECTS:RECTS + 12] = 0
    for r, rect in enumerate(rects):
        record.view(np.int32)[RECTS + 4 * r:RECTS + 4 * r + 4] = rect


def _draw_sampling(rng, record, height, width, invalid_like, num_distrib, min_val, ff_like):
    """sample_sparse_flow (:526-558) for one sample."""
    dense_or_sparse = int(rng.integers(min_val, 2))
    density = get_sampling_density(rng, dense_or_sparse, ff_like=ff_like)
    distrib = DISTRIB_INVALID_LIKE if invalid_like > 0 else int(rng.integers(num_distrib))
    record[DISTRIB] = distrib
    if distrib == DISTRIB_UNIFORM:
        record[THRESHOLD] = density_threshold(density)
        record[KEY0], record[KEY1] = rng.integers(0, 1 << 32, size=2, dtype=np.uint32)
    elif distrib == DISTRIB_INVALID_LIKE:
        set_rectangles(record, invalid_like_rectangles(rng, density, height, width))
    return density


def _draw_colour(rng, record, fast_mode):
    """distort_colour (:67-91): the chain id (one chain under fast_mode) and the four random_* draws."""
    order = int(rng.integers(1 if fast_mode else 4))
    set_colour(record, order, **{k: _uniform32(rng, lo, hi) for k, (lo, hi) in COLOUR_RANGES.items()})


def _check_sampling_args(num_distrib, min_val):
    if min_val not in (0, 1):
        raise ValueError("min_val must be 0 (dense and sparse ranges) or 1 (dense only), got %r" % (min_val,))
    if num_distrib not in (1, 2, 3):
        raise ValueError("num_distrib must be 1, 2 or 3, got %r" % (num_distrib,))


def draw_interp_params(rng, n, height, width, invalid_like=-1, num_distrib=2, min_val=0, ff_like=-1, fast_mode=False):
    """The table of augment_all_interp (dataloader.py:35-80) for n samples of height x width: uint32 [n, PARAM_WORDS]."""
    _check_sampling_args(num_distrib, min_val)
    table = empty_params(n)
    for rec in table:
        _draw_sampling(rng, rec, height, width, invalid_like, num_distrib, min_val, ff_like)
        rec[FLIP_LR], rec[FLIP_UD] = rng.integers(0, 2, size=2)
        rec[PERM] = rng.integers(6)
        _draw_colour(rng, rec, fast_mode)
    return table


def draw_validation_params(rng, n, height, width, invalid_like=1, num_distrib=2, min_val=1, ff_like=-1):
    """The table of augment_all_interp_validation (dataloader.py:83-90): re-sampling only."""
    _check_sampling_args(num_distrib, min_val)
    table = empty_params(n)
    for rec in table:
        _draw_sampling(rng, rec, height, width, invalid_like, num_distrib, min_val, ff_like)
    return table


def draw_estimation_params(rng, n, height=None, width=None, fast_mode=False, shared_colour=False):
    """The tables of augment_all_estimation (dataloader.py:93-113): (table_a, table_b).  Flips and permutation are
    shared (both tables carry them), each image has its own colour record.

    shared_colour (not in the reference; the 'pair' augmentation of unsupervised training): ONE colour record per sample,
    copied into both tables, with f_contrast = 1.  Brightness, saturation and hue act on a pixel alone, so one record
    maps equal pixels of the two frames to equal pixels; contrast is the one stage that reads a per-frame statistic (the
    mean), and a shared factor around two different means would still shift one frame against the other -- factor 1
    makes the stage the identity."""
    a, b = empty_params(n), empty_params(n)
    for ra, rb in zip(a, b):
        ra[FLIP_LR], ra[FLIP_UD] = rng.integers(0, 2, size=2)
        ra[PERM] = rng.integers(6)
        rb[[FLIP_LR, FLIP_UD, PERM]] = ra[[FLIP_LR, FLIP_UD, PERM]]
        _draw_colour(rng, ra, fast_mode)
        if shared_colour:
            ra.view(np.float32)[F_CONTRAST] = 1.0
            rb[_COLOUR_WORDS] = ra[_COLOUR_WORDS]
        else:
            _draw_colour(rng, rb, fast_mode)
    return a, b


# ------------------------------------------------------------------------------------------------ device side
def _table(params, n):
    t = np.ascontiguousarray(params)
    if t.dtype != np.uint32 or t.shape != (n, PARAM_WORDS):
        raise ValueError("parameter table must be uint32 [%d, %d], got %s %s" % (n, PARAM_WORDS, t.dtype, t.shape))
    return t


def _upload(table, dev):
    return torch.from_numpy(table.view(np.int32)).to(dev)


def _needs_stats(table):
    return bool((table[:, DISTRIB] != 0).any() or (table.view(np.int32)[:, COLOUR_ORDER] >= 0).any())


def apply_params(params, params_b=None, image_a=None, image_b=None, matches=None, sparse_flow=None, edges=None, flow=None,
                 write_flow=True):
    """fn2_selflow_stats + fn2_selflow_apply on whichever of the six batch tensors are given; returns the augmented
    ones in the same order (None where none was given).  `flow` is read for the re-sampling even when write_flow is off."""
    dev = _hip.require_device()
    given = [image_a, image_b, matches, sparse_flow, edges, flow]
    chans = (3, 3, 1, 2, 1, 2)
    tens = [None if t is None else _hip.to_device_f32(t)[0] for t in given]
    shapes = {tuple(t.shape[:3]) for t in tens if t is not None}
    if len(shapes) != 1:
        raise ValueError("the batch tensors must share [n, h, w], got %s" % sorted(shapes))
    n, h, w = shapes.pop()
    for t, c in zip(tens, chans):
        if t is not None and (t.dim() != 4 or t.shape[3] != c):
            raise ValueError("expected [n, h, w, %d], got %s" % (c, tuple(t.shape)))
    table = _table(params, n)
    table_b = None if params_b is None else _table(params_b, n)
    if tens[1] is not None and table_b is None:
        raise ValueError("image_b needs its own colour records (params_b)")
    if (table[:, DISTRIB] != 0).any() and (tens[2] is not None or tens[3] is not None) and tens[5] is None:
        raise ValueError("re-sampling the matches needs the ground-truth flow")
    lib, st = _hip.lib(), _hip.stream_ptr()
    need = int(lib.fn2_selflow_workspace_bytes(n, h, w))
    if need < 0:
        raise ValueError("bad batch size n=%d h=%d w=%d" % (n, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    d_par = _upload(table, dev)
    d_par_b = None if table_b is None else _upload(table_b, dev)
    P_ = lambda t: None if t is None else _hip.ptr(t)
    if _needs_stats(table) or (table_b is not None and _needs_stats(table_b)):
        _hip.check(lib.fn2_selflow_stats(P_(tens[0]), P_(tens[1]), P_(d_par), P_(d_par_b), P_(ws), need, n, h, w, st))
    outs = [None if t is None else torch.empty_like(t) for t in tens]
    if not write_flow:
        outs[5] = None
    _hip.check(lib.fn2_selflow_apply(*[P_(t) for t in tens], *[P_(t) for t in outs], P_(d_par), P_(d_par_b), P_(ws), need,
                                     n, h, w, st))
    return outs


def _only(params, words):
    """A copy of the table with every stage but the listed words switched off."""
    t = empty_params(len(params))
    t[:, words] = np.asarray(params)[:, words]
    return t


_SAMPLING_WORDS = list(range(DISTRIB, RECTS + 12))


def _rng(seed):
    return np.random.default_rng(seed)


def sample_sparse_flow(dm_matches, dm_flow, gt_flow, params=None, seed=None, num_distrib=2, invalid_like=-1, min_val=0,
                       ff_like=-1):
    """data_augmentation.py:526-558 on batches -> (matches, sparse_flow).  `params`: a table whose re-sampling fields
    are used; else one is drawn from `seed`."""
    n, h, w = dm_matches.shape[:3]
    if params is None:
        params = draw_validation_params(_rng(seed), n, h, w, invalid_like, num_distrib, min_val, ff_like)
    out = apply_params(_only(params, _SAMPLING_WORDS), matches=dm_matches, sparse_flow=dm_flow, flow=gt_flow,
                       write_flow=False)
    return out[2], out[3]


def random_flip_with_flow(img_list, flow_list, params=None, seed=None):
    """:132-140 on batches: every image (1 or 3 channels) and every flow flipped by the same per-sample decisions, u
    negated under flip_lr and v under flip_ud."""
    first = (list(img_list) + list(flow_list))[0]
    n = first.shape[0]
    if params is None:
        params = empty_params(n)
        params[:, [FLIP_LR, FLIP_UD]] = _rng(seed).integers(0, 2, size=(n, 2))
    t = _only(params, [FLIP_LR, FLIP_UD])
    slots = {3: ("image_a", "image_b"), 1: ("matches", "edges"), 2: ("sparse_flow", "flow")}
    order = ("image_a", "image_b", "matches", "sparse_flow", "edges", "flow")
    items = list(img_list) + list(flow_list)
    results = [None] * len(items)
    todo = list(range(len(items)))
    while todo:
        call, free, rest = {}, {c: list(s) for c, s in slots.items()}, []
        for k in todo:
            c = items[k].shape[-1]
            if c not in free:
                raise ValueError("images have 1 or 3 channels and flows 2, got %d" % c)
            if free[c]:
                call[free[c].pop(0)] = k
            else:
                rest.append(k)
        out = apply_params(t, t if "image_b" in call else None, **{name: items[k] for name, k in call.items()})
        for name, k in call.items():
            results[k] = out[order.index(name)]
        todo = rest
    return results[:len(img_list)], results[len(img_list):]


def random_channel_swap(img_list, params=None, seed=None):
    """:143-159 on batches: one permutation per sample for every image of the list."""
    n = img_list[0].shape[0]
    if params is None:
        params = empty_params(n)
        params[:, PERM] = _rng(seed).integers(6, size=n)
    t = _only(params, [PERM])
    out = []
    for k in range(0, len(img_list), 2):
        pair = list(img_list[k:k + 2])
        res = apply_params(t, t if len(pair) == 2 else None, image_a=pair[0], image_b=pair[1] if len(pair) == 2 else None)
        out += res[:len(pair)]
    return out


def distort_colour(image, params=None, seed=None, num_permutations=4):
    """:67-91 on a batch: one of the chains per sample, clipped to [0, 1] at the end."""
    n = image.shape[0]
    if params is None:
        params, rng = empty_params(n), _rng(seed)
        for rec in params:
            _draw_colour(rng, rec, num_permutations == 1)
    return apply_params(_only(params, _COLOUR_WORDS), image_a=image)[0]


def augment_all_interp(image, matches, sparse_flow, edges, gt_flow, params=None, seed=None, fast_mode=False,
                       invalid_like=-1, num_distrib=2, min_val=0, ff_like=-1):
    """dataloader.py:35-80 on batches -> (image, matches, sparse_flow, edges, gt_flow)."""
    n, h, w = image.shape[:3]
    if params is None:
        params = draw_interp_params(_rng(seed), n, h, w, invalid_like, num_distrib, min_val, ff_like, fast_mode)
    out = apply_params(params, image_a=image, matches=matches, sparse_flow=sparse_flow, edges=edges, flow=gt_flow)
    return out[0], out[2], out[3], out[4], out[5]


def augment_all_interp_validation(image, matches, sparse_flow, edges, gt_flow, params=None, seed=None, invalid_like=1,
                                  num_distrib=2, min_val=1, ff_like=-1):
    """dataloader.py:83-90 on batches: the matches re-sampled, everything else as it came."""
    matches, sparse_flow = sample_sparse_flow(matches, sparse_flow, gt_flow, params, seed, num_distrib, invalid_like,
                                              min_val, ff_like)
    return image, matches, sparse_flow, edges, gt_flow


def augment_all_estimation(image1, image2, gt_flow, params=None, seed=None, fast_mode=False):
    """dataloader.py:93-113 on batches -> (image1, image2, gt_flow); `params` = (table_a, table_b)."""
    if params is None:
        params = draw_estimation_params(_rng(seed), image1.shape[0], fast_mode=fast_mode)
    out = apply_params(params[0], params[1], image_a=image1, image_b=image2, flow=gt_flow)
    return out[0], out[1], out[5]
