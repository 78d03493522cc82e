"""Training input pipeline of the reference (src/dataloader.py:383-560 `load_batch`, src/dataset_configs.py)
over two sample sources: the reference's ZLIB TFRecord files (src/tfrecord.py reads them without TensorFlow) or a
text file listing `image_a image_b flow.flo` per line (the triples the TFRecords were built from); samples are
batched on the host, and the augmentation runs on the GPU through the preprocessing plugin's op surface (src/preprocessing.py):
DataAugmentation on both images (image b inherits image a's transform), FlowAugmentation on the ground truth.
The SelFlow-style augmentation the reference's loader itself applies (dataloader.py:35-113) is src/data_augmentation.py:
`load_interp_batches(data_augmentation=True)` and `load_batches(augmentation='selflow')` switch it on;
`load_batches(augmentation='pair')` is its pair-consistent variant for the unsupervised loss.

PREPROCESS values are the reference's FlyingChairs configuration (dataset_configs.py:60-157) as data.
"""
import numpy as np
import torch

from . import preprocessing as P
from .flowlib import read_flow, read_sparse_flow


def _p(rand_type, exp, mean, spread, prob=1.0):
    return {"rand_type": rand_type, "exp": exp, "mean": mean, "spread": spread, "prob": prob}


FLYING_CHAIRS_PREPROCESS = {
    "scale": False,
    "crop_height": 384,
    "crop_width": 448,
    "image_a": {
        "translate": _p("uniform_bernoulli", False, 0, 0.4),
        "rotate": _p("uniform_bernoulli", False, 0, 0.4),
        "zoom": _p("uniform_bernoulli", True, 0.2, 0.4),
        "squeeze": _p("uniform_bernoulli", True, 0, 0.3),
        "noise": _p("uniform_bernoulli", False, 0.03, 0.03),
    },
    # all preprocessing of image a is applied to image b in addition to the following
    "image_b": {
        "translate": _p("gaussian_bernoulli", False, 0, 0.03),
        "rotate": _p("gaussian_bernoulli", False, 0, 0.03),
        "zoom": _p("gaussian_bernoulli", True, 0, 0.03),
        "gamma": _p("gaussian_bernoulli", True, 0, 0.02),
        "brightness": _p("gaussian_bernoulli", False, 0, 0.02),
        "contrast": _p("gaussian_bernoulli", True, 0, 0.02),
        "color": _p("gaussian_bernoulli", True, 0, 0.02),
        "coeff_schedule_param": {"half_life": 50000, "initial_coeff": 0.5, "final_coeff": 1},
    },
}


def config_to_arrays(dataset_config):
    """dataloader.py:279-308: the per-parameter dict -> the parallel attribute lists of the op."""
    out = {"name": [], "rand_type": [], "exp": [], "mean": [], "spread": [], "prob": [], "coeff_schedule": []}
    for name, value in dataset_config.items():
        if name == "coeff_schedule_param":
            out["coeff_schedule"] = [value["half_life"], value["initial_coeff"], value["final_coeff"]]
        else:
            out["name"].append(name)
            for k in ("rand_type", "exp", "mean", "spread", "prob"):
                out[k].append(value[k])
    return out


def read_list(path, allow_unlabeled=False):
    """Rows of a list file: `image_a image_b flow.flo`; with allow_unlabeled also `image_a image_b` (unsupervised
    training needs no ground truth)."""
    with open(path) as f:
        rows = [ln.split() for ln in f.read().splitlines() if ln.strip()]
    for r in rows:
        if len(r) != 3 and not (allow_unlabeled and len(r) == 2):
            raise ValueError("expected `image_a image_b flow.flo`%s per line, got: %r"
                             % (" or `image_a image_b`" if allow_unlabeled else "", r))
    return rows


def crop_window(shape, crop, mode, rng, name="sample"):
    """(y0, x0) of the crop[0] x crop[1] window of a frame of shape[:2]: 'centre' (the one evaluate() cuts), or 'random'
    with y0 then x0 drawn from `rng` (one draw each, also where only one position exists).  Pure host arithmetic."""
    h, w = int(shape[0]), int(shape[1])
    ch, cw = crop
    if h < ch or w < cw:
        raise ValueError("%s is %dx%d: smaller than the crop %dx%d" % (name, h, w, ch, cw))
    if mode == "centre":
        return (h - ch) // 2, (w - cw) // 2
    return int(rng.integers(h - ch + 1)), int(rng.integers(w - cw + 1))


def check_crop(crop, crop_mode):
    """None, or (h, w) as two positive ints; crop_mode 'random' or 'centre'."""
    if crop_mode not in ("random", "centre"):
        raise ValueError("crop_mode must be 'random' or 'centre', got %r" % (crop_mode,))
    if crop is None:
        return None
    try:
        ch, cw = (int(v) for v in crop)
    except (TypeError, ValueError):
        raise ValueError("crop must be (height, width), got %r" % (crop,)) from None
    if ch < 1 or cw < 1:
        raise ValueError("crop must be (height, width) with both >= 1, got %r" % (crop,))
    return ch, cw


def _list_epoch(rows, rng, with_flow=True, sparse_gt=False, crop=None, crop_mode="random", crop_rng=None):
    """One epoch of (image_a, image_b, flow) host arrays from a list file, in a fresh random order; with_flow=False
    leaves the ground truth unread (flow is None).  sparse_gt reads the flow with read_sparse_flow (NaN where there is no
    ground truth); crop cuts one window out of both frames and the flow."""
    from .net import imread
    for j in rng.permutation(len(rows)):
        r = rows[j]
        smp = (imread(r[0]).astype(np.float32) / 255.0, imread(r[1]).astype(np.float32) / 255.0,
               (read_sparse_flow(r[2]) if sparse_gt else read_flow(r[2])) if with_flow else None)
        if crop is not None:
            smp = _crop_sample(smp, crop, crop_mode, crop_rng, r[0])
        yield smp


def _crop_sample(smp, crop, crop_mode, crop_rng, name):
    """The same window of both frames and the flow."""
    for x in smp[1:]:
        if x is not None and x.shape[:2] != smp[0].shape[:2]:
            raise ValueError("%s: the frames and the flow of a sample differ in size (%s, %s)"
                             % (name, smp[0].shape[:2], x.shape[:2]))
    y0, x0 = crop_window(smp[0].shape, crop, crop_mode, crop_rng, name)
    return tuple(None if x is None else x[y0:y0 + crop[0], x0:x0 + crop[1]] for x in smp)


def _tfrecord_epoch(path, rng, image_size, scale, shuffle_buffer):
    """One epoch over a TFRecord file of the reference's samples (src/tfrecord.py), shuffled through a bounded
    buffer like the reference's slim DatasetDataProvider queue (dataloader.py:444-451: common_queue_capacity)."""
    from . import tfrecord
    buf = []
    div = 255.0 if scale else 1.0  # records hold images already in [0,1] unless PREPROCESS['scale'] (dataloader.py:466)
    for smp in tfrecord.read_samples(path, image_size[0], image_size[1]):
        item = (smp["image_a"] / div, smp["image_b"] / div, smp["flow"])
        if len(buf) < shuffle_buffer:
            buf.append(item)
            continue
        k = int(rng.integers(len(buf)))
        out, buf[k] = buf[k], item
        yield out
    for k in rng.permutation(len(buf)):
        yield buf[k]


def is_tfrecord(path):
    return str(path).endswith((".tfrecords", ".tfrecord"))


def load_batches(list_path, batch_size, preprocess=FLYING_CHAIRS_PREPROCESS, data_augmentation=True, seed=0,
                 global_step=0, epochs=None, image_size=(384, 512), shuffle_buffer=256, augmentation="plugin",
                 fast_mode=False, allow_unlabeled=False, sparse_gt=False, crop=None, crop_mode="random"):
    """Generator of (image_a, image_b, flow) device tensors [B,h,w,3|3|2]; images in [0,1].  ``list_path`` is a
    text file of `image_a image_b flow.flo` triples or a ``.tfrecords`` file as the reference's converter writes it
    (``image_size`` = the dataset's PADDED_IMAGE_HEIGHT/WIDTH, dataset_configs.py:42-43).  With data_augmentation
    the crop is (crop_height, crop_width) and the flow is transformed with the two augmentation matrices
    (dataloader.py:480-540); without it the samples pass through unchanged.  ``augmentation='selflow'`` takes the
    augmentation the reference's live loader applies to image pairs instead of the plugin's (augment_all_estimation,
    dataloader.py:93-113 -> src/data_augmentation.py): flips, a channel permutation and a colour chain per image, no crop.
    ``allow_unlabeled`` (unsupervised training): a list file may hold `image_a image_b` lines, a third field is not read,
    and the batches are (image_a, image_b, None); 'plugin' and 'selflow' transform a ground truth and recolour the frames
    independently, so with them it needs data_augmentation=False.  ``augmentation='pair'`` is the one made for it (and fine
    on labeled lists, whose flow is flipped as under 'selflow'): selflow's flips and channel permutation with ONE colour
    record for both frames and no contrast stage (draw_estimation_params(shared_colour=True)), so equal pixels stay
    equal.
    ``sparse_gt`` (KITTI, HD1K, Middlebury): the third field of a list file is read with flowlib.read_sparse_flow -- a KITTI
    flow .png or a .flo with unknown pixels -- and the flow holds NaN where there is no ground truth.  'selflow' and 'pair'
    move a flow pixel whole and flip by negation, so a NaN stays with its pixel; the plugin augmentation interpolates the
    flow, where a NaN would spread, and is refused, as are .tfrecords files (their flow is dense).
    ``crop=(h, w)``: every sample of a list file is cut to one host window -- both frames and the flow alike -- before it
    is stacked, so frames of differing sizes (KITTI: 370..376 x 1224..1242) make one batch.  crop_mode 'random' draws the
    window from a generator of its own, so the sample order and the augmentation draws are what they are without a crop;
    'centre' is the window evaluate() cuts.  The plugin augmentation has its own crop and is refused."""
    if augmentation not in ("plugin", "selflow", "pair"):
        raise ValueError("augmentation must be 'plugin', 'selflow' or 'pair', got %r" % (augmentation,))
    if allow_unlabeled and data_augmentation and augmentation != "pair":
        raise ValueError("allow_unlabeled needs data_augmentation=False: the augmentations transform a ground truth")
    crop = check_crop(crop, crop_mode)
    plugin = bool(data_augmentation) and augmentation == "plugin"
    if sparse_gt and plugin:
        raise ValueError("sparse_gt does not go through the plugin augmentation (FlowAugmentation interpolates the flow and "
                         "a NaN would spread): use data_augmentation=False, augmentation='selflow' or 'pair'")
    if sparse_gt and is_tfrecord(list_path):
        raise ValueError("sparse_gt reads list files; the flow of a .tfrecords file is dense")
    if crop is not None and plugin:
        raise ValueError("crop does not combine with the plugin augmentation, which has its own crop "
                         "(preprocess['crop_height'], ['crop_width'])")
    if crop is not None and is_tfrecord(list_path):
        raise ValueError("crop cuts the samples of list files; the samples of a .tfrecords file share one size")
    crop_rng = np.random.default_rng([int(seed), 0xC809]) if crop is not None and crop_mode == "random" else None
    rng = np.random.default_rng(seed)
    unlabeled = bool(allow_unlabeled) and not is_tfrecord(list_path)
    rows = None if is_tfrecord(list_path) else read_list(list_path, allow_unlabeled)
    a_cfg, b_cfg = config_to_arrays(preprocess["image_a"]), config_to_arrays(preprocess["image_b"])
    plugin_crop = (preprocess["crop_height"], preprocess["crop_width"])
    epoch, step = 0, int(global_step)
    while epochs is None or epoch < epochs:
        source = _list_epoch(rows, rng, not unlabeled, bool(sparse_gt), crop, crop_mode,
                             crop_rng) if rows is not None else _tfrecord_epoch(
            list_path, rng, image_size, bool(preprocess.get("scale", False)), shuffle_buffer)
        pick = []
        produced = False
        for smp in source:
            pick.append(smp)
            if len(pick) < batch_size:
                continue
            a, b, f = (None if unlabeled and i == 2 else np.stack([p[i] for p in pick]).astype(np.float32)
                       for i in range(3))
            pick = []
            produced = True
            if not data_augmentation:
                dev = lambda x: None if x is None else torch.from_numpy(x).to(P._hip.require_device())
                yield dev(a), dev(b), dev(f)
            elif augmentation in ("selflow", "pair"):
                from . import data_augmentation as DA
                yield DA.augment_all_estimation(a, b, f, params=DA.draw_estimation_params(
                    rng, len(a), fast_mode=fast_mode, shared_colour=augmentation == "pair"))
            else:
                oa, ob, ta, itb = P.data_augmentation(
                    a, b, step, plugin_crop, a_cfg["name"], a_cfg["rand_type"], a_cfg["exp"], a_cfg["mean"], a_cfg["spread"],
                    a_cfg["prob"], a_cfg["coeff_schedule"], b_cfg["name"], b_cfg["rand_type"], b_cfg["exp"], b_cfg["mean"],
                    b_cfg["spread"], b_cfg["prob"], b_cfg["coeff_schedule"], seed=int(rng.integers(1 << 31)))
                if "noise" in preprocess["image_a"]:
                    # the plugin leaves noise to the Python side (augmentation_base.h:126): gaussian, sigma drawn per batch
                    n = preprocess["image_a"]["noise"]
                    sigma = abs(P.rng_generate(rng, n, 1.0, 0.0))
                    g = torch.Generator(device=oa.device).manual_seed(int(rng.integers(1 << 31)))
                    oa = (oa + sigma * torch.randn(oa.shape, generator=g, device=oa.device)).clamp_(0.0, 1.0)
                    ob = (ob + sigma * torch.randn(ob.shape, generator=g, device=ob.device)).clamp_(0.0, 1.0)
                yield oa, ob, P.flow_augmentation(f, ta, itb, plugin_crop)
            step += 1
        if not produced:
            raise ValueError("%s holds fewer than one batch (%d) of samples" % (list_path, batch_size))
        epoch += 1


def load_interp_batches(tfrecord_path, batch_size, image_size=(384, 512), seed=0, epochs=None, scale=False,
                        shuffle_buffer=256, data_augmentation=False, split="train", invalid_like=-1, num_distrib=2,
                        min_val=0, ff_like=-1):
    """Batches for FlowNetS_interp from the reference's `image_matches` records (dataloader.py:211-245: image_a and
    matches_a float64, sparse_flow / edges_a / flow float32, all at the dataset's padded size): device tensors
    (image_a [B,h,w,3], matches_a [B,h,w,1], sparse_flow [B,h,w,2], edges_a [B,h,w,1], flow [B,h,w,2]).
    With ``data_augmentation`` every batch goes through the reference's `augment_all_interp` (dataloader.py:35-80:
    re-sampling of the matches and the sparse flow, flips, channel permutation, colour chain) on the GPU
    (src/data_augmentation.py), or with ``split='valid'`` through `augment_all_interp_validation` (:83-90: re-sampling
    only), as dataloader.py:478-499 chooses; the decisions are drawn per sample from a stream of their own seeded by
    ``seed``, so the order of the samples does not depend on the switch.  Off (the default), the records pass through."""
    from . import tfrecord
    if split not in ("train", "valid"):
        raise ValueError("split must be 'train' or 'valid', got %r" % (split,))
    names = ("image_a", "matches_a", "sparse_flow", "edges_a", "flow")
    rng = np.random.default_rng(seed)
    aug_rng = np.random.default_rng([int(seed), 0x5E1F]) if data_augmentation else None
    div = 255.0 if scale else 1.0
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(P._hip.require_device())
    epoch = 0
    while epochs is None or epoch < epochs:
        buf, pick, produced = [], [], False

        def emit(items):
            batch = tuple(dev(np.stack([it[i] for it in items]).astype(np.float32)) for i in range(5))
            if not data_augmentation:
                return batch
            from . import data_augmentation as DA
            n, h, w = batch[0].shape[:3]
            if split == "train":
                return DA.augment_all_interp(*batch, params=DA.draw_interp_params(
                    aug_rng, n, h, w, invalid_like, num_distrib, min_val, ff_like))
            return DA.augment_all_interp_validation(*batch, params=DA.draw_validation_params(
                aug_rng, n, h, w, invalid_like, num_distrib, min_val, ff_like))

        def samples():
            for smp in tfrecord.read_samples(tfrecord_path, image_size[0], image_size[1], names):
                item = (smp["image_a"] / div, smp["matches_a"] / div, smp["sparse_flow"], smp["edges_a"], smp["flow"])
                if len(buf) < shuffle_buffer:
                    buf.append(item)
                    continue
                k = int(rng.integers(len(buf)))
                out, buf[k] = buf[k], item
                yield out
            for k in rng.permutation(len(buf)):
                yield buf[k]

        for item in samples():
            pick.append(item)
            if len(pick) == batch_size:
                yield emit(pick)
                pick, produced = [], True
        if not produced:
            raise ValueError("%s holds fewer than one batch (%d) of samples" % (tfrecord_path, batch_size))
        epoch += 1
