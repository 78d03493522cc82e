"""The loss stage of a FlowNetSTrainer step: the launches between the forward pass and the first backward launch, and the
buffers they write.  One stage per loss; the eager step (forward_backward*) and segment 0 of the captured step call the
same stage.launch(stream), so they issue one launch sequence.

  alloc()   allocates everything the loss writes; idempotent, runs before the step's zeroing and before any capture
  launch(s) the loss and its gradient at every scale of trainer.loss_terms, into the trainer's _gbuf(prediction) and
            loss_dev (both zeroed by the step); trainer.lib is read at every launch, not when the stage is built
  zeroed    the device buffers of the stage that the step's zeroing has to clear as well (counters)"""
import torch

from . import _hip, census, losses, photometric, sparse_epe


class _Stage:
    """What the stages share: per loss scale (name, prediction, its gradient buffer, loss weight), and for the supervised
    ones the labels downsample(gt_scale * gt) -- the scaling (flownet_s.py:123) happens per sample inside the op."""

    def __init__(self, trainer):
        self.tr, self.names, self.levels, self.zeroed = trainer, list(trainer.loss_terms), None, []

    def alloc(self):
        if self.levels is None:
            tr = self.tr
            levels = [(p, tr.eng.outputs[p], tr._gbuf(tr.eng.outputs[p]), wgt) for p, wgt in tr.loss_terms.items()]
            self._alloc(levels)
            self.levels = levels  # (behind _alloc: a stage that refused its shapes refuses them again)

    def _new(self, *shape, dtype=torch.float32):
        return torch.zeros(shape, dtype=dtype, device=self.tr.dev)

    def _alloc_labels(self, levels):
        self.labels = {p: torch.empty_like(pred) for p, pred, _g, _wgt in levels}

    def _label(self, p, pred, s):
        # (the labels depend on the input only; as a parallel path of the graph beside the forward pass: 5.24 -> 5.29 ms,
        # its two graph edges cost more than the 0.15 ms of small launches they would hide)
        tr, (n, h, w, _) = self.tr, pred.shape
        _hip.check(tr.lib.fn2_downsample_scaled_f32(_hip.ptr(tr.gt), tr.gt_scale, _hip.ptr(self.labels[p]), n, tr.H, tr.W, 2,
                                                    h, w, s))

    def _weighted(self, p, pred, g, wgt, s):
        tr, (n, h, w, _) = self.tr, pred.shape
        _hip.check(tr.lib.fn2_epe_loss_grad_weighted(_hip.ptr(pred), _hip.ptr(self.labels[p]), _hip.ptr(self.weights[p]),
                                                     _hip.ptr(g), _hip.ptr(tr.loss_dev), n, h, w, wgt, tr.loss_scale, s))


class Dense(_Stage):
    """Plain AEPE at every scale (flownet_s.py:122-158); also the 'edges' mode called without an edge map."""
    kind = "dense"
    _alloc = _Stage._alloc_labels

    def launch(self, s):
        tr = self.tr
        for p, pred, g, wgt in self.levels:
            n, h, w, _ = pred.shape
            self._label(p, pred, s)
            _hip.check(tr.lib.fn2_epe_loss_grad(_hip.ptr(pred), _hip.ptr(self.labels[p]), _hip.ptr(g), _hip.ptr(tr.loss_dev),
                                                n, h, w, wgt, tr.loss_scale, s))


class Hard(_Stage):
    """'hard' mining: the exact top-k selection of every scale in ONE fn2_hfem_hard_weights launch (one workgroup per
    level), then the weighted loss per scale."""
    kind = "hard"

    def _alloc(self, levels):
        self._alloc_labels(levels)
        tr, table = self.tr, []
        self.epe = {p: self._new(*pred.shape[:3]) for p, pred, _g, _wgt in levels}
        self.weights = {p: self._new(*pred.shape[:3]) for p, pred, _g, _wgt in levels}
        for p, pred, _g, _wgt in levels:
            numel = self.epe[p].numel()
            k = losses.hard_k(numel, tr.hard_perc)
            table.append(losses.hfem_level(pred, self.labels[p], self.epe[p], self.weights[p], k,
                                           losses.hard_weight_of(numel, k, tr.lambda_w)))
        self.table = (_hip.Fn2HfemLevel * len(table))(*table)

    def launch(self, s):
        for p, pred, _g, _wgt in self.levels:
            self._label(p, pred, s)
        _hip.check(self.tr.lib.fn2_hfem_hard_weights(self.table, len(self.table), s))
        for level in self.levels:
            self._weighted(*level, s)


class Edges(_Stage):
    """'edges' mining: every pixel weighted 1 + lambda * edge map.  edges_in is the static input the step copies the
    [N,H,W,1] map into; the maps at the scales' sizes are formed here."""
    kind = "edges"

    def _alloc(self, levels):
        self._alloc_labels(levels)
        self.edges_in = self._new(self.tr.N, self.tr.H, self.tr.W, 1)
        self.weights = {p: self._new(*pred.shape[:3]) for p, pred, _g, _wgt in levels}
        self.edge_maps = {p: self._new(*pred.shape[:3], 1) for p, pred, _g, _wgt in levels}

    def launch(self, s):
        tr = self.tr
        for p, pred, _g, _wgt in self.levels:
            self._label(p, pred, s)
        for p, pred, g, wgt in self.levels:
            n, h, w, _ = pred.shape
            e = self.edge_maps[p]
            _hip.check(tr.lib.fn2_downsample_f32(_hip.ptr(self.edges_in), _hip.ptr(e), n, tr.H, tr.W, 1, h, w, s))
            _hip.check(tr.lib.fn2_hfem_edge_weights(_hip.ptr(e), tr.lambda_w, _hip.ptr(self.weights[p]), e.numel(), s))
            self._weighted(p, pred, g, wgt, s)


class Photometric(_Stage):
    """The occlusion-aware photometric loss of src/photometric.py, and with a smoothness weight the term of
    src/smoothness.py behind it: per scale the frames at that size and the mask, one mask count per scale, and the level
    table over them.  scale = (1 / gt_scale) * (w_l / W) turns a prediction into pixels of its level.  launch: the frames
    at the scales' sizes, then the masks and the loss with its gradients, one launch each for all scales."""
    kind = "photometric"

    def _alloc(self, levels):
        tr = self.tr
        self.imgs, self.masks, self.scales, self.counts, table = {}, {}, {}, self._new(len(levels)), []
        for i, (p, pred, g, wgt) in enumerate(levels):
            n, h, w, _ = pred.shape
            if tr.H * w != tr.W * h:
                raise ValueError("unsupervised training needs one scale factor per level: %s is %dx%d for %dx%d frames"
                                 % (p, h, w, tr.H, tr.W))
            self.imgs[p], self.masks[p] = self._new(n, h, w, 3), self._new(n, h, w)
            self.scales[p] = (1.0 / tr.gt_scale) * (w / float(tr.W))
            table.append(photometric.level(pred, self.imgs[p], self.masks[p], self.counts[i:i + 1], g, self.scales[p], wgt))
        self.table = photometric.level_table(table)
        self.zeroed = [self.counts]

    def _frames_and_masks(self, s):
        tr, lib = self.tr, self.tr.lib
        for img in self.imgs.values():
            if min(img.shape[1:3]) == 1:
                # no pixel of a 1-high or 1-wide level is valid (0 <= Y < h - 1 is empty), so its frames are never read;
                # fn2_downsample_f32 has no size-1 output (the reference kernel divides by zero there)
                continue
            _hip.check(lib.fn2_downsample_f32(_hip.ptr(tr.eng.in_a), _hip.ptr(img), tr.N, tr.H, tr.W, 3, int(img.shape[1]),
                                              int(img.shape[2]), s))
        _hip.check(lib.fn2_photometric_masks(self.table, len(self.levels), tr.N, tr.occ_alpha, tr.occ_beta, s))

    def _photometric(self, table, s):
        tr = self.tr
        _hip.check(tr.lib.fn2_photometric_loss_grad(table, len(table), tr.N, tr.photometric_q, tr.loss_scale,
                                                    _hip.ptr(tr.loss_dev), s))

    def _smoothness(self, s):
        tr = self.tr
        if tr.smoothness_weight > 0.0:  # one more launch over the same table
            _hip.check(tr.lib.fn2_smoothness_loss_grad(self.table, len(self.levels), tr.N, tr.smoothness_order,
                                                       tr.edge_lambda, tr.smoothness_eps, tr.smoothness_weight,
                                                       tr.loss_scale, 1, _hip.ptr(tr.loss_dev), s))

    def launch(self, s):
        self._frames_and_masks(s)
        self._photometric(self.table, s)
        self._smoothness(s)


class Census(Photometric):
    """data_term='census': the frames, masks and scales of Photometric, and on every scale that holds a 7 x 7 patch the
    ternary census term of src/census.py in its place -- G, the planes W / DX / DY, V, the planes S / c and one count Mc
    per such scale.  The scales below 7 pixels (the 6 x 8 predict_flow6 of a 384 x 512 frame) have no interior pixel and
    would train on nothing but the paths through their upsampling: they keep the photometric term, on a table of their
    own.  launch: the frames, the masks of all scales, the three census launches, the photometric launch on the small
    scales if there is one, then the smoothness term over all scales as in Photometric."""
    kind = "census"

    def _alloc(self, levels):
        super()._alloc(levels)
        self.grey, self.warp, self.valid, self.coef, big, small = {}, {}, {}, {}, [], []
        names = [p for p, pred, _g, _wgt in levels if min(pred.shape[1:3]) >= census.PATCH]
        self.census_counts = self._new(max(len(names), 1))
        for i, (p, pred, g, wgt) in enumerate(levels):
            n, h, w, _ = pred.shape
            if p not in names:  # (its mask count is the one fn2_photometric_masks fills through the table of all scales)
                small.append(photometric.level(pred, self.imgs[p], self.masks[p], self.counts[i:i + 1], g, self.scales[p],
                                               wgt))
                continue
            self.grey[p], self.warp[p], self.valid[p] = self._new(n, h, w), self._new(3, n, h, w), self._new(n, h, w)
            self.coef[p] = self._new(2, n, h, w)
            big.append(census.level(pred, self.imgs[p], self.masks[p], g, self.grey[p], self.warp[p], self.valid[p],
                                    self.coef[p], self.census_counts[len(big):len(big) + 1], self.scales[p], wgt))
        self.census_names = names
        self.census_table = census.level_table(big) if big else None
        self.small_table = photometric.level_table(small) if small else None
        self.zeroed = [self.counts, self.census_counts]

    def launch(self, s):
        tr, lib = self.tr, self.tr.lib
        self._frames_and_masks(s)
        if self.census_table is not None:
            nl = len(self.census_table)
            _hip.check(lib.fn2_census_warp(self.census_table, nl, tr.N, s))
            _hip.check(lib.fn2_census_cost(self.census_table, nl, tr.N, tr.photometric_q, _hip.ptr(tr.loss_dev), s))
            _hip.check(lib.fn2_census_grad(self.census_table, nl, tr.N, tr.loss_scale, s))
        if self.small_table is not None:
            self._photometric(self.small_table, s)
        self._smoothness(s)


class Sparse(_Stage):
    """The loss of src/sparse_epe.py on the labels the dense loss forms -- scale * NaN is NaN, and the downsample skips NaN
    samples and returns NaN where more than half of the weight was NaN: one counter of valid label pixels per scale, then
    the counts and the loss with its gradients, one launch each for all scales."""
    kind = "sparse"

    def _alloc(self, levels):
        self._alloc_labels(levels)
        self.counts = self._new(len(levels), dtype=torch.int32)
        self.table = sparse_epe.level_table([sparse_epe.level(pred, self.labels[p], g, self.counts[i:i + 1], wgt)
                                             for i, (p, pred, g, wgt) in enumerate(levels)])
        self.zeroed = [self.counts]

    def launch(self, s):
        tr, nl = self.tr, len(self.levels)
        for p, pred, _g, _wgt in self.levels:
            self._label(p, pred, s)
        _hip.check(tr.lib.fn2_sparse_epe_count(self.table, nl, tr.N, s))
        _hip.check(tr.lib.fn2_sparse_epe_loss_grad(self.table, nl, tr.N, tr.loss_scale, _hip.ptr(tr.loss_dev), s))


def stage_for(trainer, with_edge_map=False):
    """The stage of the trainer's mode (its constructor has refused the combinations)."""
    if trainer.unsupervised:
        return Census(trainer) if trainer.data_term == "census" else Photometric(trainer)
    if trainer.sparse_gt:
        return Sparse(trainer)
    if trainer.hfem == "hard":
        return Hard(trainer)
    return Edges(trainer) if trainer.hfem == "edges" and with_edge_map else Dense(trainer)
