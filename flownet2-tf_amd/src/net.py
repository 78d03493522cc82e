"""Harness: the parts of /root/reference src/net.py that sit on the inference path
(``Net.test`` :484-628, ``Net.test_batch`` :632-1000, ``adapt_x`` :324-392, ``postproc_y_hat_test`` :463-473,
``get_padded_image_size`` :301-309), re-expressed over the HIP engine.

Deviations from the reference (its classic entry points are stale, SURVEY.md
Appendix C): ``test`` works for all six classic models (defect D1), the output
sub-folder is the parent directory name of ``input_a`` (the intended behaviour
behind defect D3), and a missing checkpoint falls back -- loudly -- to seeded
synthetic weights, because no trained weights can be obtained offline.
"""
import datetime
import os
import sys
from enum import Enum
from math import ceil

import numpy as np
import torch

from . import weights as W
from .engine import BatchTooLarge, Engine
from .flowlib import compute_all_metrics, endpoint_error, flow_to_image, get_metrics, read_flow, write_flow
from .training_schedules import LONG_SCHEDULE


class Mode(Enum):
    TRAIN = 1
    TEST = 2


def imread(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def imsave(path, img):
    from PIL import Image
    Image.fromarray(np.asarray(img, np.uint8)).save(path)


class Net(object):
    model_name = None  # set by subclasses: 'FlowNetS', ...

    def __init__(self, mode=Mode.TRAIN, debug=False, dtype="f32"):
        self.mode = mode
        self.debug = debug
        self.dtype = dtype
        self.weights = None
        self._engines = {}
        self._chunk_of = {}   # (height, width, dtype) -> pairs per engine when the whole batch does not fit (model())

    # ---- weights -----------------------------------------------------------------------------
    def load_weights(self, checkpoint=None, seed=1234):
        """``checkpoint``: a TensorFlow V2 checkpoint prefix as the reference restores it (``.../flownet-S.ckpt-0``
        with ``.index`` + ``.data-*``; src/tf_checkpoint.py reads the bundle without TensorFlow), an .npz keyed by
        the reference's variable names (weights.load_npz) or the .npy dict of the reference's Caffe converter
        (weights.load_npy).  A checkpoint that does not exist here -> seeded synthetic weights + warning."""
        if checkpoint is not None and W.checkpoint_exists(checkpoint):
            self.weights = W.load_weights(checkpoint)
        else:
            if checkpoint is not None:
                sys.stderr.write("WARNING: checkpoint %r not found (TF bundle prefix, .npz or .npy); using seeded synthetic "
                                 "weights (seed %d) -- flows are NOT meaningful predictions\n" % (checkpoint, seed))
            self.weights = self._init_weights(seed)
        self._engines = {}
        return self.weights

    def _init_weights(self, seed):
        return W.init_weights(self.model_name, seed)

    def engine(self, batch, height, width, uint8_inputs=False, interp_u8_inputs=False):
        if self.weights is None:
            self.load_weights()
        key = (batch, height, width, self.dtype, bool(uint8_inputs), bool(interp_u8_inputs))
        if key not in self._engines:
            extra = {"interp_u8_inputs": True} if interp_u8_inputs else {}
            self._engines[key] = Engine(self.model_name, self.weights, batch, height, width, self.dtype,
                                        uint8_inputs=uint8_inputs, **extra, **self._engine_kwargs())
        return self._engines[key]

    def _engine_kwargs(self):
        return {}

    # ---- graph: same signature as the reference's model()/loss() --------------------------------
    def model(self, inputs, training_schedule=LONG_SCHEDULE, trainable=True):
        """inputs: {'input_a','input_b'} NHWC float32 in [0,1], H and W multiples of 64.
        Returns the reference's prediction dict (predict_flow6..2 / predict_flow0, 'flow') as
        fp32 ROCm tensors."""
        a, b = inputs['input_a'], inputs['input_b']
        n, h, w, _ = a.shape
        u8 = _is_u8(a) and _is_u8(b)
        scale = inputs.get('scale', (int(a.max()) > 1, int(b.max()) > 1)) if u8 else None
        # a batch whose activation tensors would pass the kernels' 2 GiB addressing limit runs as chunks of the
        # largest batch that fits (the convolutions are per-pair: chunking changes no value); the chunk size found
        # for a shape is remembered
        chunk = self._chunk_of.get((int(h), int(w), self.dtype), int(n))
        outs, i = [], 0
        while i < n:
            m = min(chunk, int(n) - i)
            try:
                eng = self.engine(m, int(h), int(w), uint8_inputs=u8)
            except BatchTooLarge as e:
                chunk = min(e.fit, m - 1)
                self._chunk_of[(int(h), int(w), self.dtype)] = chunk
                continue
            if u8:
                # un-normalised uint8 frames (adapt_x_u8): the bytes go to the device as they are and the `/ 255.0` of
                # adapt_x (net.py:338-345) runs there -- byte-identical, a quarter of the host-link traffic
                eng.set_inputs_u8(a[i:i + m], b[i:i + m], scale=scale)
                eng.launch()
                out = eng.outputs
            else:
                out = eng(a[i:i + m], b[i:i + m])
            outs.append({k: v.clone() for k, v in out.items()})
            i += m
        if len(outs) == 1:
            return outs[0]
        return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}

    # ---- test-time input adaptation ---------------------------------------------------------------
    def get_padded_image_size(self, og_height, og_width, divisor=64):
        return int(ceil(og_height / divisor) * divisor), int(ceil(og_width / divisor) * divisor)

    def adapt_x(self, input_a, input_b, divisor=64):
        """[0,255] -> [0,1] when max > 1; add the batch axis; zero-pad bottom/right to a multiple
        of ``divisor``.  Returns (a, b, original_shape_or_None)."""
        a, b = _unit_range(input_a), _unit_range(input_b)
        if a.shape != b.shape:
            raise _shapes_differ(a.shape, b.shape)
        (a, b), info = self._batch_and_pad((a, b), divisor)
        return a.astype(np.float32), b.astype(np.float32), info

    def adapt_x_u8(self, input_a, input_b, divisor=64):
        """adapt_x for uint8 frames without leaving uint8: batch axis + zero padding on the host, and the decision
        adapt_x takes per image (`max() > 1.0` -> divide by 255, net.py:338-345) returned as `scale` for the device to
        apply.  Returns (a_u8, b_u8, original_shape_or_None, (scale_a, scale_b))."""
        a, b = np.asarray(input_a), np.asarray(input_b)
        if a.dtype != np.uint8 or b.dtype != np.uint8:
            raise ValueError("adapt_x_u8 takes uint8 images")
        if a.shape != b.shape:
            raise _shapes_differ(a.shape, b.shape)
        scale = (_exceeds_one(a), _exceeds_one(b))
        (a, b), info = self._batch_and_pad((a, b), divisor)
        return np.ascontiguousarray(a), np.ascontiguousarray(b), info, scale

    def adapt_x_matches(self, input_a, matches_a, sparse_flow, divisor=64):
        """adapt_x for (image, match mask, sparse flow) (net.py:324-392): image and mask to [0,1] when their max
        exceeds 1, mask gets its channel axis, all three batched and zero-padded to multiples of `divisor`."""
        a = _unit_range(input_a)
        m = _unit_range(np.asarray(matches_a)[..., np.newaxis])
        sf = np.asarray(sparse_flow, np.float32)
        _check_mask(a, m)
        (a, m, sf), info = self._batch_and_pad((a, m, sf), divisor)
        return a.astype(np.float32), m.astype(np.float32), sf.astype(np.float32), info

    def adapt_x_matches_u8(self, image, mask, sparse_flow, divisor=64):
        """adapt_x_matches for a uint8 image and a uint8 match mask without float arithmetic on the host: channel and
        batch axes + zero padding in the source dtypes, and the two decisions adapt_x takes (`max() > 1` -> divide by
        255, net.py:334-345) returned as `scale` for the device to apply (fn2_pack_interp_u8).
        Returns (image_u8 [1,H,W,3], mask_u8 [1,H,W,1], sparse_f32 [1,H,W,2], original_shape_or_None,
        (scale_image, scale_mask))."""
        a, m = np.asarray(image), np.asarray(mask)
        if a.dtype != np.uint8 or m.dtype != np.uint8:
            raise ValueError("adapt_x_matches_u8 takes a uint8 image and a uint8 mask")
        m = m[..., np.newaxis]
        sf = np.asarray(sparse_flow, np.float32)
        _check_mask(a, m)
        scale = (_exceeds_one(a), _exceeds_one(m))
        (a, m, sf), info = self._batch_and_pad((a, m, sf), divisor)
        return np.ascontiguousarray(a), np.ascontiguousarray(m), np.ascontiguousarray(sf), info, scale

    def _batch_and_pad(self, arrays, divisor):
        """The batch axis where it is missing, then every array zero-padded (bottom / right) to the multiples of
        `divisor` above the first one's height and width.  Returns (arrays, shape of the batched first array) -- or
        (arrays, None) when nothing had to be padded."""
        arrays = [x[None] if x.ndim == 3 else x for x in arrays]
        h, w = arrays[0].shape[1:3]
        nh, nw = self.get_padded_image_size(h, w, divisor)
        if (nh, nw) == (h, w):
            return arrays, None
        pad = [(0, 0), (0, nh - h), (0, nw - w), (0, 0)]
        return [np.pad(x, pad) for x in arrays], arrays[0].shape

    @staticmethod
    def _original_size(padded, info):
        """(h, w) of a frame before padding, from what its adaptor returned: `info`, or None where nothing was padded."""
        return (info[-3], info[-2]) if info is not None else tuple(padded.shape[1:3])

    def postproc_y_hat_test(self, pred_flows, adapt_info=None):
        if adapt_info is not None:
            pred_flows = pred_flows[0:adapt_info[-3], 0:adapt_info[-2], :]
        return pred_flows

    # ---- single-pair inference ----------------------------------------------------------------------
    def test(self, checkpoint, input_a_path, input_b_path=None, matches_a_path=None, sparse_flow_path=None,
             out_path='./', input_type='image_pairs', save_image=True, save_flo=True, compute_metrics=True,
             gt_flow=None, new_par_folder=None, occlusions=False, occ_mask=None, inv_mask=None,
             variational_refinement=False):
        """net.py:484-628: one pair, or one 'image_matches' set (FlowNetS_interp: first image + match mask + sparse flow),
        as the one-line case of test_batch -- the same launchers with `batch_size` 1 (2 with `occlusions`), so
        `variational_refinement` and `occlusions` mean what they mean there; refinement needs `input_b_path`.
        What differs is what the reference's `test` does differently: the output folder and name (below), and the
        metrics of a ground truth, printed -- the MPI-Sintel block (net.py:612-625) for 'image_matches' or with
        `occ_mask` / `inv_mask` (paths of the masks that split it into matched / unmatched regions), else one
        `EPE all` line.  Returns the forward flow."""
        if occlusions and input_type == 'image_matches':
            raise ValueError("occlusions need the second frame as a network input: input_type 'image_matches' has no "
                             "matches for it")
        if self.weights is None:
            self.load_weights(checkpoint)
        occ_files = None
        if input_type == 'image_matches':
            if matches_a_path is None or sparse_flow_path is None:
                raise ValueError("input_type 'image_matches' needs matches_a_path and sparse_flow_path")
            fields = dict(matches_line_fields([input_a_path, matches_a_path, sparse_flow_path]), image_b=input_b_path)
            flow = self._infer_matches([fields], 1, variational_refinement)[0]
        elif occlusions:
            flow, flow_bw, occ_fw, occ_bw = self._infer_pairs([[input_a_path, input_b_path]], 2, variational_refinement,
                                                              bidirectional=True)[0]
            self.last_occlusions = [(occ_fw, occ_bw)]
            occ_files = (flow_bw, occ_fw, occ_bw)
        else:
            flow = self._infer_pairs([[input_a_path, input_b_path]], 1, variational_refinement)[0]

        # net.py:546-547: the folder is the name of the first image's directory (_write_line: `split('/')[-2]`)
        parent = new_par_folder if new_par_folder is not None else \
            os.path.basename(os.path.dirname(os.path.abspath(input_a_path)))
        # net.py:546: `splitext`, an extension of any length (_write_line: `[:-4]`)
        unique_name = os.path.splitext(os.path.basename(input_a_path))[0]
        max_flow = -1
        gt = None
        if compute_metrics and gt_flow is not None:
            gt = read_flow(gt_flow)
            # net.py:595: the largest motion of the ground truth (_write_line: its largest component)
            max_flow = float(np.max(np.sqrt(gt[:, :, 0] ** 2 + gt[:, :, 1] ** 2)))
        self._write_outputs(flow, os.path.join(out_path, parent), unique_name, max_flow, save_image, save_flo, occ_files)
        if gt is not None and (input_type == 'image_matches' or occ_mask is not None or inv_mask is not None):
            occ = imread_gray(occ_mask) if occ_mask is not None else None
            inv = imread_gray(inv_mask) if inv_mask is not None else None
            metrics = compute_all_metrics(flow, gt, occ_mask=occ, inv_mask=inv)[0]
            print(get_metrics(metrics, flow_fname=unique_name))
        elif gt is not None:
            print("{}: EPE all = {:.4f}".format(unique_name, endpoint_error(flow, gt)))
        return flow

    # ---- inference over a list file (+ MPI-Sintel metrics) ---------------------------------------------
    _METRIC_ORDER = ('mangall', 'stdangall', 'EPEall', 'mangmat', 'stdangmat', 'EPEmat', 'mangumat', 'stdangumat',
                     'EPEumat', 'S0-10', 'S10-40', 'S40plus')

    def test_batch(self, checkpoint, image_paths, out_path, input_type='image_pairs', save_image=True, save_flo=True,
                   compute_metrics=True, accumulate_metrics=False, log_metrics2file=True, width=1024, height=436,
                   new_par_folder=None, variational_refinement=False, batch_size=8, occlusions=False,
                   occlusions_for_metrics=False):
        """Inference on every line of the text file `image_paths` (net.py:632-1000).  input_type 'image_pairs': a line
        is `img1 img2 [gt.flo [occ_mask.png [inv_mask.png]]]`.  input_type 'image_matches' (FlowNetS_interp): a line is
        one of the layouts of `matches_line_fields` -- `I1 MM SF [GT [[OCC [INV]] I2]]`: the last field of a 5-, 6- or
        7-field line is the second image; the reference's `I1 MM SF GT OCC` and `I1 MM SF GT OCC INV` branches are
        shadowed by those (net.py:773 / :798, :809 / :820) and are unreachable here as well.
        Per line: `<name>_viz.png`, `<name>_viz_norm_gt_max_motion.png` and `<name>_flow.flo` (_write_outputs); with a
        ground truth, the MPI-Sintel metrics block goes to `<list name>_metrics.log` (or stdout), and
        `accumulate_metrics` appends the sequence averages.
        `width`/`height` are kept for signature compatibility (the reference sizes its placeholders with them); frames
        are padded by their own size.  `batch_size` lines of equal padded size go through the engine per launch (the
        reference feeds one per sess.run).  `variational_refinement`: the cropped flows are refined on the device by
        the EpicFlow energy minimisation (src/variational.py, the reference's defaults; the reference runs its binary
        per line, net.py:889-901) before metrics and outputs; an 'image_matches' line without a second image comes
        back unrefined.
        `occlusions` / `occlusions_for_metrics` ('image_pairs' only, `batch_size` even): every line runs in both
        directions, `batch_size // 2` lines per launch (_infer_bidirectional), and the forward-backward check gives an
        occlusion mask per direction, kept as `self.last_occlusions` [(occ_fw, occ_bw) uint8 0 / 255 per line].  With
        `occlusions` a line also writes `<name>_occ.png`, `<name>_occ_bw.png` and `<name>_flow_bw.flo`; with
        `occlusions_for_metrics` a line with a ground truth and no occlusion mask file takes the estimated forward mask
        for the matched / unmatched split of its metrics.  Returns the forward flows."""
        if input_type not in ('image_pairs', 'image_matches'):
            raise NotImplementedError("test_batch: input_type must be 'image_pairs' or 'image_matches', got %r" % (input_type,))
        bidirectional = bool(occlusions or occlusions_for_metrics)
        if bidirectional and input_type == 'image_matches':
            raise ValueError("occlusions need the second frame as a network input: input_type 'image_matches' has no "
                             "matches for it")
        if bidirectional and batch_size % 2:
            raise ValueError("occlusions put the two directions of a line into neighbouring slots: batch_size must be "
                             "even, got %d" % batch_size)
        if self.weights is None:
            self.load_weights(checkpoint)
        with open(image_paths, 'r') as f:
            lines = [ln.split() for ln in f.read().splitlines() if ln.strip()]
        logfile = None
        if log_metrics2file:
            name = os.path.basename(image_paths).replace('.txt', '_metrics.log')
            full = os.path.join(out_path, name) if new_par_folder is None else os.path.join(out_path, new_par_folder, name)
            os.makedirs(os.path.dirname(full) or '.', exist_ok=True)
            logfile = open(full, 'w')
            if new_par_folder is not None:
                logfile.write("Today is {}\nOpening and logging experiment '{}'\n Written to file: '{}'\n".format(
                    datetime.datetime.now().strftime('%d-%m-%y_%H-%M-%S'), new_par_folder, full))
        rows, counts = [], np.zeros(4, np.int64)  # not occluded / empty S0-10 / S10-40 / S40+ frame counts
        flows = []
        if bidirectional:
            self.last_occlusions = []
        per_launch = batch_size // 2 if bidirectional else batch_size
        try:
            for start in range(0, len(lines), per_launch):
                chunk = lines[start:start + per_launch]
                if input_type == 'image_matches':
                    fields = [matches_line_fields(paths) for paths in chunk]
                    chunk_flows = self._infer_matches(fields, batch_size, variational_refinement)
                else:
                    fields = None
                    chunk_flows = self._infer_pairs(chunk, batch_size, variational_refinement, bidirectional=bidirectional)
                for k, (paths, flow) in enumerate(zip(chunk, chunk_flows)):
                    extra = {}
                    if bidirectional:
                        flow, flow_bw, occ_fw, occ_bw = flow
                        self.last_occlusions.append((occ_fw, occ_bw))
                        if occlusions:
                            extra['occlusions'] = (flow_bw, occ_fw, occ_bw)
                        if occlusions_for_metrics:
                            extra['estimated_occ'] = occ_fw
                    flows.append(flow)
                    if fields is not None:
                        gt_path, occ_path, inv_path = fields[k]['gt'], fields[k]['occ'], fields[k]['inv']
                    else:
                        assert 2 <= len(paths) <= 5, 'expected: img1 img2 [gt_flow [occ_mask [inv_mask]]]'
                        gt_path, occ_path, inv_path = (list(paths[2:5]) + [None] * 3)[:3]
                    m, flags = self._write_line(flow, paths[0], gt_path, occ_path, inv_path, out_path, new_par_folder,
                                                save_image, save_flo, compute_metrics, logfile, **extra)
                    if m is not None and accumulate_metrics:
                        counts += np.array(flags)
                        rows.append([m[k2] for k2 in self._METRIC_ORDER])
            if accumulate_metrics and rows:
                avg = self._average_metrics(np.array(rows, np.float64).reshape(len(rows), -1), counts)
                if logfile is not None:
                    logfile.write('\n\nToday is: {}\nNow logging final averaged metrics \n\n'.format(
                        datetime.datetime.now().strftime('%d-%m-%y_%H-%M-%S')))
                    logfile.write(get_metrics(dict(zip(self._METRIC_ORDER, avg)), average=True))
                self.last_average_metrics = dict(zip(self._METRIC_ORDER, avg))
        finally:
            if logfile is not None:
                logfile.close()
        return flows

    def _write_line(self, flow, first_path, gt_path, occ_path, inv_path, out_path, new_par_folder, save_image, save_flo,
                    compute_metrics, logfile, occlusions=None, estimated_occ=None):
        """What test_batch leaves behind for one list line, whatever its input type: the files of _write_outputs and --
        with a ground truth -- the metrics block (to `logfile`, or stdout).  `estimated_occ`: the occlusion mask of a
        line that names no mask file.  Returns (metrics, flags) of compute_all_metrics, or (None, None)."""
        gt = read_flow(gt_path) if gt_path is not None else None
        occ = imread_gray(occ_path) if occ_path is not None and compute_metrics else None
        if occ is None and occ_path is None and compute_metrics:
            occ = estimated_occ
        inv = imread_gray(inv_path) if inv_path is not None and compute_metrics else None
        # net.py:909-910: the largest component of the ground truth (test: its largest motion)
        max_flow = np.max(gt) if (compute_metrics and gt is not None) else -1
        # net.py:853: the second-last component of the path as the list spells it (test: the directory's name)
        parent = first_path.split('/')[-2] if new_par_folder is None else new_par_folder
        unique_name = os.path.basename(first_path)[:-4]  # a three-letter extension (test: `splitext`)
        self._write_outputs(flow, os.path.join(out_path, parent), unique_name, max_flow, save_image, save_flo, occlusions)
        if not (compute_metrics and gt is not None):
            return None, None
        m, *flags = compute_all_metrics(flow, gt, occ_mask=occ, inv_mask=inv)
        text = get_metrics(m, flow_fname=unique_name)
        if logfile is not None:
            logfile.write(text)
        else:
            print(text)
        return m, flags

    @staticmethod
    def _write_outputs(flow, out_dir, unique_name, max_flow, save_image, save_flo, occlusions=None):
        """`<name>_viz.png`, `<name>_viz_norm_gt_max_motion.png` (colours scaled to `max_flow`) and `<name>_flow.flo` under
        `out_dir`; with `occlusions` (flow_bw, occ_fw, occ_bw) also `<name>_occ.png` (forward mask, 0 / 255),
        `<name>_occ_bw.png` and `<name>_flow_bw.flo`."""
        stem = os.path.join(out_dir, unique_name)
        if save_image or save_flo or occlusions is not None:
            os.makedirs(out_dir, exist_ok=True)
        if save_image:
            imsave(stem + '_viz.png', flow_to_image(flow.copy()))
            imsave(stem + '_viz_norm_gt_max_motion.png', flow_to_image(flow.copy(), maxflow=max_flow))
        if save_flo:
            write_flow(flow, stem + '_flow.flo')
        if occlusions is not None:
            flow_bw, occ_fw, occ_bw = occlusions
            imsave(stem + '_occ.png', occ_fw)
            imsave(stem + '_occ_bw.png', occ_bw)
            write_flow(flow_bw, stem + '_flow_bw.flo')

    # ---- the launchers: list lines -> cropped flows ------------------------------------------------------
    def _launch_groups(self, samples, keys, batch_size, interp=False):
        """One engine launch per group of lines with equal `keys[i]`: (padded frame shape,) for the uint8 interp engine
        (`interp`), (padded frame shape, scale) for the uint8 pair engine, whose input buffers take one normalisation
        decision per launch.  samples[i]: the input tuples line i puts into neighbouring slots of the `batch_size`
        engine; a short group leaves zero samples behind it, so that one engine serves the whole list.
        Yields (engine, line indices, batch arrays, key) after each launch."""
        groups = {}
        for i, key in enumerate(keys):
            groups.setdefault(key, []).append(i)
        for key, idxs in groups.items():
            slots = [sample for i in idxs for sample in samples[i]]
            arrays = [np.zeros((batch_size,) + x.shape, x.dtype) for x in slots[0]]
            for j, sample in enumerate(slots):
                for dst, src in zip(arrays, sample):
                    dst[j] = src
            height, width = key[0][1:3]
            if interp:
                eng = self.engine(batch_size, height, width, interp_u8_inputs=True)
                eng.set_inputs_interp_u8(*arrays)
            else:
                eng = self.engine(batch_size, height, width, uint8_inputs=True)
                eng.set_inputs_u8(*arrays, key[1])
            eng.launch()
            yield eng, idxs, arrays, key

    def _infer_pairs(self, chunk, batch_size, variational_refinement=False, bidirectional=False):
        """Flows (cropped to each frame's size) of up to `batch_size` list lines (_launch_groups).
        With `variational_refinement`, one refinement call per group of equal original size.
        `bidirectional`: up to `batch_size // 2` lines, see _infer_bidirectional."""
        if bidirectional:
            return self._infer_bidirectional(chunk, batch_size, variational_refinement)
        frames = [self.adapt_x_u8(imread(p[0]), imread(p[1])) for p in chunk]
        out = [None] * len(chunk)
        for eng, idxs, _, _ in self._launch_groups([[(a[0], b[0])] for a, b, _, _ in frames],
                                                   [(a.shape, scale) for a, _, _, scale in frames], batch_size):
            if variational_refinement:
                self._refine_group(eng.outputs['flow'], frames, idxs, out)
                continue
            pred = eng.outputs['flow'].float().cpu().numpy()
            for j, i in enumerate(idxs):
                out[i] = self._crop(pred[j], frames[i][0], frames[i][2])
        return out

    def _crop(self, pred, padded, info):
        """The [h,w,2] part of a padded host flow that belongs to the frame, as an array of its own."""
        return self.postproc_y_hat_test(pred, self._original_size(padded, info) + (2,)).copy()

    def _infer_bidirectional(self, chunk, batch_size, variational_refinement=False):
        """(flow_fw, flow_bw, occ_fw, occ_bw) of up to `batch_size // 2` list lines: flows [h,w,2] float32 and
        forward-backward occlusion masks [h,w] uint8 0 / 255 (src/occlusion.py), cropped to each frame's size.  Line k
        of a group fills slot 2k with (a, b) and slot 2k + 1 with (b, a) of the `batch_size` engine _infer_pairs uses:
        the backward flows ride on the launch that is running anyway.  Both flows are cropped on the device and the
        check reads the crops in place, one call per run of neighbouring lines of equal original size.  With
        `variational_refinement` the forward flow is refined, after the masks are formed."""
        from .occlusion import occlusion
        if batch_size % 2:
            raise ValueError("bidirectional inference puts the two directions of a line into neighbouring slots: "
                             "batch_size must be even, got %d" % batch_size)
        if len(chunk) > batch_size // 2:
            raise ValueError("bidirectional inference takes batch_size // 2 = %d lines per launch, got %d"
                             % (batch_size // 2, len(chunk)))
        frames = [self.adapt_x_u8(imread(p[0]), imread(p[1])) for p in chunk]
        out = [None] * len(chunk)
        for eng, idxs, (a, b), (_, scale) in self._launch_groups([[(a[0], b[0]), (b[0], a[0])] for a, b, _, _ in frames],
                                                                 [(a.shape, scale) for a, _, _, scale in frames], batch_size):
            flow = eng.outputs['flow'].float()
            if scale[0] != scale[1]:
                # the two frames disagree on the launch's one decision per input buffer: the odd slots come from a
                # second launch with the decisions swapped
                flow = flow.clone()
                eng.set_inputs_u8(a, b, scale[::-1])
                eng.launch()
                flow[1::2] = eng.outputs['flow'][1::2].float()
            sizes = [self._original_size(frames[i][0], frames[i][2]) for i in idxs]
            k = 0
            while k < len(idxs):
                m = 1
                while k + m < len(idxs) and sizes[k + m] == sizes[k]:
                    m += 1
                h, w = sizes[k]
                fw = flow[2 * k:2 * (k + m):2, :h, :w]
                bw = flow[2 * k + 1:2 * (k + m):2, :h, :w]
                occ_fw, occ_bw = (t.cpu().numpy()[..., 0] for t in occlusion(fw, bw, as_uint8=True))
                fw, bw = fw.cpu().numpy(), bw.cpu().numpy()
                for j in range(m):
                    out[idxs[k + j]] = (np.ascontiguousarray(fw[j]), np.ascontiguousarray(bw[j]),
                                        np.ascontiguousarray(occ_fw[j]), np.ascontiguousarray(occ_bw[j]))
                k += m
            if variational_refinement:
                refined = [None] * len(chunk)
                self._refine_group(flow[0::2], frames, idxs, refined)
                for i in idxs:
                    out[i] = (refined[i],) + out[i][1:]
        return out

    def _infer_matches(self, fields, batch_size, variational_refinement=False):
        """_infer_pairs for 'image_matches' lines (`fields`: matches_line_fields records): image, match mask and sparse
        flow through the uint8 interp engine.  The scale decisions travel per sample (Engine.in_flags), so lines with
        0/255 and 0/1 masks share a launch.  With `variational_refinement`, the lines that name a second image are
        refined on (I1, I2); the others are not."""
        frames = [self.adapt_x_matches_u8(imread(f['image']), imread_gray(f['matches']), read_flow(f['sparse']))
                  for f in fields]
        out = [None] * len(fields)
        samples = [[(a[0], m[0, :, :, 0], sf[0], np.array(scale, np.uint8))] for a, m, sf, _, scale in frames]
        for eng, idxs, _, _ in self._launch_groups(samples, [(fr[0].shape,) for fr in frames], batch_size, interp=True):
            slots = [j for j, i in enumerate(idxs) if variational_refinement and fields[i]['image_b'] is not None]
            if slots:
                # (padded first frame, padded second frame, info) per line: the records _refine_group reads
                pairs = {}
                for i in (idxs[j] for j in slots):
                    pairs[i] = (frames[i][0], self._pad_like(imread(fields[i]['image_b']), frames[i][0]), frames[i][3])
                sel = torch.tensor(slots, device=eng.outputs['flow'].device)
                self._refine_group(eng.outputs['flow'].index_select(0, sel), pairs, list(pairs), out)
            if len(slots) < len(idxs):
                pred = eng.outputs['flow'].float().cpu().numpy()
                for j, i in enumerate(idxs):
                    if j not in slots:
                        out[i] = self._crop(pred[j], frames[i][0], frames[i][3])
        return out

    @staticmethod
    def _pad_like(image, padded):
        """uint8 frame [H,W,3] zero-padded (bottom / right) to the [1,Hp,Wp,3] shape of `padded`."""
        img = np.asarray(image)
        if img.shape[0] > padded.shape[1] or img.shape[1] > padded.shape[2]:
            raise _shapes_differ(padded.shape, img.shape)
        return np.pad(img, [(0, padded.shape[1] - img.shape[0]), (0, padded.shape[2] - img.shape[1]), (0, 0)])[None]

    @staticmethod
    def _refine_group(pred, frames, idxs, out):
        """Variational refinement of the cropped flows pred[j] of frames[idxs[j]] = (padded first frame, padded second
        frame, info, ...), one call per original size; the frames are read in place from their padded device copies."""
        from .variational import refine
        by_size = {}
        for j, i in enumerate(idxs):
            by_size.setdefault(Net._original_size(frames[i][0], frames[i][2]), []).append((j, i))
        for (h, w), members in by_size.items():
            js = torch.tensor([j for j, _ in members], device=pred.device)
            flow = pred.float().index_select(0, js)[:, :h, :w]
            a = torch.from_numpy(np.stack([frames[i][0][0] for _, i in members])).to(pred.device)
            b = torch.from_numpy(np.stack([frames[i][1][0] for _, i in members])).to(pred.device)
            res = refine(flow, a[:, :h, :w], b[:, :h, :w]).cpu().numpy()
            for k, (_, i) in enumerate(members):
                out[i] = res[k]

    @staticmethod
    def _average_metrics(table, counts):
        """Sequence averages exactly as the reference forms them (net.py:958-984), quirks included: the divisor of
        a column is (#entries != inf) + (#NaN entries); the unmatched columns are scaled by (1 - #frames without
        occlusions) -- operator precedence at :971-972; the S0-10 column is rescaled by n / (n - #empty frames)
        when some frame had no such pixels, while the S10-40 / S40+ rescalings sit behind inverted tests
        (`if not count > 0`, :977-982) and therefore never change anything."""
        n_cols = table.shape[-1]
        avg = np.full(n_cols, np.inf)
        divisor = np.zeros(n_cols)
        for i in range(n_cols):
            col = table[:, i]
            divisor[i] = np.sum(col != np.inf) + np.sum(np.isnan(col))
            avg[i] = np.sum(col[~np.isinf(col) & ~np.isnan(col)]) / divisor[i]
        not_occluded, empty0, empty1, empty2 = (int(c) for c in counts)
        if not_occluded > 0:
            avg[6:9] = avg[6:9] * (1.0 - not_occluded)
        if empty0 > 0:
            avg[9] = avg[9] * (divisor[9] / (divisor[9] - empty0))
        return avg


_MATCHES_LINE_ASSERT = ('More paths than expected. Expected: I1+I2 (2), I1+MM+SF(3), I1+MM+SF+GTF(4),'
                        '  I1+MM+SF+GT+OCC_MSK+INVMASK(5 to 6) optionally + 1extra if variational_refinement')


def matches_line_fields(paths):
    """Fields of one 'image_matches' list line, as the reference dispatches them (net.py:718-850; the first branch that
    matches a field count wins):

        3  I1 MM SF                 5  I1 MM SF GT I2           7  I1 MM SF GT OCC INV I2
        4  I1 MM SF GT              6  I1 MM SF GT OCC I2

    The last field of a 5-, 6- or 7-field line is the second image, which only variational refinement reads.  The
    reference also spells out `I1 MM SF GT OCC` (5) and `I1 MM SF GT OCC INV` (6), but those branches sit behind the
    ones above with the same test and can never run there; they are unreachable here as well.  Any other field count
    raises the reference's assertion (:718-720).  Returns {'image', 'matches', 'sparse', 'gt', 'occ', 'inv',
    'image_b'} with None for what the line does not carry."""
    n = len(paths)
    assert 3 <= n <= 7, _MATCHES_LINE_ASSERT
    return {'image': paths[0], 'matches': paths[1], 'sparse': paths[2],
            'gt': paths[3] if n >= 4 else None,
            'occ': paths[4] if n >= 6 else None,
            'inv': paths[5] if n == 7 else None,
            'image_b': paths[-1] if n >= 5 else None}


def str2bool(v):
    """argparse type of the CLIs' boolean flags (utils.py str2bool)."""
    import argparse
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def _exceeds_one(x):
    """adapt_x's decision (net.py:334-345): an input whose maximum exceeds 1 holds [0,255] and is divided by 255."""
    return bool(x.max() > 1)


def _unit_range(x):
    x = np.asarray(x)
    return x / 255.0 if _exceeds_one(x) else x.astype(np.float64)


def _shapes_differ(shape_a, shape_b):
    return AssertionError("FATAL: image dimensions do not match. Image 1 has shape: {0}, "
                          "Image 2 has shape: {1}".format(shape_a, shape_b))


def _check_mask(image, mask):
    assert mask.shape[:2] == image.shape[:2] and mask.shape[2] == 1, (
        "Mask has invalid dimensions. Should be ({0}, {1}, 1) but are {2}".format(image.shape[0], image.shape[1], mask.shape))


def _is_u8(x):
    return (isinstance(x, np.ndarray) and x.dtype == np.uint8) or (isinstance(x, torch.Tensor) and x.dtype == torch.uint8)


def imread_gray(path):
    """Mask image as the reference's imread returns it for single-channel PNGs: (H, W) uint8."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))
