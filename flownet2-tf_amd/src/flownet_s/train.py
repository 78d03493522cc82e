"""python -m src.flownet_s.train --list train.txt --out ./logs [--steps N --batch 8 --checkpoint w.npz --dtype f16x2
                                 --ckpt-format npz|tf --training_schedule one_cycle --optimizer sgd|momentum|adamw
                                 --momentum M | --min_momentum A --max_momentum B --weight_decay D --clip_grad_norm C
                                 --unsupervised --no-augment|--augmentation pair --photometric_q Q --occ_alpha A
                                 --occ_beta B --data_term photometric|census --smoothness_weight S
                                 --smoothness_order 1|2 --edge_lambda L
                                 --sparse_gt --crop]
The reference's src/flownet_s/train.py:8-40 + Net.train (net.py:1002-1400) over the HIP trainer: FlyingChairs-style
augmentation on the GPU, multiscale EPE loss, Adam on LONG_SCHEDULE (or the optimiser and schedule named), periodic
.npz checkpoints under the reference's variable names.  Data: a list file of `image_a image_b flow.flo` triples (the
reference's TFRecords are built from exactly these).  Under torch.distributed.run every rank trains on its own shuffling of the list (seed + rank) and
the gradients are all-reduced (data parallel).
--unsupervised: no ground truth is read (`image_a image_b` lines are accepted); every pair runs in both directions, so
--batch is even and batch / 2 pairs go in per step; the loss is the occlusion-aware photometric loss (src/photometric.py),
or with --data_term census the ternary census term (src/census.py) on every scale that holds a 7 x 7 patch,
with --smoothness_weight > 0 plus the edge-aware smoothness term (src/smoothness.py).  The one augmentation that keeps
brightness constancy is --augmentation pair (flips, channel permutation and ONE colour record for both frames, no crop).
--sparse_gt: the third field of a line is a KITTI flow .png (or a .flo with unknown pixels); pixels without ground truth take
no part in the loss (src/sparse_epe.py) and validation prints EPE and Fl-all over the valid pixels.  --crop cuts a random
--height x --width window out of every sample (the centre window of validation samples), so frames of differing sizes make
one batch; both need --no-augment or --augmentation selflow|pair."""
import argparse
import os
import sys
import time

import numpy as np

from ..dataloader import FLYING_CHAIRS_PREPROCESS, load_batches
from ..training_schedules import LONG_SCHEDULE, SCHEDULES


def unpack_weights(trainer):
    """{reference variable name: array in the reference layout}: the fp32 masters of the trained layers (packed
    layouts unpacked) over the frozen variables of the checkpoint the trainer was built from (the networks in front of
    the last one in FlowNetCS / CSS, CSS and SD in FlowNet2), optimizer slots left out."""
    from ..trainer import _index_hwio
    slots = ("/Adam", "/Adam_1")
    out = {k: np.asarray(v) for k, v in trainer.host_weights.items()
           if k.endswith(("/weights", "/biases")) and not k.endswith(slots)}
    for rec in trainer.layers:
        if rec["kind"] == "corr" or rec.get("shared_with") is not None:
            continue
        name = f"{rec['scope']}/{rec['name']}"
        flat = rec["master"].cpu().numpy().reshape(-1)
        if rec["kind"] == "upflow":
            out[name + "/weights"] = flat.reshape(4, 4, 2, 2).copy()
        else:
            out[name + "/weights"] = flat[_index_hwio(rec)].astype(np.float32)
        if rec.get("b") is not None:
            out[name + "/biases"] = rec["b"].cpu().numpy().copy()
    return out


def save_checkpoint(out_dir, step, weights, fmt="npz", stem="flownet_s"):
    """npz: <stem>-<step>.npz (flownet_s-<step>.npz / flownet_sd-<step>.npz).  tf: model.ckpt-<step>.{index,data-00000-of-00001} + the `checkpoint` state file,
    the files the reference's slim Saver leaves in its log dir (net.py:1386-1392) and that both this package and
    tf.train.Saver.restore read (variables under the reference names + global_step)."""
    from .. import weights as W
    if fmt == "tf":
        from .. import tf_checkpoint
        name = "model.ckpt-%d" % step
        tf_checkpoint.save_tf_checkpoint(os.path.join(out_dir, name), dict(weights, global_step=np.int64(step)))  # (+ slots)
        with open(os.path.join(out_dir, "checkpoint"), "w") as f:
            f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (name, name))
        return os.path.join(out_dir, name)
    path = os.path.join(out_dir, "%s-%d.npz" % (stem, step))
    W.save_npz(path, weights)
    return path


def load_full_checkpoint(path):
    """Everything a checkpoint holds, bookkeeping included ({name: array}): weights, Adam slots, global_step."""
    from .. import tf_checkpoint, weights as W
    path = str(path)
    for suffix in (".index", ".data-00000-of-00001", ".meta"):
        if path.endswith(suffix) and tf_checkpoint.is_tf_checkpoint(path[:-len(suffix)]):
            path = path[:-len(suffix)]
    if tf_checkpoint.is_tf_checkpoint(path):
        return tf_checkpoint.load_tf_checkpoint(path, float_only=False)
    return W.load_weights(path)


def add_optimizer_arguments(ap):
    """--optimizer, --momentum, --min_momentum, --max_momentum, --weight_decay, --clip_grad_norm: names and defaults of
    the reference's parser (flownet_s_interp/train.py:380-473); --optimizer unset means Adam."""
    ap.add_argument("--optimizer", type=str.lower, default=None, choices=["adam", "sgd", "momentum", "adamw"],
                    help="adam (default), sgd, momentum (SGD + Nesterov momentum) or adamw (Adam with decoupled weight decay)")
    ap.add_argument("--momentum", type=float, default=None,
                    help="constant momentum of --optimizer momentum; unset: cyclical between --min_momentum and "
                         "--max_momentum along a computed schedule (clr, one_cycle, exp_decr, lr_range_test)")
    ap.add_argument("--min_momentum", type=float, default=0.85, help="lower bound of the cyclical momentum")
    ap.add_argument("--max_momentum", type=float, default=0.95, help="upper bound of the cyclical momentum")
    ap.add_argument("--weight_decay", type=float, default=None,
                    help="decoupled weight decay of adamw (default 1e-4); for momentum it replaces the schedule's L2 "
                         "regularisation; sgd and adam ignore it")
    ap.add_argument("--clip_grad_norm", type=float, default=-1.0,
                    help="> 0: clip the norm of every gradient tensor to this value; <= 0 (default): off")


def optimizer_kwargs(flags):
    """The trainer's optimiser arguments from parsed flags (a namespace without them: the defaults, Adam)."""
    return dict(optimizer=getattr(flags, "optimizer", None) or "adam", momentum=getattr(flags, "momentum", None),
                min_momentum=getattr(flags, "min_momentum", 0.85), max_momentum=getattr(flags, "max_momentum", 0.95),
                weight_decay=getattr(flags, "weight_decay", None), clip_grad_norm=getattr(flags, "clip_grad_norm", -1.0))


POLICY_ARGUMENTS = (("clr_min_lr", float), ("clr_max_lr", float), ("clr_stepsize", int), ("clr_gamma", float),
                    ("clr_mode", str), ("one_cycle_annealing_factor", float), ("start_lr", float), ("end_lr", float))


def add_schedule_arguments(ap):
    ap.add_argument("--training_schedule", default="long_schedule",
                    help="long_schedule (default), fine_schedule, short_schedule, finetune_sintel_s1..5, finetune_kitti_s1..4, "
                         "finetune_rob, clr, one_cycle, exp_decr, lr_range_test (src/training_schedules.py)")
    for name, typ in POLICY_ARGUMENTS:
        ap.add_argument("--" + name, type=typ, default=None)


def schedule_of(flags):
    """(schedule, parameters of the computed policies: clr / one_cycle / exp_decr / lr_range_test; net.py:1139-1190)."""
    sched_name = getattr(flags, "training_schedule", "long_schedule").lower()
    if sched_name not in SCHEDULES:
        raise ValueError("--training_schedule must be one of: %s" % ", ".join(sorted(SCHEDULES)))
    return SCHEDULES[sched_name], {k: getattr(flags, k) for k, _ in POLICY_ARGUMENTS if getattr(flags, k, None) is not None}


def add_unsupervised_arguments(ap):
    ap.add_argument("--unsupervised", action="store_true",
                    help="train without ground truth on the occlusion-aware photometric loss: `image_a image_b` lines are "
                         "accepted, --batch is even (batch / 2 pairs per step, both directions); needs --no-augment or "
                         "--augmentation pair")
    ap.add_argument("--photometric_q", type=float, default=0.4, help="exponent of the robust loss (|d| + 0.01)^q")
    ap.add_argument("--data_term", default="photometric", choices=["photometric", "census"],
                    help="data term of --unsupervised: photometric (default: raw brightness differences) or census (the "
                         "ternary census transform, for pairs whose exposure changes between the frames; src/census.py)")
    ap.add_argument("--occ_alpha", type=float, default=0.01, help="forward-backward test: factor on the squared magnitudes")
    ap.add_argument("--occ_beta", type=float, default=0.5, help="forward-backward test: constant, in pixels^2 of the level")
    ap.add_argument("--smoothness_weight", type=float, default=0.0,
                    help="> 0: add the edge-aware smoothness term times this weight (untuned; 0, the default: off)")
    ap.add_argument("--smoothness_order", type=int, default=1, help="1: first differences of the flow, 2: second differences")
    ap.add_argument("--edge_lambda", type=float, default=150.0,
                    help="edge weight exp(-edge_lambda * mean |frame difference|) of the smoothness term")


def unsupervised_kwargs(flags):
    """The trainer's unsupervised arguments from parsed flags, checked before anything touches a device."""
    from ..census import check_data_term
    data_term = check_data_term(getattr(flags, "data_term", "photometric"), True)
    if not getattr(flags, "unsupervised", False):
        if data_term != "photometric":
            raise ValueError("--data_term %s is a term of the unsupervised loss: it needs --unsupervised" % data_term)
        return {}
    if getattr(flags, "augment", True) and getattr(flags, "augmentation", "plugin") != "pair":
        raise ValueError("--unsupervised needs --no-augment: both augmentations recolour the two frames independently, "
                         "which breaks the brightness constancy the photometric loss assumes")
    if flags.batch % 2:
        raise ValueError("--unsupervised runs every pair in both directions: --batch must be even, got %d" % flags.batch)
    from ..photometric import check_constants
    alpha, beta, q = check_constants(flags.occ_alpha, flags.occ_beta, flags.photometric_q)
    kwargs = dict(unsupervised=True, photometric_q=q, occ_alpha=alpha, occ_beta=beta)
    if data_term != "photometric":  # (the default: nothing handed on)
        kwargs.update(data_term=data_term)
    from ..smoothness import check_constants as check_smoothness
    order, edge_lambda, _, weight = check_smoothness(getattr(flags, "smoothness_order", 1), getattr(flags, "edge_lambda", 150.0),
                                                     1e-3, getattr(flags, "smoothness_weight", 0.0))
    if weight > 0.0:  # (off: the trainer's own defaults, nothing handed on)
        kwargs.update(smoothness_weight=weight, smoothness_order=order, edge_lambda=edge_lambda)
    return kwargs


def add_sparse_arguments(ap):
    ap.add_argument("--sparse_gt", action="store_true",
                    help="sparse ground truth (KITTI flow .png, or .flo with unknown pixels): pixels without a label take no "
                         "part in the loss; needs --no-augment or --augmentation selflow|pair; not with --unsupervised")
    ap.add_argument("--crop", action="store_true",
                    help="cut a random --height x --width window out of every training sample (the centre window of "
                         "--val-list samples); needs --no-augment or --augmentation selflow|pair")


def sparse_kwargs(flags):
    """(trainer arguments, loader arguments) of --sparse_gt and --crop from parsed flags, checked before anything touches
    a device."""
    sparse, crop = bool(getattr(flags, "sparse_gt", False)), bool(getattr(flags, "crop", False))
    plugin = getattr(flags, "augment", True) and getattr(flags, "augmentation", "plugin") == "plugin"
    if sparse and getattr(flags, "unsupervised", False):
        raise ValueError("--sparse_gt is a supervised loss: not with --unsupervised")
    if sparse and plugin:
        raise ValueError("--sparse_gt needs --no-augment or --augmentation selflow|pair: the plugin augmentation "
                         "interpolates the flow, and a pixel without ground truth would spread")
    if sparse and getattr(flags, "model", "FlowNetS") in ("FlowNetS_interp", "FlowNet2"):
        raise ValueError("--sparse_gt covers FlowNetS, FlowNetSD, FlowNetC, FlowNetCS and FlowNetCSS")
    if crop and plugin:
        raise ValueError("--crop needs --no-augment or --augmentation selflow|pair: the plugin augmentation has its own crop")
    if crop and (flags.height < 1 or flags.width < 1):
        raise ValueError("--crop takes a --height x --width window: both must be >= 1")
    loader = {}
    if sparse:
        loader["sparse_gt"] = True
    if crop:
        loader["crop"] = (flags.height, flags.width)
    return (dict(sparse_gt=True) if sparse else {}), loader


def main(flags):
    unsup = unsupervised_kwargs(flags)
    sparse, loader_kw = sparse_kwargs(flags)
    import torch
    from .. import weights as W
    from ..trainer import FlowNetSTrainer
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(os.environ.get("FN2_BENCH_BACKEND", "nccl"), rank=rank, world_size=world)
    model = getattr(flags, "model", "FlowNetS")
    wts = W.load_weights(flags.checkpoint) if flags.checkpoint else W.init_weights(model, flags.seed)
    pre = FLYING_CHAIRS_PREPROCESS
    augmentation = getattr(flags, "augmentation", "plugin")  # 'selflow' and 'pair' keep the frame size: they have no crop
    h, w = ((pre["crop_height"], pre["crop_width"]) if flags.augment and augmentation == "plugin"
            else (flags.height, flags.width))
    schedule, train_params = schedule_of(flags)
    tr = FlowNetSTrainer(wts, flags.batch, h, w, schedule=schedule, dtype=flags.dtype, model=model,
                         **optimizer_kwargs(flags), **unsup, **sparse)
    tr.train_params = train_params
    if flags.checkpoint:  # Adam moments + global_step, when the checkpoint carries them (ours and the reference's do)
        state = load_full_checkpoint(flags.checkpoint)
        restored = tr.load_optimizer_state(state)
        if rank == 0 and restored:
            print("resumed %d optimizer slots at global step %d" % (restored, tr.step_count), flush=True)
    os.makedirs(flags.out, exist_ok=True)
    t0 = time.perf_counter()
    step0 = tr.step_count
    end = step0 + flags.steps  # --steps counts the steps of THIS run; `step` is the global step (schedule, file names)
    pairs = flags.batch // 2 if unsup else flags.batch  # (an unsupervised step fills two slots per pair)
    for step, (a, b, f) in enumerate(load_batches(flags.list, pairs, pre, flags.augment, seed=flags.seed + rank,
                                                  global_step=step0, augmentation=augmentation,
                                                  allow_unlabeled=bool(unsup), **loader_kw), step0 + 1):
        loss = tr.train_step_unsupervised(a, b) if unsup else tr.train_step(a, b, f)
        if step % flags.log_every == 0 or step == end:
            val = float(loss.item()) + (tr.l2_term() if flags.report_l2 else 0.0)
            if rank == 0:
                # rate of THIS run: steps since the resumed global step, not the global step
                print("global step %6d | loss %.5f | %.1f pairs/s" % (step, val, world * pairs * (step - step0) /
                                                                      (time.perf_counter() - t0)), flush=True)
        val_every = getattr(flags, "val_every", 0)
        validate = bool(getattr(flags, "val_list", None) and val_every and (step % val_every == 0 or step == end))
        save = step % flags.save_every == 0 or step == end
        if rank == 0 and validate:
            # validation frames come at their own size (--height/--width or the list's); the trainer's engine is built
            # at the training size (the augmentation crop when --augment): evaluate() centre-crops larger frames to it
            vb = load_batches(flags.val_list, flags.batch, pre, False, seed=0, epochs=1,
                              image_size=(flags.height, flags.width), **dict(loader_kw, crop_mode="centre"))
            if sparse:
                m = tr.evaluate_sparse(vb, getattr(flags, "val_batches", None))
                print("global step %6d | validation EPE %.4f px | Fl-all %.2f %%" % (step, m["epe"], 100.0 * m["fl_all"]),
                      flush=True)
            else:
                print("global step %6d | validation EPE %.4f px" % (step, tr.evaluate(vb, getattr(flags, "val_batches", None))),
                      flush=True)
        if rank == 0 and save:
            save_checkpoint(flags.out, step, dict(unpack_weights(tr), **tr.optimizer_state()), flags.ckpt_format,
                            stem=model.lower().replace("net", "net_"))
        if world > 1 and (validate or save):
            # rank 0 alone validates / writes: the others wait here instead of inside the next step's first bucket
            # all-reduce (whose timeout a long validation would hit); every rank takes this branch at the same steps
            torch.distributed.barrier()
        if step >= end:
            break
    return tr


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", required=True, help="text file of `image_a image_b flow.flo` triples, or a .tfrecords file of the "
                                                  "reference's converter (python -m src.tfrecord builds one)")
    ap.add_argument("--out", required=True, help="directory for the .npz checkpoints")
    ap.add_argument("--checkpoint", default=None, help=".npz / .npy / TensorFlow checkpoint prefix to continue from")
    ap.add_argument("--ckpt-format", default="npz", choices=["npz", "tf"],
                    help="tf: model.ckpt-<step> TensorFlow V2 bundles (readable by the reference's Saver.restore)")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=8, help="pairs per GPU (the reference's FlyingChairs batch size)")
    ap.add_argument("--dtype", default="f16x2", choices=["f32", "f16x2"])
    ap.add_argument("--no-augment", dest="augment", action="store_false")
    ap.add_argument("--augmentation", default="plugin", choices=["plugin", "selflow", "pair"],
                    help="plugin (default): the Caffe-style DataAugmentation / FlowAugmentation ops with their crop; selflow: "
                         "what the reference's live loader applies to image pairs (augment_all_estimation: flips, channel "
                         "permutation, colour chain per image; frames keep --height x --width); pair: selflow's with one "
                         "colour record for both frames and no contrast stage, the one --unsupervised accepts")
    ap.add_argument("--height", type=int, default=384)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--log-every", type=int, default=10)
    ap.add_argument("--save-every", type=int, default=1000)
    ap.add_argument("--report-l2", action="store_true", help="add the L2 regulariser to the printed loss")
    ap.add_argument("--val-list", dest="val_list", default=None, help="validation list file or .tfrecords (no augmentation)")
    ap.add_argument("--val-every", dest="val_every", type=int, default=0, help="validate every N steps (0 = never)")
    ap.add_argument("--val-batches", dest="val_batches", type=int, default=None, help="at most this many validation batches")
    add_schedule_arguments(ap)
    add_optimizer_arguments(ap)
    add_unsupervised_arguments(ap)
    add_sparse_arguments(ap)
    return ap


def parse_and_run(model):
    FLAGS = build_parser().parse_args()
    FLAGS.model = model
    if not os.path.exists(FLAGS.list):
        raise ValueError("list path must exist")
    return main(FLAGS)


if __name__ == "__main__":
    parse_and_run("FlowNetS")
