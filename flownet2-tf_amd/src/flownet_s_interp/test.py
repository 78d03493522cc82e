"""python -m src.flownet_s_interp.test --input_a I1 --matches_a MASK --sparse_flow SF.flo --out DIR
python -m src.flownet_s_interp.test --input_a LIST.txt --out DIR
(flags of /root/reference src/flownet_s_interp/test.py:60-214).  A .txt --input_a runs Net.test_batch over its
lines with --input_type (default 'image_matches': `I1 MM SF [GT [[OCC [INV]] I2]]`, src/net.py matches_line_fields);
anything else is one frame through Net.test.  --checkpoint (.npz), --dtype and --batch_size are this build's extras;
--variational_refinement (:207-214) refines the flow between --input_a and --input_b (the last field of a list line)."""
import argparse
import os

from ..net import Mode, str2bool
from .flownet_s_interp import FlowNetS_interp

FLAGS = None


def is_list(path):
    return path[-4:] == '.txt'


def main():
    net = FlowNetS_interp(mode=Mode.TEST, no_deconv_biases=FLAGS.no_deconv_biases, dtype=FLAGS.dtype)
    if not os.path.isfile(FLAGS.input_a):
        raise ValueError("'input_a' is not valid, should be a path to a folder or a single image")
    if is_list(FLAGS.input_a):  # txt with one set of inputs per line (test.py:49-65)
        return net.test_batch(
            checkpoint=FLAGS.checkpoint,
            image_paths=FLAGS.input_a,
            out_path=FLAGS.out,
            input_type=FLAGS.input_type,
            save_flo=FLAGS.save_flo,
            save_image=FLAGS.save_image,
            compute_metrics=FLAGS.compute_metrics,
            accumulate_metrics=FLAGS.accumulate_metrics,
            log_metrics2file=FLAGS.log_metrics2file,
            width=FLAGS.width,
            height=FLAGS.height,
            new_par_folder=FLAGS.new_par_folder,
            variational_refinement=FLAGS.variational_refinement,
            batch_size=FLAGS.batch_size,
        )
    return net.test(
        checkpoint=FLAGS.checkpoint,
        input_a_path=FLAGS.input_a,
        input_b_path=FLAGS.input_b,
        matches_a_path=FLAGS.matches_a,
        sparse_flow_path=FLAGS.sparse_flow,
        input_type='image_matches',
        out_path=FLAGS.out,
        gt_flow=FLAGS.gt_flow,
        save_flo=FLAGS.save_flo,
        save_image=FLAGS.save_image,
        compute_metrics=FLAGS.compute_metrics,
        new_par_folder=FLAGS.new_par_folder,
        occ_mask=FLAGS.occ_mask,
        inv_mask=FLAGS.inv_mask,
        variational_refinement=FLAGS.variational_refinement,
    )


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--input_a', type=str, required=True,
                        help='Path to first image, or to a .txt list with one set of inputs per line')
    parser.add_argument('--input_b', type=str, default=None, help='Path to second image (unused by the network)')
    parser.add_argument('--matches_a', type=str, default=None, help='Path to matches mask (single-frame mode)')
    parser.add_argument('--sparse_flow', type=str, default=None,
                        help='Sparse flow initialized from sparse matches (single-frame mode)')
    parser.add_argument('--input_type', type=str, default='image_matches',
                        help="what the lines of a .txt --input_a hold: 'image_matches' (frame 1 + matches + sparse flow) "
                             "or 'image_pairs' (frame 1 + frame 2)")
    parser.add_argument('--checkpoint', type=str, default='./checkpoints/FlowNetS/flownet-S.ckpt-0')
    parser.add_argument('--no_deconv_biases', type=str2bool, nargs='?', default=False)
    parser.add_argument('--out', type=str, required=True, help='Path to the output folder')
    parser.add_argument('--gt_flow', type=str, default=None)
    parser.add_argument('--save_flo', type=str2bool, nargs='?', default=True)
    parser.add_argument('--save_image', type=str2bool, nargs='?', default=True)
    parser.add_argument('--compute_metrics', type=str2bool, nargs='?', default=True)
    parser.add_argument('--accumulate_metrics', type=str2bool, nargs='?', default=True,
                        help='for a list: append the averages of the metrics over its lines')
    parser.add_argument('--log_metrics2file', type=str2bool, nargs='?', default=False,
                        help='for a list: write the metrics to <list name>_metrics.log instead of stdout')
    parser.add_argument('--occ_mask', type=str, default=None, help='Path to occlusions mask (1s: occluded)')
    parser.add_argument('--inv_mask', type=str, default=None, help='Path to invalid-pixel mask (1s: not evaluated)')
    parser.add_argument('--width', type=int, default=1024, help='kept for compatibility: frames are padded by their own size')
    parser.add_argument('--height', type=int, default=436, help='kept for compatibility: frames are padded by their own size')
    parser.add_argument('--batch_size', type=int, default=8, help='for a list: lines of equal size per engine launch')
    parser.add_argument('--new_par_folder', type=str, default=None)
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16', 'f16', 'f16x2'])
    parser.add_argument('--variational_refinement', type=str2bool, nargs='?', default=False,
                        help='Refine the output flow with the EpicFlow variational energy minimisation (on the GPU; '
                             'needs --input_b)')
    return parser


if __name__ == '__main__':
    FLAGS = build_parser().parse_args()
    # a list names its own matches and sparse flows: those two paths belong to the single-frame mode
    for flag in ('input_a',) if is_list(FLAGS.input_a) else ('input_a', 'matches_a', 'sparse_flow'):
        if getattr(FLAGS, flag) is None or not os.path.exists(getattr(FLAGS, flag)):
            raise ValueError('%s path must exist' % flag)
    if not os.path.isdir(FLAGS.out):
        raise ValueError('out directory must exist')
    main()
