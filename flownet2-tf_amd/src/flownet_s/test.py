"""python -m src.flownet_s.test --input_a A --input_b B --out DIR -- same flags and
checks as /root/reference src/flownet_s/test.py:9-51; --checkpoint (.npz) and
--dtype are optional extras, and so is --occlusions: forward-backward occlusion masks and the backward flow next
to the usual outputs (Net.test)."""
import argparse
import os

from ..net import Mode, str2bool
from .flownet_s import FlowNetS

FLAGS = None


def main():
    net = FlowNetS(mode=Mode.TEST, dtype=FLAGS.dtype)
    net.test(
        checkpoint=FLAGS.checkpoint,
        input_a_path=FLAGS.input_a,
        input_b_path=FLAGS.input_b,
        out_path=FLAGS.out,
        occlusions=FLAGS.occlusions,
    )


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--input_a', type=str, required=True, help='Path to first image')
    parser.add_argument('--input_b', type=str, required=True, help='Path to second image')
    parser.add_argument('--out', type=str, required=True, help='Path to output flow result')
    parser.add_argument('--checkpoint', type=str, default='./checkpoints/FlowNetS/flownet-S.ckpt-0',
                        help='.npz weights keyed by the reference variable names')
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16', 'f16', 'f16x2'])
    parser.add_argument('--occlusions', type=str2bool, nargs='?', const=True, default=False,
                        help='also run the pair backwards in the same launch and write the forward-backward occlusion '
                             'masks (<name>_occ.png, <name>_occ_bw.png) and the backward flow (<name>_flow_bw.flo)')
    return parser


if __name__ == '__main__':
    FLAGS = build_parser().parse_args()

    # Verify arguments are valid
    if not os.path.exists(FLAGS.input_a):
        raise ValueError('image_a path must exist')
    if not os.path.exists(FLAGS.input_b):
        raise ValueError('image_b path must exist')
    if not os.path.isdir(FLAGS.out):
        raise ValueError('out directory must exist')
    main()
