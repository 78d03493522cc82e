"""The classic pair CLI behind `python -m src.flownet_{s,c,sd,cs,css,2}.test --input_a A --input_b B --out DIR`: the flags
and checks of the reference's six test.py files (src/flownet_s/test.py:9-51; they differ in the class and the
checkpoint path), with --checkpoint (.npz), --dtype and --occlusions (forward-backward occlusion masks and the
backward flow next to the usual outputs, Net.test) as optional extras."""
import argparse
import os

from .net import Mode, str2bool


def build_parser(checkpoint):
    parser = argparse.ArgumentParser()
    parser.add_argument('--input_a', type=str, required=True, help='Path to first image')
    parser.add_argument('--input_b', type=str, required=True, help='Path to second image')
    parser.add_argument('--out', type=str, required=True, help='Path to output flow result')
    parser.add_argument('--checkpoint', type=str, default=checkpoint,
                        help='.npz weights keyed by the reference variable names')
    parser.add_argument('--dtype', type=str, default='f32', choices=['f32', 'bf16', 'f16', 'f16x2'])
    parser.add_argument('--occlusions', type=str2bool, nargs='?', const=True, default=False,
                        help='also run the pair backwards in the same launch and write the forward-backward occlusion '
                             'masks (<name>_occ.png, <name>_occ_bw.png) and the backward flow (<name>_flow_bw.flo)')
    return parser


def parse_args(parser):
    """The parsed command line, after the reference's checks that its three paths exist."""
    flags = parser.parse_args()
    if not os.path.exists(flags.input_a):
        raise ValueError('image_a path must exist')
    if not os.path.exists(flags.input_b):
        raise ValueError('image_b path must exist')
    if not os.path.isdir(flags.out):
        raise ValueError('out directory must exist')
    return flags


def run(model, flags):
    net = model(mode=Mode.TEST, dtype=flags.dtype)
    net.test(
        checkpoint=flags.checkpoint,
        input_a_path=flags.input_a,
        input_b_path=flags.input_b,
        out_path=flags.out,
        occlusions=flags.occlusions,
    )
