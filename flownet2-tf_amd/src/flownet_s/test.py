"""python -m src.flownet_s.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNetS."""
from .. import cli
from .flownet_s import FlowNetS

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNetS/flownet-S.ckpt-0')


def main():
    cli.run(FlowNetS, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
