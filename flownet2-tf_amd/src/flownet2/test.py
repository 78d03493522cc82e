"""python -m src.flownet2.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNet2."""
from .. import cli
from .flownet2 import FlowNet2

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNet2/flownet-2.ckpt-0')


def main():
    cli.run(FlowNet2, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
