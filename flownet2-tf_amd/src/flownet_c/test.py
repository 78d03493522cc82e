"""python -m src.flownet_c.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNetC."""
from .. import cli
from .flownet_c import FlowNetC

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNetC/flownet-C.ckpt-0')


def main():
    cli.run(FlowNetC, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
