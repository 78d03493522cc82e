"""python -m src.flownet_sd.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNetSD."""
from .. import cli
from .flownet_sd import FlowNetSD

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNetSD/flownet-SD.ckpt-0')


def main():
    cli.run(FlowNetSD, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
