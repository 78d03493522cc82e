"""python -m src.flownet_css.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNetCSS."""
from .. import cli
from .flownet_css import FlowNetCSS

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNetCSS/flownet-CSS.ckpt-0')


def main():
    cli.run(FlowNetCSS, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
