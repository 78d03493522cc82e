"""python -m src.flownet_cs.test --input_a A --input_b B --out DIR: the classic pair CLI (src/cli.py) for FlowNetCS."""
from .. import cli
from .flownet_cs import FlowNetCS

FLAGS = None


def build_parser():
    return cli.build_parser('./checkpoints/FlowNetCS/flownet-CS.ckpt-0')


def main():
    cli.run(FlowNetCS, FLAGS)


if __name__ == '__main__':
    FLAGS = cli.parse_args(build_parser())
    main()
