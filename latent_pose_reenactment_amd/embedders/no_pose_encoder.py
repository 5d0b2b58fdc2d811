"""Embedder plugin (reference API: embedders/no_pose_encoder.py:6-99): embedders/FSTH.py without the stickman -- the same conv identity encoder on
the 3-channel encoder frames alone; no pose encoder."""
from latent_pose_reenactment_amd.fsth import ConvEmbedder


class Wrapper:
    @staticmethod
    def get_args(parser):
        parser.add('--embed_padding', type=str, default='zero', help='zero|reflection')
        parser.add('--embed_num_blocks', type=int, default=6)
        parser.add('--average_function', type=str, default='sum', help='sum|max')

    @staticmethod
    def get_net(args):
        return Embedder(args.embed_padding, args.in_channels, args.out_channels, args.num_channels, args.max_num_channels, args.embed_channels,
                        args.embed_num_blocks, args.average_function).to(args.device)


class Embedder(ConvEmbedder):
    def __init__(self, padding, in_channels, out_channels, num_channels, max_num_channels, embed_channels, embed_num_blocks, average_function):
        super().__init__(padding, in_channels, out_channels, num_channels, max_num_channels, embed_channels, embed_num_blocks, average_function,
                         with_stickman=False)
