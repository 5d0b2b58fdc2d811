"""Generator plugin (reference API: generators/FSTH.py:6-197) -- the stickman-to-image encoder-decoder the FSTH family is named after,
key-compatible state_dict before and after ``enable_finetuning``.

It reads ``dec_stickmen`` (the rendered target pose; data, no gradient) and ``embeds``, and writes ``fake_rgbs`` = the raw tanh of the head conv: no
mask, no ``fake_segm`` -- train it without the ``dice`` criterion.  There is no pose embedding: it is driven by stickman frames or, without
``dec_stickmen`` in the batch, by ``dec_keypoints`` tracks that are rendered on the device at ``--image_size`` (fsth.stickmen).
``--gen_padding reflection`` would reflect-pad the stem too and is refused at construction, as are ``--norm_layer`` other than ``in``,
``--gen_num_downsample_blocks`` < 2 and ``out_channels`` != 3.  Operand mode: ``nn.generator_prec()`` (LP_PREC_G) for encoder and decoder."""
from latent_pose_reenactment_amd.fsth_generator import GeneratorFSTH as Generator  # noqa: F401


class Wrapper:
    @staticmethod
    def get_args(parser):
        parser.add('--gen_padding', type=str, default='zero', help='zero|reflection')
        parser.add('--gen_num_downsample_blocks', type=int, default=4)
        parser.add('--gen_num_residual_blocks', type=int, default=4)
        parser.add('--norm_layer', type=str, default='in')

    @staticmethod
    def get_net(args):
        net = Generator(args.gen_padding, args.in_channels, args.out_channels, args.num_channels, args.max_num_channels, args.embed_channels,
                        args.norm_layer, args.gen_num_downsample_blocks, args.gen_num_residual_blocks, image_size=args.image_size)
        return net.to(args.device)
