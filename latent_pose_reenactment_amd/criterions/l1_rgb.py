"""L1 image loss (reference API: criterions/l1_rgb.py:3-25): ``l1_weight`` * mean |fake_rgbs - target_rgbs[:, 0]| on the lp_l1_* reductions."""
from torch import nn

from latent_pose_reenactment_amd.nn import hip_l1_mean


class Wrapper:
    @staticmethod
    def get_args(parser):
        parser.add('--l1_weight', type=float, default=30.0)

    @staticmethod
    def get_net(args):
        return Criterion(args.l1_weight).to(args.device)


class Criterion(nn.Module):
    def __init__(self, weight):
        super().__init__()
        self.weight = weight

    def forward(self, inputs):
        fake, real = inputs['fake_rgbs'], inputs['target_rgbs']
        return {'l1_rgb': self.weight * hip_l1_mean(fake, real[:, 0])}
