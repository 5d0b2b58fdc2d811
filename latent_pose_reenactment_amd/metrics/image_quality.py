"""Image-quality metric of a step's batch (``--metrics image_quality``): SSIM, PSNR and L1 between ``fake_rgbs`` and ``target_rgbs[:, 0]``, over the
whole frame and -- ``--image_quality_foreground``, when the batch carries ``real_segm`` -- weighted by the foreground mask ``real_segm[:, 0, 0]``
(``target_rgbs`` is image x segmentation: a third to a half of every frame is black in both images and inflates the whole-frame figures).
One lp_image_quality launch for the batch (hipops.image_quality), then one device-to-host copy of its [B, 6] table.

Metric contract of the runner (reference runners/holycow.py:203-210): ``forward(data_dict) -> (values, counts)``; ``values[k]`` is the mean of
column k over the images where it is defined (not NaN), ``counts[k]`` their number -- 0 makes ``Meter.add`` skip the key."""
import torch
from torch import nn

from latent_pose_reenactment_amd import hipops as ops


class Wrapper:
    @staticmethod
    def get_args(parser):
        parser.add('--image_quality_foreground', action='store_bool', default=True,
                   help='also report ssim_fg / psnr_fg / l1_fg weighted by real_segm when the batch has it')

    @staticmethod
    def get_net(args):
        return Metric(args.image_quality_foreground).to(args.device)


class Metric(nn.Module):
    def __init__(self, foreground=True):
        super().__init__()
        self.foreground = bool(foreground)

    @torch.no_grad()
    def forward(self, data_dict):
        fake, real = data_dict['fake_rgbs'], data_dict['target_rgbs']
        segm = data_dict.get('real_segm') if self.foreground else None
        mask = None
        if segm is not None:
            mask = segm[:, 0, 0] if segm.dim() == 5 else segm[:, 0]          # B x 1 x 3 x S x S (the step's batch) | B x 1 x S x S: a view
        table = ops.image_quality(fake, real, mask).cpu()
        values, counts = {}, {}
        for k, name in enumerate(ops.IMAGE_QUALITY_COLUMNS[:6 if mask is not None else 3]):
            col = table[:, k]
            col = col[col == col]
            counts[name] = int(col.numel())
            values[name] = float(col.mean()) if col.numel() else float('nan')
        return values, counts
