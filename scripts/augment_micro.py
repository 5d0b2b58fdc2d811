#!/usr/bin/env python3
"""Time of one ``hipops.augment_triplet`` call (lp_augment_triplet: ONE launch for pose image, target and mask) on a batch of the training step's
shape: B = 8, 3 x 256 x 256, the full triplet as ``[:, 0]`` views of the 5-D batch tensors, the mask ``expand``ed to 3 channels, scale + shift and
EVERY pixelwise step on (filter, multiply, add, linear and sigmoid contrast, noise).  HIP events around every call, 10 warm-up calls, 30 timed ones:
median and min ... max.  Beside it, timed the same way, the same chain composed from stock torch device ops -- ``affine_grid`` / ``grid_sample`` x 3,
``conv2d``, pointwise ops, ``randn`` -- which is what a user could do without the kernel (bilinear, reflection / zeros padding; its noise is torch's,
so the two outputs are not compared here: tests/test_augment_gpu.py holds the kernel to the fp64 restatement).  From the shapes the launch reads
and writes 2 x 3 images of B x 3 x H x W fp32 = 37.7 MB: about 5 us at the HBM peak -- both figures are
launch-latency sized.  Needs the MI355X: there is no point in timing the host path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('augment_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import hipops as ops
    b, s, c = a.batch, a.size, 3
    g = torch.Generator().manual_seed(0)
    pose = torch.rand(b, 1, c, s, s, generator=g).cuda()
    target = torch.rand(b, 1, c, s, s, generator=g).cuda()
    segm = (torch.rand(b, 1, 1, s, s, generator=g) > 0.4).float().cuda().expand(b, 1, 3, s, s)
    # one row per sample: scale (0.8 .. 1.2) + shift (up to 5 %), emboss filter, mul, per-channel add, both contrasts, noise
    sx, sy = torch.linspace(0.8, 1.2, b), torch.linspace(1.2, 0.8, b)
    tx, ty = torch.linspace(-0.05, 0.05, b) * s, torch.linspace(0.05, -0.05, b) * s
    cx = cy = (s - 1) / 2.0
    params = torch.zeros(b, 32)
    params[:, 0], params[:, 2] = 1 / sx, (cx - cx / sx) - tx / sx
    params[:, 4], params[:, 5] = 1 / sy, (cy - cy / sy) - ty / sy
    params[:, 6] = params[:, 10] = 1
    params[:, 8], params[:, 11] = -tx, -ty
    params[:, 12:21] = torch.tensor([-1.25, -0.25, 0.0, -0.25, 1.0, 0.25, 0.0, 0.25, 1.25])
    params[:, 21:29] = torch.tensor([1.2, 0.03, -0.03, 0.01, 1.1, 4.0, 0.05, 1234.0])
    params = params.cuda()

    def kernel():
        return ops.augment_triplet(pose, params, target, segm)

    # the same chain from stock device ops (normalised coordinates, align_corners=True: pixel centres at integers)
    def theta(A):
        t = torch.zeros(b, 2, 3, device='cuda')
        half = (s - 1) / 2.0
        t[:, 0, 0], t[:, 0, 1], t[:, 0, 2] = A[:, 0], A[:, 1], (A[:, 0] * half + A[:, 1] * half + A[:, 2] - half) / half
        t[:, 1, 0], t[:, 1, 1], t[:, 1, 2] = A[:, 3], A[:, 4], (A[:, 3] * half + A[:, 4] * half + A[:, 5] - half) / half
        return t
    weight = params[:, 12:21].reshape(b, 1, 3, 3)

    def stock():
        gp = F.affine_grid(theta(params[:, 0:6]), (b, c, s, s), align_corners=True)
        gt = F.affine_grid(theta(params[:, 6:12]), (b, c, s, s), align_corners=True)
        p = F.grid_sample(pose[:, 0], gp, mode='bilinear', padding_mode='reflection', align_corners=True)
        t = F.grid_sample(target[:, 0], gt, mode='bilinear', padding_mode='reflection', align_corners=True)
        m = F.grid_sample(segm[:, 0], gt, mode='bilinear', padding_mode='zeros', align_corners=True)
        p = F.pad(p, (1, 1, 1, 1), mode='reflect')
        p = F.conv2d(p.transpose(0, 1), weight, groups=b).transpose(0, 1)          # one 3 x 3 filter per sample
        p = p * params[:, 21, None, None, None] + params[:, 22:25, None, None]
        p = 0.5 + params[:, 25, None, None, None] * (p - 0.5)
        p = torch.sigmoid(params[:, 26, None, None, None] * (p - 0.5))
        p = p + params[:, 27, None, None, None] * torch.randn(b, 1, s, s, device='cuda')
        return p.clamp(0, 1), t, m

    k_med, k_min, k_max = timed(kernel, a.warmup, a.reps)
    s_med, s_min, s_max = timed(stock, a.warmup, a.reps)
    out = kernel()
    ref = stock()
    nbytes = 4 * b * s * s * 6 * c          # three logical B x 3 x H x W images read, three written
    print(f'[augment_micro] B {b} x {c} x {s} x {s}, full triplet, every pixelwise step on: {nbytes / 1e6:.1f} MB moved per call')
    print(f'[augment_micro] hipops.augment_triplet, one launch ({a.warmup} warm-up + {a.reps} timed): median {k_med:.1f} us, '
          f'min {k_min:.1f} ... max {k_max:.1f} us')
    print(f'[augment_micro] stock torch device ops (affine_grid / grid_sample x 3, conv2d, pointwise, randn): median {s_med:.1f} us, '
          f'min {s_min:.1f} ... max {s_max:.1f} us')
    # target and mask need no noise: the two paths state the same resampling
    print(f'[augment_micro] kernel vs stock ops, max-abs difference: target {(out[1][:, 0] - ref[1]).abs().max().item():.2e}, '
          f'mask {(out[2][:, 0] - ref[2]).abs().max().item():.2e}')


if __name__ == '__main__':
    main()
