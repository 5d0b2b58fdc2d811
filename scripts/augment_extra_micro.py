#!/usr/bin/env python3
"""Time of one ``hipops.augment_extra`` call (lp_augment_extra: elastic, median, saturation and JPEG of the pose image in ONE launch) on a batch of
the training step's shape: B = 8, 3 x 256 x 256, the ``[:, 0]`` view of the 5-D batch tensor, ALL FOUR steps on in every row.  HIP events around
every call, 10 warm-up calls, 30 timed ones: median and min ... max.  Beside it, timed the same way, the same chain composed from stock torch device
ops -- the hash in int64 ops, ``grid_sample`` (bilinear, reflection), reflect ``pad`` + nine shifted views + ``sort``, pointwise ops, two 8 x 8
``matmul``s each way around ``round`` -- which is what a user could do without the kernel; it states the same definition, so the two outputs are
compared (the share of pixels that agree to 1e-4 is printed: a coefficient that rounds the other way moves a whole 8 x 8 block).  From the shapes
the launch reads and writes one image of B x 3 x H x W fp32 each way = 12.6 MB (about 1.6 us at the 8 TB/s HBM peak), and executes per pixel about
4 x 8 x 3 multiply-adds for the DCT passes, 27 for the bilinear taps, 3 x 38 min / max for the median, about 60 more for hash, saturation and colour
transforms: 300 fp32 operations x 524288 pixels = 0.16 GFLOP, about 1 us at the 157 TFLOP/s fp32-vector peak -- both bounds are far below a launch.
Printed beside the result: the first stage's 70 us and the 38.7 ms meta-training step (README).  Needs the MI355X."""
import argparse
import math
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
        sys.exit('augment_extra_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import augmentation as AUG, hipops as ops
    b, s = a.batch, a.size
    assert s % 8 == 0, 'the stock-op chain is written for whole JPEG blocks'
    g = torch.Generator().manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(s) / s, torch.arange(s) / s, indexing='ij')
    waves = torch.stack([0.5 + 0.3 * torch.sin(2 * math.pi * ((1 + i % 3) * xx + (1 + i % 2) * yy) + i) for i in range(3 * b)]).reshape(b, 3, s, s)
    pose = (waves + 0.05 * torch.rand(b, 3, s, s, generator=g)).clamp(0, 1)[:, None].repeat(1, 2, 1, 1, 1).cuda()[:, :1]          # a [:, 0] view
    params = torch.zeros(b, 16)
    params[:, 0] = torch.linspace(0.5, 3.5, b)
    params[:, 1] = torch.arange(b) * 1000.0 + 17.0
    params[:, 2] = 1.0
    params[:, 3] = torch.linspace(-20.0, 20.0, b) / 255.0
    params[:, 4] = torch.linspace(70, 99, b).round()
    params = params.cuda()

    def kernel():
        return ops.augment_extra(pose, params)

    # the same chain from stock device ops
    n = (torch.arange(s, dtype=torch.int64)[:, None] * s + torch.arange(s, dtype=torch.int64)[None, :]).cuda()
    keys = ((params[:, 1].long() * AUG.EXTRA_KEY) & 0xFFFFFFFF)[:, None, None]
    base = torch.stack(torch.meshgrid(torch.arange(s, dtype=torch.float32), torch.arange(s, dtype=torch.float32), indexing='ij')[::-1], -1).cuda()
    cm = AUG._dct_matrix().cuda()
    q = torch.stack([torch.stack([t[0], t[1], t[1]]) for t in (AUG.quant_tables(int(v)) for v in params[:, 4].tolist())]).cuda()[:, :, None, None]
    pad_index = torch.tensor([1] + list(range(s)) + [s - 2]).cuda()

    def stock():
        x = pose[:, 0]
        u = [(AUG._mix32(((2 * n + j) & 0xFFFFFFFF) ^ keys) >> 8).float() * 2.0 ** -23 - 1.0 for j in (0, 1)]
        grid = (base[None] + params[:, 0, None, None, None] * torch.stack(u, -1)) * (2.0 / (s - 1)) - 1.0
        x = F.grid_sample(x, grid, mode='bilinear', padding_mode='reflection', align_corners=True)
        wide = x[:, :, pad_index][:, :, :, pad_index]
        x = torch.stack([wide[:, :, i:i + s, j:j + s] for i in range(3) for j in range(3)]).sort(0).values[4]
        big, small = x.amax(1, keepdim=True), x.amin(1, keepdim=True)
        sat = torch.where(big > 0, (big - small) / big.clamp_min(1e-30), torch.zeros_like(big))
        t = sat.clamp_min(AUG.S0)
        x = big - (big - x) * ((t + params[:, 3, None, None, None]).clamp(0, 1) / t)
        r, gg, bb = (255.0 * x).unbind(1)
        planes = torch.stack([0.299 * r + 0.587 * gg + 0.114 * bb - 128.0, -0.168736 * r - 0.331264 * gg + 0.5 * bb,
                              0.5 * r - 0.418688 * gg - 0.081312 * bb], 1)
        blocks = planes.reshape(b, 3, s // 8, 8, s // 8, 8).permute(0, 1, 2, 4, 3, 5)
        coef = cm @ (blocks @ cm.t())
        coef = q * torch.round(coef / q)
        yv, cb, cr = ((cm.t() @ coef) @ cm).permute(0, 1, 2, 4, 3, 5).reshape(b, 3, s, s).unbind(1)
        yv = yv + 128.0
        return (torch.stack([yv + 1.402 * cr, yv - 0.344136 * cb - 0.714136 * cr, yv + 1.772 * cb], 1) / 255.0).clamp(0, 1)

    k_med, k_min, k_max = timed(kernel, a.warmup, a.reps)
    s_med, s_min, s_max = timed(stock, a.warmup, a.reps)
    out, ref = kernel()[:, 0], stock()
    diff = (out - ref).abs()
    nbytes = 4 * b * s * s * 3 * 2
    print(f'[augment_extra_micro] B {b} x 3 x {s} x {s}, elastic + median + saturation + JPEG in every row: {nbytes / 1e6:.1f} MB moved per call '
          f'({nbytes / 8e12 * 1e6:.1f} us at 8 TB/s), about {300 * b * s * s / 1e9:.2f} GFLOP ({300 * b * s * s / 157e12 * 1e6:.1f} us at 157 TFLOP/s fp32 vector)')
    print(f'[augment_extra_micro] hipops.augment_extra, one launch ({a.warmup} warm-up + {a.reps} timed): median {k_med:.1f} us, '
          f'min {k_min:.1f} ... max {k_max:.1f} us')
    print(f'[augment_extra_micro] stock torch device ops (int64 hash, grid_sample, pad + sort, pointwise, 8 x 8 matmuls): median {s_med:.1f} us, '
          f'min {s_min:.1f} ... max {s_max:.1f} us')
    print(f'[augment_extra_micro] kernel vs stock ops: {100.0 * (diff <= 1e-4).float().mean().item():.3f} % of the values agree to 1e-4, '
          f'median difference {diff.median().item():.2e}, max {diff.max().item():.2e}')
    print('[augment_extra_micro] beside it: the first stage (scripts/augment_micro.py) 70 us, the meta-training step 38.7 ms')


if __name__ == '__main__':
    main()
