#!/usr/bin/env python3
"""Time of one ``hipops.image_quality`` call (lp_image_quality: the tile kernel plus its finish launch) on a batch of the training step's shape:
B = 8, 3 x 256 x 256, target as ``[:, 0]`` of the 5-D tensor, mask as ``real_segm[:, 0, 0]`` of the expanded segmentation.  HIP events around every
call, 10 warm-up calls, 30 timed ones: median and min ... max; beside it the 30 calls between ONE pair of events (per call: what a step that calls
the metric back to back would see, without the events' own cost).  From the shapes the launch reads B (2 C + 1) H W x 4 bytes and does about
110 C fused multiply-adds per pixel in the two window passes.  Needs the MI355X: there is no host path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--no-mask', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('image_quality_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import hipops as ops
    b, s, c = a.batch, a.size, 3
    g = torch.Generator().manual_seed(0)
    segm = (torch.rand(b, 1, 1, s, s, generator=g) > 0.4).float().cuda().expand(b, 1, 3, s, s)
    real = torch.rand(b, 1, c, s, s, generator=g).cuda() * segm
    fake = (real[:, 0] + 0.05 * torch.randn(b, c, s, s, generator=g).cuda()).contiguous()
    mask = None if a.no_mask else segm[:, 0, 0]
    for _ in range(a.warmup):
        table = ops.image_quality(fake, real, mask)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.image_quality(fake, real, mask)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        ops.image_quality(fake, real, mask)
    e1.record()
    e1.synchronize()
    batched = e0.elapsed_time(e1) * 1e3 / a.reps
    nbytes = 4 * b * s * s * (2 * c + (0 if a.no_mask else 1))
    fma = 110 * c * b * s * s
    med = statistics.median(times)
    print(f'[image_quality_micro] B {b} x {c} x {s} x {s}, mask {"no" if a.no_mask else "yes"}: {nbytes / 1e6:.1f} MB read, {fma / 1e6:.0f} M FMA per call')
    print(f'[image_quality_micro] per call between its own events ({a.warmup} warm-up + {a.reps} timed): median {med:.1f} us, '
          f'min {min(times):.1f} ... max {max(times):.1f} us')
    print(f'[image_quality_micro] {a.reps} calls between one pair of events: {batched:.1f} us per call '
          f'({nbytes / batched / 1e6:.2f} TB/s of input, {2 * fma / batched / 1e6:.2f} TFLOP/s fp32)')
    print('[image_quality_micro] table row 0:', [round(v, 5) for v in table[0].tolist()])


if __name__ == '__main__':
    main()
