#!/usr/bin/env python3
"""Micro-benchmark of the stickman-to-image generator (generators/FSTH.py): forward + backward of a training pass at 256 x 256, batch 8, the plugin's
default flags (4 downsample + 4 residual blocks, widths 64 .. 512, embed 512), in the generator's operand mode (bf16x3 unless LP_PREC_G / LP_PREC say
otherwise).  Timed with device events after warm-up; the figure is the median over the repetitions, the spread min .. max.  The loss is a fixed
random projection of ``fake_rgbs``; gradients go to ``embeds`` and every parameter (``nn.fused_grad_accumulation``, as the training step runs it).
Usage: python scripts/fsth_generator_micro.py [--reps 30] [--warmup 10] [--batch 8] [--size 256] [--out profiles/fsth_generator_micro.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert args.reps >= 20, 'the median is taken over at least 20 repetitions'
    from latent_pose_reenactment_amd import nn as lpnn
    from latent_pose_reenactment_amd.fsth_generator import GeneratorFSTH
    torch.manual_seed(0)
    G = GeneratorFSTH('zero', 3, 3, 64, 512, 512, 'in', 4, 4).cuda().train()
    mode = {v: k for k, v in lpnn.PREC_NAMES.items()}[G.prec]
    g = torch.Generator().manual_seed(1)
    b, s = args.batch, args.size
    stick = (torch.rand(b, 1, 3, s, s, generator=g) * (torch.rand(b, 1, 3, s, s, generator=g) < 0.15)).cuda()
    embeds = torch.randn(b, 512, generator=g).cuda().requires_grad_(True)
    r = torch.randn(b, 3, s, s, generator=g).cuda()
    for p in G.parameters():
        p.grad = torch.zeros_like(p)
    times, fwd = [], []
    for it in range(args.warmup + args.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        dd = {'embeds': embeds, 'dec_stickmen': stick}
        G(dd)
        e1.record()
        with lpnn.fused_grad_accumulation():
            (dd['fake_rgbs'] * r).sum().backward()
        e2.record()
        e2.synchronize()
        if it >= args.warmup:
            times.append(e0.elapsed_time(e2))
            fwd.append(e0.elapsed_time(e1))
    med = statistics.median(times)
    lines = [f'# fsth generator micro: {torch.cuda.get_device_name(0)}; {args.reps} repetitions after {args.warmup} warm-up, device events',
             f'generators/FSTH.py fwd+bwd {s}x{s} bs {b} operands {mode}: median {med:.2f} ms ({min(times):.2f} .. {max(times):.2f}) = {b / med * 1e3:.0f} img/s; '
             f'forward alone {statistics.median(fwd):.2f} ms']
    print('\n'.join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
