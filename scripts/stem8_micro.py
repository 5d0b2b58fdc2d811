#!/usr/bin/env python3
"""Micro-benchmark of the two-source first layer of the FSTH family (csrc/conv_stem8.hip) against the generic route of the SAME tree (what LP_THIN=0
selects, and what these shapes ran before the kernels existed: torch.cat of the channel slices + NCHW -> NHWC copy + lp_act_pack + the MFMA conv /
weight-gradient / data-gradient kernels with the thin side padded).

Shapes: 64 x 256^2 x 6 -> 64 (the embedder's 64 encoder frames) and 8 x 256^2 x 6 -> 64 (one critic pass), 3x3, in the three operand modes.
  forward  the stem's form: operand planes of relu(y) only (no fp32 y)
  wgrad    weight + bias gradient from a given dy (autograd backward with only the weights requiring grad)
  dgrad    gradient w.r.t. the image (only the image requiring grad)
The two routes are ALTERNATED in one process after warm-up and timed with device events; the figure is the median, the spread is the
min .. max over the repeats.  Achieved bytes/s are against the algorithmic bytes of the shape (inputs read once, outputs written once).
Usage: python scripts/stem8_micro.py [--reps 20] [--out profiles/fsth_stem_micro.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from latent_pose_reenactment_amd import hipops as ops, nn as lpnn
    ops._STEM8 = True          # the route under test (LP_STEM8=1); ``_THIN`` False below = the generic route
    dev = 'cuda'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f'# stem8 micro: {torch.cuda.get_device_name(0)}; reps {args.reps} after {args.warmup} warm-up rounds, routes alternated, device events')
    say('# time = median us (min .. max); GB/s = algorithmic bytes / median')
    order = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]          # the critic's interleaved map
    cmap = ops.stem8_cmap(order)
    for n in (64, 8):
        g = torch.Generator().manual_seed(n)
        stick = torch.rand(n, 3, 256, 256, generator=g).to(dev)
        img = torch.rand(n, 3, 256, 256, generator=g).to(dev)
        w0 = (torch.randn(64, 6, 3, 3, generator=g) / 54 ** 0.5).to(dev)
        b0 = torch.randn(64, generator=g).to(dev)
        dy = torch.randn(n, 256, 256, 64, generator=g).to(dev)
        px = n * 256 * 256
        for prec_name, prec in (('f16', lpnn.PREC_F16), ('bf16x3', lpnn.PREC_BF16X3), ('bf16', lpnn.PREC_BF16)):
            pl = 4 if prec == lpnn.PREC_BF16X3 else 2
            algo = {'forward': px * (6 * 4 + 64 * pl), 'wgrad': px * (6 * 4 + 64 * 4), 'dgrad': px * (64 * 4 + 3 * 4)}

            def build(thin, what):
                ops._THIN = thin
                w = w0.clone().requires_grad_(what == 'wgrad')
                b = b0.clone().requires_grad_(what == 'wgrad')
                x = img.clone().requires_grad_(what == 'dgrad')
                inp = lpnn.StemInput(stick, x, cmap, 6)
                if what == 'forward':
                    return lambda: lpnn.hip_stem_conv(inp, w, b, ksize=3, prec=prec, emit16=1, want_y=False)
                y = lpnn.hip_stem_conv(inp, w, b, ksize=3, prec=prec)
                wrt = [w, b] if what == 'wgrad' else [x]

                def run():
                    ops._THIN = thin
                    return torch.autograd.grad(y, wrt, dy, retain_graph=True)
                return run
            for what in ('forward', 'wgrad', 'dgrad'):
                times = {True: [], False: []}
                fns = {}
                for thin in (True, False):
                    fns[thin] = build(thin, what)
                for it in range(args.warmup + args.reps):
                    for thin in (True, False):
                        ops._THIN = thin
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fns[thin]()
                        e1.record()
                        e1.synchronize()
                        if it >= args.warmup:
                            times[thin].append(e0.elapsed_time(e1) * 1e3)
                med = {k: statistics.median(v) for k, v in times.items()}
                row = f'{n:3d}x256x256x6->64 3x3 {prec_name:7s} {what:8s}'
                for thin, name in ((True, 'stem8'), (False, 'generic')):
                    row += f' | {name} {med[thin]:8.1f} us ({min(times[thin]):.1f} .. {max(times[thin]):.1f}) {algo[what] / med[thin] * 1e-3:7.1f} GB/s'
                spread = max(max(v) - min(v) for v in times.values())
                row += f' | generic / stem8 = {med[False] / med[True]:.2f}x, spread {spread:.1f} us'
                say(row)
                del fns
        ops._THIN = True
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
