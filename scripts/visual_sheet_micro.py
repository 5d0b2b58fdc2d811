#!/usr/bin/env python3
"""Time of one ``hipops.visual_sheet`` call (lp_visual_sheet: ONE launch) at the logged shape -- N = 2 samples, P = 7 panels of 3 x 256 x 256 with a
caption strip; the panels are the views ``utils.visualize.make_visual`` hands over: ``[:2, 0]`` of 5-D batch tensors, a contiguous generator
output, a one-channel segmentation -- beside the same sheet composed from stock torch device ops (per panel clamp, mul, byte, permute, expand, then
cat).  HIP events around every call, 10 warm-up calls, 30 timed ones: median, min ... max, and bytes / time (what the launch reads and writes).
Needs the MI355X: a time taken on the host says nothing about it."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def torch_chain(panels, strip):
    cols = []
    for t in panels:
        n, c, h, w = t.shape
        cols.append(t.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).expand(n, h, w, 3).reshape(n * h, w, 3))
    return torch.cat((strip[:, :, None].expand(-1, -1, 3), torch.cat(cols, dim=1)), dim=0)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=2)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('visual_sheet_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import hipops as ops
    from latent_pose_reenactment_amd.utils import visualize
    b, s, n = a.batch, a.size, a.samples
    g = torch.Generator().manual_seed(0)
    data = {'enc_rgbs': torch.rand(b, 2, 3, s, s, generator=g).cuda(), 'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g).cuda(),
            'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g).cuda(), 'fake_rgbs': (torch.rand(b, 3, s, s, generator=g) * 1.2 - 0.1).cuda(),
            'fake_segm': torch.rand(b, 1, s, s, generator=g).cuda(),
            'pose_input_rgbs_other_person': torch.rand(b, 1, 3, s, s, generator=g).cuda(),
            'fake_rgbs_other_person': (torch.rand(b, 3, s, s, generator=g) * 1.2 - 0.1).cuda()}
    items = visualize.make_visual(data, n)
    panels = [t for _, t in items]
    strip = visualize.caption_strip([c for c, _ in items], s, visualize.caption_height(s)).cuda()
    out = torch.empty((strip.shape[0] + n * s, len(panels) * s, 3), dtype=torch.uint8, device='cuda')
    sheet, t_hip = timed(lambda: ops.visual_sheet(panels, caption=strip, out=out), a.warmup, a.reps)
    want, t_torch = timed(lambda: torch_chain(panels, strip), a.warmup, a.reps)
    if not torch.equal(sheet, want):
        sys.exit('visual_sheet_micro.py: the launch and the torch chain disagree')
    read = sum(4 * t.shape[0] * t.shape[1] * s * s for t in panels) + strip.numel()
    write = out.numel()
    print(f'[visual_sheet_micro] N {n}, P {len(panels)} ({sum(t.shape[1] == 1 for t in panels)} one-channel), {s} x {s}, strip {strip.shape[0]} rows: '
          f'{read / 1e6:.2f} MB read, {write / 1e6:.2f} MB written per sheet')
    for name, t in (('lp_visual_sheet, one launch', t_hip), ('torch chain (clamp, mul, byte, permute, expand, cat)', t_torch)):
        med = statistics.median(t)
        print(f'[visual_sheet_micro] {name}: median {med:.1f} us, min {min(t):.1f} ... max {max(t):.1f} us '
              f'({a.warmup} warm-up + {a.reps} timed); {(read + write) / med / 1e3:.1f} GB/s')
    print(f'[visual_sheet_micro] torch chain / one launch: {statistics.median(t_torch) / statistics.median(t_hip):.1f} x')


if __name__ == '__main__':
    main()
