#!/usr/bin/env python3
"""Time of the blur and fade of padded bands (lp_frames_pad, csrc/frames_pad.hip) on one meta-training batch: 8 samples x (8 + 1) frames = 72 image
rows and 8 mask rows, 449 x 449 frames (447 x 447 views), box side 450 -> 256, in two variants:
  (a) every box 1 pixel out at the top and left and 2 at the bottom and right -- an already-cropped dataset: a rim of tiles is blurred, the rest copied;
  (b) every box 60 pixels out at the top and left -- a bounding-box file whose scaled boxes leave the raw frames.
HIP events around every call, 10 warm-up calls, 30 timed ones: median and min ... max, for
  - the pad launches alone (plan, weights and scratch already on the device),
  - the prepare launch alone on the rewritten table and on the original one (the latter is the launch of a run without the flag),
  - the whole ``frames.prepare`` with the flag on and off (pinned host-to-device copy of the packed bytes, host-side plan and checks, launches),
  - the same pad work composed per frame from stock torch device ops: ``F.pad`` (reflect / replicate), two ``conv2d`` passes of k taps on the
    reflect-padded crop, a sort per channel for the median, the pointwise blends with precomputed weight maps, round, clamp, uint8 HWC.
From the shapes the pad launches read the 45 MB of crops twice (histogram, main) and write them once: about 21 us at the achievable HBM rate.
Needs the MI355X: there is no point in timing the host path."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, K, SIDE = 8, 8, 449


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


def batch(out, size):
    """``out`` = 0: the whole frame's box (1 | 2 pixels out); > 0: the box moved ``out`` pixels out at the top and left -> (buf, table)"""
    from latent_pose_reenactment_amd import frames
    g = torch.Generator().manual_seed(out)
    rows, chunks, at = [], [], 0

    def columns(channel=None):
        nonlocal at
        smooth = (torch.arange(SIDE)[:, None, None] * 0.3 + torch.arange(SIDE)[None, :, None] * 0.2 + torch.randint(0, 60, (SIDE, SIDE, 3), generator=g))
        chunks.append(smooth.clamp(0, 255).to(torch.uint8).reshape(-1))
        cols = frames.frame_rows(at, (SIDE, SIDE, 3), (0.0, 0.0, 1.0, 1.0), size, channel=channel)
        at += chunks[-1].numel()
        if out:
            n = cols[7] - cols[5]
            cols[5:9] = [-out, -out, n - out, n - out]
        return cols
    for b in range(B):
        for k in range(K):
            rows.append(frames.make_row(columns(), image_slot=b * K + k))
        rows.append(frames.make_row(columns(), columns(channel=1), image_slot=B * K + b, mask_slot=b, product_slot=b))
    return torch.cat(chunks), torch.tensor(rows, dtype=torch.int64)


def stock_pad(dev, plan, weights_dev, maps):
    """the plan's work from stock torch device ops, one frame at a time -> the workspace images as a list of uint8 [n, n, C]"""
    outs = []
    for p, g in zip(plan, weights_dev):
        _, view, off, h, w, rs, ps, t, l, n, pt, pl, pb, pr, k, _ = p
        radius = (k - 1) // 2
        a, f = maps[view]
        src = torch.as_strided(dev, (h, w, 1 if view else 3), (rs, ps, 1), off).permute(2, 0, 1)[None].float()
        inner = src[:, :, max(t, 0):min(t + n, h), max(l, 0):min(l + n, w)]
        if view:
            crop = F.pad(F.pad(inner, (pl, pr, 0, pb), mode='replicate'), (0, 0, pt, 0))
        else:
            crop = F.pad(inner, (pl, pr, pt, pb), mode='reflect')
        chans = crop.shape[1]
        taps = g[:k]
        blur = F.conv2d(F.pad(crop, (radius, radius, 0, 0), mode='reflect'), taps.view(1, 1, 1, k).expand(chans, 1, 1, k), groups=chans)
        blur = F.conv2d(F.pad(blur, (0, 0, radius, radius), mode='reflect'), taps.view(1, 1, k, 1).expand(chans, 1, k, 1), groups=chans)
        x = crop + (blur - crop) * a
        if view:
            y = x - x * f
        else:
            v = crop.view(chans, -1).sort(dim=1).values
            fade = ((v[:, (n * n - 1) // 2] + v[:, (n * n) // 2]) / 2).view(1, chans, 1, 1)
            y = x + (fade - x) * f
        outs.append(y.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).contiguous())
    return outs


def weight_maps(p):
    """a and f of one plan row as device tensors [n, n] (formed once per variant, outside the timed region)"""
    from latent_pose_reenactment_amd import frames
    n, pt, pl, pb, pr = p[9], p[10], p[11], p[12], p[13]
    mh, mv = frames._side(n, pl, pr)[None, :], frames._side(n, pt, pb)[:, None]
    m = torch.maximum(mh, mv)
    a = (3.0 * m + 1.0).clamp(0.0, 1.0)
    return {0: (a.cuda(), m.clamp(0.0, 1.0).cuda()), 1: (a.cuda(), mh.expand(n, n).clamp(0.0, 1.0).cuda())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('frames_pad_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import _lib, frames
    from latent_pose_reenactment_amd import hipops as ops
    s = a.size
    for out, name in ((0, '(a) 1 | 2 pixels out'), (60, '(b) 60 pixels out at the top and left')):
        buf, table = batch(out, s)
        buf = buf.pin_memory()
        table2, plan, weights, total = frames.pad_plan(table, buf.numel(), s)
        dev = torch.empty(total, dtype=torch.uint8, device='cuda')
        dev[:buf.numel()] = buf.cuda()
        plans = plan.shape[0]
        plan_dev, weights_dev = plan.cuda(), weights.cuda()
        hist, median = torch.empty(plans * 768, dtype=torch.int32, device='cuda'), torch.empty(plans * 3, device='cuda')
        counts = frames.check_table(table, buf.numel(), s)
        table_dev, table2_dev = table.cuda(), table2.cuda()
        outs = [torch.empty(c, 3, s, s, device='cuda') for c in counts]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        maps = weight_maps(plan[0].tolist())
        plan_list = plan.tolist()
        raw = {'buf': buf, 'table': table, 'label': torch.zeros(B, dtype=torch.int64), 'frames': K, 'pose': True}

        def pad_launches():
            _lib.check(_lib.lib().lp_frames_pad(dev.data_ptr(), dev.numel(), buf.numel(), plan.data_ptr(), plan_dev.data_ptr(), plans,
                                                weights_dev.data_ptr(), hist.data_ptr(), median.data_ptr(), stream), 'lp_frames_pad')

        def prepare_launch(host, device, nbytes):
            _lib.check(_lib.lib().lp_frames_prepare(dev.data_ptr(), nbytes, host.data_ptr(), device.data_ptr(), host.shape[0], s, outs[0].data_ptr(),
                                                    counts[0], outs[1].data_ptr(), counts[1], outs[2].data_ptr(), counts[2], stream),
                       'lp_frames_prepare')

        results = [
            ('lp_frames_pad, the pad launches alone', timed(pad_launches, a.warmup, a.reps)),
            ('lp_frames_prepare alone, rewritten table', timed(lambda: prepare_launch(table2, table2_dev, dev.numel()), a.warmup, a.reps)),
            ('lp_frames_prepare alone, original table (no flag)', timed(lambda: prepare_launch(table, table_dev, buf.numel()), a.warmup, a.reps)),
            ('frames.prepare, flag on (copy, plan, checks, launches)', timed(lambda: frames.prepare(raw, s, 'cuda', True), a.warmup, a.reps)),
            ('frames.prepare, flag off (copy, checks, launch)', timed(lambda: frames.prepare(raw, s, 'cuda'), a.warmup, a.reps)),
            ('hipops.frames_pad, the call on a resident buffer', timed(lambda: ops.frames_pad(dev, buf.numel(), plan, weights), a.warmup, a.reps)),
            ('stock torch device ops per frame (pad work only)', timed(lambda: stock_pad(dev, plan_list, weights_dev, maps), a.warmup, a.reps))]
        crops = sum(p[9] * p[9] * (1 if p[1] else 3) for p in plan_list)
        images = sum(p[9] * p[9] * 3 for p in plan_list if not p[1])
        print(f'[frames_pad_micro] {name}: {plans} plan rows, n {plan_list[0][9]}, k {plan_list[0][14]}: the pad launches read {(crops + images) / 1e6:.0f} MB '
              f'and write {crops / 1e6:.0f} MB: {(2 * crops + images) / 6.3e6:.0f} us at 6.3 TB/s')
        for what, (med, lo, hi) in results:
            print(f'[frames_pad_micro] {name}: {what}: median {med:.1f} us, min {lo:.1f} ... max {hi:.1f} us')
        pad_launches()
        stock = stock_pad(dev, plan_list, weights_dev, maps)
        differ, worst, count = 0, 0, 0
        for p, ref in zip(plan_list, stock):
            got = dev[p[15]:p[15] + ref.numel()].view_as(ref)
            d = (got.int() - ref.int()).abs()
            differ, worst, count = differ + int((d != 0).sum()), max(worst, int(d.max())), count + ref.numel()
        print(f'[frames_pad_micro] {name}: kernel vs stock ops: {differ} of {count} bytes differ ({100 * differ / count:.4f} %), by at most {worst}')


if __name__ == '__main__':
    main()
