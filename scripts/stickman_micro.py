#!/usr/bin/env python3
"""Micro-benchmark of the device stickman (csrc/stickman.hip through hipops.stickman_render) and of the host side it replaces.
(a) device: N = 72 stickmen (a batch of 8 samples: 8 x 8 encoder frames + 8 target frames) at 256 x 256, one launch each repetition, timed with device
    events after warm-up -> median, min .. max, bytes written / time, and which bound applies: the arithmetic the launch does (lane-operations counted
    from the kernel's inner loop) against the fp32 vector peak, and the bytes it writes against the HBM peak.
(b) host: wall time of three batches from dataloaders/synthetic_voxceleb2_stickmen.py (draws on the host) and from
    dataloaders/synthetic_voxceleb2_keypoints.py (draws nothing), batch 8, K = 8, 256 x 256, in the training process's own thread (num_workers = 0).
The script needs the GPU: there is no fallback.
Usage: python scripts/stickman_micro.py [--reps 30] [--warmup 10] [--n 72] [--size 256] [--batches 3] [--out profiles/stickman_micro.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# MI355X peaks the bound is judged against: 256 CUs x 4 SIMDs x 16 fp32 lanes x 2.4 GHz lane-operations (an FMA counts as one; the kernel is built
# without packed fp32 arithmetic, so this is half the 157 TFLOPS of the data sheet), HBM3E 8 TB/s
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
PEAK_HBM = 8.0e12
# lane-operations per (pixel, segment) of the inner loop in csrc/stickman.hip (sub, fma, mul, max, min, 2 fma, mul, fma, min; the row terms amortised)
OPS_PER_PIXEL_SEGMENT = 10.5


def device_side(args, lines):
    from latent_pose_reenactment_amd import hipops as ops
    from latent_pose_reenactment_amd.dataloaders.synthetic_voxceleb2_stickmen import PARTS, face_keypoints
    g = torch.Generator().manual_seed(0)
    pts = torch.stack([face_keypoints(g) for _ in range(args.n)]).cuda()
    out = torch.empty(args.n, 3, args.size, args.size, device='cuda')
    nseg = len(ops.stickman_table(PARTS)[0])
    times = []
    for it in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.stickman_render(pts, args.size, out=out)
        e1.record()
        e1.synchronize()
        if it >= args.warmup:
            times.append(e0.elapsed_time(e1) * 1e-3)
    med = statistics.median(times)
    written = out.numel() * 4
    t_valu = args.n * args.size * args.size * nseg * OPS_PER_PIXEL_SEGMENT / PEAK_LANE_OPS
    t_hbm = written / PEAK_HBM
    bound = 'VALU' if t_valu > t_hbm else 'write'
    lines += [f'(a) device: {args.n} stickmen {args.size}x{args.size}, {nseg} segments: median {med * 1e6:.1f} us ({min(times) * 1e6:.1f} .. {max(times) * 1e6:.1f}), '
              f'{written / 1e6:.1f} MB written = {written / med / 1e12:.2f} TB/s',
              f'    floors: arithmetic {t_valu * 1e6:.1f} us ({OPS_PER_PIXEL_SEGMENT} lane-operations per pixel and segment at the fp32 vector peak), '
              f'writes {t_hbm * 1e6:.1f} us (HBM peak) -> {bound}-bound by the floors; measured / larger floor = {med / max(t_valu, t_hbm):.2f}']


def host_side(args, lines):
    import argparse as ap
    from latent_pose_reenactment_amd.dataloaders import synthetic_voxceleb2_keypoints, synthetic_voxceleb2_stickmen
    a = ap.Namespace(image_size=args.size, n_frames_for_encoder=8, num_labels=100, synthetic_dataset_len=8 * args.batches, world_size=1, random_seed=0,
                     finetune=False)
    for mod in (synthetic_voxceleb2_stickmen, synthetic_voxceleb2_keypoints):
        loader = torch.utils.data.DataLoader(mod.Dataset.get_dataset(a, 'train'), batch_size=8, shuffle=False, num_workers=0)
        t0 = time.perf_counter()
        nbytes = 0
        for count, (data, _) in enumerate(loader, 1):
            nbytes = sum(v.numel() * v.element_size() for k, v in data.items() if 'stickmen' in k or 'keypoints' in k)
            if count == args.batches:
                break
        dt = time.perf_counter() - t0
        lines.append(f'(b) host: {mod.__name__.rsplit(".", 1)[-1]}: {args.batches} batches of 8 (K = 8, {args.size}x{args.size}) in {dt:.2f} s = {dt / args.batches:.2f} s per batch '
                     f'({torch.get_num_threads()} host threads); pose data per batch {nbytes / 1e6:.3f} MB')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--n', type=int, default=72)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batches', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stickman_micro.py needs the MI355X: the device stickman has no fallback')
    lines = [f'# stickman micro: {torch.cuda.get_device_name(0)}; {args.reps} repetitions after {args.warmup} warm-up, device events']
    device_side(args, lines)
    host_side(args, lines)
    print('\n'.join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
