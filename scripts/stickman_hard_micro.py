#!/usr/bin/env python3
"""Micro-benchmark of the hard-edged stickman (csrc/stickman_hard.hip through hipops.stickman_render_hard) with the soft renderer
(csrc/stickman.hip through hipops.stickman_render) as the yardstick in the same run, and of the host side of the keypoint loaders.
(a) device: N = 72 stickmen (a batch of 8 samples: 8 x 8 encoder frames + 8 target frames) at 256 x 256, one launch per repetition, timed with
    device events after warm-up -> median, min .. max, bytes written / time; the hard renderer at thickness 2 with and without the face oval, then
    the soft renderer on the same keypoints.
(b) host: one raw batch (read + decode + collate, no device work; host clock) of ``dataloaders/voxceleb2.py`` and of
    ``dataloaders/voxceleb2_FSTH_crop.py``, batch 8, K = 8, from JPEG frames and landmark files this script writes to a temporary folder
    (num_workers = 0: the cost of one worker).
The script needs the GPU: there is no fallback.  It reads nothing outside the tree.
Usage: python scripts/stickman_hard_micro.py [--reps 30] [--warmup 10] [--n 72] [--size 256] [--frame 256] [--out profiles/stickman_hard_micro.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'latent_pose_reenactment_amd'))          # (plugins resolve as dataloaders.<name>)


def timed(fn, warmup, reps):
    times = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(times), min(times), max(times)


def device_side(args, lines):
    from latent_pose_reenactment_amd import hipops as ops
    from latent_pose_reenactment_amd.dataloaders.synthetic_voxceleb2_stickmen import face_keypoints
    g = torch.Generator().manual_seed(0)
    pts = torch.stack([face_keypoints(g) for _ in range(args.n)]).cuda()
    out = torch.empty(args.n, 3, args.size, args.size, device='cuda')
    written = out.numel() * 4
    results = {}
    for name, fn, nseg in (('hard, T = 2, with the oval', lambda: ops.stickman_render_hard(pts, args.size, 2, out=out), len(ops.stickman_table(ops.REFERENCE_PARTS)[0])),
                           ('hard, T = 2, without the oval', lambda: ops.stickman_render_hard(pts, args.size, 2, out=out, parts=ops.REFERENCE_PARTS_NO_OVAL),
                            len(ops.stickman_table(ops.REFERENCE_PARTS_NO_OVAL)[0])),
                           ('soft (stickman_render, width S / 64)', lambda: ops.stickman_render(pts, args.size, out=out), len(ops.stickman_table(ops.PARTS)[0]))):
        med, lo, hi = timed(fn, args.warmup, args.reps)
        results[name] = med
        lines.append(f'(a) device: {name}: {args.n} stickmen {args.size}x{args.size}, {nseg} segments: median {med * 1e6:.1f} us ({lo * 1e6:.1f} .. {hi * 1e6:.1f}), '
                     f'{written / 1e6:.1f} MB written = {written / med / 1e12:.2f} TB/s')
    hard, soft = results['hard, T = 2, with the oval'], results['soft (stickman_render, width S / 64)']
    lines.append(f'    hard (with the oval) / soft = {hard / soft:.2f}: the {"hard" if hard < soft else "soft"} renderer is faster by a factor of '
                 f'{max(hard, soft) / min(hard, soft):.2f}')


def write_tree(root, frame, videos, frames):
    from PIL import Image
    rng = np.random.default_rng(0)
    for v in range(videos):
        video = f'id{v:02d}/vid0'
        (root / 'Img' / video).mkdir(parents=True)
        (root / 'landmarks' / video).mkdir(parents=True)
        for f in range(frames):
            smooth = np.add.outer(np.arange(frame), np.arange(frame))[:, :, None] // 2 + rng.integers(0, 40, (frame, frame, 3))
            Image.fromarray(np.clip(smooth, 0, 255).astype(np.uint8)).save(root / 'Img' / video / f'{f:05d}.jpg', quality=90)
            np.save(root / 'landmarks' / video / f'{f:05d}.npy', rng.uniform(0.2 * frame, 0.9 * frame, (68, 3)))
    import pandas
    pandas.DataFrame({'path': [f'id{v:02d}/vid0' for v in range(videos)]}).to_csv(root / 'split.csv', index=False)


def host_side(args, lines):
    from latent_pose_reenactment_amd.dataloaders.dataloader import Dataloader
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        write_tree(root, args.frame, 8, 9)
        for plugin in ('voxceleb2', 'voxceleb2_FSTH_crop'):
            a = SimpleNamespace(data_root=root, img_dir=Path('Img'), kp_dir=Path('landmarks'), draw_oval=True, stickman_thickness=2, n_frames_for_encoder=8,
                                image_size=args.size, train_split_path=root / 'split.csv', val_split_path=root / 'split.csv', finetune=False,
                                inference=False, checkpoint_path='', num_labels=8, world_size=1, rank=0, batch_size=8, num_gpus=1, num_workers=0,
                                device='cpu')
            loader = Dataloader(plugin).get_dataloader(a, part='val', phase='val')
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                raw = next(iter(loader.loader))          # the raw batch: read + decode + collate, nothing prepared
                times.append(time.perf_counter() - t0)
            lines.append(f'(b) host: {plugin}: one raw batch of 8 (K = 8: 72 JPEG frames {args.frame}x{args.frame} + 72 landmark files), one process: '
                         f'{min(times) * 1e3:.1f} ms (best of 3; first {times[0] * 1e3:.1f} ms); {raw["buf"].numel() / 1e6:.1f} MB of pixels and '
                         f'{raw["keypoints"].numel() * 4 / 1e3:.1f} kB of keypoints cross PCIe')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--n', type=int, default=72)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--frame', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stickman_hard_micro.py needs the MI355X: the device stickman has no fallback')
    lines = [f'# stickman_hard micro: {torch.cuda.get_device_name(0)}; {args.reps} repetitions after {args.warmup} warm-up, device events']
    device_side(args, lines)
    host_side(args, lines)
    print('\n'.join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
