#!/usr/bin/env python3
"""Time of the frame preparation of one meta-training batch (lp_frames_prepare: ONE launch from the packed uint8 frames to enc_rgbs, pose_input_rgbs,
real_segm and target_rgbs): 8 samples x (8 + 1) frames = 72 image rows and 8 mask rows, whole frames without a bounding-box file, first 449 x 449
frames (box side 450 -> 256: area), then 253 x 253 frames (254 -> 256: cubic).  HIP events around every call, 10 warm-up calls, 30 timed ones: median
and min ... max, for the launch alone (table and outputs already on the device) and for the whole ``hipops.frames_prepare`` call (table check on the
host, table upload, output allocation, launch).  Beside it, timed the same way, the same work composed per frame from stock torch device ops --
uint8 -> float, ``F.pad`` (reflect / replicate), ``F.interpolate`` (area | bicubic | bilinear), / 255, the product -- which is what a user could do
without the kernel (torch's ``area`` is adaptive average pooling -- whole pixels, equal weights -- so at the fractional ratio 450 / 256 it is another
filter than the definition's overlap weights and the printed image difference is large there; bicubic and bilinear state the same filter).  Last, the PIL decode of such a batch (72 JPEG frames + 8 PNG masks written to a temporary folder) per batch with 0 and with 8
loader workers: the part that stays on the host.  From the shapes the area launch reads 47 MB and writes 62 MB: about 14 us at the HBM peak.
Needs the MI355X: there is no point in timing the host path."""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, K = 8, 8


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


def batch(side, size):
    """-> (buf uint8, table, the frames as (offset, is the pose frame, mask offset | None))"""
    from latent_pose_reenactment_amd import frames
    g = torch.Generator().manual_seed(side)
    whole = (0.0, 0.0, 1.0, 1.0)
    rows, chunks, listing, at = [], [], [], 0
    for b in range(B):
        for k in range(K + 1):
            chunks.append(torch.randint(0, 256, (side * side * 3,), dtype=torch.uint8, generator=g))
            image = frames.frame_rows(at, (side, side, 3), whole, size)
            at += chunks[-1].numel()
            if k < K:
                rows.append(frames.make_row(image, image_slot=b * K + k))
                listing.append((image[0], False, None))
            else:
                chunks.append(torch.randint(0, 256, (side * side * 3,), dtype=torch.uint8, generator=g))
                mask = frames.frame_rows(at, (side, side, 3), whole, size, channel=1)
                at += chunks[-1].numel()
                rows.append(frames.make_row(image, mask, image_slot=B * K + b, mask_slot=b, product_slot=b))
                listing.append((image[0], True, mask[0]))
    return torch.cat(chunks), torch.tensor(rows, dtype=torch.int64), listing


def decode_times(side, warm, reps):
    """seconds per batch of 72 JPEG frames + 8 PNG masks decoded with PIL, with 0 and 8 DataLoader workers (median of ``reps`` batches)"""
    from PIL import Image
    rng = np.random.default_rng(0)
    out = {}
    with tempfile.TemporaryDirectory() as folder:
        for i in range(B * (K + 1)):
            smooth = np.add.outer(np.arange(side) % 256, np.arange(side) % 200)[:, :, None] / 2 + rng.integers(0, 40, (side, side, 3))
            Image.fromarray(np.clip(smooth, 0, 255).astype(np.uint8)).save(os.path.join(folder, f'{i:05d}.jpg'), quality=90)
        for i in range(B):
            Image.fromarray((rng.random((side, side, 3)) > 0.5).astype(np.uint8) * 255).save(os.path.join(folder, f'm{i:05d}.png'))

        class Samples(torch.utils.data.Dataset):
            def __len__(self):
                return B * (warm + reps)

            def __getitem__(self, index):
                b = index % B
                images = [np.array(Image.open(os.path.join(folder, f'{b * (K + 1) + k:05d}.jpg')).convert('RGB')) for k in range(K + 1)]
                images.append(np.array(Image.open(os.path.join(folder, f'm{b:05d}.png'))))
                return torch.cat([torch.from_numpy(x).reshape(-1) for x in images])
        for workers in (0, 8):
            loader = torch.utils.data.DataLoader(Samples(), batch_size=B, num_workers=workers, collate_fn=torch.cat)
            stamps = []
            for _ in loader:
                stamps.append(time.perf_counter())
            gaps = [b - a for a, b in zip(stamps[warm - 1:-1], stamps[warm:])]
            out[workers] = (statistics.median(gaps), min(gaps), max(gaps))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--decode_batches', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('frames_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from latent_pose_reenactment_amd import _lib, frames
    from latent_pose_reenactment_amd import hipops as ops
    s = a.size
    for side, name in ((449, 'area'), (253, 'cubic')):
        buf, table, listing = batch(side, s)
        dev = buf.cuda()
        n = side + 1
        counts = frames.check_table(table, buf.numel(), s)
        table_dev = table.cuda()
        outs = [torch.empty(c, 3, s, s, device='cuda') for c in counts]
        stream = torch.cuda.current_stream().cuda_stream

        def launch():
            _lib.check(_lib.lib().lp_frames_prepare(dev.data_ptr(), dev.numel(), table.data_ptr(), table_dev.data_ptr(), table.shape[0], s,
                                                    outs[0].data_ptr(), counts[0], outs[1].data_ptr(), counts[1], outs[2].data_ptr(), counts[2],
                                                    ctypes.c_void_p(stream)), 'lp_frames_prepare')

        def call():
            return ops.frames_prepare(dev, table, s)

        def stock():
            images, masks, products = [], [], []
            for off, is_pose, mask_off in listing:
                # the view frame[1:-1, 1:-1] and the box 1 pixel out at the top and left, 2 at the bottom and right
                frame = dev[off - side * 3 - 3:][:side * side * 3].view(side, side, 3)[1:-1, 1:-1].permute(2, 0, 1)[None].float()
                crop = F.pad(frame, (1, 2, 1, 2), mode='reflect')
                image = (F.interpolate(crop, size=(s, s), mode='area') if s <= n else
                         F.interpolate(crop, size=(s, s), mode='bicubic', align_corners=False).clamp(0, 255)) / 255
                images.append(image)
                if is_pose:
                    m = dev[mask_off - side * 3 - 3 - 1:][:side * side * 3].view(side, side, 3)[1:-1, 1:-1, 1][None, None].float()
                    m = F.pad(F.pad(m, (1, 2, 0, 2), mode='replicate'), (0, 0, 1, 0))
                    m = (F.interpolate(m, size=(s, s), mode='bilinear', align_corners=False) / 255).expand(1, 3, s, s).contiguous()
                    masks.append(m)
                    products.append(image * m)
            return torch.cat(images), torch.cat(masks), torch.cat(products)

        l_med, l_min, l_max = timed(launch, a.warmup, a.reps)
        c_med, c_min, c_max = timed(call, a.warmup, a.reps)
        s_med, s_min, s_max = timed(stock, a.warmup, a.reps)
        got, ref = call(), stock()
        order = [i for i, (_, is_pose, _) in enumerate(listing) if not is_pose] + [i for i, (_, is_pose, _) in enumerate(listing) if is_pose]
        ref_image = ref[0][order]
        read = table.shape[0] * n * n * 3 + B * n * n
        wrote = 4 * 3 * s * s * sum(counts)
        print(f'[frames_micro] {name}: {table.shape[0]} image rows + {B} mask rows, {n} x {n} -> {s} x {s}: reads {read / 1e6:.0f} MB, writes {wrote / 1e6:.0f} MB')
        print(f'[frames_micro] {name}: lp_frames_prepare, the launch alone ({a.warmup} warm-up + {a.reps} timed): median {l_med:.1f} us, '
              f'min {l_min:.1f} ... max {l_max:.1f} us')
        print(f'[frames_micro] {name}: hipops.frames_prepare, the whole call (host check, table upload, allocation, launch): median {c_med:.1f} us, '
              f'min {c_min:.1f} ... max {c_max:.1f} us')
        print(f'[frames_micro] {name}: stock torch device ops per frame (float, F.pad, F.interpolate, / 255, product; {len(listing)} frames): '
              f'median {s_med:.1f} us, min {s_min:.1f} ... max {s_max:.1f} us')
        print(f'[frames_micro] {name}: kernel vs stock ops, max-abs difference: image {(got[0] - ref_image).abs().max().item():.2e}, '
              f'mask {(got[1] - ref[1]).abs().max().item():.2e}, product {(got[2] - ref[2]).abs().max().item():.2e}')
    for workers, (med, lo, hi) in decode_times(449, 2, a.decode_batches).items():
        print(f'[frames_micro] PIL decode of one batch (72 JPEG frames + 8 PNG masks, 449 x 449), {workers} workers: median {med * 1e3:.1f} ms, '
              f'min {lo * 1e3:.1f} ... max {hi * 1e3:.1f} ms per batch')


if __name__ == '__main__':
    main()
