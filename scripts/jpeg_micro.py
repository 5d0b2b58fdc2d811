#!/usr/bin/env python3
"""Time of ``hipops.jpeg_encode`` (csrc/jpeg.hip) on the frames ``drive.py --format avi`` hands it -- 64 frames of 256 x 512 uint8 RGB at quality 90 --
whole and split by launch (lp_jpeg_transform; the four launches of lp_jpeg_entropy_size; the read-back of the size; lp_jpeg_entropy_write), bytes in
and out, and the two shape bounds: HBM time for the traffic at 8 TB/s and issue time for the work at the 157 TFLOP/s fp32-vector peak.  Beside it the
same frames through the routes drive.py had before: the device-to-host copy of the raw frames (all of ``--format npy`` but the file), that copy plus
one PIL PNG per frame (``--format png``), and that copy plus one PIL JPEG per frame (what a host-side Motion-JPEG writer would cost).  The device
routes are timed with HIP events, the host routes with the wall clock around a synchronised copy; 10 warm-up calls and 30 timed ones (the PIL routes:
1 + 3, they take seconds): median, min ... max.  Needs the MI355X: a time taken on the host says nothing about it."""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def events(fn, warmup, reps):
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


def wall(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6)
    return out, times


def line(name, t, note=''):
    med = statistics.median(t)
    print(f'[jpeg_micro] {name}: median {med:.1f} us, min {min(t):.1f} ... max {max(t):.1f} us ({len(t)} timed){note}', flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('jpeg_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from PIL import Image
    import jpeg_restatement as JR
    from latent_pose_reenactment_amd import _lib, hipops as ops
    from latent_pose_reenactment_amd.utils import mjpeg
    t, h, w, q = a.frames, a.height, a.width, a.quality
    # photographic statistics: smooth waves + noise, eight distinct frames repeated
    base = JR.image('smooth_noise', h, w, seed=4, t=min(t, 8))
    frames = torch.from_numpy(np.concatenate([base] * (-(-t // len(base))))[:t]).cuda()
    header = mjpeg.jpeg_header(h, w, q)
    rows, mcus = (h + 7) // 8, (w + 7) // 8

    (data, offsets), t_all = events(lambda: ops.jpeg_encode(frames, q), a.warmup, a.reps)
    coefs, t_tr = events(lambda: ops.jpeg_transform(frames, q), a.warmup, a.reps)
    l = _lib.lib()
    need = l.lp_jpeg_entropy_scratch_bytes(t, rows, mcus)
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda')
    offs = torch.empty(t + 1, dtype=torch.int64, device='cuda')
    head = torch.frombuffer(bytearray(header), dtype=torch.uint8).cuda()
    out = torch.empty(data.numel(), dtype=torch.uint8, device='cuda')
    stream = lambda: torch.cuda.current_stream().cuda_stream
    _, t_size = events(lambda: l.lp_jpeg_entropy_size(coefs.data_ptr(), t, rows, mcus, len(header), scratch.data_ptr(), need, offs.data_ptr(), stream()),
                       a.warmup, a.reps)
    _, t_back = wall(lambda: int(offs[t].item()), a.warmup, a.reps)
    _, t_write = events(lambda: l.lp_jpeg_entropy_write(scratch.data_ptr(), need, t, rows, mcus, head.data_ptr(), len(header), out.data_ptr(), out.numel(),
                                                        stream()), a.warmup, a.reps)
    if not torch.equal(out, data):
        sys.exit('jpeg_micro.py: the split calls and jpeg_encode disagree')
    raw, comp = frames.numel(), data.numel()
    work = 2.0 * t * rows * mcus * 64 * 3 * (5 + 16)          # colour transform + two 8-term passes per coefficient
    traffic = raw + 2 * coefs.numel() * 2 * 2 + 3 * comp      # frames in; coefficients out, in twice (count, pack); scan written, read twice, written
    print(f'[jpeg_micro] {t} frames of {h} x {w}, quality {q}: {raw / 1e6:.2f} MB in, {comp / 1e6:.3f} MB out ({raw / comp:.1f} : 1, '
          f'{comp / t / 1e3:.1f} KB per frame); scratch {need / 1e6:.1f} MB reserved')
    print(f'[jpeg_micro] bounds: {traffic / 1e6:.1f} MB of traffic = {traffic / 8e12 * 1e6:.1f} us at 8 TB/s; {work / 1e9:.2f} GFLOP = '
          f'{work / 157e12 * 1e6:.1f} us at 157 TFLOP/s fp32 vector')
    med = line('jpeg_encode, whole (6 launches + the read-back)', t_all)
    print(f'[jpeg_micro]   = {med / t:.1f} us per frame, {t / med * 1e6:.0f} frames/s')
    line('  lp_jpeg_transform (1 launch)', t_tr)
    line('  lp_jpeg_entropy_size (4 launches: count, pack, stuff, layout)', t_size)
    line('  read-back of offsets[T] (wall clock, idle stream)', t_back)
    line('  lp_jpeg_entropy_write (1 launch)', t_write)
    _, t_dev = wall(lambda: (lambda r: (r[0].cpu(), r[1].cpu()))(ops.jpeg_encode(frames, q)), a.warmup, a.reps)
    line('jpeg_encode + the compressed bytes to the host (wall clock)', t_dev)

    _, t_copy = wall(lambda: frames.cpu().numpy(), a.warmup, a.reps)
    line('raw copy to the host (--format npy without the file; wall clock)', t_copy)

    def png():
        for f in frames.cpu().numpy():
            Image.fromarray(f).save(io.BytesIO(), 'PNG')

    def pil_jpeg():
        for f in frames.cpu().numpy():
            Image.fromarray(f).save(io.BytesIO(), 'JPEG', quality=q, subsampling=0)

    _, t_png = wall(png, 1, 3)
    line('raw copy + PIL PNG per frame (--format png without the files; wall clock)', t_png)
    _, t_pj = wall(pil_jpeg, 1, 3)
    line('raw copy + PIL JPEG per frame, subsampling=0 (wall clock)', t_pj)
    m = statistics.median
    print(f'[jpeg_micro] against jpeg_encode + copy: raw copy {m(t_copy) / m(t_dev):.2f} x, PNG {m(t_png) / m(t_dev):.0f} x, PIL JPEG {m(t_pj) / m(t_dev):.0f} x')


if __name__ == '__main__':
    main()
