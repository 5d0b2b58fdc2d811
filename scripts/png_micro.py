#!/usr/bin/env python3
"""Time of ``hipops.png_encode`` (csrc/png.hip) on the frames ``drive.py --format png --png_encoder gpu`` hands it -- 64 frames of 256 x 512 uint8 RGB,
the smooth + noise frames of scripts/jpeg_micro.py and the same under a disc mask (black outside) -- whole and split by call (lp_png_filter; the two
launches of lp_png_deflate_size, which the C ABI does not expose singly; the read-back of the size; lp_png_write), bytes in, out and scratch, and the
HBM time of the traffic the shapes imply at the 6.29 TB/s the README measured.  Beside it the route ``--png_encoder pil`` takes on the same frames in the
same session: the device-to-host copy of the raw frames plus one PIL PNG per frame.  The device calls are timed with HIP events, the routes that end
on the host with the wall clock around a synchronised copy; 10 warm-up calls and 30 timed ones (the PIL route: 1 + 3, it takes about a second): median,
min ... max.  Needs the MI355X: a time taken on the host says nothing about it."""
import argparse
import ctypes
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jpeg_micro import events, wall  # noqa: E402

HBM = 6.29e12          # bytes / s: the copy rate the README measured


def line(name, t, note=''):
    med = statistics.median(t)
    print(f'[png_micro] {name}: median {med:.1f} us, min {min(t):.1f} ... max {max(t):.1f} us ({len(t)} timed){note}', flush=True)
    return med


def measure(kind, frames, a):
    from PIL import Image
    from latent_pose_reenactment_amd import _lib, hipops as ops
    t, h, w, c = frames.shape
    n = h * (1 + w * c)
    l = _lib.lib()
    stream = lambda: torch.cuda.current_stream().cuda_stream
    (data, offsets), t_all = events(lambda: ops.png_encode(frames), a.warmup, a.reps)
    filtered, t_filter = events(lambda: ops.png_filter(frames), a.warmup, a.reps)
    need = l.lp_png_deflate_scratch_bytes(t, n)
    scratch = torch.empty(need, dtype=torch.uint8, device='cuda')
    offs = torch.empty(t + 1, dtype=torch.int64, device='cuda')
    out = torch.empty(data.numel(), dtype=torch.uint8, device='cuda')
    head = (ctypes.c_ubyte * 45)(*ops._png_head(h, w, c))
    _, t_size = events(lambda: l.lp_png_deflate_size(filtered.data_ptr(), t, n, scratch.data_ptr(), need, offs.data_ptr(), stream()), a.warmup, a.reps)
    _, t_back = wall(lambda: int(offs[t].item()), a.warmup, a.reps)
    _, t_write = events(lambda: l.lp_png_write(scratch.data_ptr(), need, t, n, ctypes.addressof(head), offs.data_ptr(), out.data_ptr(), out.numel(),
                                               stream()), a.warmup, a.reps)
    if not (torch.equal(out, data) and torch.equal(offs, offsets)):
        sys.exit('png_micro.py: the split calls and png_encode disagree')
    host = frames.cpu().numpy()
    first = Image.open(io.BytesIO(data[:int(offsets[1])].cpu().numpy().tobytes()))
    if not np.array_equal(np.asarray(first), host[0]):
        sys.exit('png_micro.py: the first file does not decode to the first frame')
    raw, comp = frames.numel(), data.numel()
    traffic = raw + 2 * t * n + 3 * comp          # frames in; filtered out and in; segment bytes out, in, and out again as files
    pil_bytes = sum(len((lambda b: (Image.fromarray(f).save(b, 'PNG'), b.getvalue())[1])(io.BytesIO())) for f in host[:8]) * t / min(t, 8)
    print(f'[png_micro] {kind}: {t} frames of {h} x {w} x {c}: {raw / 1e6:.2f} MB in, {comp / 1e6:.3f} MB out ({raw / comp:.2f} : 1, '
          f'{comp / t / 1e3:.1f} KB per frame; PIL default {pil_bytes / t / 1e3:.1f} KB per frame); scratch {need / 1e6:.1f} MB reserved')
    print(f'[png_micro] {kind}: traffic bound {traffic / 1e6:.1f} MB = {traffic / HBM * 1e6:.1f} us at 6.29 TB/s')
    med = line(f'{kind}: png_encode, whole (4 launches + the read-back)', t_all)
    print(f'[png_micro] {kind}:   = {med / t:.1f} us per frame, {t / med * 1e6:.0f} frames/s')
    line(f'{kind}:   lp_png_filter (1 launch)', t_filter)
    line(f'{kind}:   lp_png_deflate_size (2 launches: segment, layout)', t_size)
    line(f'{kind}:   read-back of offsets[T] (wall clock, idle stream)', t_back)
    line(f'{kind}:   lp_png_write (1 launch)', t_write)
    _, t_dev = wall(lambda: (lambda r: (r[0].cpu(), r[1].cpu()))(ops.png_encode(frames)), a.warmup, a.reps)
    line(f'{kind}: png_encode + the compressed bytes to the host (wall clock)', t_dev)

    def pil():
        for f in frames.cpu().numpy():
            Image.fromarray(f).save(io.BytesIO(), 'PNG')

    _, t_pil = wall(pil, 1, 3)
    line(f'{kind}: raw copy + PIL PNG per frame (--png_encoder pil without the files; wall clock)', t_pil)
    m = statistics.median
    print(f'[png_micro] {kind}: PIL route / device route = {m(t_pil) / m(t_dev):.1f} x', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('png_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    import jpeg_restatement as JR
    t, h, w = a.frames, a.height, a.width
    base = JR.image('smooth_noise', h, w, seed=4, t=min(t, 8))          # eight distinct frames repeated, as scripts/jpeg_micro.py
    plain = np.concatenate([base] * (-(-t // len(base))))[:t]
    yy, xx = np.mgrid[:h, :w]
    disc = (((xx % h - h / 2) ** 2 + (yy - h / 2) ** 2) < (0.39 * h) ** 2)[None, :, :, None]          # one disc per panel of the frame grid
    measure('smooth + noise', torch.from_numpy(plain).cuda(), a)
    measure('masked smooth + noise', torch.from_numpy(plain * disc).cuda(), a)


if __name__ == '__main__':
    main()
