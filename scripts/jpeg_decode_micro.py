#!/usr/bin/env python3
"""Time of the JPEG decode on the GPU (``--decode_jpeg_on_gpu``; csrc/jpeg_decode.hip) for one meta-training batch of the image-folder loader: the
batch of scripts/frames_micro.py -- 8 samples x (8 + 1) frames = 72 frames of 450 x 450 plus 8 PNG masks -- written as 4:2:0 quality-90 JPEG files
into a temporary VoxCeleb2-layout tree, and the same at 224 x 224, VoxCeleb2's native size.  HIP events around every device call, 10 warm-up calls,
30 timed ones: median and min ... max, for the entropy launch, the pixel launches (tables already on the device), the whole ``hipops.jpeg_decode``
call, and ``frames.prepare`` of the raw batch with and without the flag (host-to-device copies included).  On the host clock, in ONE process on the
same machine: the making of the raw batch (dataset + collate, no workers) with the flag -- file reads, header parse, PIL for the masks -- and without
it -- PIL for everything --, and the PIL decode of the 72 JPEG files alone.  The route with the flag = its raw batch + its ``frames.prepare`` (ended
by a device synchronise); the condition for calling the flag a win is that this takes less time than the PIL decode of the same files.  Also printed:
the bytes that cross PCIe either way and the HBM bound of the pixel launches from the shapes.
Needs the MI355X: there is no point in timing the host path."""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, K = 8, 8
HBM = 6.29e12          # bytes / s, the measured float4-copy rate of the MI355X


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


def host_timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(times), min(times), max(times)


def fmt(t, unit='us'):
    scale = 1e-3 if unit == 'ms' else 1.0
    return f'median {t[0] * scale:.1f} {unit}, min {t[1] * scale:.1f} ... max {t[2] * scale:.1f} {unit}'


def write_tree(root, side):
    from PIL import Image
    rng = np.random.default_rng(side)
    for b in range(B):
        (root / 'Img' / f'id{b:02d}' / 'vid').mkdir(parents=True)
        (root / 'segm' / f'id{b:02d}' / 'vid').mkdir(parents=True)
        for k in range(K + 1):
            smooth = np.add.outer(np.arange(side) % 256, np.arange(side) % 200)[:, :, None] / 2 + rng.integers(0, 40, (side, side, 3))
            Image.fromarray(np.clip(smooth, 0, 255).astype(np.uint8)).save(root / 'Img' / f'id{b:02d}' / 'vid' / f'{k:05d}.jpg', quality=90, subsampling=2)
            Image.fromarray((rng.random((side, side, 3)) > 0.5).astype(np.uint8) * 255).save(root / 'segm' / f'id{b:02d}' / 'vid' / f'{k:05d}.png')
    (root / 'videos.csv').write_text('path\n' + ''.join(f'id{b:02d}/vid\n' for b in range(B)))
    return root


def dataset_for(root, size, flag):
    from latent_pose_reenactment_amd.dataloaders.voxceleb2_segmentation_nolandmarks import Collate, Dataset
    args = SimpleNamespace(data_root=root, img_dir=Path('Img'), segm_dir=Path('segm'), bboxes_dir=root / 'none.npy', n_frames_for_encoder=K, image_size=size,
                           train_split_path=root / 'videos.csv', val_split_path=root / 'videos.csv', finetune=False, inference=False, checkpoint_path='',
                           num_labels=B, world_size=1, decode_jpeg_on_gpu=flag)
    ds = Dataset(args, 'val')
    collate = Collate(ds.frames, ds.finetuning, ds.inference)
    return lambda: collate([ds[i] for i in range(len(ds))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--host_reps', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('jpeg_decode_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    from PIL import Image
    from latent_pose_reenactment_amd import _lib, frames
    from latent_pose_reenactment_amd import hipops as ops
    from latent_pose_reenactment_amd.utils import jpeg_parse
    l = _lib.lib()
    for side in (450, 224):
        tag = f'[jpeg_decode_micro] {side} x {side}'
        folder = tempfile.TemporaryDirectory()          # (lives until the end of this size's measurements: the route reads the files again)
        root = write_tree(Path(folder.name), side)
        make_flag, make_pil = dataset_for(root, a.size, True), dataset_for(root, a.size, False)
        raw_flag, raw_pil = make_flag(), make_pil()
        assert torch.equal(raw_flag['table'], raw_pil['table']) and raw_flag['nbytes'] == raw_pil['buf'].numel()
        files = sorted((root / 'Img').glob('*/*/*.jpg'))
        blobs = [p.read_bytes() for p in files]
        t_raw_flag = host_timed(make_flag, 2, a.host_reps)
        t_raw_pil = host_timed(make_pil, 2, a.host_reps)
        t_pil = host_timed(lambda: [np.array(Image.open(p).convert('RGB')) for p in files], 2, a.host_reps)
        t_parse = host_timed(lambda: [jpeg_parse.parse(p.read_bytes()) for p in files], 2, a.host_reps)
        pk = raw_flag['jpeg']
        n, nseg, blocks, plane_bytes, nbytes = pk['frames'].shape[0], pk['seg'].shape[0], int(pk['coef_blocks']), int(pk['plane_bytes']), int(raw_flag['nbytes'])
        raw_flag['buf'], raw_pil['buf'] = raw_flag['buf'].pin_memory(), raw_pil['buf'].pin_memory()
        for k in ('scan', 'seg', 'frames', 'qt', 'huffman'):
            pk[k] = pk[k].pin_memory()
        dev = {k: pk[k].cuda() for k in ('scan', 'seg', 'frames', 'qt', 'huffman')}
        out = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
        coefs = torch.empty((blocks, 64), dtype=torch.int16, device='cuda')
        planes = torch.empty(plane_bytes, dtype=torch.uint8, device='cuda')
        status = torch.empty(n, dtype=torch.int32, device='cuda')
        Kt = jpeg_parse.idct_table()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def entropy():
            _lib.check(l.lp_jpeg_decode_entropy(dev['scan'].data_ptr(), pk['scan'].numel(), pk['seg'].data_ptr(), dev['seg'].data_ptr(), nseg,
                                                pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['huffman'].data_ptr(), coefs.data_ptr(), blocks,
                                                status.data_ptr(), stream), 'lp_jpeg_decode_entropy')

        def pixels():
            _lib.check(l.lp_jpeg_decode_pixels(coefs.data_ptr(), blocks, pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['qt'].data_ptr(),
                                               Kt.ctypes.data, planes.data_ptr(), plane_bytes, out.data_ptr(), nbytes, stream), 'lp_jpeg_decode_pixels')

        t_entropy = timed(entropy, a.warmup, a.reps)
        t_pixels = timed(pixels, a.warmup, a.reps)
        t_call = timed(lambda: ops.jpeg_decode(pk, out=out), a.warmup, a.reps)
        assert status.cpu().tolist() == [0] * n
        pending = []          # as the loader calls it: the status words are looked at later, outside the timed region
        t_prep_flag = timed(lambda: frames.prepare(raw_flag, a.size, 'cuda', pending=pending), a.warmup, a.reps)
        frames.check_decoded(pending)
        t_prep_pil = timed(lambda: frames.prepare(raw_pil, a.size, 'cuda'), a.warmup, a.reps)

        def route():
            frames.prepare(make_flag(), a.size, 'cuda')
            torch.cuda.synchronize()

        t_route = host_timed(route, 2, a.host_reps)
        folder.cleanup()
        # the decoded frames against PIL's, for the record
        got = ops.jpeg_decode(pk, out=torch.zeros(nbytes, dtype=torch.uint8, device='cuda')).buf.cpu()
        rows = pk['frames']
        inside = torch.zeros(nbytes, dtype=torch.bool)
        for r in rows.tolist():
            inside[r[10]:r[10] + r[0] * r[1] * 3] = True
        diff = (got[inside].int() - raw_pil['buf'][inside].int()).abs()
        npix = n * side * side
        moved_flag = raw_flag['buf'].numel() + sum(pk[k].numel() * pk[k].element_size() for k in ('scan', 'seg', 'frames', 'qt', 'huffman'))
        pix_bytes = 128 * blocks + 2 * 64 * blocks + 3 * npix          # coefficients read, planes written and read, pixels written
        print(f'{tag}: {n} JPEG frames (4:2:0, quality 90, {sum(len(b) for b in blobs) / 1e6:.2f} MB of files, {nseg} segments, {blocks} blocks) + {B} PNG masks')
        print(f'{tag}: lp_jpeg_decode_entropy, the launch alone ({a.warmup} warm-up + {a.reps} timed): {fmt(t_entropy)}')
        print(f'{tag}: lp_jpeg_decode_pixels, the two launches alone: {fmt(t_pixels)}; from the shapes {pix_bytes / 1e6:.1f} MB = '
              f'{pix_bytes / HBM * 1e6:.1f} us at the measured HBM rate')
        print(f'{tag}: hipops.jpeg_decode, the whole call (table upload, workspaces, three launches): {fmt(t_call)}')
        print(f'{tag}: frames.prepare with the flag (copies, decode, lp_frames_prepare): {fmt(t_prep_flag)}; without (one copy, lp_frames_prepare): {fmt(t_prep_pil)}')
        print(f'{tag}: bytes over PCIe per batch: {moved_flag / 1e6:.2f} MB with the flag, {raw_pil["buf"].numel() / 1e6:.2f} MB without '
              f'({raw_pil["buf"].numel() / moved_flag:.1f} : 1)')
        print(f'{tag}: host, one process: raw batch with the flag (read, parse, PIL masks) {fmt(t_raw_flag, "ms")}; without (PIL for all) {fmt(t_raw_pil, "ms")}')
        print(f'{tag}: host, one process: PIL decode of the {n} JPEG files alone {fmt(t_pil, "ms")}; read + parse of the same files {fmt(t_parse, "ms")}')
        print(f'{tag}: the route with the flag, raw batch + frames.prepare + synchronise, host clock: {fmt(t_route, "ms")} -- against the PIL decode of the '
              f'same files: {"faster" if t_route[0] < t_pil[0] else "SLOWER"} ({t_pil[0] / t_route[0]:.2f} x)')
        print(f'{tag}: decoded pixels against PIL: worst difference {int(diff.max())} levels, {100.0 * float((diff == 0).float().mean()):.1f} % equal')


if __name__ == '__main__':
    main()
