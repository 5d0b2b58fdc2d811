#!/usr/bin/env python3
"""The drive loop WITH its output route, in frames/s, for each ``drive.py --format``: the full-size nets of ``bench.py``'s drive measurement
(MobileNetV2 pose encoder + generator at 256 x 256, fine-tuned form, eval mode, random weights), ``drive.drive_frames`` called eagerly on batches of
B driving frames resident on the device, as ``drive.main`` does, then the sequence written to a temporary directory: npy (``torch.cat(...).cpu()`` +
``np.save``), png (that copy + ``write_png_frames``), avi (``write_avi``: JPEG on the GPU, the compressed bytes to the host, the container),
png with ``--png_encoder gpu`` (``write_png_frames_gpu``: PNG on the GPU, the compressed bytes to the host, one file per frame).  The
host clock around a whole sequence, a synchronisation at either end; one warm-up sequence, then ``--reps`` timed: median, min ... max.  The npy and
png routes are the code of the commit before ``--format avi`` existed, unchanged.  Needs the MI355X."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'latent_pose_reenactment_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=128)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--png-frames', type=int, default=32, help='the png route takes about 14 ms per frame: a shorter sequence')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('drive_output_micro.py: no GPU (a time taken on the host says nothing about the MI355X)')
    import bench
    import drive
    from generators.vector_pose_unsupervised_segmentation_noBottleneck import Wrapper as GW
    from embedders.unsupervised_pose_separate_embResNeXt_segmentation import Wrapper as EW
    args = bench.make_args(256, 8, 'cuda:0', 1, 0, 'f16', finetune=True)
    torch.manual_seed(5)
    G, E = GW.get_net(args), EW.get_net(args)
    G.enable_finetuning({'embeds': torch.randn(1, args.embed_channels, device=args.device) * 0.1})
    E.enable_finetuning()
    G.eval(); E.eval()
    tmp = tempfile.mkdtemp(prefix='drive_output_')

    def sequence(fmt, batch, total):
        frames = []
        for _ in range(0, total, batch):
            frames.append(drive.drive_frames(E, G, {'pose_input_rgbs': driver[:batch]}))
        if fmt == 'avi':
            drive.write_avi(os.path.join(tmp, 'out.avi'), torch.cat(frames), 25, 90)
        elif fmt == 'png-gpu':
            drive.write_png_frames_gpu(os.path.join(tmp, 'png_gpu'), torch.cat(frames))
        elif fmt == 'none':
            torch.cat(frames)
        else:
            video = torch.cat(frames).cpu().numpy()
            if fmt == 'png':
                drive.write_png_frames(os.path.join(tmp, 'png'), video)
            else:
                np.save(os.path.join(tmp, 'out.npy'), video)

    with torch.no_grad():
        driver = torch.rand(8, 1, 3, 256, 256, device='cuda:0')
        for batch in (1, 8):
            for fmt in ('none', 'npy', 'avi', 'png-gpu', 'png'):
                total = a.png_frames if fmt == 'png' else a.frames
                sequence(fmt, batch, total)
                times = []
                for _ in range(a.reps if fmt != 'png' else min(a.reps, 3)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sequence(fmt, batch, total)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                fps = sorted(total / t for t in times)
                what = {'none': 'no output (the frames stay on the device)', 'png-gpu': '--format png --png_encoder gpu'}.get(fmt, f'--format {fmt}')
                print(f'[drive_output_micro] B = {batch}, {total} frames, {what}: median {statistics.median(fps):.0f} frames/s, '
                      f'min {fps[0]:.0f} ... max {fps[-1]:.0f} ({len(times)} timed)', flush=True)
    for name in ('out.avi', 'out.npy'):
        print(f'[drive_output_micro] {name}: {os.path.getsize(os.path.join(tmp, name)) / 1e6:.2f} MB for {a.frames} frames')
    import shutil
    shutil.rmtree(tmp)


if __name__ == '__main__':
    main()
