#!/usr/bin/env python3
"""What a logged iteration costs with ``--visuals``: wall time (host clock around a device synchronisation) of the eager meta-training step of
bench.py's flagship configuration (B = 8, 3 x 256 x 256, 8 encoder frames) alone, and of the same step followed by ``runners.holycow.log_visuals``
(the running-average forward, the cross-driving call, the sheet launch, one device-to-host copy, the PNG).  Medians over a few iterations; the
figure is informational and concerns the logged iterations only."""
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

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--image_size', type=int, default=256)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('visuals_step_cost.py: no GPU (a time taken on the host says nothing about the MI355X)')
    import bench
    args = bench.make_args(a.image_size, a.batch, 'cuda:0', 1, 0, os.environ.get('LP_PREC', 'f16'), finetune=False)
    args.set_eval_mode_in_test, args.num_visuals_per_img, args.iteration = True, 2, 0
    tm, opt_G, opt_D, holycow = bench.build(args)
    data, target = bench.synthetic_batch(args, a.batch, seed=0)

    def plain():
        holycow.train_step(tm, data, target, opt_G, opt_D, args)

    with tempfile.TemporaryDirectory() as tmp:
        args.experiment_dir = tmp

        def logged():
            plain()
            holycow.log_visuals(tm, data, target, args)

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            return times
        t_plain, t_logged = timed(plain), timed(logged)
        size = os.path.getsize(os.path.join(tmp, 'visuals', 'train_00000000.png'))
    for name, t in (('plain eager step', t_plain), ('step + log_visuals', t_logged)):
        print(f'[visuals_step_cost] {name}: median {statistics.median(t):.1f} ms, min {min(t):.1f} ... max {max(t):.1f} ms '
              f'({a.warmup} warm-up + {a.reps} timed)')
    print(f'[visuals_step_cost] a logged iteration costs {statistics.median(t_logged) - statistics.median(t_plain):.1f} ms more; '
          f'the PNG is {size / 1e3:.0f} kB')


if __name__ == '__main__':
    main()
