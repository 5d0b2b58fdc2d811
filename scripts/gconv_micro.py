"""Per-launch time of the grouped 3x3 convs of the identity encoder (ResNeXt conv2 at 64 frames: the five shapes of the meta-training step),
forward (mode-0 pack) and data gradient (mode-1 pack), on conv_dma_kernel (LP_GCONV_ROWS=0) and on gconv_rows_kernel (the default dispatch).
The knob is read once per process, so every measurement runs in a child interpreter of its own and the two routes ALTERNATE (ROUNDS times
each).  Prints us per launch (torch events over REPS launches), algorithmic bytes / time and its share of the 8 TB/s HBM peak -- the bound of
these layers is their bytes: operand planes read once (2 B per element and plane) + fp32 y written once (4 B).  The launches rotate over
enough copies of the operand planes (COLD_MB, default 1024 MB per shape) that no launch finds its input in the 256 MB last-level cache, as in
the training step, where other kernels run between two launches of a layer; COLD_MB=0 re-reads one copy (the cache-resident figure).  The
statistics partials of the forward launches are on, as in the step.

    PREC=1 python scripts/gconv_micro.py        (PREC: 1 bf16x3 | 2 fp16;  REPS, ROUNDS, COLD_MB)"""
import os
import subprocess
import sys

SHAPES = [(64, 64, 64, 128, 4), (64, 64, 64, 256, 8), (64, 32, 32, 256, 8), (64, 32, 32, 512, 16), (64, 16, 16, 512, 16)]      # N, H, W, C, group size
PEAK = 8.0e12


def child():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from latent_pose_reenactment_amd import hipops as ops
    prec, reps = int(os.environ.get('PREC', '1')), int(os.environ.get('REPS', '20'))

    def timeit(f):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3
    for (n, h, w, c, cg) in SHAPES:
        x = torch.randn(n, h, w, c, device='cuda')
        wt = torch.randn(c, cg, 3, 3, device='cuda') / (cg * 9) ** 0.5
        nbytes = n * h * w * c * ((4 if prec == 1 else 2) + 4)
        copies = max(1, -(-int(os.environ.get('COLD_MB', '1024')) * (1 << 20) // (nbytes - n * h * w * c * 4)))
        a = [ops.act_pack(x, pro=2, prec=prec) for _ in range(copies)]
        dy = torch.randn(n, h, w, c, device='cuda') * 1e-3
        d = [ops.act_pack(dy, prec=prec, grad=True) for _ in range(copies)]
        for name, acts, mode in (('fwd', a, 0), ('dgrad', d, 1)):
            pk = ops.pack_grouped(wt, mode, prec)
            turn = [0]

            def launch():
                turn[0] = (turn[0] + 1) % copies
                return ops.gconv16(acts[turn[0]], pk, prec=prec, stats=(mode == 0))
            us = timeit(launch)
            print(f'LP_GCONV_ROWS={os.environ.get("LP_GCONV_ROWS", "default")} copies={copies} prec={prec} {str((n, h, w, c, cg)):24s} {name:5s} {us:7.1f} us  '
                  f'{nbytes / us / 1e6:5.2f} TB/s algorithmic  {100 * nbytes / us / 1e-6 / PEAK:4.1f} % of the 8 TB/s peak (bound: bytes)', flush=True)


if __name__ == '__main__':
    if '--child' in sys.argv:
        child()
        sys.exit(0)
    for rnd in range(int(os.environ.get('ROUNDS', '2'))):
        for route in ('0', None):
            env = dict(os.environ)
            env.pop('LP_GCONV_ROWS', None)
            if route is not None:
                env['LP_GCONV_ROWS'] = route
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, timeout=300)
            if r.returncode != 0:                      # nothing more is started after a failed child
                sys.exit(r.returncode)
