"""Cases of tests/test_conv_pipe_exact.py: every tile form of the tap-pipelined 3x3 kernel conv_pipe_kernel and of the chunk-pipelined 1x1 kernel
conv1x1_pipe_kernel (csrc/conv_pipe.hip) on operands for which fp32 accumulation is exact (tests/exact_operands.py).  Run as a script in a fresh
interpreter per knob setting: LP_CONV_PIPE_MR = 4 | 8 forces conv_pipe_kernel onto every eligible 3x3 shape (bf16x3 included) and runs the 3x3 cases,
LP_CONV1X1_PIPE = 2 forces conv1x1_pipe_kernel and runs the 1x1 cases.  A case is built, launched and compared by tests/conv_dma_cases.py's run_case --
planes that decode to the inputs, torch.equal against the fp64 contraction for y, the out16 planes, planes-only output and the amax slot, statistics at
2e-5 -- and this module asserts the kernel and the tile form from the launch record.  A failure names (n, y, x, channel).

Shapes are (N, H, W, Cin, Cout) with H x W the OUTPUT map, at most 2048 pixels.  conv_pipe_kernel takes Cin % 32 == 0, H >= 16, W >= 16 and Cout in 32 .. 64
(256 x 64 tiles) or >= 128.  What differs from the list first proposed:
  * the upsampled ragged case is `1x40x32 160->128`: 48 rows are whole tiles at 8 and at 16 rows per tile, 40 rows leave the 16-row tile of MR = 8 half
    empty (W = 32 keeps the columns whole, so `1x24x40` stays the case that is ragged both ways)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import exact_operands as E  # noqa: E402
import conv_dma_cases as DMA  # noqa: E402
from conv_dma_cases import C  # noqa: E402

ALL = dict(bias=1, res=1, mask=1, out16=1, y_relu=1)

CASES_3X3 = [
    C('1x16x16 32->128 one chunk', (1, 16, 16, 32, 128), bias=1, big=1),          # (the kernel loops over the chunks of REAL channels: C8 / 32)
    C('2x16x32 96->256 every option, two channel blocks', (2, 16, 32, 96, 256), stats=1, **ALL),
    C('ragged 1x24x40 64->128', (1, 24, 40, 64, 128), bias=1, mask=1, out16=0, stats=1),
    C('planes-only 1x16x32 256->128 eight chunks', (1, 16, 32, 256, 128), res=1, out16=1, want_y=0),
    C('ups 1x32x32 64->128 res_shift1', (1, 32, 32, 64, 128), ups=1, bias=1, res=1, rs=1, out16=1, stats=1),
    C('ups ragged 1x40x32 160->128', (1, 40, 32, 160, 128), ups=1, bias=1, res=1, rs=1, out16=0, stats=1),
    C('bn64 1x32x32 64->64', (1, 32, 32, 64, 64), stats=1, **ALL),
    C('bn64 2x16x16 96->48 channel tail', (2, 16, 16, 96, 48), bias=1, res=1, out16=0),
    C('bn64 ups 1x32x32 128->64', (1, 32, 32, 128, 64), ups=1, res=1, rs=1, out16=1, stats=1),
    C('dgrad 1x16x32 64->128', (1, 16, 32, 64, 128), dgrad=1, mask=1, amax=1),
]

CASES_1X1 = [
    C('1x1 1x16x16 64->128 all issued in the prologue', (1, 16, 16, 64, 128), ks=1, bias=1, stats=1),
    C('1x1 1x25x16 152->256 channel tail in the last chunk, ragged rows', (1, 25, 16, 152, 256), ks=1, bias=1, res=1, out16=0, stats=1),
    C('1x1 <4,1> 2x24x24 256->64 ring wrap-around', (2, 24, 24, 256, 64), ks=1, bias=1, mask=1, out16=1, y_relu=1),
    C('1x1 planes-only 1x64x16 320->192 ten chunks', (1, 64, 16, 320, 192), ks=1, res=1, out16=1, want_y=0, stats=1, big=1),
    C('1x1 3x8x8 96->136', (3, 8, 8, 96, 136), ks=1, bias=1, out16=0),
    C('1x1 4x2x2 64->72 the 2x2 minimum', (4, 2, 2, 64, 72), ks=1, bias=1, res=1),
]
CASES = CASES_3X3 + CASES_1X1
assert len({c['id'] for c in CASES}) == len(CASES)
assert all(c['shape'][0] * c['shape'][1] * c['shape'][2] <= 2048 for c in CASES)
assert all(c['shape'][3] % 32 == 0 and min(c['shape'][1:3]) >= 16 and (32 <= c['shape'][4] <= 64 or c['shape'][4] >= 128) for c in CASES_3X3)

PRECS = DMA.PRECS
roles = DMA.roles


def pro_of(index, case):
    return 0 if case['dgrad'] else (0, 2)[index & 1]


def cases_of(env):
    """the cases a knob setting runs: the kernel it forces"""
    if env.get('LP_CONV_PIPE_MR') in ('4', '8'):
        return CASES_3X3
    if env.get('LP_CONV1X1_PIPE') == '2':
        return CASES_1X1
    raise SystemExit('run under LP_CONV_PIPE_MR=4 | 8 or LP_CONV1X1_PIPE=2')


def check_form(case, prec, rec, env):
    n, h, w, cin, cout = case['shape']
    assert rec['what'] == 'conv' and rec['prec'] == prec and rec['ks'] == case['ks'] and rec['ups'] == case['ups'] and rec['ksplit'] == 1 and rec['finish'] == 0, rec
    th, tw, nb = 1 << rec['lth'], 1 << rec['ltw'], 1 << rec['lnb']
    if case['ks'] == 3:
        mr = int(env['LP_CONV_PIPE_MR'])
        want = dict(wm=4, wn=1, mr=4, nr=4) if cout <= 64 else dict(wm=2, wn=2, mr=mr, nr=4)
        assert rec['kernel'] == 'pipe' and rec['nbuf'] == 3 and all(rec[k] == v for k, v in want.items()), (case['id'], want, rec)
        assert tw == 16 and nb == 1 and th * 16 == rec['wm'] * rec['mr'] * 16, rec
        covered = h % th == 0 and w % 16 == 0 and cout % 4 == 0
    else:
        want = dict(wm=4, wn=1) if cout <= 64 else dict(wm=2, wn=2)
        assert rec['kernel'] == 'pipe1x1' and rec['nbuf'] == (3 if prec == E.PREC_BF16X3 else 4) and all(rec[k] == v for k, v in want.items()), (case['id'], want, rec)
        covered = nb * th * tw == rec['wm'] * 64 and th * tw >= 64 and h % th == 0 and w % tw == 0 and cout % 4 == 0
    # statistics: offered exactly on the geometries the header names (whole tiles, every wave's rows inside one image)
    assert rec['stats'] == (1 if (case['stats'] and covered) else 0), (case['id'], 'statistics', covered, rec)


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('LP_CONV')}
    log = os.environ.get('LP_FORM_LOG')
    t0 = time.time()
    bad = []
    todo = cases_of(env)
    for prec in PRECS:
        for index, case in enumerate(todo):
            for wide in roles(index, prec):
                try:
                    rec, errs, quanta = DMA.run_case(index, case, prec, wide, env, log)
                    check_form(case, prec, rec, env)
                    form = f"{rec['kernel']}<{rec['ks']},{rec['ups']},{rec['wm']},{rec['wn']},{rec['mr']},{rec['nr']}> ring={rec['nbuf']} stats={rec['stats']} " \
                           f"tile=2^({rec['lth']},{rec['ltw']},{rec['lnb']})"
                    print(f"[conv_pipe_exact {env}] prec={prec} wide={wide} {case['id']}: {form} budget=2^{np.log2(max(quanta, 1)):.1f} "
                          + ' '.join(f'{k}={v:.1e}' for k, v in errs.items()), flush=True)
                except AssertionError as e:
                    print(f"[conv_pipe_exact {env}] prec={prec} wide={wide} {case['id']}: FAILED {e}", flush=True)
                    bad.append((prec, wide, case['id'], str(e)[:400]))
    print(f'[conv_pipe_exact {env}] wall {time.time() - t0:.1f} s', flush=True)
    if bad:
        print('FAILED', bad)
        sys.exit(1)
    print('CONV_PIPE_EXACT_OK')


if __name__ == '__main__':
    main()
