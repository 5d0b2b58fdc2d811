"""Cases of tests/test_gconv_rows.py, run as a script in a fresh interpreter (LP_GCONV_ROWS=2 puts gconv_rows_kernel of csrc/gconv_rows.hip on
every shape it can express, LP_GCONV_ROWS_WGS caps its workgroups per channel block; both knobs are read once per process).

Every case runs forward (mode-0 pack) and data gradient (mode-1 pack) in the bf16x3 and fp16 modes against the fp64 grouped conv
(F.conv2d / F.conv_transpose2d with groups = C / cg) of the SAME operand planes (hi + lo in bf16x3) and the same rounded weights, so only the
accumulation order differs (K <= 144 fp32 terms): gates 2e-5 (one plane) and 3e-5 (bf16x3, which drops the lo x lo products), those of
tests/wgrad3_pipe_cases.py.  `python tests/gconv_rows_cases.py`: all cases and the epilogue checks; `... walk`: only the shape on which one
workgroup walks many tiles (also under LP_GCONV_ROWS=0, on conv_dma_kernel).  Both print `DET <prec> <sha256 of y and the statistics partials>` of that
shape: the new kernel adds every output's products tap by tap in conv_dma_kernel's order and leaves the same partials in the same row blocks, so the
digest is the same for every tile walk AND for the old route."""
import hashlib
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'latent_pose_reenactment_amd'))
from latent_pose_reenactment_amd import hipops as ops  # noqa: E402

CASES = [  # N, H, W, C, group size
    (1, 2, 2, 64, 4),              # smallest legal map, one block, every tap partly outside
    (3, 5, 7, 128, 8),             # odd sizes, ragged tiles in both directions, two blocks
    (2, 16, 16, 128, 4),           # exact tiles
    (1, 8, 24, 64, 16),            # W not a power of two
    (1, 12, 20, 192, 4),           # three blocks with CP = 256: padded weight rows
    (4, 16, 16, 256, 8),           # the statistics shape of test_conv_stats.py
]
WALK = (2, 32, 32, 128, 16)        # 32 tiles per block: with LP_GCONV_ROWS_WGS = 1 | 3 one workgroup walks 32 | 11, 11, 10 of them
GATE = {1: 3e-5, 2: 2e-5}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def dec16(t, prec):
    return t.view(torch.float16 if prec == 2 else torch.bfloat16).double().cpu()


def planes(a, prec):
    """Act16 -> the fp64 values of its operand planes [N,H,W,C] (times 1/scale of a scaled fp16 gradient operand)"""
    v = dec16(a.hi, prec)[..., :a.c]
    if prec == 1:
        v = v + dec16(a.lo, prec)[..., :a.c]
    return v if a.inv is None else v * a.inv.double().cpu()


def rounded_weights(pack, prec, c, cg):
    """the operand values of the weights, read back from the mode-0 image [9][CP][64]: w[co][j][t] = img[t][co][cg * ((co % 64) / cg) + j]"""
    img = dec16(pack.hi, prec)
    if prec == 1:
        img = img + dec16(pack.lo, prec)
    co = torch.arange(c)
    cols = (((co % 64) // cg) * cg)[:, None] + torch.arange(cg)[None, :]
    return img[:, co[:, None], cols].permute(1, 2, 0).reshape(c, cg, 3, 3).contiguous()


def inputs(case, prec):
    n, h, w, c, cg = case
    g = torch.Generator().manual_seed(sum(case) + prec)
    x = torch.randn(n, h, w, c, generator=g).cuda()
    dy = torch.randn(n, h, w, c, generator=g).cuda()
    wt = (torch.randn(c, cg, 3, 3, generator=g) / (cg * 9) ** 0.5).cuda()
    return x, dy, wt


def ref_fwd(a64, w64, cg):
    return F.conv2d(a64.permute(0, 3, 1, 2), w64, None, 1, 1, 1, w64.shape[0] // cg).permute(0, 2, 3, 1)


def ref_dgrad(d64, w64, cg):
    return F.conv_transpose2d(d64.permute(0, 3, 1, 2), w64, None, 1, 1, 0, w64.shape[0] // cg).permute(0, 2, 3, 1)


def run_case(case, prec):
    n, h, w, c, cg = case
    x, dy, wt = inputs(case, prec)
    a, d = ops.act_pack(x, pro=0, prec=prec), ops.act_pack(dy, pro=0, prec=prec)
    pk0, pk1 = ops.pack_grouped(wt, 0, prec), ops.pack_grouped(wt, 1, prec)
    y, dx = ops.gconv16(a, pk0, prec=prec), ops.gconv16(d, pk1, prec=prec)
    torch.cuda.synchronize()
    w64 = rounded_weights(pk0, prec, c, cg)
    return {'fwd': rel(y, ref_fwd(planes(a, prec), w64, cg)), 'dgrad': rel(dx, ref_dgrad(planes(d, prec), w64, cg))}


def digest(*tensors):
    m = hashlib.sha256()
    for t in tensors:
        m.update(t.detach().cpu().contiguous().numpy().tobytes())
    return m.hexdigest()


def run_epilogue_checks(case, bad):
    """statistics partials, the 16-bit-resident output, the bf16x3 output planes, a scaled fp16 gradient operand, amax"""
    n, h, w, c, cg = case
    gam, bet = torch.ones(c).cuda(), torch.zeros(c).cuda()

    def check(name, value, gate):
        print(f'[gconv_rows] {case} {name}: {value:.2e} (gate {gate:.0e})', flush=True)
        if not value < gate:
            bad.append((case, name, value))

    def must(name, cond):
        print(f'[gconv_rows] {case} {name}: {"ok" if cond else "FAILED"}', flush=True)
        if not cond:
            bad.append((case, name))
    for prec in (1, 2):
        x, dy, wt = inputs(case, prec)
        a = ops.act_pack(x, pro=0, prec=prec)
        pk0 = ops.pack_grouped(wt, 0, prec)
        y, cs = ops.gconv16(a, pk0, prec=prec, stats=True)
        must(f'prec{prec} statistics rows == H W / 64', cs is not None and cs.rows == h * w // 64 and cs.images == n)
        if cs is not None:
            got = ops.norm_stats_finalize(cs, 1, c, gam, bet, 1e-5)
            want = ops.bn_train_stats(y, gam, bet, None, None, 0.1, 1e-5)
            for nm, g_, w_ in zip(('mean', 'rstd'), got, want):
                check(f'prec{prec} merged statistics {nm} vs bn_train_stats of y', rel(g_, w_), 5e-6)
        if prec == 2:
            none, y16, cs16 = ops.gconv16(a, pk0, prec=2, stats=True, want_y=False, out16=True)
            must('fp16 plane bit-equal to y.half()', none is None and torch.equal(y16.hi.view(torch.float16), y.half()))
            k = h * w // 64 * n * c * 3
            must('partials bit-equal with and without fp32 y', cs is not None and cs16 is not None and torch.equal(cs16.part[:k], cs.part[:k]))
            d16 = ops.act_pack(dy * 1e-3, prec=2, grad=True)                  # scaled by a power of two from its amax; 1/scale = alpha2
            must('the gradient operand is scaled', d16.inv is not None and float(d16.inv) != 1.0)
            dx = ops.gconv16(d16, ops.pack_grouped(wt, 1, 2), prec=2)
            check('scaled fp16 gradient operand (alpha2)', rel(dx, ref_dgrad(planes(d16, 2), rounded_weights(pk0, 2, c, cg), cg)), GATE[2])
            ya = ops.gconv16(a, pk0, prec=2, amax=True)
            rec = getattr(ya, '_lp_amax', None)
            must('amax slots attached', rec is not None)
            if rec is not None:
                m, t = float(rec[0].max()), float(ya.abs().max())
                check('amax slot maximum vs max|y|', abs(m - t) / t, 1e-6)
        else:
            y2, o16 = ops.gconv16(a, pk0, prec=1, out16=True)
            must('y independent of the plane output', torch.equal(y2, y))
            check('bf16x3 output planes decode to y', rel(planes(o16, 1), y), 3e-6)


def run_walk(bad):
    for prec in (1, 2):
        errs = run_case(WALK, prec)
        print(f'[gconv_rows wgs={os.environ.get("LP_GCONV_ROWS_WGS")}] prec={prec} {WALK}: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()), flush=True)
        bad += [(prec, WALK, k, v) for k, v in errs.items() if not v < GATE[prec]]
        x, _, wt = inputs(WALK, prec)
        a, pk0 = ops.act_pack(x, pro=0, prec=prec), ops.pack_grouped(wt, 0, prec)
        hs = []
        for _ in range(2):
            y, cs = ops.gconv16(a, pk0, prec=prec, stats=True)
            k = WALK[1] * WALK[2] // 64 * WALK[0] * WALK[3] * 3
            hs.append(digest(y, cs.part[:k]) if cs is not None else 'no statistics')
        if hs[0] != hs[1] or cs is None:
            bad.append((prec, WALK, 'two launches differ', hs))
        print(f'DET {prec} {hs[0]}', flush=True)
    # Which kernel ran?  Its results cannot tell (they are conv_dma_kernel's bit for bit); the amax slots can: a wave commits its maximum to slot
    # (workgroup id [+ 7 x block row] + wave) & 63, so gconv_rows_kernel capped to ONE workgroup per channel block (2 blocks, 4 waves) touches at
    # most 5 slots, conv_dma_kernel's grid of 8 tiles x 2 blocks more than that
    ya = ops.gconv16(a, pk0, prec=2, amax=True)
    torch.cuda.synchronize()
    nz = int((ya._lp_amax[0] != 0).sum())
    print(f'SLOTS {nz}', flush=True)
    if os.environ.get('LP_GCONV_ROWS') == '2' and os.environ.get('LP_GCONV_ROWS_WGS') == '1' and not 1 <= nz <= 5:
        bad.append(('gconv_rows_kernel did not run with one workgroup per block: amax slots', nz))
    if os.environ.get('LP_GCONV_ROWS') == '0' and not nz > 5:
        bad.append(('the old route touches no more amax slots than the capped new kernel: the signal is void', nz))


def main():
    bad = []
    walk_only = 'walk' in sys.argv[1:]
    assert os.environ.get('LP_GCONV_ROWS') == '2' or (walk_only and os.environ.get('LP_GCONV_ROWS') == '0'), 'run with LP_GCONV_ROWS=2 (walk: or 0, the old route)'
    if not walk_only:
        for prec in (1, 2):
            for case in CASES:
                errs = run_case(case, prec)
                print(f'[gconv_rows] prec={prec} {case}: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()), flush=True)
                bad += [(prec, case, k, v) for k, v in errs.items() if not v < GATE[prec]]
        for case in (CASES[5], WALK):
            run_epilogue_checks(case, bad)
        errs = run_case(CASES[2], 0)          # plain bf16: the third instantiation (one plane: the fp16 gate)
        print(f'[gconv_rows] prec=0 {CASES[2]}: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()), flush=True)
        bad += [(0, CASES[2], k, v) for k, v in errs.items() if not v < GATE[2]]
    run_walk(bad)
    if bad:
        print('FAILED', bad)
        sys.exit(1)
    print('GCONV_ROWS_OK')


if __name__ == '__main__':
    main()
