"""Cases of tests/test_wgrad_exact.py: every dispatch form of the generic weight-gradient kernel conv_wgrad_kernel<KS, UPS, PREC, COB>
(csrc/conv_wgrad.hip) and of the three reductions behind it (wgrad_reduce_kernel, wgrad_reduce_flat_kernel<32> / <256>), with the bias gradient,
its accumulation into a non-zero tensor and the fp16 out_scale, on operands for which fp32 accumulation is exact (tests/exact_operands.py): dw
and db must equal the fp64 sums bit for bit.  The budget sum_pixels |dy| |a| <= 2^22 quanta is asserted on the CPU before anything is launched.
Run as a script in a fresh interpreter per knob setting; every case asserts the form its id names from the launch record (lp_last_launch_form).
The 1x1 shapes run twice: with a bias gradient they keep conv_wgrad_kernel, without one they must record wgrad1x1_kernel (exact as well).
The spectral-norm dot of the reductions is a sum that is not exact; it stays with tests/test_spectral_norm_gpu.py.
Shapes are (N, H, W, Cin, Cout), H x W the map of dy."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import exact_operands as E  # noqa: E402


def C(cid, shape, ks=3, ups=0, **opt):
    d = dict(id=cid, shape=shape, ks=ks, ups=ups, kernel='generic', cob=None, red=None, splits=None, bias=0, accum=0)
    assert set(opt) <= set(d), set(opt) - set(d)
    d.update(opt)
    return d


# ``kernel`` / ``cob`` / ``red``: what the launch record must show under the default knobs; ``splits``: the count passed (None: default_splits)
CASES = [
    # kernel forms
    C('cob128 8x4x4 64->128', (8, 4, 4, 64, 128), cob=128, bias=1),
    C('cob128 ups 2x8x8 64->128', (2, 8, 8, 64, 128), ups=1, cob=128),
    C('cob64 2x8x8 64->64', (2, 8, 8, 64, 64), cob=64, bias=1, accum=1),
    C('cob64 ups 2x16x16 128->64', (2, 16, 16, 128, 64), ups=1, cob=64, bias=1),
    C('cob64 channel tails 2x12x10 72->40', (2, 12, 10, 72, 40), cob=64, bias=1),
    C('1x1 bias cob128 2x16x16 64->128', (2, 16, 16, 64, 128), ks=1, cob=128, bias=1),
    C('1x1 bias cob64 3x9x8 72->40', (3, 9, 8, 72, 40), ks=1, cob=64, bias=1, accum=1),
    C('1x1 no bias 2x16x16 64->128', (2, 16, 16, 64, 128), ks=1, kernel='1x1'),
    C('1x1 no bias 3x9x8 72->40', (3, 9, 8, 72, 40), ks=1, kernel='1x1'),
    # tile edges
    C('tile 1x4x4 64->64 eight image slots, one image', (1, 4, 4, 64, 64), cob=64, bias=1),
    C('tile 3x5x7 64->64', (3, 5, 7, 64, 64), cob=64, bias=1),
    C('tile 2x2x4 64->64', (2, 2, 4, 64, 64), cob=64),
]
# the reductions, each with 1 split, an uneven explicit count and more splits than tiles (6 tiles of 128 pixels)
for _name, _cin, _cout, _ks, _red in (('flat32 64->64', 64, 64, 3, 'flat32'), ('flat256 128->128', 128, 128, 3, 'flat256'),
                                      ('tiled 64->512', 64, 512, 3, 'tiled'), ('tiled 1x1 bias 256->256', 256, 256, 1, 'tiled')):
    for _s in (1, 5, 64):
        CASES.append(C(f'red {_name} splits {_s}', (6, 8, 16, _cin, _cout), ks=_ks, red=_red, splits=_s, bias=1, accum=int(_s == 5),
                       cob=128 if _cout >= 128 else 64))
assert len({c['id'] for c in CASES}) == len(CASES)
assert all(c['shape'][0] * c['shape'][1] * c['shape'][2] <= 2048 for c in CASES)

PRECS = (E.PREC_F16, E.PREC_BF16X3, E.PREC_BF16)


def roles(index, prec):
    return ('a', 'w') if prec == E.PREC_BF16X3 else (('a', 'w')[index & 1],)


def hash_id(s):
    v = 0
    for ch in s.encode():
        v = (v * 131 + ch) & 0x7FFFFFFF
    return v


def build(case, prec, wide, pro=0):
    """CPU side: a (the conv's activated input, NCHW), dy (NCHW), the non-zero bias accumulator; budget asserted; fp64 references dw, db"""
    n, h, w, cin, cout = case['shape']
    ks, ups = case['ks'], case['ups']
    hin, win = (h // 2, w // 2) if ups else (h, w)
    seed = (hash_id(case['id']) + 7 * prec + (1 if wide == 'w' else 0)) & 0x7FFFFFFF
    g = torch.Generator().manual_seed(seed ^ 0x5EED)
    acc0 = E.draw_ints(g, (cout,), 1023).float() * E.QW if case['accum'] else None

    def bound(a_terms, d_terms):
        q1 = E.assert_budget(E.wgrad64([E.abs_sum(a_terms)], [E.abs_sum(d_terms)], ks, bool(ups)), E.QA * E.QW, case['id'] + ' dw')
        db = E.abs_sum(d_terms).sum((0, 2, 3))
        if acc0 is not None:
            db = db + acc0.double().abs()
        return max(q1, E.assert_budget(db, E.QW, case['id'] + ' db'))
    x_in, dy = E.draw_pair(seed, (n, cin, hin, win), (n, cout, h, w), prec, wide, bound)
    a = torch.relu(x_in) if pro == 2 else x_in
    a_terms, d_terms = E.terms(a, prec), E.terms(dy, prec)
    quanta = bound(a_terms, d_terms)
    dw = E.wgrad64(a_terms, d_terms, ks, bool(ups))
    db = dy.double().sum((0, 2, 3))
    if acc0 is not None:
        db = db + acc0.double()
    assert torch.equal(dw.float().double(), dw) and torch.equal(db.float().double(), db)
    return dict(x=x_in, a_terms=a_terms, dy=dy, d_terms=d_terms, acc0=acc0, dw=dw, db=db, quanta=quanta)


def check_form(case, prec, rec, env, splits_in):
    assert rec['what'] == 'wgrad' and rec['prec'] == prec and rec['ks'] == case['ks'] and rec['ups'] == case['ups'], rec
    assert rec['bias'] == case['bias'], rec
    knobs = {k: v for k, v in env.items() if k.startswith('LP_WGRAD')}
    assert rec['kernel'] == case['kernel'], (case['id'], rec)          # (no shape here is in wgrad3_pipe_kernel's range, under any of the knob settings)
    assert rec['red'] in ('tiled', 'flat32', 'flat256') and (case['red'] is None or rec['red'] == case['red']), (case['id'], rec)
    if rec['kernel'] == 'generic':
        cob = case['cob']
        if knobs.get('LP_WGRAD_COB') == '64' and case['ks'] == 3:          # (the knob is the 3x3 kernel's: lp_knobs.h)
            cob = 64
        assert rec['cob'] == cob, (case['id'], rec)
        assert rec['splits'] == min(splits_in, rec['tiles']), (case['id'], rec, splits_in)
        n, h, w = case['shape'][:3]
        th, tw, nb = 1 << rec['lth'], 1 << rec['ltw'], 1 << rec['lnb']
        assert th * tw * nb == 128 and rec['tiles'] == ((h + th - 1) // th) * ((w + tw - 1) // tw) * ((n + nb - 1) // nb), rec
    else:
        assert 1 <= rec['splits'] <= splits_in, rec


def run_case(index, case, prec, wide, env, log):
    from latent_pose_reenactment_amd import hipops as ops
    from conv_pipe_cases import planes64
    n, h, w, cin, cout = case['shape']
    ks, ups = case['ks'], case['ups']
    pro = (0, 2)[index & 1]
    b = build(case, prec, wide, pro)
    dev = 'cuda'
    a = ops.act_pack(b['x'].permute(0, 2, 3, 1).contiguous().to(dev), pro=pro, prec=prec)
    dy = ops.act_pack(b['dy'].permute(0, 2, 3, 1).contiguous().to(dev), pro=0, prec=prec, grad=True)
    inv = dy.inv.double().cpu().item() if dy.inv is not None else 1.0
    assert (dy.inv is not None) == (prec == E.PREC_F16)
    for nm, got, want in (('a', [t.cpu() for t in planes64(a.hi, a.lo, prec, cin)], b['a_terms']),
                          ('dy', [t.cpu() * inv for t in planes64(dy.hi, dy.lo, prec, cout)], b['d_terms'])):
        for gt, wt in zip(got, want):
            assert torch.equal(gt, wt), f'{nm} planes do not decode to the input: ' + E.first_mismatch(gt, wt, 'ncyx')
    splits = case['splits'] if case['splits'] is not None else ops.default_splits(n, h, w, cin, cout, ks, prec, bool(case['bias']))
    acc = b['acc0'].clone().to(dev) if b['acc0'] is not None else None
    out = ops.conv_wgrad16(a, dy, ksize=ks, upsample=bool(ups), prec=prec, splits=splits, bias_grad=bool(case['bias']), bias_accum=acc)
    rec = ops.last_launch_form()
    torch.cuda.synchronize()
    if log:
        with open(log, 'a') as f:
            f.write(json.dumps(dict(case=case['id'], prec=prec, wide=wide, env=env, rec=rec)) + '\n')
    check_form(case, prec, rec, env, splits)
    tag = f"{case['id']} prec={prec} wide={wide}"
    dw, db = out if case['bias'] else (out, None)
    gw = dw.cpu().double()
    assert torch.equal(gw, b['dw']), f'{tag}: dw: ' + E.first_mismatch(gw, b['dw'], ('co', 'ci', 'ky', 'kx'))
    if case['bias']:
        gb = (acc if acc is not None else db).cpu().double()
        assert (db is None) == (acc is not None)
        assert torch.equal(gb, b['db']), f'{tag}: db: ' + E.first_mismatch(gb, b['db'], ('co',))
    return rec, b['quanta']


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('LP_CONV') or k.startswith('LP_WGRAD')}
    log = os.environ.get('LP_FORM_LOG')
    t0 = time.time()
    bad = []
    for prec in PRECS:
        for index, case in enumerate(CASES):
            for wide in roles(index, prec):
                try:
                    rec, quanta = run_case(index, case, prec, wide, env, log)
                    print(f"[wgrad_exact {env}] prec={prec} wide={wide} {case['id']}: {rec['kernel']}<{rec['ks']},{rec['ups']},cob {rec['cob']}> "
                          f"splits={rec['splits']} tiles={rec['tiles']} red={rec['red']} bias={rec['bias']} budget=2^{np.log2(max(quanta, 1)):.1f}", flush=True)
                except AssertionError as e:
                    print(f"[wgrad_exact {env}] prec={prec} wide={wide} {case['id']}: FAILED {e}", flush=True)
                    bad.append((prec, wide, case['id'], str(e)[:400]))
    print(f'[wgrad_exact {env}] wall {time.time() - t0:.1f} s', flush=True)
    if bad:
        print('FAILED', bad)
        sys.exit(1)
    print('WGRAD_EXACT_OK')


if __name__ == '__main__':
    main()
