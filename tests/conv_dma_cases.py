"""Cases of tests/test_conv_dma_exact.py: every dispatch form of the dense convolution kernel conv_dma_kernel (csrc/conv_dma.hip) and of its split-K
finish splitk_reduce_kernel, on operands for which fp32 accumulation is exact (tests/exact_operands.py).  Run as a script in a fresh interpreter per
knob setting (the knob table is read once per process).  Every case builds its planes with act_pack / pack_weights, asserts that they decode to the
inputs, calls conv16, reads the launch record (lp_last_launch_form), asserts the form its id names, and then asserts torch.equal against the fp64
contraction -- y, the out16 planes (against the bit-level packer of tests/operand_restatement.py applied to the exact y), planes-only output and
the amax slot.  A failure names (n, y, x, channel).  Norm statistics (not exact) keep tests/conv_pipe_cases.py's 2e-5.

All launches are at most 2048 output pixels.  Shapes are (N, H, W, Cin, Cout) with H x W the OUTPUT map.  Shapes that differ from the ones first proposed
for their form, because the launch record showed that those miss it:
  * ragged <2,2,4,4>: (3,20,20,64,72) -- a 20 x 12 map has <= 256 pixels and goes to the 8-wave form;
  * 1x1 (1,16,16,544,64): pack_weights pads the contraction to a multiple of 64 (576), so the 64-channel chunks apply; the 32-channel fall-back of
    dispatch_conv16 (CinP % 64 != 0 with Cin >= 512) cannot be reached through the packer.  The case stays: its last chunk is half padding;
  * 8-wave 1x1: dispatch_conv16 has one 8-wave 1x1 form, <2,4,4,2>, in every precision mode (the <2,2,4,2> substitute is a 3x3 form)."""
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
import operand_restatement as R  # noqa: E402


def C(cid, shape, ks=3, ups=0, form=None, x3=None, **opt):
    d = dict(id=cid, shape=shape, ks=ks, ups=ups, form=form or {}, x3=x3, bias=0, res=0, rs=0, mask=0, out16=None, y_relu=0, want_y=1, stats=0, amax=0,
             dgrad=0, big=0, both_wide=0, pp1=0, nbuf3=0, ksplit=None)
    assert set(opt) <= set(d), set(opt) - set(d)
    d.update(opt)
    return d


ALL = dict(bias=1, res=1, mask=1, out16=1, y_relu=1)                  # every epilogue option of the split-K finish at once
W8 = dict(wm=2, wn=4, mr=4, nr=2)                                     # the 8-wave tiling ...
W8X3 = dict(wm=2, wn=2, mr=4, nr=2)                                   # ... and its bf16x3 substitute (3x3)
T4114, T4144, T2244 = dict(wm=4, wn=1, mr=4, nr=1), dict(wm=4, wn=1, mr=4, nr=4), dict(wm=2, wn=2, mr=4, nr=4)

# ``form``: what the launch record must show under the DEFAULT knobs (``x3``: the bf16x3 override); ``ksplit``: the split factor under the default knobs
CASES = [
    # split-K 3x3 with every option of splitk_reduce_kernel
    C('splitk2 8x4x4 128->64', (8, 4, 4, 128, 64), form=T2244, ksplit=2, stats=1, **ALL),
    C('splitk4 2x4x4 256->128 w8', (2, 4, 4, 256, 128), form=W8, x3=W8X3, ksplit=4, **ALL),
    C('splitk8 1x4x4 512->128 w8', (1, 4, 4, 512, 128), form=W8, x3=W8X3, ksplit=8, big=1, **ALL),
    C('splitk6 2x4x4 576->128 w8 (18 chunks: fixed-point shrink)', (2, 4, 4, 576, 128), form=W8, x3=W8X3, ksplit=6, **ALL),
    # split-K upsampled with the low-resolution residual
    C('splitk4 ups 2x8x8 256->192 res_shift1', (2, 8, 8, 256, 192), ups=1, form=W8, x3=W8X3, ksplit=4, bias=1, res=1, rs=1, out16=0),
    C('splitk4 ups 2x8x8 256->192 res_shift1 planes-only', (2, 8, 8, 256, 192), ups=1, form=W8, x3=W8X3, ksplit=4, res=1, rs=1, out16=0, want_y=0),
    # 8-wave forms
    C('w8 3x3 3x8x16 64->128', (3, 8, 16, 64, 128), form=W8, x3=W8X3, ksplit=1, bias=1, stats=1, out16=1),
    C('w8 3x3 ups 1x16x16 128->136', (1, 16, 16, 128, 136), ups=1, form=W8, x3=W8X3, res=1, rs=1, mask=1),
    C('w8 1x1 3x8x8 96->136', (3, 8, 8, 96, 136), ks=1, form=W8, ksplit=1, bias=1, out16=0),
    # narrow forms
    C('<4,1,4,1> 1x16x16 32->8', (1, 16, 16, 32, 8), form=T4114, ksplit=1, bias=1, out16=1),
    C('<4,1,4,1> 1x32x32 16->12 planes by the pack pass', (1, 32, 32, 16, 12), form=T4114, ksplit=1, res=1, out16=1, big=1),
    C('<4,1,4,1> 2x16x16 64->6 element-wise epilogue', (2, 16, 16, 64, 6), form=T4114, ksplit=1, bias=1, res=1, mask=1, y_relu=1),
    C('<4,1,4,1> 2x16x16 128->6 must not split', (2, 16, 16, 128, 6), form=T4114, ksplit=1, bias=1, out16=0),
    C('<4,1,4,4> 1x16x16 64->24', (1, 16, 16, 64, 24), form=T4144, ksplit=1, bias=1, mask=1, out16=1, stats=1),
    C('<4,1,4,4> ups 2x32x32 64->40', (2, 32, 32, 64, 40), ups=1, form=T4144, ksplit=1, res=1, rs=1, out16=0, stats=1),
    # 4-wave <2,2,4,4> outside the tap-pipelined kernel's range
    C('<2,2,4,4> 1x32x32 64->96', (1, 32, 32, 64, 96), form=T2244, bias=1, res=1, out16=1, stats=1, nbuf3=1),
    C('<2,2,4,4> ragged 3x20x20 64->72', (3, 20, 20, 64, 72), form=T2244, bias=1, mask=1, out16=0, stats=1),
    # 1x1: 64-channel chunks in the single-plane modes, 32 in bf16x3
    C('1x1 cc64 <4,1,4,4> 1x16x16 512->64', (1, 16, 16, 512, 64), ks=1, form=dict(T4144, cc=64), x3=dict(T4144, cc=32), bias=1, out16=1, stats=1),
    C('1x1 cc64 <2,2,4,4> 1x32x16 512->72', (1, 32, 16, 512, 72), ks=1, form=dict(T2244, cc=64), x3=dict(T2244, cc=32), res=1, mask=1, big=1),
    C('1x1 cc64 1x16x16 544->64 half-padded last chunk', (1, 16, 16, 544, 64), ks=1, form=dict(T4144, cc=64), x3=dict(T4144, cc=32), bias=1, out16=0),
    C('1x1 x3 single buffer 2x16x16 256->64', (2, 16, 16, 256, 64), ks=1, form=dict(T4144, cc=32, a_dbuf=1), x3=dict(T4144, cc=32, a_dbuf=0), bias=1, out16=1),
    C('1x1 x3 double buffer 2x16x16 288->64', (2, 16, 16, 288, 64), ks=1, form=dict(T4144, cc=32, a_dbuf=1), res=1, out16=0, want_y=0),
    C('1x1 both operands wide 1x4x4 8->72', (1, 4, 4, 8, 72), ks=1, both_wide=1, bias=1),
    # tile geometry edges
    C('tile 32x2x2 64->64 many images per tile', (32, 2, 2, 64, 64), form=T2244, bias=1, res=1, out16=1),
    C('tile 5x3x5 64->64', (5, 3, 5, 64, 64), form=T2244, bias=1, mask=1, out16=0),
    C('tile 1x2x16 64->128', (1, 2, 16, 64, 128), res=1, y_relu=1),
    C('tile 3x4x4 64->64 N below the images per tile', (3, 4, 4, 64, 64), form=T2244, bias=1),
    C('tile 2x8x8 64->128 plain', (2, 8, 8, 64, 128), form=W8, x3=W8X3),
    # ping-pong with an odd tile count (LP_CONV_PP=1: two tiles per workgroup, the second group of the last workgroup masked)
    C('pp 3x8x16 64->64 three tiles', (3, 8, 16, 64, 64), form=T2244, ksplit=1, bias=1, res=1, out16=1, stats=1, pp1=1),
    # data gradient: mode-1 pack, gradient operand (fp16: power-of-two scale and alpha2), ReLU mask, amax
    C('dgrad splitk2 8x4x4 128->256 w8', (8, 4, 4, 128, 256), form=W8, x3=W8X3, ksplit=2, dgrad=1, mask=1, amax=1),
    C('dgrad <4,1,4,1> 2x16x16 64->4', (2, 16, 16, 64, 4), form=T4114, ksplit=1, dgrad=1, mask=1, amax=1),
]
assert len({c['id'] for c in CASES}) == len(CASES)
assert all(c['shape'][0] * c['shape'][1] * c['shape'][2] <= 2048 for c in CASES)

PRECS = (E.PREC_F16, E.PREC_BF16X3, E.PREC_BF16)


def roles(index, prec):
    """which operand is wide: bf16x3 runs both (so that hi*lo and lo*hi are both live), the single-plane modes alternate by case"""
    return ('a', 'w') if prec == E.PREC_BF16X3 else (('a', 'w')[index & 1],)


def build(case, prec, wide, pro=0):
    """CPU side of a case: the fp32 inputs (integers times a power of two), the asserted budget, the exact fp64 reference y (NCHW) -> dict"""
    n, h, w, cin, cout = case['shape']
    ks, ups = case['ks'], case['ups']
    hin, win = (h // 2, w // 2) if ups else (h, w)
    seed = (hash_id(case['id']) + 7 * prec + (1 if wide == 'w' else 0)) & 0x7FFFFFFF
    g = torch.Generator().manual_seed(seed ^ 0x5EED)
    q = E.ALPHA * E.QA * E.QW
    bias = E.draw_ints(g, (cout,), 1023).float() * q if case['bias'] else None
    rs = case['rs']
    res = E.draw_ints(g, (n, h >> rs, w >> rs, cout), 1023).float() * q if case['res'] else None
    res_full = None
    if res is not None:
        res_full = res.permute(0, 3, 1, 2)
        if rs:
            res_full = E.up2(res_full)
    mask_src = torch.randn((n, h, w, cout), generator=g) if case['mask'] else None

    def bound(a_terms, w_terms):
        return E.assert_budget(E.conv_bound(a_terms, w_terms, bool(ups), E.ALPHA, bias, res_full), q, case['id'])
    x_in, wt = E.draw_pair(seed, (n, cin, hin, win), (cout, cin, ks, ks), prec, wide, bound, big=bool(case['big']), both_wide=bool(case['both_wide']))
    a = torch.relu(x_in) if pro == 2 else x_in      # the pack's prologue: the operand is relu of the drawn input (the bound only shrinks)
    a_terms, w_terms = E.terms(a, prec), E.terms(wt, prec)
    quanta = bound(a_terms, w_terms)
    ref = E.ALPHA * E.conv64(a_terms, w_terms, bool(ups))
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
    if res_full is not None:
        ref = ref + res_full.double()
    if mask_src is not None:
        ref = torch.where(mask_src.permute(0, 3, 1, 2) > 0, ref, torch.zeros_like(ref))
    if case['y_relu']:
        ref = torch.relu(ref)
    assert torch.equal(ref.float().double(), ref), 'the reference itself is not an fp32 value'
    return dict(x=x_in, a=a, w=wt, a_terms=a_terms, w_terms=w_terms, bias=bias, res=res, mask_src=mask_src, ref=ref, quanta=quanta)


def hash_id(s):
    v = 0
    for ch in s.encode():
        v = (v * 131 + ch) & 0x7FFFFFFF
    return v


def expected_form(case, prec):
    f = dict(case['form'])
    if prec == E.PREC_BF16X3 and case['x3'] is not None:
        f = dict(case['x3'])
    return f


def check_form(case, prec, rec, env):
    """the record against what the case's id names (default knobs) and against what each knob promises"""
    n, h, w, cin, cout = case['shape']
    assert rec['what'] == 'conv' and rec['prec'] == prec, rec
    assert rec['ks'] == case['ks'] and rec['ups'] == case['ups'], rec
    knobs = {k: v for k, v in env.items() if k.startswith('LP_CONV')}
    if not knobs:
        assert rec['kernel'] == 'dma', rec
        for k, v in expected_form(case, prec).items():
            assert rec[k] == v, (case['id'], k, v, rec)
        if case['ksplit'] is not None:
            assert rec['ksplit'] == case['ksplit'], (case['id'], rec)
    if rec['kernel'] != 'dma':
        return
    if knobs.get('LP_CONV_KSPLIT') == '1':
        assert rec['ksplit'] == 1, rec
    if (cout & 3) or case['ks'] == 1:
        assert rec['ksplit'] == 1, rec
    assert rec['finish'] == (1 if rec['ksplit'] > 1 else 0), rec
    if knobs.get('LP_CONV_W8') == '0':
        assert rec['wm'] * rec['wn'] == 4, rec
    if knobs.get('LP_CONV_W8') == '1' and cout > 64:
        want = W8X3 if (prec == E.PREC_BF16X3 and case['ks'] == 3) else W8
        assert all(rec[k] == v for k, v in want.items()), rec
    if knobs.get('LP_CONV_PP') == '0':
        assert rec['pp'] == 0, rec
    if knobs.get('LP_CONV_PP') == '1' and case['pp1']:
        tiles = tile_count(case, rec)
        assert rec['pp'] == 1 and tiles % 2 == 1 and rec['tiles'] == (tiles + 1) // 2, (rec, tiles)
    if knobs.get('LP_CONV_NBUF') == '2':
        assert rec['nbuf'] == 2, rec
    if knobs.get('LP_CONV_NBUF') == '3' and case['nbuf3'] and prec != E.PREC_BF16X3:      # (bf16x3: three hi + lo weight stages of this tile exceed the LDS)
        assert rec['nbuf'] == 3 and rec['pp'] == 0, rec


def tile_count(case, rec):
    n, h, w = case['shape'][:3]
    th, tw, nb = 1 << rec['lth'], 1 << rec['ltw'], 1 << rec['lnb']
    return ((h + th - 1) // th) * ((w + tw - 1) // tw) * ((n + nb - 1) // nb)


def words(t):
    """int16 plane tensor -> numpy uint16 [N][HW][C8] with -0 folded onto +0"""
    a = t.cpu().numpy().view(np.uint16).reshape(t.shape[0], -1, t.shape[-1]).copy()
    a[a == 0x8000] = 0
    return a


def run_case(index, case, prec, wide, env, log):
    from latent_pose_reenactment_amd import hipops as ops
    n, h, w, cin, cout = case['shape']
    ks, ups = case['ks'], case['ups']
    pro = 0 if case['dgrad'] else (0, 2)[index & 1]
    b = build(case, prec, wide, pro)
    dev = 'cuda'
    x = b['x'].permute(0, 2, 3, 1).contiguous().to(dev)
    alpha = torch.tensor([E.ALPHA], device=dev)
    if case['dgrad']:
        # the effective conv weight W[o][c][t] is the mode-1 image of w_orig[c][o][T - 1 - t]
        w_orig = b['w'].transpose(0, 1).flip(2, 3).contiguous().to(dev)
        pack = ops.pack_weights(w_orig, 1, prec)
        a = ops.act_pack(x, pro=0, prec=prec, grad=True)
    else:
        pack = ops.pack_weights(b['w'].to(dev), 0, prec)
        a = ops.act_pack(x, pro=pro, prec=prec)
    # the planes decode to the inputs (pro 2 = relu on the way in)
    from conv_pipe_cases import planes64, weights64
    inv = a.inv.double().cpu().item() if a.inv is not None else 1.0
    got_a = [t.cpu() * inv for t in planes64(a.hi, a.lo, prec, cin)]
    for gt, wt_ in zip(got_a, b['a_terms']):
        assert torch.equal(gt, wt_), 'activation planes do not decode to the input: ' + E.first_mismatch(gt, wt_, 'ncyx')
    got_w = [t.cpu() for t in weights64(pack, prec, cout, cin, ks)]
    for gt, wt_ in zip(got_w, b['w_terms']):
        assert torch.equal(gt, wt_), 'weight pack does not decode to the input: ' + E.first_mismatch(gt, wt_, ('co', 'ci', 'ky', 'kx'))
    bias = b['bias'].to(dev) if b['bias'] is not None else None
    res = b['res'].contiguous().to(dev) if b['res'] is not None else None
    m16 = ops.act_pack(b['mask_src'].to(dev), pro=0, prec=0) if b['mask_src'] is not None else None
    want_amax = bool(case['amax']) and prec == E.PREC_F16
    out = ops.conv16(a, pack, ksize=ks, upsample=bool(ups), bias=bias, res=res, res_shift=case['rs'], alpha=alpha, prec=prec, relu_mask=m16,
                     out16=case['out16'], stats=bool(case['stats']), want_y=bool(case['want_y']), y_relu=bool(case['y_relu']), amax=want_amax)
    rec = ops.last_launch_form()
    torch.cuda.synchronize()
    if log:
        with open(log, 'a') as f:
            f.write(json.dumps(dict(case=case['id'], prec=prec, wide=wide, env=env, rec=rec)) + '\n')
    check_form(case, prec, rec, env)
    out = out if isinstance(out, tuple) else (out,)
    y = out[0]
    o16 = out[1] if case['out16'] is not None else None
    cs = out[-1] if case['stats'] else None
    ref = b['ref']
    ref_nhwc = ref.permute(0, 2, 3, 1).contiguous()
    tag = f"{case['id']} prec={prec} wide={wide}"
    if case['want_y']:
        gy = y.cpu().double()
        assert torch.equal(gy, ref_nhwc), f'{tag}: y: ' + E.first_mismatch(gy, ref_nhwc, 'nyxc')
    else:
        assert y is None
    if o16 is not None:
        hi_w, lo_w = R.planes(ref_nhwc.float().numpy(), 2 if case['out16'] else 0, prec=prec)
        for nm, got, want in (('hi', o16.hi, hi_w), ('lo', o16.lo, lo_w)):
            if want is None:
                assert got is None
                continue
            want = want.copy()
            want[want == 0x8000] = 0
            gw = torch.from_numpy(words(got).astype(np.int32)).reshape(n, h, w, -1)
            ww = torch.from_numpy(want.astype(np.int32)).reshape(n, h, w, -1)
            assert torch.equal(gw, ww), f'{tag}: out16 {nm} words: ' + E.first_mismatch(gw, ww, 'nyxc')
    if want_amax:
        slots = y._lp_amax[0]
        assert slots.max().item() == ref.abs().max().item(), (tag, 'amax', slots.max().item(), ref.abs().max().item())
    errs = {}
    if case['stats']:
        th, tw = 1 << rec['lth'], 1 << rec['ltw']
        if rec['ksplit'] > 1 or (h % th) or (w % tw):
            assert cs is None and rec['stats'] == 0, f'{tag}: split-K / ragged launches must not offer fused statistics'
        if cs is not None:
            assert rec['stats'] == 1, rec
            from conv_pipe_cases import rel
            gamma, beta = torch.ones(n, cout, device=dev), torch.zeros(n, cout, device=dev)
            mean, rstd, _, _ = ops.norm_stats_finalize(cs, n, cout, gamma, beta, 1e-4)
            r64 = ref.reshape(n, cout, -1)
            errs['mean'] = rel(mean.cpu(), r64.mean(2))
            errs['rstd'] = rel(rstd.cpu(), (r64.var(2, unbiased=False) + 1e-4).rsqrt())
            for k, v in errs.items():
                assert v < 2e-5, (tag, k, v)
    return rec, errs, b['quanta']


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('LP_CONV') or k.startswith('LP_WGRAD')}
    log = os.environ.get('LP_FORM_LOG')
    t0 = time.time()
    bad = []
    for prec in PRECS:
        for index, case in enumerate(CASES):
            for wide in roles(index, prec):
                try:
                    rec, errs, quanta = run_case(index, case, prec, wide, env, log)
                    form = f"{rec['kernel']}<{rec['ks']},{rec['ups']},{rec['wm']},{rec['wn']},{rec['mr']},{rec['nr']}> cc={rec['cc']} pp={rec['pp']} " \
                           f"nbuf={rec['nbuf']} ksplit={rec['ksplit']} a_dbuf={rec['a_dbuf']} stats={rec['stats']}"
                    print(f"[conv_dma_exact {env}] prec={prec} wide={wide} {case['id']}: {form} budget=2^{np.log2(max(quanta, 1)):.1f} "
                          + ' '.join(f'{k}={v:.1e}' for k, v in errs.items()), flush=True)
                except AssertionError as e:
                    print(f"[conv_dma_exact {env}] prec={prec} wide={wide} {case['id']}: FAILED {e}", flush=True)
                    bad.append((prec, wide, case['id'], str(e)[:400]))
    print(f'[conv_dma_exact {env}] wall {time.time() - t0:.1f} s', flush=True)
    if bad:
        print('FAILED', bad)
        sys.exit(1)
    print('CONV_DMA_EXACT_OK')


if __name__ == '__main__':
    main()
