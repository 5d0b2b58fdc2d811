"""Cases of tests/test_conv_phase_exact.py: the KS = 2 forms of conv_dma_kernel (csrc/conv_dma.hip) -- phase == 1, the scatter to the x2 grid, and phase == 2,
the gather with its K loop over (phase, chunk) -- through their four callers, lp_pack_weights modes 2 (forward of the upsampled conv), 3 (its data
gradient), 4 (conv + AvgPool2d(2) forward) and 5 (its data gradient, with the ReLU mask), on operands for which fp32 accumulation is exact
(tests/exact_operands.py).  Run as a script in a fresh interpreter per knob setting (the knob table is read once per process).  Every case asserts
its budget on the CPU, packs its weights with lp_pack_weights and asserts the planes equal tests/operand_restatement.py's weight_pack word for word
and decode to the pre-summed integers, calls conv16, reads the launch record, asserts the form its id names, and asserts torch.equal against the fp64
reference: y, the out16 planes (the bit-level packer applied to the exact y), planes-only output and the amax slot.  A failure names (n, y, x, channel).

The reference is E.phase_conv64 on the split of the PRE-SUMMED taps.  In the single-plane modes a wide weight is bounded by 63, so every tap sum is
exact in 8 significand bits, and the reference of modes 2 and 4 is the DENSE definition -- conv64(ups=True) and the average pool of conv64 with the
original 3x3 weights -- which build() asserts to be the same numbers.  Modes 4 / 5 carry the factor 1/4: their weight quantum is QW / 4.

Shapes are (N, H, W, Cin, Cout) with H x W the OUTPUT map of the launch, Cin its contraction and Cout its output channels; at most 2048 output pixels.
What differs from the list first proposed, because the dispatcher's rules say so (the launch record is the authority):
  * mode 2 `2x16x16 64->128`: the 8 x 8 low-resolution grid puts two images into a 128-row tile, so statistics are requested and must NOT be offered;
    the <2,2,4,4> case that is offered them is the ping-pong pair's `2x16x64 64->128` (8 x 16 tiles, one image each);
  * the data-gradient shrink of the split factor: lp_pack_weights through hipops pads the contraction to a multiple of 64, so the gather form always has
    a multiple of 8 (phase, chunk) stages and a power-of-two split never shrinks; with CinP = 96 (12 stages) the split loop stops at 4 (it wants two
    stages per slice) and does not shrink either.  The case packs dy's 160 channels with ColsP = 160 through the C entry point (the header pads to 32):
    20 stages, the loop reaches 8 and must shrink to 7 (ceil(20 / 3)).  Split 6 is reached by the scatter form with Cin 576 (18 chunks), as in the dense
    kernel;
  * ping-pong: with the default knobs no shape of this size pairs tiles (it takes 200 paired workgroups); under LP_CONV_PP=1 `2x16x64` (two tile
    positions per phase) must pair and `1x16x96` (three) must not, and the gather form pairs whenever it has two tiles (`1x12x20`)."""
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import exact_operands as E  # noqa: E402
import operand_restatement as R  # noqa: E402
from conv_dma_cases import hash_id, words  # noqa: E402


def C(cid, mode, shape, form, **opt):
    d = dict(id=cid, mode=mode, shape=shape, form=form, bias=0, res=0, mask=0, out16=None, y_relu=0, want_y=1, stats=0, amax=0, big=0, pp1=None,
             cols_p=None, ksplit=1, offered=0)
    assert set(opt) <= set(d), set(opt) - set(d)
    d.update(opt)
    return d


T4144, T2244 = dict(wm=4, wn=1, mr=4, nr=4), dict(wm=2, wn=2, mr=4, nr=4)
ALL = dict(bias=1, res=1, mask=1, out16=1, y_relu=1)                  # every option of the split-K finish at once
POOL = dict(bias=1, res=1, y_relu=1, out16=1)                         # what nn.ConvPoolFn asks of the mode-4 launch
DGRAD = dict(mask=1, amax=1)                                          # ... and of the mode-5 launch

# ``ksplit`` / ``offered``: the split factor and whether requested statistics are offered, under the DEFAULT knobs (where every case runs unpaired on the 3-deep ring)
CASES = [
    # mode 2: forward of the upsampled conv, upsample = 2, the residual at low resolution (res_shift = 1)
    C('m2 <2,2,4,4> 2x16x16 64->128 two images per tile', 2, (2, 16, 16, 64, 128), T2244, bias=1, res=1, out16=0, stats=1),
    C('m2 <4,1,4,4> 1x32x32 64->64', 2, (1, 32, 32, 64, 64), T4144, bias=1, out16=1, stats=1, offered=1),
    C('m2 3x16x16 32->16 two images per tile', 2, (3, 16, 16, 32, 16), T2244, res=1, stats=1),
    C('m2 splitk4 2x8x8 256->192', 2, (2, 8, 8, 256, 192), T2244, ksplit=4, **ALL),
    C('m2 ragged 1x24x40 160->128 five chunks', 2, (1, 24, 40, 160, 128), T2244, ksplit=2, bias=1, out16=0, stats=1),
    C('m2 3x4x4 96->136 2x2 grid, channel tails', 2, (3, 4, 4, 96, 136), T2244, ksplit=2, bias=1, res=1, out16=1),
    C('m2 planes-only 2x16x16 64->64', 2, (2, 16, 16, 64, 64), T2244, res=1, out16=1, want_y=0),
    C('m2 pp even 2x16x64 64->128', 2, (2, 16, 64, 64, 128), T2244, bias=1, res=1, out16=1, stats=1, offered=1, pp1='even'),
    C('m2 pp odd 1x16x96 64->128', 2, (1, 16, 96, 64, 128), T2244, bias=1, stats=1, offered=1, pp1='odd', big=1),
    C('m2 splitk6 2x8x8 576->128 (18 chunks: fixed-point shrink)', 2, (2, 8, 8, 576, 128), T2244, ksplit=6, bias=1, out16=0),
    # mode 5: data gradient of conv + pool, upsample = 2, ReLU mask, amax, the fp16 gradient scale through alpha2
    C('m5 2x16x16 64->64', 5, (2, 16, 16, 64, 64), T2244, **DGRAD),
    C('m5 <4,1,4,4> 1x32x32 128->64', 5, (1, 32, 32, 128, 64), T4144, ksplit=2, **DGRAD),
    C('m5 splitk4 2x8x8 256->128', 5, (2, 8, 8, 256, 128), T2244, ksplit=4, big=1, **DGRAD),
    # mode 3: phase data gradient, upsample = 3; the sizes are the low-resolution output
    C('m3 splitk8 2x8x8 128->64', 3, (2, 8, 8, 128, 64), T2244, ksplit=8, amax=1),
    C('m3 <4,1,4,4> 1x16x16 64->32', 3, (1, 16, 16, 64, 32), T4144, ksplit=4, amax=1, stats=1),
    C('m3 splitk8 1x4x4 512->128 64 stages', 3, (1, 4, 4, 512, 128), T2244, ksplit=8),
    C('m3 splitk7 1x4x4 160->64 ColsP 160 (20 stages: 8 shrinks to 7)', 3, (1, 4, 4, 160, 64), T2244, ksplit=7, cols_p=160, amax=1),
    C('m3 ragged 1x12x20 64->64', 3, (1, 12, 20, 64, 64), T2244, ksplit=4, pp1='gather', big=1),
    # mode 4: conv + pool forward, upsample = 3, bias, pooled-resolution residual, y_relu, planes of relu(y)
    C('m4 2x8x8 64->128', 4, (2, 8, 8, 64, 128), T2244, ksplit=4, **POOL),
    C('m4 <4,1,4,4> 1x16x16 64->64', 4, (1, 16, 16, 64, 64), T4144, ksplit=4, stats=1, **POOL),
    C('m4 splitk8 8x4x4 128->128', 4, (8, 4, 4, 128, 128), T2244, ksplit=8, **POOL),
    C('m4 planes-only 2x8x8 64->64', 4, (2, 8, 8, 64, 64), T2244, ksplit=4, bias=1, res=1, out16=1, want_y=0),
]
assert len({c['id'] for c in CASES}) == len(CASES)
assert all(c['shape'][0] * c['shape'][1] * c['shape'][2] <= 2048 for c in CASES)

PRECS = (E.PREC_F16, E.PREC_BF16X3, E.PREC_BF16)


def roles(index, prec):
    """which operand is wide: bf16x3 runs both (so that hi*lo and lo*hi are both live), the single-plane modes alternate by case"""
    return ('a', 'w') if prec == E.PREC_BF16X3 else (('a', 'w')[index & 1],)


def pro_of(index, case):
    """the activation pack's prologue: gradients (modes 3 / 5) are packed as they are, forward inputs alternate identity and relu"""
    return 0 if case['mode'] in (3, 5) else (0, 2)[index & 1]


def geometry(case):
    """-> gather, (hin, win), res_shift, weight shape [Cout_fwd][Cin_fwd][3][3], weight quantum"""
    n, h, w, cin, cout = case['shape']
    mode = case['mode']
    gather = mode in (3, 4)
    hw_in = (2 * h, 2 * w) if gather else (h // 2, w // 2)
    w_shape = (cout, cin, 3, 3) if mode in (2, 4) else (cin, cout, 3, 3)          # (the data-gradient launches contract over the forward conv's Cout)
    return gather, hw_in, (1 if mode == 2 else 0), w_shape, (E.QW / 4 if mode >= 4 else E.QW)


def build(case, prec, wide, pro=0):
    """CPU side of a case: the fp32 inputs (integers times a power of two), the 16 pre-summed taps, the asserted budget, the exact fp64 reference y"""
    n, h, w, cin, cout = case['shape']
    mode = case['mode']
    gather, (hin, win), rs, w_shape, qw = geometry(case)
    seed = (hash_id(case['id']) + 7 * prec + (1 if wide == 'w' else 0)) & 0x7FFFFFFF
    g = torch.Generator().manual_seed(seed ^ 0x5EED)
    q = E.ALPHA * E.QA * qw
    bias = E.draw_ints(g, (cout,), 1023).float() * q if case['bias'] else None
    res = E.draw_ints(g, (n, h >> rs, w >> rs, cout), 1023).float() * q if case['res'] else None
    res_full = None
    if res is not None:
        res_full = res.permute(0, 3, 1, 2)
        if rs:
            res_full = E.up2(res_full)
    mask_src = torch.randn((n, h, w, cout), generator=g) if case['mask'] else None

    def taps_of(wt):
        return torch.from_numpy(R.weight_values(wt.numpy(), mode))          # fp32 [16][rows = Cout][cols = Cin]: sums of integers, exact

    def bound(a, wt):
        return E.assert_budget(E.phase_bound(E.terms(a, prec), E.terms(taps_of(wt), prec), gather, E.ALPHA, bias, res_full), q, case['id'])
    x_in, wt = E.draw_phase_pair(seed, (n, cin, hin, win), w_shape, prec, wide, bound, big=bool(case['big']))
    a = torch.relu(x_in) if pro == 2 else x_in      # the pack's prologue: the operand is relu of the drawn input (the bound only shrinks)
    taps = taps_of(wt)
    assert tuple(taps.shape) == (16, cout, cin)
    ti = taps.double() / qw
    assert torch.equal(ti, ti.round()) and (prec == E.PREC_BF16X3 or float(ti.abs().max()) <= 4 * E.WIDE_W_PHASE), 'tap sums are integers of the weight quantum'
    a_terms, t_terms = E.terms(a, prec), E.terms(taps, prec)
    quanta = E.assert_budget(E.phase_bound(a_terms, t_terms, gather, E.ALPHA, bias, res_full), q, case['id'])
    contraction = E.phase_conv64(a_terms, t_terms, gather)
    if prec != E.PREC_BF16X3 and mode in (2, 4):      # the operation itself: exact tap sums make the dense definition the same numbers
        dense = E.conv64(a_terms, E.terms(wt, prec), ups=True) if mode == 2 else F.avg_pool2d(E.conv64(a_terms, E.terms(wt, prec)), 2)
        assert torch.equal(contraction, dense), 'the phase algebra of the taps is not the dense operation: ' + E.first_mismatch(contraction, dense, 'ncyx')
        contraction = dense
    ref = E.ALPHA * contraction
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
    if res_full is not None:
        ref = ref + res_full.double()
    if mask_src is not None:
        ref = torch.where(mask_src.permute(0, 3, 1, 2) > 0, ref, torch.zeros_like(ref))
    if case['y_relu']:
        ref = torch.relu(ref)
    assert tuple(ref.shape) == (n, cout, h, w)
    assert torch.equal(ref.float().double(), ref), 'the reference itself is not an fp32 value'
    return dict(x=x_in, a=a, w=wt, a_terms=a_terms, t_terms=t_terms, bias=bias, res=res, mask_src=mask_src, ref=ref, quanta=quanta)


def pack(ops, wt, mode, prec, cols_p=None):
    """hipops.pack_weights; ``cols_p``: the same entry point with the contraction padded to this multiple of 32 (include/lp_hip.h) instead of hipops' 64"""
    if cols_p is None:
        return ops.pack_weights(wt, mode, prec)
    cout, cin, taps, taps_out, rows, cols, rows_p, _ = ops._pack_geometry(wt, mode, False)
    assert cols_p % 32 == 0 and cols_p >= cols
    hi = torch.empty((taps_out, rows_p, cols_p), dtype=torch.int16, device=wt.device)
    lo = torch.empty_like(hi) if prec == E.PREC_BF16X3 else None
    ops.check(ops._lib.lib().lp_pack_weights(wt.data_ptr(), hi.data_ptr(), ops._p(lo), cout, cin, taps, rows_p, cols_p, mode, ops._f16(prec), ops._stream()),
              'lp_pack_weights')
    return ops.WeightPack(hi, lo, rows, cols, rows_p, cols_p, taps_out)


def check_pack(case, prec, pk, b, tag):
    """the planes lp_pack_weights wrote == tests/operand_restatement.py's weight_pack word for word, and they decode to the pre-summed integers"""
    n, h, w, cin, cout = case['shape']
    want_hi, want_lo = R.weight_pack(b['w'].numpy(), case['mode'], pk.rows_p, pk.cols_p, prec)
    dt = torch.float16 if prec == E.PREC_F16 else torch.bfloat16
    for nm, got, want, term in (('hi', pk.hi, want_hi, b['t_terms'][0]), ('lo', pk.lo, want_lo, b['t_terms'][-1])):
        if want is None:
            assert got is None
            continue
        gw = torch.from_numpy(got.cpu().numpy().view(np.uint16).astype(np.int32))
        ww = torch.from_numpy(want.astype(np.int32))
        assert torch.equal(gw, ww), f'{tag}: weight pack {nm} words differ from the restatement: ' + E.first_mismatch(gw, ww, ('tap', 'row', 'col'))
        dec = got.cpu().view(dt if nm == 'hi' else torch.bfloat16).double()
        assert not dec[:, cout:, :].any() and not dec[:, :, cin:].any(), f'{tag}: pad rows / columns of the pack are not zero'
        assert torch.equal(dec[:, :cout, :cin], term), f'{tag}: weight pack {nm} does not decode to the pre-summed taps: ' + \
            E.first_mismatch(dec[:, :cout, :cin], term, ('tap', 'row', 'col'))


def tile_positions(case, rec):
    """tile positions per image group on the grid the tiles cover (scatter: the low-resolution INPUT; gather: the output)"""
    n, h, w = case['shape'][:3]
    gh, gw = (h // 2, w // 2) if case['mode'] in (2, 5) else (h, w)
    th, tw = 1 << rec['lth'], 1 << rec['ltw']
    return ((gh + th - 1) // th) * ((gw + tw - 1) // tw), gh, gw, th, tw


def check_form(case, prec, rec, env):
    """the record against what the case's id names (the tile in every setting; split, ring, pairing, statistics under the default knobs) and
    against what each knob promises"""
    assert rec['what'] == 'conv' and rec['prec'] == prec and rec['kernel'] == 'dma' and rec['ks'] == 2 and rec['cc'] == 32, rec
    for k, v in case['form'].items():
        assert rec[k] == v, (case['id'], k, v, rec)
    knobs = {k: v for k, v in env.items() if k.startswith('LP_CONV')}
    scatter = case['mode'] in (2, 5)
    txy, gh, gw, th, tw = tile_positions(case, rec)
    assert rec['finish'] == (1 if rec['ksplit'] > 1 else 0), rec
    assert not (scatter and rec['pp'] and (txy & 1)), ('a pair of tiles straddles two phases', rec)
    if not knobs:
        assert rec['ksplit'] == case['ksplit'] and rec['pp'] == 0 and rec['nbuf'] == 3, (case['id'], rec)
        assert rec['stats'] == (case['offered'] if case['stats'] else 0), (case['id'], rec)
    if knobs.get('LP_CONV_KSPLIT') == '1':
        assert rec['ksplit'] == 1, rec
    if knobs.get('LP_CONV_PP') == '0':
        assert rec['pp'] == 0, rec
    if knobs.get('LP_CONV_PP') == '1' and case['pp1']:
        assert rec['pp'] == (0 if case['pp1'] == 'odd' else 1) and (txy & 1) == (1 if case['pp1'] == 'odd' else 0), (case['id'], rec, txy)
    if knobs.get('LP_CONV_NBUF') == '2':
        assert rec['nbuf'] == 2 and rec['pp'] == 0, rec
    if knobs.get('LP_CONV_NBUF') == '3' and not rec['pp']:
        assert rec['nbuf'] == 3, rec
    # statistics may only be offered on full tiles of one launch without split-K whose row blocks stay inside one image; the scatter form
    # orders its rows (image group, phase, tile), so it needs one image per tile as well
    covered = rec['ksplit'] == 1 and gh % th == 0 and gw % tw == 0 and (th * tw << rec['lnb']) == rec['wm'] * rec['mr'] * 16 and th * tw >= rec['mr'] * 16 and \
        (not scatter or rec['lnb'] == 0)
    if not (case['stats'] and covered):
        assert rec['stats'] == 0, ('statistics offered on a geometry that is not covered', case['id'], rec)


def run_case(index, case, prec, wide, env, log):
    from latent_pose_reenactment_amd import hipops as ops
    from conv_pipe_cases import planes64, rel
    n, h, w, cin, cout = case['shape']
    mode = case['mode']
    gather, (hin, win), rs, w_shape, qw = geometry(case)
    grad = mode in (3, 5)
    pro = pro_of(index, case)
    b = build(case, prec, wide, pro)
    dev = 'cuda'
    tag = f"{case['id']} prec={prec} wide={wide}"
    x = b['x'].permute(0, 2, 3, 1).contiguous().to(dev)
    alpha = torch.tensor([E.ALPHA], device=dev)
    pk = pack(ops, b['w'].to(dev), mode, prec, case['cols_p'])
    a = ops.act_pack(x, pro=pro, prec=prec, grad=grad)
    assert (a.inv is not None) == (grad and prec == E.PREC_F16)
    inv = a.inv.double().cpu().item() if a.inv is not None else 1.0
    got_a = [t.cpu() * inv for t in planes64(a.hi, a.lo, prec, cin)]
    for gt, wt_ in zip(got_a, b['a_terms']):
        assert torch.equal(gt, wt_), f'{tag}: activation planes do not decode to the input: ' + E.first_mismatch(gt, wt_, 'ncyx')
    check_pack(case, prec, pk, b, tag)
    bias = b['bias'].to(dev) if b['bias'] is not None else None
    res = b['res'].contiguous().to(dev) if b['res'] is not None else None
    m16 = ops.act_pack(b['mask_src'].to(dev), pro=0, prec=prec) if b['mask_src'] is not None else None
    want_amax = bool(case['amax']) and prec == E.PREC_F16
    out = ops.conv16(a, pk, ksize=3, upsample=not gather, phase=not gather, phase_dgrad=gather, bias=bias, res=res, res_shift=rs, alpha=alpha, prec=prec,
                     relu_mask=m16, out16=case['out16'], stats=bool(case['stats']), want_y=bool(case['want_y']), y_relu=bool(case['y_relu']), amax=want_amax)
    rec = ops.last_launch_form()
    torch.cuda.synchronize()
    if log:
        with open(log, 'a') as f:
            f.write(json.dumps(dict(case=case['id'], mode=mode, prec=prec, wide=wide, env=env, rec=rec)) + '\n')
    check_form(case, prec, rec, env)
    out = out if isinstance(out, tuple) else (out,)
    y = out[0]
    o16 = out[1] if case['out16'] is not None else None
    cs = out[-1] if case['stats'] else None
    ref = b['ref']
    ref_nhwc = ref.permute(0, 2, 3, 1).contiguous()
    if case['want_y']:
        gy = y.cpu().double()
        assert tuple(gy.shape) == (n, h, w, cout)
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
            gw_ = torch.from_numpy(words(got).astype(np.int32)).reshape(n, h, w, -1)
            ww = torch.from_numpy(want.astype(np.int32)).reshape(n, h, w, -1)
            assert torch.equal(gw_, ww), f'{tag}: out16 {nm} words: ' + E.first_mismatch(gw_, ww, 'nyxc')
    if want_amax:
        slots = y._lp_amax[0]
        assert slots.max().item() == ref.abs().max().item(), (tag, 'amax', slots.max().item(), ref.abs().max().item())
    errs = {}
    if case['stats']:
        assert (cs is not None) == bool(rec['stats']), (tag, rec)
        if cs is not None:
            gamma, beta = torch.ones(n, cout, device=dev), torch.zeros(n, cout, device=dev)
            mean, rstd, _, _ = ops.norm_stats_finalize(cs, n, cout, gamma, beta, 1e-4)
            r64 = ref.reshape(n, cout, -1)
            errs['mean'] = rel(mean.cpu(), r64.mean(2))
            errs['rstd'] = rel(rstd.cpu(), (r64.var(2, unbiased=False) + 1e-4).rsqrt())
            for k, v in errs.items():
                assert v < 2e-5, (tag, k, v)
    return rec, errs, b['quanta']


def main():
    env = {k: v for k, v in os.environ.items() if k.startswith('LP_CONV')}
    log = os.environ.get('LP_FORM_LOG')
    t0 = time.time()
    bad = []
    for prec in PRECS:
        for index, case in enumerate(CASES):
            for wide in roles(index, prec):
                try:
                    rec, errs, quanta = run_case(index, case, prec, wide, env, log)
                    form = f"{rec['kernel']}<{rec['ks']},{rec['wm']},{rec['wn']},{rec['mr']},{rec['nr']}> pp={rec['pp']} nbuf={rec['nbuf']} ksplit={rec['ksplit']} " \
                           f"stats={rec['stats']} tile=2^({rec['lth']},{rec['ltw']},{rec['lnb']})"
                    print(f"[conv_phase_exact {env}] prec={prec} wide={wide} {case['id']}: {form} budget=2^{np.log2(max(quanta, 1)):.1f} "
                          + ' '.join(f'{k}={v:.1e}' for k, v in errs.items()), flush=True)
                except AssertionError as e:
                    print(f"[conv_phase_exact {env}] prec={prec} wide={wide} {case['id']}: FAILED {e}", flush=True)
                    bad.append((prec, wide, case['id'], str(e)[:400]))
    print(f'[conv_phase_exact {env}] wall {time.time() - t0:.1f} s', flush=True)
    if bad:
        print('FAILED', bad)
        sys.exit(1)
    print('CONV_PHASE_EXACT_OK')


if __name__ == '__main__':
    main()
