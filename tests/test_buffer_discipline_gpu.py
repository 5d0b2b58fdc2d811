"""The kernel surface under tests/guarded_alloc.differential: every entry builds its inputs from a seeded CPU generator and calls hipops wrappers;
the call runs plain, with every fresh buffer full of NaN-like words (fill A) and with every fresh buffer full of large positive finite words (fill
B), inputs fenced, and EVERY word of every returned tensor must be the same in the three runs, every guard word intact.  No reference and no
tolerance: the fp64 comparisons stay in the per-kernel modules.  What fails here is a kernel that reads a workspace slot, pad word or output
element it never wrote, reads an input before its start or past its end, or stores outside a buffer (within guarded_alloc.GUARD_BYTES).

Shapes are the smallest the per-kernel modules show to be supported at which a ragged tile, a halo, a pad channel or a split is live.  An entry
returns the intermediate planes and packs too, so a failure names the first tensor that differs.  Where a wrapper or the C side chooses between
two forms of a kernel (fused statistics or none, a sliced weight gradient with its workspace or one slice, planes written directly or by a second
launch), the entry asserts the form its id names.  The amax slot cache of hipops is replaced by a fenced buffer per run and put back afterwards;
device tables a wrapper copies for itself (frames, PackBatch) are passed as fenced copies.

``unwritten=`` exemptions (the only ones; each with the line of include/lp_hip.h that says the kernel does not write the tensor): none so far --
``pool_grad_pack`` does not return ``scale_out`` in the bf16 modes and ``adain_relu_bwd`` does not return dx with ``keep_dx=False``, so neither is
reachable.  The statistics of a conv epilogue are compared over the [N * rows][Cout][3] words the header defines ("stats [rows][Cout][3] (capacity
stats_capacity_floats >= lp_conv16_stats_floats())"): the capacity behind them is no output."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as GA  # noqa: E402
from guarded_alloc import differential  # noqa: E402

pytestmark = pytest.mark.gpu

PRECS = [(0, 'bf16'), (1, 'bf16x3'), (2, 'f16')]
ENTRIES = []


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def _lib():
    from latent_pose_reenactment_amd import _lib
    return _lib.lib()


def entry(name, **opts):
    def deco(make):
        ENTRIES.append(pytest.param(make, opts, id=name))
        return make
    return deco


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 12345)


def rn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


_SLOTS = {'saved': None, 'buf': None}


def fence_amax_slots():
    """hipops hands the amax slot groups out of a cached zeroed buffer (torch.zeros, 256 groups): put a fenced, zeroed one of the same size in its place
    for this run; ``restore_amax_slots`` puts the cache back when the entry is over"""
    s = _ops()._AMAX_SLOTS
    if _SLOTS['saved'] is None:
        _SLOTS['saved'] = (s.buf, s.pos, s.captured, s.n)
    n = _lib().lp_amax_slots() * _lib().lp_amax_slot_stride()
    _SLOTS['buf'] = torch.empty(n * 256, dtype=torch.float32, device='cuda').zero_()
    s.buf, s.pos, s.captured, s.n = _SLOTS['buf'], 0, False, n


def restore_amax_slots():
    if _SLOTS['saved'] is not None:
        s = _ops()._AMAX_SLOTS
        s.buf, s.pos, s.captured, s.n = _SLOTS['saved']
    _SLOTS['saved'] = _SLOTS['buf'] = None


def slots_of(t):
    """the amax slot group a kernel folded max|t| into (None: none attached) -- which must lie in the buffer ``fence_amax_slots`` installed"""
    rec = getattr(t, '_lp_amax', None)
    if rec is None:
        return None
    assert _SLOTS['buf'] is not None and rec[0].untyped_storage().data_ptr() == _SLOTS['buf'].untyped_storage().data_ptr(), \
        'the slot group did not come from the fenced buffer'
    return rec[0]


def stats_words(cs, cout):
    """the [N * rows][Cout][3] words of a conv epilogue's statistics (module docstring)"""
    if cs is None:
        return None
    return type(cs)(cs.part[:cs.rows * cs.images * cout * 3], cs.rows, cs.images)


# ---- wide convs: lp_conv16_fwd(_stats) through act_pack + pack_weights + conv16 ---------------------------------------------------------------
def conv_entry(name, n, h, w, cin, cout, k, *, precs=(0, 1, 2), form='plain', bias=False, res_shift=None, out16=None, want_y=True, stats=False,
               relu_mask=False, amax=False, small_k=False, mode=0, y_relu=False, covered=None, expect=None):
    """(n, h, w) = the OUTPUT map of the launch; form: plain | up (fused x2 upsample) | phase (mode-2 pack) | phase_dgrad (mode-3) | pool (mode-4
    pack, conv + AvgPool2d(2)) | pool_dgrad (mode-5); ``covered`` (with ``stats``): whether the epilogue's fused statistics cover the geometry -- asserted;
    ``expect``: fields of the launch record (hipops.last_launch_form) that the form named by the entry must show (a value, or a predicate) -- asserted"""
    assert not stats or covered is not None
    for prec in precs:
        def make(prec=prec):
            ops = _ops()
            g = gen(n, h, w, cin, cout, k, prec, len(name))
            hin, win = {'plain': (h, w), 'up': (h // 2, w // 2), 'phase': (h // 2, w // 2), 'phase_dgrad': (2 * h, 2 * w), 'pool': (2 * h, 2 * w),
                        'pool_dgrad': (h // 2, w // 2)}[form]
            pmode = {'plain': mode, 'up': mode, 'phase': 2, 'phase_dgrad': 3, 'pool': 4, 'pool_dgrad': 5}[form]
            wshape = (cin, cout, k, k) if pmode % 2 else (cout, cin, k, k)          # a data-gradient pack contracts over the weight's OUTPUT channels
            ins = {'x': rn(g, n, hin, win, cin), 'wt': rn(g, *wshape, scale=1 / math.sqrt(cin * k * k)), 'alpha': torch.tensor([0.83])}
            if bias:
                ins['bias'] = rn(g, cout)
            if res_shift is not None:
                ins['res'] = rn(g, n, h >> res_shift, w >> res_shift, cout)
            if relu_mask:
                ins['mask'] = rn(g, n, h, w, cout)

            def fn(x, wt, alpha, bias=None, res=None, mask=None):
                if amax:
                    fence_amax_slots()
                a = ops.act_pack(x, pro=2, prec=prec)
                pk = ops.pack_weights(wt, pmode, prec, small_k=small_k)
                m16 = ops.act_pack(mask, pro=0, prec=0) if mask is not None else None
                out = ops.conv16(a, pk, ksize=k, upsample=form in ('up', 'phase', 'pool_dgrad'), bias=bias, res=res, res_shift=res_shift or 0, alpha=alpha,
                                 prec=prec, relu_mask=m16, out16=out16, amax=amax, stats=stats, want_y=want_y, phase=form in ('phase', 'pool_dgrad'),
                                 phase_dgrad=form in ('phase_dgrad', 'pool'), y_relu=y_relu)
                rec = ops.last_launch_form()
                for key, want in (expect or {}).items():
                    assert want(rec[key]) if callable(want) else rec[key] == want, f'the entry names a form that did not run: {key} = {rec[key]} in {rec}'
                out = list(out) if isinstance(out, tuple) else [out]
                r = {'planes': a, 'pack': pk, 'mask16': m16, 'slots': slots_of(out[0]) if out[0] is not None else None}
                if stats:
                    assert (out[-1] is not None and out[-1].rows > 0) == covered, 'the other form ran: statistics ' + ('missing' if covered else 'present')
                    out[-1] = stats_words(out[-1], cout)
                r['out'] = out
                return r
            return fn, ins
        entry(f'conv16 {name} {n}x{h}x{w} {cin}->{cout} k{k} {dict(PRECS)[prec]}')(make)


conv_entry('plain', 2, 8, 8, 64, 128, 3)
conv_entry('1x1 cout 24', 2, 16, 16, 128, 24, 1, expect=dict(ks=1))
SPLITS = dict(ksplit=lambda v: v > 1, finish=1)          # (a slice needs >= 2 chunks of 32 input channels: 64 channels do not split)
conv_entry('split-K workspace residual', 8, 4, 4, 128, 64, 3, res_shift=0, expect=SPLITS)
conv_entry('fused upsample res_shift 1', 2, 8, 8, 64, 192, 3, form='up', res_shift=1, expect=dict(ks=3, ups=1))
conv_entry('narrow output bias', 2, 32, 32, 64, 4, 3, bias=True, expect=dict(wn=1, nr=1))
conv_entry('small-K pack', 1, 32, 32, 16, 8, 3, small_k=True)
conv_entry('masked last group H != W', 3, 8, 16, 64, 128, 3, expect=dict(tiles=3))          # (an odd number of tiles)
conv_entry('data-gradient pack', 2, 8, 8, 64, 128, 3, mode=1)
conv_entry('phase up', 3, 8, 8, 96, 136, 3, form='phase', bias=True, expect=dict(ks=2))          # (KS = 2: the phase forms' 2 x 2 taps)
conv_entry('phase up statistics not covered', 4, 8, 8, 32, 32, 3, form='phase', out16=0, stats=True, covered=False, expect=dict(ks=2, stats=0))
conv_entry('phase dgrad', 3, 4, 4, 136, 96, 3, form='phase_dgrad', expect=dict(ks=2))
conv_entry('conv+pool', 3, 8, 12, 64, 128, 3, form='pool', bias=True, res_shift=0, out16=1, y_relu=True, precs=(1, 2), expect=dict(ks=2))
conv_entry('conv+pool dgrad', 3, 16, 24, 128, 64, 3, form='pool_dgrad', precs=(1, 2), expect=dict(ks=2))
conv_entry('out planes', 2, 8, 8, 64, 128, 3, out16=1, bias=True)
conv_entry('out planes cout 20', 2, 8, 8, 64, 20, 3, out16=0)
conv_entry('planes only', 2, 8, 8, 64, 128, 3, out16=1, want_y=False)
conv_entry('statistics covered', 8, 16, 16, 128, 64, 1, stats=True, precs=(1, 2), covered=True, expect=dict(ks=1, stats=1))
conv_entry('statistics 3x3', 5, 16, 32, 64, 192, 3, stats=True, precs=(1, 2), covered=True, expect=dict(ks=3, stats=1))
conv_entry('statistics not covered', 1, 8, 8, 256, 128, 3, stats=True, precs=(1, 2), covered=False, expect=dict(stats=0))
conv_entry('statistics planes only', 2, 16, 16, 64, 64, 3, stats=True, out16=1, want_y=False, precs=(1, 2), covered=True)
conv_entry('relu_mask', 2, 8, 8, 64, 128, 3, relu_mask=True, mode=1)
conv_entry('relu_mask cout 20', 2, 8, 8, 64, 20, 3, relu_mask=True, mode=1)
conv_entry('amax slots', 2, 8, 8, 64, 128, 3, amax=True, mode=1, precs=(2,))
conv_entry('amax slots split-K', 8, 4, 4, 128, 64, 3, amax=True, mode=1, precs=(2,), expect=SPLITS)


# ---- lp_conv16_wgrad ---------------------------------------------------------------------------------------------------------------------------
def wgrad_entries():
    """the first five WGRAD_CASES of test_hip_ops.py (plain, tiny maps, fused x2 upsampling, Cout 4, 1x1) straight on lp_conv16_wgrad, then three shapes of
    wgrad3_pipe_cases.py: ragged with channel tails, upsampled through the DMA-staged kernel's geometry, and an uneven explicit split"""
    import test_hip_ops as TH
    import wgrad3_pipe_cases as WC
    cases = [c[:7] + (None,) for c in TH.WGRAD_CASES[:5]] + [c[:5] + (3,) + c[5:] for c in (WC.CASES[4], WC.CASES[6], WC.CASES[3])]
    assert [c[6] for c in cases[:5]] == [0, 0, 1, 0, 0] and cases[1][:3] == (8, 4, 4) and cases[3][4] == 4 and cases[4][5] == 1
    for case in cases:
        for prec, pname in PRECS:
            for variant in ('bias_grad', 'dbias_accumulate', 'sn_dot'):
                def make(case=case, prec=prec, variant=variant):
                    ops = _ops()
                    n, h, w, cin, cout, ks, ups, splits = case
                    g = gen(*case[:7], prec)
                    hin, win = (h // 2, w // 2) if ups else (h, w)
                    ins = {'x': rn(g, n, hin, win, cin), 'dy': rn(g, n, h, w, cout), 'bias_accum': rn(g, cout), 'w_orig': rn(g, cout, cin, ks, ks),
                           'u': rn(g, cout), 'v': rn(g, cin * ks * ks), 'sig': torch.tensor([1.7, 1 / 1.7]), 'accum': rn(g, cout, cin, ks, ks)}

                    def fn(x, dy, bias_accum, w_orig, u, v, sig, accum):
                        a = ops.act_pack(x, pro=2, prec=prec)
                        d = ops.act_pack(dy, pro=0, prec=prec, grad=True)
                        kw = dict(ksize=ks, upsample=bool(ups), prec=prec, splits=splits)
                        if variant == 'bias_grad':
                            out = ops.conv_wgrad16(a, d, bias_grad=True, **kw)
                        elif variant == 'dbias_accumulate':
                            out = (ops.conv_wgrad16(a, d, bias_grad=True, bias_accum=bias_accum, **kw), bias_accum)
                        else:          # the reduction launch leaves the <dw, W_orig> partials, lp_sn_grad_apply (ndot > 0) consumes them
                            out = (ops.conv_wgrad16(a, d, sn=(w_orig, u, v, sig), accum=accum, **kw), accum,
                                   ops.conv_wgrad16(a, d, sn=(w_orig, u, v, sig), **kw))
                        return {'a': a, 'd': d, 'out': out}
                    return fn, ins
                n, h, w, cin, cout, ks, ups, splits = case
                entry(f'conv_wgrad16 {variant} {n}x{h}x{w} {cin}->{cout} k{ks} up={ups} splits={splits} {pname}')(make)
    for prec, pname in PRECS:          # 1x1: wgrad1x1_kernel (no bias gradient) and conv_wgrad_kernel (with one), ragged channels and pixels
        for bias_grad in (False, True):
            def make(prec=prec, bias_grad=bias_grad):
                ops = _ops()
                g = gen(77, prec, bias_grad)
                ins = (rn(g, 3, 9, 8, 72), rn(g, 3, 9, 8, 40))

                def fn(x, dy):
                    a, d = ops.act_pack(x, pro=0, prec=prec), ops.act_pack(dy, pro=0, prec=prec, grad=True)
                    return a, d, ops.conv_wgrad16(a, d, ksize=1, prec=prec, bias_grad=bias_grad)
                return fn, ins
            entry(f'conv_wgrad16 1x1 3x9x8 72->40 bias_grad={int(bias_grad)} {pname}')(make)


wgrad_entries()


# ---- thin convs ------------------------------------------------------------------------------------------------------------------------------------
def thin_entries():
    for (n, h, w, cin, cout, k) in [(2, 20, 12, 3, 128, 1), (3, 12, 20, 3, 64, 3)]:
        for prec, pname in PRECS:
            for out16, want_y in ((None, True), (1, True), (1, False)):
                def make(n=n, h=h, w=w, cin=cin, cout=cout, k=k, prec=prec, out16=out16, want_y=want_y):
                    ops = _ops()
                    g = gen(n, h, w, cin, cout, k, prec)
                    ins = (rn(g, n, h, w, cin), rn(g, cout, cin, k, k, scale=0.3), rn(g, cout), torch.tensor([0.7]))

                    def fn(x, wt, bias, alpha):
                        assert ops.thin_conv_supported(cin, cout, k, w)
                        pk = ops.pack_weights(wt, 0, prec)
                        return pk, ops.thin_conv(x, pk, ksize=k, bias=bias, alpha=alpha, prec=prec, out16=out16, want_y=want_y)
                    return fn, ins
                entry(f'thin_conv {n}x{h}x{w} {cin}->{cout} k{k} out16={out16} want_y={int(want_y)} {pname}')(make)
    for (n, h, w, cin, cout, k) in [(2, 20, 12, 128, 4, 3), (2, 16, 16, 64, 3, 3)]:
        for pro in (0, 1):
            def make(n=n, h=h, w=w, cin=cin, cout=cout, k=k, pro=pro):
                ops = _ops()
                g = gen(n, h, w, cin, cout, k, pro)
                ins = (rn(g, n, h, w, cin), rn(g, n, h, w, cout), rn(g, n, cin), rn(g, n, cin))

                def fn(x, dy, scale, shift):
                    assert ops.thin_wgrad_supported(cin, cout, k, pro, w)
                    return ops.thin_wgrad(x, dy, ksize=k, pro=pro, scale=scale if pro else None, shift=shift if pro else None, bias_grad=True)
                return fn, ins
            entry(f'thin_wgrad {n}x{h}x{w} {cin}->{cout} k{k} pro{pro}')(make)
    for (n, h, w, cin, cout, k) in [(2, 20, 12, 3, 128, 1), (3, 12, 20, 3, 64, 3)]:          # the thin side is the INPUT
        def make(n=n, h=h, w=w, cin=cin, cout=cout, k=k):
            ops = _ops()
            g = gen(n, h, w, cin, cout, k, 5)
            ins = (rn(g, n, h, w, cin), rn(g, n, h, w, cout))

            def fn(x, dy):
                assert ops.thin_wgrad_supported(cin, cout, k, 0, w)
                return ops.thin_wgrad(x, dy, ksize=k, bias_grad=True)
            return fn, ins
        entry(f'thin_wgrad {n}x{h}x{w} {cin}->{cout} k{k}')(make)

    def make16():
        ops = _ops()
        g = gen(16, 16, 64, 4)
        ins = (rn(g, 2, 16, 16, 64), rn(g, 2, 16, 16, 4), rn(g, 2, 64), rn(g, 2, 64))

        def fn(x, dy, scale, shift):
            x16 = ops.act_pack(x, pro=0, prec=2)
            return x16, ops.thin_wgrad16(x16, dy, ksize=3, pro=1, scale=scale, shift=shift), ops.thin_wgrad16(x16, dy, ksize=3)
        return fn, ins
    entry('thin_wgrad16 2x16x16 64->4 k3')(make16)


thin_entries()


# ---- reflect border ----------------------------------------------------------------------------------------------------------------------------------
def reflect_entries():
    # the three smallest CASES of test_reflect_border.py run the weight gradient in ONE slice (no workspace); the two larger ones cut the border pixels
    # into slices whose partial tiles go through the workspace and lp_reflect_border_wgrad's reduction launch
    for case, sliced in [((2, 4, 4, 16, 16, False), False), ((3, 8, 8, 24, 40, False), False), ((2, 8, 8, 16, 8, True), False),
                         ((8, 16, 16, 64, 64, False), True), ((2, 32, 32, 32, 32, True), True)]:
        for prec, pname in PRECS:
            def make(case=case, prec=prec, sliced=sliced):
                ops = _ops()
                n, h, w, cin, cout, up = case
                g = gen(*case, prec)
                hs, ws = (h // 2, w // 2) if up else (h, w)
                ins = {'x': rn(g, n, hs, ws, cin), 'wgt': rn(g, cout, cin, 3, 3, scale=0.2), 'alpha': torch.tensor([0.6]), 'y': rn(g, n, h, w, cout),
                       'dy': rn(g, n, h, w, cout), 'dx': rn(g, n, h, w, cin), 'dxm': rn(g, n, h, w, cin), 'accum': rn(g, cout, cin, 3, 3),
                       'u': rn(g, cout), 'v': rn(g, cin * 9), 'sig': torch.tensor([1.3, 1 / 1.3])}

                def fn(x, wgt, alpha, y, dy, dx, dxm, accum, u, v, sig):
                    assert (_lib().lp_reflect_border_wgrad_workspace_bytes(n, h, w, cin, cout) > 0) == sliced, 'the other form of the weight gradient ran'
                    a = ops.act_pack(x, pro=2, prec=prec)
                    r = {'a': a, 'fwd': ops.reflect_border_fwd(a, wgt, alpha, y, prec=prec, upsample=up),
                         'wgrad': ops.reflect_border_wgrad(a, dy, prec=prec, upsample=up),
                         'wgrad_sn': (ops.reflect_border_wgrad(a, dy, prec=prec, upsample=up, sn=(wgt, u, v, sig), accum=accum), accum),
                         'dgrad': ops.reflect_border_dgrad(dy, wgt, alpha, dx)}
                    if not up:
                        r['dgrad_masked'] = ops.reflect_border_dgrad(dy, wgt, alpha, dxm, a)
                    return r
                return fn, ins
            entry(f'reflect_border {"x".join(str(int(v)) for v in case)} wgrad {"with" if sliced else "without"} workspace {pname}')(make)


reflect_entries()


# ---- norms ---------------------------------------------------------------------------------------------------------------------------------------------
def norm_entries():
    for shape in [(2, 4, 4, 64), (2, 32, 32, 4), (3, 5, 7, 8)]:
        for affine in (False, True):
            def make(shape=shape, affine=affine):
                ops = _ops()
                n, h, w, c = shape
                g = gen(*shape, affine)
                proj = rn(g, n, 2 * c)          # gamma / beta are [N, C] views of the projector's output row

                def fn(x, proj):
                    gamma, beta = (proj[:, :c], proj[:, c:2 * c]) if affine else (None, None)
                    return ops.instnorm_stats(x, gamma, beta, 1e-4)
                return fn, (rn(g, *shape, shift=0.5), proj)
            entry(f'instnorm_stats {"x".join(map(str, shape))} affine={int(affine)}')(make)

    for prec in (1, 2):          # lp_norm_stats_finalize on the partials of a conv epilogue: per image with [N, C] views, and as one BatchNorm
        def make(prec=prec):
            ops = _ops()
            n, h, w, cin, cout = 3, 16, 16, 64, 64
            g = gen(n, h, w, cin, cout, prec, 3)
            ins = (rn(g, n, h, w, cin, shift=0.3), rn(g, cout, cin, 1, 1, scale=1 / 8), rn(g, n, 2 * cout), rn(g, cout), rn(g, cout),
                   torch.zeros(cout), torch.ones(cout))

            def fn(x, wt, proj, gam, bet, rm, rv):
                a = ops.act_pack(x, pro=0, prec=prec)
                y, cs = ops.conv16(a, ops.pack_weights(wt, 0, prec), ksize=1, prec=prec, stats=True)
                assert cs is not None
                return (ops.norm_stats_finalize(cs, n, cout, proj[:, :cout], proj[:, cout:2 * cout], 1e-4),
                        ops.norm_stats_finalize(cs, 1, cout, gam, bet, 1e-5, running_mean=rm, running_var=rv, momentum=0.1), rm, rv)
            return fn, ins
        entry(f'norm_stats_finalize {dict(PRECS)[prec]}')(make)

    for shape in [(3, 5, 7, 8), (1, 65, 64, 8)]:
        for ups in (False, True):
            for add in (False, True):
                for form in ('fp32', 'planes bf16 keep_dx', 'planes bf16x3', 'x16'):
                    def make(shape=shape, ups=ups, add=add, form=form):
                        ops = _ops()
                        n, h, w, c = shape
                        g = gen(*shape, ups, add, len(form))
                        s = 2 if ups else 1
                        ins = {'dA': rn(g, n, h * s, w * s, c), 'x': rn(g, n, h, w, c), 'add': rn(g, n, h, w, c) if add else None, 'proj': rn(g, n, 2 * c),
                               'dproj': rn(g, n, 2 * c)}

                        def fn(dA, x, add, proj, dproj):
                            if form == 'x16':
                                fence_amax_slots()
                            gamma = proj[:, :c]
                            mean, rstd, scale, shift = ops.instnorm_stats(x, gamma, proj[:, c:2 * c], 1e-4)
                            xa = ops.act_pack(x, pro=0, prec=2) if form == 'x16' else x
                            assert not form.startswith('planes') or ops.planes_direct_ok(0, x, c), 'the two-launch fallback would run'
                            kw = {'fp32': {}, 'x16': {'amax': True}, 'planes bf16 keep_dx': {'planes': 0, 'keep_dx': True},
                                  'planes bf16x3': {'planes': 1, 'keep_dx': False}}[form]
                            out = ops.adain_relu_bwd(dA, xa, add, gamma, mean, rstd, scale, shift, dproj[:, :c], dproj[:, c:2 * c], ups, **kw)
                            return {'out': out, 'dproj': dproj, 'slots': slots_of(out) if form == 'x16' else None}
                        return fn, ins
                    entry(f'adain_relu_bwd {form} {"x".join(map(str, shape))} up={int(ups)} add={int(add)}')(make)

    for mask_mode, frozen, want_g in [(0, False, False), (0, False, True), (1, False, False), (2, False, True), (0, True, False)]:
        for shape in [(3, 5, 7, 8), (1, 65, 64, 24)]:
            def make(mask_mode=mask_mode, frozen=frozen, want_g=want_g, shape=shape):
                ops = _ops()
                c = shape[-1]
                g = gen(*shape, mask_mode, frozen, want_g)
                ins = (rn(g, *shape), rn(g, *shape), rn(g, *shape), rn(g, c, shift=1.0), rn(g, c))

                def fn(dA, x, msrc, gamma, beta):
                    mean, rstd, scale, shift = ops.bn_train_stats(x, gamma, beta, None, None, 0.1, 1e-5)
                    return ops.norm_act_bwd(dA, x, gamma, mean, rstd, scale, shift, mask_mode=mask_mode, mask_src=msrc if mask_mode == 2 else None,
                                            want_g=want_g, act_hi=6.0 if want_g and mask_mode == 0 else 0.0, frozen=frozen)
                return fn, ins
            entry(f'norm_act_bwd mask_mode={mask_mode} frozen={int(frozen)} want_g={int(want_g)} {"x".join(map(str, shape))}')(make)

    for prec, pname in PRECS:          # lp_bn_bwd16(_h): 65 splits of 64 pixels + a tail, 3 channel groups
        for mask_mode, x16, m16 in [(0, False, False), (1, False, False), (2, False, False), (2, False, True), (0, True, False)]:
            if x16 and prec != 2:
                continue
            def make(prec=prec, mask_mode=mask_mode, x16=x16, m16=m16):
                ops = _ops()
                shape = (1, 65, 64, 24)
                g = gen(*shape, prec, mask_mode, x16, m16)
                ins = (rn(g, *shape), rn(g, *shape), rn(g, *shape), rn(g, 24, shift=1.0), rn(g, 24))

                def fn(dA, x, msrc, gamma, beta):
                    mean, rstd, scale, shift = ops.bn_train_stats(x, gamma, beta, None, None, 0.1, 1e-5)
                    xa = ops.act_pack(x, pro=0, prec=2) if x16 else x
                    ms = None if mask_mode != 2 else (ops.act_pack(msrc, pro=2, prec=prec if prec != 1 else 0) if m16 else msrc)
                    return xa, ms, ops.bn_bwd16(dA, xa, gamma, mean, rstd, scale, shift, prec=prec, mask_mode=mask_mode, mask_src=ms, want_g=mask_mode == 2)
                return fn, ins
            entry(f'bn_bwd16 mask_mode={mask_mode} x16={int(x16)} mask16={int(m16)} {pname}')(make)

    def make_bts():
        ops = _ops()
        g = gen(1000, 256)
        ins = (rn(g, 1000, 256, shift=0.2), rn(g, 256, shift=1.0), rn(g, 256), torch.zeros(256), torch.ones(256))

        def fn(y, gamma, beta, rm, rv):
            return ops.bn_train_stats(y, gamma, beta, rm, rv, 0.1, 1e-5), rm, rv
        return fn, ins
    entry('bn_train_stats 1000x256')(make_bts)

    for accumulate in (False, True):
        def make(accumulate=accumulate):
            ops = _ops()
            g = gen(5, 40, accumulate)
            ins = (rn(g, 5, 2 * 40), rn(g, 40), rn(g, 40))

            def fn(dproj, ag, ab):
                out = ops.norm_affine_grad(dproj[:, :40], dproj[:, 40:80], ag if accumulate else None, ab if accumulate else None)
                return out, ag, ab
            return fn, ins
        entry(f'norm_affine_grad accumulate={int(accumulate)}')(make)


norm_entries()


# ---- identity encoder ----------------------------------------------------------------------------------------------------------------------------------
def resnext_entries():
    import gconv_rows_cases as GC
    import test_resnext_hip as TR
    # the two smallest shapes of gconv_rows_cases.py (every tap partly outside; odd sizes) and the two smallest GCASES of test_resnext_hip.py (groups of
    # 4 and of 32).  lp_gconv16_wgrad needs W >= 4, so the 2 x 2 map runs forward and data gradient only -- its entry name says so.
    # covered = the epilogue leaves statistics partials (asserted)
    gcases = [(GC.CASES[0], False), (GC.CASES[1], False), (TR.GCASES[0], True), (TR.GCASES[4], False)]
    assert gcases[2][0] == (2, 16, 16, 128, 4) and gcases[3][0] == (8, 4, 4, 1024, 32)
    for case, covered in gcases:
        for prec, pname in PRECS:
            def make(case=case, prec=prec, covered=covered):
                ops = _ops()
                n, h, w, c, cg = case
                g = gen(*case, prec)
                ins = (rn(g, n, h, w, c), rn(g, n, h, w, c), rn(g, c, cg, 3, 3, scale=1 / math.sqrt(cg * 9)))

                def fn(x, dy, wt):
                    fence_amax_slots()
                    a, d = ops.act_pack(x, pro=0, prec=prec), ops.act_pack(dy, pro=0, prec=prec, grad=True)
                    pk0, pk1 = ops.pack_grouped(wt, 0, prec), ops.pack_grouped(wt, 1, prec)
                    fwd = list(ops.gconv16(a, pk0, prec=prec, stats=True, out16=True))
                    assert (fwd[-1] is not None and fwd[-1].rows > 0) == covered, 'the other form ran'
                    fwd[-1] = stats_words(fwd[-1], c)
                    po = list(ops.gconv16(a, pk0, prec=prec, stats=True, out16=True, want_y=False))
                    po[-1] = stats_words(po[-1], c)
                    dx = ops.gconv16(d, pk1, prec=prec, amax=True)
                    return {'a': a, 'd': d, 'pk0': pk0, 'pk1': pk1, 'fwd': fwd, 'planes_only': po, 'dgrad': dx, 'slots': slots_of(dx),
                            'wgrad': ops.gconv_wgrad16(a, d, cg, prec=prec) if w >= 4 else None}          # (lp_gconv16_wgrad: W >= 4)
                return fn, ins
            entry(f'gconv16 fwd dgrad {"wgrad " if case[2] >= 4 else "(no wgrad: W < 4) "}planes {"x".join(map(str, case))} {pname}')(make)

    for prec, pname in PRECS:
        def make_im2col(prec=prec):
            ops = _ops()
            g = gen(2, 3, 21, 19, prec)
            return (lambda x: ops.im2col_planes(x, 7, 2, 3, prec)), (rn(g, 2, 3, 21, 19),)
        entry(f'im2col_planes 2x3x21x19 k7 s2 {pname}')(make_im2col)

        def make_maxpool(prec=prec):
            ops = _ops()
            g = gen(2, 9, 7, 16, prec)
            ins = (rn(g, 2, 9, 7, 16), rn(g, 16, shift=1.0), rn(g, 16), rn(g, 2, 5, 4, 16))

            def fn(y, scale, shift, dout):
                out, o16, idx = ops.bn_relu_maxpool(y, scale, shift, prec)
                return out, o16, idx, ops.maxpool_bwd(dout, idx, 9, 7), ops.bn_relu_maxpool(y, scale, shift, prec, want_idx=False)
            return fn, ins
        entry(f'bn_relu_maxpool maxpool_bwd 2x9x7x16 {pname}')(make_maxpool)

        def make_baa(prec=prec):
            ops = _ops()
            shape = (3, 5, 7, 24)
            g = gen(*shape, prec, 9)
            ins = (rn(g, *shape), rn(g, 24, shift=1.0), rn(g, 24), rn(g, *shape), rn(g, 24, shift=1.0), rn(g, 24))

            def fn(y, scale, shift, res, rs, rsh):
                r = {'plain': ops.bn_add_act(y, scale, shift), 'res': ops.bn_add_act(y, scale, shift, res, prec=prec),
                     'res_affine': ops.bn_add_act(y, scale, shift, res, rs, rsh, relu=False, prec=prec)}
                if prec != 2:
                    r16 = ops.act_pack(res, pro=0, prec=prec)
                    r['planes'] = (r16, ops.bn_add_act(y, scale, shift, r16, prec=prec), ops.bn_add_act(y, scale, shift, r16, prec=prec, want_out=False))
                else:
                    y16 = ops.act_pack(y, pro=0, prec=2)
                    r['y16'] = (y16, ops.bn_add_act(y16, scale, shift, res, prec=2), ops.bn_add_act(y16, scale, shift, res, rs, rsh, prec=2, want_out=False),
                                ops.bn_act16(y16, scale, shift), ops.bn_act16(y16, scale, shift, relu=False))
                return r
            return fn, ins
        entry(f'bn_add_act planes 16 bn_act16 3x5x7x24 {pname}')(make_baa)

        def make_sub(prec=prec):
            ops = _ops()
            shape = (2, 7, 5, 16)
            g = gen(*shape, prec, 4)
            ins = (rn(g, *shape), rn(g, *shape), rn(g, 2, 4, 3, 16))

            def fn(x, d, s):
                a = ops.act_pack(x, pro=0, prec=prec)
                sub = ops.subsample2_16(a)
                return a, ops.subsample2(x), sub, ops.zero_stuff2_16(sub, 7, 5), ops.add_strided2(d, s)
            return fn, ins
        entry(f'subsample2 zero_stuff2 add_strided2 2x7x5x16 {pname}')(make_sub)

    def make_adain16():
        ops = _ops()
        g = gen(3, 5, 7, 24, 16)
        ins = (rn(g, 3, 5, 7, 24), rn(g, 3, 24, shift=1.0), rn(g, 3, 24))

        def fn(y, scale, shift):
            y16 = ops.act_pack(y, pro=0, prec=2)
            return y16, ops.adain_act16(y16, scale, shift), ops.adain_act16(y16, scale, shift, relu=False)
        return fn, ins
    entry('adain_act16 3x5x7x24')(make_adain16)

    def make_pg():
        ops = _ops()
        g = gen(192, 8)
        return (lambda wt: [ops.pack_grouped(wt, m, p) for m in (0, 1) for p in (0, 1, 2)]), (rn(g, 192, 8, 3, 3),)
    entry('pack_grouped 192/8 (pad rows)')(make_pg)

    def make_sm():
        ops = _ops()
        g = gen(3, 5, 7, 40)
        return (lambda x, gr: (ops.spatial_mean(x), ops.spatial_mean_bwd(gr, 5, 7))), (rn(g, 3, 5, 7, 40), rn(g, 3, 40))
    entry('spatial_mean fwd bwd 3x5x7x40')(make_sm)


resnext_entries()


# ---- pose encoder ------------------------------------------------------------------------------------------------------------------------------------------
def mobilenet_entries():
    def make_stem():
        ops = _ops()
        g = gen(3, 30, 18, 8)
        return (lambda x, w: ops.stem_conv_s2(x, w)), (rn(g, 3, 3, 30, 18), rn(g, 8, 3, 3, 3))
    entry('stem_conv_s2 3x30x18 -> 8')(make_stem)

    for (n, h, w, c, s) in [(3, 15, 9, 24, 2), (2, 8, 8, 4, 2), (3, 9, 13, 32, 1)]:
        def make(n=n, h=h, w=w, c=c, s=s):
            ops = _ops()
            g = gen(n, h, w, c, s)
            ho, wo = (h + s - 1) // s, (w + s - 1) // s
            ins = (rn(g, n, h, w, c), rn(g, c, 1, 3, 3), rn(g, c, shift=1.0), rn(g, c), rn(g, n, ho, wo, c))

            def fn(x, wt, sc, sh, dy):
                r = {'fwd': ops.dwconv3x3(x, wt, s), 'fwd_affine': ops.dwconv3x3(x, wt, s, sc, sh)}
                if s == 1:
                    r.update(dgrad=ops.dwconv3x3_dgrad(dy, wt, h, w, s), wgrad=ops.dwconv3x3_wgrad(x, dy, s), wgrad_affine=ops.dwconv3x3_wgrad(x, dy, s, sc, sh))
                y, (part, rows) = ops.dwconv3x3_stats(x, wt, s, sc, sh)
                assert rows > 0
                rm, rv = torch.zeros(c, device=x.device), torch.ones(c, device=x.device)
                r['stats'] = (y, part, rows, ops.bn_finalize((part, rows), sc, sh, rm, rv, 0.1, 1e-5), rm, rv)
                return r
            return fn, ins
        entry(f'dwconv3x3 fwd stats dgrad wgrad bn_finalize {n}x{h}x{w}x{c} s{s}')(make)

    def make_pw():
        ops = _ops()
        g = gen(1, 7, 5, 960, 160)
        ins = (rn(g, 1, 7, 5, 960), rn(g, 160, 960, scale=1 / 31), rn(g, 960, shift=1.0), rn(g, 960), rn(g, 1, 7, 5, 960), rn(g, 160, shift=1.0), rn(g, 160))

        def fn(x, wt, sc, sh, res, bw, bb):
            y, xo, st = ops.pwconv(x, wt, in_scale=sc, in_shift=sh, in_relu6=True, in_res=res, want_x=True, stats=True)
            y2, _, st2 = ops.pwconv(x, wt, stats=True)
            return y, xo, st, ops.bn_finalize(st, bw, bb, None, None, 0.1, 1e-5), y2, st2, ops.pwconv(x, wt, in_scale=sc, in_shift=sh)[0]
        return fn, ins
    entry('pwconv 1x7x5 960->160 x_out stats_part bn_finalize')(make_pw)

    for prec in (None, 0, 1, 2):
        def make(prec=prec):
            ops = _ops()
            shape = (3, 5, 7, 24)
            g = gen(*shape, 3 if prec is None else prec)
            ins = (rn(g, *shape), rn(g, 24, shift=1.0), rn(g, 24), rn(g, *shape), torch.zeros(24), torch.ones(24))

            def fn(y, gamma, beta, res, rm, rv):
                scale, shift = ops.bn_batch_affine(y, gamma, beta, rm, rv, 0.1, 1e-5)
                return scale, shift, rm, rv, ops.affine_res(y, scale, shift, res, prec=prec), ops.affine_res(y, scale, shift, prec=prec), \
                    ops.affine_relu6_mean(y, scale, shift)
            return fn, ins
        entry(f'bn_stats affine_res affine_relu6_mean 3x5x7x24 planes={prec}')(make)


mobilenet_entries()


# ---- elementwise, heads, pools, losses ---------------------------------------------------------------------------------------------------------------------
def elementwise_entries():
    for (b, n, k) in [(11, 40, 64), (3, 1, 512)]:
        def make(b=b, n=n, k=k):
            ops = _ops()
            g = gen(b, n, k)
            ins = (rn(g, b, k), rn(g, n, k), rn(g, n), torch.tensor([0.9]), rn(g, b, n))

            def fn(x, w, bias, alpha, gr):
                return ops.linear_fwd(x, w, bias, alpha), ops.linear_fwd(x, w, None, None), ops.linear_bwd(x, w, gr, alpha, True, True, True), \
                    ops.linear_bwd(x, w, gr, None, True, False, False), ops.linear_bwd(x, w, gr, None, False, True, True)
            return fn, ins
        entry(f'linear fwd bwd B{b} N{n} K{k}')(make)

    def make_crop():
        ops = _ops()
        g = gen(2, 3, 24, 24, 32, 32)
        boxes = torch.tensor([[2.0, 20.0, 3.0, 21.0], [-5.0, 30.0, -4.0, 29.0]])          # the second box reaches beyond the image on every side
        return (lambda img, bx, dout: (ops.grid_crop_fwd(img, bx, (32, 32)), ops.grid_crop_bwd(dout, bx, (2, 3, 24, 24)))), \
            (rn(g, 2, 3, 24, 24), boxes, rn(g, 2, 3, 32, 32))
    entry('grid_crop fwd bwd 2x3x24x24 -> 32x32')(make_crop)

    def make_head():
        ops = _ops()
        g = gen(3, 5, 7, 4)
        ins = (rn(g, 3, 5, 7, 4), rn(g, 3, 3, 5, 7), rn(g, 3, 1, 5, 7))

        def fn(z, dr, ds):
            fence_amax_slots()
            t, rgbs, segm = ops.head_fwd(z)
            dz = ops.head_bwd(t, dr, ds, amax=True)
            return t, rgbs, segm, ops.head_fwd(z, want_t=False), dz, slots_of(dz), ops.head_bwd(t, dr, None)
        return fn, ins
    entry('head fwd bwd 3x5x7')(make_head)

    for cz in (3, 4):
        def make(cz=cz):
            ops = _ops()
            g = gen(3, 5, 7, cz, 1)
            ins = (rn(g, 3, 5, 7, cz), rn(g, 3, 3, 5, 7))

            def fn(z, dr):
                fence_amax_slots()
                t, rgbs = ops.tanh_head_fwd(z)
                dz = ops.tanh_head_bwd(t, dr, amax=True)
                return t, rgbs, ops.tanh_head_fwd(z, want_t=False), dz, slots_of(dz), ops.tanh_head_bwd(t, dr)
            return fn, ins
        entry(f'tanh_head fwd bwd 3x5x7 Cz{cz}')(make)

    def make_sum():
        ops = _ops()
        g = gen(3, 10, 14, 8)

        def fn(x):
            fence_amax_slots()
            assert ops.planes_direct_ok(0, x, x.shape[3]) and ops.planes_direct_ok(1, x, x.shape[3])          # lp_sum2x2_planes runs for bf16 / bf16x3
            s = ops.sum2x2(x, amax=True)
            return s, slots_of(s), ops.sum2x2(x), [ops.sum2x2_planes(x, p) for p in (0, 1, 2)]
        return fn, (rn(g, 3, 10, 14, 8),)
    entry('sum2x2 and planes 3x10x14x8')(make_sum)

    def make_pool():
        ops = _ops()
        g = gen(3, 10, 14, 8, 2)
        ins = (rn(g, 3, 10, 14, 8), rn(g, 3, 5, 7, 8), rn(g, 3, 10, 14, 12))

        def fn(x, dy, x12):
            fence_amax_slots()
            r = {'fwd': [ops.avgpool2_fwd(x, ri, None, ro) for ri in (False, True) for ro in (False, True)],
                 'fwd_planes': [ops.avgpool2_fwd(x, True, p, True) for p in (0, 1, 2)], 'fwd_c12': ops.avgpool2_fwd(x12, True, 2)}
            x16 = ops.act_pack(x, pro=2, prec=2)
            xb16 = ops.act_pack(x, pro=2, prec=0)
            r['fwd16'] = (x16, ops.avgpool2_fwd16(x16, 2), xb16, ops.avgpool2_fwd16(xb16, 0))
            y = r['fwd'][3]
            dx = ops.avgpool2_bwd(dy, x, True, amax=True)
            r['bwd'] = (dx, slots_of(dx), ops.avgpool2_bwd(dy, None, False), ops.avgpool2_bwd(dy, None, False, y_relu=y))
            dm = ops.avgpool2_bwd_m16(dy, x16, amax=True)
            r['bwd_m16'] = (dm, slots_of(dm), ops.avgpool2_bwd_m16(dy, xb16))
            return r
        return fn, ins
    entry('avgpool2 fwd fwd16 bwd bwd_m16 3x10x14x8')(make_pool)

    for prec, pname in PRECS:
        for masked in (False, True):
            def make(prec=prec, masked=masked):
                ops = _ops()
                g = gen(3, 5, 7, 8, prec, masked)
                ins = (rn(g, 3, 5, 7, 8), rn(g, 3, 5, 7, 8))

                def fn(dy, ym):
                    m = ym if masked else None
                    return ops.pool_grad_pack(dy, m, prec, True, True, True), ops.pool_grad_pack(dy, m, prec, False, True, False), \
                        ops.pool_grad_pack(dy, m, prec, False, False, True)
                return fn, ins
            entry(f'pool_grad_pack 3x5x7x8 masked={int(masked)} {pname}')(make)

    def make_relu():
        ops = _ops()
        g = gen(3, 5, 7, 12)
        return (lambda dA, x: ops.relu_bwd(dA, x)), (rn(g, 3, 5, 7, 12), rn(g, 3, 5, 7, 12))
    entry('relu_bwd 1260')(make_relu)

    def make_l1():
        ops = _ops()
        shape = (3, 5, 7, 24)          # 2520 elements: no multiple of 256
        g = gen(*shape, 11)
        ins = (rn(g, *shape), rn(g, *shape), rn(g, *shape), torch.tensor(0.7))

        def fn(a, b, add, go):
            fence_amax_slots()
            r = {'l1': [ops.l1_sum(a, b, ri, 0.5) for ri in (False, True)], 'l1_sign': ops.l1_sum(a, b, True, 0.5, want_sign=True)}
            for prec in (0, 2):
                ta, tb = ops.Tap16(ops.act_pack(a, pro=2, prec=prec), prec), ops.Tap16(ops.act_pack(b, pro=2, prec=prec), prec)
                r[f'b16_{prec}'] = (tb, ops.l1_sum(a, tb, True, 0.5), ops.l1_sum(a, tb, True, 0.5, want_sign=True))
                r[f'ab16_{prec}'] = (ta, ops.l1_sum16(ta, tb, 0.5), ops.l1_sum16(ta, tb, 0.5, want_sign=True))
            sgn = r['l1_sign'][1]
            da = ops.l1_bwd(a, b, go, 0.5, True, add=add, amax=True)
            r['bwd'] = (da, slots_of(da), ops.l1_bwd(a, b, go, 0.5, False), ops.l1_bwd(None, None, go, 0.5, True, add=add, sign=sgn, shape=a.shape),
                        ops.l1_bwd(None, None, go, 0.5, True, sign=sgn, shape=a.shape))
            return r
        return fn, ins
    entry('l1 fwd b16 ab16 bwd 2520 elements')(make_l1)

    for (n, h, w, c) in [(3, 2, 5, 40), (1, 1, 1, 300)]:
        for with_embed in (False, True):
            def make(n=n, h=h, w=w, c=c, with_embed=with_embed):
                ops = _ops()
                g = gen(n, h, w, c, with_embed)
                ins = (rn(g, n, h, w, c), rn(g, n, c) if with_embed else None, rn(g, n, c), rn(g, n))

                def fn(out, embed, gp, gd):
                    pooled, dot = ops.proj_score_fwd(out, embed)
                    r = [pooled, dot, ops.proj_score_bwd(out, embed, pooled, gp, gd if with_embed else None, True, with_embed)]
                    if with_embed:
                        r.append(ops.proj_score_bwd(out, embed, pooled, None, gd, True, True))
                    return r
                return fn, ins
            entry(f'proj_score fwd bwd {n}x{h}x{w}x{c} embed={int(with_embed)}')(make)

    for k in (1, 3, 5):
        for c in (40, 72):
            for use_max in (False, True):
                def make(k=k, c=c, use_max=use_max):
                    ops = _ops()
                    b, h, w = 2, 3, 5
                    g = gen(b, k, h, w, c, use_max)
                    ins = (rn(g, b * k, h, w, c), rn(g, b, k, c), rn(g, b, c))

                    def fn(out, ge, gm):
                        elem, embeds, argk = ops.embed_tail_fwd(out, b, k, use_max)
                        return elem, embeds, argk, ops.embed_tail_bwd(out, ge, gm, argk, b, k, use_max), ops.embed_tail_bwd(out, None, gm, argk, b, k, use_max), \
                            ops.embed_tail_bwd(out, ge, None, argk, b, k, use_max)
                    return fn, ins
                entry(f'embed_tail fwd bwd K{k} C{c} {"max" if use_max else "mean"}')(make)

    def make_prep():
        ops = _ops()
        g = gen(2, 3, 5, 7)
        ins = (torch.rand(2, 3, 5, 7, generator=g) * 2 - 1, torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225]), rn(g, 2, 5, 7, 3))
        return (lambda x, mean, std, gr: (ops.image_prep_fwd(x, mean, std), ops.image_prep_bwd(gr, std))), ins
    entry('image_prep fwd bwd HW 35')(make_prep)


elementwise_entries()


# ---- packers --------------------------------------------------------------------------------------------------------------------------------------------------
def packer_entries():
    for prec, pname in PRECS:
        def make_act(prec=prec):
            ops = _ops()
            shape = (3, 5, 7, 12)          # vector-eligible C whose last group falls back to scalar loads, 4 pad channels
            g = gen(*shape, prec)
            ins = (rn(g, *shape), rn(g, 3, 12), rn(g, 3, 12), rn(g, 1, 9, 11, 70))

            def fn(x, sc, sf, x70):
                r = [ops.act_pack(x, pro=p, scale=sc if p == 1 else sc[0] if p >= 3 else None, shift=sf if p == 1 else sf[0] if p >= 3 else None, prec=prec)
                     for p in range(6)]
                return r, ops.act_pack(x70, pro=2, prec=prec), ops.act_pack(x, prec=prec, grad=True), ops.act_pack(x70 * 1e-3, prec=prec, grad=True)
            return fn, ins
        entry(f'act_pack every prologue, gradient form {pname}')(make_act)

        def make_pw(prec=prec):
            ops = _ops()
            g = gen(70, 12, prec)
            ins = (rn(g, 70, 12, 3, 3), rn(g, 24, 16, 1, 1), rn(g, 4, 64, 3, 3))

            def fn(w3, w1, w4):
                return [ops.pack_weights(w3, m, prec) for m in range(6)], [ops.pack_weights(w1, m, prec) for m in (0, 1)], \
                    ops.pack_weights(w3, 0, prec, small_k=True), [ops.pack_weights(w4, m, prec) for m in range(6)]
            return fn, ins
        entry(f'pack_weights modes 0..5 {pname}')(make_pw)

    for prec in (0, 1, 2):
        def make_pb(prec=prec):
            ops = _ops()
            g = gen(900, prec)
            ins = tuple(rn(g, *s) for s in [(70, 130, 3, 3), (24, 16, 1, 1), (4, 64, 3, 3), (8, 8, 1, 1), (32, 8, 3, 3), (12, 70, 3, 3)])

            def fn(p0, p1, p2, s0, s1, s2):
                pairs = [p0, p1, p2]
                specs = [(s0, 0, False), (s1, 0, True)] + [(w, 0, False) for w in pairs] + [(s2, 2, False)]
                specs += [(w, 1, w.shape[0] <= 32 and w.shape[2] == 3) for w in pairs] + [(s2, 4, False)]
                pb = ops.PackBatch(specs, prec)
                assert pb.npair == 3 and pb.nsingle == 4
                pb.table, pb.ptable = GA.guarded(pb.table), GA.guarded(pb.ptable)          # the descriptor tables the two kernels read: fenced copies
                return pb.update()
            return fn, ins
        entry(f'PackBatch pack_weights_batch pack_weights_pairs {dict(PRECS)[prec]}')(make_pb)

    def make_amax():
        lib = _lib()

        def fn(x):
            out = []
            for numel in (1, 5, 1023):
                part = torch.empty(lib.lp_amax_blocks(), dtype=torch.float32, device=x.device)
                assert lib.lp_amax_partial(x.data_ptr(), numel, part.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
                out.append(part)
            return out
        return fn, (rn(gen(1023), 1023),)
    entry('amax_partial 1, 5, 1023 elements')(make_amax)


packer_entries()


# ---- spectral norm --------------------------------------------------------------------------------------------------------------------------------------------
def sn_entries():
    for rows, cols in [(7, 8 * 9), (40, 130)]:
        def make(rows=rows, cols=cols):
            ops = _ops()
            g = gen(rows, cols)
            ins = (rn(g, rows, cols), rn(g, rows, cols), rn(g, rows), rn(g, cols), torch.tensor([1.7, 1 / 1.7]), rn(g, rows, cols))

            def fn(gr, w, u, v, sig, accum):
                g2 = gr.clone()
                return ops.sn_grad_apply(g2, w, u, v, sig), (ops.sn_grad_apply(gr, w, u, v, sig, accum=accum), accum, gr)
            return fn, ins
        entry(f'sn_grad_apply in place and into accum {rows}x{cols}')(make)


    for prec, pname in PRECS:          # lp_sn_grad_apply_batch: the deferred rule of three weight gradients, run when the deferral ends
        def make_batch(prec=prec):
            ops = _ops()
            g = gen(31, prec)
            ins = (rn(g, 2, 8, 16, 64), rn(g, 2, 8, 16, 64), rn(g, 64, 64, 3, 3), rn(g, 64), rn(g, 64 * 9), torch.tensor([1.7, 1 / 1.7]), rn(g, 64, 64, 3, 3),
                   rn(g, 64, 64, 1, 1), rn(g, 64, 64, 1, 1), rn(g, 2, 4, 8, 64), rn(g, 64, 64, 3, 3))

            def fn(x, dy, w3, u, v, sig, acc3, w1, acc1, xlo, accu):
                a, d = ops.act_pack(x, pro=2, prec=prec), ops.act_pack(dy, pro=0, prec=prec, grad=True)
                ops.sn_defer_begin()
                try:
                    r3 = ops.conv_wgrad16(a, d, ksize=3, prec=prec, sn=(w3, u, v, sig), accum=acc3)
                    r1 = ops.conv_wgrad16(a, d, ksize=1, prec=prec, sn=(w1, u, v[:64], sig), accum=acc1)
                    ru = ops.conv_wgrad16(ops.act_pack(xlo, pro=2, prec=prec), d, ksize=3, upsample=True, prec=prec, sn=(w3, u, v, sig), accum=accu)
                finally:
                    ops.sn_defer_end()
                assert r3 is None and r1 is None and ru is None
                return acc3, acc1, accu
            return fn, ins
        entry(f'sn_grad_apply_batch three deferred jobs (3x3, 1x1, upsampled 3x3) {pname}')(make_batch)

    for do_iter in (0, 1):
        def make_pi(do_iter=do_iter):
            import struct
            lib = _lib()
            rb = lib.lp_sn_row_block()
            shapes = [(max(1, rb - 3), 72), (2 * rb + 5, 100)]          # rows < lp_sn_row_block(); cols no multiple of 64
            g = gen(rb, do_iter)
            ins = tuple(t for r, c in shapes for t in (rn(g, r, c), torch.nn.functional.normalize(rn(g, r), dim=0), torch.nn.functional.normalize(rn(g, c), dim=0)))

            def fn(*t):
                assert lib.lp_sn_desc_bytes() == 72
                blob, outs = bytearray(), []
                for i, (r, c) in enumerate(shapes):
                    w, u, v = t[3 * i:3 * i + 3]
                    ui, vi, si = torch.empty(r, device=w.device), torch.empty(c, device=w.device), torch.empty(2, device=w.device)
                    part = torch.empty(((r + rb - 1) // rb) * c + r + (c + 63) // 64, device=w.device)
                    blob += struct.pack('<QQQQQQQiifi', w.data_ptr(), u.data_ptr(), v.data_ptr(), ui.data_ptr(), vi.data_ptr(), si.data_ptr(),
                                        part.data_ptr(), r, c, 1e-12, 0)
                    outs.append((u, v, ui, vi, si, part))
                table = torch.frombuffer(blob, dtype=torch.uint8).clone().to(t[0].device)
                rc = lib.lp_sn_power_iter(table.data_ptr(), len(shapes), do_iter, max(r for r, _ in shapes), max(c for _, c in shapes),
                                          torch.cuda.current_stream().cuda_stream)
                assert rc == 0, lib.lp_last_error()
                return [o[:5] for o in outs]          # (the scratch `part` is no output)
            return fn, ins
        entry(f'sn_power_iter two layers do_iter={do_iter}')(make_pi)

    for kind in (0, 1):
        def make_opt(kind=kind):
            from latent_pose_reenactment_amd import optim
            lib = _lib()
            g = gen(1025, kind)
            sizes = (1, 255, 1025)
            ins = tuple(rn(g, n, scale=s) for n in sizes for s in (1.0, 0.1, 0.01)) + tuple(torch.rand(n, generator=g) * 1e-3 for n in sizes) + \
                (torch.tensor([3], dtype=torch.int64),)

            def fn(*t):
                p, gr, m = t[0:9:3], t[1:9:3], t[2:9:3]
                v, step = t[9:12], t[12]
                table, max_n = optim._build_table(list(zip(p, gr, m, v)), step.device)
                st = torch.cuda.current_stream().cuda_stream
                for _ in range(2):
                    assert lib.lp_mt_optimizer_step(table.data_ptr(), 3, max_n, step.data_ptr(), kind, 1e-3, 0.9, 0.999, 1e-8, st) == 0, lib.lp_last_error()
                return p, gr, m, v, step
            return fn, ins
        entry(f'mt_optimizer_step kind {kind}, 1 / 255 / 1025 elements')(make_opt)

    def make_embed():
        lib = _lib()
        g = gen(7, 8, 3, 1)
        ins = (rn(g, 7, 8), rn(g, 7), rn(g, 8), torch.tensor([0.3]), torch.tensor([3, 1], dtype=torch.int64), rn(g, 2, 8))

        def fn(grad, u, v, coef, label, rows):
            rc = lib.lp_sn_embed_grad(grad.data_ptr(), u.data_ptr(), v.data_ptr(), coef.data_ptr(), label.data_ptr(), rows.data_ptr(), 7, 8, 2,
                                      torch.cuda.current_stream().cuda_stream)
            assert rc == 0, lib.lp_last_error()
            return grad
        return fn, ins
    entry('sn_embed_grad 7x8 labels [3, 1]')(make_embed)

    def make_ema():
        from latent_pose_reenactment_amd import optim
        lib = _lib()
        g = gen(1025, 7)
        ins = tuple(rn(g, n) for n in (1, 255, 1025) for _ in range(2))

        def fn(*t):
            avg, cur = t[0::2], t[1::2]
            table, max_n = optim._build_table([(a, c, None, None) for a, c in zip(avg, cur)], t[0].device)
            st = torch.cuda.current_stream().cuda_stream
            assert lib.lp_mt_ema(table.data_ptr(), 3, max_n, 0.25, 0, st) == 0, lib.lp_last_error()
            blended = [a.clone() for a in avg]
            assert lib.lp_mt_ema(table.data_ptr(), 3, max_n, 0.0, 1, st) == 0, lib.lp_last_error()
            return blended, avg, cur
        return fn, ins
    entry('mt_ema blend and copy, 1 / 255 / 1025 elements')(make_ema)


sn_entries()


# ---- losses behind autograd Functions, the two-source first layer ---------------------------------------------------------------------------------------------
def loss_and_stem8_entries():
    for cf in (1, 3):
        def make(cf=cf):
            from latent_pose_reenactment_amd.criterions.dice import DiceFn
            g = gen(2, cf, 9, 7)
            ins = (torch.rand(2, cf, 9, 7, generator=g), torch.rand(2, 3, 9, 7, generator=g), torch.tensor(0.7))

            def fn(fake, real, go):
                fake.requires_grad_(True)
                loss = DiceFn.apply(fake, real, 2.0)
                loss.backward(go)
                return loss.detach(), fake.grad
            return fn, ins
        entry(f'dice fwd bwd Cf {cf} Cr 3')(make)

    def make_rows():
        from latent_pose_reenactment_amd.embedders.mobilenet_hip import LinearRowsFunction
        g = gen(5, 72, 24)
        ins = (rn(g, 5, 72), rn(g, 24, 72, scale=0.1), rn(g, 24), rn(g, 5, 24))

        def fn(x, w, b, dy):
            for t in (x, w, b):
                t.requires_grad_(True)
            y = LinearRowsFunction.apply(x, w, b)
            y.backward(dy)
            return y.detach(), x.grad, w.grad, b.grad
        return fn, ins
    entry('LinearRowsFunction fwd bwd 5 rows (padded to 8) 72->24')(make_rows)

    for b in (1, 65):
        def make(b=b):
            from latent_pose_reenactment_amd.criterions.adversarial import HingeDFn, HingeGFn
            g = gen(b, 17)
            ins = (rn(g, b, 1), rn(g, b, 1), rn(g, b, 1), torch.tensor(0.7))

            def fn(real, fd, fg, go):
                for t in (real, fd, fg):
                    t.requires_grad_(True)
                ld, lg = HingeDFn.apply(real, fd), HingeGFn.apply(fg)
                ld.backward(go)
                lg.backward(go)
                return ld.detach(), lg.detach(), real.grad, fd.grad, fg.grad
            return fn, ins
        entry(f'hinge fwd bwd B {b}')(make)

    for case in [(2, 7, 16, 3, 4, 64), (1, 13, 32, 3, 3, 64)]:
        for ks in (3, 1):
            for prec, pname in PRECS:
                def make(case=case, ks=ks, prec=prec):
                    ops = _ops()
                    n, h, w, cs, cr, cout = case
                    cin = cs + cr
                    g = gen(*case, ks, prec)
                    od = [(0, c) for c in range(cs)] + [(1, c) for c in range(cr)]
                    # both sources are NCHW VIEWS of NHWC tensors (strided, read in place)
                    ins = (rn(g, n, h, w, cs).permute(0, 3, 1, 2), rn(g, n, h, w, cr).permute(0, 3, 1, 2), rn(g, cout, cin, ks, ks, scale=0.3), rn(g, cout),
                           torch.tensor([0.73]), rn(g, n, h, w, cout))

                    def fn(xa, xb, wgt, bias, alpha, dy):
                        assert ops.stem8_supported(cin, cout, ks, w) and not xa.is_contiguous()
                        pack = ops.pack_weights(wgt, 0, prec, small_k=(ks == 3))
                        cmap = ops.stem8_cmap(od)
                        kw = dict(ksize=ks, cin=cin, bias=bias, alpha=alpha, prec=prec)
                        return {'pack': pack, 'y': ops.stem8_conv(xa, xb, cmap, pack, **kw), 'y_planes': ops.stem8_conv(xa, xb, cmap, pack, out16=1, **kw),
                                'planes_only': ops.stem8_conv(xa, xb, cmap, pack, out16=0, want_y=False, **kw),
                                'wgrad': ops.stem8_wgrad(xa, xb, cmap, dy, ksize=ks, cin=cin, bias_grad=True),
                                'dgrad': ops.stem8_dgrad(dy, wgt, alpha, cmap, cr, ksize=ks)}
                    return fn, ins
                entry(f'stem8 fwd wgrad dgrad {"x".join(map(str, case))} k{ks} strided sources {pname}')(make)


loss_and_stem8_entries()


# ---- image path: strided views whose last row ends exactly at the end of the fenced allocation ------------------------------------------------------------
def frames_case(pad=False):
    """(one decoded 22 x 22 RGB frame, output size, table): an image + mask + product row resampled by area and an image row resampled cubically; ``pad``:
    one image row whose box leaves the frame at the top and on the left"""
    from latent_pose_reenactment_amd import frames
    g = gen(22, 22, 3, pad)
    frame = torch.randint(0, 256, (22, 22, 3), generator=g, dtype=torch.uint8)
    size = 8
    if pad:
        rows = [frames.make_row(image=frames.frame_rows(0, (22, 22, 3), (-0.2, -0.2, 0.6, 0.6), size), image_slot=0)]
    else:
        wide, narrow = (0.1, 0.1, 0.9, 0.9), (0.4, 0.4, 0.6, 0.6)
        rows = [frames.make_row(image=frames.frame_rows(0, (22, 22, 3), wide, size), mask=frames.frame_rows(0, (22, 22, 3), wide, size, channel=1),
                                image_slot=0, mask_slot=0, product_slot=0),
                frames.make_row(image=frames.frame_rows(0, (22, 22, 3), narrow, size), image_slot=1)]
        assert [r[9] for r in rows] == [frames.MODE_AREA, frames.MODE_CUBIC]
    return frame, size, torch.tensor(rows, dtype=torch.int64)


def image_entries():
    for (h, w) in [(11, 11), (13, 19)]:
        def make(h=h, w=w):
            ops = _ops()
            g = gen(h, w, 6)
            x = torch.rand(2, 2, 3, h, w, generator=g)[:, 1]                    # the LAST frame of each sample: the view ends where the allocation ends
            y = torch.rand(2, 3, 3, h, w, generator=g)[:, 2]
            mask = torch.rand(2, 1, w, generator=g).expand(2, h, w)             # an expanded mask: row stride 0
            return (lambda x, y, mask: (ops.image_quality(x, y, mask), ops.image_quality(x, y))), (x, y, mask)
        entry(f'image_quality {h}x{w} views, expanded mask')(make)

    def make_aug():
        import augment_restatement as AR
        ops = _ops()
        b, c, h, w = 3, 3, 17, 19
        g = gen(b, c, h, w, 8)
        rows = AR.family_rows(h, w)
        params = torch.from_numpy(np.stack([rows['neutral'][0], rows['all_together'][0], rows['int_shift'][1]])).float()
        pose = torch.rand(b, 2, c, h, w, generator=g)[:, 1]
        target = torch.rand(b, 2, c, h, w, generator=g)[:, 1]
        segm = torch.rand(b, 1, h, w, generator=g).expand(b, 3, h, w)
        return (lambda pose, params, target, segm: (ops.augment_triplet(pose, params, target, segm), ops.augment_triplet(pose, params))), \
            (pose, params, target, segm)
    entry('augment_triplet 3x3x17x19 views, one neutral row')(make_aug)

    def make_extra():
        import augment_extra_restatement as XR
        ops = _ops()
        b, h, w = 3, 17, 19
        g = gen(b, h, w, 9)
        params = torch.from_numpy(np.stack([XR.row(), XR.row(alpha=2.0, seed=77, median=1, d=0.2, quality=40), XR.row(alpha=1.0, seed=5)])).float()
        pose = torch.rand(b, 2, 3, h, w, generator=g)[:, 1]
        return (lambda pose, params: ops.augment_extra(pose, params)), (pose, params)
    entry('augment_extra 3x3x17x19 view, one neutral row')(make_extra)

    def make_frames():
        ops = _ops()
        from latent_pose_reenactment_amd import frames
        frame, size, table = frames_case()
        counts = frames.check_table(table, frame.numel(), size)

        def fn(buf, table_dev):
            """through the wrapper, and through the C ABI with the DEVICE copy of the table a fenced input (the wrapper makes its own copy)"""
            outs = [torch.empty((c, 3, size, size), dtype=torch.float32, device=buf.device) if c else None for c in counts]
            p = lambda t: None if t is None else t.data_ptr()
            rc = _lib().lp_frames_prepare(buf.data_ptr(), buf.numel(), table.data_ptr(), table_dev.data_ptr(), table.shape[0], size, p(outs[0]), counts[0],
                                          p(outs[1]), counts[1], p(outs[2]), counts[2], torch.cuda.current_stream().cuda_stream)
            assert rc == 0, _lib().lp_last_error()
            return ops.frames_prepare(buf, table, size), outs
        return fn, (frame.reshape(-1), table)
    entry('frames_prepare one area row, one cubic row')(make_frames)

    def make_pad():
        from latent_pose_reenactment_amd import frames
        ops = _ops()
        frame, size, table = frames_case(pad=True)
        nbytes = frame.numel()
        _, plan, weights, total = frames.pad_plan(table, nbytes, size)
        assert plan.shape[0] == 1 and plan[0, 10] > 0 and plan[0, 11] > 0 and plan[0, 12] == 0 and plan[0, 13] == 0          # pads on two sides
        buf = torch.zeros(total, dtype=torch.uint8)
        buf[:nbytes] = frame.reshape(-1)

        def fn(buf, buf2, plan_dev, weights_dev):
            """through the wrapper on ``buf``, and through the C ABI on ``buf2`` with the DEVICE copies of plan and weights fenced inputs"""
            head = buf[:nbytes].clone()
            out = ops.frames_pad(buf, nbytes, plan, weights)
            hist = torch.empty(768, dtype=torch.int32, device=buf.device)
            median = torch.empty(3, dtype=torch.float32, device=buf.device)
            rc = _lib().lp_frames_pad(buf2.data_ptr(), buf2.numel(), nbytes, plan.data_ptr(), plan_dev.data_ptr(), 1, weights_dev.data_ptr(), hist.data_ptr(),
                                      median.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, _lib().lp_last_error()
            assert out is buf and torch.equal(buf[:nbytes], head) and torch.equal(buf2[:nbytes], head), 'only the workspace image may change'
            return buf, buf2
        return fn, (buf, buf.clone(), plan, weights)
    entry('frames_pad one plan, pads on two sides')(make_pad)

    def make_sheet():
        ops = _ops()
        n, h, w = 2, 9, 13
        g = gen(n, h, w, 10)
        rgb = torch.rand(n, 2, 3, h, w, generator=g)[:, 1]
        grey = torch.rand(n, 1, 1, w, generator=g).expand(n, 1, h, w)
        cap = torch.randint(0, 256, (5, 2 * w), generator=g, dtype=torch.uint8)
        return (lambda rgb, grey, cap: (ops.visual_sheet([rgb, grey], cap), ops.visual_sheet([grey]))), (rgb, grey, cap)
    entry('visual_sheet 1-channel expanded panel, caption')(make_sheet)

    def make_stick():
        ops = _ops()
        g = gen(2, 68, 40)
        pts = torch.rand(2, 68, 2, generator=g) * 1.2 - 0.1          # some points outside the frame
        return (lambda pts: (ops.stickman_render(pts, 40), ops.stickman_render(pts, 19, width=2.5))), (pts,)
    entry('stickman_render 2 x 68 points, 40 and 19 pixels')(make_stick)

    def make_jpeg():
        import jpeg_restatement as JR
        from latent_pose_reenactment_amd.utils import mjpeg
        ops = _ops()
        h, w = 9, 17          # the last MCU row and column are partial
        wide = torch.from_numpy(JR.image('smooth_noise', h, w + 5, seed=3, t=2))
        frames = wide[:, :, 5:, :]                                       # a strided view whose last row ends the allocation
        header = mjpeg.jpeg_header(h, w, 75)

        def fn(frames):
            coefs = ops.jpeg_transform(frames, 75)
            return coefs, ops.jpeg_entropy(coefs, header)
        return fn, (frames,)
    entry('jpeg transform entropy_size entropy_write 2x9x17 view')(make_jpeg)


image_entries()


@pytest.mark.parametrize('make,opts', ENTRIES)
def test_no_result_depends_on_fresh_memory(make, opts):
    fn, inputs = make()
    try:
        differential(fn, inputs, device='cuda', **opts)
    finally:
        restore_amax_slots()


def test_the_fence_reaches_the_wrappers_buffers():
    """an output, a split-K workspace and a plane of one conv call were all served by the harness (and so were the pack and the input planes)"""
    ops = _ops()
    g = gen(1)
    x, wt = rn(g, 8, 4, 4, 64).cuda(), rn(g, 64, 64, 3, 3, scale=1 / 24).cuda()
    assert _lib().lp_conv16_fwd_workspace_bytes(8, 4, 4, 64, 3) > 0
    with GA.Guarded('A') as ctx:
        a = ops.act_pack(GA.guarded(x), pro=0, prec=1)
        pk = ops.pack_weights(GA.guarded(wt), 0, 1)
        before = len(ctx.records)
        y, o16 = ops.conv16(a, pk, ksize=3, prec=1, out16=0)
        torch.cuda.synchronize()
        new = ctx.records[before:]
        for t in (y, o16.hi, o16.lo, a.hi, a.lo, pk.hi, pk.lo):
            rec = ctx.served(t)
            assert rec is not None and 'hipops.py' in rec.where, t.shape
        ws = [r for r in new if r.kind == 'torch.empty' and r.dtype == torch.float32 and len(r.shape) == 1]
        assert len(ws) == 1 and ws[0].nbytes == _lib().lp_conv16_fwd_workspace_bytes(8, 4, 4, 64, 3) and 'hipops.py' in ws[0].where
        assert len(new) == 4 and not torch.isnan(y).any()
        ctx.check_guards()
