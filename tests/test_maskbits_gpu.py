"""The one-bit ReLU pattern of the identity encoder's residual junctions (LP_E_MASKBITS) on the GPU.  Every comparison is bit for bit: the route
changes where a predicate is evaluated and which bytes are read, never a value.
  forward   lp_bn_add_act*_bits: planes and fp32 output as without the bits; bits = the NumPy rule (maskbits_ref) on the returned HI plane
  backward  lp_bn_bwd16_h mask mode 4 (bits) against mode 3 (the plane the bits were made from); lp_bn_bwd16_dual against two single calls;
            lp_conv16_fwd_gated (res = d_out under the bits) against res = the masked fp32 copy of d_out
  encoder   resnext50_32x4d, LP_E_MASKBITS on against off: logits and every parameter gradient"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'latent_pose_reenactment_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
pytestmark = pytest.mark.gpu

import maskbits_ref as MB  # noqa: E402
from guarded_alloc import differential  # noqa: E402

NAN = float('nan')


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def words(t):
    """a tensor's elements as integer words on the host (NaN payloads and the sign of zero count)"""
    t = t.detach().contiguous().cpu()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(words(a), words(b)), f'{what}: {int((words(a) != words(b)).sum())} of {a.numel()} words differ'


def same_act(a, b, what):
    same(a.hi, b.hi, what + '.hi'); same(a.lo, b.lo, what + '.lo'); same(a.inv, b.inv, what + '.inv')
    assert a.c == b.c


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------------
def _specials(prec):
    """what the pattern must get right: exact zeros of both signs, a positive value below half of the smallest subnormal of the plane (fp16 2^-24,
    bf16 2^-133: rounds to zero in the plane, bit 0 although v > 0), the smallest fp32 subnormal, NaN (relu'd away, or a NaN plane word)"""
    tiny = 2.0 ** -26 if prec == 2 else 2.0 ** -135
    return torch.tensor([0.0, -0.0, tiny, tiny * 0.5, 2.0 ** -149, NAN, -tiny, 1.0, -1.0], dtype=torch.float32)


def _forward_case(form, prec, p, c, seed):
    """-> (fn(want_bits), inputs): block-output inputs whose pre-activation v = y * scale + shift + r hits the special values exactly: on the even
    channels scale = 1 and shift = -0, and at the chosen positions one of (y, r) is the special value and the other -0 (x + -0 = x for every x)"""
    ops = _ops()
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(p, c, generator=g)
    r = torch.randn(p, c, generator=g)
    sc = torch.rand(c, generator=g) + 0.5
    sh = torch.randn(c, generator=g) * 0.3
    sc[0::2] = 1.0; sh[0::2] = -0.0
    sp = _specials(prec)
    pick = torch.rand(p, c // 2, generator=g) < 0.4
    val = sp[torch.randint(0, len(sp), (p, c // 2), generator=g)]
    ye, re_ = y[:, 0::2], r[:, 0::2]                      # (views)
    in_r = form in ('y16',)                               # a 16-bit y cannot hold the tiny values: they come in through the fp32 residual
    ye[pick] = -0.0 if in_r else val[pick]
    re_[pick] = val[pick] if in_r else -0.0
    if form == 'y16':
        yin = y.to(torch.float16).view(torch.int16)

        def fn(y16, sc, sh, r, want_bits):
            return ops.bn_add_act(ops.Act16(y16, None, c, None), sc, sh, r, relu=True, prec=2, **({'want_bits': True} if want_bits else {}))
        return fn, (yin, sc, sh, r)
    if form == 'res16':
        rh = r.to(torch.bfloat16)
        rl = (r - rh.float()).to(torch.bfloat16) if prec == 1 else None
        rl = None if rl is None else torch.where(torch.isnan(rl), torch.zeros_like(rl), rl)

        def fn(y, sc, sh, rhi, rlo, want_bits):
            return ops.bn_add_act(y, sc, sh, ops.Act16(rhi, rlo, c, None), relu=True, prec=prec, want_out=(seed % 2 == 0),
                                  **({'want_bits': True} if want_bits else {}))
        return fn, (y, sc, sh, rh.view(torch.int16), None if rl is None else rl.view(torch.int16))
    if form == 'down':          # the residual through its own per-channel affine (a downsample block), no ReLU: NaNs reach the plane
        rsc = torch.ones(c); rsh = torch.full((c,), -0.0)
        rsc[1::2] = torch.rand(c // 2, generator=g) + 0.5

        def fn(y, sc, sh, r, rsc, rsh, want_bits):
            return ops.bn_add_act(y, sc, sh, r, rsc, rsh, relu=False, prec=prec, **({'want_bits': True} if want_bits else {}))
        return fn, (y, sc, sh, r, rsc, rsh)

    def fn(y, sc, sh, r, want_bits):
        return ops.bn_add_act(y, sc, sh, r, relu=True, prec=prec, **({'want_bits': True} if want_bits else {}))
    return fn, (y, sc, sh, r)


FORMS = [('f32', 0), ('f32', 1), ('f32', 2), ('down', 0), ('down', 1), ('down', 2), ('y16', 2), ('res16', 0), ('res16', 1)]


@pytest.mark.parametrize('form,prec', FORMS, ids=[f'{f}-{p}' for f, p in FORMS])
def test_forward_bits_follow_the_stored_hi_plane(form, prec):
    for c in (8, 24, 64):
        for p in (1, 37, 300):
            fn, inputs = _forward_case(form, prec, p, c, seed=1000 * c + p)
            out0, a0 = differential(lambda *t: fn(*t, want_bits=False), inputs, device='cuda')
            out1, a1, bits = differential(lambda *t: fn(*t, want_bits=True), inputs, device='cuda')
            tag = f'{form} prec {prec} P={p} C={c}'
            same(out0, out1, tag + ' out'); same_act(a0, a1, tag + ' planes')
            assert bits.dtype == torch.uint8 and tuple(bits.shape) == (p, c // 8)
            w = MB.plane_words(a1.hi)
            assert np.array_equal(bits.cpu().numpy(), MB.pack(w)), tag
            # the rule is the plane's, not v > 0: wherever the fp32 output is positive but its plane word is zero the bit is clear
            if out1 is not None:
                o = out1.cpu().numpy()
                lost = (o > 0) & ((w & 0x7fff) == 0)
                assert not (np.unpackbits(bits.cpu().numpy(), axis=-1, bitorder='little').astype(bool) & lost).any(), tag
                if p >= 37 and form in ('f32', 'down') and prec == 2:          # (2^-26 is a normal fp32 number: no denormal handling is involved)
                    assert lost.any(), tag + ': the case holds no positive value that rounds to zero in the plane'


# ---- lp_bn_bwd16_h: mode 4 against mode 3 -------------------------------------------------------------------------------------------------------------
def _bwd_inputs(p, c, x16, seed, n_x=1):
    g = torch.Generator().manual_seed(seed)
    dA = torch.randn(p, c, generator=g) * 1e-2
    dA[torch.rand(p, c, generator=g) < 0.02] = 0.0
    xs, bns = [], []
    for _ in range(n_x):
        x = torch.randn(p, c, generator=g) * 1.5 + 0.3
        xs.append(x.to(torch.float16).view(torch.int16) if x16 else x)
        gamma = torch.rand(c, generator=g) + 0.5
        mean = torch.randn(c, generator=g) * 0.2 + 0.3
        rstd = 1.0 / (torch.rand(c, generator=g) + 0.5)
        bns.append((gamma, mean, rstd, gamma * rstd, torch.randn(c, generator=g) * 0.1))
    # the block output's HI plane: random values with the special words mixed in (any word may stand in a plane: only its pattern is read)
    plane = (torch.randn(p, c, generator=g)).to(torch.bfloat16).view(torch.int16)
    sw = torch.tensor([0, -32768, 1, 0x7fff, -32767, 0x7fc0, -64], dtype=torch.int16)          # +0, -0, 0x0001, 0x7fff, 0x8001, NaN, 0xffc0
    pick = torch.rand(p, c, generator=g) < 0.3
    plane[pick] = sw[torch.randint(0, len(sw), (p, c), generator=g)][pick]
    bits = torch.from_numpy(MB.pack(plane.numpy().view(np.uint16)))
    return dA, xs, bns, plane, bits


BWD_SHAPES = [(p, c) for c in (8, 64, 72) for p in (1, 17, 300)] + [(3, 2056)]      # 300 pixels: 5 splits; 2056 channels: the non-rows apply kernel


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('prec,x16', [(0, False), (1, False), (2, False), (2, True)])
def test_bn_bwd16_mode4_equals_mode3(prec, x16, frozen):
    ops = _ops()
    for p, c in BWD_SHAPES:
        dA, (x,), ((gamma, mean, rstd, scale, shift),), plane, bits = _bwd_inputs(p, c, x16, seed=7 * p + c)
        dev = lambda t: t.cuda()
        xd = ops.Act16(dev(x), None, c, None) if x16 else dev(x)
        args = (dev(dA), xd, dev(gamma), dev(mean), dev(rstd), dev(scale), dev(shift))
        r3 = ops.bn_bwd16(*args, prec=prec, mask_mode=2, mask_src=ops.Act16(dev(plane), None, c, None), frozen=frozen)
        r4 = ops.bn_bwd16(*args, prec=prec, mask_mode=2, mask_src=dev(bits), frozen=frozen)
        tag = f'prec {prec} x16={x16} frozen={frozen} P={p} C={c}'
        same_act(r3[0], r4[0], tag + ' planes'); same(r3[1], r4[1], tag + ' dgamma'); same(r3[2], r4[2], tag + ' dbeta')
        assert r3[3] is None and r4[3] is None
        # g_out stays available with the bits
        g4 = ops.bn_bwd16(*args, prec=prec, mask_mode=2, mask_src=dev(bits), frozen=frozen, want_g=True)[3]
        keep = torch.from_numpy(MB.positive(plane.numpy().view(np.uint16)))
        same(g4.cpu(), torch.where(keep, dA, torch.zeros_like(dA)), tag + ' g')


# ---- the dual form against two single calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec,x16', [(0, False), (1, False), (2, False), (2, True)])
def test_bn_bwd16_dual_equals_two_single_calls(prec, x16):
    ops = _ops()
    for c in (64, 72):
        for p in (17, 300):
            dA, xs, bns, plane, bits = _bwd_inputs(p, c, x16, seed=13 * p + c, n_x=2)

            def wrap(x):
                return ops.Act16(x, None, c, None) if x16 else x

            def dual(dA, xa, xb, bna, bnb, bits):
                return ops.bn_bwd16_dual(dA, wrap(xa), bna[:3], wrap(xb), bnb[:3], prec=prec, mask_src=bits)

            def single(dA, xa, xb, bna, bnb, bits):
                return tuple(ops.bn_bwd16(dA, wrap(x), *bn, prec=prec, mask_mode=2, mask_src=bits)[:3] for x, bn in ((xa, bna), (xb, bnb)))
            inputs = (dA, xs[0], xs[1], bns[0], bns[1], bits)
            rd = differential(dual, inputs, device='cuda')
            rs = differential(single, inputs, device='cuda')
            for k, name in enumerate(('bn a', 'bn b')):
                tag = f'prec {prec} x16={x16} P={p} C={c} {name}'
                same_act(rd[k][0], rs[k][0], tag + ' planes'); same(rd[k][1], rs[k][1], tag + ' dgamma'); same(rd[k][2], rs[k][2], tag + ' dbeta')


def test_bn_bwd16_dual_non_rows_apply_kernel():
    """C = 2056 (257 channel groups): the apply kernel that re-reads its coefficients per item, in its dual form"""
    ops = _ops()
    p, c = 3, 2056
    for prec in (1, 2):
        dA, xs, bns, plane, bits = _bwd_inputs(p, c, False, seed=99, n_x=2)
        d = lambda t: t.cuda()
        bn = [tuple(d(t) for t in b) for b in bns]
        rd = ops.bn_bwd16_dual(d(dA), d(xs[0]), bn[0][:3], d(xs[1]), bn[1][:3], prec=prec, mask_src=d(bits))
        for k in range(2):
            rs = ops.bn_bwd16(d(dA), d(xs[k]), *bn[k], prec=prec, mask_mode=2, mask_src=d(bits))
            same_act(rd[k][0], rs[0], f'prec {prec} bn {k} planes'); same(rd[k][1], rs[1], 'dgamma'); same(rd[k][2], rs[2], 'dbeta')


# ---- the gated residual of the conv epilogue ---------------------------------------------------------------------------------------------------------
GATED = [(16, 8, 64), (16, 8, 200), (64, 64, 64), (64, 64, 200), (128, 72, 64), (128, 72, 200), (2048, 1024, 256)]


@pytest.mark.parametrize('prec', [0, 1, 2])
@pytest.mark.parametrize('cin,cout,p', GATED, ids=[f'{a}to{b}-P{p}' for a, b, p in GATED])
def test_gated_residual_equals_the_masked_fp32_residual(cin, cout, p, prec):
    """1x1 layers on flattened pixels, as the data gradient of a block's first conv runs: y = conv(a) + (bit ? d_out : 0) against y = conv(a) + g with
    g = the masked copy.  d_out holds NaNs under cleared bits: a select drops them, a multiply would not.  (2048 -> 1024 at 256 pixels is a shape
    whose 3x3 sibling runs split-K; a 1x1 conv never does, so it takes the same gated epilogue and must match.)"""
    ops = _ops()
    g = torch.Generator().manual_seed(cin + cout + p)
    h, w = ops.flat_hw(p)
    x = (torch.randn(1, h, w, cin, generator=g) * 1e-2).cuda()
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).cuda()
    d_out = torch.randn(1, h, w, cout, generator=g)
    plane = torch.randn(1, h, w, cout, generator=g).to(torch.bfloat16).view(torch.int16)
    plane[torch.rand(plane.shape, generator=g) < 0.1] = 0
    keep = torch.from_numpy(MB.positive(plane.numpy().view(np.uint16)))
    bits = torch.from_numpy(MB.pack(plane.numpy().view(np.uint16)))
    d_out[(~keep) & (torch.rand(d_out.shape, generator=g) < 0.3)] = NAN
    assert torch.isnan(d_out).any()
    gm = torch.where(keep, d_out, torch.zeros_like(d_out))
    a = ops.act_pack(x, prec=prec, grad=True)
    pack = ops.pack_weights(wt, 0, prec)
    y_ref = ops.conv16(a, pack, ksize=1, res=gm.cuda(), prec=prec)
    y = ops.conv16(a, pack, ksize=1, res=d_out.cuda(), res_bits=bits.cuda(), prec=prec)
    assert torch.isfinite(y_ref).all()
    assert torch.equal(y, y_ref), f'{int((y != y_ref).sum())} of {y.numel()} differ'
    # and with the residual's own bits all set it is the plain residual
    full = torch.full(bits.shape, 255, dtype=torch.uint8)
    same(ops.conv16(a, pack, ksize=1, res=gm.cuda(), res_bits=full.cuda(), prec=prec), y_ref, 'all bits set')


def test_gated_residual_is_refused_where_it_is_not_covered():
    """the gate lives in the 1x1 kernels only: a 3x3 conv with res_bits is an error, not a silently ungated sum"""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 8, 8, 32, generator=g).cuda()
    wt = torch.randn(32, 32, 3, 3, generator=g).cuda()
    a = ops.act_pack(x, prec=1)
    res = torch.randn(1, 8, 8, 32, generator=g).cuda()
    bits = torch.zeros(1, 8, 8, 4, dtype=torch.uint8).cuda()
    with pytest.raises(Exception, match='1x1'):
        ops.conv16(a, ops.pack_weights(wt, 0, 1), ksize=3, res=res, res_bits=bits, prec=1)


# ---- the whole encoder ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['default', 'bf16x3'])
def test_encoder_is_bit_identical_with_and_without_the_bits(case):
    """resnext50_32x4d at the smallest geometry supported() takes (8 frames of 128 x 128), train mode, default operand-mode assignment and the strict
    bf16x3 mode: LP_E_MASKBITS on against off -- logits and every parameter gradient"""
    import rounding_study as RS
    from embedders import resnext_hip
    from test_resnext_hip import _nets, structured_frames
    assert resnext_hip.supported(8, 128, 128) and not resnext_hip.supported(4, 128, 128) and not resnext_hip.supported(8, 96, 96)
    calls = {}

    def run(on):
        with pytest.MonkeyPatch.context() as mp:
            for k in RS.MODE_ENV:          # (the default assignment: nothing set)
                mp.delenv(k, raising=False)
            if case == 'bf16x3':
                mp.setenv('LP_PREC', 'bf16x3')
            for k in ('Y16', 'RES16', 'MASK16'):
                mp.setattr(resnext_hip, k, True)
            mp.setattr(resnext_hip, 'MASKBITS', on)
            ops = resnext_hip.ops
            n = {'dual': 0, 'gated': 0}
            dual, conv16 = ops.bn_bwd16_dual, ops.conv16
            mp.setattr(ops, 'bn_bwd16_dual', lambda *a, **k: (n.__setitem__('dual', n['dual'] + 1), dual(*a, **k))[1])
            mp.setattr(ops, 'conv16', lambda *a, **k: (n.__setitem__('gated', n['gated'] + (k.get('res_bits') is not None)), conv16(*a, **k))[1])
            m, _ = _nets(32, 7)
            m.train()
            y = m(structured_frames(8, 128, 3).cuda())
            (y * RS.loss_weights(8, 32).cuda()).sum().backward()
            calls[on] = n
            return y.detach(), [p.grad for p in m.parameters()]
    y1, g1 = run(True)
    y0, g0 = run(False)
    assert calls[False] == {'dual': 0, 'gated': 0}
    assert calls[True]['gated'] == 12 and calls[True]['dual'] >= (4 if case == 'bf16x3' else 1), calls      # 12 identity blocks, 4 downsample blocks
    assert torch.equal(y1, y0)
    assert all(a is not None for a in g1) and len(g1) == len(g0)
    bad = [i for i, (a, b) in enumerate(zip(g1, g0)) if not torch.equal(a, b)]
    assert not bad, f'{len(bad)} of {len(g1)} parameter gradients differ, first {bad[:5]}'
