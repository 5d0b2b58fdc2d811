"""The 16-bit-resident and planes-only kernels of the fp16 mode against fp64 directly (references: tests/emu_ops.py, proven on the CPU by
tests/test_resident16_refs.py).  Pins lp_adain_act16, lp_adain_relu_bwd16, lp_norm_act_bwd / lp_bn_bwd16(_h) at more than 64 pixel splits
and a channel-group count that does not divide 256, lp_l1_fwd_ab16 + lp_l1_bwd from its sign pattern, lp_avgpool2_bwd_m16, lp_avgpool2_fwd."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
pytestmark = pytest.mark.gpu

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
from guarded_alloc import fence_fixture  # noqa: E402

# every buffer a wrapper takes from torch.empty / empty_like while a test of this module runs is full of NaN-like words (guarded_alloc fill A) and sits
# between two fences that are checked when the test is over; the assertions and tolerances below are what they were
fenced_buffers = fence_fixture()

F16_MAX, BF16_MAX = 0x7bff, 0x7f7f            # largest finite patterns


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def report(name, err, tol, what='rel-L2'):
    print(f'[parity] {name}: {what} {err:.3e} (tol {tol:.0e})')
    assert err < tol, f'{name}: {what} {err:.3e} >= {tol}'


def dtype_of(prec):
    return torch.float16 if prec == 2 else torch.bfloat16


def decode(a, prec):
    """operand planes -> fp64 values (x 1/scale for scaled fp16 gradient operands)"""
    v = a.hi.view(dtype_of(prec)).double()
    if prec == 1:
        v = v + a.lo.view(torch.bfloat16).double()
    if a.inv is not None:
        v = v * a.inv.double()
    return v[..., :a.c]


def set_bits(plane, idx, pattern):
    """plane: int16 tensor; writes the 16-bit pattern (0 .. 0xffff) at flat index idx"""
    plane.view(-1)[idx] = pattern - 0x10000 if pattern >= 0x8000 else pattern


def relu_guard(name, x, scale, shift):
    """the ReLU pattern of kernel and reference can differ only where the kernel's fp32 fma t = x*scale + shift lands on the other side of
    0: excluded if |t| is not tiny against its two terms.  Asserted on the reference side over EVERY element (the seed is chosen for it)."""
    t = x * scale + shift
    margin = (t.abs() / ((x * scale).abs() + shift.abs())).min().item()
    print(f'[parity] {name}: min |t| / (|x*scale| + |shift|) = {margin:.3e} (> 2^-20 = {2.0 ** -20:.3e})')
    assert margin > 2.0 ** -20, margin


# ---- (a) lp_adain_act16 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 3, 5, 8), (2, 4, 4, 24), (3, 8, 8, 72)])
def test_adain_act16(shape):
    """G = C/8 = 1 and 3 are the smallest group counts; N = 3 with a different affine per image and channel shows a wrong image index or
    channel offset.  (1) relu on: bit-equal to lp_act_pack pro 1 on the decoded plane (the kernel's own claim); (2) relu on and off against
    fp64, EVERY element: |got - ref| <= 2^-11 |ref| + 2^-24 + 2^-23 (|y*scale| + |shift|) -- one fp16 rounding (2^-24: its subnormal step)
    plus one fp32 fma."""
    ops = _ops()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(31)
    y = (torch.randn(n, h, w, c, generator=g) * 2).half()
    assert bool((y > 0).any()) and bool((y < 0).any())
    scale, shift = torch.randn(n, c, generator=g).cuda(), torch.randn(n, c, generator=g).cuda()
    y16 = ops.Act16(y.view(torch.int16).cuda(), None, c, None)
    ys = y.double() * scale.double().cpu()[:, None, None, :]
    sh = shift.double().cpu()[:, None, None, :].expand_as(ys)
    for relu in (True, False):
        out = ops.adain_act16(y16, scale, shift, relu=relu)
        torch.cuda.synchronize()
        assert out.lo is None and out.inv is None and out.c == c and out.hi.shape == y16.hi.shape
        if relu:
            want = ops.act_pack(ops.y16_to_f32(y16).contiguous(), pro=1, scale=scale, shift=shift, prec=2)
            assert torch.equal(out.hi, want.hi)
        ref = torch.relu(ys + sh) if relu else ys + sh
        got = out.hi.view(torch.float16).double().cpu()
        bound = 2.0 ** -11 * ref.abs() + 2.0 ** -24 + 2.0 ** -23 * (ys.abs() + sh.abs())
        report(f'adain_act16{shape} relu={relu}', ((got - ref).abs() / bound).max().item(), 1.0, 'worst |err| / bound')


# ---- (b) lp_adain_relu_bwd16 ----------------------------------------------------------------------------------------------------
_ADAIN_SEED = 4                    # (relu_guard holds for all four shapes: checked on the CPU, asserted in the test)


def _adain_case(shape, ups, seed):
    """x as an fp16 plane; statistics in fp64 from the decoded plane (eps 1e-4), rounded to fp32: kernel and reference get the SAME values"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(seed)
    x16 = (torch.randn(n, h, w, c, generator=g) * 2 + 1).half()
    aff = torch.randn(n, 2 * c, generator=g)
    dA = torch.randn(n, h << ups, w << ups, c, generator=g)
    add = torch.randn(n, h, w, c, generator=g)
    x = x16.double()
    gamma, beta = aff[:, c:].double(), aff[:, :c].double()
    mean = x.mean((1, 2)); var = x.var((1, 2), unbiased=False)
    rstd = 1 / torch.sqrt(var + 1e-4)
    scale = gamma * rstd
    st32 = [t.float().contiguous() for t in (mean, rstd, scale, beta - mean * scale)]
    return x16, aff, dA, add, st32


@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('ups', [0, 1])
@pytest.mark.parametrize('shape', [(2, 4, 4, 64), (3, 5, 7, 8), (2, 12, 20, 72), (1, 65, 64, 8)])
def test_adain_relu_bwd16(shape, ups, with_add):
    """x an ``Act16``.  (2,4,4,64): one split; (3,5,7,8): HW = 35 < 64 and C < 64; (2,12,20,72): four splits with a ragged 48-pixel tail and
    a ragged second channel block; (1,65,64,8): S = 65 pixel splits -- the second step of norm_bwd_merge's loop.  Gates: fp64 at 2e-5 (what
    test_hip_ops.test_adain_relu_bwd holds the fp32 instance to: the arithmetic after the load is the same), and bit-equality with the fp32
    entry on the decoded plane."""
    import emu_ops
    ops = _ops()
    n, h, w, c = shape
    x16, aff, dA, add, st32 = _adain_case(shape, ups, _ADAIN_SEED)
    st64 = [t.double() for t in st32]
    gamma64 = aff[:, c:].double()
    relu_guard(f'adain_relu_bwd16{shape}', x16.double(), st64[2][:, None, None, :], st64[3][:, None, None, :])
    rdx, rdg, rdb = emu_ops.adain_relu_bwd(dA.double(), x16.double(), add.double() if with_add else None, gamma64, *st64, bool(ups))
    affc, dAc, addc = aff.cuda(), dA.cuda(), (add.cuda() if with_add else None)
    st = [t.cuda() for t in st32]
    xa = ops.Act16(x16.view(torch.int16).cuda(), None, c, None)
    xf = ops.y16_to_f32(xa).contiguous()
    res = {}
    for name, xin in (('x16', xa), ('fp32', xf)):
        daff = torch.zeros_like(affc)
        dx = ops.adain_relu_bwd(dAc, xin, addc, affc[:, c:], *st, daff[:, c:], daff[:, :c], bool(ups), amax=True)
        torch.cuda.synchronize()
        slots, ver = dx._lp_amax
        res[name] = (dx, daff, slots.clone())
    dx, daff, slots = res['x16']
    tag = f'adain_relu_bwd16{shape} ups={ups} add={int(with_add)}'
    report(f'{tag} dx', rel(dx, rdx), 2e-5)
    report(f'{tag} dgamma', rel(daff[:, c:], rdg), 2e-5)
    report(f'{tag} dbeta', rel(daff[:, :c], rdb), 2e-5)
    top = float(dx.abs().max())
    report(f'{tag} amax slots', abs(float(slots.max()) - top) / top, 1e-6, 'rel. distance to max|dx|')
    for a, b in zip(res['x16'], res['fp32']):
        assert torch.equal(a, b)


# ---- (c) lp_norm_act_bwd / lp_bn_bwd16(_h): 65 pixel splits, 3 channel groups -----------------------------------------------------
_PC_SHAPE = (1, 65, 64, 24)         # P x C = 4160 x 24: S = 65 splits of 64 pixels; G = C/8 = 3 does not divide 256 (rows = 85: thread 255 idles)
_PC_SEED = 16                      # (chosen on the CPU so that relu_guard holds for x as fp32 and as the fp16 plane; 15 does not)


def _pc_case(x16):
    import emu_ops
    g = torch.Generator().manual_seed(_PC_SEED)
    n, h, w, c = _PC_SHAPE
    x = torch.randn(n, h, w, c, generator=g)
    dA = torch.randn(n, h, w, c, generator=g) * 1e-4
    src = torch.randn(n, h, w, c, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    if x16:
        x = x.half()
    stats = emu_ops.bn_train_stats(x.double(), gamma.double(), beta.double(), None, None, 0.1, 1e-5)
    st32 = [t.float().contiguous() for t in stats]
    return x, dA, src, gamma, st32


def _mask_kw(mode, src, prec, ops):
    """-> (kernel kwargs, fp64 mask_src | None).  'src16': the pattern from the operand planes of relu(src), with -0, +0 and the smallest
    subnormal written in by hand; the reference masks by the DECODED plane."""
    if mode == 'relu':
        return dict(mask_mode=0), None
    if mode == 'none':
        return dict(mask_mode=1), None
    if mode == 'src':
        return dict(mask_mode=2, mask_src=src.cuda()), src.double()
    m16 = ops.act_pack(src.cuda(), pro=2, prec=prec)
    for idx, pattern in ((0, 0x8000), (1, 0x0000), (2, 0x0001), (24 * 64 * 64 + 5, 0x8000), (24 * 64 * 64 + 6, 0x0001)):
        set_bits(m16.hi, idx, pattern)
    return dict(mask_mode=2, mask_src=m16), m16.hi.view(dtype_of(prec)).double().cpu()


@pytest.mark.parametrize('mode', ['relu', 'none', 'src'])
def test_norm_act_bwd_65_splits(mode):
    """lp_norm_act_bwd (the fp32 instance of the per-image kernels) where the fp64 merge of the split partials takes its second step"""
    import emu_ops
    ops = _ops()
    x, dA, src, gamma, st32 = _pc_case(False)
    st64 = [t.double() for t in st32]
    if mode == 'relu':
        relu_guard('norm_act_bwd[relu]', x.double(), st64[2], st64[3])
    kw, m64 = _mask_kw(mode, src, None, ops)
    dx, dg, db, gm = ops.norm_act_bwd(dA.cuda(), x.cuda(), gamma.cuda(), *[t.cuda() for t in st32], want_g=True, amax=True, **kw)
    torch.cuda.synchronize()
    rdx, rdg, rdb, rg = emu_ops.norm_act_bwd(dA.double(), x.double(), gamma.double(), *st64, mask_mode=kw['mask_mode'], mask_src=m64, want_g=True)
    report(f'norm_act_bwd[{mode}] S=65 dx', rel(dx, rdx), 2e-5)
    report(f'norm_act_bwd[{mode}] S=65 dgamma', rel(dg, rdg), 2e-5)
    report(f'norm_act_bwd[{mode}] S=65 dbeta', rel(db, rdb), 2e-5)
    report(f'norm_act_bwd[{mode}] S=65 g', rel(gm, rg), 1e-7)
    slots, ver = dx._lp_amax
    top = float(dx.abs().max())
    report(f'norm_act_bwd[{mode}] S=65 amax slots', abs(float(slots.max()) - top) / top, 1e-6, 'rel. distance to max|dx|')


@pytest.mark.parametrize('mode,prec,xform', [pytest.param(mode, prec, xform, id=f'{mode}-{prec}-{xform}')
                                             for prec, xform in ((0, 'f32'), (1, 'f32'), (2, 'f32'), (2, 'x16'))
                                             for mode in ('relu', 'none', 'src', 'src16')])
def test_bn_bwd16_65_splits_3_channel_groups(mode, prec, xform):
    """lp_bn_bwd16 / lp_bn_bwd16_h at P x C = 4160 x 24: the merge loop's second step AND the live `r >= rows` tail of the rows apply kernel
    (G = 3: 256 / 3 = 85 pixel rows, the last thread has none).  Gates as tests/test_resnext_hip.py::test_bn_bwd_straight_to_operand_planes."""
    import emu_ops
    ops = _ops()
    x, dA, src, gamma, st32 = _pc_case(xform == 'x16')
    st64 = [t.double() for t in st32]
    if mode == 'relu':
        relu_guard(f'bn_bwd16[relu] {xform}', x.double(), st64[2], st64[3])
    kw, m64 = _mask_kw(mode, src, prec, ops)
    xin = ops.Act16(x.view(torch.int16).cuda(), None, x.shape[-1], None) if xform == 'x16' else x.cuda()
    d16, dg, db, gm = ops.bn_bwd16(dA.cuda(), xin, gamma.cuda(), *[t.cuda() for t in st32], prec=prec, want_g=True, **kw)
    torch.cuda.synchronize()
    rdx, rdg, rdb, rg = emu_ops.norm_act_bwd(dA.double(), x.double(), gamma.double(), *st64, mask_mode=kw['mask_mode'], mask_src=m64, want_g=True)
    tag = f'bn_bwd16[{mode}] prec{prec} {xform} S=65 G=3'
    report(f'{tag} planes', rel(decode(d16, prec), rdx), {0: 1e-2, 1: 3e-6, 2: 4e-4}[prec])
    assert (d16.lo is None) == (prec != 1)
    report(f'{tag} dgamma', rel(dg, rdg), 2e-5)
    report(f'{tag} dbeta', rel(db, rdb), 2e-5)
    report(f'{tag} g', rel(gm, rg), 1e-7)
    if prec == 2:
        top = d16.hi.view(torch.float16).float().abs().max().item()
        print(f'[parity] {tag}: largest scaled plane element {top:.1f} (window [2^9, 2^13.01))')
        assert 2.0 ** 9 <= top < 2.0 ** 13.01, top


# ---- (d) lp_l1_fwd_ab16 and lp_l1_bwd from its sign pattern -------------------------------------------------------------------------
def _edge_planes(ops, shape, prec, pro, seed):
    """planes of relu?(randn) for a and b (lp_act_pack), then by hand: exact ties, a = +0 and a = -0 against b > 0, the smallest subnormal on
    either side, negative patterns (a ReLU plane never holds them; the mask kernels must still read them as not > 0).  No NaNs.  The
    largest finite value is added by the caller (``_add_largest``)."""
    g = torch.Generator().manual_seed(seed)
    a = ops.act_pack(torch.randn(shape, generator=g).cuda(), pro=pro, prec=prec)
    b = ops.act_pack(torch.randn(shape, generator=g).cuda(), pro=pro, prec=prec)
    one = 0x3c00 if prec == 2 else 0x3f80
    last = a.hi.numel() - 1
    for idx, pa, pb in ((0, one, one), (1, 0x0000, 0x0000), (2, 0x0001, 0x0001),                   # ties
                        (3, 0x0000, one), (4, 0x8000, one), (5, 0x8000, 0x0000),                   # a = +0 / -0
                        (6, 0x0001, 0x0000), (7, 0x0001, one), (8, 0x0000, 0x0001), (9, 0x8000, 0x0001),
                        (last, 0x0001, one), (last - 1, 0x8000, one), (last - 2, one, one)):
        set_bits(a.hi, idx, pa); set_bits(b.hi, idx, pb)
    return a, b


def _add_largest(a, b, prec):
    """the largest finite value: on both sides in fp16; in bf16 (3.4e38) once -- a second one overflows the fp32 SUM the loss term is"""
    one, big = (0x3c00, F16_MAX) if prec == 2 else (0x3f80, BF16_MAX)
    set_bits(a.hi, 10, big); set_bits(b.hi, 10, one)
    if prec == 2:
        set_bits(a.hi, 11, one); set_bits(b.hi, 11, big)
        set_bits(a.hi, 12, big); set_bits(b.hi, 12, big)


@pytest.mark.parametrize('prec', [2, 0])
@pytest.mark.parametrize('shape', [(2, 6, 10, 8), (1, 16, 16, 72)])
def test_l1_between_planes_and_backward_from_its_sign_pattern(shape, prec):
    """lp_l1_fwd_ab16 (l1_partial_kernel<1,1> / <2,2>).  The term is gated twice: without the largest finite value (every element then
    weighs in at the 1e-5 gate) and with it (it dominates the sum; the sign pattern still checks every element exactly)."""
    import emu_ops
    ops = _ops()
    a, b = _edge_planes(ops, shape, prec, 2, 41)
    dt = dtype_of(prec)
    numel = a.hi.numel()
    coef = 1.0 / numel
    for stage in ('edges', 'edges + largest finite'):
        if stage != 'edges':
            _add_largest(a, b, prec)
        av, bv = a.hi.view(dt).double().cpu(), b.hi.view(dt).double().cpu()
        assert not bool(torch.isnan(av).any() | torch.isnan(bv).any())
        ta, tb = ops.Tap16(a, prec), ops.Tap16(b, prec)
        term, sgn = ops.l1_sum16(ta, tb, coef, want_sign=True)
        term0 = ops.l1_sum16(ta, tb, coef)
        torch.cuda.synchronize()
        rterm, rsgn = emu_ops.l1_planes(av, bv)
        assert torch.equal(sgn.cpu(), rsgn)
        assert set(rsgn.tolist()) == {-1, 0, 1}
        report(f'l1_sum16{shape} prec{prec} [{stage}] term', abs(term.item() - rterm.item()) / rterm.item(), 1e-5, 'rel. error')
        assert torch.equal(term, term0)
    g = torch.Generator().manual_seed(43)
    add = torch.randn(shape, generator=g)
    go = torch.tensor(0.37)
    for addc in (None, add.cuda()):
        da = ops.l1_bwd(None, None, go.cuda(), coef, False, add=addc, sign=sgn, shape=shape)
        torch.cuda.synchronize()
        ref = coef * go.double() * rsgn.double().reshape(shape) + (0 if addc is None else add.double())
        report(f'l1_bwd(sign){shape} prec{prec} add={int(addc is not None)}', rel(da, ref), 1e-6)


# ---- (e) lp_avgpool2_bwd_m16 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [2, 0])
@pytest.mark.parametrize('shape', [(3, 6, 10, 8), (1, 2, 2, 64), (2, 4, 4, 72)])
def test_avgpool2_bwd_with_the_mask_from_planes(shape, prec):
    """the kernel never decodes: the same rule on planes read as fp16 (prec 2) and as bf16 (prec 0), with -0, +0, 0x0001, negative values and
    the largest finite value in the mask.  x 0.25 is the only arithmetic: bit-exact against fp64."""
    import emu_ops
    ops = _ops()
    n, h, w, c = shape
    mask, other = _edge_planes(ops, shape, prec, 0, 47)
    _add_largest(mask, other, prec)
    mbits = mask.hi.cpu()
    mv = mbits.view(dtype_of(prec)).double()
    assert not bool(torch.isnan(mv).any()) and bool((mv < 0).any())
    assert torch.equal(emu_ops.plane_positive(mbits), mv > 0)
    g = torch.Generator().manual_seed(49)
    dy = torch.randn(n, h // 2, w // 2, c, generator=g)
    dx = ops.avgpool2_bwd_m16(dy.cuda(), mask, amax=True)
    dx32 = ops.avgpool2_bwd(dy.cuda(), mv.float().cuda(), relu_in=True)
    torch.cuda.synchronize()
    ref = emu_ops.avgpool2_bwd_mask(dy.double(), mv)
    assert ref.float().double().equal(ref)
    nbad = int((dx.cpu() != ref.float()).sum())
    report(f'avgpool2_bwd_m16{shape} prec{prec}', nbad, 0.5, 'elements differing from fp64')
    assert torch.equal(dx, dx32)
    slots, ver = dx._lp_amax
    assert float(slots.max()) == float(dx.abs().max())
    for idx in (1, 3, 4, 5, 8, 9):               # (+0 and -0 pass nothing; 0x0001 at 2, 6, 7 passes)
        assert float(dx.view(-1)[idx]) == 0.0
    for idx in (2, 6, 7):
        assert float(dx.view(-1)[idx]) != 0.0


# ---- (f) lp_avgpool2_fwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out16_prec', [None, 2, 0, 1])
@pytest.mark.parametrize('shape', [(3, 6, 10, 8), (1, 4, 4, 72)])
def test_avgpool2_fwd_relu_flags_and_plane_outputs(shape, out16_prec):
    """relu_in x relu_out x planes.  y against fp64, EVERY element: |got - ref| <= 3 * 2^-24 * 0.25 * sum |a_k| (three fp32 adds over the four
    inputs a_k after relu_in; x 0.25 is exact).  One-plane outputs: the RNE rounding of y itself; prec 1 (two planes) is the wrapper's
    lp_act_pack fallback."""
    import emu_ops
    ops = _ops()
    n, h, w, c = shape
    g = torch.Generator().manual_seed(53)
    x = torch.randn(n, h, w, c, generator=g)
    x[0, 0:2, 0:2, 0] = torch.tensor([[1.0, -1.0], [0.5, -0.5]])              # a window whose mean is exactly 0
    assert bool((x > 0).any()) and bool((x < 0).any())
    xc = x.cuda()
    for relu_in in (False, True):
        for relu_out in (False, True):
            y = ops.avgpool2_fwd(xc, relu_in, None, relu_out)
            torch.cuda.synchronize()
            ref = emu_ops.avgpool2(x.double(), relu_in, relu_out)
            mag = emu_ops.avgpool2((torch.relu(x) if relu_in else x).abs().double(), False, False) * 4          # sum |a_k|
            bound = 3 * 2.0 ** -24 * 0.25 * mag
            err = (y.double().cpu() - ref).abs()
            assert bool((err <= bound).all())
            tag = f'avgpool2_fwd{shape} relu_in={int(relu_in)} relu_out={int(relu_out)} planes={out16_prec}'
            report(f'{tag} y', (err / bound.clamp_min(1e-300)).max().item(), 1.0 + 1e-12, 'worst |err| / bound')
            if out16_prec is None:
                continue
            y2, p16 = ops.avgpool2_fwd(xc, relu_in, out16_prec, relu_out)
            torch.cuda.synchronize()
            assert torch.equal(y2, y)
            assert p16.c == c and p16.inv is None and (p16.lo is None) == (out16_prec != 1)
            if out16_prec == 1:
                report(f'{tag} hi + lo', rel(decode(p16, 1), y), 3e-6)
            else:
                dt = dtype_of(out16_prec)
                assert torch.equal(p16.hi.view(dt), y.to(dt))
