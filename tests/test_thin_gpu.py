"""Direct GPU tests of the thin-channel kernels (csrc/conv_thin.hip: <= 4 channels on one side of the conv) at small shapes that reach every template
instance: the fp32 VALU forward (1x1 | 3x3, 4 | < 4 channels), the one-k-step MFMA forward with its operand-plane emission, the weight gradient with
the thin side on the input or on the output (fp32 or 16-bit-resident wide input) and the bias gradient of the same pass.  References: fp64 torch on the
CPU, with the tolerances of tests/test_hip_ops.py: rel-L2 1e-2 (bf16) / 3e-5 (bf16x3) / 1e-3 (f16), bias gradient 3e-3 / 1e-5 / 5e-4.  The weight-gradient
kernels are fp32 whatever the operand mode, so they are held to the strictest of the three (bf16x3)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
from guarded_alloc import fence_fixture  # noqa: E402

# every buffer a wrapper takes from torch.empty / empty_like while a test of this module runs is full of NaN-like words (guarded_alloc fill A) and sits
# between two fences that are checked when the test is over; the assertions and tolerances below are what they were
fenced_buffers = fence_fixture()

TOL = {0: 1e-2, 1: 3e-5, 2: 1e-3}
TOL_DB = {0: 3e-3, 1: 1e-5, 2: 5e-4}
STRICT = 1


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def report(name, err, tol):
    print(f'[parity] {name}: rel-L2 {err:.3e} (tol {tol:.0e})')
    assert err < tol, f'{name}: rel-L2 {err:.3e} >= {tol}'


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


# N, H, W, Cin, Cout, ks
FWD_CASES = [
    (2, 7, 16, 3, 64, 3),       # MFMA kernel in bf16 / fp16, VALU in bf16x3; H no multiple of the 4-row group
    (1, 5, 48, 3, 128, 3),      # three 16-pixel segments, two channel blocks
    (2, 6, 12, 3, 64, 3),       # W % 16 != 0: VALU in every mode
    (2, 5, 16, 4, 64, 3),       # 4 live channels
    (2, 5, 16, 1, 64, 1),
    (2, 9, 20, 4, 128, 1),
]


def fwd_setup(case, prec):
    ops = _ops()
    n, h, w, cin, cout, ks = case
    g = torch.Generator().manual_seed(21)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wgt = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) / (cin * ks * ks) ** 0.5
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    alpha = torch.tensor(0.73, dtype=torch.float64)
    ref = alpha * F.conv2d(x, wgt, None, 1, ks // 2) + bias[None, :, None, None]
    assert ops.thin_conv_supported(cin, cout, ks, w)
    pack = ops.pack_weights(wgt.float().cuda(), 0, prec, small_k=(ks == 3))
    kw = dict(ksize=ks, bias=bias.float().cuda(), alpha=alpha.float().cuda(), prec=prec)
    return ops, nhwc(x), pack, kw, ref


def same_planes(got, want, cout):
    assert got.c == cout and torch.equal(got.hi, want.hi)
    assert (got.lo is None) == (want.lo is None) and (want.lo is None or torch.equal(got.lo, want.lo))


@pytest.mark.parametrize('prec', [1, 0, 2])
@pytest.mark.parametrize('case', FWD_CASES)
def test_thin_conv_forward_and_planes(case, prec):
    """y against fp64; where the kernel emits the operand planes itself, they equal lp_act_pack of the fp32 y bit for bit, with and without y"""
    ops, x, pack, kw, ref = fwd_setup(case, prec)
    n, h, w, cin, cout, ks = case
    y = ops.thin_conv(x, pack, **kw)
    torch.cuda.synchronize()
    report(f'thin_conv{case} prec={prec}', rel(y.permute(0, 3, 1, 2), ref), TOL[prec])
    from latent_pose_reenactment_amd import _lib
    emits = bool(_lib.lib().lp_thin_conv_emits_planes(cin, cout, ks, w, prec))
    assert emits == (cin == 3 and ks == 3 and w % 16 == 0 and prec != 1)
    if not emits:
        return
    y0, p0 = ops.thin_conv(x, pack, out16=0, **kw)
    y1, p1 = ops.thin_conv(x, pack, out16=1, **kw)
    none, q1 = ops.thin_conv(x, pack, out16=1, want_y=False, **kw)
    torch.cuda.synchronize()
    assert none is None and torch.equal(y, y0) and torch.equal(y, y1)
    same_planes(p0, ops.act_pack(y, pro=0, prec=prec), cout)
    same_planes(p1, ops.act_pack(y, pro=2, prec=prec), cout)
    same_planes(q1, ops.act_pack(y, pro=2, prec=prec), cout)


def test_thin_conv_planes_in_another_operand_mode():
    """a strict (bf16x3) first conv that feeds fp16 layers: the planes are those of ``out16_prec``"""
    case = FWD_CASES[0]
    ops, x, pack, kw, ref = fwd_setup(case, 1)
    y, p = ops.thin_conv(x, pack, out16=1, out16_prec=2, **kw)
    torch.cuda.synchronize()
    report(f'thin_conv{case} bf16x3, fp16 planes', rel(y.permute(0, 3, 1, 2), ref), TOL[1])
    same_planes(p, ops.act_pack(y, pro=2, prec=2), case[4])


def wgrad_inputs(n, h, w, cin, cout):
    g = torch.Generator().manual_seed(23)
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    dy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    scale = torch.randn(n, cin, generator=g, dtype=torch.float64)
    shift = torch.randn(n, cin, generator=g, dtype=torch.float64) * 0.5
    return x, dy, scale, shift


def wgrad_ref(a, dy, cout, cin, ks):
    wgt = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(a, wgt, None, 1, ks // 2).backward(dy)
    return wgt.grad


@pytest.mark.parametrize('shape', [(2, 7, 12), (3, 13, 16)])
@pytest.mark.parametrize('cout', [64, 128])
@pytest.mark.parametrize('ks', [1, 3])
@pytest.mark.parametrize('cin', [1, 3, 4])
def test_thin_wgrad_thin_input(cin, ks, cout, shape):
    """Cin <= 4: weight and bias gradient from one pass over dy; two runs agree bit for bit"""
    ops = _ops()
    n, h, w = shape
    x, dy, _, _ = wgrad_inputs(n, h, w, cin, cout)
    assert ops.thin_wgrad_supported(cin, cout, ks, 0, w)
    xd, dyd = nhwc(x), nhwc(dy)
    dw, db = ops.thin_wgrad(xd, dyd, ksize=ks, bias_grad=True)
    dw2, db2 = ops.thin_wgrad(xd, dyd, ksize=ks, bias_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    tag = f'({n}, {h}, {w}, {cin}, {cout}, {ks})'
    report('thin_wgrad thin input ' + tag, rel(dw, wgrad_ref(x, dy, cout, cin, ks)), TOL[STRICT])
    report('thin_wgrad bias ' + tag, rel(db, dy.sum(dim=(0, 2, 3))), TOL_DB[STRICT])


def prologue(x, pro, scale, shift):
    if pro == 1:
        return torch.relu(x * scale[:, :, None, None] + shift[:, :, None, None])
    return torch.relu(x) if pro == 2 else x


@pytest.mark.parametrize('shape', [(2, 7, 12), (3, 13, 16)])
@pytest.mark.parametrize('pro', [0, 1, 2])
@pytest.mark.parametrize('cin', [64, 128])
@pytest.mark.parametrize('cout', [1, 3, 4])
def test_thin_wgrad_thin_output(cout, cin, pro, shape):
    """Cout <= 4, 3x3: the prologue of the wide input (none | AdaIN + ReLU | ReLU) applied on the fly; two runs agree bit for bit"""
    ops = _ops()
    n, h, w = shape
    x, dy, scale, shift = wgrad_inputs(n, h, w, cin, cout)
    assert ops.thin_wgrad_supported(cin, cout, 3, pro, w)
    xd, dyd = nhwc(x), nhwc(dy)
    kw = dict(ksize=3, pro=pro, scale=scale.float().cuda() if pro == 1 else None, shift=shift.float().cuda() if pro == 1 else None)
    dw = ops.thin_wgrad(xd, dyd, **kw)
    dw2 = ops.thin_wgrad(xd, dyd, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2)
    report(f'thin_wgrad thin output ({n}, {h}, {w}, {cin}, {cout}) pro={pro}', rel(dw, wgrad_ref(prologue(x, pro, scale, shift), dy, cout, cin, 3)),
           TOL[STRICT])


@pytest.mark.parametrize('pro', [1, 2])
@pytest.mark.parametrize('case', [(2, 8, 12, 64, 4, 3), (1, 5, 16, 128, 3, 3)])
def test_thin_wgrad16_equals_the_fp32_form_on_the_same_values(case, pro):
    """the 16-bit-resident wide input decodes to exactly the fp32 values given to ``thin_wgrad``, so the two results are the same bits"""
    ops = _ops()
    n, h, w, cin, cout, ks = case
    x, dy, scale, shift = wgrad_inputs(n, h, w, cin, cout)
    hi = nhwc(x).half().view(torch.int16)
    x16 = ops.Act16(hi, None, cin, None)
    dyd = nhwc(dy)
    kw = dict(ksize=ks, pro=pro, scale=scale.float().cuda() if pro == 1 else None, shift=shift.float().cuda() if pro == 1 else None)
    dw = ops.thin_wgrad16(x16, dyd, **kw)
    dw2 = ops.thin_wgrad16(x16, dyd, **kw)
    want = ops.thin_wgrad(x16.hi.view(torch.float16).float(), dyd, **kw)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(dw, want)
    a = prologue(x16.hi.view(torch.float16).double().cpu().permute(0, 3, 1, 2), pro, scale, shift)
    report(f'thin_wgrad16{case} pro={pro}', rel(dw, wgrad_ref(a, dy, cout, cin, ks)), TOL[STRICT])
