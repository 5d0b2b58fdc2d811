"""CPU proof of tests/operand_restatement.py, the reference that tests/test_operand_packers_gpu.py holds the operand packers to word for word.
The conversions are pinned bit for bit to torch's CPU conversions, the fused affine to exact rational arithmetic, the weight images to the conv
algebra they stand for (fp64, no rounding) and the amax scale to a table.  No GPU needed."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operand_restatement as R  # noqa: E402


def _values():
    """2^20 random fp32 values over the fp16 / bf16 ranges of interest plus the edge list (fp32 subnormals included: on the CPU both sides are IEEE)"""
    rng = np.random.default_rng(11)
    n = 1 << 20
    mant = rng.standard_normal(n)
    expo = rng.integers(-30, 18, size=n)                        # 2^-30 .. 2^17: fp16 underflow, subnormals, normals, overflow
    x = (mant * np.exp2(expo)).astype(np.float32)
    ties16 = (rng.integers(-(1 << 12), 1 << 12, size=4096) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -12)      # odd multiples of 2^-12: fp16 ties in [1, 2)
    ties_b = (rng.integers(-(1 << 9), 1 << 9, size=4096) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -9)        # odd multiples of 2^-9: bf16 ties in [1, 2)
    return np.concatenate([x, ties16, ties_b, R.edge_values(True)])


def _same_words(got, want, nan_of):
    nan = nan_of(want)
    assert np.array_equal(nan_of(got), nan)
    assert np.array_equal(got[~nan], want[~nan])


def test_bf16_rne_equals_torch_bit_for_bit():
    x = _values()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    _same_words(R.bf16_rne(x), want, lambda w: R.is_nan_word(w, R.PREC_BF16))
    assert np.array_equal(R.bf16_decode(want)[~np.isnan(x)], torch.from_numpy(x).to(torch.bfloat16).float().numpy()[~np.isnan(x)])


def test_f16_sat_equals_torch_bit_for_bit():
    x = _values()
    want = torch.from_numpy(x).clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16).numpy().view(np.uint16)
    _same_words(R.f16_sat(x), want, lambda w: R.is_nan_word(w, R.PREC_F16))


def test_conversion_edges_by_value():
    """the IEEE facts themselves, as literal words: independent of any library"""
    f = lambda v: int(R.f16_sat(np.float32(v)).item())
    b = lambda v: int(R.bf16_rne(np.float32(v)).item())
    assert (f(7e4), f(np.inf), f(-np.inf), f(65520.0), f(65519.0), f(65504.0)) == (0x7BFF, 0x7BFF, 0xFBFF, 0x7BFF, 0x7BFF, 0x7BFF)
    assert (f(2.0 ** -14), f(2.0 ** -24), f(2.0 ** -25), f(3 * 2.0 ** -25), f(5 * 2.0 ** -25), f(1e-30), f(-0.0)) == (0x0400, 1, 0, 2, 2, 0, 0x8000)
    assert (f(1 + 2.0 ** -11), f(1 + 3 * 2.0 ** -11), f(-(1 + 2.0 ** -11))) == (0x3C00, 0x3C02, 0xBC00)
    assert (b(1 + 2.0 ** -8), b(1 + 3 * 2.0 ** -8), b(-(1 + 2.0 ** -8)), b(np.inf), b(-0.0)) == (0x3F80, 0x3F82, 0xBF80, 0x7F80, 0x8000)
    assert R.is_nan_word(R.f16_sat(np.float32(np.nan)), 2).all() and R.is_nan_word(R.bf16_rne(np.float32(np.nan)), 0).all()


def test_split_reconstructs_to_2_pow_minus_16():
    """hi + lo = x within 2^-16 |x| (csrc/lp_common.h): two half-ulp roundings of 8-bit significands; and q - hi is exact in fp32"""
    x = _values()
    x = x[np.isfinite(x) & (np.abs(x) >= 2.0 ** -100)]               # the claim is about normal values (lo must not underflow)
    hi, lo = R.split(x, R.PREC_BF16X3)
    h = R.bf16_decode(hi)
    assert np.array_equal((x - h).astype(np.float64), x.astype(np.float64) - h.astype(np.float64))
    err = np.abs(R.decode(hi, lo, R.PREC_BF16X3) - x.astype(np.float64))
    assert (err <= 2.0 ** -16 * np.abs(x.astype(np.float64))).all()
    assert np.array_equal(lo, R.bf16_rne(x - h))


def _adversarial_fma():
    """(x, a, b) whose exact x * a + b lies within 2^-70 of an fp32 rounding midpoint: x * a = +-2^-24 (1 - k^2 2^-46), b in [1, 2) -- the fp64 sum
    lands exactly ON the midpoint and only the TwoSum error term knows the side"""
    rng = np.random.default_rng(5)
    k = rng.integers(1, 1000, size=2000)
    sgn = np.where(rng.integers(0, 2, size=2000) == 1, 1.0, -1.0)
    x = (sgn * 2.0 ** -12 * (1 + k * 2.0 ** -23)).astype(np.float32)
    a = (2.0 ** -12 * (1 - k * 2.0 ** -23)).astype(np.float32)
    b = (1 + rng.integers(0, 1 << 23, size=2000) * 2.0 ** -23).astype(np.float32)
    return x, a, b


def _fma_exact(x, a, b):
    """correctly rounded fp32 of the exact rational x * a + b"""
    out = np.empty(len(x), dtype=np.float32)
    for i, (xi, ai, bi) in enumerate(zip(x.tolist(), a.tolist(), b.tolist())):
        t = Fraction(xi) * Fraction(ai) + Fraction(bi)
        r = np.float32(float(t))                                     # a first guess (double rounding possible), then the exact nearest of its neighbours
        cands = [r, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - t), int(np.float32(c).view(np.uint32)) & 1))      # nearest; an exact tie goes to even
        out[i] = best
    return out


def test_fma32_is_the_correctly_rounded_fused_affine():
    """no element is excused for double rounding: on 2000 adversarial triples (where rounding the fp64 sum IS wrong for a part of them) and 4000
    random ones the restated fused multiply-add equals the correctly rounded exact rational result"""
    x, a, b = _adversarial_fma()
    got, naive = R.fma32(x, a, b, return_naive=True)
    want = _fma_exact(x, a, b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (naive != want).sum() > 100, 'the adversarial set must contain cases that plain fp64 evaluation gets wrong'
    rng = np.random.default_rng(6)
    x, a, b = (rng.standard_normal(4000).astype(np.float32) for _ in range(3))
    assert np.array_equal(R.fma32(x, a, b).view(np.uint32), _fma_exact(x, a, b).view(np.uint32))


def test_grid_set_affines_are_exact_and_hold_ties():
    """the bit-exact GPU input set: 1 M triples, every affine exact in fp32 whether fused or not, and tens of thousands of exact bf16 ties among them"""
    x, sc, sf = R.grid_set(np.random.default_rng(7), (1 << 20,), (1 << 20,))
    exact = x.astype(np.float64) * sc.astype(np.float64) + sf.astype(np.float64)
    unfused = (x * sc) + sf
    assert np.array_equal(unfused.astype(np.float64), exact) and np.array_equal(R.fma32(x, sc, sf).astype(np.float64), exact)
    u = unfused.view(np.uint32)
    ties = int(((u & 0xFFFF) == 0x8000).sum())
    assert 10000 < ties < 100000, ties
    assert (np.abs(unfused[unfused != 0]) >= 2.0 ** -14).all()        # no fp32 subnormal can arise


def test_act_prologues_against_torch():
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 9, 11)).astype(np.float32) * 4
    x[0, 0, :3] = [np.nan, -np.inf, np.inf]
    sn, fn = rng.standard_normal((2, 11)).astype(np.float32), rng.standard_normal((2, 11)).astype(np.float32)
    sc, fc = sn[0], fn[0]
    xt = torch.from_numpy(x).double()
    ref = {0: xt, 2: torch.relu(xt),
           1: torch.relu(xt * torch.from_numpy(sn).double()[:, None] + torch.from_numpy(fn).double()[:, None]),
           3: F.relu6(xt * torch.from_numpy(sc).double() + torch.from_numpy(fc).double()),
           4: torch.relu(xt * torch.from_numpy(sc).double() + torch.from_numpy(fc).double()),
           5: xt * torch.from_numpy(sc).double() + torch.from_numpy(fc).double()}
    for pro in range(6):
        got = R.act(x, pro, sn if pro == 1 else sc, fn if pro == 1 else fc)
        want = ref[pro].float().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), pro
        ok = ~np.isnan(want)
        assert np.array_equal(got[ok], want[ok]), pro
    assert np.isnan(R.act(x, 2)[0, 0, 0]) and R.act(x, 2)[0, 0, 1] == 0 and np.isinf(R.act(x, 0)[0, 0, 2])


def test_planes_layout_and_pads():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((3, 5, 7, 3)).astype(np.float32)
    hi, lo = R.planes(x, 0, prec=R.PREC_BF16X3, in_scale=0.5)
    assert hi.shape == lo.shape == (3, 35, 8) and not hi[:, :, 3:].any() and not lo[:, :, 3:].any()
    assert np.array_equal(hi[:, :, :3].reshape(3, 5, 7, 3), R.bf16_rne(x * np.float32(0.5)))


@pytest.mark.parametrize('m,want', [(1.0, 2.0 ** 12), (0.75, 2.0 ** 13), (4096.0, 1.0), (2.0 ** -140, 2.0 ** 100), (3e-30, 2.0 ** 100), (2.0 ** 120, 2.0 ** -100),
                                    (0.0, 1.0), (-1.0, 1.0), (np.inf, 1.0), (np.nan, 1.0), (3.2e38, 1.0)])
def test_amax_scale_table(m, want):
    s, inv = R.amax_scale(m)
    assert s == np.float32(want) and inv == np.float32(1.0 / want) and float(s) * float(inv) == 1.0


# ---- weight images against the conv algebra, fp64, no rounding -----------------------------------------------------------------------
def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _wx(cout=5, cin=3, h=6, w=6, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64), torch.randn(2, cin, h, w, generator=g, dtype=torch.float64)


def _img(w, mode):
    return torch.from_numpy(R.weight_values(w.numpy(), mode))


def _shifted(t, oy, ox):
    """t[.., y + oy, x + ox] with zeros outside"""
    h, w = t.shape[-2:]
    p = F.pad(t, (2, 2, 2, 2))
    return p[..., 2 + oy:2 + oy + h, 2 + ox:2 + ox + w]


def test_modes_0_and_1_are_the_conv_and_its_data_gradient():
    w, x = _wx()
    img0 = _img(w, 0)                                               # [t][co][ci]
    assert _rel(F.conv2d(x, img0.permute(1, 2, 0).reshape(5, 3, 3, 3), padding=1), F.conv2d(x, w, padding=1)) < 1e-12
    x.requires_grad_(True)
    y = F.conv2d(x, w, padding=1)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    y.backward(dy)
    img1 = _img(w, 1)                                               # [t][ci][co]: conv taps over dy
    assert _rel(F.conv2d(dy, img1.permute(1, 2, 0).reshape(3, 5, 3, 3), padding=1), x.grad) < 1e-12
    w1, x1 = torch.randn(6, 4, 1, 1, dtype=torch.float64), torch.randn(1, 4, 3, 3, dtype=torch.float64)
    assert torch.equal(_img(w1, 0)[0], w1[:, :, 0, 0]) and torch.equal(_img(w1, 1)[0], w1[:, :, 0, 0].t())
    assert _rel(F.conv2d(x1, _img(w1, 0).permute(1, 2, 0).reshape(6, 4, 1, 1)), F.conv2d(x1, w1)) < 1e-12


def test_modes_2_and_3_are_the_upsampled_conv_and_its_adjoint():
    w, x = _wx()
    n, _, h, wd = x.shape
    img2, img3 = _img(w, 2), _img(w, 3)
    x.requires_grad_(True)
    ref = F.conv2d(x.repeat_interleave(2, 2).repeat_interleave(2, 3), w, padding=1)
    out = torch.zeros_like(ref)
    for a in range(2):
        for b in range(2):
            for i in range(2):
                for j in range(2):                                  # tap (i, j) of phase (a, b) reads the low-resolution pixel (y + a - 1 + i, x + b - 1 + j)
                    out[:, :, a::2, b::2] += torch.einsum('oc,nchw->nohw', img2[(2 * a + b) * 4 + 2 * i + j], _shifted(x.detach(), a - 1 + i, b - 1 + j))
    assert _rel(out, ref.detach()) < 1e-12
    dy = torch.randn(ref.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    ref.backward(dy)
    dx = torch.zeros(n, 3, h, wd, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for i in range(2):
                for j in range(2):                                  # a 2x2 conv per phase over the phase-subsampled dy with origin y - a
                    dx += torch.einsum('co,nohw->nchw', img3[(2 * a + b) * 4 + 2 * i + j], _shifted(dy[:, :, a::2, b::2], i - a, j - b))
    assert _rel(dx, x.grad) < 1e-12


def test_modes_4_and_5_are_conv_then_avgpool_and_its_adjoint():
    w, x = _wx()
    n, _, h, wd = x.shape
    img4, img5 = _img(w, 4), _img(w, 5)
    x.requires_grad_(True)
    ref = F.avg_pool2d(F.conv2d(x, w, padding=1), 2)
    w44 = torch.zeros(5, 3, 4, 4, dtype=torch.float64)              # [u + 1][v + 1]: pooled[y] = sum_u W4[u] in[2y + u], u = -1 .. 2
    for pa in range(2):
        for pb in range(2):
            for ky in range(2):
                for kx in range(2):
                    w44[:, :, 2 * ky - pa + 1, 2 * kx - pb + 1] = img4[pa * 8 + pb * 4 + ky * 2 + kx]
    assert _rel(F.conv2d(x.detach(), w44, stride=2, padding=1), ref.detach()) < 1e-12
    dp = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref.backward(dp)
    dx = torch.zeros(n, 3, h, wd, dtype=torch.float64)
    for a in range(2):
        for b in range(2):
            for i in range(2):
                for j in range(2):                                  # hi-res pixel (2y + a, 2x + b) collects from the pooled pixel (y + a - 1 + i, x + b - 1 + j)
                    dx[:, :, a::2, b::2] += torch.einsum('co,nohw->nchw', img5[a * 8 + b * 4 + i * 2 + j], _shifted(dp, a - 1 + i, b - 1 + j))
    assert _rel(dx, x.grad) < 1e-12


@pytest.mark.parametrize('c,cg', [(128, 4), (64, 64), (128, 32)])
def test_grouped_image_is_the_grouped_conv_and_its_adjoint(c, cg):
    g = torch.Generator().manual_seed(4)
    w = torch.randn(c, cg, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(1, c, 5, 4, generator=g, dtype=torch.float64, requires_grad=True)
    ref = F.conv2d(x, w, padding=1, groups=c // cg)
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(dy)
    cp = c + 64
    for mode, src, want in ((0, x.detach(), ref.detach()), (1, dy, x.grad)):
        img = torch.from_numpy(R.grouped_values(w.numpy(), cg, cp, mode))      # [9][CP][64]
        assert not img[:, c:].any()
        dense = torch.zeros(c, c, 9, dtype=torch.float64)           # [row][other side][t]: block diagonal over aligned 64-channel blocks
        for blk in range(c // 64):
            dense[blk * 64:blk * 64 + 64, blk * 64:blk * 64 + 64] = img[:, blk * 64:blk * 64 + 64, :].permute(1, 2, 0)
        assert _rel(F.conv2d(src, dense.reshape(c, c, 3, 3), padding=1), want) < 1e-12


def test_weight_pack_pads_and_grid_sums_exact():
    """weights on the 2^-10 grid in [-2, 2): every tap sum of modes 2 .. 5 is exact in fp32 (so the order of the additions cannot matter), pads are zero words"""
    rng = np.random.default_rng(10)
    w = (rng.integers(-2048, 2048, size=(7, 5, 3, 3)) / 1024.0).astype(np.float32)
    for mode in range(6):
        assert np.array_equal(R.weight_values(w, mode).astype(np.float64), R.weight_values(w.astype(np.float64), mode))
        rows, cols = (7, 5) if mode in (0, 2, 4) else (5, 7)
        for prec in range(3):
            hi, lo = R.weight_pack(w, mode, 16, 8, prec)
            assert hi.shape == (9 if mode < 2 else 16, 16, 8) and not hi[:, rows:].any() and not hi[:, :, cols:].any()
            assert (lo is None) == (prec != 1)
            if lo is not None:
                assert not lo[:, rows:].any() and not lo[:, :, cols:].any()
            assert np.array_equal(hi[:, :rows, :cols], R.split(R.weight_values(w, mode), prec)[0])
