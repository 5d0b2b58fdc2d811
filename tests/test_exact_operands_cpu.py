"""CPU proof of tests/exact_operands.py, before tests/test_conv_dma_exact.py, tests/test_conv_phase_exact.py, tests/test_conv_pipe_exact.py and
tests/test_wgrad_exact.py hold kernels to it bit for bit: the hi / lo split identity, the budget assertion, the fp64 references against integer
arithmetic, the phase forms of the 16 pre-summed taps against the dense operations and against their adjoints in int64, and the decoded planes of the
bit-level packers of tests/operand_restatement.py against the inputs.  No GPU, nothing from the library."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_operands as E  # noqa: E402
import operand_restatement as R  # noqa: E402


def test_hi_lo_split_reproduces_every_integer_up_to_65535():
    v = torch.arange(-65535, 65536, dtype=torch.float32)
    hi, lo = E.split_hi_lo(v)
    assert torch.equal(hi.double() + lo.double(), v.double())
    # ... also times the power-of-two quanta of the cases, and the restatement's integer-arithmetic split agrees word for word
    for q in (E.QA, E.QW):
        h2, l2 = E.split_hi_lo(v * q)
        assert torch.equal(h2.double() + l2.double(), (v * q).double())
        hw, lw = R.split((v * q).numpy(), R.PREC_BF16X3)
        assert np.array_equal(R.bf16_decode(hw), h2.numpy()) and np.array_equal(R.bf16_decode(lw), l2.numpy())


def test_wide_ranges_are_exact_in_their_formats_and_load_the_lo_plane():
    for prec in (E.PREC_BF16, E.PREC_F16):
        v = torch.arange(-255, 256, dtype=torch.float32) * E.QA
        assert torch.equal(E.terms(v, prec)[0], v.double())
    with pytest.raises(AssertionError):
        E.terms(torch.tensor([257.0]), E.PREC_BF16)                     # nine significand bits: not a bf16 value
    for big, lo_frac in ((False, 0.25), (True, 0.5)):
        b = E.wide_bound(E.PREC_BF16X3, big)
        v = torch.arange(-b, b + 1, dtype=torch.float32)
        lo = E.terms(v, E.PREC_BF16X3)[1]
        assert abs(float((lo != 0).double().mean()) - lo_frac) < 0.1, float((lo != 0).double().mean())


def test_budget_assertion_fires_on_an_over_budget_draw():
    g = torch.Generator().manual_seed(1)
    # Cin 576, 3x3, both operands at full width: 5184 terms of up to 255 * 255 quanta >> 2^22
    a = E.draw_ints(g, (1, 576, 4, 4), 255).float() * E.QA
    w = E.draw_ints(g, (8, 576, 3, 3), 255).float() * E.QW
    with pytest.raises(E.BudgetError):
        E.assert_budget(E.conv_bound(E.terms(a, 0), E.terms(w, 0), False, E.ALPHA), E.ALPHA * E.QA * E.QW, 'over budget')
    # the same draw with the narrow weight range is inside, and draw_pair finds it by shrinking
    seen = []

    def bound(at, wt):
        seen.append(float(wt[0].abs().max()) / E.QW)
        return E.assert_budget(E.conv_bound(at, wt, False, E.ALPHA), E.ALPHA * E.QA * E.QW, 'case')
    a2, w2 = E.draw_pair(3, (1, 576, 4, 4), (8, 576, 3, 3), E.PREC_BF16X3, 'a', bound)
    assert seen and seen[-1] <= 2 and float(a2.abs().max()) / E.QA > 255
    # a bias that alone exceeds the budget
    with pytest.raises(E.BudgetError):
        E.assert_budget(E.conv_bound(E.terms(a2, 1), E.terms(w2, 1), False, E.ALPHA, bias=torch.full((8,), 2.0 ** 23) * E.ALPHA * E.QA * E.QW),
                        E.ALPHA * E.QA * E.QW, 'bias')
    # the largest contraction of the conv table: Cin 576, 3x3, |a| <= 511, w in {-1, 0, 1}: about 9e5 quanta
    g = torch.Generator().manual_seed(2)
    a = E.draw_ints(g, (2, 576, 4, 4), 511).float() * E.QA
    w = E.draw_ints(g, (128, 576, 3, 3), 1).float() * E.QW
    quanta = E.assert_budget(E.conv_bound(E.terms(a, 1), E.terms(w, 1), False, 1.0), E.QA * E.QW, 'largest')
    assert 5e5 < quanta < 2 ** 20


@pytest.mark.parametrize('prec', [E.PREC_BF16, E.PREC_BF16X3, E.PREC_F16])
@pytest.mark.parametrize('ks,ups', [(3, False), (3, True), (1, False)])
def test_fp64_references_equal_integer_arithmetic(prec, ks, ups):
    g = torch.Generator().manual_seed(10 * prec + ks + int(ups))
    n, cin, cout, h, w = 2, 24, 10, 6, 8
    hin, win = (h // 2, w // 2) if ups else (h, w)
    b = E.wide_bound(prec)
    ai = E.draw_ints(g, (n, cin, hin, win), b)
    wi = E.draw_ints(g, (cout, cin, ks, ks), 2)
    at, wt = E.terms(ai.float() * E.QA, prec), E.terms(wi.float() * E.QW, prec)
    ref = E.conv64(at, wt, ups)
    # integer restatement: the terms as integers of their own quantum (2^-8 of the operand quantum covers every lo word here)
    s = 256
    ti = [[(t / q * s).round().long() for t in ts] for ts, q in ((at, E.QA), (wt, E.QW))]
    assert all(torch.equal(i.double() / s * q, t) for ts, it, q in ((at, ti[0], E.QA), (wt, ti[1], E.QW)) for t, i in zip(ts, it))
    want = E.conv_int64(ti[0][0], sum(ti[1]), ups)
    if prec == E.PREC_BF16X3:
        want = want + E.conv_int64(ti[0][1], ti[1][0], ups)
    assert torch.equal(ref, want.double() * (E.QA * E.QW / (s * s)))
    if prec != E.PREC_BF16X3:                                          # single-plane modes: the contraction of the integers themselves
        assert torch.equal(ref, E.conv_int64(ai, wi, ups).double() * (E.QA * E.QW))
    # weight gradient: dw[co][ci][ky][kx] = sum dy[n, co, y, x] * up2?(a)[n, ci, y + ky - pad, x + kx - pad], by integer shifted sums
    di = E.draw_ints(g, (n, cout, h, w), 2)
    dt = E.terms(di.float() * E.QW, prec)
    dw = E.wgrad64(at, dt, ks, ups)
    assert dw.shape == (cout, cin, ks, ks)
    au = E.up2(ti[0][0]) if ups else ti[0][0]
    al = (E.up2(ti[0][1]) if ups else ti[0][1]) if prec == E.PREC_BF16X3 else None
    dsum = sum((t / E.QW * s).round().long() for t in dt)
    dhi = (dt[0] / E.QW * s).round().long()
    pad = ks // 2
    want = torch.zeros((cout, cin, ks, ks), dtype=torch.int64)
    for ky in range(ks):
        for kx in range(ks):
            for src, d in ((au, dsum), (al, dhi)):
                if src is None:
                    continue
                ap = torch.zeros((n, cin, h + 2 * pad, w + 2 * pad), dtype=torch.int64)
                ap[:, :, pad:pad + h, pad:pad + w] = src
                want[:, :, ky, kx] += torch.einsum('nchw,nohw->oc', ap[:, :, ky:ky + h, kx:kx + w], d)
    assert torch.equal(dw, want.double() * (E.QA * E.QW / (s * s)))


def _int_taps(wi, mode):
    """the 16 pre-summed taps of R.weight_values as int64 [16][rows][cols]; modes 4 / 5 carry the factor 1/4 and are returned TIMES FOUR"""
    v = R.weight_values(wi.numpy().astype(np.float64), mode) * (4.0 if mode >= 4 else 1.0)
    assert np.array_equal(v, np.round(v))
    return torch.from_numpy(v.astype(np.int64))


def _box2(t):
    return t[:, :, 0::2, 0::2] + t[:, :, 0::2, 1::2] + t[:, :, 1::2, 0::2] + t[:, :, 1::2, 1::2]


PHASE_GEOMETRIES = [(2, 5, 7, 3, 4), (1, 3, 2, 6, 5), (3, 2, 2, 1, 1), (1, 1, 1, 2, 3)]      # N, Cin, Cout, low-resolution h, w


@pytest.mark.parametrize('geo', PHASE_GEOMETRIES)
def test_scatter_form_of_the_mode_2_taps_is_the_upsampled_conv(geo):
    """int64: the 16-tap scatter form == conv3x3(nearest_up2(x)) with the original 3x3 weights"""
    n, cin, cout, h, w = geo
    g = torch.Generator().manual_seed(sum(geo))
    x, wi = E.draw_ints(g, (n, cin, h, w), 255), E.draw_ints(g, (cout, cin, 3, 3), 63)
    got = E.phase_conv(x, _int_taps(wi, 2), gather=False)
    assert got.dtype == torch.int64 and torch.equal(got, E.conv_int64(x, wi, ups=True))


@pytest.mark.parametrize('geo', PHASE_GEOMETRIES)
def test_gather_form_of_the_mode_4_taps_is_the_box_sum_of_the_dense_conv(geo):
    """int64: the gather form with 4 x the mode-4 taps == the 2 x 2 box sum of conv3x3(x), i.e. 4 x AvgPool2d(2)"""
    n, cin, cout, h, w = geo
    g = torch.Generator().manual_seed(sum(geo) + 1)
    x, wi = E.draw_ints(g, (n, cin, 2 * h, 2 * w), 255), E.draw_ints(g, (cout, cin, 3, 3), 63)
    got = E.phase_conv(x, _int_taps(wi, 4), gather=True)
    assert torch.equal(got, _box2(E.conv_int64(x, wi)))


@pytest.mark.parametrize('fwd,bwd', [(2, 3), (4, 5)])
@pytest.mark.parametrize('geo', PHASE_GEOMETRIES)
def test_data_gradient_modes_are_the_adjoints_of_the_forward_modes(geo, fwd, bwd):
    """int64: <f(x), d> == <x, f^T(d)> -- mode 3 (gather) is the adjoint of mode 2 (scatter), mode 5 (scatter) of mode 4 (gather)"""
    n, cin, cout, h, w = geo
    g = torch.Generator().manual_seed(sum(geo) + fwd)
    wi = E.draw_ints(g, (cout, cin, 3, 3), 63)
    x = E.draw_ints(g, (n, cin, h, w) if fwd == 2 else (n, cin, 2 * h, 2 * w), 255)
    d = E.draw_ints(g, (n, cout, 2 * h, 2 * w) if fwd == 2 else (n, cout, h, w), 255)
    fx = E.phase_conv(x, _int_taps(wi, fwd), gather=(fwd == 4))
    ftd = E.phase_conv(d, _int_taps(wi, bwd), gather=(bwd == 3))
    assert fx.shape == d.shape and ftd.shape == x.shape
    assert int((fx * d).sum()) == int((x * ftd).sum())
    # ... and element by element against the adjoint written out: the gradient of <f(x), d> w.r.t. every x is the response to a unit impulse
    lin = torch.zeros_like(x)
    for idx in ((0, 0, 0, 0), (n - 1, cin - 1, x.shape[2] - 1, x.shape[3] - 1), (0, cin - 1, x.shape[2] // 2, 0)):
        e = torch.zeros_like(x)
        e[idx] = 1
        lin[idx] = int((E.phase_conv(e, _int_taps(wi, fwd), gather=(fwd == 4)) * d).sum())
        assert lin[idx] == ftd[idx], (idx, lin[idx], ftd[idx])


@pytest.mark.parametrize('prec', [E.PREC_BF16, E.PREC_BF16X3, E.PREC_F16])
def test_phase_conv64_on_the_terms_of_the_pre_summed_taps(prec):
    """the fp64 phase references against integer arithmetic on the terms (hi * (hi + lo) + lo * hi over the split of the PRE-SUMMED value); in the
    single-plane modes they equal the dense definitions -- conv64(ups) and the average pool of conv64 -- because the tap sums are exact"""
    g = torch.Generator().manual_seed(40 + prec)
    n, cin, cout, h, w = 2, 12, 6, 4, 6
    b = E.wide_bound(prec, big=True)
    s = 256
    for mode in (2, 3, 4, 5):
        gather = mode in (3, 4)
        qw = E.QW / 4 if mode >= 4 else E.QW
        wi = E.draw_ints(g, (cout, cin, 3, 3), b if prec == E.PREC_BF16X3 else E.WIDE_W_PHASE)
        wt = wi.float() * E.QW
        taps = torch.from_numpy(R.weight_values(wt.numpy(), mode))
        cols = taps.shape[2]
        ai = E.draw_ints(g, (n, cols, 2 * h, 2 * w) if gather else (n, cols, h, w), 2)
        at, tt = E.terms(ai.float() * E.QA, prec), E.terms(taps, prec)
        ref = E.phase_conv64(at, tt, gather)
        ti = [[(t / q * s).round().long() for t in ts] for ts, q in ((at, E.QA), (tt, qw))]
        assert all(torch.equal(i.double() / s * q, t) for ts, it, q in ((at, ti[0], E.QA), (tt, ti[1], qw)) for t, i in zip(ts, it))
        want = E.phase_conv(ti[0][0], sum(ti[1]), gather)
        if prec == E.PREC_BF16X3:
            want = want + E.phase_conv(ti[0][1], ti[1][0], gather)
        assert torch.equal(ref, want.double() * (E.QA * qw / (s * s))), mode
        bound = E.phase_bound(at, tt, gather, 1.0)
        assert bool((ref.abs() <= bound).all())
        if prec != E.PREC_BF16X3 and mode == 2:
            assert torch.equal(ref, E.conv64(at, E.terms(wt, prec), ups=True))
        if prec != E.PREC_BF16X3 and mode == 4:
            assert torch.equal(ref, torch.nn.functional.avg_pool2d(E.conv64(at, E.terms(wt, prec)), 2))


@pytest.mark.parametrize('prec', [E.PREC_BF16, E.PREC_BF16X3, E.PREC_F16])
def test_restated_packers_decode_to_the_inputs(prec):
    """what lp_act_pack / lp_pack_weights are documented to write (tests/operand_restatement.py), decoded, is the exact operand again -- pad words zero"""
    g = torch.Generator().manual_seed(prec)
    b = E.wide_bound(prec, big=True)
    x = (E.draw_ints(g, (2, 5, 7, 12), b).float() * E.QA).numpy()              # [N][H][W][C], C = 12 -> C8 = 16
    hi, lo = R.planes(x, 0, prec=prec)
    assert hi.shape == (2, 35, 16) and not hi[:, :, 12:].any() and (lo is None or not lo[:, :, 12:].any())
    assert np.array_equal(R.decode(hi, lo, prec)[:, :, :12], x.reshape(2, 35, 12).astype(np.float64))
    hi, lo = R.planes(x, 2, prec=prec)                                            # the relu prologue
    assert np.array_equal(R.decode(hi, lo, prec)[:, :, :12], np.maximum(x, 0).reshape(2, 35, 12).astype(np.float64))
    # the fp16 gradient scale is a power of two that keeps the integers exact
    x8 = (E.draw_ints(g, (2, 5, 7, 12), 255).float() * E.QA).numpy()
    s, inv = R.amax_scale(np.abs(x8).max())
    assert s * inv == 1 and float(np.log2(s)).is_integer()
    hs, _ = R.planes(x8, 0, prec=R.PREC_F16, in_scale=s)
    assert np.array_equal(R.decode(hs, None, R.PREC_F16)[:, :, :12] * np.float64(inv), x8.reshape(2, 35, 12).astype(np.float64))
    w = (E.draw_ints(g, (10, 12, 3, 3), b).float() * E.QW).numpy()
    for mode in (0, 1):
        rows, cols = (10, 12) if mode == 0 else (12, 10)
        wh, wl = R.weight_pack(w, mode, 128, 64, prec)
        dec = R.decode(wh, wl, prec)
        assert not dec[:, rows:, :].any() and not dec[:, :, cols:].any()
        img = dec[:, :rows, :cols]
        want = w.reshape(10, 12, 9).transpose(2, 0, 1) if mode == 0 else w.reshape(10, 12, 9)[:, :, ::-1].transpose(2, 1, 0)
        assert np.array_equal(img, want.astype(np.float64))
