"""The ill-conditioned inputs of tests/conditioning_inputs.py DISCRIMINATE (no GPU): on every family and every shape the GPU file
(tests/test_norm_conditioning_gpu.py) uses, an fp32 emulation of the shifted-sums + Chan-merge algorithm is inside the gate the GPU routes are
held to, and plain fp32 sums (E[x^2] - E[x]^2) miss that gate by at least 10x on the worst kappa >= 1e3 channel -- which is what makes the GPU
gate mean something.  On today's `randn * 3 + 10` inputs (test_hip_ops.test_instnorm_stats) the plain sums PASS today's 2e-5 gate up to
HW = 1024: recorded here as an assertion so that the reason for the conditioning tests stays visible.  Errors are per (n, c) against fp64
statistics of the same fp32 tensor: e_mean in standard deviations, e_rstd relative (see conditioning_inputs)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conditioning_inputs as ci  # noqa: E402

FAMILIES = ('kappa', 'constant', 'ramp', 'first_far')
_CACHE = {}


def case(shape, per_image):
    """inputs, their kinds per column and the fp64 reference: computed once per shape"""
    key = (shape, per_image)
    if key not in _CACHE:
        x, kd = ci.make(shape, seed=sum(shape), per_image=per_image)
        cols = ci.columns(x, per_image)
        flat = [k for row in kd for k in row] if per_image else kd[0]
        _CACHE[key] = (cols, flat, ci.reference(cols))
    return _CACHE[key]


def ids(v):
    return 'x'.join(map(str, v[0])) + ('-per-image' if v[1] else '-batch')


@pytest.mark.parametrize('case_', ci.SHAPES, ids=ids)
def test_every_family_is_present_and_as_conditioned_as_it_claims(case_):
    cols, flat, ref = case(*case_[:2])
    assert {k.name for k in flat} == set(FAMILIES)
    assert max(k.kappa for k in flat if k.name == 'kappa') >= 1e3
    for j, k in enumerate(flat):
        if k.name == 'kappa' and k.kappa > 0:
            assert 0.8 * k.kappa < ref.kappa[j] < 1.25 * k.kappa, (k, ref.kappa[j])            # the measured kappa is the nominal one
            assert np.sign(ref.mean[j]) == k.sign
        if k.name == 'constant':
            assert ref.var[j] == 0 and ref.mean[j] == k.value
    assert np.isfinite(cols).all()


@pytest.mark.parametrize('block', [64, 1024])
@pytest.mark.parametrize('case_', ci.SHAPES, ids=ids)
def test_shifted_sums_with_chan_merge_are_inside_every_route_gate(case_, block):
    cols, flat, ref = case(*case_[:2])
    mean, rstd = ci.shifted_stats(cols, block=block)
    assert np.isfinite(mean).all() and np.isfinite(rstd).all()
    e_mean, e_rstd = ci.errors(mean, rstd, ref)
    gates = [ci.gate(r, ref) for r in list(ci.ROUTES.values()) + [ci.emulation_route(block)]]      # ALL routes, not only the shape's
    g_mean, g_rstd = np.min([g[0] for g in gates], 0), np.min([g[1] for g in gates], 0)         # the tightest of them, per column
    for fam in FAMILIES:
        sel = np.array([k.name == fam for k in flat])
        if fam == 'constant':
            want = np.array([k.value for k in flat], np.float32)[sel]
            assert np.array_equal(mean[sel], want), 'a constant channel has its value as mean, bit for bit'
            assert (rstd[sel] == ci.const_rstd(ci.EPS)).all(), 'M2 = 0: rstd = 1/sqrtf(eps) to the bit'
            continue
        jm, jr = (int(np.argmax(np.where(sel, e / np.maximum(g, 1e-300), -1.0))) for e, g in ((e_mean, g_mean), (e_rstd, g_rstd)))            # the channels nearest their gates
        print(f'[conditioning] {ids(case_)} block {block} shifted {fam}: e_mean {e_mean[jm]:.2e} (its gate {g_mean[jm]:.2e}), '
              f'e_rstd {e_rstd[jr]:.2e} (its gate {g_rstd[jr]:.2e})')
        assert (e_mean[sel] <= g_mean[sel]).all() and (e_rstd[sel] <= g_rstd[sel]).all(), fam


@pytest.mark.parametrize('case_', ci.SHAPES, ids=ids)
def test_plain_fp32_sums_miss_the_gate_by_10x_at_large_kappa(case_):
    cols, flat, ref = case(*case_[:2])
    mean, rstd = ci.naive_stats(cols)
    _, e_rstd = ci.errors(mean, rstd, ref)
    g_rstd = np.max([ci.gate(ci.ROUTES[r], ref)[1] for r in case_[2]], 0)                      # the LOOSEST gate of the shape's routes, per column
    sel = np.array([k.name == 'kappa' and k.kappa >= 1e3 for k in flat])
    ratio = np.where(sel, e_rstd / g_rstd, 0.0)
    j = int(np.argmax(ratio))
    print(f'[conditioning] {ids(case_)} plain sums, worst kappa >= 1e3 channel ({flat[j].kappa:.0e}, std {flat[j].std}): e_rstd {e_rstd[j]:.2e} = '
          f'{ratio[j]:.1e} x its loosest gate {g_rstd[j]:.2e}')
    assert ratio[j] >= 10.0, (flat[j], e_rstd[j], g_rstd[j])


@pytest.mark.parametrize('shape', [(2, 4, 4, 64), (3, 16, 16, 128), (1, 32, 32, 8), (2, 32, 32, 4)])
def test_todays_inputs_do_not_tell_the_algorithms_apart(shape):
    """test_hip_ops.test_instnorm_stats at HW <= 1024: plain fp32 sums pass its 2e-5 rel-L2 gate on rstd (and so would any regression to them)"""
    cols = ci.columns(ci.today(shape, 3))
    ref = ci.reference(cols)
    _, rstd = ci.naive_stats(cols)
    rel_l2 = np.linalg.norm(rstd.astype(np.float64) - ref.rstd) / np.linalg.norm(ref.rstd)
    print(f'[conditioning] randn * 3 + 10 at {shape}: plain fp32 sums, rstd rel-L2 {rel_l2:.2e} (today\'s gate 2e-5)')
    assert shape[1] * shape[2] <= 1024 and rel_l2 < 2e-5


@pytest.mark.parametrize('act_hi', [0.0, 6.0])
@pytest.mark.parametrize('shape,per_image', ci.CONSUMER_SHAPES)
def test_consumer_inputs_keep_the_tie_mask_under_its_cap(shape, per_image, act_hi):
    """part 4 of the GPU file leaves out the elements whose fp64 pre-activation is within the forward bound of 0 (or 6): with the gamma and beta of
    ``consumer_case`` the fp64 restatement alone flags at most 2 % of any case (every seed the GPU file uses)"""
    for seed in (41, 43, 50, 60, 70, 80):
        cs = ci.consumer_case(shape, per_image, seed)
        frac = ci.tie_flags(cs, per_image, act_hi).mean()
        assert frac <= 0.02, (seed, frac)
        fam = {k.name for row in cs.kinds for k in row}
        assert fam == {'kappa', 'constant'} and max(k.kappa for row in cs.kinds for k in row) == 1e3
        assert np.isfinite(cs.scale).all() and np.isfinite(cs.shift).all()
