"""The norm-statistics kernels and their consumers on ILL-CONDITIONED inputs, per channel against fp64 (inputs, emulations and the derivation of
every bound: tests/conditioning_inputs.py; tests/test_norm_conditioning_cpu.py proves on the CPU that these inputs tell shifted sums + Chan merges
from plain fp32 sums: the latter miss the gate below by >= 10x at kappa >= 1e3).

PART 3, producers of (mean, rstd).  Every route runs on the four families (kappa up to 1e4 with both signs and std 1 | 1e-2, constant channels,
the row ramp, the far first row), every channel with its own condition, and is compared per (n, c) -- never through a norm over channels -- with
fp64 statistics of the fp32 tensor the statistics describe (for the conv routes: the y the launch wrote).  e_mean is in standard deviations,
e_rstd relative.  Gate per route (m, L, W), conditioning_inputs.gate:
    e_mean <= D u,  e_rstd <= [2 sqrt(W) D + (3 m + 3) R^2 / 2 + 2 W + L + 3] u,   D = D_lane + L (K + 3 R) + K,   u = 2^-24,
linear in K = max|x| / sigma_e >= kappa, from counting roundings (worst case, every one at half an ulp in the same direction), not from any result.
Constant channels are held to EXACT values instead: mean = the constant bit for bit, var = 0 (running_var under momentum 1), rstd = 1/sqrtf(eps).
scale is held to gamma rstd64 at the rstd gate; shift to beta - mean scale of the route's OWN mean and scale within two roundings (as a number of
its own it carries kappa times the error of rstd -- which cancels against x scale in every consumer); the running statistics start from random
values and are held to fp64 with the unbiased variance.  Routes and the kernel form each test asserts:
  1  lp_instnorm_stats            4, 16 and 1 splits of 64 pixels (workspace size), a 64-channel block boundary (C = 68), scalar loads (C % 4 != 0)
  2  lp_bn_train_stats            P = 16384 x C = 64 (256 partials per channel) and P = 256 (4): both finish in the one-wave form, which is the only
                                  one lp_bn_train_stats launches; the one-workgroup form (instnorm_finalize_kernel<4>, S >= 256) belongs to
                                  lp_norm_stats_finalize and runs in route 3 on the 256 row blocks of the flat 1x1 conv
  3  conv16(stats) + finalize     prec 1 and 2; the condition enters y through the bias (kappa_c x the measured std of the bias-free output), through the
                                  residual (the families themselves), and as zero activations + bias (every channel constant): 3x3, x2-upsampled 3x3,
                                  the flat 1x1 (BatchNorm, images == 1, running statistics), the conv_pipe.hip form (a fresh interpreter under
                                  LP_CONV_PIPE_MR=4, the knob of test_conv_pipe.py), and an 8 x 8 map whose statistics the wrapper must refuse (None):
                                  its fallback lp_instnorm_stats is then inside the gate
  4  gconv16(stats) + finalize    gconv_rows_kernel (C = 256, groups of 8) and groups of 32, which stay on conv_dma_kernel; the conv has neither bias
                                  nor residual, so the conditioned channels copy their input through a centre-tap weight (y = the operand-rounded x)
  5  MobileNet family             lp_bn_stats; lp_pwconv_fwd in its tiled and its 8-position form (asserted through lp_pwconv_stat_rows) and
                                  lp_dwconv3x3_stats_fwd with stride 1 and 2, each + lp_bn_finalize.  These return (scale, shift) only: a first call with
                                  gamma = 1, beta = 0, momentum = 1 reads rstd = scale, mean = running_mean, var = running_var (n - 1) / n; a second
                                  one with random gamma, beta and momentum 0.1 checks scale, shift and the running statistics.  The 1x1's condition
                                  enters through the weights of a constant input component, the depthwise one's through centre-tap weights.
kappa is measured from the fp64 output and printed with every line.

PART 4, consumers of (mean, rstd) at kappa <= 1e3 and on constant channels, element-wise against the fp64 restatements of tests/emu_ops.py fed
with the UNROUNDED fp64 statistics (the kernels get them rounded to fp32, so part 3's error is not inherited, and the cancellation x scale + shift /
cb x + cc is measured against the truth): act_pack pro 1 and pro 3 (prec 1), bn_add_act; adain_relu_bwd plain and with the 2x2 sum, norm_act_bwd
with mask modes 0 and 1, batch and frozen statistics, bn_bwd16 (prec 1).  Bounds (conditioning_inputs.forward_bound / backward_bounds):
    forward   2 u (|x scale| + |shift|) [+ 2^-16 |out| for bf16 hi + lo planes]
    backward  u |ca| {3 |g| + k (3 G2 + |xhat| G1) + (m + 27) |xhat| G2 + (m + 21) G1} + 2 u |dx|,   k = |mean| rstd
Elements whose fp64 pre-activation lies within the forward bound of 0 (or 6) are flagged from the restatement alone (cap 2 % per case), left out
of the dx comparison, and what they could add to the sums widens the other bounds.  On constant channels xhat = 0: dgamma = 0, dx = gamma rstd
(g - mean g) with rstd = 1/sqrt(eps).  OUT OF SCOPE: the 16-bit-resident inputs (X16, adain_act16, bn_act16) -- an fp16 plane rounds y at
kappa 2^-11 by construction.

MEASURED on one MI355X, per route the channel nearest its bound (value / its bound; every [parity] line prints its own pair):
  route                                              e_mean              e_rstd
  instnorm_stats                                     7.4e-4 / 1.1e-2     1.0e-7 / 3.9e-5
  bn_train_stats                                     9.2e-4 / 1.0e-2     1.7e-7 / 4.2e-5
  conv16 3x3 + finalize                              7.6e-4 / 2.8e-3     8.3e-8 / 3.9e-6
  conv16 x2-upsampled 3x3                            6.7e-4 / 3.0e-3     7.0e-8 / 4.5e-6
  conv16 flat 1x1, BatchNorm (finalize<4>)           4.9e-4 / 3.0e-3     7.7e-8 / 5.5e-6
  conv_pipe.hip form                                 9.9e-4 / 2.9e-3     7.7e-8 / 4.1e-6
  refused 8 x 8 map -> instnorm_stats                1.9e-4 / 1.0e-3     6.0e-8 / 5.9e-6
  gconv16 (both forms)                               6.1e-5 / 2.5e-4     1.2e-7 / 2.6e-5
  bn_batch_affine                                    9.5e-5 / 1.6e-3     7.4e-8 / 1.0e-4
  pwconv tiled / 8-position form                     1.0e-5 / 1.6e-4, 1.3e-5 / 1.1e-4     8.9e-8 / 1.1e-4, 7.3e-7 / 4.2e-4
  dwconv3x3_stats                                    1.5e-3 / 1.7e-2     8.2e-5 / 7.0e-2
  constant channels: exact on every route (37 checks).  Consumers, worst |err| / bound: act_pack 0.49, bn_add_act 0.75, adain_relu_bwd 0.13,
  norm_act_bwd 0.76, bn_bwd16 0.50; tie mask: no element flagged.
The mean bounds are met within a factor 3 .. 20, the rstd bounds within 50 .. 1400: their linear-in-K term assumes that the L roundings of a
partial mean all fall the same way and that every merge's d is wrong by twice that, while in fact d = mean_b - mean_a of neighbouring partials is
far smaller than the spread the Cauchy-Schwarz step allows.  Nothing was fitted: no route missed a bound.
FOUND: the conv_pipe.hip case gave NaN statistics for the last image in the fp16 mode -- conv_pipe_kernel walked CinP / 32 chunks and read a
padding chunk (Cin = 32 packed to CinP = 64) from beyond the pixel; fixed in the kernel (C8 / 32 chunks), see test_conv_pipe_form_statistics."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'latent_pose_reenactment_amd'))
import conditioning_inputs as ci  # noqa: E402
import emu_ops  # noqa: E402
from guarded_alloc import fence_fixture  # noqa: E402

pytestmark = pytest.mark.gpu
fenced_buffers = fence_fixture()

EPS = ci.EPS
U = ci.U


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def _lib():
    from latent_pose_reenactment_amd import _lib
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def names_of(kd, per_image):
    return [k.name for row in kd for k in row] if per_image else [k.name for k in kd[0]]


def check_stats(label, form, route, y, per_image, names, mean, rstd, *, eps=EPS, scale=None, shift=None, gamma=None, beta=None, run=None):
    """y: the fp32 tensor [N,H,W,C] the statistics describe; mean / rstd / scale / shift / gamma / beta: [N,C] (per image) or [C];
    names: family of every statistic; run: dict(rm0, rv0, rm, rv, momentum) of a running-statistics update.  Prints one [parity] line per family."""
    r = ci.ROUTES[route]
    ref = ci.reference(ci.columns(host(y).astype(np.float32), per_image), eps)
    mean, rstd = host(mean).reshape(-1), host(rstd).reshape(-1)
    assert mean.shape == ref.mean.shape, (label, mean.shape, ref.mean.shape)
    nonfinite = ~(np.isfinite(mean) & np.isfinite(rstd))
    assert not nonfinite.any(), (label, form, 'non-finite statistics at', np.nonzero(nonfinite)[0][:16], mean[nonfinite][:8], rstd[nonfinite][:8],
                                 'y finite:', bool(np.isfinite(host(y)).all()))
    e_mean, e_rstd = ci.errors(mean, rstd, ref)
    g_mean, g_rstd = ci.gate(r, ref)
    names = np.array(names)
    const = ref.var == 0
    assert (const == (names == 'constant')).all(), (label, 'the constant channels of y are not the ones the inputs name')
    bad = []
    for fam in sorted(set(names)):
        sel = names == fam
        if fam == 'constant':
            ok = (mean[sel] == ref.mean[sel]).all() and (rstd[sel] == float(ci.const_rstd(eps))).all()
            if run is not None and run['momentum'] == 1.0:
                ok = ok and (host(run['rv']).reshape(-1)[sel] == 0).all() and (host(run['rm']).reshape(-1)[sel] == ref.mean[sel]).all()
            print(f'[parity] {label} [{form}] constant channels ({int(sel.sum())}): mean bit-equal, var 0, rstd 1/sqrtf(eps): {"exact" if ok else "NOT EXACT"}')
            if not ok:
                bad.append((fam, mean[sel], rstd[sel]))
            continue
        jm, jr = (int(np.argmax(np.where(sel, e / np.maximum(g, 1e-300), -1.0))) for e, g in ((e_mean, g_mean), (e_rstd, g_rstd)))
        kap = ref.kappa[sel]
        print(f'[parity] {label} [{form}] {fam} (measured kappa <= {kap.max():.1e}): worst e_mean {e_mean[jm]:.2e} (bound {g_mean[jm]:.2e}), '
              f'worst e_rstd {e_rstd[jr]:.2e} (bound {g_rstd[jr]:.2e})')
        if not ((e_mean[sel] <= g_mean[sel]).all() and (e_rstd[sel] <= g_rstd[sel]).all()):
            bad.append((fam, e_mean[jm], g_mean[jm], e_rstd[jr], g_rstd[jr]))
    if scale is not None:
        sc, sh, ga, be = (host(t).reshape(-1) for t in (scale, shift, gamma, beta))
        want = ga * ref.rstd
        e_sc = np.abs(sc - want) / np.abs(want)
        b_sc = np.where(const, 4 * U, g_rstd + 2 * U)                           # (constant channels: gamma / sqrtf(eps), eps as fp32)
        own = be - mean * sc                                                    # the route's own mean and scale
        e_sh, b_sh = np.abs(sh - own), 2 * U * (np.abs(be) + np.abs(mean * sc))
        j1, j2 = int(np.argmax(e_sc / b_sc)), int(np.argmax(e_sh / np.maximum(b_sh, 1e-300)))
        print(f'[parity] {label} [{form}] scale: worst rel {e_sc[j1]:.2e} (bound {b_sc[j1]:.2e}); shift vs beta - mean scale: worst {e_sh[j2]:.2e} (bound {b_sh[j2]:.2e})')
        if not ((e_sc <= b_sc).all() and (e_sh <= b_sh).all()):
            bad.append(('scale / shift', e_sc[j1], b_sc[j1], e_sh[j2], b_sh[j2]))
    if run is not None and run['momentum'] != 1.0:
        mo, n = run['momentum'], ref.n
        rm0, rv0, rm, rv = (host(run[k]).reshape(-1) for k in ('rm0', 'rv0', 'rm', 'rv'))
        unb = ref.var * n / (n - 1)
        e_rm = np.abs(rm - ((1 - mo) * rm0 + mo * ref.mean))
        b_rm = mo * ref.sigma_e * g_mean + 4 * U * (np.abs((1 - mo) * rm0) + np.abs(mo * ref.mean))
        e_rv = np.abs(rv - ((1 - mo) * rv0 + mo * unb))
        b_rv = mo * 2 * g_rstd * ref.sigma_e ** 2 * n / (n - 1) + 4 * U * (np.abs((1 - mo) * rv0) + mo * unb)
        j1, j2 = int(np.argmax(e_rm / np.maximum(b_rm, 1e-300))), int(np.argmax(e_rv / np.maximum(b_rv, 1e-300)))
        print(f'[parity] {label} [{form}] running_mean: worst {e_rm[j1]:.2e} (bound {b_rm[j1]:.2e}); running_var (unbiased): worst {e_rv[j2]:.2e} (bound {b_rv[j2]:.2e})')
        if not ((e_rm <= b_rm).all() and (e_rv <= b_rv).all()):
            bad.append(('running statistics', e_rm[j1], b_rm[j1], e_rv[j2], b_rv[j2]))
    assert not bad, (label, form, bad)


def affine(st, seed):
    """gamma in [0.5, 1.5), beta ~ randn of shape st; random non-trivial running statistics"""
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*st, generator=g) + 0.5).cuda(), torch.randn(*st, generator=g).cuda(),
            (torch.randn(st[-1], generator=g) * 3).cuda(), (torch.rand(st[-1], generator=g) * 4 + 0.25).cuda())


# ---- route 1 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,splits', list(zip(ci.INSTNORM_SHAPES, (4, 16, 1))))
def test_instnorm_stats(shape, splits):
    ops = _ops()
    n, h, w, c = shape
    x, kd = ci.make(shape, seed=sum(shape))
    gamma, beta, _, _ = affine((n, c), 1)
    assert _lib().lp_instnorm_workspace_bytes(n, h * w, c) == n * splits * c * 12, 'the split of the pixels is not the one this case is about'
    xg = dev(x)
    m, r, sc, sh = ops.instnorm_stats(xg, gamma, beta, EPS)
    torch.cuda.synchronize()
    check_stats(f'instnorm_stats {shape}', f'{splits} x 64-pixel splits, one-wave finish', 'instnorm', xg, True, names_of(kd, True), m, r,
                scale=sc, shift=sh, gamma=gamma, beta=beta)


# ---- route 2 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,partials', list(zip(ci.BN_SHAPES, (256, 4))))
def test_bn_train_stats(shape, partials):
    ops = _ops()
    n, h, w, c = shape
    p = n * h * w
    x, kd = ci.make(shape, seed=sum(shape), per_image=False)
    gamma, beta, rm0, rv0 = affine((c,), 2)
    assert _lib().lp_bn_train_stats_workspace_bytes(p, c) == partials * c * 12
    xg = dev(x)
    names = names_of(kd, False)
    rm, rv = rm0.clone(), rv0.clone()
    m, r, sc, sh = ops.bn_train_stats(xg, gamma, beta, rm, rv, 0.1, EPS)
    torch.cuda.synchronize()
    form = f'{partials} partials per channel, one-wave finish'
    check_stats(f'bn_train_stats P={p} C={c}', form, 'instnorm', xg, False, names, m, r, scale=sc, shift=sh, gamma=gamma, beta=beta,
                run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=0.1))
    rm, rv = rm0.clone(), rv0.clone()
    m, r, _, _ = ops.bn_train_stats(xg, gamma, beta, rm, rv, 1.0, EPS)                 # momentum 1: the running statistics ARE the batch's
    torch.cuda.synchronize()
    check_stats(f'bn_train_stats P={p} C={c} momentum 1', form, 'instnorm', xg, False, names, m, r, run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=1.0))


# ---- route 3 ----------------------------------------------------------------------------------------------------------------------------------
KAPPA_SWEEP = ((0.0, 1.0), (1e2, -1.0), (1e3, 1.0), (1e4, -1.0), (1e2, 1.0), (1e3, -1.0), (1e4, 1.0))


def conv_case(label, form, geom, prec, mode, batchnorm, expect_rows):
    """geom = (N, H, W, Cin, Cout, ks, ups) with H x W the OUTPUT map.  mode 'bias': bias_c = kappa_c x the measured std of the bias-free output;
    'res': the families enter as the residual (weights x 1e-3, so that their own std stays the larger part); 'zero': zero activations + a bias
    from the three constants.  batchnorm: the flat 1x1 form (one image of all pixels, running statistics).  expect_rows None: the wrapper must
    refuse the statistics and the fallback route runs."""
    ops = _ops()
    n, h, w, cin, cout, ks, ups = geom
    g = torch.Generator().manual_seed(sum(geom) + prec)
    hin, win = (h // 2, w // 2) if ups else (h, w)
    x = torch.randn(n, hin, win, cin, generator=g).cuda()
    wt = (torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5).cuda()
    bias = res = None
    per_image = not batchnorm
    if mode == 'zero':
        x = torch.zeros_like(x)
        bias = torch.tensor([ci.CONSTANTS[j % 3] for j in range(cout)]).cuda()
        names = ['constant'] * (cout * (n if per_image else 1))
    elif mode == 'res':
        wt = wt * 1e-3
        r, kd = ci.make((n, h, w, cout), seed=sum(geom), per_image=per_image)
        res, names = dev(r), [nm + ' + conv' if nm == 'constant' else nm for nm in names_of(kd, per_image)]      # (no longer constant: an exact K ~ 1e6)
    a = ops.act_pack(x, pro=0, prec=prec)
    pk = ops.pack_weights(wt, 0, prec)
    nhw = (1,) + ops.flat_hw(n * h * w) if batchnorm else (n, h, w)
    run = lambda **kw: ops.conv16(ops.flat16(a) if batchnorm else a, pk, ksize=ks, upsample=bool(ups), prec=prec, stats=True, **kw)
    if mode == 'bias':
        y0, _ = run()
        std = y0.double().reshape(-1, cout).std(0)
        bias = torch.tensor([KAPPA_SWEEP[j % 7][0] * KAPPA_SWEEP[j % 7][1] for j in range(cout)], dtype=torch.float64).cuda().mul(std).float()
        names = ['bias kappa'] * (cout * (n if per_image else 1))
    y, cs = run(bias=bias, res=None if res is None else res.reshape(nhw + (cout,)))
    torch.cuda.synchronize()
    y4 = y.reshape(n, h, w, cout)
    st = (n, cout) if per_image else (cout,)
    gamma, beta, rm0, rv0 = affine(st, 3)
    label = f'{label} {geom} prec{prec} {mode}'
    if expect_rows is None:
        assert cs is None, f'{label}: this geometry has no fused statistics; the wrapper must say so'
        m, r, sc, sh = ops.instnorm_stats(y4, gamma, beta, EPS)
        torch.cuda.synchronize()
        check_stats(label, 'statistics refused (None) -> lp_instnorm_stats of y', 'instnorm', y4, True, names, m, r, scale=sc, shift=sh, gamma=gamma, beta=beta)
        return
    assert cs is not None and cs.rows == expect_rows and cs.images == (1 if batchnorm else n), (label, cs and (cs.rows, cs.images))
    form = f'{form}: {cs.rows} row blocks x {cs.images} image(s)'
    if not batchnorm:
        m, r, sc, sh = ops.norm_stats_finalize(cs, n, cout, gamma, beta, EPS)
        torch.cuda.synchronize()
        check_stats(label, form, 'conv', y4, True, names, m, r, scale=sc, shift=sh, gamma=gamma, beta=beta)
        return
    for mo in (0.1, 1.0):
        rm, rv = rm0.clone(), rv0.clone()
        m, r, sc, sh = ops.norm_stats_finalize(cs, 1, cout, gamma, beta, EPS, running_mean=rm, running_var=rv, momentum=mo)
        torch.cuda.synchronize()
        check_stats(f'{label} momentum {mo}', form, 'conv', y4, False, names, m, r, scale=sc, shift=sh, gamma=gamma, beta=beta,
                    run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=mo))


CONV_GEOMS = {  # name: (geometry, batchnorm, rows per image | None, kernel form)
    '3x3': ((2, 16, 16, 32, 64, 3, 0), False, 4, 'conv_dma_kernel 3x3'),
    '3x3 up2': ((2, 32, 32, 32, 64, 3, 1), False, 16, 'conv_dma_kernel x2-upsampled 3x3'),
    'flat 1x1': ((4, 64, 64, 64, 64, 1, 0), True, 256, 'conv_dma_kernel 1x1 on flat16, instnorm_finalize_kernel<4>'),
    'refused': ((1, 8, 8, 64, 64, 3, 0), False, None, ''),
}
PIPE_GEOM = ((2, 16, 16, 32, 128, 3, 0), False, 4, 'conv_pipe_kernel (LP_CONV_PIPE_MR=4)')


@pytest.mark.parametrize('mode', ['bias', 'res', 'zero'])
@pytest.mark.parametrize('prec', [1, 2])
@pytest.mark.parametrize('name', list(CONV_GEOMS))
def test_conv_epilogue_statistics(name, prec, mode):
    geom, batchnorm, rows, form = CONV_GEOMS[name]
    conv_case(name, form, geom, prec, mode, batchnorm, rows)


def test_conv_pipe_form_statistics():
    """conv_pipe.hip takes a 3x3 layer only where its tiling fills the chip; LP_CONV_PIPE_MR = 4 (read once per process) puts it on every eligible
    shape, the bf16x3 mode included: this file as a script in a fresh interpreter, under the same NaN-like fenced buffers as the tests here.
    Cin = 32 is packed to CinP = 64: conv_pipe_kernel used to walk CinP / 32 chunks and read the second one from the NEXT pixel's channels (the
    fence behind the planes at the last pixel) -- 0 x NaN pattern = NaN in y and in the statistics of the last image.  It now walks C8 / 32."""
    env = dict(os.environ, LP_CONV_PIPE_MR='4')
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and 'CONDITIONING_PIPE_OK' in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])


# ---- route 4 ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [1, 2])
@pytest.mark.parametrize('shape,cg,form', [((4, 16, 16, 256), 8, 'gconv_rows_kernel'), ((2, 16, 16, 64), 32, 'conv_dma_kernel, grouped (groups of 32)')])
def test_grouped_conv_statistics(shape, cg, form, prec):
    """the grouped conv has no bias and no residual: a conditioned channel copies its own input channel through a centre-tap weight of 1 (y = x as
    the operand planes hold it: 16 bits in bf16x3, 11 in fp16 -- the statistics describe that y); the kappa = 0 channels keep a full random
    3 x 3 x cg weight"""
    ops = _ops()
    n, h, w, c = shape
    x, kd = ci.make(shape, seed=sum(shape) + cg, per_image=False)
    g = torch.Generator().manual_seed(cg)
    wt = torch.zeros(c, cg, 3, 3)
    for j, k in enumerate(kd[0]):
        if k.name == 'kappa' and k.kappa == 0:
            wt[j] = torch.randn(cg, 3, 3, generator=g) / (cg * 9) ** 0.5
        else:
            wt[j, j % cg, 1, 1] = 1.0
    a = ops.act_pack(dev(x), pro=0, prec=prec)
    y, cs = ops.gconv16(a, ops.pack_grouped(wt.cuda(), 0, prec), prec=prec, stats=True)
    assert cs is not None and cs.rows == h * w // 64 and cs.images == n, (cs and (cs.rows, cs.images))
    gamma, beta, rm0, rv0 = affine((c,), 4)
    flat_var = host(y).reshape(-1, c).var(0)
    names = ['constant' if v == 0 else nm for v, nm in zip(flat_var, names_of(kd, False))]      # (fp16 planes round mean 100, std 0.01 to a constant)
    for mo in (0.1, 1.0):
        rm, rv = rm0.clone(), rv0.clone()
        m, r, sc, sh = ops.norm_stats_finalize(cs, 1, c, gamma, beta, EPS, running_mean=rm, running_var=rv, momentum=mo)
        torch.cuda.synchronize()
        check_stats(f'gconv16 {shape} groups of {cg} prec{prec} momentum {mo}', f'{form}: {cs.rows} row blocks x {cs.images} images', 'gconv', y, False,
                    names, m, r, scale=sc, shift=sh, gamma=gamma, beta=beta, run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=mo))


# ---- route 5 ----------------------------------------------------------------------------------------------------------------------------------
def mobilenet_check(label, form, route, y, names, finalize):
    """finalize(weight, bias, rm, rv, momentum) -> (scale, shift).  First call: gamma 1, beta 0, momentum 1 -> rstd = scale, mean = running_mean
    ((1 - 1) old + 1 mean: exact), var from running_var; second call: random affine, momentum 0.1."""
    c = y.shape[-1]
    gamma, beta, rm0, rv0 = affine((c,), 5)
    rm, rv = rm0.clone(), rv0.clone()
    sc, sh = finalize(torch.ones(c).cuda(), torch.zeros(c).cuda(), rm, rv, 1.0)
    torch.cuda.synchronize()
    mean, rstd = rm.clone(), sc.clone()
    check_stats(f'{label} momentum 1', form, route, y, False, names, mean, rstd, run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=1.0))
    rm, rv = rm0.clone(), rv0.clone()
    sc, sh = finalize(gamma, beta, rm, rv, 0.1)
    torch.cuda.synchronize()
    check_stats(label, form, route, y, False, names, mean, rstd, scale=sc, shift=sh, gamma=gamma, beta=beta,
                run=dict(rm0=rm0, rv0=rv0, rm=rm, rv=rv, momentum=0.1))


def test_bn_batch_affine():
    ops = _ops()
    shape = ci.CONV_BN_SHAPES[0]
    x, kd = ci.make(shape, seed=sum(shape) + 5, per_image=False)
    y = dev(x)
    mobilenet_check(f'bn_batch_affine {shape}', 'bn_partial_kernel (folded blocks) + bn_finalize_kernel', 'lp_bn_stats', y, names_of(kd, False),
                    lambda wg, b, rm, rv, mo: ops.bn_batch_affine(y, wg, b, rm, rv, mo, EPS))


@pytest.mark.parametrize('xshape,tiled', [((4, 32, 32, 16), True), ((1, 16, 16, 32), False)])
def test_pwconv_statistics(xshape, tiled):
    """input channel 0 is the constant 1, the others randn: w[c][0] = mean_c and w[c][1:] = std_c x a unit vector give y_c = mean_c + std_c randn with
    kappa_c under control; zero w[c][1:] with w[c][0] from the three constants gives the constant channels"""
    ops = _ops()
    n, h, wd, k = xshape
    cout, p = 64, n * h * wd
    rows = _lib().lp_pwconv_stat_rows(p, k, cout)
    assert rows == (p // 64 if tiled else p // 8), 'the other kernel form would run'
    g = torch.Generator().manual_seed(k)
    x = torch.randn(n, h, wd, k, generator=g)
    x[..., 0] = 1.0
    kd = ci.kinds(1, cout, False, ci.CONSUMER_CYCLE + tuple(kk for kk in ci.CYCLE if kk.name == 'kappa' and kk.kappa == 1e4))[0]
    wt = torch.zeros(cout, k)
    for j, kk in enumerate(kd):
        if kk.name == 'constant':
            wt[j, 0] = kk.value
        else:
            v = torch.randn(k - 1, generator=g)
            wt[j, 0], wt[j, 1:] = kk.sign * kk.kappa * kk.std, kk.std * v / v.norm()
    xg, wg = x.cuda(), wt.cuda()
    y, _, st = ops.pwconv(xg, wg, stats=True)
    assert st[1] == rows
    mobilenet_check(f'pwconv {xshape} -> {cout}', ('pwconv_kernel (64 x 64 tiles)' if tiled else 'pwconv_rows_kernel (8 positions)') + f': {rows} partial rows',
                    'pwconv' if tiled else 'pwconv_rows', y, [kk.name for kk in kd], lambda wg_, b, rm, rv, mo: ops.bn_finalize(st, wg_, b, rm, rv, mo, EPS))


@pytest.mark.parametrize('stride', [1, 2])
def test_dwconv_statistics(stride):
    """conditioned channels: centre-tap weight 1 (y = x, or its stride-2 subsample: row 0 stays); kappa = 0 channels: a full random 3 x 3 weight"""
    ops = _ops()
    shape = ci.CONV_BN_SHAPES[1]
    n, h, w, c = shape
    x, kd = ci.make(shape, seed=sum(shape) + stride, per_image=False)
    g = torch.Generator().manual_seed(stride)
    wt = torch.zeros(c, 3, 3)
    for j, k in enumerate(kd[0]):
        if k.name == 'kappa' and k.kappa == 0:
            wt[j] = torch.randn(3, 3, generator=g) / 3
        else:
            wt[j, 1, 1] = 1.0
    y, st = ops.dwconv3x3_stats(dev(x), wt.reshape(c, 9).cuda(), stride)
    assert st[1] == _lib().lp_dwconv_stat_rows(n, h, w, c, stride) and tuple(y.shape) == (n, h // stride, w // stride, c)
    mobilenet_check(f'dwconv3x3_stats {shape} stride {stride}', f'dwconv3x3_stats_kernel: {st[1]} partial rows', 'dwconv', y, names_of(kd, False),
                    lambda wg, b, rm, rv, mo: ops.bn_finalize(st, wg, b, rm, rv, mo, EPS))


# ---- part 4: consumers ---------------------------------------------------------------------------------------------------------------------------
T64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))


def consumer(per_image, seed):
    shape = ci.CONSUMER_SHAPES[0][0]
    cs = ci.consumer_case(shape, per_image, seed)
    fam = np.array(names_of(cs.kinds, per_image))
    gpu = {k: dev(getattr(cs, k)) for k in ('x', 'gamma', 'beta', 'mean', 'rstd', 'scale', 'shift')}          # statistics: fp64 rounded to fp32
    return cs, fam, gpu


def planes64(a):
    """bf16 hi + lo operand planes -> fp64"""
    return (a.hi.view(torch.bfloat16).double() + a.lo.view(torch.bfloat16).double())[..., :a.c].cpu().numpy()


def report_elements(label, form, got, want, bound, fam_elem, skip=None):
    """worst |err| / bound per family over the elements not in ``skip``"""
    err = np.abs(got - want)
    assert np.isfinite(got).all(), label
    keep = np.ones(err.shape, bool) if skip is None else ~skip
    bad = []
    for fam in sorted(set(fam_elem.reshape(-1))):
        sel = (fam_elem == fam) & keep
        ratio = np.where(sel, err / np.maximum(bound, 1e-300), 0.0)
        j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print(f'[parity] {label} [{form}] {fam}: worst |err| / bound {ratio[j]:.3f} (|err| {err[j]:.2e}, bound {bound[j]:.2e})')
        if ratio[j] > 1.0:
            bad.append((fam, err[j], bound[j]))
    assert not bad, (label, bad)


def elem_family(fam, shape, per_image):
    n, h, w, c = shape
    f = fam.reshape(n, c) if per_image else np.broadcast_to(fam, (n, c))
    return np.broadcast_to(f[:, None, None, :], shape)


@pytest.mark.parametrize('pro', [1, 3])
def test_act_pack_forward(pro):
    ops = _ops()
    per_image = pro == 1
    cs, fam, gpu = consumer(per_image, 40 + pro)
    a = ops.act_pack(gpu['x'], pro=pro, scale=gpu['scale'], shift=gpu['shift'], prec=1)
    torch.cuda.synchronize()
    want = emu_ops.act_pack(T64(cs.x), pro=pro, scale=T64(cs.scale), shift=T64(cs.shift)).hi.numpy()
    bound = ci.forward_bound(cs, per_image) + 2.0 ** -16 * np.abs(want)
    report_elements(f'act_pack pro={pro} prec1', 'per-image affine + ReLU' if pro == 1 else 'per-channel affine + ReLU6', planes64(a), want, bound,
                    elem_family(fam, cs.x.shape, per_image))


@pytest.mark.parametrize('relu', [True, False])
def test_bn_add_act_forward(relu):
    ops = _ops()
    cs, fam, gpu = consumer(False, 50)
    res = np.random.RandomState(51).standard_normal(cs.x.shape).astype(np.float32)
    out = ops.bn_add_act(gpu['x'], gpu['scale'], gpu['shift'], res=dev(res), relu=relu)
    torch.cuda.synchronize()
    want = emu_ops.bn_add_act(T64(cs.x), T64(cs.scale), T64(cs.shift), res=T64(res), relu=relu).numpy()
    pre = cs.x.astype(np.float64) * cs.scale + cs.shift + res
    bound = ci.forward_bound(cs, False) + U * np.abs(pre)                       # + the rounding of the residual add
    report_elements(f'bn_add_act relu={relu}', 'fp32 out', host(out), want, bound, elem_family(fam, cs.x.shape, False))


def backward_case(label, form, cs, fam, per_image, dA, run, *, mask_mode=0, act_hi=0.0, frozen=False, ups=False, plane_rounding=0.0):
    """run() -> (dx, dgamma, dbeta) as fp64 numpy.  Restatement: emu_ops with the unrounded fp64 statistics."""
    x64 = T64(cs.x)
    tt = lambda v: T64(v)
    if per_image:
        assert mask_mode == 0 and act_hi == 0.0 and not frozen
        dxw, dgw, dbw = (t.numpy() for t in emu_ops.adain_relu_bwd(T64(dA), x64, None, tt(cs.gamma), tt(cs.mean), tt(cs.rstd), tt(cs.scale), tt(cs.shift), ups))
    else:
        dxw, dgw, dbw, _ = emu_ops.norm_act_bwd(T64(dA), x64, tt(cs.gamma), tt(cs.mean), tt(cs.rstd), tt(cs.scale), tt(cs.shift), mask_mode=mask_mode,
                                               act_hi=act_hi, frozen=frozen)
        dxw, dgw, dbw = dxw.numpy(), dgw.numpy(), dbw.numpy()
    n, h, w, c = cs.x.shape
    d64 = dA.astype(np.float64)
    g_abs = None
    if ups:
        g_abs = np.abs(d64).reshape(n, h, 2, w, 2, c).sum((2, 4))
        d64 = d64.reshape(n, h, 2, w, 2, c).sum((2, 4))
    pe = lambda v: ci.per_element(v, per_image)
    pre = cs.x.astype(np.float64) * pe(cs.scale) + pe(cs.shift)
    flagged = None
    if mask_mode == 0:
        flagged = ci.tie_flags(cs, per_image, act_hi)
        frac = flagged.mean()
        print(f'[parity] {label} [{form}] tie mask: {frac:.4%} of the elements (cap 2 %)')
        assert frac <= 0.02
        mask = (pre > 0) & ((pre < act_hi) if act_hi > 0 else True)
        d64 = d64 * mask
        if g_abs is not None:
            g_abs = g_abs * (mask | flagged)
    xhat = (cs.x.astype(np.float64) - pe(cs.mean)) * pe(cs.rstd)
    b_dx, b_dg, b_db = ci.backward_bounds(cs, per_image, d64, xhat, dxw, 4, frozen=frozen, g_abs=g_abs, flagged=flagged)
    b_dx = b_dx + plane_rounding * np.abs(dxw)
    b_dg, b_db = b_dg + U * np.abs(dgw), b_db + U * np.abs(dbw)
    dx, dg, db = run()
    fe = elem_family(fam, cs.x.shape, per_image)
    report_elements(f'{label} dx', form, dx, dxw, b_dx, fe, skip=flagged)
    report_elements(f'{label} dgamma', form, dg.reshape(fam.shape), dgw.reshape(fam.shape), np.broadcast_to(b_dg, dgw.shape).reshape(fam.shape), fam)
    report_elements(f'{label} dbeta', form, db.reshape(fam.shape), dbw.reshape(fam.shape), np.broadcast_to(b_db, dbw.shape).reshape(fam.shape), fam)
    const = fam == 'constant'
    assert (dg.reshape(fam.shape)[const] == 0).all(), 'xhat = 0 on a constant channel: dgamma = 0'


@pytest.mark.parametrize('ups', [False, True])
def test_adain_relu_bwd(ups):
    ops = _ops()
    cs, fam, gpu = consumer(True, 60)
    n, h, w, c = cs.x.shape
    dA = np.random.RandomState(61 + ups).standard_normal((n, h << ups, w << ups, c)).astype(np.float32)

    def run():
        dgb = torch.empty(2, n, c, device='cuda')
        dx = ops.adain_relu_bwd(dev(dA), gpu['x'], None, gpu['gamma'], gpu['mean'], gpu['rstd'], gpu['scale'], gpu['shift'], dgb[0], dgb[1], ups)
        torch.cuda.synchronize()
        return host(dx), host(dgb[0]), host(dgb[1])
    backward_case(f'adain_relu_bwd ups={int(ups)}', 'adain_bwd kernels, fp32 x' + (', 2x2 sum of dA' if ups else ''), cs, fam, True, dA, run, ups=ups)


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('mask_mode,act_hi', [(0, 0.0), (0, 6.0), (1, 0.0)])
def test_norm_act_bwd(mask_mode, act_hi, frozen):
    ops = _ops()
    cs, fam, gpu = consumer(False, 70)
    dA = np.random.RandomState(71).standard_normal(cs.x.shape).astype(np.float32)

    def run():
        dx, dg, db, _ = ops.norm_act_bwd(dev(dA), gpu['x'], gpu['gamma'], gpu['mean'], gpu['rstd'], gpu['scale'], gpu['shift'], mask_mode=mask_mode,
                                         act_hi=act_hi, frozen=frozen)
        torch.cuda.synchronize()
        return host(dx), host(dg), host(db)
    backward_case(f'norm_act_bwd mask {mask_mode} act_hi {act_hi} frozen {int(frozen)}', 'adain_bwd kernels, one image of P pixels', cs, fam, False, dA, run,
                  mask_mode=mask_mode, act_hi=act_hi, frozen=frozen)


@pytest.mark.parametrize('frozen', [False, True])
@pytest.mark.parametrize('mask_mode', [0, 1])
def test_bn_bwd16(mask_mode, frozen):
    ops = _ops()
    cs, fam, gpu = consumer(False, 80)
    dA = np.random.RandomState(81).standard_normal(cs.x.shape).astype(np.float32)

    def run():
        d16, dg, db, _ = ops.bn_bwd16(dev(dA), gpu['x'], gpu['gamma'], gpu['mean'], gpu['rstd'], gpu['scale'], gpu['shift'], prec=1, mask_mode=mask_mode,
                                      frozen=frozen)
        torch.cuda.synchronize()
        assert d16.inv is None and d16.lo is not None
        return planes64(d16), host(dg), host(db)
    backward_case(f'bn_bwd16 prec1 mask {mask_mode} frozen {int(frozen)}', 'bn_bwd16 kernels (rows form of the apply pass), bf16 hi + lo planes', cs, fam,
                  False, dA, run, mask_mode=mask_mode, frozen=frozen, plane_rounding=2.0 ** -16)


if __name__ == '__main__':          # the conv_pipe.hip form: test_conv_pipe_form_statistics starts this under LP_CONV_PIPE_MR=4
    import guarded_alloc
    assert os.environ.get('LP_CONV_PIPE_MR') == '4'
    geom_, bn_, rows_, form_ = PIPE_GEOM
    with guarded_alloc.Guarded() as fences_:          # as the module's fixture: fresh buffers are NaN-like and fenced
        for prec_ in (1, 2):
            for mode_ in ('bias', 'res', 'zero'):
                conv_case('3x3', form_, geom_, prec_, mode_, bn_, rows_)
        torch.cuda.synchronize()
        fences_.check_guards()
    print('CONDITIONING_PIPE_OK')
