"""Ill-conditioned inputs for the norm-statistics kernels, two fp32 emulations of a per-channel variance, and the gate the GPU routes are
held to (tests/test_norm_conditioning_cpu.py proves that the inputs discriminate, tests/test_norm_conditioning_gpu.py runs the kernels).
No GPU, numpy only.

INPUTS.  NHWC fp32 tensors in which EVERY CHANNEL HAS ITS OWN CONDITION, so one tensor carries the whole sweep and a per-channel failure cannot
hide in a norm over channels.  kappa = |mean| / std.  The channel kinds cycle through CYCLE (13 entries; the first six hold one of every kind, so
that a tensor of 6 channels still has them all; with ``per_image`` image n starts the cycle 5 entries later):
  kappa      mean + std * randn, kappa in {0, 1e2, 1e3, 1e4}, both signs of the mean, std in {1, 1e-2} (with eps = 1e-4 the sum var + eps is
             variance-dominated in the first and eps-dominated in the second)
  constant   one value everywhere, from {0, +0.75, -1234.5} (a dead ReLU channel; a conv of a zero input = its bias).  Expected EXACTLY:
             mean = the value bit for bit, M2 = var = 0, rstd = 1/sqrtf(eps).  The three values have short mantissas: sums of up to 2^12 of them
             are exact in fp32, so the exactness also holds for the kernels that sum before they subtract (the two-pass 1x1-conv epilogues).
  ramp       image row y holds 10 y + 0.01 randn: every 64-pixel partial is nearly constant and the partials lie far apart -- the d^2 term of
             every merge level carries the whole variance
  first_far  the first image row is 0, the rest 1e3 + randn: the shift reference of the lanes that start there is an outlier (benign by
             arithmetic -- the outliers raise the variance -- but it is the `first value is the reference` branch with a bad reference)

EMULATIONS (of arithmetic, not of kernel code; section 2 of the CPU test is their only user):
  naive_stats    running fp32 sums of x and x^2, var = E[x^2] - E[x]^2
  shifted_stats  blocks of ``block`` pixels; 16 strided lanes per block, each with fp32 sums of d = x - (the lane's first value) and d^2; the
                 lanes merged with Chan's formula in fp32; the blocks finished in fp64 about one reference; var rounded to fp32, rstd in fp32

GATE.  u = 2^-24.  Per channel, from the fp64 statistics of the fp32 tensor (properties of the INPUT, never of a kernel's result):
  sigma_e = max(std, sqrt(eps)),  K = max|x| / sigma_e (>= kappa),  R = (max x - min x) / sigma_e,
  e_mean = |mean - mean64| / sigma_e   (in standard deviations: the error xhat sees),   e_rstd = |rstd - rstd64| / rstd64.
A route is (m, L, W): m elements per first-stage partial, L fp32 Chan merges on the longest dependency chain behind it, W = the sum over ALL merges
(the fp64 finish counted as one stage) of n_a n_b / (n_ab n).  First-order worst-case counting, every rounding at its largest:
  lane    d = x - ref and the m-term sum of d round at <= u |partial sum| <= u k R sigma_e;  sd / m and ref + sd / m each round once more, the
          last one at |mean|:                                               D_lane = (m/2 + 2) R + K           [in u sigma_e]
          (two-pass epilogues -- sum, mean, then sum (x - mean)^2: the sum rounds at the size of x itself:       D_lane = ((m + 1)/2 + 1) K)
  merge   mean_a += d n_b / n: d, the quotient and the product round at <= u |d| <= u R sigma_e each, the sum at u |mean|; the inputs' errors enter
          as a convex combination:                                          + (K + 3 R) per merge level
  store   the fp32 rounding of the finished mean:                           + K
  ==>     e_mean <= D u,   D = D_lane + L (K + 3 R) + K
  M2      a merge adds w d^2, w = n_a n_b / n_ab, with d wrong by <= 2 D u sigma_e:  sum_k w_k 2 |d_k| 2 D u sigma_e.  The w_k d_k^2 of all merges add
          up to the between-partials sum of squares <= n std^2, so by Cauchy-Schwarz  sum w |d| <= sqrt(sum w) sqrt(n std^2) = n std sqrt(W):
          relative to n sigma_e^2 that is 4 sqrt(W) D u -- LINEAR in K, through the rounding of partial means near |mean| before their differences
          are taken, and never quadratic.  The products d d w round 4 times (4 W u in all), every M2 accumulation twice per level (2 L u).
          lane: sq = sum d^2 (m fma, d^2 carries 2 u) and sd^2 / m (2 (m - 1) u through sd, 3 u of its own), both <= sum d^2 <= m R^2 sigma_e^2:
          (3 m + 3) R^2 u  (two-pass: (m + 2) R^2 u, plus the second-order m (D_lane u sigma_e)^2 of a mean that is off)
  rstd    = (var + eps)^-1/2 halves the relative error of var + eps >= sigma_e^2; var -> fp32, + eps, sqrtf and the division round once each
  ==>     e_rstd <= [2 sqrt(W) D + (3 m + 3) R^2 / 2 + 2 W + L + 3] u   (+ (D_lane u)^2 / 2 for the two-pass epilogues)
i.e. the form a u + b K u with b = 2 sqrt(W) (L + 2) and a from R (7 .. 8 for 10^3 .. 10^4 gaussian samples, sqrt(12) for the ramp).  The bound is a
worst case -- every rounding at half an ulp and in the same direction -- so typical results sit two to three orders below it; what it separates
is linear from quadratic growth in kappa: plain fp32 sums err by ~ kappa^2 u and miss it by orders at kappa >= 1e3 (asserted on the CPU)."""
from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
EPS = 1e-4


class Kind(NamedTuple):
    name: str                 # 'kappa' | 'constant' | 'ramp' | 'first_far'
    kappa: float = 0.0        # nominal |mean| / std (kappa kinds)
    std: float = 1.0
    sign: float = 1.0
    value: float = 0.0        # constant kinds


CYCLE = (Kind('kappa', 1e4, 1.0, -1.0), Kind('constant', value=-1234.5), Kind('ramp'), Kind('first_far'), Kind('kappa', 1e4, 1e-2, 1.0),
         Kind('constant', value=0.0),
         Kind('kappa', 0.0, 1.0, 1.0), Kind('kappa', 1e2, 1.0, 1.0), Kind('kappa', 1e3, 1.0, -1.0), Kind('constant', value=0.75),
         Kind('kappa', 0.0, 1e-2, 1.0), Kind('kappa', 1e2, 1e-2, -1.0), Kind('kappa', 1e3, 1e-2, 1.0))
CONSTANTS = (0.0, 0.75, -1234.5)


# the consumers' x (part 4): kappa <= 1e3 and the constants
CONSUMER_CYCLE = tuple(k for k in CYCLE if (k.name == 'kappa' and k.kappa <= 1e3) or k.name == 'constant')
CONSUMER_SHAPES = (((2, 16, 16, 16), True), ((2, 16, 16, 16), False))       # AdaIN (per image) and BatchNorm (P = 512) consumers


# every (shape, per_image, routes) on which the GPU file puts these families; the CPU file proves each of them discriminates at its routes' gates
INSTNORM_SHAPES = ((2, 16, 16, 8), (1, 32, 32, 68), (2, 8, 8, 6))       # 4, 16 and 1 splits of 64 pixels; a 64-channel block boundary; C % 4 != 0
BN_SHAPES = ((4, 64, 64, 64), (1, 16, 16, 64))                          # P = 16384 (256 partials per channel) and P = 256
CONV_SHAPES = ((2, 16, 16, 64), (2, 32, 32, 64), (2, 16, 16, 128), (1, 8, 8, 64))       # the residual of the conv-epilogue routes (per image); the last one falls back
CONV_BN_SHAPES = ((4, 16, 16, 64), (2, 16, 16, 64), (4, 16, 16, 256))      # ... of the BatchNorm conv routes (with BN_SHAPES[0]); the MobileNet family; the grouped conv
SHAPES = (tuple((s, True, ('instnorm',)) for s in INSTNORM_SHAPES) + tuple((s, True, ('instnorm', 'conv')) for s in CONV_SHAPES) +
          ((BN_SHAPES[0], False, ('instnorm', 'conv')), (BN_SHAPES[1], False, ('instnorm',))) +
          tuple((s, False, ('instnorm', 'conv', 'gconv', 'lp_bn_stats', 'pwconv', 'pwconv_rows', 'dwconv')) for s in CONV_BN_SHAPES))


def kinds(n, c, per_image=True, cycle=CYCLE):
    """[n][c] -> Kind.  per_image=False: the condition belongs to the channel alone (BatchNorm: statistics over all images)"""
    return [[cycle[(j + (5 * i if per_image else 0)) % len(cycle)] for j in range(c)] for i in range(n)]


def fill(kind, h, w, rng):
    """one [h, w] fp32 plane of ``kind``"""
    z = rng.standard_normal((h, w))
    if kind.name == 'kappa':
        v = kind.sign * kind.kappa * kind.std + kind.std * z
    elif kind.name == 'constant':
        v = np.full((h, w), kind.value)
    elif kind.name == 'ramp':
        v = 10.0 * np.arange(h)[:, None] + 0.01 * z
    elif kind.name == 'first_far':
        v = 1e3 + z
        v[0] = 0.0
    else:
        raise ValueError(kind.name)
    return v.astype(np.float32)


def make(shape, seed, per_image=True, cycle=CYCLE):
    """-> (x fp32 [N,H,W,C], kinds [N][C])"""
    n, h, w, c = shape
    rng = np.random.RandomState(seed)
    kd = kinds(n, c, per_image, cycle)
    x = np.empty(shape, np.float32)
    for i in range(n):
        for j in range(c):
            x[i, :, :, j] = fill(kd[i][j], h, w, rng)
    return x, kd


def today(shape, seed):
    """the inputs of test_hip_ops.test_instnorm_stats: randn * 3 + 10"""
    return (np.random.RandomState(seed).standard_normal(shape) * 3 + 10).astype(np.float32)


def columns(x, per_image=True):
    """[N,H,W,C] -> [P, K]: one column per statistic -- (n, c) with ``per_image``, else c over all images"""
    n, h, w, c = x.shape
    if per_image:
        return np.ascontiguousarray(x.reshape(n, h * w, c).transpose(1, 0, 2).reshape(h * w, n * c))
    return x.reshape(n * h * w, c)


class Ref(NamedTuple):
    """fp64 statistics of the fp32 columns [P, K] and the input properties the gate is made of"""
    n: int
    mean: np.ndarray
    var: np.ndarray           # biased
    rstd: np.ndarray
    sigma_e: np.ndarray
    K: np.ndarray             # max|x| / sigma_e
    R: np.ndarray             # range / sigma_e
    kappa: np.ndarray         # |mean| / std (inf for a constant channel that is not 0)


def reference(cols, eps=EPS):
    x = cols.astype(np.float64)
    mean, var = x.mean(0), x.var(0)
    se = np.maximum(np.sqrt(var), np.sqrt(eps))
    with np.errstate(divide='ignore', invalid='ignore'):
        kappa = np.where(var > 0, np.abs(mean) / np.sqrt(var), np.where(mean != 0, np.inf, 0.0))
    return Ref(x.shape[0], mean, var, 1.0 / np.sqrt(var + eps), se, np.abs(x).max(0) / se, (x.max(0) - x.min(0)) / se, kappa)


def errors(mean, rstd, ref):
    """-> (e_mean in standard deviations, relative e_rstd), per column"""
    return np.abs(np.asarray(mean, np.float64) - ref.mean) / ref.sigma_e, np.abs(np.asarray(rstd, np.float64) - ref.rstd) / ref.rstd


class Route(NamedTuple):
    name: str
    m: int                    # elements per first-stage partial (the largest the route's launch shapes give)
    L: int                    # fp32 Chan merges on the longest dependency chain
    W: float                  # sum over all merges of n_a n_b / (n_ab n), the fp64 finish counted as 1
    two_pass: bool = False    # first stage: sum -> mean -> sum (x - mean)^2 instead of shifted sums


def gate(route, ref):
    """-> (bound on e_mean, bound on e_rstd) per column: the module docstring's derivation"""
    m, L, W = route.m, route.L, route.W
    d_lane = ((m + 1) / 2 + 1) * ref.K if route.two_pass else (m / 2 + 2) * ref.R + ref.K
    D = d_lane + L * (ref.K + 3 * ref.R) + ref.K
    lane_m2 = (m + 2) * ref.R ** 2 / 2 + (d_lane * U) ** 2 / 2 / U if route.two_pass else (3 * m + 3) * ref.R ** 2 / 2
    return D * U, (2 * np.sqrt(W) * D + lane_m2 + 2 * W + L + 3) * U


# (m, L, W) per route, read off the kernels' reduction structure at the launch shapes the GPU file uses (all within SHAPES):
ROUTES = {
    # instnorm_partial_kernel at the 64-pixel split: 16 lanes x 4 pixels, the lanes chained by one thread (15 merges, weights <= 1 in all); the
    # finish of the splits is fp64 (instnorm_finalize_kernel, either form): one more stage
    'instnorm': Route('lp_instnorm_stats / lp_bn_train_stats', 4, 15, 2.0),
    # conv16_epilogue: a lane owns 4 channels and every RPP-th row of its wave's <= 128 rows (RPP = 4 | 8: <= 32 rows), the RPP lanes merge by
    # a balanced butterfly (<= 3 levels of weight 1/4), lp_norm_stats_finalize is the fp64 finish
    'conv': Route('conv16 epilogue + lp_norm_stats_finalize', 32, 3, 1.75),
    # gconv_rows_kernel / the grouped conv_dma_kernel: 16 pixels per lane, a two-level butterfly, the fp64 finish
    'gconv': Route('gconv16 epilogue + lp_norm_stats_finalize', 16, 2, 1.5),
    # bn_partial_kernel: <= 9 float4 per thread (8 + a tail) while P C / 4 <= 2^20, the block's BT / G4 <= 16 threads of a group chained (15);
    # bn_finalize_kernel is fp32 throughout: <= 2 partials chained per thread (1), a 6-level shuffle tree (weight 6/4), 3 waves chained (3)
    'lp_bn_stats': Route('lp_bn_stats', 9, 25, 4.5),
    # pwconv_kernel: two-pass over 16 positions, 4 threads chained (3); bn_finalize_kernel as above
    'pwconv': Route('lp_pwconv_fwd (64 x 64 tiles) + lp_bn_finalize', 16, 13, 4.5, True),
    # pwconv_rows_kernel: two-pass over its 8 positions by one lane; bn_finalize_kernel
    'pwconv_rows': Route('lp_pwconv_fwd (8-position form) + lp_bn_finalize', 8, 10, 3.5, True),
    # dwconv3x3_stats_kernel: bn_partial_kernel's shape with <= 5 float4 per thread (4 + a tail; <= 1024 blocks: <= 4 partials chained per
    # finalize thread, 3 merges)
    'dwconv': Route('lp_dwconv3x3_stats_fwd + lp_bn_finalize', 5, 27, 4.5),
}


# the emulation's own structure: 16 lanes chained (L = 15, W <= 1) + the fp64 finish (W = 1)
def emulation_route(block):
    return Route('shifted emulation', max(1, block // 16), 15, 2.0)


def rstd_f32(var, eps):
    var = np.maximum(np.asarray(var, np.float32), np.float32(0))
    return np.float32(1) / np.sqrt(var + np.float32(eps), dtype=np.float32)


def const_rstd(eps):
    """1/sqrtf(eps): the rstd of a constant channel, to the bit"""
    return np.float32(1) / np.sqrt(np.float32(eps), dtype=np.float32)


def naive_stats(cols, eps=EPS):
    """running fp32 sums of x and x^2 (np.cumsum adds in order, in the array's type) -> (mean, rstd) fp32"""
    x = np.asarray(cols, np.float32)
    n = np.float32(x.shape[0])
    s = np.cumsum(x, axis=0, dtype=np.float32)[-1]
    q = np.cumsum(x * x, axis=0, dtype=np.float32)[-1]
    mean = s / n
    return mean, rstd_f32(q / n - mean * mean, eps)


def chan_merge_f32(na, ma, qa, nb, mb, qb):
    n = np.float32(na + nb)
    d = mb - ma
    return n, ma + d * (np.float32(nb) / n), qa + (qb + d * d * (np.float32(na) * np.float32(nb) / n))


def shifted_stats(cols, eps=EPS, block=1024, lanes=16):
    """shifted lane sums in fp32, Chan merge of the lanes in fp32, fp64 finish of the blocks -> (mean, rstd) fp32"""
    x = np.asarray(cols, np.float32)
    p = x.shape[0]
    parts = []
    for b0 in range(0, p, block):
        xb = x[b0:b0 + block]
        acc = None
        for l in range(min(lanes, xb.shape[0])):
            xl = xb[l::lanes]
            cnt = np.float32(xl.shape[0])
            d = xl - xl[0]
            sd = np.cumsum(d, axis=0, dtype=np.float32)[-1]
            sq = np.cumsum(d * d, axis=0, dtype=np.float32)[-1]
            lane = (cnt, xl[0] + sd / cnt, sq - sd * sd / cnt)
            acc = lane if acc is None else chan_merge_f32(*acc, *lane)
        parts.append(acc)
    ref = parts[0][1].astype(np.float64)
    nn = sum(float(a[0]) for a in parts)
    s1 = sum(float(a[0]) * (a[1].astype(np.float64) - ref) for a in parts)
    s2 = sum(a[2].astype(np.float64) + float(a[0]) * (a[1].astype(np.float64) - ref) ** 2 for a in parts)
    m2 = np.maximum(s2 - s1 * s1 / nn, 0.0)
    return (ref + s1 / nn).astype(np.float32), rstd_f32((m2 / nn).astype(np.float32), eps)


# ---- consumers of (mean, rstd): inputs, the tie rule and the bounds (part 4 of the GPU file) --------------------------------------------------
class Consumer(NamedTuple):
    """fp64 inputs of a norm consumer; statistics in the layout of the route ([N, C] per image, [C] for a BatchNorm)"""
    x: np.ndarray             # fp32 [N,H,W,C]
    kinds: list
    gamma: np.ndarray
    beta: np.ndarray
    mean: np.ndarray          # fp64 statistics of x; the kernels get them rounded to fp32
    rstd: np.ndarray
    scale: np.ndarray         # gamma rstd
    shift: np.ndarray         # beta - mean gamma rstd
    kappa_r: np.ndarray       # |mean| rstd: kappa where the variance dominates eps, |mean| / sqrt(eps) for a constant channel


def consumer_case(shape, per_image, seed, eps=EPS):
    """x from CONSUMER_CYCLE; gamma in [0.5, 1.5); |beta| in [0.5, 1.5) with random sign, so that a constant channel (pre-activation = beta
    everywhere) is never inside the tie band and the fp64 restatement alone keeps the tie mask far under its 2 % cap (asserted on the CPU)"""
    x, kd = make(shape, seed, per_image, CONSUMER_CYCLE)
    n, c = shape[0], shape[3]
    rng = np.random.RandomState(seed + 1)
    st = (n, c) if per_image else (c,)
    gamma = (0.5 + rng.rand(*st)).astype(np.float32).astype(np.float64)
    beta = ((0.5 + rng.rand(*st)) * np.where(rng.rand(*st) < 0.5, -1.0, 1.0)).astype(np.float32).astype(np.float64)
    x64 = x.astype(np.float64)
    ax = (1, 2) if per_image else (0, 1, 2)
    mean, var = x64.mean(ax), x64.var(ax)
    rstd = 1.0 / np.sqrt(var + eps)
    return Consumer(x, kd, gamma, beta, mean, rstd, gamma * rstd, beta - mean * gamma * rstd, np.abs(mean) * rstd)


def per_element(v, per_image):
    """statistics [N, C] | [C] -> broadcastable against [N,H,W,C]"""
    return v[:, None, None, :] if per_image else v


def forward_bound(cs, per_image):
    """|fma(x, scale32, shift32) - (x scale + shift)| <= 2 u (|x scale| + |shift|): scale and shift reach the kernel rounded to fp32 (u each,
    at the size of the two terms that cancel: kappa gamma), the fma rounds once at the size of the result"""
    sc, sh = per_element(cs.scale, per_image), per_element(cs.shift, per_image)
    return 2 * U * (np.abs(cs.x.astype(np.float64) * sc) + np.abs(sh))


def tie_flags(cs, per_image, act_hi=0.0):
    """elements whose fp64 pre-activation lies within the forward bound of 0 (or of act_hi): the sign of the fp32 fma there is not the
    restatement's to decide.  From the restatement alone."""
    a = cs.x.astype(np.float64) * per_element(cs.scale, per_image) + per_element(cs.shift, per_image)
    b = forward_bound(cs, per_image)
    f = np.abs(a) <= b
    return f | (np.abs(a - act_hi) <= b) if act_hi > 0 else f


def backward_bounds(cs, per_image, g, xhat, dx, m, frozen=False, g_abs=None, flagged=None):
    """-> (bound of dx per element, of dgamma, of dbeta per statistic).  g: the masked incoming gradient (fp64), P elements per statistic;
    m + 15 fp32 additions sit on the longest path of the two sums (m per lane of a 64-pixel split, 16 lanes chained; the splits merge in fp64).
    With k = |mean| rstd, G1 = sum|g| / P, G2 = sum|g xhat| / P, ca = gamma rstd:
      xhat   (x - fl(mean)) fl(rstd): u |mean| rstd from the rounded mean, 3 u |xhat| from the subtraction, rstd and the product
      S1     (m + 15) u sum|g|;      S2  u [k sum|g| + (m + 19) sum|g xhat|]
      ca     2 u;   cb = -ca rstd S2 / P: 7 u |cb| + |ca rstd / P| dS2;   cc = -ca S1 / P - cb fl(mean): the product rounds at |cb mean|, as does cc itself
      dx = fma(ca, g, fma(cb, x, cc)):  cb x and cb mean cancel BY CONSTRUCTION, three roundings at |cb mean| = k |ca S2 / P| stay -- linear in k
      ==>  |d dx| <= u |ca| { 3 |g| + k (3 G2 + |xhat| G1) + (m + 27) |xhat| G2 + (m + 21) G1 } + 2 u |dx|         (frozen statistics: 3 u |ca g|)
    g_abs (the 2x2 sum of the upsampled form: sum of the four |dA|, two more roundings per element) replaces |g| and adds 2 to every count.
    flagged (tie mask): what those elements could add to the sums is added to every bound: sum_f |g_abs| and sum_f |g_abs xhat|."""
    ax = (1, 2) if per_image else (0, 1, 2)
    P = g.shape[1] * g.shape[2] * (1 if per_image else g.shape[0])
    ga = np.abs(g) if g_abs is None else g_abs
    e = 0 if g_abs is None else 2
    k, ca = cs.kappa_r, np.abs(cs.scale)
    G1, G2 = ga.sum(ax) / P, (ga * np.abs(xhat)).sum(ax) / P
    t1 = t2 = 0.0
    if flagged is not None:
        t1, t2 = (ga * flagged).sum(ax), (ga * np.abs(xhat) * flagged).sum(ax)
    b_dbeta = (m + 16 + e) * U * G1 * P + t1
    b_dgamma = U * (k * G1 + (m + 20 + e) * G2) * P + t2
    pe = lambda v: per_element(np.broadcast_to(v, cs.scale.shape), per_image)
    if frozen:
        return (3 + e) * U * pe(ca) * ga, b_dgamma, b_dbeta
    b_dx = U * pe(ca) * ((3 + e) * ga + pe(k) * (3 * pe(G2) + np.abs(xhat) * pe(G1)) + (m + 27 + e) * np.abs(xhat) * pe(G2) + (m + 21 + e) * pe(G1)) \
        + 2 * U * np.abs(dx) + pe(ca) * (pe(t1) / P + np.abs(xhat) * pe(t2) / P)
    return b_dx, b_dgamma, b_dbeta
