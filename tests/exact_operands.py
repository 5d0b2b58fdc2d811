"""Operands on which a 16-bit contraction with fp32 accumulation is EXACT, whatever the order and the split of its sums.

Every value is an integer times a power of two that the operand format holds exactly; every sum the kernel can form is then a multiple of one
quantum q, and as long as its magnitude stays under 2^24 q the fp32 sum has no rounding at all.  The budget held here is 2^22 q (asserted per
case, on the CPU, before anything is launched): the two spare bits cover the unmeasured internal alignment of the matrix core's multi-term 16-bit
dot product and are not to be spent.  The kernel's result must then equal the fp64 contraction bit for bit, element by element, in all three
precision modes -- no tolerance is chosen anywhere.

One operand is "wide", the other "narrow":
  bf16 / f16   wide: integers |v| <= 255 (8 significand bits)
  bf16x3       wide: |v| <= 511 or 1023 -- hi = bf16(v), lo = bf16(v - hi) reproduces every |v| <= 65535; 25 - 50 % of the lo words are non-zero
  narrow       {-2 .. 2}, shrunk to {-1, 0, 1} and then thinned with zeros until the budget holds
The bf16x3 kernels form hi*hi + hi*lo + lo*hi and drop lo*lo by design: that is the reference (from the decoded planes), and the budget is taken
on |hi| + |lo|.  The phase forms (lp_pack_weights modes 2 .. 5) contract 16 PRE-SUMMED taps: phase_conv64 / phase_bound / draw_phase_pair below.
CPU-only module: torch on the host, nothing from the library."""
import torch
import torch.nn.functional as F

PREC_BF16, PREC_BF16X3, PREC_F16 = 0, 1, 2
BUDGET_BITS = 22                      # |every sum| <= 2^22 quanta (the hard limit of exact fp32 sums is 2^24)
QA, QW = 2.0 ** -4, 2.0 ** -3         # quanta of the activation-side and the weight-side operand
ALPHA = 0.5                           # the conv epilogue's scale: a power of two


class BudgetError(AssertionError):
    pass


def wide_bound(prec, big=False):
    return (1023 if big else 511) if prec == PREC_BF16X3 else 255


def draw_ints(gen, shape, bound, keep=1.0):
    """int64 tensor, uniform in [-bound, bound]; ``keep`` < 1 zeroes entries at random (thinning)"""
    v = torch.randint(-bound, bound + 1, shape, generator=gen, dtype=torch.int64)
    if keep < 1.0:
        v = v * (torch.rand(shape, generator=gen) < keep)
    return v


def split_hi_lo(v):
    """fp32 values -> (hi, lo) fp32: hi = bf16(v), lo = bf16(v - hi), by torch's CPU conversions (round to nearest even)"""
    v = v.float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi, lo


def terms(v, prec):
    """the fp64 values the matrix core multiplies for the fp32 operand v: [v] (bf16 / f16: v must be exact in the format) | [hi, lo]"""
    v = v.float()
    if prec == PREC_BF16X3:
        hi, lo = split_hi_lo(v)
        assert torch.equal(hi + lo, v), 'value not reproduced by the hi + lo split'
        return [hi.double(), lo.double()]
    dt = torch.float16 if prec == PREC_F16 else torch.bfloat16
    assert torch.equal(v.to(dt).float(), v), 'value not exact in the 16-bit operand format'
    return [v.double()]


def abs_sum(ts):
    return sum(t.abs() for t in ts)


def up2(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)


def conv64(a_terms, w_terms, ups=False):
    """fp64 contraction the kernels form, NCHW x [Cout][Cin][k][k]: hi*hi (+ hi*lo + lo*hi), zero padding k // 2, fused nearest x2 upsampling"""
    pad = w_terms[0].shape[-1] // 2
    u = up2 if ups else (lambda t: t)
    ref = F.conv2d(u(a_terms[0]), sum(w_terms), None, 1, pad)
    if len(a_terms) == 2:
        ref = ref + F.conv2d(u(a_terms[1]), w_terms[0], None, 1, pad)
    return ref


def conv_int64(a, w, ups=False):
    """the same contraction on int64 tensors (a [N][C][H][W], w [Cout][Cin][k][k]) by shifted adds: integer arithmetic only"""
    if ups:
        a = up2(a)
    k = w.shape[-1]
    pad = k // 2
    n, c, h, wd = a.shape
    ap = torch.zeros((n, c, h + 2 * pad, wd + 2 * pad), dtype=torch.int64)
    ap[:, :, pad:pad + h, pad:pad + wd] = a
    out = torch.zeros((n, w.shape[0], h, wd), dtype=torch.int64)
    for ky in range(k):
        for kx in range(k):
            out += torch.einsum('nchw,oc->nohw', ap[:, :, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
    return out


def wgrad64(a_terms, d_terms, ks, ups=False):
    """fp64 weight gradient dw[co][ci][ky][kx] = sum_pixels dy[n, co, y, x] * up2?(a)[n, ci, y + ky - pad, x + kx - pad] (+ the two cross terms)"""
    u = up2 if ups else (lambda t: t)
    pad = ks // 2

    def one(a, d):
        # conv of the (channel-major) input with dy as the kernel: batch <-> channel roles swapped
        g = F.conv2d(u(a).transpose(0, 1), d.transpose(0, 1), None, 1, pad)        # [Cin][Cout][k'][k'] over the full correlation window
        return g.transpose(0, 1)
    h = d_terms[0].shape[2]
    ref = one(a_terms[0], sum(d_terms))
    if len(a_terms) == 2:
        ref = ref + one(a_terms[1], d_terms[0])
    assert ref.shape[-1] == ks and ref.shape[-2] == ks, (ref.shape, ks, h)
    return ref


def assert_budget(bound64, quantum, what=''):
    """bound64: fp64 tensor of the largest magnitude any partial sum can reach, per output element"""
    m = float(bound64.max())
    if not m <= 2.0 ** BUDGET_BITS * quantum:
        raise BudgetError(f'{what}: sum bound {m:.4g} = {m / quantum:.4g} quanta exceeds 2^{BUDGET_BITS}')
    return m / quantum


def conv_bound(a_terms, w_terms, ups, alpha, bias=None, res=None):
    """alpha * conv(|A|, |W|) + |bias| + |res| in fp64 (bias [Cout], res NCHW at output resolution, or None)"""
    b = alpha * conv64([abs_sum(a_terms)], [abs_sum(w_terms)], ups)
    if bias is not None:
        b = b + bias.double().abs()[None, :, None, None]
    if res is not None:
        b = b + res.double().abs()
    return b


NARROW_STEPS = [(2, 1.0), (1, 1.0), (1, 0.5), (1, 0.25), (1, 0.125)]      # (bound, keep): {-2..2}, {-1,0,1}, then thinned


def draw_pair(seed, a_shape, w_shape, prec, wide, bound_fn, big=False, both_wide=False):
    """(a, w) fp32 tensors of integers times QA / QW; ``wide`` = 'a' | 'w' names the wide operand, the other is narrow and is shrunk until
    bound_fn(a_terms, w_terms) (the fp64 bound of the case) passes the budget.  Deterministic in seed."""
    wb = wide_bound(prec, big)
    last = None
    for nb, keep in ([(wb, 1.0)] if both_wide else NARROW_STEPS):
        g = torch.Generator().manual_seed(seed)
        a = draw_ints(g, a_shape, wb if wide == 'a' else nb, 1.0 if wide == 'a' else keep).float() * QA
        w = draw_ints(g, w_shape, wb if wide == 'w' else nb, 1.0 if wide == 'w' else keep).float() * QW
        try:
            bound_fn(terms(a, prec), terms(w, prec))
            return a, w
        except BudgetError as e:
            last = e
    raise last


# ---- the phase forms (lp_pack_weights modes 2 .. 5, lp_conv16_fwd upsample = 2 | 3; include/lp_hip.h) ---------------------------------------
# Sixteen pre-summed taps W'[t], t = p * 8 + q * 4 + i * 2 + j, each a [rows][cols] matrix (rows = the launch's output channels, cols = its
# contraction).  Written from the definitions of the header, on plain strided slices:
#   scatter (modes 2 and 5, upsample = 2): in [N][cols][h][w] -> out [N][rows][2h][2w],
#       out[2y + p, 2x + q] = sum_{i, j} W'[t] . in[y + p - 1 + i, x + q - 1 + j]
#   gather  (modes 3 and 4, upsample = 3): in [N][cols][2h][2w] -> out [N][rows][h][w],
#       out[y, x] = sum_{p, q, i, j} W'[t] . in[2y + 2i - p, 2x + 2j - q]
#     mode 4 by its definition (pooled[y] = sum_u W4[u] in[2y + u], W'[t] = W4[2i - p][2j - q]); mode 3 as the adjoint of the scatter form: the pixel
#     (2y' + p, 2x' + q) that scatter tap (p, q, i', j') fills from (y, x) has y' = y - p + 1 - i', so with i = 1 - i' it is row 2y + 2i - p, and the
#     mode-3 image holds exactly the (p, q, 1 - i, 1 - j) sums, transposed.
# Positions outside the input read zero.
WIDE_W_PHASE = 63                     # single-plane modes: up to 4 taps coincide, |sum| <= 252 stays exact in 8 significand bits


def phase_conv(a, w16, gather):
    """one term of the contraction above, in the dtype of its operands (fp64 or int64: shifted adds and channel contractions only)"""
    n, c, h, w = a.shape
    assert w16.shape[0] == 16 and w16.shape[2] == c, (w16.shape, a.shape)
    rows = w16.shape[1]
    ap = torch.zeros((n, c, h + 2, w + 2), dtype=a.dtype)
    ap[:, :, 1:1 + h, 1:1 + w] = a
    if gather:
        assert h % 2 == 0 and w % 2 == 0
        ho, wo = h // 2, w // 2
        out = torch.zeros((n, rows, ho, wo), dtype=a.dtype)
    else:
        out = torch.zeros((n, rows, 2 * h, 2 * w), dtype=a.dtype)
    for t in range(16):
        p, q, i, j = (t >> 3) & 1, (t >> 2) & 1, (t >> 1) & 1, t & 1
        if gather:       # input row 2y + 2i - p sits at padded index 2y + 2i - p + 1
            src = ap[:, :, 2 * i - p + 1:2 * i - p + 1 + 2 * ho:2, 2 * j - q + 1:2 * j - q + 1 + 2 * wo:2]
            out += torch.einsum('nchw,oc->nohw', src, w16[t])
        else:            # input row y + p - 1 + i sits at padded index y + p + i
            src = ap[:, :, p + i:p + i + h, q + j:q + j + w]
            out[:, :, p::2, q::2] += torch.einsum('nchw,oc->nohw', src, w16[t])
    return out


def phase_conv64(a_terms, w16_terms, gather):
    """fp64 contraction of a phase-form launch from the 16 PRE-SUMMED taps: hi*hi (+ hi*lo + lo*hi over the split of the pre-summed value -- the
    split happens after the sum, so the split of the dense 3x3 weight is not the reference)"""
    ref = phase_conv(a_terms[0], sum(w16_terms), gather)
    if len(a_terms) == 2:
        ref = ref + phase_conv(a_terms[1], w16_terms[0], gather)
    return ref


def phase_bound(a_terms, w16_terms, gather, alpha, bias=None, res=None):
    """alpha * phase_conv(|A|, |W'|) + |bias| + |res| in fp64 (bias [rows], res NCHW at output resolution, or None): no partial sum of the launch,
    of one split-K slice or of one phase, exceeds it"""
    b = alpha * phase_conv(abs_sum(a_terms), abs_sum(w16_terms), gather)
    if bias is not None:
        b = b + bias.double().abs()[None, :, None, None]
    if res is not None:
        b = b + res.double().abs()
    return b


def draw_phase_pair(seed, a_shape, w_shape, prec, wide, bound_fn, big=False):
    """draw_pair for the phase forms: w [.][.][3][3] are integers times QW whose tap sums must stay exact -- a wide weight of the single-plane modes
    is bounded by WIDE_W_PHASE, bf16x3 keeps 511 / 1023 (hi + lo reproduces every sum).  bound_fn(a, w) takes the fp32 tensors."""
    wb = wide_bound(prec, big)
    wwb = wb if prec == PREC_BF16X3 else WIDE_W_PHASE
    last = None
    for nb, keep in NARROW_STEPS:
        g = torch.Generator().manual_seed(seed)
        a = draw_ints(g, a_shape, wb if wide == 'a' else nb, 1.0 if wide == 'a' else keep).float() * QA
        w = draw_ints(g, w_shape, wwb if wide == 'w' else nb, 1.0 if wide == 'w' else keep).float() * QW
        try:
            bound_fn(a, w)
            return a, w
        except BudgetError as e:
            last = e
    raise last


def first_mismatch(got, ref, names):
    """index of the first differing element of two equal-shaped tensors, formatted with the axis names"""
    bad = (got != ref).nonzero()
    i = bad[0].tolist()
    return (f'{len(bad)} of {ref.numel()} elements differ; first at (' + ', '.join(f'{n}={v}' for n, v in zip(names, i)) +
            f'): got {got[tuple(i)].item()!r}, want {ref[tuple(i)].item()!r}')
