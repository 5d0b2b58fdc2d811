"""Plain CPU restatement (numpy) of the 16-bit operand formats that every contraction of this project reads: what lp_act_pack, lp_amax_partial,
lp_pack_weights (+ _batch / _pairs) and lp_pack_grouped are documented to write (include/lp_hip.h, the format comments of csrc/lp_common.h).
Written from those documents with integer arithmetic on the bit patterns -- no kernel code is transcribed and no library conversion decides a
rounding.  tests/test_operand_packers_cpu.py proves it against torch's CPU conversions, exact rational arithmetic and the conv algebra in fp64 before
tests/test_operand_packers_gpu.py holds the kernels to it word for word.

Words are numpy uint16; activations [N][HW][C] (or [N][H][W][C]) float32; weights [Cout][Cin][k][k] float32."""
import math

import numpy as np

PREC_BF16, PREC_BF16X3, PREC_F16 = 0, 1, 2
F16_MAX = 65504.0


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- conversions --------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """fp32 -> bf16 word, round to nearest even on the bit pattern: add 0x7FFF plus bit 16 (the lsb of the result), shift right 16.
    A NaN keeps its sign and top payload bits and is made quiet (only its NaN-ness is ever compared)."""
    u = _f32(x).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    v = np.where(nan, np.uint32(0), u)                               # keeps the addition below inside 32 bits
    r = (v + np.uint32(0x7FFF) + ((v >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    r = np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), r)
    return r.astype(np.uint16)


def f16_sat(x):
    """fp32 -> IEEE binary16 word: finite values and +-inf are clamped to +-65504 first, then rounded to nearest even with gradual underflow
    (results under 2^-14 are fp16 subnormals, quantum 2^-24).  NaN stays NaN."""
    u = _f32(x).view(np.uint32)
    sign = (u >> np.uint32(16)) & np.uint32(0x8000)
    mag = np.minimum(u & np.uint32(0x7FFFFFFF), np.uint32(0x477FE000))      # bits of 65504.0f: non-negative floats order like their bit patterns
    # normal results (|x| >= 2^-14 = 0x38800000): rebias the exponent by 112 and drop 13 significand bits, to nearest even; a rounding carry moves
    # into the exponent field, which is the right answer
    r = ((np.maximum(mag, np.uint32(0x38800000)) - np.uint32(0x38000000)) + np.uint32(0xFFF) + ((mag >> np.uint32(13)) & np.uint32(1))) >> np.uint32(13)
    r = np.where(mag <= np.uint32(0x33000000), np.uint32(0), r)             # |x| <= 2^-25: at most half of the subnormal quantum 2^-24 (the tie goes to the even 0)
    small = np.nonzero((mag > np.uint32(0x33000000)) & (mag < np.uint32(0x38800000)))
    if len(small[0]):
        # subnormal results in between: |x| = m * 2^(ef - 150) with the 24-bit significand m, so 126 - ef (14 .. 24) bits are dropped, to nearest even
        ms = mag[small].astype(np.int64)
        ef = ms >> 23
        m = (ms & 0x7FFFFF) | 0x800000
        shift = 126 - ef
        q = m >> shift
        rem, half = m & ((np.int64(1) << shift) - 1), np.int64(1) << (shift - 1)
        r[small] = (q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))).astype(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    r = np.where(nan, np.uint32(0x7E00), r) | sign
    return r.astype(np.uint16)


def bf16_decode(w):
    return (np.asarray(w, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f16_decode(w):
    return np.ascontiguousarray(w, dtype=np.uint16).view(np.float16).astype(np.float32)


def is_nan_word(w, prec):
    """NaN-ness of operand words (the lo plane of the split mode is bf16 like its hi plane)"""
    w = np.asarray(w, dtype=np.uint16) & np.uint16(0x7FFF)
    return w > np.uint16(0x7C00 if prec == PREC_F16 else 0x7F80)


def split(q, prec):
    """fp32 -> (hi, lo) words of an operand mode: bf16 (lo None) | bf16 hi + lo, lo = bf16_rne(q - f32(hi)) (the subtraction is exact in fp32: hi
    and q agree in their leading 8 bits) | fp16 saturating (lo None)"""
    q = _f32(q)
    if prec == PREC_F16:
        return f16_sat(q), None
    hi = bf16_rne(q)
    if prec == PREC_BF16:
        return hi, None
    with np.errstate(invalid='ignore'):                              # inf - inf: the lo word of an infinite operand is NaN
        lo = bf16_rne(q - bf16_decode(hi))
    return hi, lo


def decode(hi, lo, prec):
    """operand words -> the fp64 value the MFMA multiplies (hi + lo in the split mode)"""
    if prec == PREC_F16:
        return f16_decode(hi).astype(np.float64)
    v = bf16_decode(hi).astype(np.float64)
    return v + bf16_decode(lo).astype(np.float64) if prec == PREC_BF16X3 else v


# ---- the activation prologues -------------------------------------------------------------------------------------------------------
def fma32(x, a, b, return_naive=False):
    """x * a + b as ONE fused multiply-add rounded once to fp32 (inputs fp32, normal range).  The product of two 24-bit significands is exact in
    fp64; the fp64 sum s = p + b is rounded once more, with its error term e kept by TwoSum (s + e = p + b exactly).  Rounding s to fp32 is the
    correctly rounded result unless s sits exactly on an fp32 rounding midpoint while e != 0: the true sum is then off the midpoint on the side
    of e, and the answer is the neighbour on that side, not the even one."""
    p = _f32(x).astype(np.float64) * _f32(a).astype(np.float64)
    b = np.broadcast_to(_f32(b).astype(np.float64), p.shape)
    with np.errstate(invalid='ignore', over='ignore'):
        s = p + b
        naive = s.astype(np.float32)
    r = naive.copy()
    i = np.nonzero(np.isfinite(s) & (naive.astype(np.float64) != s))        # where the fp32 rounding of s was inexact
    if len(i[0]):
        pi, bi, si, ri = p[i], b[i], s[i], naive[i]
        bb = si - pi
        ei = (pi - (si - bb)) + (bi - bb)                                    # TwoSum: si + ei = pi + bi exactly
        other = np.nextafter(ri, np.where(si > ri.astype(np.float64), np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        mid = (ri.astype(np.float64) + other.astype(np.float64)) * 0.5 == si        # the sum of two neighbouring fp32 values is exact in fp64
        lo_n, hi_n = np.minimum(ri, other), np.maximum(ri, other)
        r[i] = np.where(mid & (ei != 0), np.where(ei > 0, hi_n, lo_n), ri)
    return (r, naive) if return_naive else r


def act(x, pro, scale=None, shift=None):
    """the prologue of lp_act_pack in fp32: pro 0 x | 1 relu(x*scale[n,c]+shift[n,c]) | 2 relu(x) | 3 relu6 / 4 relu / 5 identity of
    x*scale[c]+shift[c].  x [N][HW][C].  A NaN stays NaN through the ReLUs."""
    x = _f32(x)
    assert x.ndim == 3 and 0 <= pro <= 5
    if pro == 1:
        a = fma32(x, _f32(scale)[:, None, :], _f32(shift)[:, None, :])
    elif pro >= 3:
        a = fma32(x, _f32(scale)[None, None, :], _f32(shift)[None, None, :])
    else:
        a = x
    if pro in (1, 2, 4):
        c = np.maximum(a, np.float32(0))
    elif pro == 3:
        c = np.minimum(np.maximum(a, np.float32(0)), np.float32(6))
    else:
        c = a
    return np.where(np.isnan(a), a, c).astype(np.float32)


def planes(x, pro, scale=None, shift=None, prec=PREC_BF16, in_scale=None):
    """operand planes (hi, lo | None) [N][HW][C8] of act(x) * in_scale, C8 = C rounded up to 8, pad channels zero words"""
    x = _f32(x)
    if x.ndim == 4:
        x = x.reshape(x.shape[0], -1, x.shape[3])
    q = act(x, pro, scale, shift)
    if in_scale is not None:
        q = q * np.float32(in_scale)
    n, hw, c = q.shape
    c8 = (c + 7) // 8 * 8
    hi, lo = split(q, prec)
    out = []
    for p in (hi, lo):
        if p is None:
            out.append(None)
            continue
        full = np.zeros((n, hw, c8), dtype=np.uint16)
        full[:, :, :c] = p
        out.append(full)
    return out[0], out[1]


def amax_scale(m):
    """(s, 1/s) of an fp16 gradient operand: s = 2^(13 - e) for m = f * 2^e, f in [0.5, 1) -- the scaled amax lands in [2^12, 2^13); the
    exponent is clamped to +-100; m <= 0, m >= 3e38 (inf included) and NaN give (1, 1)"""
    m = np.float32(m)
    if not (m > np.float32(0) and m < np.float32(3.0e38)):
        return np.float32(1), np.float32(1)
    _, e = math.frexp(float(m))
    k = max(-100, min(100, 13 - e))
    return np.float32(2.0 ** k), np.float32(2.0 ** -k)


# ---- weight images ------------------------------------------------------------------------------------------------------------------
# Phase form of conv3x3(nearest_up2(x)) (modes 2 / 3): output row 2y + a reads, through tap dy, the upsampled row 2y + a + dy - 1 = the low-resolution
# row y + floor((a + dy - 1) / 2); tap i of phase a is the low-resolution row y + a - 1 + i.  PHASE_TAPS[a][i] = the dy that meet it (columns alike).
PHASE_TAPS = {0: {0: (0,), 1: (1, 2)}, 1: {0: (0, 1), 1: (2,)}}
# conv3x3 followed by AvgPool2d(2) (modes 4 / 5) as a 4x4 stride-2 conv: pooled[y] = 1/4 sum_{a in {0, 1}} conv[2y + a] = sum_{u = -1..2} W4[u] in[2y + u],
# W4[u] = 1/4 * sum of w[dy] over the dy = u - a + 1 inside [0, 2].  POOL_TAPS[u] = those dy (columns alike).
POOL_TAPS = {-1: (0,), 0: (0, 1), 1: (1, 2), 2: (2,)}
POOL_U = {0: (2, 0), 1: (1, -1)}            # mode 5: hi-res pixel 2y + a collects W4[u_a(i)]^T d_pooled[y + a - 1 + i]


def _tap_sum(w, rows, cols):
    """sum of w[:, :, r, c] over the index set rows x cols, in w's dtype"""
    s = np.zeros(w.shape[:2], dtype=w.dtype)
    for r in rows:
        for c in cols:
            s = s + w[:, :, r, c]
    return s


def weight_values(w, mode):
    """the UNPADDED image of lp_pack_weights in w's dtype (fp32: what the pack rounds; fp64: the algebra): [taps][rows][cols] with
    mode 0 [t][co][ci] = w[co][ci][t] | 1 [T-1-t][ci][co] = w[co][ci][t] | 2 [t = (2a+b)*4 + 2i + j][co][ci] = the phase tap sum (a, b, i, j) |
    3 [t][ci][co] = the (phase, 1-i, 1-j) sum | 4 [t = (pa, pb, ky, kx)][co][ci] = W4[2ky - pa][2kx - pb] | 5 [t = (a, b, i, j)][ci][co] = W4[u_a(i)][u_b(j)]"""
    w = np.asarray(w)
    cout, cin = w.shape[:2]
    if mode in (0, 1):
        wt = w.reshape(cout, cin, -1)
        if mode == 0:
            return np.ascontiguousarray(wt.transpose(2, 0, 1))
        return np.ascontiguousarray(wt[:, :, ::-1].transpose(2, 1, 0))
    assert w.shape[2:] == (3, 3), 'modes 2 .. 5 are forms of a 3x3 weight'
    out = []
    for t in range(16):
        p, q, i, j = (t >> 3) & 1, (t >> 2) & 1, (t >> 1) & 1, t & 1
        if mode == 2:
            v = _tap_sum(w, PHASE_TAPS[p][i], PHASE_TAPS[q][j])
        elif mode == 3:
            v = _tap_sum(w, PHASE_TAPS[p][1 - i], PHASE_TAPS[q][1 - j]).T
        elif mode == 4:
            v = _tap_sum(w, POOL_TAPS[2 * i - p], POOL_TAPS[2 * j - q]) * w.dtype.type(0.25)
        elif mode == 5:
            v = (_tap_sum(w, POOL_TAPS[POOL_U[p][i]], POOL_TAPS[POOL_U[q][j]]) * w.dtype.type(0.25)).T
        else:
            raise ValueError(mode)
        out.append(v)
    return np.stack(out)


def weight_pack(w, mode, rows_p, cols_p, prec):
    """(hi, lo | None) [taps][rows_p][cols_p] words of lp_pack_weights: the fp32 image, zero padded, then split"""
    v = weight_values(_f32(w), mode)
    taps, rows, cols = v.shape
    assert rows_p >= rows and cols_p >= cols
    full = np.zeros((taps, rows_p, cols_p), dtype=np.float32)
    full[:, :rows, :cols] = v
    return split(full, prec)


def grouped_values(w, group_size, cp, mode):
    """image [9][CP][64] of lp_pack_grouped in w's dtype.  w [C][cg][3][3] (nn.Conv2d(C, C, 3, groups = C / cg)); the grouped conv as a block-diagonal
    conv over aligned 64-channel blocks: mode 0 [t][co][cl] = w[co][ci % cg][t] for ci = 64 * (co / 64) + cl in co's group, else 0;
    mode 1 [8-t][ci][cl] = w[co][ci % cg][t] for co = 64 * (ci / 64) + cl in ci's group, else 0; rows from C on are zero"""
    w = np.asarray(w)
    c, cg = w.shape[:2]
    assert cg == group_size and c % 64 == 0 and 64 % cg == 0 and cp >= c
    wt = w.reshape(c, cg, 9)
    out = np.zeros((9, cp, 64), dtype=w.dtype)
    for row in range(c):
        for other in range(row // cg * cg, row // cg * cg + cg):         # the channels of the other side that share row's group
            cl = other - row // 64 * 64
            if mode == 0:
                out[:, row, cl] = wt[row, other % cg, :]
            else:
                out[:, row, cl] = wt[other, row % cg, ::-1]
    return out


def grouped_pack(w, group_size, cp, mode, prec):
    return split(grouped_values(_f32(w), group_size, cp, mode), prec)


# ---- input sets shared by the CPU proof and the GPU tests --------------------------------------------------------------------------------
def edge_values(fp32_subnormals):
    """fp32 inputs at which a conversion can go wrong: signed zeros, exact ties of both formats in both directions (to the even neighbour below /
    above), the fp16 maximum, the first value that would round to fp16 inf (65520), 7e4, +-inf, the smallest fp16 normal (2^-14) and subnormal
    (2^-24), half of it (2^-25: a tie that goes to zero), fp16-subnormal results that round gradually, 1e-30, NaN; fp32 subnormals on request"""
    t8, t11 = 2.0 ** -8, 2.0 ** -11
    v = [0.0, -0.0, 1.0, -1.0,
         1 + t8, 1 + 3 * t8, -(1 + t8), -(1 + 3 * t8), 1 + t8 + 2.0 ** -20, 1 + t8 - 2.0 ** -20,           # bf16 ties and their neighbourhood
         1 + t11, 1 + 3 * t11, -(1 + t11), -(1 + 3 * t11), 1 + t11 + 2.0 ** -22, 1 + t11 - 2.0 ** -22,     # fp16 ties
         65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 7e4, -7e4, 3.0e38, -3.0e38, np.inf, -np.inf,
         2.0 ** -14, -2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 2.0 ** -25 + 2.0 ** -40,
         3 * 2.0 ** -25, 5 * 2.0 ** -25, 1.75 * 2.0 ** -24, 2.0 ** -15 + 2.0 ** -25, 2.0 ** -26, 1e-30, -1e-30,
         6.0, 6.0 + 2.0 ** -21, 5.96875, np.nan, -np.nan]
    if fp32_subnormals:
        v += [2.0 ** -127, -2.0 ** -130, 2.0 ** -149]
    return np.array(v, dtype=np.float32)


def grid_set(rng, x_shape, scale_shape):
    """(x, scale, shift) whose affine x * scale + shift is EXACT in fp32, fused or not: x and shift multiples of 2^-8 in [-4, 4), scale multiples of
    2^-6 in [-2, 2) -- the product is a multiple of 2^-14 under 8, the sum one under 12: 18 bits"""
    x = rng.integers(-1024, 1024, size=x_shape, dtype=np.int16).astype(np.float32) * np.float32(2.0 ** -8)
    scale = rng.integers(-128, 128, size=scale_shape, dtype=np.int16).astype(np.float32) * np.float32(2.0 ** -6)
    shift = rng.integers(-1024, 1024, size=scale_shape, dtype=np.int16).astype(np.float32) * np.float32(2.0 ** -8)
    return x, scale, shift
