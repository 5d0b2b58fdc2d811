"""fp64 restatement of the second augmentation stage defined in the header comment of csrc/augment_extra.hip, written from that text with numpy
indexing; it calls neither the kernel nor latent_pose_reenactment_amd/augmentation.py.  The hash is integer arithmetic (uint64 holding values below
2^32: no product overflows), so the displacement field is exact.  Also here: the gates with the near-tie rule of the JPEG step (derived in the
docstring of tests/test_augment_extra_gpu.py), and the inputs and parameter rows that the CPU and the GPU tests share."""
import math

import numpy as np

NCOLS = 16
M32 = np.uint64(0xFFFFFFFF)
KEY = 0x85EBCA6B
S0 = 20.0 / 255.0
K1 = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
K2 = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def row(alpha=0.0, seed=0, median=0, d=0.0, quality=0):
    r = np.zeros(NCOLS)
    r[:5] = [alpha, seed, median, d, quality]
    return np.float32(r).astype(np.float64)          # the rows are fp32 values: both sides see the same parameters


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def mix32(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def displacement(seed, h, w):
    """(u(0), u(1)) of every pixel, each [H, W] in [-1, 1)"""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing='ij')
    n = (y * np.uint64(w) + x) & M32
    key = np.uint64((int(seed) * KEY) & 0xFFFFFFFF)
    u = [(mix32(((np.uint64(2) * n + np.uint64(j)) & M32) ^ key) >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0 for j in (0, 1)]
    return u[0], u[1]


def elastic(img, alpha, seed):
    c, h, w = img.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    u0, u1 = displacement(seed, h, w)
    xs, ys = x + alpha * u0, y + alpha * u1
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = xs - x0, ys - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(yy, xx):
        return img[:, reflect101(yy, h), reflect101(xx, w)]
    top = tap(y0, x0) * (1.0 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1.0 - fx) + tap(y0 + 1, x0 + 1) * fx
    return top * (1.0 - fy) + bot * fy


def median3(img):
    c, h, w = img.shape
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    nine = np.stack([img[:, reflect101(y + i, h), reflect101(x + j, w)] for i in (-1, 0, 1) for j in (-1, 0, 1)])
    return np.median(nine, axis=0)


def saturation(img, d):
    big, small = img.max(0), img.min(0)
    s = np.where(big > 0, (big - small) / np.where(big > 0, big, 1.0), 0.0)
    t = np.maximum(s, S0)
    g = np.clip(t + d, 0.0, 1.0) / t
    return big[None] - (big[None] - img) * g[None]


def quant_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [np.array([min(max((v * scale + 50) // 100, 1), 255) for v in base], dtype=np.float64).reshape(8, 8) for base in (K1, K2)]


def dct_matrix():
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing='ij')
    c = 0.5 * np.cos((2 * n + 1) * k * math.pi / 16.0)
    c[0] = math.sqrt(1.0 / 8.0)
    return c


def jpeg(img, quality, detail=False):
    """-> the decoded image [3, H, W]; with ``detail`` also D / q before the rounding, [3, by, bx, 8, 8], and q [3, 8, 8]"""
    c, h, w = img.shape
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    yy, xx = np.minimum(np.arange(hp), h - 1), np.minimum(np.arange(wp), w - 1)
    r, g, b = 255.0 * img[:, yy][:, :, xx]
    planes = np.stack([0.299 * r + 0.587 * g + 0.114 * b - 128.0, -0.168736 * r - 0.331264 * g + 0.5 * b, 0.5 * r - 0.418688 * g - 0.081312 * b])
    ql, qc = quant_tables(quality)
    q = np.stack([ql, qc, qc])
    cm = dct_matrix()
    blocks = planes.reshape(3, hp // 8, 8, wp // 8, 8).transpose(0, 1, 3, 2, 4)
    ratio = np.einsum('un,pyxnm,vm->pyxuv', cm, blocks, cm) / q[:, None, None]
    coef = q[:, None, None] * np.rint(ratio)          # (np.rint: ties to even)
    back = np.einsum('un,pyxuv,vm->pyxnm', cm, coef, cm).transpose(0, 1, 3, 2, 4).reshape(3, hp, wp)[:, :h, :w]
    yv, cb, cr = back[0] + 128.0, back[1], back[2]
    out = np.stack([yv + 1.402 * cr, yv - 0.344136 * cb - 0.714136 * cr, yv + 1.772 * cb]) / 255.0
    return (out, ratio, q) if detail else out


def augment_extra(x, params, detail=False):
    """x [B, 3, H, W], params [B, 16] (anything numpy converts) -> the fp64 result; with ``detail`` also, per sample, None or the (D / q, q) of the
    JPEG step"""
    x = np.asarray(x, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64)
    out, info = np.zeros_like(x), []
    for i in range(x.shape[0]):
        alpha, seed, med, d, quality = params[i][:5]
        v = x[i]
        if alpha != 0.0:
            v = elastic(v, alpha, int(min(max(seed, 0.0), 16777215.0)))
        if med != 0.0:
            v = median3(v)
        if d != 0.0:
            v = saturation(v, d)
        if quality != 0.0:
            v, ratio, q = jpeg(v, int(min(max(quality, 1.0), 100.0)), detail=True)
            info.append((ratio, q))
        else:
            info.append(None)
        out[i] = np.clip(v, 0.0, 1.0)
    return (out, info) if detail else out


# ---- the gates (derived in the docstring of tests/test_augment_extra_gpu.py) ---------------------------------------------------------------------
U = 2.0 ** -23
L_SAT = 3.0 + S0                                   # Lipschitz constant of the saturation step for |d| <= s0
DELTA_DCT = 2.0 ** -9                              # fp32 error bound of a forward coefficient (255-units), exact inputs
JPEG_OUT = (2 * 9 * 8192 + 2048) * 2.0 ** -24 / 255.0          # fp32 error bound of the inverse transform, as a pixel value in [0, 1]
PLANE_GAIN = np.array([1.0, 1.772, 1.402])         # the largest weight of Y, Cb, Cr in an RGB channel


def upstream_gate(p, h, w):
    """max-abs bound of an fp32 implementation's error BEFORE the JPEG step of row ``p``, i.e. the gate of a row without JPEG"""
    alpha, _, med, d, _ = p[:5]
    e = (8.0 * max(h, w) + 8.0) * U if alpha != 0.0 else 0.0          # elastic: the bilinear bound; the median is 1-Lipschitz and rounds nothing
    if d != 0.0:
        assert abs(d) <= S0 + 1e-8, d          # (20 / 255 rounded to fp32 may sit 4e-9 above)
        e = L_SAT * e + 8.0 * U                # saturation: Lipschitz constant 3 + s0, own roundings 15 * 2^-24
    return e


def check(got, x, params):
    """``got`` [B, 3, H, W] against the restatement of (x, params) -> per sample a dict: ratio = worst error / gate over the pixels (blocks with a
    near-tie get their allowance added to the gate), flagged = share of the 8 x 8 pixel blocks that hold a near-tie in any plane, abs = max-abs
    error.  Which blocks hold a near-tie is decided here from the fp64 values alone."""
    got = np.asarray(got, dtype=np.float64)
    params = np.asarray(params, dtype=np.float64)
    want, info = augment_extra(x, params, detail=True)
    b, _, h, w = want.shape
    res = []
    for i in range(b):
        err = np.abs(got[i] - want[i]).max(0)                                           # [H, W], worst channel
        up = upstream_gate(params[i], h, w)
        if info[i] is None:
            gate = np.full((h, w), up if up > 0.0 else 0.0)
            flagged = 0.0
            ratio = float(np.where(err == 0.0, 0.0, err / np.maximum(gate, 1e-300)).max())
        else:
            ratio_c, q = info[i]
            delta = 8.0 * 255.0 * up + DELTA_DCT                                        # error bound of a coefficient before the rounding
            tau = delta / q[:, None, None]
            near = np.abs(ratio_c - np.floor(ratio_c) - 0.5) <= tau                     # within tau of a half-integer step
            allowance = (near * (q[:, None, None] / 4.0) * PLANE_GAIN[:, None, None, None, None]).sum((0, 3, 4)) / 255.0          # [by, bx]
            flagged = float((allowance > 0).mean())
            gate = JPEG_OUT + np.kron(allowance, np.ones((8, 8)))[:h, :w]
            ratio = float((err / gate).max())
        res.append({'ratio': ratio, 'flagged': flagged, 'abs': float(err.max())})
    return res


# ---- inputs and rows shared by the CPU and GPU tests -----------------------------------------------------------------------------------------------
SIZES = ((8, 8), (16, 16), (20, 24), (33, 18), (64, 64))
BATCHES = (1, 3)


def smooth_image(b, h, w, seed=0):
    """[B, 3, H, W] fp64 in [0.1, 0.9]: per channel a few low-frequency waves -- a JPEG block of it has few coefficients away from 0"""
    rng = np.random.RandomState(1000 + seed)
    y, x = np.meshgrid(np.arange(h) / 64.0, np.arange(w) / 64.0, indexing='ij')
    out = np.zeros((b, 3, h, w))
    for i in range(b):
        for c in range(3):
            f, ph = rng.uniform(0.5, 2.5, size=(2, 2)), rng.uniform(0, 2 * math.pi, size=2)
            out[i, c] = 0.5 + 0.2 * np.sin(2 * math.pi * (f[0, 0] * x + f[0, 1] * y) + ph[0]) + 0.2 * np.sin(2 * math.pi * (f[1, 0] * x - f[1, 1] * y) + ph[1])
    return np.float32(out).astype(np.float64)


# the JPEG cases' inputs: smooth_image(b, h, w, seed=100 * JPEG_SEED[(h, w)] + 10 * b + k) for the k-th batch of B rows.  The smallest sizes have
# 1 .. 4 blocks per image, so ONE near-tie breaks the 1 / 8 cap: the seeds are the first for which the fp64 values alone keep every case of the
# size inside the cap (tests/test_augment_extra_cpu.py checks that they do)
JPEG_SEED = {(8, 8): 0, (16, 16): 1, (20, 24): 1, (33, 18): 1, (64, 64): 0}


def noise_image(b, h, w, seed=0):
    return np.float32(np.random.RandomState(2000 + seed).uniform(0.0, 1.0, size=(b, 3, h, w))).astype(np.float64)


def step_rows():
    """{step: [rows]}: each step ALONE at the ends of its range"""
    return {
        'neutral': [row()],
        'elastic': [row(alpha=0.5, seed=12345), row(alpha=3.5, seed=16777215)],
        'median': [row(median=1)],
        'saturation': [row(d=20.0 / 255.0), row(d=-20.0 / 255.0), row(d=7.0 / 255.0)],
        'jpeg': [row(quality=70), row(quality=85), row(quality=95)],
    }


def batches(rows, b):
    out = []
    for start in range(0, len(rows), b):
        out.append(np.stack([rows[(start + i) % len(rows)] for i in range(b)]))
    return out
