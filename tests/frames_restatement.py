"""fp64 restatement of the frame preparation defined in the header comment of csrc/frames.hip, written from that text with numpy indexing; it calls
neither the kernel nor latent_pose_reenactment_amd/frames.py.  The tap positions and the area weights are integer arithmetic (exact), the cubic and
linear weights are evaluated in fp64 from the exact fraction r / (2 S); every sum is a float64 matrix product.  ``gate`` is the per-row bound an
fp32 implementation is held to (tests/test_frames_cpu.py for ``frames.prepare_host``, tests/test_frames_gpu.py for the kernel)."""
import math

import numpy as np

NCOLS = 24
(IMG_OFF, IMG_H, IMG_W, IMG_RS, IMG_PS, IMG_T, IMG_L, IMG_B, IMG_R, IMG_MODE,
 MSK_OFF, MSK_H, MSK_W, MSK_RS, MSK_PS, MSK_T, MSK_L, MSK_B, MSK_R, IMAGE_SLOT, MASK_SLOT, PRODUCT_SLOT) = range(22)
AREA, CUBIC, LINEAR = 0, 1, 2
A = -0.75


def row(image=None, mask=None, image_slot=-1, mask_slot=-1, product_slot=-1):
    """one table row.  image = (off, H, W, row stride, pixel stride, t, l, b, r, mode), mask = (off, H, W, row stride, pixel stride, t, l, b, r);
    a view that is not given stays all zero (H == 0)"""
    r = [0] * NCOLS
    if image is not None:
        r[IMG_OFF:IMG_MODE + 1] = list(image)
    if mask is not None:
        r[MSK_OFF:MSK_R + 1] = list(mask)
    r[IMAGE_SLOT], r[MASK_SLOT], r[PRODUCT_SLOT] = image_slot, mask_slot, product_slot
    return r


def mode_for(n, size):
    return AREA if size <= n else CUBIC


def reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def crop_plane(buf, off, h, w, rs, ps, c, t, l, n, mask):
    """the n x n crop of channel c of a view, through the border rule, as float64 (raw values 0 .. 255)"""
    ys, xs = t + np.arange(n, dtype=np.int64), l + np.arange(n, dtype=np.int64)
    if mask:
        above = ys < 0
        ys, xs = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
    else:
        ys, xs = reflect101(ys, h), reflect101(xs, w)
    plane = buf[off + ys[:, None] * rs + xs[None, :] * ps + c].astype(np.float64)
    if mask:
        plane[above, :] = 0.0
    return plane


def taps(mode, n, size, d):
    """-> (first tap index in crop coordinates, fp64 weights) of output d of one axis"""
    if mode == AREA:
        first, end = (d * n) // size, ((d + 1) * n + size - 1) // size
        w = [max(0, min((j + 1) * size, (d + 1) * n) - max(j * size, d * n)) / n for j in range(first, end)]
        return first, w
    num, den = (2 * d + 1) * n - size, 2 * size
    q = num // den                                   # floor, also for a negative numerator
    f = (num - q * den) / den
    if mode == LINEAR:
        return q, [1.0 - f, f]
    w0 = ((A * (f + 1) - 5 * A) * (f + 1) + 8 * A) * (f + 1) - 4 * A
    w1 = ((A + 2) * f - (A + 3)) * f * f + 1
    w2 = ((A + 2) * (1 - f) - (A + 3)) * (1 - f) * (1 - f) + 1
    return q - 1, [w0, w1, w2, 1.0 - w0 - w1 - w2]


def axis_matrix(mode, n, size):
    """[size, n] fp64: row d holds the weights of output d, a tap index clamped to the crop adding to the column it lands on"""
    m = np.zeros((size, n), dtype=np.float64)
    for d in range(size):
        first, w = taps(mode, n, size, d)
        for k, wk in enumerate(w):
            m[d, min(max(first + k, 0), n - 1)] += wk
    return m


def abs_weight_sum(mode, n, size):
    """max over the outputs of one axis of sum |w|"""
    return max(sum(abs(x) for x in taps(mode, n, size, d)[1]) for d in range(size))


def resample(plane, size, mode, clamp=True):
    n = plane.shape[0]
    m = axis_matrix(mode, n, size)
    out = m @ plane @ m.T
    if mode == CUBIC and clamp:
        out = np.clip(out, 0.0, 255.0)
    return out / 255.0


def prepare(buf, table, size):
    """buf: uint8 numpy vector, table: rows of NCOLS integers -> (image, mask, product) float64 [slots, 3, size, size] (None where no row asks)"""
    buf = np.asarray(buf, dtype=np.uint8)
    table = [[int(v) for v in r] for r in table]
    outs = []
    for col in (IMAGE_SLOT, MASK_SLOT, PRODUCT_SLOT):
        count = max([r[col] for r in table] + [-1]) + 1
        outs.append(np.zeros((count, 3, size, size), dtype=np.float64) if count else None)
    for r in table:
        img = msk = None
        if r[IMG_H] > 0:
            assert r[IMG_B] - r[IMG_T] == r[IMG_R] - r[IMG_L] >= 1
            img = np.stack([resample(crop_plane(buf, r[IMG_OFF], r[IMG_H], r[IMG_W], r[IMG_RS], r[IMG_PS], c, r[IMG_T], r[IMG_L],
                                                r[IMG_B] - r[IMG_T], False), size, r[IMG_MODE]) for c in range(3)])
        if r[MSK_H] > 0:
            assert r[MSK_B] - r[MSK_T] == r[MSK_R] - r[MSK_L] >= 1
            msk = resample(crop_plane(buf, r[MSK_OFF], r[MSK_H], r[MSK_W], r[MSK_RS], r[MSK_PS], 0, r[MSK_T], r[MSK_L], r[MSK_B] - r[MSK_T], True),
                           size, LINEAR)
        if r[IMAGE_SLOT] >= 0:
            outs[0][r[IMAGE_SLOT]] = img
        if r[MASK_SLOT] >= 0:
            outs[1][r[MASK_SLOT]] = msk[None]
        if r[PRODUCT_SLOT] >= 0:
            outs[2][r[PRODUCT_SLOT]] = img * msk[None]
    return tuple(outs)


def gate(n, size, mode):
    """bound on |fp32 result - restatement| per element of a row: (n_y + n_x + 8) 2^-24 W -- the fp32 dot-product bound of the two separable passes
    plus the weight arithmetic; n_y = n_x = taps per axis (ceil(scale) + 1 | 4 | 2), W = the product of the per-axis sum |w| (1 for area and linear)"""
    k = {AREA: math.ceil(n / size) + 1, CUBIC: 4, LINEAR: 2}[mode]
    w = abs_weight_sum(mode, n, size) ** 2 if mode == CUBIC else 1.0
    assert w <= 1.375 ** 2 + 1e-12
    return (2 * k + 8) * 2.0 ** -24 * w


def product_gate(n_img, mode, n_msk, size):
    """product = image x mask, both in [0, 1]: the two errors add, plus the rounding of the product"""
    return gate(n_img, size, mode) + gate(n_msk, size, LINEAR) + 2.0 ** -24
