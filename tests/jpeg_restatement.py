"""Independent restatement of the coefficient half of csrc/jpeg.hip in numpy, fp64 and integers: colour conversion, edge replication, the
orthonormal DCT-II, the IJG-scaled Annex K tables, zigzag order.  Written from the definition, sharing no code with utils/mjpeg.py or hipops.py
(the tables are typed in again, the zigzag order is the literal list of T.81 Figure A.6 where mjpeg.py walks the diagonals).  Also the seeded
test images of tests/test_mjpeg_cpu.py and tests/test_jpeg_gpu.py."""
import numpy as np

LUMA = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
    [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]])
CHROMA = np.array([
    [17, 18, 24, 47, 99, 99, 99, 99], [18, 21, 26, 66, 99, 99, 99, 99], [24, 26, 56, 99, 99, 99, 99, 99], [47, 66, 99, 99, 99, 99, 99, 99],
    [99, 99, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99], [99, 99, 99, 99, 99, 99, 99, 99]])
# zigzag position -> natural index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
TAU = 2.0 ** -8          # absolute bound on the fp32 chain's error of a coefficient, |D| <= 1024 (tests/test_jpeg_gpu.py)


def quant_tables(quality):
    """int64 [3, 64] in ZIGZAG order, one row per component (Y, Cb, Cr)"""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    tabs = [np.clip((base * s + 50) // 100, 1, 255).reshape(64)[ZIGZAG] for base in (LUMA, CHROMA)]
    return np.stack((tabs[0], tabs[1], tabs[1]))


def basis():
    k, n = np.arange(8)[:, None], np.arange(8)[None, :]
    c = 0.5 * np.cos((2 * n + 1) * k * np.pi / 16)
    c[0] = np.sqrt(1 / 8)
    return c


def dct_coefficients(frames):
    """frames uint8 [T, H, W, 3] -> the unquantised coefficients D, fp64 [T, rows, mcus, 3, 64] in zigzag order"""
    f = np.asarray(frames)
    t, h, w, _ = f.shape
    rows, mcus = -(-h // 8), -(-w // 8)
    f = f[:, np.minimum(np.arange(8 * rows), h - 1)][:, :, np.minimum(np.arange(8 * mcus), w - 1)].astype(np.float64)
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    planes = np.stack((0.299 * r + 0.587 * g + 0.114 * b - 128, -0.168736 * r - 0.331264 * g + 0.5 * b, 0.5 * r - 0.418688 * g - 0.081312 * b), axis=1)
    x = planes.reshape(t, 3, rows, 8, mcus, 8).transpose(0, 2, 4, 1, 3, 5)          # [T, rows, mcus, 3, y, x]
    c = basis()
    d = c @ x @ c.T
    return d.reshape(t, rows, mcus, 3, 64)[..., ZIGZAG]


def quantise(d, quality):
    """(k int64, flagged bool): k = rint(D / Q) ties to even with the definition's clamps; flagged where D lies within TAU of (n + 1/2) Q"""
    q = quant_tables(quality).astype(np.float64)
    k = np.rint(d / q).astype(np.int64)
    k[..., 1:] = np.clip(k[..., 1:], -1023, 1023)
    k[..., 0] = np.clip(k[..., 0], -1024, 1023)
    half = (np.floor(d / q) + 0.5) * q
    return k, np.abs(d - half) <= TAU


def inverse(k, quality, h, w, tables=None):
    """coefficients int [T, rows, mcus, 3, 64] (zigzag) -> RGB fp64 [T, h, w, 3], unrounded and unclamped; ``tables`` [3, 64] (zigzag) in place of
    the ones of ``quality``: a file's own"""
    k = np.asarray(k, dtype=np.float64) * (quant_tables(quality) if tables is None else np.asarray(tables))
    t, rows, mcus = k.shape[:3]
    nat = np.empty_like(k)
    nat[..., ZIGZAG] = k
    c = basis()
    x = c.T @ nat.reshape(t, rows, mcus, 3, 8, 8) @ c
    p = x.transpose(0, 3, 1, 4, 2, 5).reshape(t, 3, rows * 8, mcus * 8)[:, :, :h, :w]
    y, cb, cr = p[:, 0] + 128, p[:, 1], p[:, 2]
    return np.stack((y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb), axis=-1)


def image(kind, h, w, seed=0, t=1):
    """seeded uint8 RGB test frames [t, h, w, 3]: 'noise' uniform, 'smooth' low-frequency waves, 'smooth_noise' the waves + noise of +-12, 'checker'
    4 x 4 squares of two colours"""
    rng = np.random.default_rng(1000 * seed + 7 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for i in range(t):
        if kind == 'noise':
            f = rng.integers(0, 256, (h, w, 3))
        elif kind == 'checker':
            a, b = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
            f = np.where((((yy // 4) + (xx // 4) + i) % 2)[..., None] == 0, a, b)
        else:
            ph = rng.uniform(0, 2 * np.pi, (3, 2))
            f = np.stack([127.5 + 60 * np.sin(yy / (5.0 + c) + ph[c, 0]) + 50 * np.cos(xx / (7.0 - c) + ph[c, 1]) for c in range(3)], axis=-1)
            if kind == 'smooth_noise':
                f = f + rng.uniform(-12, 12, f.shape)
        out.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return np.stack(out)
