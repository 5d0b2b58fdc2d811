"""Augmentation of the pose-encoder input (reference API: dataloaders/common/augmentation.py:15-160): the same three flags and the same
``ParametricAugmenter``, split in two.  The LOADER draws what the reference's imgaug pipeline would have drawn -- ``ParametricAugmenter.sample``: one
row of 32 floats per sample, ``hipops.AUG_COLUMNS`` -- and the row travels with the batch as ``data_dict['aug_params']``; the PIXELS are resampled
and filtered where they are consumed, at the top of ``TrainingModule.forward`` (``apply``): one lp_augment_triplet launch on the GPU, or
``augment_triplet_host`` -- the same definition in fp32 torch ops -- for CPU tensors.  The definition, and what it leaves out of the reference's
pipeline, is the header comment of csrc/augment.hip; tests/augment_restatement.py restates it in fp64.

A SECOND, opt-in stage (``--use_extra_pixelwise_augs``) adds four more of the reference's pixelwise augmenters to the pose image: elastic jitter,
3 x 3 median, saturation and JPEG block quantisation.  ``ParametricAugmenter.sample_extra`` draws one row of 16 floats
(``hipops.AUG_EXTRA_COLUMNS``) from a generator stream of its own, the row travels as ``data_dict['aug_params_extra']``, and ``apply`` runs
lp_augment_extra -- one more launch -- on the first stage's pose output (``augment_extra_host`` for CPU tensors).  Definition and deviations:
the header comment of csrc/augment_extra.hip; tests/augment_extra_restatement.py restates it in fp64."""
import logging
import math

import torch

logger = logging.getLogger('augmentation')

NCOLS = 32
NCOLS_EXTRA = 16
EXTRA_SLOTS = ('elastic', 'median', 'saturation', 'jpeg')          # the second stage's steps; sample_extra picks a subset of 0 .. 2 of them
SLOTS = ('filter', 'noise', 'add', 'multiply', 'contrast')          # the pixelwise steps; SomeOf((0, 5)) picks a subset (augmentation.py:46)


def get_args(parser):
    parser.add('--use_pixelwise_augs', action='store_bool', default=False)
    parser.add('--use_affine_scale', action='store_bool', default=False)
    parser.add('--use_affine_shift', action='store_bool', default=False)
    parser.add('--use_extra_pixelwise_augs', action='store_bool', default=False)
    return parser


def neutral_row():
    """the row that changes nothing: identity maps, identity filter, mul = alpha = 1, everything else 0"""
    row = torch.zeros(NCOLS)
    row[0] = row[4] = row[6] = row[10] = row[16] = row[21] = row[25] = 1.0
    return row


def neutral_row_extra():
    """the second stage's row that changes nothing: all zeros"""
    return torch.zeros(NCOLS_EXTRA)


def extra_stream_seed(seed, index, visit):
    """the seed of the generator that ``sample_extra`` draws from: the loaders' (seed, index, visit) seeding of ``sample`` with another additive
    constant, so the two rows of a sample come from two streams and ``aug_params`` does not depend on the second stage's flag"""
    return (seed * 1000003 + index) * 8191 + visit + 700001 + (1 << 40)


def _uniform(g, lo, hi):
    return lo + (hi - lo) * float(torch.rand((), generator=g))


def _filter_taps(g):
    """one of the reference's four 3 x 3 filters (augmentation.py:49-57; MedianBlur is a step of the second stage) -> 9 taps, row-major"""
    kind = int(torch.randint(0, 4, (), generator=g))
    ident = [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    if kind == 0:                                                   # GaussianBlur((0, 1.0)): sampled on 3 x 3 and normalised
        sigma = _uniform(g, 0.0, 1.0)
        if sigma < 1e-6:
            return ident
        e = math.exp(-1.0 / (2.0 * sigma * sigma))
        row = [e, 1.0, e]
        taps = [a * b for a in row for b in row]
        total = sum(taps)
        return [t / total for t in taps]
    if kind == 1:                                                   # AverageBlur(k=(1, 3))
        return ident if int(torch.randint(0, 2, (), generator=g)) == 0 else [1.0 / 9.0] * 9
    a = _uniform(g, 0.0, 1.0)
    if kind == 2:                                                   # Sharpen(alpha=(0, 1.0), lightness=(1.0, 1.5))
        light = _uniform(g, 1.0, 1.5)
        effect = [-1.0, -1.0, -1.0, -1.0, 8.0 + light, -1.0, -1.0, -1.0, -1.0]
    else:                                                           # Emboss(alpha=(0, 1.0), strength=(0, 0.5))
        s = _uniform(g, 0.0, 0.5)
        effect = [-1.0 - s, -s, 0.0, -s, 1.0, s, 0.0, s, 1.0 + s]
    return [(1.0 - a) * i + a * e for i, e in zip(ident, effect)]


class ParametricAugmenter:
    """what the reference's ParametricAugmenter draws (augmentation.py:26-103), as parameters: ``sample(generator)`` -> one row of 32 floats"""

    def __init__(self, args):
        self.width = self.height = int(getattr(args, 'image_size', 256))
        if getattr(args, 'inference', False):
            logger.info("`args.inference` is set, so switching off all augmentations")
            self.pixelwise = self.scale = self.shift = self.extra = False
            return
        self.pixelwise = bool(getattr(args, 'use_pixelwise_augs', False))
        self.scale = bool(getattr(args, 'use_affine_scale', False))
        self.shift = bool(getattr(args, 'use_affine_shift', False))
        self.extra = bool(getattr(args, 'use_extra_pixelwise_augs', False))
        logger.info(f"Pixelwise augmentation: {self.pixelwise}")
        logger.info(f"Affine scale augmentation: {self.scale}")
        logger.info(f"Affine shift augmentation: {self.shift}")
        logger.info(f"Extra pixelwise augmentation: {self.extra}")

    def is_empty(self):
        return not (self.pixelwise or self.scale or self.shift or self.extra)

    def has_first_stage(self):
        """does any of the reference's three flags ask for an ``aug_params`` row"""
        return self.pixelwise or self.scale or self.shift

    def has_extra_stage(self):
        """does ``--use_extra_pixelwise_augs`` ask for an ``aug_params_extra`` row"""
        return self.extra

    def sample_extra(self, generator):
        """one row of the second stage (16 floats, ``hipops.AUG_EXTRA_COLUMNS``), drawn from ``generator`` -- a stream of its own
        (``extra_stream_seed``) -- with the reference's ranges: a random subset of 0 .. 2 of the four steps (in place of ``SomeOf((0, 5))`` of
        eleven, augmentation.py:46, of which these are four); the neutral row when the flag is off"""
        g, row = generator, neutral_row_extra()
        if not self.extra:
            return row
        count = int(torch.randint(0, 3, (), generator=g))
        chosen = [EXTRA_SLOTS[i] for i in torch.randperm(len(EXTRA_SLOTS), generator=g)[:count].tolist()]
        if 'elastic' in chosen and float(torch.rand((), generator=g)) < 0.5:          # sometimes(ElasticTransformation(alpha=(0.5, 3.5), sigma=0.15))
            row[0] = _uniform(g, 0.5, 3.5)
            row[1] = float(int(torch.randint(0, 1 << 24, (), generator=g)))
        if 'median' in chosen:                                                       # MedianBlur(k=(1, 3)): k = 3 is the only effect
            row[2] = 1.0
        if 'saturation' in chosen:                                                   # AddToSaturation((-20, 20))
            row[3] = _uniform(g, -20.0, 20.0) / 255.0
        if 'jpeg' in chosen:                                                         # JpegCompression((70, 99)), taken as the quality
            row[4] = float(int(torch.randint(70, 100, (), generator=g)))
        return row

    def sample(self, generator):
        """one parameter row, drawn from ``generator`` (a CPU torch.Generator) with the reference's probabilities and ranges"""
        g, row = generator, neutral_row()
        w, h = self.width, self.height
        sx = sy = 1.0
        tx = ty = 0.0
        if self.scale and float(torch.rand((), generator=g)) < 0.5:          # sometimes(Affine(scale x, y in (0.8, 1.2))), about the centre
            sx, sy = _uniform(g, 0.8, 1.2), _uniform(g, 0.8, 1.2)
        if self.shift and float(torch.rand((), generator=g)) < 0.5:          # sometimes(Affine(translate_percent x, y in (-0.05, 0.05)))
            tx, ty = _uniform(g, -0.05, 0.05) * w, _uniform(g, -0.05, 0.05) * h
        cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
        # forward: xd = sx (xs - cx) + cx + tx; the rows hold the INVERSE (destination -> source).  Without a scale the pose row IS the target row.
        row[0], row[2] = 1.0 / sx, (cx - cx / sx) - tx / sx
        row[4], row[5] = 1.0 / sy, (cy - cy / sy) - ty / sy
        row[8], row[11] = -tx, -ty
        if self.pixelwise:
            count = int(torch.randint(0, len(SLOTS) + 1, (), generator=g))
            chosen = [SLOTS[i] for i in torch.randperm(len(SLOTS), generator=g)[:count].tolist()]
            if 'filter' in chosen:
                row[12:21] = torch.tensor(_filter_taps(g))
            if 'noise' in chosen:                                           # AdditiveGaussianNoise(scale=(0, 0.05 * 255), per_channel=False)
                row[27] = _uniform(g, 0.0, 0.05)
                row[28] = float(int(torch.randint(0, 1 << 24, (), generator=g)))
            if 'add' in chosen:                                             # Add((-10, 10), per_channel=0.5)
                if float(torch.rand((), generator=g)) < 0.5:
                    row[22:25] = torch.tensor([_uniform(g, -10.0, 10.0) / 255.0 for _ in range(3)])
                else:
                    row[22:25] = _uniform(g, -10.0, 10.0) / 255.0
            if 'multiply' in chosen:                                        # Multiply((0.5, 1.5), per_channel=False)
                row[21] = _uniform(g, 0.5, 1.5)
            if 'contrast' in chosen:                                        # OneOf(LinearContrast((0.75, 1.25)), SigmoidContrast(gain=(3, 11)))
                if float(torch.rand((), generator=g)) < 0.5:
                    row[25] = _uniform(g, 0.75, 1.25)
                else:
                    row[26] = _uniform(g, 3.0, 11.0)
        return row


def get_augmentation_seq(args):
    return ParametricAugmenter(args)


# ---- the definition in fp32 torch ops (host) --------------------------------------------------------------------------------------------------------
def _reflect101(i, n):
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    m = torch.remainder(i, p)
    return torch.where(m < n, m, p - m)


def _warp(img, A, reflect, pad):
    """img [C, H, W] fp32, A = 6 floats -> warp(img, A, border) on the destination rows / columns -pad .. H - 1 + pad: [C, H + 2 pad, W + 2 pad]"""
    c, h, w = img.shape
    yd = torch.arange(-pad, h + pad, dtype=torch.int64)[:, None].expand(h + 2 * pad, w + 2 * pad)
    xd = torch.arange(-pad, w + pad, dtype=torch.int64)[None, :].expand(h + 2 * pad, w + 2 * pad)

    def tap(y, x):
        if reflect:
            return img[:, _reflect101(y, h), _reflect101(x, w)]
        inside = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        return img[:, y.clamp(0, h - 1), x.clamp(0, w - 1)] * inside.to(img.dtype)
    if A == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]:
        return tap(yd, xd)
    a = [torch.tensor(v, dtype=torch.float32) for v in A]
    fxd, fyd = xd.to(torch.float32), yd.to(torch.float32)
    xs, ys = a[0] * fxd + a[1] * fyd + a[2], a[3] * fxd + a[4] * fyd + a[5]
    x0f, y0f = torch.floor(xs), torch.floor(ys)
    fx, fy = xs - x0f, ys - y0f
    x0, y0 = x0f.clamp(-1.0e9, 1.0e9).to(torch.int64), y0f.clamp(-1.0e9, 1.0e9).to(torch.int64)
    top = tap(y0, x0) * (1.0 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1.0 - fx) + tap(y0 + 1, x0 + 1) * fx
    return top * (1.0 - fy) + bot * fy


def _mul32(x, c):
    """x * c mod 2^32 on int64 tensors holding values below 2^32 (no 64-bit overflow: the constant is split in 16-bit halves)"""
    lo = (x * (c & 0xFFFF)) & 0xFFFFFFFF
    hi = ((x * (c >> 16)) & 0xFFFF) << 16
    return (lo + hi) & 0xFFFFFFFF


def _mix32(x):
    x = x ^ (x >> 16)
    x = _mul32(x, 0x7feb352d)
    x = x ^ (x >> 15)
    x = _mul32(x, 0x846ca68b)
    return x ^ (x >> 16)


def noise_field(seed, h, w):
    """z(yd, xd) of the definition, [H, W] fp32: a pure function of (seed, yd, xd)"""
    n = (torch.arange(h, dtype=torch.int64)[:, None] * w + torch.arange(w, dtype=torch.int64)[None, :]) & 0xFFFFFFFF
    key = (int(seed) * 0x9E3779B9) & 0xFFFFFFFF
    h0, h1 = _mix32(((2 * n) & 0xFFFFFFFF) ^ key), _mix32(((2 * n + 1) & 0xFFFFFFFF) ^ key)
    u1 = ((h0 >> 9).to(torch.float32) + 0.5) * 2.0 ** -23
    u2 = (h1 >> 8).to(torch.float32) * 2.0 ** -24
    return torch.sqrt(-2.0 * torch.log(u1)) * torch.cos(torch.tensor(2.0 * math.pi, dtype=torch.float32) * u2)


def _frames(name, t):
    if t.dim() == 5 and t.shape[1] == 1:
        return t[:, 0], True
    if t.dim() != 4:
        raise ValueError(f'augment_triplet_host: {name} must be [B, C, H, W] or [B, 1, C, H, W], got shape {tuple(t.shape)}')
    return t, False


def augment_triplet_host(pose, params, target=None, segm=None):
    """``hipops.augment_triplet`` for CPU tensors: the definition of csrc/augment.hip in fp32 torch ops, step for step (neutral steps skipped)"""
    for name, t in (('pose', pose), ('params', params), ('target', target), ('segm', segm)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f'augment_triplet_host: {name} must be fp32, got {t.dtype}')
    p4, p5 = _frames('pose', pose)
    b, c, h, w = p4.shape
    if tuple(params.shape) != (b, NCOLS):
        raise ValueError(f'augment_triplet_host: params must be [B, 32] = {(b, NCOLS)}, got {tuple(params.shape)}')
    t4, t5 = _frames('target', target) if target is not None else (None, False)
    s4, s5 = _frames('segm', segm) if segm is not None else (None, False)
    if t4 is not None and t4.shape != p4.shape:
        raise ValueError(f'augment_triplet_host: shape mismatch between pose {tuple(pose.shape)} and target {tuple(target.shape)}')
    if s4 is not None and (s4.shape[0], s4.shape[2], s4.shape[3]) != (b, h, w):
        raise ValueError(f'augment_triplet_host: shape mismatch between pose {tuple(pose.shape)} and segm {tuple(segm.shape)}')
    p4 = p4.detach()
    pose_out = torch.empty(p4.shape, dtype=torch.float32)
    target_out = None if t4 is None else torch.empty(t4.shape, dtype=torch.float32)
    segm_out = None if s4 is None else torch.empty(s4.shape, dtype=torch.float32)
    for i in range(b):
        row = params[i].detach().tolist()
        Ap, At, k = row[0:6], row[6:12], row[12:21]
        mul, add, alpha, gain, sigma, seed = row[21], row[22:25], row[25], row[26], row[27], row[28]
        if t4 is not None:
            target_out[i] = _warp(t4[i].detach(), At, True, 0)
        if s4 is not None:
            segm_out[i] = _warp(s4[i].detach(), At, False, 0)
        if k != [0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]:
            wide = _warp(p4[i], Ap, True, 1)
            v = torch.zeros(c, h, w, dtype=torch.float32)
            for ii in range(3):
                for jj in range(3):
                    v = v + torch.tensor(k[3 * ii + jj], dtype=torch.float32) * wide[:, ii:ii + h, jj:jj + w]
        else:
            v = _warp(p4[i], Ap, True, 0)
        if mul != 1.0:
            v = v * torch.tensor(mul, dtype=torch.float32)
        for ch in range(c):
            a = add[ch] if ch < 3 else 0.0
            if a != 0.0:
                v[ch] = v[ch] + torch.tensor(a, dtype=torch.float32)
        if alpha != 1.0:
            v = 0.5 + torch.tensor(alpha, dtype=torch.float32) * (v - 0.5)
        if gain != 0.0:
            v = 1.0 / (1.0 + torch.exp(torch.tensor(gain, dtype=torch.float32) * (0.5 - v)))
        if sigma != 0.0:
            v = v + torch.tensor(sigma, dtype=torch.float32) * noise_field(int(min(max(seed, 0.0), 16777215.0)), h, w)[None]
        pose_out[i] = v.clamp(0.0, 1.0)
    return (pose_out.unsqueeze(1) if p5 else pose_out,
            None if t4 is None else (target_out.unsqueeze(1) if t5 else target_out),
            None if s4 is None else (segm_out.unsqueeze(1) if s5 else segm_out))


# ---- the second stage in fp32 torch ops (host) ---------------------------------------------------------------------------------------------------------
EXTRA_KEY = 0x85EBCA6B
S0 = 20.0 / 255.0
QBASE = (          # ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major with the vertical frequency as the row
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)


def quant_tables(quality):
    """(luminance, chrominance) 8 x 8 fp32 quantisation tables of an integer quality 1 .. 100: the base tables scaled by the IJG rule"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(torch.tensor([min(max((v * scale + 50) // 100, 1), 255) for v in base], dtype=torch.float32).reshape(8, 8) for base in QBASE)


def _dct_matrix():
    k, n = torch.arange(8, dtype=torch.float64)[:, None], torch.arange(8, dtype=torch.float64)[None, :]
    c = 0.5 * torch.cos((2.0 * n + 1.0) * k * math.pi / 16.0)
    c[0] = math.sqrt(1.0 / 8.0)
    return c.to(torch.float32)


def _elastic_host(img, alpha, seed):
    c, h, w = img.shape
    y = torch.arange(h, dtype=torch.int64)[:, None].expand(h, w)
    x = torch.arange(w, dtype=torch.int64)[None, :].expand(h, w)
    n = (y * w + x) & 0xFFFFFFFF
    key = (int(seed) * EXTRA_KEY) & 0xFFFFFFFF
    ux = (_mix32(((2 * n) & 0xFFFFFFFF) ^ key) >> 8).to(torch.float32) * 2.0 ** -23 - 1.0
    uy = (_mix32(((2 * n + 1) & 0xFFFFFFFF) ^ key) >> 8).to(torch.float32) * 2.0 ** -23 - 1.0
    a = torch.tensor(alpha, dtype=torch.float32)
    xs, ys = x.to(torch.float32) + a * ux, y.to(torch.float32) + a * uy
    x0f, y0f = torch.floor(xs), torch.floor(ys)
    fx, fy = xs - x0f, ys - y0f
    x0, y0 = x0f.clamp(-1.0e9, 1.0e9).to(torch.int64), y0f.clamp(-1.0e9, 1.0e9).to(torch.int64)

    def tap(yy, xx):
        return img[:, _reflect101(yy, h), _reflect101(xx, w)]
    top = tap(y0, x0) * (1.0 - fx) + tap(y0, x0 + 1) * fx
    bot = tap(y0 + 1, x0) * (1.0 - fx) + tap(y0 + 1, x0 + 1) * fx
    return top * (1.0 - fy) + bot * fy


def _median_host(img):
    c, h, w = img.shape
    yr = _reflect101(torch.arange(-1, h + 1, dtype=torch.int64), h)
    xr = _reflect101(torch.arange(-1, w + 1, dtype=torch.int64), w)
    wide = img[:, yr][:, :, xr]
    nine = torch.stack([wide[:, i:i + h, j:j + w] for i in range(3) for j in range(3)])
    return nine.sort(0).values[4]


def _saturation_host(img, d):
    big, small = img.max(0).values, img.min(0).values
    s = torch.where(big > 0, (big - small) / torch.where(big > 0, big, torch.ones_like(big)), torch.zeros_like(big))
    t = s.clamp(min=torch.tensor(S0, dtype=torch.float32).item())
    g = (t + torch.tensor(d, dtype=torch.float32)).clamp(0.0, 1.0) / t
    return big[None] - (big[None] - img) * g[None]


def _jpeg_host(img, quality):
    c, h, w = img.shape
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    yy, xx = torch.arange(hp).clamp(max=h - 1), torch.arange(wp).clamp(max=w - 1)
    r, g, b = (255.0 * img[:, yy][:, :, xx]).unbind(0)
    planes = torch.stack([0.299 * r + 0.587 * g + 0.114 * b - 128.0, -0.168736 * r - 0.331264 * g + 0.5 * b, 0.5 * r - 0.418688 * g - 0.081312 * b])
    ql, qc = quant_tables(quality)
    q = torch.stack([ql, qc, qc])[:, None, None]                                          # [3, 1, 1, 8, 8]
    cm = _dct_matrix()
    blocks = planes.reshape(3, hp // 8, 8, wp // 8, 8).permute(0, 1, 3, 2, 4)              # [3, by, bx, 8, 8]
    coef = cm @ (blocks @ cm.t())                                                        # rows first, then columns
    coef = q * torch.round(coef / q)                                                      # (torch.round: ties to even)
    back = (cm.t() @ coef) @ cm                                                          # columns first, then rows
    yv, cb, cr = back.permute(0, 1, 3, 2, 4).reshape(3, hp, wp)[:, :h, :w].unbind(0)
    yv = yv + 128.0
    return torch.stack([yv + 1.402 * cr, yv - 0.344136 * cb - 0.714136 * cr, yv + 1.772 * cb]) / 255.0


def augment_extra_host(pose, params_extra):
    """``hipops.augment_extra`` for CPU tensors: the definition of csrc/augment_extra.hip in fp32 torch ops, step for step (neutral steps skipped)"""
    for name, t in (('pose', pose), ('params_extra', params_extra)):
        if t.dtype != torch.float32:
            raise ValueError(f'augment_extra_host: {name} must be fp32, got {t.dtype}')
    if pose.dim() == 5 and pose.shape[1] == 1:
        p4 = pose[:, 0]
    elif pose.dim() == 4:
        p4 = pose
    else:
        raise ValueError(f'augment_extra_host: pose must be [B, 3, H, W] or [B, 1, 3, H, W], got shape {tuple(pose.shape)}')
    b, c, h, w = p4.shape
    if c != 3:
        raise ValueError(f'augment_extra_host: pose must have 3 channels, got C = {c}')
    if tuple(params_extra.shape) != (b, NCOLS_EXTRA):
        raise ValueError(f'augment_extra_host: params_extra must be [B, 16] = {(b, NCOLS_EXTRA)}, got {tuple(params_extra.shape)}')
    p4 = p4.detach()
    out = torch.empty(p4.shape, dtype=torch.float32)
    for i in range(b):
        alpha, seed, median, d, quality = params_extra[i].detach().tolist()[:5]
        v = p4[i]
        if alpha != 0.0:
            v = _elastic_host(v, alpha, int(min(max(seed, 0.0), 16777215.0)))
        if median != 0.0:
            v = _median_host(v)
        if d != 0.0:
            v = _saturation_host(v, d)
        if quality != 0.0:
            v = _jpeg_host(v, int(min(max(quality, 1.0), 100.0)))
        out[i] = v.clamp(0.0, 1.0)
    return out.reshape(pose.shape)


def _apply_extra(pose, extra):
    if pose.is_cuda:
        from latent_pose_reenactment_amd import hipops
        return hipops.augment_extra(pose, extra)
    return augment_extra_host(pose, extra)


def apply(data_dict, target_dict):
    """-> shallow copies of the two dicts in which ``pose_input_rgbs``, ``target_rgbs`` and ``real_segm`` (whichever are there, in either dict) are
    replaced by their augmented versions, and from which ``aug_params`` ([B, 32]) and ``aug_params_extra`` ([B, 16]) are gone: they are consumed
    here.  ``aug_params``: CUDA tensors go through ONE lp_augment_triplet launch on the current stream (graph-safe: no host read of the parameters),
    CPU tensors through ``augment_triplet_host``.  ``aug_params_extra``: the pose image -- the first stage's output when both keys are there --
    goes through ONE lp_augment_extra launch, or ``augment_extra_host``.  With the second key alone the first stage is not launched."""
    data_dict = dict(data_dict)
    target_dict = dict(target_dict) if isinstance(target_dict, dict) else target_dict
    extra = data_dict.pop('aug_params_extra', None)
    if extra is not None and 'aug_params' not in data_dict:
        where =data_dict if torch.is_tensor(data_dict.get('pose_input_rgbs')) else (target_dict if isinstance(target_dict, dict) else {})
        if not torch.is_tensor(where.get('pose_input_rgbs')):
            raise KeyError("augmentation.apply: the batch carries 'aug_params_extra' but no 'pose_input_rgbs'")
        where['pose_input_rgbs'] = _apply_extra(where['pose_input_rgbs'], extra)
        return data_dict, target_dict
    params = data_dict.pop('aug_params')
    dicts = [data_dict] + ([target_dict] if isinstance(target_dict, dict) else [])

    def find(key):
        for d in dicts:
            if torch.is_tensor(d.get(key)):
                return d
        return None
    where = {key: find(key) for key in ('pose_input_rgbs', 'target_rgbs', 'real_segm')}
    if where['pose_input_rgbs'] is None:
        raise KeyError("augmentation.apply: the batch carries 'aug_params' but no 'pose_input_rgbs'")
    pose = where['pose_input_rgbs']['pose_input_rgbs']
    target = None if where['target_rgbs'] is None else where['target_rgbs']['target_rgbs']
    segm = None if where['real_segm'] is None else where['real_segm']['real_segm']
    if pose.is_cuda:
        from latent_pose_reenactment_amd import hipops
        outs = hipops.augment_triplet(pose, params, target, segm)
    else:
        outs = augment_triplet_host(pose, params, target, segm)
    if extra is not None:
        outs = (_apply_extra(outs[0], extra),) + tuple(outs[1:])
    for key, out in zip(('pose_input_rgbs', 'target_rgbs', 'real_segm'), outs):
        if out is not None:
            where[key][key] = out
    return data_dict, target_dict
