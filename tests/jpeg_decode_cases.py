"""The files the JPEG-decode tests share (tests/test_jpeg_decode_cpu.py, tests/test_jpeg_decode_gpu.py), written at test time with PIL, and their
decode by the restatement (tests/jpeg_decode_restatement.py), computed once per process and never changed.

Files: sizes 1x1, 7x9, 8x8, 16x16, 17x33, 33x18, 64x64; grey and ``subsampling`` 0, 1, 2; qualities 1, 30, 75, 90, 100; plain, ``optimize=True``,
``restart_marker_rows=1``; four image kinds: smooth, smooth + noise, uniform noise, and a checker of 4 x 4 squares of the smooth image and its
negative."""
import functools
import io

import numpy as np

SIZES = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (33, 18), (64, 64))
SAMPLINGS = ('grey', 0, 1, 2)
QUALITIES = (1, 30, 75, 90, 100)
VARIANTS = ('plain', 'optimize', 'restart')
KINDS = ('smooth', 'smooth_noise', 'noise', 'checker')
GROUPS = tuple((s, q) for s in SAMPLINGS for q in QUALITIES)


def image(kind, h, w):
    """seeded uint8 RGB [h, w, 3]"""
    rng = np.random.default_rng(31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    ph = rng.uniform(0, 2 * np.pi, (3, 2))
    smooth = np.stack([127.5 + 60 * np.sin(yy / (5.0 + c) + ph[c, 0]) + 50 * np.cos(xx / (7.0 - c) + ph[c, 1]) for c in range(3)], axis=-1)
    if kind == 'smooth':
        f = smooth
    elif kind == 'smooth_noise':
        f = smooth + rng.uniform(-12, 12, smooth.shape)
    elif kind == 'noise':
        f = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
    else:
        f = np.where((((yy // 4) + (xx // 4)) % 2)[..., None] == 0, smooth, 255.0 - smooth)
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def write(pixels, sampling, quality, variant='plain'):
    """-> the bytes of the JPEG file PIL writes"""
    from PIL import Image
    im = Image.fromarray(pixels)
    kw = {'quality': quality}
    if sampling == 'grey':
        im = im.convert('L')
    else:
        kw['subsampling'] = sampling
    if variant == 'optimize':
        kw['optimize'] = True
    elif variant == 'restart':
        kw['restart_marker_rows'] = 1
    out = io.BytesIO()
    im.save(out, 'JPEG', **kw)
    return out.getvalue()


def pil_pixels(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def group(sampling, quality):
    """every file of one (sampling, quality): [(name, bytes, descriptor, the restatement's decode)]"""
    import jpeg_decode_restatement as R
    from latent_pose_reenactment_amd.utils import jpeg_parse
    out = []
    for h, w in SIZES:
        for kind in KINDS:
            for variant in VARIANTS:
                data = write(image(kind, h, w), sampling, quality, variant)
                d = jpeg_parse.parse(data)
                assert d is not None, (sampling, quality, h, w, kind, variant)
                out.append((f'{sampling}_q{quality}_{h}x{w}_{kind}_{variant}', data, d, R.decode(d)))
    return out


def restated_planes(decoded):
    """the planes of one file as the device lays them out: luma, Cb, Cr over their block areas, back to back"""
    return np.concatenate([p.reshape(-1) for p in decoded['planes']])
