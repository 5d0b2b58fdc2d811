"""CPU checks of the Motion-JPEG output: the frame header and the AVI container of utils/mjpeg.py, and the host encoder ``hipops.jpeg_encode_host``
(the torch / numpy form of csrc/jpeg.hip that tests/test_jpeg_gpu.py holds the kernels to).

The reference of the entropy coder is ``decode`` below: an independent baseline-JPEG scan decoder written from T.81 in plain Python.  It takes
everything from the file it is given -- the segments, the Huffman tables of the DHT segments (Annex C code assignment), the restart interval -- and
walks the codes bit by bit, undoing stuffing, RST markers and DC prediction; it checks on the way that the restart markers count m = row mod 8, that
every interval holds exactly its MCUs and that the bits behind the last one are 1-bits of one byte at the most.  It shares nothing with the encoder;
``test_decoder_on_a_pil_stream`` validates it on a stream PIL wrote.

Fidelity gate.  r = RMS(PIL-decode(ours) - input) / RMS(PIL-decode(PIL's own encode, subsampling=0) - input) on four 64 x 64 images at
qualities 50, 75, 90: both encoders quantise with the same tables, ours with a float DCT, PIL's with an integer one.  Measured on the host encoder
(README, "Video output"): every r lies in 0.9734 .. 1.0001; worst 1.0001 (checker, quality 75), gate = 1.25 x worst = ``R_GATE`` (the margin: PIL's
integer DCT rounding the other way on other images; never above 1.5, which would mean wrong tables or order).  Quality 100 is printed, not gated
(0.897 .. 1.046 there: with steps of 1 .. 3 the two DCTs' roundings are the whole error)."""
import io
import os
import struct
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import jpeg_restatement as JR          # noqa: E402
from latent_pose_reenactment_amd import hipops          # noqa: E402
from latent_pose_reenactment_amd.utils import mjpeg          # noqa: E402

R_WORST = 1.0001
R_GATE = 1.25 * R_WORST
assert R_GATE <= 1.5


# ---- the test's own decoder --------------------------------------------------------------------------------------------------------------------------
def segments(data):
    """[(marker, payload)] of a JPEG file up to and including SOS, and the position where the scan starts"""
    assert data[:2] == b'\xff\xd8', 'no SOI'
    at, out = 2, []
    while True:
        assert data[at] == 0xFF, f'no marker at {at}'
        marker = data[at + 1]
        length = struct.unpack('>H', data[at + 2:at + 4])[0]
        out.append((marker, bytes(data[at + 4:at + 2 + length])))
        at += 2 + length
        if marker == 0xDA:
            return out, at


def decode(data):
    """a baseline 4:4:4 JFIF file -> dict(H, W, tables [3, 64] zigzag, coefs int [rows, mcus, 3, 64] zigzag, segments, intervals = the unstuffed
    bytes of every restart interval, pads = the padding bits of each, stuffed = how many 0xFF 0x00 pairs the scan held)"""
    data = bytes(data)
    segs, at = segments(data)
    qt, huff, dri, frame, scan = {}, {}, 0, None, None
    for marker, p in segs:
        if marker == 0xDB:
            while p:
                assert p[0] >> 4 == 0, '16-bit quantisation table'
                qt[p[0] & 15] = np.frombuffer(p[1:65], dtype=np.uint8).astype(np.int64)
                p = p[65:]
        elif marker == 0xC4:
            while p:
                bits, n = p[1:17], sum(p[1:17])
                vals, code, k, table = p[17:17 + n], 0, 0, {}
                for length in range(1, 17):
                    for _ in range(bits[length - 1]):
                        table[(length, code)] = vals[k]
                        code, k = code + 1, k + 1
                    code <<= 1
                huff[(p[0] >> 4, p[0] & 15)] = table
                p = p[17 + n:]
        elif marker == 0xDD:
            dri = struct.unpack('>H', p)[0]
        elif marker == 0xC0:
            assert p[0] == 8 and p[5] == 3
            h, w = struct.unpack('>HH', p[1:5])
            frame = [(p[6 + 3 * i], p[7 + 3 * i], p[8 + 3 * i]) for i in range(3)]
            assert all(f[1] == 0x11 for f in frame), 'not 4:4:4'
        elif marker == 0xDA:
            assert p[0] == 3 and p[-3:] == bytes((0, 63, 0))
            scan = [(p[1 + 2 * i], p[2 + 2 * i] >> 4, p[2 + 2 * i] & 15) for i in range(3)]
        else:
            assert marker in (0xE0, 0xFE) or 0xE0 <= marker <= 0xEF, f'unexpected segment {marker:#x}'
    assert [s[0] for s in scan] == [f[0] for f in frame]
    rows, mcus = -(-h // 8), -(-w // 8)
    per = dri if dri else rows * mcus
    # split the scan at its markers, undoing the stuffing
    intervals, cur, stuffed, expect = [], bytearray(), 0, 0
    while True:
        b = data[at]
        if b != 0xFF:
            cur.append(b)
            at += 1
            continue
        nxt = data[at + 1]
        if nxt == 0x00:
            cur.append(0xFF)
            stuffed += 1
        elif 0xD0 <= nxt <= 0xD7:
            assert nxt - 0xD0 == expect % 8, f'RST{nxt - 0xD0} where RST{expect % 8} belongs'
            expect += 1
            intervals.append(bytes(cur))
            cur = bytearray()
        elif nxt == 0xD9:
            intervals.append(bytes(cur))
            assert at + 2 == len(data), 'bytes behind EOI'
            break
        else:
            raise AssertionError(f'marker {nxt:#x} inside the scan')
        at += 2
    assert len(intervals) == -(-rows * mcus // per), (len(intervals), rows, mcus, per)
    coefs = np.zeros((rows * mcus, 3, 64), dtype=np.int64)
    pads, mcu = [], 0
    for raw in intervals:
        nbits, pos, pred = 8 * len(raw), 0, [0, 0, 0]

        def bit():
            nonlocal pos
            assert pos < nbits, 'the interval ends inside a code'
            v = raw[pos >> 3] >> (7 - (pos & 7)) & 1
            pos += 1
            return v

        def symbol(table):
            code = 0
            for length in range(1, 17):
                code = code << 1 | bit()
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError('no code of 16 bits or fewer matches')

        def receive(size):
            v = 0
            for _ in range(size):
                v = v << 1 | bit()
            return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1

        for _ in range(min(per, rows * mcus - mcu)):
            for c, (_, td, ta) in enumerate(scan):
                pred[c] += receive(symbol(huff[(0, td)]))
                coefs[mcu, c, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(huff[(1, ta)])
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if run != 15:
                            assert run == 0, 'EOBn in a baseline scan'
                            break
                        k += 16
                        continue
                    k += run
                    assert k < 64, 'a run leaves the block'
                    coefs[mcu, c, k] = receive(size)
                    k += 1
            mcu += 1
        pad = nbits - pos
        assert 0 <= pad < 8, f'{pad} bits left behind the last MCU of an interval'
        assert all(bit() for _ in range(pad)), 'padding with 0-bits'
        pads.append(pad)
    assert mcu == rows * mcus
    tables = np.stack([qt[f[2]] for f in frame])
    return dict(H=h, W=w, tables=tables, coefs=coefs.reshape(rows, mcus, 3, 64), segments=segs, intervals=intervals, pads=pads, stuffed=stuffed)


def split(data, offsets):
    data, offsets = np.asarray(data.cpu() if hasattr(data, 'cpu') else data), [int(o) for o in offsets]
    return [data[a:b].tobytes() for a, b in zip(offsets, offsets[1:])]


def pil_pixels(blob):
    im = Image.open(io.BytesIO(blob))
    im.load()
    return np.asarray(im.convert('RGB')).astype(np.float64)


# ---- coefficient tables (shared with tests/test_jpeg_gpu.py) ----------------------------------------------------------------------------------------
SIZES = [(h, w) for h in (8, 16, 40, 80) for w in (8, 16, 24, 72)]


def seeded_table(kind, t, h, w, seed=0):
    """int16 [t, rows, mcus, 3, 64]: 'sparse' about one coefficient in sixteen, small values; 'dense' all of them, sizes 1 .. 10 alike"""
    rng = np.random.default_rng(977 * seed + 31 * h + w + (0 if kind == 'sparse' else 5000) + t)
    shape = (t, h // 8, w // 8, 3, 64)
    if kind == 'sparse':
        c = rng.integers(-6, 7, shape) * (rng.random(shape) < 1 / 16)
        c[..., 0] = rng.integers(-200, 201, shape[:-1])
    else:
        c = np.ldexp(rng.uniform(-1, 1, shape), rng.integers(1, 11, shape)).astype(np.int64)
        c[..., 0] = rng.integers(-1024, 1024, shape[:-1])
    c[..., 1:] = np.clip(c[..., 1:], -1023, 1023)
    return c.astype(np.int16)


def _blocks(mcus, rows=1):
    return np.zeros((1, rows, mcus, 3, 64), dtype=np.int16)


def constructed_tables():
    out = {}
    out['all_zero'] = _blocks(3, 2)                                  # EOB only
    c = _blocks(2)
    c[0, 0, :, :, 63] = (5, -3, 1)                                   # three ZRL, no EOB
    out['lone_63'] = c
    c = _blocks(2)
    c[0, 0, :, :, 16], c[0, 0, :, :, 33], c[0, 0, :, :, 51] = 2, -7, 90          # runs of exactly 15, 16 and 17
    out['runs_15_16_17'] = c
    c = _blocks(3)
    c[0, 0, 0, :, 1:], c[0, 0, 1, :, 1:] = 1023, -1023
    c[0, 0, 2, :, 1:] = np.where(np.arange(63) % 2, 1023, -1023)
    out['ac_extremes'] = c
    c = _blocks(6, 2)
    c[0, :, :, :, 0] = np.where(np.arange(6) % 2, 1023, -1024)[None, :, None]    # differences of +-2047: category 11
    out['dc_category_11'] = c
    return out


def _scan_ff(blob):
    d = decode(blob)
    padded = sum(1 for raw, pad in zip(d['intervals'], d['pads']) if pad and raw[-1] == 0xFF)
    return d['stuffed'], padded


def stuffing_tables():
    """found by search: 'ff_inside' a seeded dense table whose scan holds 0xFF bytes; 'ff_padded_last' one whose interval ends in a PADDED 0xFF byte:
    its last block (Cr) ends with coefficient 63 = 1023, ten 1-bits of extra bits, so no EOB follows and whenever the interval does not end on a
    byte boundary the last byte is all ones.  The search walks the DC of the first block until that holds"""
    out = {}
    for seed in range(64):
        c = seeded_table('dense', 1, 8, 16, seed=100 + seed)
        if _scan_ff(split(*hipops.jpeg_encode_host(coefs=torch.from_numpy(c)))[0])[0] >= 2:
            out['ff_inside'] = c
            break
    for dc in range(64):
        c = _blocks(2, 2)
        c[0, :, 0, 0, 0] = dc
        c[0, :, 1, 2, 63] = 1023
        if _scan_ff(split(*hipops.jpeg_encode_host(coefs=torch.from_numpy(c)))[0])[1] >= 2:
            out['ff_padded_last'] = c
            break
    return out


_TABLES = {}


def coefficient_tables():
    """{name: int16 [T, rows, mcus, 3, 64]}: every table of this file, built once"""
    if not _TABLES:
        for h, w in SIZES:
            for kind, t in (('sparse', 1), ('dense', 1), ('sparse', 3), ('dense', 3)):
                _TABLES[f'{kind}_{h}x{w}_T{t}'] = seeded_table(kind, t, h, w)
        _TABLES.update(constructed_tables())
        _TABLES.update(stuffing_tables())
    return _TABLES


def roundtrip(name, c):
    data, offsets = hipops.jpeg_encode_host(coefs=torch.from_numpy(c))
    files = split(data, offsets)
    assert len(files) == c.shape[0] and int(offsets[0]) == 0 and int(offsets[-1]) == len(data)
    for t, blob in enumerate(files):
        d = decode(blob)
        assert (d['H'], d['W']) == (8 * c.shape[1], 8 * c.shape[2])
        assert np.array_equal(d['coefs'], c[t]), f'{name}: frame {t} does not come back'
    return files


# ---- the header ------------------------------------------------------------------------------------------------------------------------------------
def _pil_jpeg(frame, quality, **kw):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, 'JPEG', quality=quality, subsampling=0, optimize=False, **kw)
    return buf.getvalue()


def test_header_layout_and_dht_against_pil():
    frame = JR.image('smooth_noise', 24, 40)[0]
    ours = segments(mjpeg.jpeg_header(24, 40, 75))[0]
    pil = segments(_pil_jpeg(frame, 75, restart_marker_rows=1))[0]
    assert [(m, len(p) + 2) for m, p in ours] == [(0xE0, 16), (0xDB, 67), (0xDB, 67), (0xC0, 17), (0xC4, 31), (0xC4, 181), (0xC4, 31), (0xC4, 181),
                                                  (0xDD, 4), (0xDA, 12)]
    assert [m for m, _ in ours] == [m for m, _ in pil]
    for marker in (0xC4, 0xDD, 0xC0, 0xDA):
        assert [p for m, p in ours if m == marker] == [p for m, p in pil if m == marker], f'segment {marker:#x} differs from PIL\'s'


@pytest.mark.parametrize('quality', [1, 25, 50, 75, 90, 100])
def test_quantisation_tables_against_pil(quality):
    frame = JR.image('smooth_noise', 16, 16)[0]
    ours = split(*hipops.jpeg_encode_host(torch.from_numpy(frame[None]), quality))[0]
    q_ours = Image.open(io.BytesIO(ours)).quantization
    q_pil = Image.open(io.BytesIO(_pil_jpeg(frame, quality))).quantization
    assert {k: list(v) for k, v in q_ours.items()} == {k: list(v) for k, v in q_pil.items()}
    # and the restatement's, which the transform tests rely on
    d = decode(ours)
    assert np.array_equal(d['tables'], JR.quant_tables(quality))
    assert np.array_equal(mjpeg.quant_tables(quality).astype(np.int64)[[0, 1, 1]][:, JR.ZIGZAG], JR.quant_tables(quality))


def test_quality_is_refused_outside_1_100():
    for bad in (0, 101, -5, 90.0, None):
        with pytest.raises(ValueError, match='quality'):
            mjpeg.jpeg_header(8, 8, bad)


def test_code_table_of_the_library_matches_the_dht_segments():
    """the coder's codes, read from liblp_hip.so on the host (no device work), are the ones the DHT segments announce"""
    import ctypes
    from latent_pose_reenactment_amd import _lib
    table = np.zeros(2 * 12 + 2 * 256, dtype=np.uint32)
    assert _lib.lib().lp_jpeg_code_table(table.ctypes.data_as(ctypes.c_void_p)) == table.size
    assert np.array_equal(table, mjpeg.code_table())
    assert np.count_nonzero(table) == 12 + 12 + 162 + 162


def test_c_abi_refuses_before_any_device_work():
    import ctypes
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    qt = mjpeg.quant_tables(90)
    strides = (ctypes.c_longlong * 4)(192, 24, 3, 1)
    fake = ctypes.c_void_p(4096)
    assert l.lp_jpeg_transform(None, strides, 1, 8, 8, qt.ctypes.data, fake, None) == -1 and b'null' in l.lp_last_error()
    assert l.lp_jpeg_transform(fake, strides, 1, 0, 8, qt.ctypes.data, fake, None) == -1 and b'H >= 1' in l.lp_last_error()
    assert l.lp_jpeg_transform(fake, strides, 0, 8, 8, qt.ctypes.data, fake, None) == -1
    assert l.lp_jpeg_transform(fake, strides, 1, 8, 65536, qt.ctypes.data, fake, None) == -1 and b'65535' in l.lp_last_error()
    zero = qt.copy()
    zero[1, 5] = 0
    assert l.lp_jpeg_transform(fake, strides, 1, 8, 8, zero.ctypes.data, fake, None) == -1 and b'quality' in l.lp_last_error()
    assert l.lp_jpeg_entropy_scratch_bytes(1, 1, 1) > 0
    assert l.lp_jpeg_entropy_scratch_bytes(0, 1, 1) == -1
    assert l.lp_jpeg_entropy_scratch_bytes(4096, 128, 128) == -2 and b'2^31' in l.lp_last_error()          # 201 M blocks
    assert l.lp_jpeg_entropy_size(None, 1, 1, 1, 600, fake, 1 << 20, fake, None) == -1
    assert l.lp_jpeg_entropy_size(fake, 1, 1, 1, 600, fake, 16, fake, None) == -1 and b'scratch' in l.lp_last_error()
    assert l.lp_jpeg_entropy_size(fake, 1, 1, 1, 600, ctypes.c_void_p(4100), 1 << 20, fake, None) == -1 and b'aligned' in l.lp_last_error()
    assert l.lp_jpeg_entropy_write(fake, 1 << 20, 1, 1, 1, fake, 600, None, 100, None) == -1
    assert l.lp_jpeg_entropy_write(fake, 1 << 20, 1, 1, 1, fake, 600, fake, 0, None) == -1 and b'out_bytes' in l.lp_last_error()


# ---- the host encoder ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
def test_roundtrip_seeded_tables(h, w):
    tables = coefficient_tables()
    for kind, t in (('sparse', 1), ('dense', 1), ('sparse', 3), ('dense', 3)):
        name = f'{kind}_{h}x{w}_T{t}'
        files = roundtrip(name, tables[name])
        assert len(decode(files[0])['intervals']) == h // 8          # one restart interval per MCU row; at 80 rows m wraps past 7 (checked in decode)


@pytest.mark.parametrize('name', sorted(constructed_tables()))
def test_roundtrip_constructed_tables(name):
    files = roundtrip(name, coefficient_tables()[name])
    scan = files[0][len(mjpeg.jpeg_header(8, 8, 90)):]
    if name == 'all_zero':          # per block: DC category 0 and EOB: 2 + 4, 2 + 2, 2 + 2 bits = 14 bits per MCU, 42 per interval of 3
        assert all(len(raw) == 6 for raw in decode(files[0])['intervals'])
    if name == 'lone_63':
        assert len(scan) > 0 and all(c == 0 or k in (0, 63) for blk in decode(files[0])['coefs'].reshape(-1, 64) for k, c in enumerate(blk))


def test_stuffing_is_exercised():
    tables = coefficient_tables()
    assert 'ff_inside' in tables and 'ff_padded_last' in tables, 'the search found no table'
    inside = roundtrip('ff_inside', tables['ff_inside'])[0]
    stuffed, _ = _scan_ff(inside)
    assert stuffed >= 2 and inside.count(b'\xff\x00') >= stuffed
    last = roundtrip('ff_padded_last', tables['ff_padded_last'])[0]
    stuffed, padded = _scan_ff(last)
    assert padded >= 2 and stuffed >= padded
    assert b'\xff\x00\xff\xd0' in last and last.endswith(b'\xff\x00\xff\xd9')          # the stuffed zero sits between the padded byte and the marker


def test_decoder_on_a_pil_stream():
    """the test decoder itself: a stream PIL wrote (restart_marker_rows=1), dequantised and inverse-transformed in fp64, against PIL's decoded
    pixels: within 2 levels (the inverse transform is the only inexact step: PIL's is an integer one)"""
    frame = JR.image('smooth_noise', 40, 24, seed=3)[0]
    blob = _pil_jpeg(frame, 75, restart_marker_rows=1)
    d = decode(blob)
    assert len(d['intervals']) == 5 and (d['H'], d['W']) == (40, 24)
    rgb = JR.inverse(d['coefs'][None], 75, 40, 24, tables=d['tables'])[0]
    diff = np.abs(np.clip(np.rint(rgb), 0, 255) - pil_pixels(blob)).max()
    print(f'decoder on PIL\'s stream: max |difference| = {diff:.0f} levels')
    assert diff <= 2


@pytest.mark.parametrize('h,w', [(1, 1), (7, 9), (9, 7), (33, 33), (1, 33), (33, 1)])
def test_pil_opens_every_frame(h, w):
    frames = JR.image('smooth_noise', h, w, seed=2, t=2)
    data, offsets = hipops.jpeg_encode_host(torch.from_numpy(frames), 90)
    for t, blob in enumerate(split(data, offsets)):
        im = Image.open(io.BytesIO(blob))
        assert im.size == (w, h) and im.mode == 'RGB' and im.format == 'JPEG'
        assert pil_pixels(blob).shape == (h, w, 3)
        # edge replication: the coefficients are the restatement's, which replicates the last column / row
        k, flagged = JR.quantise(JR.dct_coefficients(frames[t:t + 1]), 90)
        got = decode(blob)['coefs']
        assert np.abs(got - k[0]).max() <= 1 and np.all((got == k[0]) | flagged[0])


# ---- the transform (cases shared with tests/test_jpeg_gpu.py) -----------------------------------------------------------------------------------------
TRANSFORM_SIZES = [(8, 8), (16, 24), (33, 18), (64, 64)]
TRANSFORM_QUALITIES = (50, 75, 90, 100)
FLAG_CAP = 1 / 16


def transform_frames(h, w, t):
    """{kind: uint8 [t, h, w, 3]}: uniform noise and smooth + noise -- nothing flat or synthetic, which would put D / Q exactly on half-integers"""
    return {kind: JR.image(kind, h, w, seed=11, t=t) for kind in ('noise', 'smooth_noise')}


def check_coefficients(got, frames, quality, what):
    """``got`` [T, rows, mcus, 3, 64] against the fp64 restatement: equal, except where the fp64 D lies within tau = 2^-8 of (n + 1/2) Q (flagged from
    the restatement alone), where it may differ by 1; at most 1 / 16 of the case's coefficients may be flagged.  Returns (flagged share, share that
    differs)"""
    k, flagged = JR.quantise(JR.dct_coefficients(frames), quality)
    got = np.asarray(got, dtype=np.int64)
    assert got.shape == k.shape, (what, got.shape, k.shape)
    diff = np.abs(got - k)
    share = flagged.mean()
    assert share <= FLAG_CAP, f'{what}: {share:.4f} of the coefficients are flagged: the case proves too little'
    assert diff.max() <= 1 and np.all((diff == 0) | flagged), f'{what}: {np.count_nonzero((diff != 0) & ~flagged)} unflagged coefficients differ, max {diff.max()}'
    return share, (diff != 0).mean()


@pytest.mark.parametrize('h,w', TRANSFORM_SIZES)
def test_host_transform_against_restatement(h, w):
    """the torch fp32 form against the fp64 restatement, and the flagged share of every case of the GPU test on all three planes"""
    for t in (1, 3):
        for kind, frames in transform_frames(h, w, t).items():
            for quality in TRANSFORM_QUALITIES:
                got = hipops.jpeg_transform_host(torch.from_numpy(frames), quality).numpy()
                share, wrong = check_coefficients(got, frames, quality, f'{kind} {h}x{w} T{t} q{quality}')
                print(f'host transform {kind:13s} {h:2d}x{w:2d} T{t} quality {quality:3d}: flagged {100 * share:.3f} %, differing {100 * wrong:.4f} %')


FIDELITY_IMAGES = ('smooth', 'smooth_noise', 'checker', 'noise')


def fidelity_ratio(frame, blob, quality):
    rms = lambda px: np.sqrt(np.mean((px - frame.astype(np.float64)) ** 2))
    return rms(pil_pixels(blob)) / rms(pil_pixels(_pil_jpeg(frame, quality)))


def test_fidelity_against_pil_encoder():
    worst = 0.0
    for kind in FIDELITY_IMAGES:
        frame = JR.image(kind, 64, 64, seed=1)[0]
        for quality in (50, 75, 90, 100):
            blob = split(*hipops.jpeg_encode_host(torch.from_numpy(frame[None]), quality))[0]
            r = fidelity_ratio(frame, blob, quality)
            print(f'fidelity host {kind:13s} quality {quality:3d}: r = {r:.4f}' + ('  (reported, not gated)' if quality == 100 else ''))
            if quality != 100:
                worst = max(worst, r)
    assert worst <= R_GATE, (worst, R_GATE)


# ---- the container ---------------------------------------------------------------------------------------------------------------------------------
def riff_walk(blob):
    """a small RIFF reader: dict(avih, strh, strf = their payloads, frames = [(position of the chunk, payload)], index = [(id, flags, offset, size)],
    movi = the position of the 'movi' fourcc); asserts that every size is consistent"""
    assert blob[:4] == b'RIFF' and blob[8:12] == b'AVI ' and struct.unpack('<I', blob[4:8])[0] == len(blob) - 8
    out = dict(frames=[], index=[])

    def walk(at, end):
        while at < end:
            fourcc, size = blob[at:at + 4], struct.unpack('<I', blob[at + 4:at + 8])[0]
            assert at + 8 + size <= end, (fourcc, at, size, end)
            if fourcc == b'LIST':
                kind = blob[at + 8:at + 12]
                if kind == b'movi':
                    out['movi'] = at + 8
                walk(at + 12, at + 8 + size)
            elif fourcc == b'00dc':
                out['frames'].append((at, blob[at + 8:at + 8 + size]))
            elif fourcc == b'idx1':
                assert size % 16 == 0
                out['index'] = [struct.unpack('<4sIII', blob[at + 8 + 16 * i:at + 24 + 16 * i]) for i in range(size // 16)]
            else:
                out[fourcc.decode()] = blob[at + 8:at + 8 + size]
            at += 8 + size + (size & 1)
        assert at == end, (at, end)

    walk(12, len(blob))
    return out


def check_avi(blob, t, h, w, fps):
    """the RIFF walk of an AviWriter file of t frames; returns the decoded frames"""
    r = riff_walk(blob)
    avih, strh, strf = struct.unpack('<14I', r['avih']), struct.unpack('<4s4sIHHIIIIIIII4h', r['strh']), struct.unpack('<IiiHH4sIiiII', r['strf'])
    assert avih[4] == t and strh[9] == t and len(r['frames']) == t and len(r['index']) == t
    assert avih[3] & 0x10 and avih[6] == 1 and (avih[8], avih[9]) == (w, h)
    assert strh[0] == b'vids' and strh[1] == b'MJPG' and strf[:6] == (40, w, h, 1, 24, b'MJPG')
    assert abs(strh[7] / strh[6] - fps) < 1e-3 * fps and abs(avih[0] - 1e6 / fps) <= 1          # fps round-trips through scale / rate
    pixels = []
    for (fourcc, flags, offset, size), (at, payload) in zip(r['index'], r['frames']):
        assert fourcc == b'00dc' and flags & 0x10 and r['movi'] + offset == at and size == len(payload)
        assert at % 2 == 0, 'a chunk at an odd position: the one before it was not padded'
        assert blob[at:at + 4] == b'00dc' and struct.unpack('<I', blob[at + 4:at + 8])[0] == size
        im = Image.open(io.BytesIO(payload))
        assert im.size == (w, h)
        pixels.append(pil_pixels(payload))
    assert max(len(p) for _, p in r['frames']) <= avih[7] == strh[10]
    return pixels


@pytest.mark.parametrize('fps', [25, 30, 29.97, 12.5])
def test_avi_container(tmp_path, fps):
    frames = JR.image('smooth_noise', 24, 40, seed=5, t=5)
    frames[1] = JR.image('noise', 24, 40, seed=6)[0]
    data, offsets = hipops.jpeg_encode_host(torch.from_numpy(frames), 80)
    files = split(data, offsets)
    assert any(len(f) % 2 for f in files) and any(len(f) % 2 == 0 for f in files), 'the case must hold odd and even frame lengths'
    path = tmp_path / 'clip.avi'
    with mjpeg.AviWriter(path, 24, 40, fps) as avi:
        avi.add(data[:int(offsets[2])], offsets[:3])                              # in two calls, as drive.py's chunks
        avi.add(data[int(offsets[2]):], offsets[2:] - offsets[2])
    pixels = check_avi(path.read_bytes(), 5, 24, 40, fps)
    for px, f in zip(pixels, files):
        assert np.array_equal(px, pil_pixels(f))


def test_avi_refuses_two_gib(tmp_path, monkeypatch):
    monkeypatch.setattr(mjpeg, 'AVI_LIMIT', 4096)
    data, offsets = hipops.jpeg_encode_host(torch.from_numpy(JR.image('noise', 32, 32, t=4)), 90)
    avi = mjpeg.AviWriter(tmp_path / 'big.avi', 32, 32, 25)
    with pytest.raises(ValueError, match='2 GiB'):
        avi.add(data, offsets)
    avi.close()
    riff_walk((tmp_path / 'big.avi').read_bytes())          # what was written before the refusal is still a consistent file


def test_host_refusals_name_the_cause():
    ok = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for bad, word in ((ok.float(), 'uint8'), (ok[0], '4-D'), (torch.zeros(1, 8, 8, 4, dtype=torch.uint8), 'C = 4'),
                      (torch.zeros(1, 0, 8, 3, dtype=torch.uint8), 'empty')):
        with pytest.raises(ValueError, match=word):
            hipops.jpeg_encode(bad)
    with pytest.raises(ValueError, match='quality'):
        hipops.jpeg_encode(ok, quality=0)
