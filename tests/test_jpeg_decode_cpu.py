"""The JPEG decode of ``--decode_jpeg_on_gpu`` without a GPU: the host twin (``hipops.jpeg_decode_host``) against the restatement of the definition
(tests/jpeg_decode_restatement.py) bit for bit, the restatement against PIL's decode of the same files, the integer IDCT against the fp64 one, the
round trip with the project's own encoder, the parser's ``None`` / ``ValueError`` cases, a corrupt stream through the host twin, the loader with
the flag on the CPU, and the refusals of the C ABI and of the wrapper.

Gates.  Twin == restatement: exact (integer arithmetic).  Restatement vs PIL 12.2 (libjpeg-turbo) on the files of tests/jpeg_decode_cases.py:
at most 3 levels in colour and 1 in grey, at least 90 % of all values equal -- PIL's integer IDCT rounds some samples one level differently than
any other accurate IDCT and the colour matrix scales that by up to 1.772.  Measured: worst 3 (colour; 2 at quality 1), 1 (grey); 96.43 % of the
4 057 200 values equal.  Integer IDCT vs fp64 before rounding: <= 1 (measured 0.613: the rounded basis and the two shifts' halves)."""
import ctypes
import io
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import jpeg_decode_cases as C          # noqa: E402
import jpeg_decode_restatement as R          # noqa: E402
from latent_pose_reenactment_amd import frames, hipops          # noqa: E402
from latent_pose_reenactment_amd.utils import jpeg_parse          # noqa: E402


def check_decoded_group(result, files):
    """a ``JpegDecoded`` of all ``files`` of a group in one call against the restatement: coefficients, sample planes, pixels exact, status 0"""
    rows = result.frames.tolist()
    coefs, planes, buf = result.coefs.cpu().numpy(), result.planes.cpu().numpy(), result.buf.cpu().numpy()
    assert result.status.cpu().tolist() == [0] * len(files)
    for (name, _, d, want), r in zip(files, rows):
        blocks, flat = d.blocks, C.restated_planes(want)
        assert np.array_equal(coefs[r[8]:r[8] + blocks], want['coefs']), f'{name}: coefficients'
        assert np.array_equal(planes[r[9]:r[9] + flat.size], flat), f'{name}: sample planes'
        assert np.array_equal(buf[r[10]:r[10] + d.h * d.w * 3].reshape(d.h, d.w, 3), want['pixels']), f'{name}: pixels'


@pytest.mark.parametrize('sampling,quality', C.GROUPS)
def test_host_twin_equals_restatement(sampling, quality):
    files = C.group(sampling, quality)
    assert len(files) == len(C.SIZES) * len(C.KINDS) * len(C.VARIANTS)
    check_decoded_group(hipops.jpeg_decode_host([d for _, _, d, _ in files]), files)


@pytest.mark.parametrize('sampling,quality', C.GROUPS)
def test_restatement_against_pil(sampling, quality):
    worst = 0
    for name, data, d, want in C.group(sampling, quality):
        pil = C.pil_pixels(data)
        assert pil.shape == want['pixels'].shape, name
        diff = int(np.abs(pil.astype(np.int64) - want['pixels'].astype(np.int64)).max())
        worst = max(worst, diff)
        assert diff <= (1 if sampling == 'grey' else 3), (name, diff)
    print(f'[jpeg_decode] restatement vs PIL, sampling {sampling}, quality {quality}: worst difference {worst} levels')


def test_restatement_against_pil_share():
    equal = total = 0
    for sampling, quality in C.GROUPS:
        for _, data, _, want in C.group(sampling, quality):
            pil = C.pil_pixels(data)
            equal += int((pil == want['pixels']).sum())
            total += pil.size
    print(f'[jpeg_decode] restatement vs PIL: {100.0 * equal / total:.2f} % of {total} values equal')
    assert equal >= 0.90 * total


def test_integer_idct_against_fp64():
    worst = 0.0
    for sampling, quality in C.GROUPS:
        for _, _, _, want in C.group(sampling, quality):
            worst = max(worst, float(np.abs(want['S'] - R.idct_exact(want['F'])).max()))
    print(f'[jpeg_decode] integer IDCT vs fp64 IDCT before rounding: worst {worst:.3f}')
    assert worst <= 1.0


def test_idct_table():
    K = jpeg_parse.idct_table()
    assert K.dtype == np.int32 and K.tolist() == [v for row in R.K for v in row]
    assert np.abs(K.reshape(8, 8)).sum(axis=0).max() <= 31569 and int(np.abs(K).max()) <= 4096          # the 32-bit argument of pass 1


@pytest.mark.parametrize('h,w', [(8, 8), (17, 33), (40, 24)])
@pytest.mark.parametrize('quality', [50, 90])
def test_round_trip_with_the_projects_encoder(h, w, quality):
    """parse + entropy decode of what ``jpeg_encode_host`` writes gives exactly the coefficients it coded"""
    import jpeg_restatement as JR
    frames_in = torch.from_numpy(JR.image('smooth_noise', h, w, seed=3, t=2))
    data, offsets = hipops.jpeg_encode_host(frames_in, quality)
    want = hipops.jpeg_transform_host(frames_in, quality).numpy()
    blob = data.numpy().tobytes()
    ds = [jpeg_parse.parse(blob[a:b]) for a, b in zip(offsets.tolist(), offsets.tolist()[1:])]
    assert all(d is not None and d.restart == -(-w // 8) and (d.hmax, d.vmax) == (1, 1) for d in ds)
    got = hipops.jpeg_decode_host(ds)
    assert got.status.tolist() == [0, 0]
    assert np.array_equal(got.coefs.numpy().reshape(want.shape), want)
    for t, d in enumerate(ds):
        assert np.array_equal(R.entropy(d)[0].reshape(want.shape[1:]), want[t])


# ---- the parser ------------------------------------------------------------------------------------------------------------------------------------
def _plain(sampling=2, size=(17, 33), quality=90, variant='plain'):
    return C.write(C.image('smooth_noise', *size), sampling, quality, variant)


def _segments(data):
    """[(marker, offset of its 0xFF, offset behind its payload)] up to and including SOS"""
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, length = data[at + 1], (data[at + 2] << 8) | data[at + 3]
        out.append((marker, at, at + 2 + length))
        at += 2 + length
        if marker == 0xDA:
            return out


def test_parser_returns_none_for_unsupported_files():
    from PIL import Image
    rgb = Image.fromarray(C.image('smooth_noise', 17, 33))
    out = io.BytesIO()
    rgb.save(out, 'JPEG', quality=90, progressive=True)
    assert jpeg_parse.parse(out.getvalue()) is None                      # progressive (SOF2)
    out = io.BytesIO()
    rgb.convert('CMYK').save(out, 'JPEG', quality=90)
    assert jpeg_parse.parse(out.getvalue()) is None                      # four components
    data = bytearray(_plain())
    segs = _segments(data)
    sof = next(s for s in segs if s[0] == 0xC0)
    patched = bytearray(data)
    patched[sof[1] + 1] = 0xC1
    assert jpeg_parse.parse(bytes(patched)) is None                      # extended sequential (SOF1)
    dqt = next(s for s in segs if s[0] == 0xDB)
    patched = bytearray(data)
    patched[dqt[1] + 4] |= 0x10
    assert jpeg_parse.parse(bytes(patched)) is None                      # 16-bit quantisation table
    sos = segs[-1]
    second = bytes(data[:-2]) + bytes(data[sos[1]:])                       # the scan once more in place of EOI
    assert jpeg_parse.parse(second) is None
    patched = bytearray(data)
    patched[sof[1] + 4] = 12
    assert jpeg_parse.parse(bytes(patched)) is None                      # 12-bit samples
    assert jpeg_parse.parse(bytes(data)) is not None
    # component ids 'R', 'G', 'B': with the JFIF marker still YCbCr (supported), without it libjpeg and PIL read RGB samples
    app0 = next(s for s in segs if s[0] == 0xE0)
    patched = bytearray(data)
    for c, ident in enumerate(b'RGB'):
        patched[sof[1] + 10 + 3 * c] = ident
        patched[sos[1] + 5 + 2 * c] = ident
    assert jpeg_parse.parse(bytes(patched)) is not None
    bare = bytes(patched[:app0[1]]) + bytes(patched[app0[2]:])
    assert jpeg_parse.parse(bare) is None
    assert int(np.abs(C.pil_pixels(bare).astype(int) - C.pil_pixels(bytes(data)).astype(int)).max()) > 3          # (PIL does read it differently)


def test_parser_raises_for_malformed_files():
    data = _plain(sampling=0, variant='restart', size=(33, 18))
    segs = _segments(data)
    dht = next(s for s in segs if s[0] == 0xC4)
    sos = segs[-1]
    for cut, word in ((1, 'SOI'), (segs[0][1] + 3, 'truncated'), (dht[1] + 20, 'truncated'), (sos[1] + 2, 'truncated'), (sos[2] + 5, 'truncated'),
                      (len(data) - 2, 'truncated')):
        with pytest.raises(ValueError, match=word):
            jpeg_parse.parse(data[:cut])
    rst = [i for i in range(sos[2], len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(rst) == 4                                                   # 33 rows of 4:4:4: 5 MCU rows, 5 intervals, 4 markers
    swapped = bytearray(data)
    swapped[rst[1] + 1], swapped[rst[2] + 1] = swapped[rst[2] + 1], swapped[rst[1] + 1]
    with pytest.raises(ValueError, match='RST out of order'):
        jpeg_parse.parse(bytes(swapped))
    marked = bytearray(data)
    marked[rst[0] + 1] = 0xC4
    with pytest.raises(ValueError, match='0xFFC4 inside the scan'):
        jpeg_parse.parse(bytes(marked))
    dropped = bytearray(data)
    del dropped[rst[3]:rst[3] + 2]
    with pytest.raises(ValueError, match='restart intervals'):
        jpeg_parse.parse(bytes(dropped))
    missing = bytearray(data)
    missing[sos[2] - 4] = 0x33                                             # the last component's tables: DC 3, AC 3
    with pytest.raises(ValueError, match='missing table'):
        jpeg_parse.parse(bytes(missing))
    longer = bytearray(data)
    longer[dht[1] + 2], longer[dht[1] + 3] = 0xFF, 0xF0
    with pytest.raises(ValueError, match='declares a length'):
        jpeg_parse.parse(bytes(longer))


def test_fill_bytes_before_markers_parse():
    data = _plain(variant='restart', size=(33, 18))
    want = jpeg_parse.parse(data)
    segs = _segments(data)
    filled = bytearray()
    at = 2
    filled += data[:2]
    for marker, start, end in segs:
        filled += b'\xff\xff' + data[start:end]
        at = end
    scan = data[at:]
    rst = [i for i in range(len(scan) - 1) if scan[i] == 0xFF and (0xD0 <= scan[i + 1] <= 0xD7 or scan[i + 1] == 0xD9)]
    prev = 0
    for i in rst:
        filled += scan[prev:i] + b'\xff\xff'
        prev = i
    filled += scan[prev:]
    assert len(filled) == len(data) + 2 * (len(segs) + len(rst))
    got = jpeg_parse.parse(bytes(filled))
    assert got is not None and np.array_equal(got.scan, want.scan) and np.array_equal(got.seg, want.seg) and np.array_equal(got.qt, want.qt)
    assert np.array_equal(C.pil_pixels(bytes(filled)), C.pil_pixels(data))          # (and PIL reads the filled file as the same image)


# ---- a corrupt stream ------------------------------------------------------------------------------------------------------------------------------
def corrupt_case():
    """(good descriptor A, the corrupt one, good descriptor B): a file of the list with ONE bit of its scan flipped, the first position from the
    front at which the restatement reports a status"""
    a = jpeg_parse.parse(C.write(C.image('smooth_noise', 16, 16), 2, 90))
    b = jpeg_parse.parse(C.write(C.image('noise', 17, 33), 0, 75, 'restart'))
    victim = jpeg_parse.parse(C.write(C.image('smooth_noise', 33, 18), 1, 90))
    for bit in range(8 * len(victim.scan)):
        scan = victim.scan.copy()
        scan[bit >> 3] ^= 0x80 >> (bit & 7)
        bad = victim._replace(scan=scan)
        if R.entropy(bad)[1] != 0:
            return a, bad, b
    raise AssertionError('no single flipped bit breaks the stream')


def test_corrupt_stream_is_isolated_in_the_host_twin():
    a, bad, b = corrupt_case()
    both = hipops.jpeg_decode_host([a, bad, b])
    assert both.status[1].item() == R.entropy(bad)[1] != 0 and both.status[0].item() == 0 and both.status[2].item() == 0
    offs = both.offsets.tolist()
    for d, i in ((a, 0), (b, 2)):
        alone = hipops.jpeg_decode_host([d])
        n = d.h * d.w * 3
        assert alone.status.tolist() == [0] and torch.equal(alone.buf, both.buf[offs[i]:offs[i] + n])
        assert torch.equal(alone.coefs, both.coefs[both.frames[i, 8]:both.frames[i, 8] + d.blocks])


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------------
def build_jpeg_tree(root):
    """the tree of tests/test_voxceleb2_loader_cpu.py (one video of JPEG frames, the others PNG) with one frame of the JPEG video turned into a PNG"""
    from PIL import Image
    import test_voxceleb2_loader_cpu as L
    root = L.build_tree(root)
    folder = root / 'Img' / L.JPEG_VIDEO[0] / L.JPEG_VIDEO[1]
    first = folder / (L.NAMES[0] + '.jpg')
    Image.open(first).save(first.with_suffix('.png'))
    first.unlink()
    return root


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return build_jpeg_tree(tmp_path_factory.mktemp('voxceleb2_jpeg'))


def full_buffer(raw):
    """the decoded layout of a flagged raw batch, through the host twin"""
    full = torch.zeros(int(raw['nbytes']), dtype=torch.uint8)
    for d, s, n in raw['regions'].tolist():
        full[d:d + n] = raw['buf'][s:s + n]
    if raw['jpeg'] is not None:
        assert hipops.jpeg_decode_host(raw['jpeg'], out=full).status.tolist() == [0] * len(raw['files'])
    return full


def test_loader_with_the_flag_on_the_cpu(tree):
    import test_voxceleb2_loader_cpu as L
    split = L.video_split(tree)
    plain = L.loader_for(L.make_args(tree, val_split_path=split, batch_size=6), 'val')
    flagged = L.loader_for(L.make_args(tree, val_split_path=split, batch_size=6, decode_jpeg_on_gpu=True), 'val')
    raws_p, raws_f = list(plain.loader), list(flagged.loader)
    assert len(raws_p) == len(raws_f) == 1
    p, f = raws_p[0], raws_f[0]
    assert torch.equal(p['table'], f['table']) and torch.equal(p['label'], f['label']) and torch.equal(p['index'], f['index'])
    assert f['nbytes'] == p['buf'].numel() and f['buf'].numel() < p['buf'].numel()
    jpeg_rows = f['jpeg']['frames']
    assert len(f['files']) == jpeg_rows.shape[0] in (L.K, L.K + 1)                                   # the JPEG video's frames, less its PNG one if drawn
    assert all(name.endswith('.jpg') and '/'.join(L.JPEG_VIDEO) in name for name in f['files'])
    full = full_buffer(f)
    inside = torch.zeros(full.numel(), dtype=torch.bool)
    for r in jpeg_rows.tolist():
        inside[r[10]:r[10] + r[0] * r[1] * 3] = True
    assert torch.equal(full[~inside], p['buf'][~inside])                                              # masks and fallback frames: the same bytes
    diff = (full[inside].int() - p['buf'][inside].int()).abs()
    assert 0 < int(diff.max()) <= 3                                                                   # the decoders' pixel difference, nothing else
    # through the preparation: an area resampling is a convex combination (every box here is at least the output size), so 3 levels stay 3 levels
    assert int(f['table'][:, 9].max()) == frames.MODE_AREA
    for got, want in zip(frames.prepare_host(full, f['table'], L.SIZE), frames.prepare_host(p['buf'], p['table'], L.SIZE)):
        assert float((got - want).abs().max()) <= 3.0 / 255.0 + 1e-5
    # and the loader itself yields that batch
    (dd, dt), = list(flagged)
    want = frames.prepare({'buf': full, 'table': f['table'], 'label': f['label'], 'frames': f['frames'], 'pose': f['pose']}, L.SIZE, 'cpu')
    assert set(dd) == set(want[0]) and all(torch.equal(dd[k], want[0][k]) for k in dd) and all(torch.equal(dt[k], want[1][k]) for k in dt)
    # --blur_padded_bands on top: the same buffer through pad_host
    blurred = L.loader_for(L.make_args(tree, val_split_path=split, batch_size=6, decode_jpeg_on_gpu=True, blur_padded_bands=True), 'val')
    (bd, _), = list(blurred)
    want = frames.prepare_host(full, f['table'], L.SIZE, blur_padded_bands=True)
    assert torch.equal(bd['target_rgbs'].reshape(want[2].shape), want[2])


def test_loader_names_the_corrupt_file(tmp_path):
    import test_voxceleb2_loader_cpu as L
    root = build_jpeg_tree(tmp_path / 'tree')
    split = L.video_split(root)
    folder = root / 'Img' / L.JPEG_VIDEO[0] / L.JPEG_VIDEO[1]
    files = sorted(folder.glob('*.jpg'))
    originals = {p: p.read_bytes() for p in files}
    # a flipped bit in the scan of every JPEG frame (whichever the loader draws): the stream parses, the decode reports it
    for p, data in originals.items():
        d = jpeg_parse.parse(data)
        at = data.index(bytes(d.scan[:8]))
        for bit in range(64):
            mangled = bytearray(data)
            mangled[at + (bit >> 3)] ^= 0x80 >> (bit & 7)
            try:
                bad = jpeg_parse.parse(bytes(mangled))
            except ValueError:
                continue
            if bad is not None and R.entropy(bad)[1] != 0:
                p.write_bytes(bytes(mangled))
                break
        else:
            raise AssertionError('no flipped bit found')
    loader = L.loader_for(L.make_args(root, val_split_path=split, batch_size=6, decode_jpeg_on_gpu=True), 'val')
    with pytest.raises(ValueError, match=str(folder)) as e:
        list(loader)
    assert 'does not decode' in str(e.value) and '.jpg' in str(e.value)
    # a truncated file: the parser raises in the loader, naming the path
    for p, data in originals.items():
        p.write_bytes(data[:len(data) // 2])
    loader = L.loader_for(L.make_args(root, val_split_path=split, batch_size=6, decode_jpeg_on_gpu=True), 'val')
    with pytest.raises(ValueError, match=str(folder)) as e:
        list(loader)
    assert 'truncated' in str(e.value)


def test_flag_is_off_by_default_and_leaves_the_raw_batch_alone(tree):
    import test_voxceleb2_loader_cpu as L
    raw = next(iter(L.loader_for(L.make_args(tree, val_split_path=L.video_split(tree), batch_size=6), 'val').loader))
    assert set(raw) == {'buf', 'table', 'frames', 'pose', 'label', 'index'}

    class Parser:
        def __init__(self):
            self.flags = {}

        def add(self, name, **kw):
            self.flags[name] = kw

    from latent_pose_reenactment_amd.dataloaders.voxceleb2_segmentation_nolandmarks import Dataset
    parser = Parser()
    Dataset.get_args(parser)
    assert parser.flags['--decode_jpeg_on_gpu']['default'] is False and parser.flags['--decode_jpeg_on_gpu']['action'] == 'store_bool'


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_before_any_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    d = jpeg_parse.parse(_plain())
    pk = jpeg_parse.pack([d])
    fake, K = ctypes.c_void_p(4096), jpeg_parse.idct_table()

    def entropy(frm=pk['frames'], seg=pk['seg'], scan=fake, scan_bytes=len(pk['scan']), coefs=fake, blocks=pk['coef_blocks'], segments=None):
        frm, seg = np.ascontiguousarray(frm), np.ascontiguousarray(seg)
        return l.lp_jpeg_decode_entropy(scan, scan_bytes, seg.ctypes.data, fake, len(seg) if segments is None else segments, frm.ctypes.data, fake,
                                        len(frm), fake, coefs, blocks, fake, None)

    def pixels(frm=pk['frames'], blocks=pk['coef_blocks'], plane_bytes=pk['plane_bytes'], out=fake, out_bytes=pk['out_bytes'], table=K, n=None):
        frm = np.ascontiguousarray(frm)
        return l.lp_jpeg_decode_pixels(fake, blocks, frm.ctypes.data, fake, len(frm) if n is None else n, fake, table.ctypes.data, fake, plane_bytes,
                                       out, out_bytes, None)

    def changed(col, value, table='frames'):
        t = pk[table].copy()
        t[0, col] = value
        return t

    assert entropy(scan=None) == -1 and b'null' in l.lp_last_error()
    assert entropy(coefs=ctypes.c_void_p(4100)) == -1 and b'aligned' in l.lp_last_error()
    assert entropy(segments=0) == -1
    assert entropy(frm=changed(0, 0)) == -1 and b'frame 0' in l.lp_last_error() and b'65535' in l.lp_last_error()
    assert entropy(frm=changed(1, 65536)) == -1
    assert entropy(frm=changed(3, 4)) == -2 and b'4:2:0' in l.lp_last_error()
    assert entropy(frm=changed(5, 7)) == -1 and b'MCUs' in l.lp_last_error()
    assert entropy(frm=changed(12, 2)) == -1 and b'segments' in l.lp_last_error()
    assert entropy(frm=changed(19, 4)) == -1 and b'table' in l.lp_last_error()
    assert entropy(blocks=pk['coef_blocks'] - 1) == -1 and b'coefficient buffer' in l.lp_last_error()
    assert entropy(seg=changed(2, len(pk['scan']) + 1, 'seg')) == -1 and b'segment 0' in l.lp_last_error() and b'scan buffer' in l.lp_last_error()
    assert entropy(seg=changed(0, 1, 'seg')) == -1 and b'segment 0' in l.lp_last_error()
    assert pixels(out=None) == -1 and b'null' in l.lp_last_error()
    assert pixels(n=0) == -1
    assert pixels(plane_bytes=pk['plane_bytes'] - 17) == -1 and b'sample planes' in l.lp_last_error()
    assert pixels(out_bytes=pk['out_bytes'] - 1) == -1 and b'destination' in l.lp_last_error()
    assert pixels(frm=changed(10, -1)) == -1 and b'destination' in l.lp_last_error()
    big = K.copy()
    big[3] = 5000
    assert pixels(table=big) == -1 and b'IDCT' in l.lp_last_error()
    many = np.repeat(pk['frames'], 65536, axis=0)
    assert pixels(frm=many) == -2 and b'65535' in l.lp_last_error()
    # two frames that share blocks, planes, destination bytes or segments: the frames of a call are independent only on disjoint ranges
    two = jpeg_parse.pack([d, d])
    for col, word in ((8, b'coefficient'), (9, b'plane'), (10, b'destination')):
        t = two['frames'].copy()
        t[1, col] = t[0, col]
        rc = l.lp_jpeg_decode_pixels(fake, two['coef_blocks'], t.ctypes.data, fake, 2, fake, K.ctypes.data, fake, two['plane_bytes'], fake,
                                     two['out_bytes'], None)
        assert rc == -1 and b'frames 0 and 1 overlap' in l.lp_last_error() and word in l.lp_last_error(), l.lp_last_error()
    t = two['frames'].copy()
    t[1, 11] = 0
    assert l.lp_jpeg_decode_entropy(fake, len(two['scan']), two['seg'].ctypes.data, fake, len(two['seg']), t.ctypes.data, fake, 2, fake, fake,
                                    two['coef_blocks'], fake, None) == -1 and b'segment table' in l.lp_last_error()


def test_wrapper_refusals_name_the_cause():
    d = jpeg_parse.parse(_plain())
    for bad, word in (([], 'Descriptor'), ([None], 'Descriptor'), ('file.jpg', 'Descriptor')):
        with pytest.raises(ValueError, match=word):
            hipops.jpeg_decode_host(bad)
    with pytest.raises(ValueError, match='offsets'):
        hipops.jpeg_decode_host([d], offsets=[0, 1])
    with pytest.raises(ValueError, match='out'):
        hipops.jpeg_decode_host([d], offsets=[0])
    with pytest.raises(ValueError, match='lies outside'):
        hipops.jpeg_decode_host([d], out=torch.zeros(d.h * d.w * 3 + 3, dtype=torch.uint8), offsets=[4])
    with pytest.raises(ValueError, match='uint8'):
        hipops.jpeg_decode_host([d], out=torch.zeros(10000), offsets=[0])
    out = torch.full((d.h * d.w * 3 + 8,), 7, dtype=torch.uint8)
    got = hipops.jpeg_decode([d], out=out, offsets=[4])                      # a CPU buffer: the host twin
    assert got.buf is out and out[:4].tolist() == [7] * 4 and out[-4:].tolist() == [7] * 4
    assert np.array_equal(out[4:-4].numpy().reshape(d.h, d.w, 3), R.decode(d)['pixels'])
