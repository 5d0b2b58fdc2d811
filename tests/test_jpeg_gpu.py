"""csrc/jpeg.hip on the MI355X: the entropy coder against the host encoder byte for byte, the transform against the fp64 restatement, the whole
encoder through PIL and the test's own scan decoder, and the function drive.py's ``--format avi`` uses.

Coder: every coefficient table of tests/test_mjpeg_cpu.py (seeded sparse and dense at W in {8, 16, 24, 72} x H in {8, 16, 40, 80} x T in {1, 3}, the
constructed rows, the two stuffing tables found by search) through lp_jpeg_entropy_size / lp_jpeg_entropy_write, the output inside a buffer with 64
guard bytes on either side: bytes and offsets EQUAL ``hipops.jpeg_encode_host``'s, which the CPU file holds to its independent decoder; the same
call twice gives the same bytes; all tables of one size stacked as T frames give the concatenation of their single encodings (a frame's bytes do
not depend on T or on its neighbours).

Transform: tests/test_mjpeg_cpu.check_coefficients -- equal to the fp64 restatement except where its D lies within tau = 2^-8 of (n + 1/2) Q, those
flagged from the restatement alone and allowed to differ by 1, at most 1 / 16 of a case flagged.  tau bounds the fp32 chain for |D| <= 1024: the
colour transform, 3 products with rounded constants and 3 sums below 256: 5.5 x 255 u per plane value (u = 2^-24), x 8 (the sup-norm gain of the 2-D
DCT) = 6.7e-4; the two passes 1.1e-3 (tests/test_augment_extra_gpu.py, the same chain); the division's 1024 u; together < 2^-9, doubled for the
restatement's own side of the comparison.  The CPU file checks the cap on all three planes of every case (measured there: at most 0.10 % flagged
at qualities 50 .. 90 and 1.04 % at 100).  A flat frame (value 129) puts D / Q on half-integers and is checked through the decoder instead: every
coefficient within 1 of the restatement's.

No ``main()`` run: the checkpoint fixture has no driving images on disk and ``main`` reads them through a dataloader; the fixture's generator drives
five frames through ``drive_frames`` and ``write_avi`` -- what ``main`` calls -- instead."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import jpeg_restatement as JR          # noqa: E402
import test_mjpeg_cpu as MC          # noqa: E402
from latent_pose_reenactment_amd import _lib, hipops          # noqa: E402
from latent_pose_reenactment_amd.utils import mjpeg          # noqa: E402

GUARD = 64
_HOST = {}


def host_encoding(name):
    """(bytes uint8 array, offsets list) of the host encoder for a table of the CPU file, computed once"""
    if name not in _HOST:
        data, offsets = hipops.jpeg_encode_host(coefs=torch.from_numpy(MC.coefficient_tables()[name]))
        _HOST[name] = (data.numpy(), offsets.tolist())
    return _HOST[name]


def entropy_guarded(coefs):
    """lp_jpeg_entropy_size + lp_jpeg_entropy_write through the C ABI, the output between two runs of guard bytes -> (bytes, offsets) on the host"""
    l = _lib.lib()
    c = torch.from_numpy(np.ascontiguousarray(coefs)).cuda()
    t, rows, mcus = c.shape[:3]
    header = mjpeg.jpeg_header(8 * rows, 8 * mcus, 90)
    need = l.lp_jpeg_entropy_scratch_bytes(t, rows, mcus)
    assert need > 0
    scratch = torch.full((need,), 0xC3, dtype=torch.uint8, device='cuda')          # "contents irrelevant on entry"
    offsets = torch.empty(t + 1, dtype=torch.int64, device='cuda')
    head = torch.frombuffer(bytearray(header), dtype=torch.uint8).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    assert l.lp_jpeg_entropy_size(c.data_ptr(), t, rows, mcus, len(header), scratch.data_ptr(), need, offsets.data_ptr(), stream) == 0, l.lp_last_error()
    total = int(offsets[t].item())
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    assert l.lp_jpeg_entropy_write(scratch.data_ptr(), need, t, rows, mcus, head.data_ptr(), len(header), buf.data_ptr() + GUARD, total, stream) == 0, \
        l.lp_last_error()
    buf = buf.cpu().numpy()
    assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + total:] == 0xA5), 'a guard byte was written'
    return buf[GUARD:GUARD + total], offsets.tolist()


@pytest.mark.parametrize('name', sorted(MC.coefficient_tables()))
def test_coder_equals_host_encoder(name):
    want, want_offsets = host_encoding(name)
    got, offsets = entropy_guarded(MC.coefficient_tables()[name])
    assert offsets == want_offsets
    assert np.array_equal(got, want), f'{name}: first difference at byte {int(np.flatnonzero(got != want)[0]) if len(got) == len(want) else "(lengths)"}'
    again, offsets2 = entropy_guarded(MC.coefficient_tables()[name])
    assert offsets2 == offsets and np.array_equal(again, got), 'the same call twice gives other bytes'
    # and through the public wrapper, which allocates at the exact size
    data, offs = hipops.jpeg_entropy(torch.from_numpy(MC.coefficient_tables()[name]).cuda(), mjpeg.jpeg_header(*(8 * s for s in got_shape(name)), 90))
    assert offs.tolist() == want_offsets and np.array_equal(data.cpu().numpy(), want)


def got_shape(name):
    return MC.coefficient_tables()[name].shape[1:3]


def test_coder_on_stacked_tables_is_the_concatenation():
    groups = {}
    for name, c in MC.coefficient_tables().items():
        groups.setdefault(c.shape[1:3], []).append(name)
    assert max(len(v) for v in groups.values()) >= 4
    for shape, names in groups.items():
        stack = np.concatenate([MC.coefficient_tables()[n] for n in names])
        got, offsets = entropy_guarded(stack)
        want = np.concatenate([host_encoding(n)[0] for n in names])
        sizes = [b - a for n in names for a, b in zip(host_encoding(n)[1], host_encoding(n)[1][1:])]
        assert offsets == [0] + list(np.cumsum(sizes)), shape
        assert np.array_equal(got, want), shape


def _strided(frames):
    """the frames as the right half of a wider grid: a ``[:, :, W:]`` view, as drive_frames concatenates driver | result"""
    t, h, w, _ = frames.shape
    wide = torch.randint(0, 256, (t, h, 2 * w, 3), dtype=torch.uint8, device='cuda', generator=torch.Generator('cuda').manual_seed(1))
    wide[:, :, w:] = frames
    view = wide[:, :, w:]
    assert not view.is_contiguous() or w == 0
    return view


@pytest.mark.parametrize('h,w', MC.TRANSFORM_SIZES)
def test_transform_against_restatement(h, w):
    for t in (1, 3):
        for kind, frames in MC.transform_frames(h, w, t).items():
            dev = torch.from_numpy(frames).cuda()
            for layout, x in (('contiguous', dev), ('strided', _strided(dev))):
                for quality in MC.TRANSFORM_QUALITIES:
                    got = hipops.jpeg_transform(x, quality)
                    assert got.dtype == torch.int16 and tuple(got.shape) == (t, -(-h // 8), -(-w // 8), 3, 64)
                    share, wrong = MC.check_coefficients(got.cpu().numpy(), frames, quality, f'{kind} {h}x{w} T{t} {layout} q{quality}')
                    print(f'device transform {kind:13s} {h:2d}x{w:2d} T{t} {layout:10s} quality {quality:3d}: flagged {100 * share:.3f} %, '
                          f'differing {100 * wrong:.4f} %')
                    if layout == 'strided':
                        assert torch.equal(got, hipops.jpeg_transform(dev, quality)), 'the strided view gives other coefficients'


def test_flat_frame_through_the_decoder():
    frames = np.full((1, 24, 40, 3), 129, dtype=np.uint8)
    data, offsets = hipops.jpeg_encode(torch.from_numpy(frames).cuda(), 90)
    got = MC.decode(MC.split(data, offsets)[0])['coefs']
    k, _ = JR.quantise(JR.dct_coefficients(frames), 90)
    assert np.abs(got - k[0]).max() <= 1
    assert np.abs(MC.pil_pixels(MC.split(data, offsets)[0]) - 129).max() <= 2


def test_end_to_end_256x512():
    frames = JR.image('smooth_noise', 256, 512, seed=4, t=2)
    dev = torch.from_numpy(frames).cuda()
    data, offsets = hipops.jpeg_encode(dev, 90)
    assert data.is_cuda and data.dtype == torch.uint8 and offsets.dtype == torch.int64 and tuple(offsets.shape) == (3,)
    assert int(offsets[0]) == 0 and int(offsets[2]) == data.numel()
    files = MC.split(data, offsets)
    for t, blob in enumerate(files):
        im = Image.open(io.BytesIO(blob))
        assert im.size == (512, 256) and im.mode == 'RGB'
        r = MC.fidelity_ratio(frames[t], blob, 90)
        print(f'fidelity device 256x512 frame {t} quality 90: r = {r:.4f} (gate {MC.R_GATE:.4f}), {len(blob)} bytes')
        assert r <= MC.R_GATE
    coefs = hipops.jpeg_transform(dev, 90).cpu().numpy()
    d = MC.decode(files[1])
    assert len(d['intervals']) == 32 and np.array_equal(d['coefs'], coefs[1]), 'the scan does not hold the device\'s own coefficients'
    # the same bytes whatever T: the second frame alone
    alone, offs = hipops.jpeg_encode(dev[1:], 90)
    assert alone.cpu().numpy().tobytes() == files[1]


def test_write_avi_in_chunks(tmp_path, monkeypatch):
    """what ``main`` does for ``--format avi``, on frames the checkpoint fixture's generator drove: T = 5 in chunks of 2"""
    import test_checkpoint_fixture as CF
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    CF._register()
    import drive
    torch.set_grad_enabled(True)
    with torch.no_grad():
        E, G, _ = drive.load_for_inference(CF.CKPT, '/nonexistent', 'cuda:0')
        drivers = torch.rand(5, 1, 3, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
        video = torch.cat([drive.drive_frames(E, G, {'pose_input_rgbs': drivers[i:i + 2]}) for i in range(0, 5, 2)])
    assert video.is_cuda and tuple(video.shape) == (5, 32, 64, 3)
    path = tmp_path / 'driver.avi'
    assert drive.write_avi(path, video, fps=25, quality=90, chunk=2) == os.path.getsize(path)
    pixels = MC.check_avi(path.read_bytes(), 5, 32, 64, 25)
    whole = MC.split(*hipops.jpeg_encode(video, 90))
    for t in range(5):
        assert np.array_equal(pixels[t], MC.pil_pixels(whole[t]))
        # the panels (driver | result) come back as well as from PIL's own encoder: the gate of the fidelity test
        assert MC.fidelity_ratio(video[t].cpu().numpy(), whole[t], 90) <= MC.R_GATE
    with pytest.raises(ValueError, match='uint8'):
        drive.write_avi(tmp_path / 'bad.avi', video.float())


def test_refusals_name_the_cause_and_leave_no_device_error():
    ok = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device='cuda')
    for bad, word in ((ok.float(), 'uint8'), (ok[0], '4-D'), (torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device='cuda'), 'C = 4'),
                      (torch.zeros(1, 0, 8, 3, dtype=torch.uint8, device='cuda'), 'empty')):
        with pytest.raises(ValueError, match=word):
            hipops.jpeg_encode(bad)
    with pytest.raises(ValueError, match='quality'):
        hipops.jpeg_encode(ok, quality=0)
    with pytest.raises(ValueError, match='int16'):
        hipops.jpeg_entropy(torch.zeros(1, 1, 1, 3, 64, device='cuda'), b'')
    torch.cuda.synchronize()
    data, offsets = hipops.jpeg_encode(ok, 90)
    torch.cuda.synchronize()
    assert Image.open(io.BytesIO(MC.split(data, offsets)[0])).size == (8, 8)
