"""csrc/png.hip on the MI355X: bytes and offsets EQUAL to ``hipops.png_encode_host`` on every case of tests/test_png_cpu.py, which holds that twin to
the byte-wise restatement, to PIL and to zlib.  Nothing here has a tolerance.

Each image case and each constructed stream goes through the C ABI with the output inside a buffer with 64 guard bytes on either side and a scratch
that holds 0xC3 on entry, twice, and through the public wrapper; frames of one shape are stacked (up to 12 in a call) and must give the concatenation
of their single encodings; ``guarded_alloc.differential`` runs ``png_encode`` and the deflate stage over poisoned workspaces; a captured graph of
filter + deflate-size is replayed on new frames; and the two call sites -- ``drive.write_png_frames_gpu`` and ``visualize.save_png(encoder='gpu')``
-- are checked through PIL, their default (PIL) routes byte for byte against PIL itself and on the absence of any png launch.

No ``main()`` run of drive.py: the checkpoint fixture has no driving images on disk (tests/test_jpeg_gpu.py); five frames its generator drove go
through ``write_png_frames_gpu`` -- what ``main`` calls -- instead."""
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

import guarded_alloc as GA          # noqa: E402
import test_png_cpu as PC          # noqa: E402
from latent_pose_reenactment_amd import _lib, hipops          # noqa: E402

GUARD = 64


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def deflate_guarded(filtered, head):
    """lp_png_deflate_size + lp_png_write through the C ABI on a device stream table [T, L], the output between two runs of guard bytes, the scratch
    full of 0xC3 on entry -> (bytes, offsets) on the host"""
    l = _lib.lib()
    t, n = filtered.shape
    need = l.lp_png_deflate_scratch_bytes(t, n)
    assert need > 0
    scratch = torch.full((need,), 0xC3, dtype=torch.uint8, device='cuda')
    offsets = torch.full((t + 1,), -7, dtype=torch.int64, device='cuda')
    assert l.lp_png_deflate_size(filtered.data_ptr(), t, n, scratch.data_ptr(), need, offsets.data_ptr(), stream_ptr()) == 0, l.lp_last_error()
    total = int(offsets[t].item())
    buf = torch.full((total + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    head_c = (ctypes.c_ubyte * 45)(*head)
    assert l.lp_png_write(scratch.data_ptr(), need, t, n, ctypes.addressof(head_c), offsets.data_ptr(), buf.data_ptr() + GUARD, total,
                          stream_ptr()) == 0, l.lp_last_error()
    buf = buf.cpu().numpy()
    assert np.all(buf[:GUARD] == 0xA5) and np.all(buf[GUARD + total:] == 0xA5), 'a guard byte of the output was written'
    return buf[GUARD:GUARD + total].tobytes(), offsets.tolist()


def encode_guarded(frames):
    """lp_png_filter into a guarded workspace, then ``deflate_guarded``; ``frames``: a device tensor [T, H, W, C], any strides"""
    l = _lib.lib()
    t, h, w, c = frames.shape
    n = h * (1 + w * c)
    work = torch.full((t * n + 2 * GUARD,), 0x3C, dtype=torch.uint8, device='cuda')
    strides = (ctypes.c_longlong * 4)(*frames.stride())
    assert l.lp_png_filter(frames.data_ptr(), ctypes.addressof(strides), t, h, w, c, work.data_ptr() + GUARD, stream_ptr()) == 0, l.lp_last_error()
    edge = work.cpu().numpy()
    assert np.all(edge[:GUARD] == 0x3C) and np.all(edge[GUARD + t * n:] == 0x3C), 'a guard byte of the filter workspace was written'
    return deflate_guarded(work[GUARD:GUARD + t * n].view(t, n), hipops._png_head(h, w, c))


def first_difference(got, want):
    if len(got) != len(want):
        return f'lengths {len(got)} and {len(want)}'
    return f'first difference at byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}'


@pytest.mark.parametrize('name', sorted(PC.image_cases()))
def test_device_equals_host_twin(name):
    frames = PC.image_cases()[name]
    want, want_offsets = PC.host_encoding(name)
    dev = torch.from_numpy(frames).cuda()
    got, offsets = encode_guarded(dev)
    assert offsets == want_offsets
    assert got == want, f'{name}: {first_difference(got, want)}'
    again, offsets2 = encode_guarded(dev)
    assert offsets2 == offsets and again == got, 'the same call twice gives other bytes'
    data, offs = hipops.png_encode(dev)          # the public wrapper, which allocates at the exact size
    assert data.is_cuda and data.dtype == torch.uint8 and offs.dtype == torch.int64
    assert offs.tolist() == want_offsets and data.cpu().numpy().tobytes() == want
    assert torch.equal(hipops.png_filter(dev).cpu(), hipops.png_filter_host(torch.from_numpy(frames)))


def test_stacked_frames_give_the_concatenation():
    groups = {}
    for name, frames in PC.image_cases().items():
        groups.setdefault(frames.shape[1:], []).append(name)
    # twelve frames of one shape in one call: the four 64 x 64 RGB frames three times over
    rgb64 = [n for n in groups[(64, 64, 3)]]
    assert sum(len(PC.image_cases()[n]) for n in rgb64) == 4
    groups[(64, 64, 3)] = rgb64 * 3
    assert max(sum(len(PC.image_cases()[n]) for n in names) for names in groups.values()) == 12
    for shape, names in groups.items():
        stack = torch.from_numpy(np.concatenate([PC.image_cases()[n] for n in names])).cuda()
        got, offsets = encode_guarded(stack)
        files = [f for n in names for f in PC.split(*PC.host_encoding(n))]
        assert offsets == [0] + list(np.cumsum([len(f) for f in files])), shape
        assert got == b''.join(files), shape


def test_strided_half_grid_view_and_its_surroundings():
    frames = PC.image_cases()['smooth_noise_64']
    view = PC.half_grid_view(frames)
    wide = view._base.cuda()
    before = wide.clone()
    dev_view = wide[:, :, frames.shape[2]:]
    assert not dev_view.is_contiguous()
    got, offsets = encode_guarded(dev_view)
    assert (got, offsets) == PC.host_encoding('smooth_noise_64')
    data, offs = hipops.png_encode(dev_view)
    assert data.cpu().numpy().tobytes() == got and offs.tolist() == offsets
    assert torch.equal(wide, before), 'the grid around the sliced input changed'


@pytest.mark.parametrize('name', sorted(PC.stream_cases()))
def test_constructed_streams_on_the_device(name):
    f = PC.stream_cases()[name]
    want, want_offsets = PC.host_stream_encoding(name)
    dev = torch.from_numpy(f)[None].cuda()
    got, offsets = deflate_guarded(dev, hipops._png_stream_head(len(f)))
    assert offsets == want_offsets and got == want, f'{name}: {first_difference(got, want)}'
    data, offs = hipops.png_deflate(dev)
    assert offs.tolist() == want_offsets and data.cpu().numpy().tobytes() == want
    PC.check_file(got, f)
    # the same stream twice in one call: the same file twice
    got2, offsets2 = deflate_guarded(torch.cat((dev, dev)), hipops._png_stream_head(len(f)))
    assert got2 == want + want and offsets2 == [0, len(want), 2 * len(want)]


def test_nothing_depends_on_what_the_workspaces_held():
    frames = torch.from_numpy(np.concatenate([PC.image_cases()[n] for n in ('half_noise_half_flat',)]))
    data, offsets = GA.differential(hipops.png_encode, (frames,), device='cuda')
    assert (data.cpu().numpy().tobytes(), offsets.tolist()) == PC.host_encoding('half_noise_half_flat')
    mixed = torch.from_numpy(np.concatenate([PC.image_cases()[n] for n in ('smooth_64', 'masked_smooth_noise_64')]))
    GA.differential(hipops.png_encode, (PC.half_grid_view(mixed.numpy()),), device='cuda')
    stream = torch.from_numpy(PC.stream_cases()['three_segments_of_levels'])[None]
    data, offsets = GA.differential(hipops.png_deflate, (stream,), device='cuda')
    assert (data.cpu().numpy().tobytes(), offsets.tolist()) == PC.host_stream_encoding('three_segments_of_levels')


def test_graph_of_filter_and_deflate_size_replays_on_new_frames():
    l = _lib.lib()
    first, second = PC.image_cases()['smooth_noise_64'], PC.image_cases()['masked_smooth_noise_64']
    t, h, w, c = first.shape
    n = h * (1 + w * c)
    static = torch.from_numpy(first).cuda()
    strides = (ctypes.c_longlong * 4)(*static.stride())
    filtered = torch.zeros((t, n), dtype=torch.uint8, device='cuda')
    need = l.lp_png_deflate_scratch_bytes(t, n)
    scratch = torch.zeros(need, dtype=torch.uint8, device='cuda')
    offsets = torch.zeros(t + 1, dtype=torch.int64, device='cuda')

    def launches():
        assert l.lp_png_filter(static.data_ptr(), ctypes.addressof(strides), t, h, w, c, filtered.data_ptr(), stream_ptr()) == 0
        assert l.lp_png_deflate_size(filtered.data_ptr(), t, n, scratch.data_ptr(), need, offsets.data_ptr(), stream_ptr()) == 0

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    head = hipops._png_head(h, w, c)
    head_c = (ctypes.c_ubyte * 45)(*head)
    for frames, name in ((second, 'masked_smooth_noise_64'), (first, 'smooth_noise_64')):
        static.copy_(torch.from_numpy(frames))
        scratch.fill_(0x5A)
        offsets.fill_(-1)
        graph.replay()
        total = int(offsets[t].item())
        out = torch.zeros(total, dtype=torch.uint8, device='cuda')
        assert l.lp_png_write(scratch.data_ptr(), need, t, n, ctypes.addressof(head_c), offsets.data_ptr(), out.data_ptr(), total, stream_ptr()) == 0
        assert (out.cpu().numpy().tobytes(), offsets.tolist()) == PC.host_encoding(name), name


def _driven_frames():
    import test_checkpoint_fixture as CF
    CF._register()
    import drive
    torch.set_grad_enabled(True)
    with torch.no_grad():
        E, G, _ = drive.load_for_inference(CF.CKPT, '/nonexistent', 'cuda:0')
        drivers = torch.rand(5, 1, 3, 32, 32, generator=torch.Generator().manual_seed(9)).cuda()
        video = torch.cat([drive.drive_frames(E, G, {'pose_input_rgbs': drivers[i:i + 2]}) for i in range(0, 5, 2)])
    assert video.is_cuda and tuple(video.shape) == (5, 32, 64, 3)
    return drive, video


def _pil_bytes(array):
    b = io.BytesIO()
    Image.fromarray(array).save(b, 'PNG')
    return b.getvalue()


def test_write_png_frames_gpu_in_chunks_and_the_default_route(tmp_path, monkeypatch):
    """what ``main`` does for ``--format png``: ``--png_encoder gpu`` on five frames in chunks of two, and the default route untouched"""
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    drive, video = _driven_frames()
    host = video.cpu().numpy()
    paths = drive.write_png_frames_gpu(tmp_path / 'gpu', video, chunk=2)
    assert [p.name for p in paths] == [f'{t:06}.png' for t in range(5)]
    monkeypatch.setattr(hipops, 'PROFILE', [])
    pil_paths = drive.write_png_frames(tmp_path / 'pil', host)
    assert hipops.PROFILE == [], 'the default route launched something'
    assert [p.name for p in pil_paths] == [p.name for p in paths]
    whole = PC.split(*hipops.png_encode(video))
    for t, (a, b) in enumerate(zip(paths, pil_paths)):
        assert b.read_bytes() == _pil_bytes(host[t]), 'the PIL route no longer writes what PIL writes'
        assert np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(b))) and np.array_equal(np.asarray(Image.open(a)), host[t])
        assert a.read_bytes() == whole[t], 'a frame\'s file depends on the chunking'
        PC.check_file(a.read_bytes(), hipops.png_filter_host(torch.from_numpy(host[t:t + 1]))[0].numpy(), host[t])
    with pytest.raises(ValueError, match='uint8'):
        drive.write_png_frames_gpu(tmp_path / 'bad', video.float())


def test_save_png_on_a_captioned_sheet(tmp_path, monkeypatch):
    from latent_pose_reenactment_amd.utils import visualize as V
    g = torch.Generator().manual_seed(6)
    d = {'enc_rgbs': torch.rand(3, 2, 3, 32, 32, generator=g).cuda(), 'pose_input_rgbs': torch.rand(3, 1, 3, 32, 32, generator=g).cuda(),
         'target_rgbs': torch.rand(3, 1, 3, 32, 32, generator=g).cuda(), 'fake_rgbs': torch.rand(3, 3, 32, 32, generator=g).cuda()}
    sheet = V.sheet(d, 2)
    assert sheet.is_cuda and sheet.shape[0] > 2 * 32 and sheet.shape[2] == 3
    want = sheet.cpu().numpy()
    V.save_png(tmp_path / 'gpu.png', sheet, encoder='gpu')
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'gpu.png')), want)
    monkeypatch.setattr(hipops, 'PROFILE', [])
    V.save_png(tmp_path / 'pil.png', sheet)
    V.save_png(tmp_path / 'pil2.png', sheet, encoder='pil')
    assert not [r for r in hipops.PROFILE if str(r[0]).startswith('png')], 'the default route launched the encoder'
    assert (tmp_path / 'pil.png').read_bytes() == _pil_bytes(want) == (tmp_path / 'pil2.png').read_bytes()
    with pytest.raises(ValueError, match='encoder'):
        V.save_png(tmp_path / 'x.png', sheet, encoder='zlib')


def test_refusals_name_the_cause_and_leave_no_device_error():
    l = _lib.lib()
    ok = torch.zeros(1, 8, 8, 3, dtype=torch.uint8, device='cuda')
    for bad, word in ((ok.float(), 'uint8'), (ok[0], '4-D'), (torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device='cuda'), 'C = 4'),
                      (torch.zeros(1, 0, 8, 3, dtype=torch.uint8, device='cuda'), 'empty')):
        with pytest.raises(ValueError, match=word):
            hipops.png_encode(bad)
    strides = (ctypes.c_longlong * 4)(*ok.stride())
    out = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    for args, word in (((0, ctypes.addressof(strides), 1, 8, 8, 3, out.data_ptr()), 'null'),
                       ((ok.data_ptr(), ctypes.addressof(strides), 0, 8, 8, 3, out.data_ptr()), '>= 1'),
                       ((ok.data_ptr(), ctypes.addressof(strides), 1, 8, 8, 2, out.data_ptr()), 'C must be'),
                       ((ok.data_ptr(), ctypes.addressof(strides), 70000, 40000, 8, 3, out.data_ptr()), 'launch grid'),
                       ((ok.data_ptr(), ctypes.addressof(strides), 4, 30000, 30000, 3, out.data_ptr()), '2\\^31')):
        with pytest.raises(ValueError, match=word):
            hipops._jpeg_refusal(l.lp_png_filter(*args, stream_ptr()), 'lp_png_filter')
    assert l.lp_png_deflate_scratch_bytes(0, 10) == -1 and l.lp_png_deflate_scratch_bytes(1, 0) == -1
    assert l.lp_png_deflate_scratch_bytes(200000, 16384) == -2          # the scratch beyond 2^31 - 1 bytes
    with pytest.raises(ValueError, match='scratch smaller'):
        hipops._jpeg_refusal(l.lp_png_deflate_size(ok.data_ptr(), 1, 100, out.data_ptr(), 16, out.data_ptr(), stream_ptr()), 'lp_png_deflate_size')
    torch.cuda.synchronize()
    data, offsets = hipops.png_encode(ok)
    torch.cuda.synchronize()
    assert Image.open(io.BytesIO(PC.split(data, offsets)[0])).size == (8, 8)
