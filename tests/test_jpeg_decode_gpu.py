"""csrc/jpeg_decode.hip on the MI355X: every file of tests/jpeg_decode_cases.py against the restatement bit for bit (coefficients, sample planes,
pixels, status 0), all files mixed in one call and alone, guard bytes and fallback regions around the destinations, the poisoned-buffer
differential, a corrupt stream between two good ones, ``frames.prepare`` with ``decode_jpeg_on_gpu`` against ``prepare_host``, and a graph capture
of the decode launches plus lp_frames_prepare.  The corrupt stream checks isolation and bounded reads on valid memory; nothing here tries to make
a kernel misbehave.  The largest frame is 64 x 64."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
pytestmark = pytest.mark.gpu

import guarded_alloc as GA          # noqa: E402
import jpeg_decode_cases as C          # noqa: E402
import test_jpeg_decode_cpu as DC          # noqa: E402
from latent_pose_reenactment_amd import _lib, frames, hipops          # noqa: E402
from latent_pose_reenactment_amd.utils import jpeg_parse          # noqa: E402

GUARD = 96          # bytes of 0xA5 in front of, between and behind the destination regions


@pytest.mark.parametrize('sampling,quality', C.GROUPS)
def test_device_equals_restatement(sampling, quality):
    files = C.group(sampling, quality)
    got = hipops.jpeg_decode([d for _, _, d, _ in files])
    assert got.buf.is_cuda and got.status.is_cuda and got.coefs.dtype == torch.int16
    DC.check_decoded_group(got, files)


def all_files():
    return [f for g in C.GROUPS for f in C.group(*g)]


def test_mixed_call_with_guards_twice_and_alone():
    """all files in ONE call, every destination between guard bytes, a 50-byte 'fallback frame' copied in beforehand in front of every 42nd file: the pixels are the
    restatement's, guards and fallback regions are intact, the second run gives the same bytes; a file alone gives the bytes it gives here"""
    files = all_files()
    layout, at = [], GUARD
    rng = np.random.default_rng(5)
    host = np.full(GUARD + sum(d.h * d.w * 3 + GUARD for _, _, d, _ in files) + 40 * (GUARD + 50), 0xA5, dtype=np.uint8)
    fallback, offsets = [], []
    for i, (_, _, d, _) in enumerate(files):
        if i % 42 == 0:
            host[at:at + 50] = rng.integers(0, 256, 50)
            fallback.append((at, host[at:at + 50].copy()))
            at += 50 + GUARD
        offsets.append(at)
        at += d.h * d.w * 3 + GUARD
    assert at == host.size
    runs = []
    for _ in range(2):
        out = torch.from_numpy(host).cuda()
        got = hipops.jpeg_decode([d for _, _, d, _ in files], out=out, offsets=offsets)
        assert got.buf is out and got.status.cpu().tolist() == [0] * len(files)
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]), 'the same call twice gives other bytes'
    written = np.zeros(host.size, dtype=bool)
    for (name, _, d, want), off in zip(files, offsets):
        n = d.h * d.w * 3
        written[off:off + n] = True
        assert np.array_equal(runs[0][off:off + n].reshape(d.h, d.w, 3), want['pixels']), name
    assert np.array_equal(runs[0][~written], host[~written]), 'a guard byte or a fallback region was written'
    assert all(np.array_equal(runs[0][a:a + 50], v) for a, v in fallback)
    # alone: every 61st file of the list (61 is prime to the list's periods: all sizes, samplings, qualities and variants occur)
    for i in range(0, len(files), 61):
        name, _, d, want = files[i]
        alone = hipops.jpeg_decode([d])
        assert alone.status.cpu().tolist() == [0]
        assert np.array_equal(alone.buf.cpu().numpy(), runs[0][offsets[i]:offsets[i] + d.h * d.w * 3]), name


def test_nothing_depends_on_fresh_memory():
    """``guarded_alloc.differential`` around ``hipops.jpeg_decode``: destination, coefficients (also behind every EOB), planes and status from
    poisoned, fenced allocations -- bit-identical under both fills, fences intact"""
    files = [C.group(s, q)[i] for s, q, i in (('grey', 30, 50), (0, 1, 13), (1, 75, 40), (2, 90, 83), (2, 100, 60), (0, 30, 3))]
    ds = [d for _, _, d, _ in files]
    got = GA.differential(lambda: hipops.jpeg_decode(ds), ())
    DC.check_decoded_group(got, files)


def test_corrupt_stream_between_two_good_ones():
    a, bad, b = DC.corrupt_case()
    sizes = [d.h * d.w * 3 for d in (a, bad, b)]
    offsets = [GUARD, 2 * GUARD + sizes[0], 3 * GUARD + sizes[0] + sizes[1]]
    host = torch.full((offsets[2] + sizes[2] + GUARD,), 0xA5, dtype=torch.uint8)
    got = hipops.jpeg_decode([a, bad, b], out=host.cuda(), offsets=offsets)
    status = got.status.cpu().tolist()
    assert status[0] == 0 and status[2] == 0 and status[1] == hipops.jpeg_decode_host([bad]).status.item() != 0
    out = got.buf.cpu()
    twin = hipops.jpeg_decode_host([a, bad, b], out=host.clone(), offsets=offsets)
    assert torch.equal(out, twin.buf) and torch.equal(got.coefs.cpu(), twin.coefs)          # the failed frame too: what it decoded stays, then zeros
    for d, i in ((a, 0), (b, 2)):
        alone = hipops.jpeg_decode([d])
        assert torch.equal(alone.buf.cpu(), out[offsets[i]:offsets[i] + sizes[i]])
    inside = torch.zeros(host.numel(), dtype=torch.bool)
    for off, n in zip(offsets, sizes):
        inside[off:off + n] = True
    assert bool((out[~inside] == 0xA5).all()), 'a guard byte was written'


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return DC.build_jpeg_tree(tmp_path_factory.mktemp('voxceleb2_jpeg_gpu'))


def test_prepare_with_the_flag_on_the_device_equals_prepare_host(tree):
    """the loader with ``decode_jpeg_on_gpu`` on the device against the same loader on the CPU (host twin + ``prepare_host``): per sample under the
    gate of tests/test_frames_gpu.py's loader comparison; the decoded bytes are equal, so nothing is added to it.  With ``blur_padded_bands`` on
    top the batch is BIT-equal to the unflagged device route fed the decoded bytes: the same launches on the same buffer."""
    import test_voxceleb2_loader_cpu as L
    split = L.video_split(tree)
    flags = dict(val_split_path=split, batch_size=6, decode_jpeg_on_gpu=True)
    blurred = L.loader_for(L.make_args(tree, device='cuda', blur_padded_bands=True, **flags), 'val')
    raw = next(iter(blurred.loader))
    full = DC.full_buffer(raw)
    want = frames.prepare({k: raw[k] for k in ('table', 'label', 'frames', 'pose')} | {'buf': full}, L.SIZE, 'cuda', blur_padded_bands=True)
    got = frames.prepare(raw, L.SIZE, 'cuda', blur_padded_bands=True)
    assert all(torch.equal(got[0][k], want[0][k]) for k in want[0]) and torch.equal(got[1]['real_segm'], want[1]['real_segm'])
    device_loader = L.loader_for(L.make_args(tree, device='cuda', **flags), 'val')
    device = list(device_loader)
    host = list(L.loader_for(L.make_args(tree, device='cpu', **flags), 'val'))
    assert len(device) == len(host) == 1 and not device_loader.pending
    (dd, dt), (hd, ht) = device[0], host[0]
    assert set(dd) == set(hd) and torch.equal(dt['label'].cpu(), ht['label'])
    worst = 0.0
    for b in range(hd['enc_rgbs'].shape[0]):
        g_img, g_msk, g_prod = L.tolerance(L.PATHS[b])
        for got, want, gate in ((dd['enc_rgbs'], hd['enc_rgbs'], g_img), (dd['pose_input_rgbs'], hd['pose_input_rgbs'], g_img),
                                (dt['real_segm'], ht['real_segm'], g_msk), (dd['target_rgbs'], hd['target_rgbs'], g_prod)):
            err = (got[b].cpu().double() - want[b].double()).abs().max().item()
            worst = max(worst, err / gate)
            assert err <= gate, (L.PATHS[b], err, gate)
    print(f'[jpeg_decode] loader with the flag on the device vs prepare_host: worst difference / gate {worst:.2f}')


def test_graph_capture_replays_to_the_same_bytes(tree):
    """the two decode launches and lp_frames_prepare captured on static inputs: a replay into cleared outputs gives the bytes of the eager run"""
    import test_voxceleb2_loader_cpu as L
    raw = next(iter(L.loader_for(L.make_args(tree, val_split_path=L.video_split(tree), batch_size=6, decode_jpeg_on_gpu=True), 'val').loader))
    pk, table, nbytes = raw['jpeg'], raw['table'], int(raw['nbytes'])
    eager_buf = torch.zeros(nbytes, dtype=torch.uint8, device='cuda')
    for d, s, n in raw['regions'].tolist():
        eager_buf[d:d + n] = raw['buf'][s:s + n].cuda()
    start = eager_buf.clone()
    eager = hipops.frames_prepare(hipops.jpeg_decode(pk, out=eager_buf).buf, table, L.SIZE)
    l = _lib.lib()
    n, nseg, blocks, planes_n = pk['frames'].shape[0], pk['seg'].shape[0], int(pk['coef_blocks']), int(pk['plane_bytes'])
    dev = {k: pk[k].cuda() for k in ('scan', 'seg', 'frames', 'qt', 'huffman')}
    buf, table_dev = start.clone(), table.cuda()
    coefs = torch.empty((blocks, 64), dtype=torch.int16, device='cuda')
    planes = torch.empty(planes_n, dtype=torch.uint8, device='cuda')
    status = torch.empty(n, dtype=torch.int32, device='cuda')
    counts = frames.check_table(table, nbytes, L.SIZE)
    outs = [torch.empty(c, 3, L.SIZE, L.SIZE, device='cuda') for c in counts]
    K = jpeg_parse.idct_table()

    def launches():
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert l.lp_jpeg_decode_entropy(dev['scan'].data_ptr(), pk['scan'].numel(), pk['seg'].data_ptr(), dev['seg'].data_ptr(), nseg,
                                        pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['huffman'].data_ptr(), coefs.data_ptr(), blocks,
                                        status.data_ptr(), stream) == 0, l.lp_last_error()
        assert l.lp_jpeg_decode_pixels(coefs.data_ptr(), blocks, pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['qt'].data_ptr(),
                                       K.ctypes.data, planes.data_ptr(), planes_n, buf.data_ptr(), nbytes, stream) == 0, l.lp_last_error()
        assert l.lp_frames_prepare(buf.data_ptr(), nbytes, table.data_ptr(), table_dev.data_ptr(), table.shape[0], L.SIZE, outs[0].data_ptr(), counts[0],
                                   outs[1].data_ptr(), counts[1], outs[2].data_ptr(), counts[2], stream) == 0, l.lp_last_error()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launches()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for _ in range(2):
        buf.copy_(start)
        status.fill_(7)
        for o in outs:
            o.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * n and torch.equal(buf, eager_buf)
        assert all(torch.equal(o, e) for o, e in zip(outs, eager))


def test_wrapper_refusals_leave_no_device_error():
    d = C.group(2, 90)[0][2]
    with pytest.raises(ValueError, match='lies outside'):
        hipops.jpeg_decode([d], out=torch.zeros(d.h * d.w * 3, dtype=torch.uint8, device='cuda'), offsets=[1])
    pk = jpeg_parse.pack([d])
    pk['frames'][0, 5] += 1
    with pytest.raises(ValueError, match='MCUs'):
        hipops.jpeg_decode(pk)
    torch.cuda.synchronize()
    assert hipops.jpeg_decode([d]).status.cpu().tolist() == [0]
