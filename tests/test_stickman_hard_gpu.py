"""GPU checks of the hard-edged stickman (csrc/stickman_hard.hip -> hipops.stickman_render_hard): the kernel against the restatement with Python
integers (tests/stickman_hard_restatement.py) on every case of tests/stickman_hard_cases.py -- S in {1, 5, 8, 22, 64}, T in {1, 2, 3, 8}, 1 and 3
images, with and without the oval, seven keypoint sets -- plus S = 96 and S = 256 once each, the crossing parts and the boundary of the body's test:
EXACT equality, no tolerance, no flagged pixels.  Then the wrapper: ``out=`` an unaligned slice with guard values around it (both store paths),
all cases of one S in one call and twice, poisoned and fenced buffers (tests/guarded_alloc.py), capture into a graph and replay on new keypoints,
and the refusals, which come before any launch."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
pytestmark = pytest.mark.gpu

import guarded_alloc          # noqa: E402
import stickman_hard_cases as C          # noqa: E402
import stickman_hard_restatement as HR          # noqa: E402


def ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def parts_of(oval):
    return C.REFERENCE_PARTS if oval else C.REFERENCE_PARTS_NO_OVAL


@pytest.mark.parametrize('oval', [True, False])
@pytest.mark.parametrize('thickness', C.THICKNESSES)
@pytest.mark.parametrize('size', C.SIZES)
def test_kernel_equals_the_restatement(size, thickness, oval):
    o = ops()
    for name in C.SET_NAMES:
        pts, want = C.points(size, name).cuda(), C.want(size, thickness, oval, name)
        for n in (1, 3):
            got = o.stickman_render_hard(pts[:n], size, thickness, parts=parts_of(oval))
            assert tuple(got.shape) == (n, 3, size, size) and got.dtype == torch.float32
            assert torch.equal(got.cpu(), want[:n]), (name, n, int((got.cpu() != want[:n]).sum()))
        assert torch.equal(o.stickman_render_hard(pts.reshape(C.N_MAX, 136), size, thickness, parts=parts_of(oval)).cpu(), want)          # [..., 2P]


@pytest.mark.parametrize('size,thickness,oval', [(96, 2, True), (256, 2, True)])
def test_kernel_equals_the_restatement_on_several_workgroups_per_image(size, thickness, oval):
    o = ops()
    for name in ('faces', 'outside', 'far-outside'):
        pts = C.points(size, name)[:2]
        got = o.stickman_render_hard(pts.cuda(), size, thickness, parts=parts_of(oval)).cpu()
        want = HR.render(pts, size, parts_of(oval), thickness)
        assert torch.equal(got, want), (name, int((got != want).sum()))
        assert float(got.max()) == 1.0 and bool(((got == 0) | (got == 1)).all())


def test_painters_order_and_the_boundary_of_the_body():
    o = ops()
    for size in (22, 64):
        pts = C.crossing_points(size)
        for parts in (C.CROSSING_PARTS, C.CROSSING_PARTS[::-1]):
            got = o.stickman_render_hard(pts.cuda(), size, 2, parts=parts).cpu()
            assert torch.equal(got, HR.render(pts, size, parts, 2))
            assert got[0, :, size // 2, size // 2].tolist() == list(parts[1][3])          # the crossing: the later part
    for size, thickness in ((22, 2), (64, 8)):
        pts, parts, c = C.boundary_case(size, thickness)
        got = o.stickman_render_hard(pts.cuda(), size, thickness, parts=parts).cpu()
        assert torch.equal(got, HR.render(pts, size, parts, thickness))
        half = thickness // 2
        assert float(got[0, 1, c - half, size // 2]) == 1.0 and float(got[0, 1, c + half, size // 2]) == 1.0          # 4 cross^2 == T^2 L2: covered
        assert float(got[0, 1, c - half - 1, size // 2]) == 0.0 and float(got[0, 1, c + half + 1, size // 2]) == 0.0


@pytest.mark.parametrize('size', [22, 64])          # S % 4 != 0: pixel stores; S % 4 == 0: 16-byte stores where the slice is aligned, pixel stores where not
def test_out_may_be_an_unaligned_slice_between_guard_values(size):
    o = ops()
    pts = C.points(size, 'faces').cuda()
    fresh = o.stickman_render_hard(pts, size)
    assert fresh.data_ptr() % 16 == 0
    count = C.N_MAX * 3 * size * size
    for lead in (4, 1, 3):          # elements in front of the slice: 16-byte aligned, and two that are not
        flat = torch.full((lead + count + 5,), -7.0, device='cuda')
        out = flat[lead:lead + count].view(C.N_MAX, 3, size, size)
        assert (out.data_ptr() % 16 == 0) == (lead == 4)
        ret = o.stickman_render_hard(pts, size, out=out)
        assert ret.data_ptr() == out.data_ptr() and torch.equal(out, fresh)
        assert bool((flat[:lead] == -7).all()) and bool((flat[lead + count:] == -7).all())          # the guard values in front and behind


@pytest.mark.parametrize('size', C.SIZES)
def test_all_cases_of_one_size_in_one_call_and_twice(size):
    o = ops()
    for thickness in (2, 3):
        every = torch.cat([C.points(size, name) for name in C.SET_NAMES]).cuda()
        first = o.stickman_render_hard(every, size, thickness)
        second = o.stickman_render_hard(every, size, thickness)
        assert torch.equal(first, second)          # bit-identical from run to run
        for i, name in enumerate(C.SET_NAMES):
            alone = o.stickman_render_hard(C.points(size, name).cuda(), size, thickness)
            assert torch.equal(first[i * C.N_MAX:(i + 1) * C.N_MAX], alone), name


@pytest.mark.parametrize('size', [22, 64])
def test_poisoned_and_fenced_buffers(size):
    o = ops()
    o.stickman_render_hard(C.points(size, 'faces').cuda(), size)          # (the polyline table reaches the device outside the fence)
    for name in ('faces', 'far-outside'):
        plain = guarded_alloc.differential(lambda p: o.stickman_render_hard(p, size, 3), (C.points(size, name),), device='cuda')
        assert torch.equal(plain.cpu(), C.want(size, 3, True, name))


def test_capture_and_replay_on_new_keypoints():
    o = ops()
    s = 64
    first, second = C.faces(4, seed=1).reshape(2, 2, 136).cuda(), C.faces(4, seed=9).reshape(2, 2, 136).cuda()
    static_in = first.clone()
    static_out = torch.zeros(2, 2, 3, s, s, device='cuda')
    o.stickman_render_hard(static_in, s, out=static_out)          # eager: the polyline table reaches the device outside the capture
    want_first, want_second = o.stickman_render_hard(first, s), o.stickman_render_hard(second, s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o.stickman_render_hard(static_in, s, out=static_out)
    static_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_first)
    static_in.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_second) and not torch.equal(want_first, want_second)
    assert torch.equal(want_second.cpu(), HR.render(second.cpu(), s, C.REFERENCE_PARTS, 2))


def test_refusals_come_before_any_launch():
    from latent_pose_reenactment_amd import _lib
    o = ops()
    pts = C.faces(C.N_MAX).cuda()
    s = 16
    with pytest.raises(ValueError, match='CUDA'):
        o.stickman_render_hard(pts.cpu(), s)
    with pytest.raises(ValueError, match='CPU'):
        o.stickman_render_hard_host(pts, s)
    with pytest.raises(ValueError, match='fp32'):
        o.stickman_render_hard(pts.double(), s)
    with pytest.raises(ValueError, match='size must be'):
        o.stickman_render_hard(pts, 4097)
    with pytest.raises(ValueError, match='thickness must be'):
        o.stickman_render_hard(pts, s, 9)
    with pytest.raises(ValueError, match='P >= 60'):
        o.stickman_render_hard(pts[:, :40], s)
    with pytest.raises(ValueError, match='contiguous'):
        o.stickman_render_hard(pts, s, out=torch.empty(C.N_MAX, 3, s, 2 * s, device='cuda')[..., :s])
    with pytest.raises(ValueError, match='out must be'):
        o.stickman_render_hard(pts, s, out=torch.empty(C.N_MAX, 3, s, s, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError, match='out must be'):
        o.stickman_render_hard(pts, s, out=torch.empty(C.N_MAX, 3, s, s))
    # the C entry: device pointers this time, every refusal leaves the output as it was
    out = torch.full((1, 3, s, s), -3.0, device='cuda')
    seg, part_end, colour, nseg, nparts, _ = o._stickman_device_table(C.REFERENCE_PARTS, pts.device)
    l = _lib.lib()
    one = pts[:1].contiguous()

    def call(N=1, P=68, L=nseg, parts=nparts, S=s, T=2):
        return l.lp_stickman_render_hard(one.data_ptr(), N, P, seg.data_ptr(), part_end.data_ptr(), colour.data_ptr(), L, parts, S, T, out.data_ptr(), None)
    for bad in (dict(N=0), dict(P=0), dict(P=257), dict(L=0), dict(L=257), dict(parts=0), dict(parts=17), dict(S=0), dict(S=4097), dict(T=0), dict(T=9)):
        assert call(**bad) == -1 and b'lp_stickman_render_hard' in l.lp_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out == -3).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), HR.render(one.cpu(), s, C.REFERENCE_PARTS, 2))
