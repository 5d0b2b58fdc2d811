"""CPU checks of the hard-edged stickman (no GPU): ``hipops.stickman_render_hard_host`` (numpy integers) against the restatement with Python
integers (tests/stickman_hard_restatement.py), with exact equality, on every case of tests/stickman_hard_cases.py; painter's order; the boundary of
the body's test; the reference's tables; and the argument checks of lp_stickman_render_hard and of the wrappers, which run before any device work."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import stickman_hard_cases as C          # noqa: E402
import stickman_hard_restatement as HR          # noqa: E402


def ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def test_reference_tables_are_the_topology_of_the_reference():
    o = ops()
    assert o.REFERENCE_PARTS == C.REFERENCE_PARTS and o.REFERENCE_PARTS_NO_OVAL == C.REFERENCE_PARTS_NO_OVAL
    assert o.REFERENCE_PARTS[0] == (0, 16, False, (1.0, 1.0, 1.0)) and o.REFERENCE_PARTS[1:] == o.REFERENCE_PARTS_NO_OVAL
    assert [(f, l, c) for f, l, c, _ in o.REFERENCE_PARTS_NO_OVAL] == [(17, 21, False), (22, 26, False), (27, 30, False), (31, 35, False),
                                                                      (36, 41, True), (42, 47, True), (48, 59, True)]
    assert [rgb for *_, rgb in o.REFERENCE_PARTS_NO_OVAL] == [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)]
    seg, part_end, colour, npoints = o.stickman_table(o.REFERENCE_PARTS)
    assert len(part_end) == 8 and npoints == 60 and len(seg) == 16 + 4 + 4 + 3 + 4 + 6 + 6 + 12          # points 60 .. 67 are not drawn
    assert o.stickman_table(o.REFERENCE_PARTS_NO_OVAL)[1][-1] == len(seg) - 16


def test_the_integer_point():
    """ties to even, the clamp, NaN and infinities -- the restatement's own arithmetic, spelled out"""
    assert [HR.integer_point(v, 8) for v in (0.0625, 0.1875, 0.3125, -0.0625, -0.1875)] == [0, 2, 2, 0, -2]          # 0.5, 1.5, 2.5, -0.5, -1.5
    assert HR.integer_point(float('nan'), 64) == -4096 and HR.integer_point(float('inf'), 64) == 8191 and HR.integer_point(float('-inf'), 64) == -4096
    assert HR.integer_point(1.0e6, 64) == 8191 and HR.integer_point(-3.0e38, 4096) == -4096 and HR.integer_point(3.0e38, 4096) == 8191
    assert HR.integer_point(1.0, 4096) == 4096 and HR.integer_point(2.0, 4096) == 8191 and HR.integer_point(-1.0, 4096) == -4096


@pytest.mark.parametrize('oval', [True, False])
@pytest.mark.parametrize('thickness', C.THICKNESSES)
@pytest.mark.parametrize('size', C.SIZES)
def test_host_twin_equals_the_restatement(size, thickness, oval):
    o = ops()
    parts = o.REFERENCE_PARTS if oval else o.REFERENCE_PARTS_NO_OVAL
    for name in C.SET_NAMES:
        pts, want = C.points(size, name), C.want(size, thickness, oval, name)
        for n in (1, 3):
            got = o.stickman_render_hard_host(pts[:n], size, thickness, parts=parts)
            assert tuple(got.shape) == (n, 3, size, size) and got.dtype == torch.float32
            assert torch.equal(got, want[:n]), (name, n, int((got != want[:n]).sum()))
            assert bool(((got == 0) | (got == 1)).all())
        assert torch.equal(o.stickman_render_hard_host(pts.reshape(C.N_MAX, 136), size, thickness, parts=parts), want)          # [..., 2P]
    if size >= 22:
        assert float(C.want(size, thickness, oval, 'faces').max()) == 1.0
        assert float(C.want(size, thickness, oval, 'all-equal').sum()) > 0          # a dot of diameter T


def test_the_box_pruning_of_the_restatement_changes_nothing():
    """the restatement visits only the pixels of a segment's box grown by ceil(T / 2); here every pixel is visited"""
    size, thickness = 22, 3
    for name in ('faces', 'outside', 'far-outside', 'one-nan'):
        pts = C.points(size, name)[0].tolist()
        ipts = [(HR.integer_point(x, size), HR.integer_point(y, size)) for x, y in pts]
        img = torch.zeros(3, size, size)
        for first, last, closed, colour in C.REFERENCE_PARTS:
            idx = list(range(first, last + 1))
            for i, j in list(zip(idx[:-1], idx[1:])) + ([(idx[-1], idx[0])] if closed else []):
                for v in range(size):
                    for u in range(size):
                        if HR.covers(u, v, *ipts[i], *ipts[j], thickness):
                            img[:, v, u] = torch.tensor(colour)
        assert torch.equal(img, C.want(size, thickness, True, name)[0]), name


@pytest.mark.parametrize('size', [22, 64])
def test_painters_order_decides_where_two_parts_cross(size):
    o = ops()
    pts, m = C.crossing_points(size), size // 2
    got = o.stickman_render_hard_host(pts, size, 2, parts=C.CROSSING_PARTS)
    assert torch.equal(got, HR.render(pts, size, C.CROSSING_PARTS, 2))
    assert got[0, :, m, m].tolist() == [1.0, 0.0, 0.0]          # the crossing: the later part
    assert got[0, :, m, 2].tolist() == [1.0, 1.0, 1.0] and got[0, :, 2, m].tolist() == [1.0, 0.0, 0.0] and got[0, :, 2, 2].tolist() == [0.0, 0.0, 0.0]
    swapped = o.stickman_render_hard_host(pts, size, 2, parts=C.CROSSING_PARTS[::-1])
    assert swapped[0, :, m, m].tolist() == [1.0, 1.0, 1.0] and torch.equal(swapped, HR.render(pts, size, C.CROSSING_PARTS[::-1], 2))


@pytest.mark.parametrize('size,thickness', [(22, 2), (64, 8)])
def test_a_pixel_exactly_on_the_boundary_of_the_body_is_covered(size, thickness):
    o = ops()
    pts, parts, c = C.boundary_case(size, thickness)
    u, half = size // 2, thickness // 2
    ax, bx = 1, size - 2
    assert HR.integer_point(float(pts[0, 0, 0]), size) == ax and HR.integer_point(float(pts[0, 1, 0]), size) == bx
    cross, l2 = (bx - ax) * half, (bx - ax) ** 2
    assert 4 * cross * cross == thickness * thickness * l2          # the case is what it claims to be
    got = o.stickman_render_hard_host(pts, size, thickness, parts=parts)
    assert torch.equal(got, HR.render(pts, size, parts, thickness))
    for v, lit in ((c - half, 1.0), (c + half, 1.0), (c - half - 1, 0.0), (c + half + 1, 0.0)):
        assert float(got[0, 1, v, u]) == lit, (v, lit)
    assert float(got[0, 0].sum()) == 0 and float(got[0, 2].sum()) == 0


def test_argument_checks_of_the_c_entry_come_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 16)()
    ptr = ctypes.addressof(buf)

    def call(points=ptr, N=1, P=68, seg=ptr, part_end=ptr, colour=ptr, L=55, parts=8, S=8, T=2, out=ptr):
        return l.lp_stickman_render_hard(points, N, P, seg, part_end, colour, L, parts, S, T, out, None)
    for null in ('points', 'seg', 'part_end', 'colour', 'out'):
        assert call(**{null: None}) == -1 and b'lp_stickman_render_hard' in l.lp_last_error() and b'null' in l.lp_last_error(), null
    # host pointers only: every one of these is refused before anything is dereferenced or launched
    for bad in (dict(N=0), dict(N=-3), dict(P=0), dict(P=257), dict(L=0), dict(L=257), dict(parts=0), dict(parts=17), dict(S=0), dict(S=4097),
                dict(S=-1), dict(T=0), dict(T=9), dict(T=-2)):
        assert call(**bad) == -1, bad
        assert b'lp_stickman_render_hard' in l.lp_last_error(), (bad, l.lp_last_error())
    assert call(N=1 << 24, S=4096) != 0 and b'launch grid' in l.lp_last_error()          # 2^24 images x 16384 workgroups


def test_wrappers_refuse_by_cause():
    o = ops()
    pts = C.points(8, 'faces')
    with pytest.raises(ValueError, match='CUDA'):
        o.stickman_render_hard(pts, 16)
    with pytest.raises(ValueError, match='fp32'):
        o.stickman_render_hard_host(pts.double(), 16)
    with pytest.raises(ValueError, match='size must be in 1 .. 4096'):
        o.stickman_render_hard_host(pts, 4097)
    with pytest.raises(ValueError, match='size must be in 1 .. 4096'):
        o.stickman_render_hard_host(pts, 0)
    for t in (0, 9):
        with pytest.raises(ValueError, match='thickness must be in 1 .. 8'):
            o.stickman_render_hard_host(pts, 16, t)
    with pytest.raises(ValueError, match='P >= 60'):
        o.stickman_render_hard_host(pts[:, :50], 16)
    with pytest.raises(ValueError, match='out must be'):
        o.stickman_render_hard_host(pts, 16, out=torch.empty(3, 3, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match='contiguous'):
        o.stickman_render_hard_host(pts, 16, out=torch.empty(3, 3, 16, 32)[..., :16])
    out = torch.full((4, 3, 16, 16), -1.0)
    ret = o.stickman_render_hard_host(pts, 16, out=out[1:])
    assert ret.data_ptr() == out[1:].data_ptr() and bool((out[0] == -1).all()) and torch.equal(out[1:], o.stickman_render_hard_host(pts, 16))
