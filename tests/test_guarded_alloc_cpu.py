"""tests/guarded_alloc.py has teeth: small fake "wrappers" written in torch on the CPU, each with ONE planted fault of the kind the GPU file
(test_buffer_discipline_gpu.py) exists to find, and the harness must flag exactly those.  A fake reaches the memory next to a tensor the way a kernel
does -- through the pointer: ``beyond(t, 1, 1)`` is the flat view of t's elements with one more on each side.  (The fakes that STORE out of bounds run
under ``Guarded`` only: in a plain run that store would land in the host allocator's own words.)"""
import os
import sys
from typing import NamedTuple, Optional

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded_alloc as GA  # noqa: E402
from guarded_alloc import Guarded, GuardError, differential  # noqa: E402

DTYPES = [torch.float32, torch.int16, torch.uint8, torch.int8, torch.int32, torch.int64]          # every dtype hipops.py allocates


def beyond(t, before, after):
    """the elements of the contiguous tensor ``t`` as a flat view, with ``before`` / ``after`` more elements of its storage on either side"""
    assert t.is_contiguous()
    return t.as_strided((before + t.numel() + after,), (1,), t.storage_offset() - before)


def fmax0(v):
    """relu as a kernel computes it: fmaxf(v, 0), which is 0 for a NaN"""
    return torch.where(v > 0, v, torch.zeros_like(v))


def inputs(n=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g), torch.randn(n, generator=g))


# ---- fake wrappers -------------------------------------------------------------------------------------------------------------------------
def good(x, g):
    ws = torch.empty(4)
    ws.copy_(x[:4] * 2)
    out = torch.empty_like(x)
    out.copy_(x * g + ws.sum())
    return out


def store_past_end(x, g):
    out = torch.empty_like(x)
    beyond(out, 0, 1).copy_(torch.cat([x, x[:1]]))
    return out


def store_before_start(x, g):
    out = torch.empty_like(x)
    beyond(out, 1, 0).copy_(torch.cat([x[:1], x]))
    return out


def last_element_unwritten(x, g):
    out = torch.empty_like(x)
    out[:-1] = x[:-1] * g[:-1]
    return out


def pad_channel_unwritten(x, g):
    """planes [N, C8] with C = 5 logical channels: channel 7 is never written"""
    planes = torch.empty((4, 8), dtype=torch.int16)
    planes[:, :7] = 0
    planes[:, :5] = (x[:20].reshape(4, 5) * 100).to(torch.int16)
    return planes


def workspace_read_before_written(x, g):
    ws = torch.empty(8)
    ws[:7] = x[:7]
    out = torch.empty(1)
    out[0] = ws.sum() * 1e-3          # slot 7 was never written
    return out


def read_past_end(x, g):
    out = torch.empty_like(x)
    out.copy_(x + 1e-6 * beyond(x, 0, 1)[1:])          # a right neighbour: element n of an n-element plane
    return out


def read_before_start(x, g):
    out = torch.empty_like(x)
    out.copy_(x + 1e-6 * beyond(x, 1, 0)[:-1])
    return out


def stale_read_behind_relu(x, g):
    out = torch.empty_like(x)
    out.copy_(x + fmax0(beyond(x, 0, 1)[1:]))          # relu(right neighbour): fmaxf gives 0 for fill A's NaN, 1e30 for fill B
    return out


def stale_read_behind_mask(x, g):
    """dx = m > 0 ? g : 0 with the mask read one element too far: false for the plain run's zero AND for fill A's NaN"""
    out = torch.empty_like(x)
    m = beyond(x, 0, 1)[1:]
    out.copy_(torch.where(m > 0, g, torch.zeros_like(g)))
    return out


class Planes(NamedTuple):
    hi: torch.Tensor
    lo: Optional[torch.Tensor]
    c: int


class PackLike:
    def __init__(self, hi, lo):
        self.hi, self.lo, self.rows = hi, lo, 3


# ---- the harness flags exactly the planted faults --------------------------------------------------------------------------------------------
def test_a_well_behaved_wrapper_passes():
    x, g = inputs()
    out = differential(good, (x, g))
    assert torch.equal(out, x * g + (x[:4] * 2).sum())


@pytest.mark.parametrize('fake,side,first,last', [(store_past_end, 'past the end', 37 * 4, 37 * 4 + 3), (store_before_start, 'before the start', -4, -1)])
@pytest.mark.parametrize('fill', ['A', 'B'])
def test_a_store_outside_the_buffer_is_named(fake, side, first, last, fill):
    x, g = inputs()
    with Guarded(fill) as ctx:
        fake(GA.guarded(x), GA.guarded(g))
        with pytest.raises(GuardError) as e:
            GA.check_guards()
    msg = str(e.value)
    assert msg.count('damaged') == 1, msg          # the one allocation, the one side
    assert f'torch.empty_like (37,) torch.float32 allocated at test_guarded_alloc_cpu.py' in msg and f'({fake.__name__})' in msg, msg
    assert f'4 bytes damaged {side}, byte offsets {first} .. {last}' in msg, msg


@pytest.mark.parametrize('fake,path', [(last_element_unwritten, 'result (37,)'), (pad_channel_unwritten, 'result (4, 8)'),
                                       (workspace_read_before_written, 'result (1,)'), (read_past_end, 'result (37,)'),
                                       (read_before_start, 'result (37,)'), (stale_read_behind_relu, 'result (37,)'),
                                       (stale_read_behind_mask, 'result (37,)')])
def test_a_result_that_depends_on_fresh_memory_is_flagged(fake, path):
    with pytest.raises(AssertionError, match='depend on what fresh memory held') as e:
        differential(fake, inputs())
    assert path in str(e.value) and not isinstance(e.value, GuardError), str(e.value)


def test_the_flagged_element_is_the_planted_one():
    with pytest.raises(AssertionError) as e:
        differential(last_element_unwritten, inputs())
    assert '1 of 37 words' in str(e.value) and 'first at flat index 36' in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:
        differential(pad_channel_unwritten, inputs())
    assert '4 of 32 words' in str(e.value) and 'first at flat index 7 (last 31)' in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:
        differential(read_past_end, inputs())
    assert '1 of 37 words' in str(e.value) and 'first at flat index 36' in str(e.value), str(e.value)
    with pytest.raises(AssertionError) as e:
        differential(read_before_start, inputs())
    assert '1 of 37 words' in str(e.value) and 'first at flat index 0 ' in str(e.value), str(e.value)


def test_relu_hides_fill_a_and_the_mask_hides_it_too_the_pair_catches_both():
    """fmaxf(NaN, 0) = 0 and NaN > 0 is false: under fill A both stale reads give the plain run's bits.  Run A is compared with the plain run first, so
    a failure that names run B says that run A passed: fill B (1e30 > 0) is what exposes them."""
    for fake in (stale_read_behind_relu, stale_read_behind_mask):
        with pytest.raises(AssertionError, match='in run plain, .* in run fill B'):
            differential(fake, inputs())
    # where the stale value is not behind a comparison, fill A's NaN shows at once
    with pytest.raises(AssertionError, match='in run fill A'):
        differential(read_past_end, inputs())


def test_unwritten_exempts_only_the_named_tensor():
    def fake(x, g):
        dx = torch.empty_like(x)
        dx.copy_(x * g)
        return {'dx': dx, 'scale_out': torch.empty(2)}          # "scale_out: not written in the bf16 modes"
    with pytest.raises(AssertionError, match='result.scale_out'):
        differential(fake, inputs())
    out = differential(fake, inputs(), unwritten=('scale_out',))
    assert torch.equal(out['dx'], inputs()[0] * inputs()[1])

    def fake2(x, g):
        return {'dx': torch.empty_like(x), 'scale_out': torch.empty(2)}
    with pytest.raises(AssertionError, match='result.dx'):
        differential(fake2, inputs(), unwritten=('scale_out',))


def test_planes_and_pack_objects_are_reached():
    def fake(x, g, bad):
        hi = torch.empty((4, 8), dtype=torch.int16)
        lo = torch.empty_like(hi)
        hi.fill_(3)
        lo[:, :(7 if bad == 'lo' else 8)] = 1
        p_hi = torch.empty(6, dtype=torch.int16)
        p_hi[:(5 if bad == 'pack' else 6)] = 2
        return [Planes(hi, lo, 5), {'pack': PackLike(p_hi, None)}]
    x, g = inputs()
    differential(lambda x, g: fake(x, g, None), (x, g))
    with pytest.raises(AssertionError, match=r'result\[0\]\.lo'):
        differential(lambda x, g: fake(x, g, 'lo'), (x, g))
    with pytest.raises(AssertionError, match=r'result\[1\]\.pack\.hi'):
        differential(lambda x, g: fake(x, g, 'pack'), (x, g))
    paths = [p for p, _ in GA.reachable(fake(x, g, None))]
    assert paths == ['result[0].hi', 'result[0].lo', 'result[0].c', 'result[1].pack.hi', 'result[1].pack.lo'], paths


def test_in_place_updates_of_fenced_inputs_are_compared_and_fresh_per_run():
    def step(p, m):
        m.mul_(0.9).add_(p, alpha=0.1)
        p.sub_(m)
        return p, m
    x, g = inputs()
    p, m = differential(step, (x, g))
    assert torch.equal(m, (g * 0.9).add_(x, alpha=0.1)) and torch.equal(p, x - m)          # every run started from the caller's values, which are untouched
    assert torch.equal(x, inputs()[0])


# ---- the allocations themselves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fill', ['A', 'B'])
@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_every_dtype_is_fenced_and_filled(dtype, fill):
    with Guarded(fill) as ctx:
        t = torch.empty((3, 5), dtype=dtype)
        rec = ctx.served(t)
        assert rec is not None and rec.nbytes == 15 * t.element_size() and len(ctx.records) == 1
        wt, val = ctx.fill.word(dtype)
        assert t.dtype == dtype and t.shape == (3, 5) and t.is_contiguous() and t.data_ptr() % 512 == 0
        assert (t.view(wt) == val).all()
        n = ctx.guard // t.element_size()
        wide = beyond(t, n, n).view(wt)
        assert wide.numel() == 15 + 2 * n and (wide == val).all()          # a whole guard of the fill on either side
        assert ctx.guard % 512 == 0 and ctx.guard == GA.GUARD_BYTES >= 288 * 1024
        ctx.check_guards()
    if dtype == torch.float32:
        assert torch.isnan(t).all() if fill == 'A' else (t == 1e30).all()
    if dtype == torch.int16:
        h = t.view(torch.float16)
        assert torch.isnan(h).all() and torch.isnan(t.view(torch.bfloat16)).all() if fill == 'A' else \
            (torch.isfinite(h).all() and (h > 5e4).all() and torch.isfinite(t.view(torch.bfloat16)).all() and (t.view(torch.bfloat16) > 1e30).all())
    if dtype in (torch.int32, torch.int64):
        assert (t < -10 ** 9).all() if fill == 'A' else (t > 10 ** 9).all()
    if dtype in (torch.uint8, torch.int8):
        assert (t.view(torch.uint8) == (0xA5 if fill == 'A' else 0x5A)).all()


def test_the_dtype_list_is_what_hipops_allocates():
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'latent_pose_reenactment_amd', 'hipops.py')).read()
    used = set()
    for line in src.splitlines():
        if 'torch.empty(' in line:
            used.update(re.findall(r'dtype=torch\.(\w+)', line))
    assert used == {str(d).split('.')[-1] for d in DTYPES}, used


def test_strides_are_those_of_the_real_call():
    base = torch.zeros(2, 6, 5, 8)
    with Guarded('A') as ctx:
        real_cl = GA._REAL_EMPTY((2, 8, 6, 5), memory_format=torch.channels_last)
        cl = torch.empty((2, 8, 6, 5), memory_format=torch.channels_last)
        assert cl.stride() == real_cl.stride() and cl.is_contiguous(memory_format=torch.channels_last) and torch.isnan(cl).all()
        nchw_view = base.permute(0, 3, 1, 2)                           # dense, not contiguous: empty_like keeps the permutation
        like = torch.empty_like(nchw_view)
        assert like.stride() == GA._REAL_EMPTY_LIKE(nchw_view).stride() == nchw_view.stride() and like.shape == nchw_view.shape
        sliced = base[:, ::2, :, 1:5]                                   # not dense: empty_like gives a contiguous tensor
        like2 = torch.empty_like(sliced)
        assert like2.stride() == GA._REAL_EMPTY_LIKE(sliced).stride() and like2.is_contiguous()
        forced = torch.empty_like(nchw_view, memory_format=torch.contiguous_format)
        assert forced.is_contiguous()
        ints = torch.empty_like(nchw_view, dtype=torch.int32)
        assert ints.dtype == torch.int32 and ints.stride() == nchw_view.stride() and (ints < 0).all()
        for t in (cl, like, like2, forced, ints, torch.empty(7), torch.empty(3, 4, dtype=torch.int64), torch.empty(0), torch.empty((2, 0, 3))):
            assert t.data_ptr() % 512 == 0 and ctx.served(t) is not None or t.numel() == 0
        assert len(ctx.records) == 9
        ctx.check_guards()


def test_guarded_inputs_keep_their_strides_and_end_at_the_fence():
    base = torch.arange(2 * 6 * 5 * 8, dtype=torch.float32).reshape(2, 6, 5, 8)
    view = base[:, 1:5, :, 2:5]                                         # a strided view: its last element is NOT the last one of ``base``
    mask = torch.ones(1, 1, 5).expand(2, 6, 5)
    with Guarded('B') as ctx:
        assert GA.active() is ctx
        v = GA.guarded(view)
        assert torch.equal(v, view) and v.stride() == view.stride() and v.data_ptr() % 512 == 0
        rec = ctx.served(v)
        extent = 1 + sum((n - 1) * s for n, s in zip(view.shape, view.stride()))
        assert rec.nbytes == 4 * extent < 4 * base.numel()             # the allocation ends with the view's last element
        end = v.as_strided((2,), (1,), v.storage_offset() + extent - 1)
        assert end[0] == view[-1, -1, -1, -1] and end[1] == 1e30       # ... and the next word is the fill
        assert v.as_strided((1,), (1,), v.storage_offset() + 3)[0] == 1e30          # so is a hole of the view
        m = GA.guarded(mask)
        assert m.stride() == mask.stride() and torch.equal(m, mask) and ctx.served(m).nbytes == 4 * 5
        ctx.check_guards()
    assert GA.guarded(view) is view and GA.active() is None


def test_zeros_and_full_stay_untouched():
    with Guarded('A') as ctx:
        z, f, o = torch.zeros(1000), torch.full((5,), 2.5), torch.ones(3, dtype=torch.int32)
        assert not z.any() and (f == 2.5).all() and (o == 1).all() and torch.zeros_like(f).sum() == 0
        assert len(ctx.records) == 0
        assert torch.empty(4, device='meta').device.type == 'meta' and len(ctx.records) == 0


def test_the_real_calls_are_back_after_the_context_and_after_an_exception():
    real, real_like = torch.empty, torch.empty_like
    with Guarded('A'):
        assert torch.empty is not real and torch.empty_like is not real_like
        with Guarded('B') as inner:
            assert (torch.empty(3) == 1e30).all() and GA.active() is inner
        assert torch.isnan(torch.empty(3)).all()
    assert torch.empty is real and torch.empty_like is real_like
    with pytest.raises(RuntimeError):
        with Guarded('B'):
            raise RuntimeError('a failing test body')
    assert torch.empty is real and torch.empty_like is real_like and GA.active() is None


fenced_buffers = GA.fence_fixture(autouse=False)


def test_the_fixture_provides_fill_a_and_checks_at_teardown(fenced_buffers):
    assert torch.isnan(torch.empty(5)).all() and (torch.empty(5, dtype=torch.int16) == 0x7fff).all()
    assert GA.active() is fenced_buffers and len(fenced_buffers.records) == 2


def test_the_fixtures_teardown_raises_on_a_damaged_guard():
    real = torch.empty
    gen = GA.fenced('A')
    next(gen)
    store_past_end(*inputs())
    with pytest.raises(GuardError, match='past the end'):
        next(gen)
    assert torch.empty is real and GA.active() is None
