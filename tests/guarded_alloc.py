"""Poisoned, fenced buffers for the kernel wrappers: what a kernel may not depend on, and where it may not store.

Every wrapper of ``hipops`` takes its outputs and workspaces from ``torch.empty`` / ``torch.empty_like`` and hands the raw pointer to the C ABI.  Inside
``Guarded(fill)`` those two calls are served from a flat allocation of ``guard + payload + guard`` bytes: both guards AND the payload hold ``fill``, the
tensor handed back is the payload (requested shape, dtype and strides, 512-byte aligned like the caching allocator's blocks), every allocation is
recorded.  ``torch.zeros`` / ``torch.full`` and everything else are untouched.  ``guarded(t)`` puts an input the test built into such an allocation, so
that the element before its first and behind its last one is poison too; ``check_guards()`` compares every guard word with the fill, on the device.

``differential(fn, inputs)`` is the reference-free test built from this: ``fn`` runs plain, under fill ``A`` (NaN-like) and under fill ``B`` (large,
finite, positive), and every tensor reachable from its result must be BIT-identical in all three runs, the guards intact in both fenced runs.

What this proves: no returned word depends on what fresh memory held (an output element, pad word or workspace slot read before it was written; an
input read before its start or past its end that reaches a result), and no store lands within ``GUARD_BYTES`` of a buffer's ends.  Two fills because
one value can hide: relu() swallows a NaN-like negative or NaN, ``x > 0 ? g : 0`` is false for NaN AND for the zero the plain run usually finds.
What it cannot prove: a stray READ that never reaches a result is invisible, and so is a store that jumps further than the guard.

``GUARD_BYTES`` must cover the largest block of memory a single workgroup stores.  That is set by conv_wgrad_kernel<.., COB = 128> (csrc/conv_wgrad.hip):
one workgroup stores the split-K partial slab of 128 output x 64 input channels x 9 taps in fp32 = 288 KiB (the widest conv output tile, conv_dma_kernel
<WM 4, WN 2, MR 4, NR 4>: 256 pixels x 128 channels fp32 = 128 KiB, lies below it; the 256 x 64 tile is 64 KiB).  Rounded up to 512 KiB.

A new wrapper goes behind the fence by one entry in tests/test_buffer_discipline_gpu.py: a function that builds CPU inputs from a seeded generator and
returns ``(fn, inputs)``; a buffer the wrapper does not take from ``torch.empty`` (a cache, a module's buffer) is passed in as an input.  A whole test
module goes behind fill ``A`` with ``fenced_buffers = fence_fixture()`` at module level."""
import os
import sys

import pytest
import torch

GUARD_BYTES = 512 * 1024
ALIGN = 512
assert GUARD_BYTES % ALIGN == 0

_WORD = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


class Fill:
    """one word pattern per dtype, written through the integer type of the same width"""

    def __init__(self, name, f32, f64, w16, w8, i32, i64):
        self.name = name
        self._by = {torch.float32: _signed(f32, 32), torch.float64: _signed(f64, 64), torch.int16: _signed(w16, 16), torch.float16: _signed(w16, 16),
                    torch.bfloat16: _signed(w16, 16), torch.uint8: w8, torch.int8: w8, torch.bool: w8, torch.int32: _signed(i32, 32),
                    torch.int64: _signed(i64, 64)}
        self._w8 = w8

    def word(self, dtype):
        """(integer dtype of the element's width, the value to fill_ it with)"""
        if dtype in self._by:
            return _WORD[_itemsize(dtype)], self._by[dtype]
        size = _REAL_EMPTY((), dtype=dtype).element_size()
        v = int.from_bytes(bytes([self._w8]) * size, 'little')          # any other dtype: the byte pattern
        return _WORD[size], _signed(v, 8 * size) if size > 1 else v

    def __repr__(self):
        return f'Fill({self.name})'


def _itemsize(dtype):
    return {torch.float32: 4, torch.float64: 8, torch.int16: 2, torch.float16: 2, torch.bfloat16: 2, torch.uint8: 1, torch.int8: 1, torch.bool: 1,
            torch.int32: 4, torch.int64: 8}[dtype]


# A: NaN-like.  fp32 a quiet NaN with the payload 0xBEEF, 16-bit 0x7fff (a NaN in bf16 and in fp16), bytes 0xA5, integers large and negative.
FILL_A = Fill('A', 0x7FC0BEEF, 0x7FF8BEEFBEEFBEEF, 0x7FFF, 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5)
# B: large, finite, positive.  fp32 1e30 (0x7149F2CA), 16-bit 0x7b00 (57344 in fp16, 2^119 in bf16), bytes 0x5A, integers large and positive.
FILL_B = Fill('B', 0x7149F2CA, 0x46293E5939A08CEA, 0x7B00, 0x5A, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A)
FILLS = {'A': FILL_A, 'B': FILL_B}

_REAL_EMPTY, _REAL_EMPTY_LIKE = torch.empty, torch.empty_like
_ACTIVE = []          # stack of active Guarded contexts
_HERE = os.path.abspath(__file__)


class GuardError(AssertionError):
    pass


class _Record:
    __slots__ = ('raw', 'start', 'nbytes', 'shape', 'dtype', 'where', 'kind')

    def describe(self):
        return f'{self.kind} {tuple(self.shape)} {self.dtype} allocated at {self.where}'


def _extent(shape, strides):
    """elements from the first to behind the last one a (shape, strides) view addresses"""
    if any(s == 0 for s in shape):
        return 0
    return 1 + sum((n - 1) * st for n, st in zip(shape, strides))


def _copy_into(g, t):
    """the values of ``t`` into the view ``g`` of the same shape and strides"""
    src, dst = t.detach(), g
    for d, (n, st) in enumerate(zip(t.shape, t.stride())):
        if st == 0 and n > 1:          # an expanded dimension: one copy of it exists
            src, dst = src.narrow(d, 0, 1), dst.narrow(d, 0, 1)
    if t.numel():
        dst.copy_(src)
    return g


def _caller():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _HERE:
        f = f.f_back
    return 'unknown' if f is None else f'{os.path.basename(f.f_code.co_filename)}:{f.f_lineno} ({f.f_code.co_name})'


class Guarded:
    """context manager: ``torch.empty`` / ``torch.empty_like`` hand out poisoned, fenced tensors while it is active"""

    def __init__(self, fill=FILL_A, guard_bytes=GUARD_BYTES):
        self.fill = FILLS[fill] if isinstance(fill, str) else fill
        assert guard_bytes % ALIGN == 0 and guard_bytes > 0
        self.guard = guard_bytes
        self.records = []

    # ---- the allocation itself --------------------------------------------------------------------------------------------------------------
    def alloc(self, shape, strides, dtype, device, kind, where=None):
        shape, strides = tuple(int(s) for s in shape), tuple(int(s) for s in strides)
        item = _itemsize(dtype) if dtype in FILL_A._by else _REAL_EMPTY((), dtype=dtype).element_size()
        nbytes = _extent(shape, strides) * item
        raw = _REAL_EMPTY(2 * self.guard + nbytes + ALIGN, dtype=torch.uint8, device=device)
        start = (-raw.data_ptr()) % ALIGN + self.guard          # byte offset of the payload: 512-aligned, a whole guard in front of it
        wt, val = self.fill.word(dtype)
        lo = start - self.guard
        raw[lo:lo + 2 * self.guard + nbytes].view(wt).fill_(val)
        rec = _Record()
        rec.raw, rec.start, rec.nbytes, rec.shape, rec.dtype, rec.kind = raw, start, nbytes, shape, dtype, kind
        rec.where = where or _caller()
        self.records.append(rec)
        if nbytes == 0:
            return raw[start:start].view(dtype).as_strided(shape, strides)
        return raw[start:start + nbytes].view(dtype).as_strided(shape, strides)

    def _serve(self, real, kind, args, kwargs):
        if kwargs.get('out') is not None or kwargs.get('pin_memory') or kwargs.get('layout', torch.strided) is not torch.strided:
            return real(*args, **kwargs)
        model = real(*args, **kwargs)          # the shape, dtype, strides and device the real call gives
        if model.device.type == 'meta' or model.is_quantized or model.is_complex():
            return model
        t = self.alloc(model.shape, model.stride(), model.dtype, model.device, kind)
        if kwargs.get('requires_grad'):
            t.requires_grad_(True)
        return t

    def empty(self, *args, **kwargs):
        return self._serve(_REAL_EMPTY, 'torch.empty', args, kwargs)

    def empty_like(self, *args, **kwargs):
        return self._serve(_REAL_EMPTY_LIKE, 'torch.empty_like', args, kwargs)

    def guarded(self, t):
        """a copy of ``t`` (same shape, dtype, strides) whose first element follows a guard and whose last element is followed by one; the holes of a
        strided view hold the fill"""
        return _copy_into(self.alloc(t.shape, t.stride(), t.dtype, t.device, 'guarded input', _caller()), t)

    # ---- the check ----------------------------------------------------------------------------------------------------------------------------
    def _sides(self, rec):
        wt, val = self.fill.word(rec.dtype)
        lo = rec.raw[rec.start - self.guard:rec.start].view(wt)
        hi = rec.raw[rec.start + rec.nbytes:rec.start + rec.nbytes + self.guard].view(wt)
        return (('before the start', lo, -self.guard), ('past the end', hi, rec.nbytes)), val

    def check_guards(self):
        """every guard word of every recorded allocation still holds the fill; else GuardError naming the allocation, the side and the first and last
        damaged byte (offsets from the buffer's first byte: negative in front of it)"""
        by_dev = {}
        for rec in self.records:
            sides, val = self._sides(rec)
            for _, words, _ in sides:
                by_dev.setdefault(rec.raw.device, []).append((words != val).any())
        if not any(bool(torch.stack(flags).any()) for flags in by_dev.values()):
            return
        msgs = []
        for rec in self.records:
            sides, val = self._sides(rec)
            for side, words, base in sides:
                bad = torch.nonzero((words.view(torch.uint8).reshape(-1, words.element_size()) !=
                                     words.new_full((1,), val).view(torch.uint8)).reshape(-1)).reshape(-1)
                if bad.numel():
                    msgs.append(f'{rec.describe()}: {bad.numel()} bytes damaged {side}, byte offsets {base + int(bad[0])} .. {base + int(bad[-1])} '
                                f'(the buffer is bytes 0 .. {rec.nbytes - 1})')
        raise GuardError('guard words overwritten (fill %s):\n  ' % self.fill.name + '\n  '.join(msgs))

    def served(self, t):
        """the record whose payload holds ``t``'s first byte, or None"""
        if t.numel() == 0:
            return None
        p = t.data_ptr()
        for rec in self.records:
            base = rec.raw.data_ptr() + rec.start
            if rec.raw.device == t.device and base <= p < base + max(rec.nbytes, 1):
                return rec
        return None

    # ---- context --------------------------------------------------------------------------------------------------------------------------------
    def __enter__(self):
        self._prev = (torch.empty, torch.empty_like)
        torch.empty, torch.empty_like = self.empty, self.empty_like
        _ACTIVE.append(self)
        return self

    def __exit__(self, *exc):
        assert _ACTIVE and _ACTIVE[-1] is self
        _ACTIVE.pop()
        torch.empty, torch.empty_like = self._prev
        self.records = []
        return False


def active():
    return _ACTIVE[-1] if _ACTIVE else None


def guarded(t):
    """``t`` inside a fenced allocation of the active context (no context: ``t`` itself)"""
    g = active()
    return t if g is None else g.guarded(t)


def check_guards():
    g = active()
    assert g is not None, 'check_guards() outside a Guarded context'
    g.check_guards()


def fenced(fill='A'):
    """the body of the fixture: a ``Guarded(fill)`` context around the test, the guards checked when it is over"""
    with Guarded(fill) as g:
        yield g
        if any(r.raw.is_cuda for r in g.records):
            torch.cuda.synchronize()
        g.check_guards()


def fence_fixture(fill='A', autouse=True):
    """pytest fixture factory: ``fenced_buffers = fence_fixture()`` at module level puts every test of the module under ``fill`` and checks the guards
    at teardown"""
    @pytest.fixture(autouse=autouse)
    def fenced_buffers():
        yield from fenced(fill)
    return fenced_buffers


# ---- the differential ------------------------------------------------------------------------------------------------------------------------------
def _map_tensors(obj, f):
    """``obj`` with every tensor replaced by f(tensor): through tuples (named ones too), lists and dicts"""
    if isinstance(obj, torch.Tensor):
        return f(obj)
    if isinstance(obj, tuple) and hasattr(obj, '_fields'):
        return type(obj)(*(_map_tensors(v, f) for v in obj))
    if isinstance(obj, (tuple, list)):
        return type(obj)(_map_tensors(v, f) for v in obj)
    if isinstance(obj, dict):
        return {k: _map_tensors(v, f) for k, v in obj.items()}
    return obj


def _place(t, device, ctx):
    """``t`` with its own strides on ``device``: fenced under a context, else in a zeroed allocation of exactly its extent"""
    dev = torch.device(device) if device is not None else t.device
    if ctx is not None:
        g = ctx.alloc(t.shape, t.stride(), t.dtype, dev, 'guarded input', _caller())
    else:
        slack = ALIGN // t.element_size()          # what follows a tensor in an allocator block: readable, and usually zero
        flat = torch.zeros(_extent(t.shape, t.stride()) + 2 * slack, dtype=t.dtype, device=dev)
        g = flat.as_strided(tuple(t.shape), tuple(t.stride()), slack)
    return _copy_into(g, t)


def reachable(obj, path='result', out=None):
    """[(path, tensor | plain value)] of everything reachable from a wrapper's return value: tuples, lists, dicts, named tuples (hipops.Act16,
    WeightPack, ConvStats, Tap16: by field name) and the attributes of any other object that carries ``hi`` / ``lo`` planes or packs"""
    out = [] if out is None else out
    if isinstance(obj, torch.Tensor) or obj is None or isinstance(obj, (bool, int, float, str, bytes)):
        out.append((path, obj))
    elif isinstance(obj, tuple) and hasattr(obj, '_fields'):
        for k, v in zip(obj._fields, obj):
            reachable(v, f'{path}.{k}', out)
    elif isinstance(obj, (tuple, list)):
        for i, v in enumerate(obj):
            reachable(v, f'{path}[{i}]', out)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            reachable(v, f'{path}.{k}', out)
    elif hasattr(obj, '__dict__'):
        for k, v in sorted(vars(obj).items()):
            if v is None or isinstance(v, (torch.Tensor, tuple, list, dict)) or hasattr(v, 'hi'):
                reachable(v, f'{path}.{k}', out)
    else:
        out.append((path, obj))
    return out


def _words(t):
    """the logical elements of ``t`` as integer words on the host (a NaN equals the same NaN)"""
    t = t.detach()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = t.contiguous().cpu()
    return t.view(_WORD[t.element_size()])


def _snapshot(result):
    return [(p, _words(v) if isinstance(v, torch.Tensor) else v) for p, v in reachable(result)]


def _named(path, names):
    last = path.rsplit('.', 1)[-1]
    return path in names or last in names or last.split('[')[0] in names


def compare_runs(runs, unwritten=()):
    """``runs`` = [(label, snapshot)]: every path present in all, every tensor bit-identical; paths named in ``unwritten`` are only required to exist"""
    (l0, s0), rest = runs[0], runs[1:]
    for label, snap in rest:
        assert [p for p, _ in snap] == [p for p, _ in s0], f'runs {l0} and {label} return different structures'
        for (path, a), (_, b) in zip(s0, snap):
            if _named(path, unwritten):
                continue
            if isinstance(a, torch.Tensor) != isinstance(b, torch.Tensor):
                raise AssertionError(f'{path}: a tensor in one of the runs {l0} / {label} only')
            if not isinstance(a, torch.Tensor):
                assert a == b, f'{path}: {a!r} in run {l0}, {b!r} in run {label}'
                continue
            assert a.shape == b.shape and a.dtype == b.dtype, f'{path}: {tuple(a.shape)} {a.dtype} in run {l0}, {tuple(b.shape)} {b.dtype} in run {label}'
            if not torch.equal(a, b):
                ne = torch.nonzero((a != b).reshape(-1)).reshape(-1)
                i = int(ne[0])
                fmt = f'0x%0{2 * a.element_size()}x'
                mask = (1 << 8 * a.element_size()) - 1
                raise AssertionError(f'{path} {tuple(a.shape)}: {ne.numel()} of {a.numel()} words depend on what fresh memory held; first at flat index {i} '
                                     f'(last {int(ne[-1])}): ' + fmt % (int(a.reshape(-1)[i]) & mask) + f' in run {l0}, ' +
                                     fmt % (int(b.reshape(-1)[i]) & mask) + f' in run {label}')


def differential(fn, inputs, *, device=None, unwritten=(), fills=('A', 'B')):
    """fn(*inputs) plain, then under each fill with fenced inputs: guards intact, every reachable tensor of the result bit-identical in all runs ->
    the plain result.  ``inputs``: a tuple / list (or a dict: keyword arguments) whose tensors -- nested ones too -- are copied afresh for every run
    (onto ``device``, keeping their strides), so ``fn`` may update them in place and return them.  ``unwritten``: names (field, key or full path) of
    returned tensors the kernel's header says it does not write; they are left out of the comparison, nothing else is."""
    def run(ctx):
        placed = _map_tensors(inputs, lambda t: _place(t, device, ctx))
        res = fn(**placed) if isinstance(placed, dict) else fn(*placed)
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        return res

    plain = run(None)
    runs = [('plain', _snapshot(plain))]
    for name in fills:
        with Guarded(name) as g:
            res = run(g)
            g.check_guards()
            runs.append((f'fill {name}', _snapshot(res)))
            del res
    compare_runs(runs, unwritten)
    return plain
