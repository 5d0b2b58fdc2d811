"""Mode-aware layer over tests/emu_ops.py.  TEST INFRASTRUCTURE ONLY, opt-in: tests/emu_ops.py itself (the per-op GPU reference of
tests/test_resnext_hip.py and tests/test_resident16_gpu.py) is not touched and keeps ignoring every ``prec`` argument.

On the GPU ``hipops.Act16`` and ``hipops.WeightPack`` carry no operand mode: a plane written as bf16 hi + lo and handed to an fp16
contraction is silently read as fp16 bits.  This module has the entry points of ``emu_ops`` (``resnext_hip.ops`` is monkeypatched with it)
and
  * records the mode every operand plane and weight pack was PRODUCED in -- a side table keyed by the plane's storage (so the record
    survives ``view`` / ``reshape`` / ``flat16`` and the positional rebuild of ``resnext_hip._v16``), which keeps the tensor alive so that
    no pointer is reused -- and raises ``ModeError`` naming the consumer when a consumer's ``prec`` differs from it, when a 16-bit-resident
    conv output (y16) is not fp16, or when the planes residual of ``bn_add_act`` is anything but bf16x3 planes of the output's mode;
  * optionally (``rounding()``) ROUNDS what the kernels round, in the arithmetic of the tensors it is given (fp64 in the study): the
    operands of every contraction according to the ``prec`` that call receives (bf16: one bf16; bf16x3: hi + lo bf16; f16: fp16, gradient
    operands scaled by the power of two that puts their amax into [2^12, 2^13)), 16-bit-resident conv outputs to fp16, the planes
    residual to its planes' mode, and every fp32-resident result to fp32.  That is the error an assignment of modes itself implies on a
    network and input, independent of any kernel: tests/rounding_study.py derives the gates of tests/test_resnext_hip.py from it.
``reset()`` empties the tables (call it once per network pass: the tables hold every plane of the pass)."""
import contextlib
import math

import torch

import emu_ops as E
from emu_ops import Act16, ConvStats, Pack          # noqa: F401  (part of the emulated interface)

BF16, BF16X3, F16 = 0, 1, 2
NAMES = {BF16: 'bf16', BF16X3: 'bf16x3', F16: 'f16', None: 'untagged'}


class ModeError(AssertionError):
    pass


_planes = {}          # storage pointer -> (tensor (kept alive), mode, holds scaled fp16 gradient values already)
_packs = {}           # id(pack.w) -> (pack.w (kept alive), mode)
_round = [False]
checks = [0]          # consumer-side checks made since reset(): a test can tell that the layer was in the path


def reset():
    _planes.clear()
    _packs.clear()
    checks[0] = 0


@contextlib.contextmanager
def rounding(on=True):
    old = _round[0]
    _round[0] = on
    try:
        yield
    finally:
        _round[0] = old


def __getattr__(name):          # everything that neither produces nor consumes operand planes: the emulation itself (results stored as fp32)
    fn = getattr(E, name)
    if not callable(fn) or isinstance(fn, type):
        return fn
    return lambda *a, **kw: _f32(fn(*a, **kw))


# ---- the side tables
def tag(a, mode, scaled=False):
    """record that the planes ``a`` (Act16 | tensor) were written in ``mode``"""
    t = a.hi if isinstance(a, Act16) else a
    _planes[t.untyped_storage().data_ptr()] = (t, mode, scaled)
    return a


def _entry(a):
    return _planes.get(a.hi.untyped_storage().data_ptr(), (None, None, False))


def mode_of(a):
    return _entry(a)[1]


def tag_pack(pack, mode):
    _packs[id(pack.w)] = (pack.w, mode)
    return pack


def pack_mode_of(pack):
    return _packs.get(id(pack.w), (None, None))[1]


def _expect(consumer, what, have, want):
    checks[0] += 1
    if have != want:
        raise ModeError(f'{consumer}: {what} was written as {NAMES[have]} and is consumed as {NAMES[want]}')


# ---- rounding
def rnd(t, mode):
    if mode == F16:
        return t.to(torch.float16).to(t.dtype)
    hi = t.to(torch.bfloat16).to(t.dtype)
    if mode == BF16:
        return hi
    return hi + (t - hi).to(torch.bfloat16).to(t.dtype)


def _rnd_grad_f16(t):
    """fp16 gradient operand: scaled by the power of two that puts the amax into [2^12, 2^13), rounded, scaled back"""
    m = float(t.abs().max())
    if not (m > 0 and math.isfinite(m)):
        return t
    s = 2.0 ** (13 - math.frexp(m)[1])
    return (t * s).to(torch.float16).to(t.dtype) / s


def _f32(r):
    """results that live in fp32 on the GPU"""
    if not _round[0]:
        return r
    if isinstance(r, torch.Tensor):
        return r.float().to(r.dtype) if r.dtype == torch.float64 else r
    if isinstance(r, ConvStats):
        return ConvStats(_f32(r.part), r.rows)
    if isinstance(r, tuple) and not isinstance(r, Act16):
        return tuple(_f32(t) for t in r)
    return r


def _operand(a, prec):
    """the values a contraction in mode ``prec`` multiplies"""
    if not _round[0] or _entry(a)[2]:
        return a
    return Act16(rnd(a.hi, prec), None, a.c, a.inv)


def _weights(pack, prec):
    return Pack(rnd(pack.w, prec), pack.mode) if _round[0] else pack


def _grad_planes(a, prec):
    """planes a producer of gradient operands writes: fp16 ones carry their power-of-two scale"""
    if _round[0] and prec == F16:
        return tag(Act16(_rnd_grad_f16(a.hi), None, a.c, a.inv), prec, scaled=True)
    return tag(a, prec)


def _conv_out(r, prec):
    """(y | None[, out16 planes][, stats]): the 16-bit planes of y are tagged (and rounded) in the conv's mode"""
    if not isinstance(r, tuple):
        return _f32(r)
    out = []
    for t in r:
        if isinstance(t, Act16):
            out.append(tag(Act16(rnd(t.hi, prec), None, t.c, t.inv) if _round[0] else t, prec))
        else:
            out.append(_f32(t))
    return tuple(out)


# ---- producers
class PackBatch(E.PackBatch):
    def update(self):
        return [tag_pack(p, self.prec) for p in super().update()]


def pack_grouped(w, mode, prec):
    return tag_pack(E.pack_grouped(w, mode, prec), prec)


def pack_weights(w, mode, prec, small_k=False):
    return tag_pack(Pack(w, mode), prec)


def act_pack(x, *, pro=0, scale=None, shift=None, prec=0, grad=False):
    a = E.act_pack(x, pro=pro, scale=scale, shift=shift, prec=prec, grad=grad)
    if a.hi.untyped_storage().data_ptr() == x.untyped_storage().data_ptr():          # (pro 0: the emulated plane is x itself; planes are a tensor of their own)
        a = Act16(a.hi.clone(), None, a.c, a.inv)
    return _grad_planes(a, prec) if grad else tag(a, prec)


def im2col_planes(x, ksize, stride, pad, prec):
    return tag(E.im2col_planes(x, ksize, stride, pad, prec), prec)


def bn_relu_maxpool(y, scale, shift, prec, want_idx=True):
    out, out16, idx = E.bn_relu_maxpool(y, scale, shift, prec, want_idx)
    tag(out16, prec)
    return _f32(out), out16, idx


def subsample2_16(a):
    _, mode, scaled = _entry(a)
    return tag(E.subsample2_16(a), mode, scaled)


def zero_stuff2_16(a, h, w):
    _, mode, scaled = _entry(a)
    return tag(E.zero_stuff2_16(a, h, w), mode, scaled)


# ---- consumers (and what they produce)
def conv16(a, pack, *, prec=0, kind=None, **kw):
    who = f'conv16 ({kind or "1x1"}, {"forward" if pack.mode == 0 else "data-gradient"} pack)'
    _expect(who, 'the activation plane', mode_of(a), prec)
    _expect(who, 'the weight pack', pack_mode_of(pack), prec)
    return _conv_out(E.conv16(_operand(a, prec), _weights(pack, prec), prec=prec, kind=kind, **kw), prec)


def gconv16(a, pack, *, prec=0, **kw):
    who = f'gconv16 ({"forward" if pack.mode == 0 else "data-gradient"} pack)'
    _expect(who, 'the activation plane', mode_of(a), prec)
    _expect(who, 'the weight pack', pack_mode_of(pack), prec)
    return _conv_out(E.gconv16(_operand(a, prec), _weights(pack, prec), prec=prec, **kw), prec)


def conv_wgrad16(a, dy, *, prec=0, kind=None, **kw):
    who = f'conv_wgrad16 ({kind or "1x1"})'
    _expect(who, 'the activation plane', mode_of(a), prec)
    _expect(who, 'the gradient plane', mode_of(dy), prec)
    return _f32(E.conv_wgrad16(_operand(a, prec), _operand(dy, prec), prec=prec, kind=kind, **kw))


def gconv_wgrad16(a, dy, group_size, *, prec=0, **kw):
    _expect('gconv_wgrad16', 'the activation plane', mode_of(a), prec)
    _expect('gconv_wgrad16', 'the gradient plane', mode_of(dy), prec)
    return _f32(E.gconv_wgrad16(_operand(a, prec), _operand(dy, prec), group_size, prec=prec, **kw))


def bn_act16(y16, scale, shift, relu=True):
    _expect('bn_act16', 'the 16-bit-resident conv output', mode_of(y16), F16)
    return tag(E.bn_act16(y16, scale, shift, relu), F16)


def bn_add_act(y, scale, shift, res=None, res_scale=None, res_shift=None, relu=True, prec=None, want_out=True):
    if isinstance(y, Act16):          # lp_bn_add_act16 reads an fp16 plane and writes fp16 planes
        _expect('bn_add_act (y16 form)', 'the 16-bit-resident conv output', mode_of(y), F16)
        if prec not in (None, F16):
            raise ModeError(f'bn_add_act (y16 form): asked for {NAMES[prec]} output planes (lp_bn_add_act16 writes fp16 planes only)')
    if isinstance(res, Act16):        # lp_bn_add_act_planes: hi + lo planes of the output's own mode, the only planes that are a residual stream
        _expect('bn_add_act (planes residual)', 'the residual plane', mode_of(res), prec)
        if prec != BF16X3:
            checks[0] += 1
            raise ModeError(f'bn_add_act (planes residual): a {NAMES[prec]} block takes the planes-residual route (bf16x3 only: '
                            f'{NAMES[prec]} planes re-round the residual stream of every identity block)')
        res = _operand(res, prec)
    r = E.bn_add_act(y, scale, shift, res, res_scale, res_shift, relu, prec, want_out)
    if prec is None:
        return _f32(r)
    out, out16 = r
    tag(out16, prec)
    return _f32(out), out16


def bn_bwd16(dA, x, gamma, mean, rstd, scale, shift, *, prec=0, **kw):
    if isinstance(x, Act16):
        _expect('bn_bwd16 (y16 form)', 'the 16-bit-resident conv output', mode_of(x), F16)
        if prec != F16:
            raise ModeError(f'bn_bwd16 (y16 form): asked for {NAMES[prec]} gradient planes (a 16-bit-resident conv output is read in the fp16 mode only)')
    d16, dg, db, g = E.bn_bwd16(dA, x, gamma, mean, rstd, scale, shift, prec=prec, **kw)
    return _grad_planes(d16, prec), _f32(dg), _f32(db), _f32(g)
