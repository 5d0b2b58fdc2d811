"""Tensor-level wrappers around the C ABI.  Activations are NHWC fp32 contiguous CUDA tensors of shape [N,H,W,C]; the operands of
the conv kernels are 16-bit planes (``Act16`` from ``act_pack`` / a conv epilogue, ``WeightPack``).
PyTorch here is plumbing only: it owns the buffers and the stream; all arithmetic happens in liblp_hip.so."""
import os
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib
from ._lib import PREC_BF16, PREC_BF16X3, PREC_F16, check
from .dataloaders.synthetic_voxceleb2_stickmen import PARTS      # the one place that knows the face topology (stickman_render's default table)
from .dataloaders.synthetic_voxceleb2_stickmen import REFERENCE_PARTS, REFERENCE_PARTS_NO_OVAL      # (stickman_render_hard's)

Tensor = torch.Tensor


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional live profiling hook used by bench.py: when PROFILE is a list, every conv / wgrad launch is bracketed by
# HIP events recorded on the launch stream and appended as (kind, flops, start_event, end_event).
PROFILE = None


class _Timed:
    def __init__(self, kind, flops, tag=None, nbytes=0.0, mm=1):
        """``nbytes``: algorithmic HBM bytes of the launch -- a total, or (read, write); ``mm``: MFMAs per algorithmic MAC (bf16x3: 3)"""
        self.mm = mm
        self.rw = tuple(nbytes) if isinstance(nbytes, tuple) else None
        self.kind, self.flops, self.tag, self.nbytes = kind, flops, tag, (sum(nbytes) if isinstance(nbytes, tuple) else nbytes)

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.kind, self.flops, self.e0, self.e1, self.tag, self.nbytes, self.rw, self.mm))


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _chk(t: Tensor, name: str):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f'{name}: expected a contiguous fp32 CUDA tensor, got {t.dtype} {t.device} contiguous={t.is_contiguous()}')


def _round_up(v, m):
    return (v + m - 1) // m * m


def _f16(prec: int) -> int:
    return int(prec == PREC_F16)


class WeightPack(NamedTuple):
    hi: Tensor
    lo: Optional[Tensor]
    rows: int      # logical rows (Cout for mode 0, Cin for mode 1)
    cols: int
    rows_p: int
    cols_p: int
    taps: int


def _pack_geometry(w: Tensor, mode: int, small_k: bool):
    """(cout, cin, taps in, taps out, rows, cols, rows_p, cols_p) of a pack: modes 0 / 2 are [taps][Cout][Cin] images, 1 / 3 [taps][Cin][Cout];
    2 / 3 = the phase forms of a x2-upsampled 3x3 conv, 4 / 5 = forward / data gradient of a 3x3 conv followed by AvgPool2d(2) (16 taps:
    lp_pack_weights)"""
    cout, cin = w.shape[0], w.shape[1]
    taps = w.numel() // (cout * cin)
    assert mode in (0, 1) or taps == 9, 'the phase forms (modes 2 / 3) pack a 3x3 weight'
    rows, cols = (cout, cin) if mode in (0, 2, 4) else (cin, cout)
    rows_p = _round_up(rows, 128)
    cols_p = _round_up(cols, 32 if (small_k and cols <= 32) else 64)
    return cout, cin, taps, (16 if mode >= 2 else taps), rows, cols, rows_p, cols_p


def pack_weights(w: Tensor, mode: int, prec: int, small_k: bool = False) -> WeightPack:
    """w: [Cout, Cin, k, k] (or [Cout, Cin]) fp32.  mode 0 = forward pack, mode 1 = dgrad pack (flipped + transposed); 2 / 3 = the phase forms
    (forward / data gradient) of a x2-upsampled 3x3 conv; 4 / 5 = the same pair for a 3x3 conv followed by AvgPool2d(2) (include/lp_hip.h).  small_k pads the contraction dim to 32 instead of 64 (only valid for 3x3
    non-upsampled convs)."""
    _chk(w, 'w')
    cout, cin, taps, taps_out, rows, cols, rows_p, cols_p = _pack_geometry(w, mode, small_k)
    hi = torch.empty((taps_out, rows_p, cols_p), dtype=torch.int16, device=w.device)
    lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
    check(_lib.lib().lp_pack_weights(w.data_ptr(), hi.data_ptr(), _p(lo), cout, cin, taps, rows_p, cols_p, mode, _f16(prec), _stream()),
          'lp_pack_weights')
    return WeightPack(hi, lo, rows, cols, rows_p, cols_p, taps_out)


def phase_weights(w: Tensor) -> Tensor:
    """w [Cout, Cin, 3, 3] -> [Cout, Cin, 4, 2, 2]: the phase form of conv3x3(nearest_up2(x)).  Output pixel (2y + a, 2x + b) reads the upsampled rows
    2y + a + dy - 1, i.e. the low-resolution rows y - 1, y, y (a = 0) / y, y, y + 1 (a = 1) for dy = 0, 1, 2: taps that meet the same low-resolution
    pixel are summed -- rows {0}, {1, 2} for a = 0 and {0, 1}, {2} for a = 1 (columns alike); tap (i, j) of phase (a, b) reads pixel
    (y + a - 1 + i, x + b - 1 + j).  Plain fp32 sums of the reference's taps (generators/common/blocks.py:74-88)."""
    r = [[w[:, :, 0], w[:, :, 1] + w[:, :, 2]], [w[:, :, 0] + w[:, :, 1], w[:, :, 2]]]          # [a][i] -> [Cout, Cin, 3 (dx)]
    out = []
    for a in range(2):
        for b in range(2):
            taps = []
            for i in range(2):
                row = r[a][i]
                cols = [[row[..., 0], row[..., 1] + row[..., 2]], [row[..., 0] + row[..., 1], row[..., 2]]][b]
                taps.append(torch.stack(cols, dim=-1))
            out.append(torch.stack(taps, dim=-2))          # [Cout, Cin, 2 (i), 2 (j)]
    return torch.stack(out, dim=2).contiguous()           # [Cout, Cin, 4 (phase = 2a + b), 2, 2]


def pack_phase_weights(w: Tensor, prec: int, dgrad: bool = False) -> WeightPack:
    """[4 phases x 4 taps] pack of the phase-decomposed x2-upsampled 3x3 conv: forward [CoutP][CinP] (``conv16(..., upsample=True, phase=True)``) or
    data gradient [CinP][CoutP] -- lp_pack_weights modes 2 / 3 (the tap sums happen inside the pack launch; ``phase_weights`` is their torch form)"""
    return pack_weights(w, 3 if dgrad else 2, prec)


class PackBatch:
    """16-bit packs of MANY conv weights, refreshed by one or two launches.  ``specs`` = [(w, mode, small_k)]; the pack buffers and
    the device descriptor tables are allocated once (static addresses: hipGraph friendly); ``update()`` re-packs all entries from
    the current weight values and returns the list of WeightPacks (same order as ``specs``).  A weight that appears in both
    orientations (training: forward + data-gradient pack) is handled by lp_pack_weights_pairs -- one coalesced read of W through an
    LDS tile for both packs; the rest by lp_pack_weights_batch.  ``precs``: operand mode per entry (a net whose blocks run in different
    modes: nn.Generator's fp16 tail); default: ``prec`` for all."""

    def __init__(self, specs, prec: int, precs=None):
        import struct
        assert _lib.lib().lp_pack_desc_bytes() == 56 and _lib.lib().lp_pack_pair_desc_bytes() == 80
        self.prec = prec
        self.precs = tuple(precs) if precs is not None else (prec,) * len(specs)
        assert len(self.precs) == len(specs)
        self.key = tuple((w.data_ptr(), mode, bool(sk)) for w, mode, sk in specs)
        self.packs = []
        geo = []
        for (w, mode, small_k), prec in zip(specs, self.precs):
            _chk(w, 'w')
            cout, cin, taps, taps_out, rows, cols, rows_p, cols_p = _pack_geometry(w, mode, small_k)
            hi = torch.empty((taps_out, rows_p, cols_p), dtype=torch.int16, device=w.device)
            lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
            self.packs.append(WeightPack(hi, lo, rows, cols, rows_p, cols_p, taps_out))
            geo.append((w, mode, cout, cin, taps))
        by_w = {}
        for i, (w, mode, *_rest) in enumerate(geo):
            by_w.setdefault(w.data_ptr(), {}).setdefault(mode, i)
        paired = {}
        for ptr, modes in by_w.items():
            if 0 in modes and 1 in modes and geo[modes[0]][4] in (1, 9):
                paired[modes[0]] = modes[1]
        in_pair = set(paired) | set(paired.values())
        blob, pblob = bytearray(), bytearray()
        self.chunks = self.tiles = self.nsingle = self.npair = 0
        lop = lambda pk: 0 if pk.lo is None else pk.lo.data_ptr()
        for i, (w, mode, cout, cin, taps) in enumerate(geo):
            pk = self.packs[i]
            prec = self.precs[i]
            if i in paired:
                pk1 = self.packs[paired[i]]
                assert self.precs[paired[i]] == prec, 'both orientations of one weight are packed in one operand mode'
                tco = (max(pk.rows_p, pk1.cols_p) + 31) // 32
                tci = (max(pk.cols_p, pk1.rows_p) + 31) // 32
                pblob += struct.pack('<QQQQQiiiiiiiiii', w.data_ptr(), pk.hi.data_ptr(), lop(pk), pk1.hi.data_ptr(), lop(pk1), cout, cin, taps,
                                     pk.rows_p, pk.cols_p, pk1.rows_p, pk1.cols_p, self.tiles, tci, _f16(prec))
                self.tiles += tco * tci
                self.npair += 1
            elif i not in in_pair:
                blob += struct.pack('<QQQiiiiiiii', w.data_ptr(), pk.hi.data_ptr(), lop(pk), cout, cin, taps, pk.rows_p, pk.cols_p, mode,
                                    self.chunks, _f16(prec))
                self.chunks += (pk.taps * pk.rows_p * pk.cols_p + 1023) // 1024
                self.nsingle += 1
        dev = specs[0][0].device
        self.table = torch.frombuffer(blob, dtype=torch.uint8).clone().to(dev) if self.nsingle else None
        self.ptable = torch.frombuffer(pblob, dtype=torch.uint8).clone().to(dev) if self.npair else None

    def update(self):
        if self.npair:
            check(_lib.lib().lp_pack_weights_pairs(self.ptable.data_ptr(), self.npair, self.tiles, _stream()), 'lp_pack_weights_pairs')
        if self.nsingle:
            check(_lib.lib().lp_pack_weights_batch(self.table.data_ptr(), self.nsingle, self.chunks, _stream()), 'lp_pack_weights_batch')
        return self.packs


class Act16(NamedTuple):
    """Operand planes of a conv input: ``hi`` (, ``lo``) int16 [N,H,W,C8] holding act(x) * scale in the operand format of the
    precision mode; ``c`` = logical channels (C8 = c rounded up to 8, pad channels zero); ``inv`` = device scalar 1/scale of an
    fp16 gradient operand (None: unscaled)."""
    hi: Tensor
    lo: Optional[Tensor]
    c: int
    inv: Optional[Tensor]

    @property
    def nhw(self):
        return tuple(self.hi.shape[:3])


def _alloc16(n, h, w, c, prec, device):
    c8 = _round_up(c, 8)
    hi = torch.empty((n, h, w, c8), dtype=torch.int16, device=device)
    lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
    return hi, lo


FUSE_AMAX = os.environ.get('LP_FUSE_AMAX', '1') != '0'      # LP_FUSE_AMAX=0: every gradient operand gets its own amax pass (test knob)
AMAX_STATS = {'fused': 0, 'pass': 0}


class _AmaxSlots:
    """Zeroed slot groups (lp_amax_slots() slots, lp_amax_slot_stride() floats apart) for the kernels that fold max|y| of a gradient tensor into their epilogue.
    Handed out from one buffer zeroed by a single fill launch; under hipGraph capture the buffer (and its fill) belong to the
    capture, so every replay starts from zeros."""

    def __init__(self):
        self.buf, self.pos, self.captured, self.n = None, 0, False, 0

    def take(self, device):
        if not self.n:
            self.n = _lib.lib().lp_amax_slots() * _lib.lib().lp_amax_slot_stride()
        capturing = torch.cuda.is_current_stream_capturing()
        if (self.buf is None or self.pos + self.n > self.buf.numel() or self.buf.device != device or capturing != self.captured):
            self.buf = torch.zeros(self.n * 256, dtype=torch.float32, device=device)
            self.pos, self.captured = 0, capturing
        s = self.buf[self.pos:self.pos + self.n]
        self.pos += self.n
        return s


_AMAX_SLOTS = _AmaxSlots()


def _amax_attach(out: Tensor, want: bool):
    """slot group for a kernel about to write gradient tensor ``out`` (or None): remembered on the tensor object, together with its
    version counter -- an in-place update (autograd accumulating a second gradient into it) invalidates the recorded maximum"""
    if not (want and FUSE_AMAX):
        return None
    slots = _AMAX_SLOTS.take(out.device)
    out._lp_amax = (slots, out._version)
    return slots


def act_pack(x: Tensor, *, pro: int = 0, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None, prec: int = PREC_BF16,
             grad: bool = False) -> Act16:
    """x [N,H,W,C] fp32 -> operand planes of act(x): pro 0 identity | 1 relu(x*scale[n,c]+shift[n,c]) | 2 relu(x) |
    3 relu6(x*scale[c]+shift[c]) | 4 relu(x*scale[c]+shift[c]) | 5 x*scale[c]+shift[c] (3 .. 5: a BatchNorm folded to a per-channel affine).
    ``grad``: x is a gradient (dY): in fp16 mode it is scaled by a power of two taken from its amax (two extra small launches) so
    that it sits in the fp16 normal range; the consumer gets 1/scale through ``Act16.inv``."""
    _chk(x, 'x')
    n, h, w, c = x.shape
    hi, lo = _alloc16(n, h, w, c, prec, x.device)
    sc = part = None
    npart, pstride = 0, 1
    if grad and prec == PREC_F16:
        rec = getattr(x, '_lp_amax', None)
        if rec is not None and rec[1] == x._version and FUSE_AMAX:
            part, npart, pstride = rec[0], _lib.lib().lp_amax_slots(), _lib.lib().lp_amax_slot_stride()    # folded in by the kernel that wrote x
            sc = torch.empty(2, dtype=torch.float32, device=x.device)
            AMAX_STATS['fused'] += 1
        else:
            npart = _lib.lib().lp_amax_blocks()
            buf = torch.empty(npart + 2, dtype=torch.float32, device=x.device)
            part, sc = buf[:npart], buf[npart:]
            check(_lib.lib().lp_amax_partial(x.data_ptr(), x.numel(), part.data_ptr(), _stream()), 'lp_amax_partial')
            AMAX_STATS['pass'] += 1
    for t, nm in ((scale, 'scale'), (shift, 'shift')):
        if t is not None:
            _chk(t, nm)
    check(_lib.lib().lp_act_pack(x.data_ptr(), _p(scale), _p(shift), pro, hi.data_ptr(), _p(lo), n, h * w, c, prec, None, _p(part), npart,
                                 pstride, _p(sc), _stream()), 'lp_act_pack')
    return Act16(hi, lo, c, None if sc is None else sc[1:])


class ConvStats(NamedTuple):
    """{count, mean, M2} partials a conv epilogue left behind: ``part`` [rows, Cout, 3] floats, ``rows`` partial rows per image"""
    part: Tensor
    rows: int
    images: int = 1         # images of the launch: a BatchNorm over all of them merges rows * images partials per channel


def conv16(a: Act16, pack: WeightPack, *, ksize: int, upsample: bool = False, bias: Optional[Tensor] = None,
           res: Optional[Tensor] = None, res_shift: int = 0, alpha: Optional[Tensor] = None, prec: int = PREC_BF16,
           relu_mask: Optional[Act16] = None, out16: Optional[int] = None, amax: bool = False, stats: bool = False, want_y: bool = True,
           kind: str = 'conv_igemm', phase: bool = False, phase_dgrad: bool = False, y_relu: bool = False, res_bits: Optional[Tensor] = None):
    """y = alpha * conv(up2?(a), pack) + bias + res on operand planes; a [N,Hin,Win,C8] -> y [N,H,W,Cout] fp32.
    ``res_bits`` (uint8 [N,H,W,Cout/8], the one-bit pattern of ``bn_add_act(want_bits=True)``; Cout % 8 == 0, no ``res_shift``): the residual is
    GATED, y += res where the bit is set and += 0 elsewhere (lp_conv16_fwd_gated) -- the skip gradient d_out * [out > 0] of a residual block taken
    from d_out itself.
    ``relu_mask``: operand planes [N,H,W,Co8] of the forward conv's input; y is zeroed where they are <= 0 (fused ReLU backward
    when this launch is a data gradient).  ``out16`` = 0 | 1: also return the operand planes of y (1: of relu(y)) -> (y, Act16).
    ``stats``: the epilogue also leaves the norm-statistics partials of y -> (..., ConvStats | None) appended (None: geometry not covered
    by the fused path -- run ``instnorm_stats`` / ``bn_train_stats`` on y).  ``want_y=False`` (with ``out16`` and Cout % 8 == 0): no fp32 y
    is written, y is returned as None.  ``phase`` (with ``upsample``, 3x3; round 6): ``pack`` is a ``pack_phase_weights`` image and the conv runs in
    its phase-decomposed form -- per output phase (a, b) a 2 x 2 conv on the low-resolution planes with the coinciding taps pre-summed: the same
    result with 4/9 of the matrix work.  ``phase_dgrad``: ``a`` = the planes of dy [N, 2H, 2W, C8] of such a conv, ``pack`` =
    ``pack_phase_weights(w, prec, dgrad=True)`` -> the gradient w.r.t. the LOW-resolution input [N, H, W, Cout] (the upsample's 2x2 sum included).
    The same two kernel forms run a 3x3 conv FOLLOWED BY AvgPool2d(2) as one 4x4 stride-2 conv (``pack_weights`` modes 4 / 5; nn.ConvPoolFn):
    ``phase_dgrad`` with a mode-4 pack = pooled conv output from the full-resolution planes, ``phase`` with a mode-5 pack = its data gradient.
    ``y_relu``: y is stored as relu(y) (the next block's in-place ReLU)."""
    n, hin, win = a.nhw
    cin = a.c
    assert not phase or (upsample and ksize == 3)
    assert not phase_dgrad or (ksize == 3 and not upsample and not phase and hin % 2 == 0 and win % 2 == 0)
    assert cin == pack.cols and pack.taps == (16 if (phase or phase_dgrad) else ksize * ksize), (a.hi.shape, a.c, pack.rows, pack.cols, pack.taps)
    h, w = (hin * 2, win * 2) if upsample else (hin // 2, win // 2) if phase_dgrad else (hin, win)
    cout = pack.rows
    dev = a.hi.device
    if not want_y:
        assert out16 is not None and cout % 8 == 0 and not amax, 'want_y=False needs out16 and Cout % 8 == 0'
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=dev) if want_y else None
    for t, nm in ((bias, 'bias'), (res, 'res')):
        if t is not None:
            _chk(t, nm)
    if res is not None:
        assert res.shape == (n, h >> res_shift, w >> res_shift, cout), (res.shape, (n, h, w, cout), res_shift)
    if relu_mask is not None:
        assert relu_mask.hi.shape == (n, h, w, _round_up(cout, 8)), (relu_mask.hi.shape, (n, h, w, cout))
    if res_bits is not None:
        assert res is not None and res_shift == 0 and cout % 8 == 0 and res_bits.dtype == torch.uint8 and res_bits.is_cuda and \
            res_bits.is_contiguous() and res_bits.shape == (n, h, w, cout // 8), (res_bits.shape, (n, h, w, cout), res_shift)
    o_hi = o_lo = None
    if out16 is not None:
        o_hi, o_lo = _alloc16(n, h, w, cout, prec, dev)
    slots = _amax_attach(y, amax and prec == PREC_F16) if y is not None else None       # y is a gradient that will be packed: max|y| from the epilogue
    ws_bytes = _lib.lib().lp_conv16_fwd_workspace_bytes(n, h, w, cout, ksize)          # split-K partial tiles (small feature maps)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=dev) if ws_bytes else None
    st_buf, st_rows, st_cap = None, None, 0
    if stats:
        import ctypes
        st_cap = _lib.lib().lp_conv16_stats_floats(n, h, w, cout)
        st_buf = torch.empty(st_cap, dtype=torch.float32, device=dev)
        st_rows = ctypes.c_int(0)
    pl = 4 if prec == PREC_BF16X3 else 2              # bytes per operand-plane element
    nbytes = (n * hin * win * a.hi.shape[3] * pl + pack.hi.numel() * pl + (n * (h >> res_shift) * (w >> res_shift) * cout * 4 if res is not None else 0)
              + (res_bits.numel() if res_bits is not None else 0),
              n * h * w * cout * ((4 if want_y else 0) + (pl if out16 is not None else 0)))          # (read: planes once + weights + residual, write)
    # (roofline accounting: the DENSE count of the conv as the reference executes it -- the phase forms do 4/9 of it; the data-gradient form's dense
    #  conv lives on the 2h x 2w grid)
    dh, dw_ = (2 * h, 2 * w) if phase_dgrad else (h, w)
    with _Timed(kind, 2.0 * n * dh * dw_ * cout * cin * ksize * ksize, (n, dh, dw_, cin, cout, ksize, 3 if phase_dgrad else 2 if phase else int(upsample), 0), nbytes,
                mm=3 if prec == PREC_BF16X3 else 1):
        tail = (_p(alpha), _p(a.inv), n, h, w, cin, cout, pack.cols_p, pack.rows_p, ksize, 3 if phase_dgrad else 2 if phase else int(upsample),
                res_shift, prec, None if relu_mask is None else relu_mask.hi.data_ptr(), _p(o_hi), _p(o_lo),
                int(bool(out16)) | (2 if y_relu else 0), _p(ws), ws_bytes, _p(slots), _p(st_buf), st_cap,
                None if st_rows is None else ctypes.addressof(st_rows), _stream())
        if res_bits is not None:
            check(_lib.lib().lp_conv16_fwd_gated(a.hi.data_ptr(), _p(a.lo), pack.hi.data_ptr(), _p(pack.lo), _p(y), _p(bias), _p(res), res_bits.data_ptr(), *tail),
                  'lp_conv16_fwd')
        else:
            check(_lib.lib().lp_conv16_fwd_stats(a.hi.data_ptr(), _p(a.lo), pack.hi.data_ptr(), _p(pack.lo), _p(y), _p(bias), _p(res), *tail), 'lp_conv16_fwd')
    out = (y,) if out16 is None else (y, Act16(o_hi, o_lo, cout, None))
    if stats:
        out = out + ((ConvStats(st_buf, st_rows.value, n) if st_rows.value > 0 else None),)
    return out[0] if len(out) == 1 else out


_FORM_CONV = ('what', 'kernel', 'ks', 'ups', 'wm', 'wn', 'mr', 'nr', 'cc', 'pp', 'nbuf', 'ksplit', 'a_dbuf', 'stats', 'finish', 'tiles', 'lth', 'ltw', 'lnb')
_FORM_WGRAD = ('what', 'kernel', 'ks', 'ups', 'cob', 'splits', 'red', 'bias', 'tiles', 'lth', 'ltw', 'lnb')
_FORM_KERNEL = {1: {1: 'dma', 2: 'pipe', 3: 'pipe1x1'}, 2: {1: 'generic', 2: '1x1', 3: 'pipe3'}}
_FORM_RED = {0: None, 1: 'tiled', 2: 'flat32', 3: 'flat256'}


def last_launch_form() -> dict:
    """the form the conv / weight-gradient dispatcher chose for this thread's last launch (lp_last_launch_form, include/lp_hip.h) as a dict:
    ``what`` None | 'conv' | 'wgrad', ``kernel`` by name, the slots by name, ``prec``.  A diagnostic for tests: host state only, nothing is synchronised."""
    import ctypes
    rec = (ctypes.c_int * 20)()
    check(_lib.lib().lp_last_launch_form(ctypes.addressof(rec), 20), 'lp_last_launch_form')
    v = list(rec)
    if v[0] == 0:
        return {'what': None}
    names = _FORM_CONV if v[0] == 1 else _FORM_WGRAD
    d = dict(zip(names, v))
    d['what'] = 'conv' if v[0] == 1 else 'wgrad'
    d['kernel'] = _FORM_KERNEL[v[0]][v[1]]
    d['prec'] = v[19]
    if v[0] == 2:
        d['red'] = _FORM_RED[d['red']]
    return d


_THIN = os.environ.get('LP_THIN', '1') != '0'     # LP_THIN=0: thin-channel layers through the MFMA kernels (test knob)
_THIN_MFMA = os.environ.get('LP_THIN_MFMA', '1') != '0'


def thin_conv_supported(cin: int, cout: int, ksize: int, w: int) -> bool:
    return _THIN and bool(_lib.lib().lp_thin_conv_supported(cin, cout, ksize, w))


def thin_conv(x: Tensor, pack: WeightPack, *, ksize: int, bias: Optional[Tensor] = None, alpha: Optional[Tensor] = None,
              prec: int = PREC_BF16, out16: Optional[int] = None, out16_prec: Optional[int] = None, want_y: bool = True):
    """conv with <= 4 input channels (RGB -> 64, dz -> 64) on the plain NHWC tensor (no input operand planes): fp32 VALU kernel, or --
    RGB 3x3 in the fp16 / bf16 modes -- one MFMA k-step per output block.  ``out16`` = 0 | 1: also return the operand planes of y
    (1: of relu(y)) -> (y, Act16); written by the same launch where the MFMA kernel runs, by a pack pass otherwise."""
    _chk(x, 'x')
    n, h, w, cin = x.shape
    cout = pack.rows
    # ``out16_prec``: operand mode of the emitted planes when it differs from this conv's own (a strict first layer feeding fp16 layers)
    oprec = prec if out16_prec is None else out16_prec
    fused = out16 is not None and oprec == prec and bool(_lib.lib().lp_thin_conv_emits_planes(cin, cout, ksize, w, prec)) and _THIN_MFMA
    # ``want_y=False``: planes-only output where the MFMA kernel emits them (else y is produced and dropped by the caller)
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.device) if (want_y or not fused) else None
    o_hi = torch.empty((n, h, w, cout), dtype=torch.int16, device=x.device) if fused else None
    with _Timed('conv_thin', 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, 0, 0)):
        check(_lib.lib().lp_thin_conv_fwd(x.data_ptr(), pack.hi.data_ptr(), _p(pack.lo), _p(y), _p(bias), _p(alpha), n, h, w, cin,
                                          cout, pack.cols_p, pack.rows_p, ksize, prec, _p(o_hi), int(bool(out16)), _stream()),
              'lp_thin_conv_fwd')
    if out16 is None:
        return y
    if fused:
        return y, Act16(o_hi, None, cout, None)
    return y, act_pack(y, pro=2 if out16 else 0, prec=oprec)


# ---- first layer of the stickman-conditioned nets: 5..8 input channels gathered from TWO fp32 tensors (csrc/conv_stem8.hip) -------------------
def stem8_cmap(order) -> int:
    """channel map of a two-source conv input: ``order`` = [(source 0 | 1, channel inside that source)] per conv input channel -> packed nibbles"""
    order = list(order)
    assert 5 <= len(order) <= 8 and all(s in (0, 1) and 0 <= c < 8 for s, c in order), order
    v = 0
    for i, (s, c) in enumerate(order):
        v |= ((s << 3) | c) << (4 * i)
    return v


def stem8_cmap_order(cmap: int, cin: int):
    return [((cmap >> (4 * i + 3)) & 1, (cmap >> (4 * i)) & 7) for i in range(cin)]


# The two-source route has not been timed against the generic one on an MI355X yet (scripts/stem8_micro.py), so it is OPT-IN: LP_STEM8=1 routes the
# first convs of the FSTH family through csrc/conv_stem8.hip; the default is the generic MFMA path on the materialised concatenation.
_STEM8 = os.environ.get('LP_STEM8', '0') != '0'


def stem8_supported(cin: int, cout: int, ksize: int, w: int) -> bool:
    """the two-source kernels cover the shape (LP_THIN=0: never -- the test knob sends every thin-channel layer through the generic MFMA path)"""
    return _THIN and bool(_lib.lib().lp_stem8_supported(cin, cout, ksize, w))


def stem8_route(cin: int, cout: int, ksize: int, w: int) -> bool:
    """the first layer of a two-source input runs on the two-source kernels: LP_STEM8=1 and a covered shape"""
    return _STEM8 and stem8_supported(cin, cout, ksize, w)


def _src4(t: Optional[Tensor], name: str):
    """logical N x C x H x W fp32 CUDA tensor with ANY strides (or None) -> ((pointer, address of its 4 element strides, channels) as they go into
    the C call, the stride array itself: the caller holds it until the call has returned)"""
    import ctypes
    if t is None:
        return (None, None, 0), None
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 4):
        raise ValueError(f'{name}: expected a 4-D fp32 CUDA tensor, got {t.dtype} {t.device} dim={t.dim()}')
    st = (ctypes.c_longlong * 4)(*t.stride())
    return (t.data_ptr(), ctypes.addressof(st), t.shape[1]), st


def _c_int32(v: int) -> int:
    return v - (1 << 32) if v >= (1 << 31) else v


def stem8_conv(xa: Optional[Tensor], xb: Optional[Tensor], cmap: int, pack: WeightPack, *, ksize: int, cin: int, bias: Optional[Tensor] = None,
               alpha: Optional[Tensor] = None, prec: int = PREC_BF16, out16: Optional[int] = None, want_y: bool = True):
    """y [N,H,W,Cout] = alpha * conv(concat_by_cmap(xa, xb), pack) + bias on the matrix cores, the sources read in place (logical NCHW, any strides).
    ``out16`` = 0 | 1: also return the operand planes of y (1: of relu(y)), written by the same launch -> (y, Act16); ``want_y=False``: planes only."""
    ref = xa if xa is not None else xb
    n, _, h, w = ref.shape
    assert xa is None or xb is None or (xa.shape[0], xa.shape[2], xa.shape[3]) == (xb.shape[0], xb.shape[2], xb.shape[3]), (xa.shape, xb.shape)
    cout = pack.rows
    assert want_y or out16 is not None
    y = torch.empty((n, h, w, cout), dtype=torch.float32, device=ref.device) if want_y else None
    o_hi, o_lo = _alloc16(n, h, w, cout, prec, ref.device) if out16 is not None else (None, None)
    (a, keep_a), (b, keep_b) = _src4(xa, 'xa'), _src4(xb, 'xb')
    pl = 4 if prec == PREC_BF16X3 else 2
    nbytes = (n * h * w * cin * 4, n * h * w * cout * ((4 if want_y else 0) + (pl if out16 is not None else 0)))
    with _Timed('conv_thin', 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, 0, 0), nbytes, mm=3 if prec == PREC_BF16X3 else 1):
        check(_lib.lib().lp_stem8_fwd(*a, *b, _c_int32(cmap), pack.hi.data_ptr(), _p(pack.lo), _p(y), _p(bias), _p(alpha), n, h, w, cin, cout,
                                      pack.cols_p, pack.rows_p, ksize, prec, _p(o_hi), _p(o_lo), int(bool(out16)), _stream()), 'lp_stem8_fwd')
    if out16 is None:
        return y
    return y, Act16(o_hi, o_lo, cout, None)


def stem8_wgrad(xa: Optional[Tensor], xb: Optional[Tensor], cmap: int, dy: Tensor, *, ksize: int, cin: int, sn=None, accum: Optional[Tensor] = None,
                bias_grad: bool = False):
    """dw [Cout,Cin,k,k] (and db [Cout]) of ``stem8_conv`` from the fp32 gradient dy [N,H,W,Cout]; fp32, the same summation order in every run.
    ``sn`` / ``accum`` as in ``conv_wgrad16``."""
    _chk(dy, 'dy')
    n, h, w, cout = dy.shape
    ws = torch.empty(_lib.lib().lp_stem8_wgrad_workspace_bytes(n, h, cout, ksize) // 4, dtype=torch.float32, device=dy.device)
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=dy.device)
    db = torch.empty(cout, dtype=torch.float32, device=dy.device) if bias_grad else None
    (a, keep_a), (b, keep_b) = _src4(xa, 'xa'), _src4(xb, 'xb')
    with _Timed('wgrad_thin', 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, 0, 0), (n * h * w * (cout + cin) * 4, dw.numel() * 4)):
        check(_lib.lib().lp_stem8_wgrad(*a, *b, _c_int32(cmap), dy.data_ptr(), dw.data_ptr(), _p(db), ws.data_ptr(), n, h, w, cin, cout, ksize,
                                        _stream()), 'lp_stem8_wgrad')
    dw = _sn_finish(dw, sn, accum)
    return (dw, db) if bias_grad else dw


def stem8_dgrad(dy: Tensor, w_orig: Tensor, alpha: Optional[Tensor], cmap: int, cb: int, *, ksize: int) -> Tensor:
    """gradient of ``stem8_conv`` w.r.t. its SECOND source (the image; the stickman has none) -> contiguous N x Cb x H x W; fp32 on fp32 W_orig"""
    _chk(dy, 'dy'); _chk(w_orig, 'w_orig')
    n, h, w, cout = dy.shape
    cin = w_orig.shape[1]
    dx = torch.empty((n, cb, h, w), dtype=torch.float32, device=dy.device)
    (_, dx_strides, _), keep = _src4(dx, 'dx')
    with _Timed('conv_thin', 2.0 * n * h * w * cout * cb * ksize * ksize, (n, h, w, cout, cb, ksize, 0, 0), (dy.numel() * 4, dx.numel() * 4)):
        check(_lib.lib().lp_stem8_dgrad(dy.data_ptr(), w_orig.data_ptr(), _p(alpha), dx.data_ptr(), dx_strides, cb, _c_int32(cmap), n, h, w,
                                        cin, cout, ksize, _stream()), 'lp_stem8_dgrad')
    return dx


def embed_tail_fwd(out: Tensor, b: int, k: int, use_max: bool):
    """conv embedders' tail: out [B*K,H,W,C] -> (embeds_elemwise [B,K,C] = sum_hw relu(out), embeds [B,C] = mean | max over K, argk | None), one launch"""
    _chk(out, 'out')
    bk, h, w, c = out.shape
    assert bk == b * k, (out.shape, b, k)
    elem = torch.empty((b, k, c), dtype=torch.float32, device=out.device)
    embeds = torch.empty((b, c), dtype=torch.float32, device=out.device)
    argk = torch.empty((b, c), dtype=torch.int32, device=out.device) if use_max else None
    check(_lib.lib().lp_embed_tail_fwd(out.data_ptr(), elem.data_ptr(), embeds.data_ptr(), _p(argk), b, k, h * w, c, int(use_max), _stream()), 'lp_embed_tail_fwd')
    return elem, embeds, argk


def embed_tail_bwd(out: Tensor, g_elem: Optional[Tensor], g_embeds: Optional[Tensor], argk: Optional[Tensor], b: int, k: int, use_max: bool) -> Tensor:
    for t, nm in ((g_elem, 'g_elem'), (g_embeds, 'g_embeds')):
        if t is not None:
            _chk(t, nm)
    bk, h, w, c = out.shape
    d_out = torch.empty_like(out)
    check(_lib.lib().lp_embed_tail_bwd(out.data_ptr(), _p(g_elem), _p(g_embeds), _p(argk), d_out.data_ptr(), b, k, h * w, c, int(use_max), _stream()),
          'lp_embed_tail_bwd')
    return d_out


def conv(x: Tensor, pack: WeightPack, *, ksize: int, upsample: bool = False, pro: int = 0, scale: Optional[Tensor] = None,
         shift: Optional[Tensor] = None, bias: Optional[Tensor] = None, res: Optional[Tensor] = None, res_shift: int = 0,
         alpha: Optional[Tensor] = None, prec: int = PREC_BF16, relu_mask: Optional[Tensor] = None, grad: bool = False) -> Tensor:
    """Convenience form on an fp32 NHWC tensor: y = alpha * conv(up2?(act(x)), pack) + bias + res = lp_act_pack + lp_conv16_fwd
    (or the thin-channel kernel for <= 4 input channels).  ``relu_mask`` fp32 [N,H,W,Cout]: y zeroed where relu_mask <= 0.
    ``grad``: x is a gradient (fp16 mode scales it).  Callers that reuse the planes (forward + weight gradient) use
    ``act_pack`` / ``conv16`` directly."""
    _chk(x, 'x')
    cin = x.shape[3]
    if (not upsample and pro == 0 and res is None and relu_mask is None and thin_conv_supported(cin, pack.rows, ksize, x.shape[2])):
        return thin_conv(x, pack, ksize=ksize, bias=bias, alpha=alpha, prec=prec)
    a = act_pack(x, pro=pro, scale=scale, shift=shift, prec=prec, grad=grad)
    m16 = None
    if relu_mask is not None:
        m16 = act_pack(relu_mask, pro=0, prec=PREC_BF16)      # (bf16 keeps the sign / zero-ness of every normal fp32 value)
    return conv16(a, pack, ksize=ksize, upsample=upsample, bias=bias, res=res, res_shift=res_shift, alpha=alpha, prec=prec, relu_mask=m16)


def default_splits(n, h, w, cin, cout, ksize=3, prec=None, bias=False):
    """pixel-range splits of the weight-gradient launch.  3x3: ~2 workgroups per CU in total (9 taps of MFMA work per staged tile).
    1x1 without a bias gradient (wgrad1x1_kernel: 128 x 128 weight tiles, 64-pixel stages): one resident set of workgroups -- 2 per CU
    (64 KB of LDS each; 1 per CU for bf16x3's doubled planes) -- each walking >= 8 stages, a multiple of 8 so that the tiles of one
    pixel range share an XCD.  1x1 with a bias gradient (conv_wgrad_kernel): ~4 workgroups per CU, >= 4 128-pixel tiles each."""
    if ksize == 1 and not bias:
        stages = (n * h * w + 63) // 64
        blocks = (_round_up(cout, 64) + 127) // 128 * ((_round_up(cin, 64) + 127) // 128)
        s = max(1, min(512 // blocks, stages // 8))          # (bf16x3 too since round 4: 32-pixel stages, two workgroups per CU)
        return s // 8 * 8 if s >= 8 else s
    tiles = (n * h * w + 127) // 128
    if ksize == 1:
        blocks = (_round_up(cout, 128) // 128 if cout >= 128 else 1) * (_round_up(cin, 64) // 64)
        return max(1, min(1024 // blocks, tiles // 4))
    blocks = _round_up(cout, 64) // 64 * (_round_up(cin, 64) // 64)
    return max(1, min(512 // blocks, tiles))


# Deferred weight gradients (round 6, one-GPU meta-training step): a weight gradient whose result is ADDED to the parameter's .grad (spectral-norm rule
# included) has no consumer inside the backward pass, so its launch need not sit in the data-gradient chain.  Inside ``wgrad_defer()`` such launches
# are recorded instead of issued; ``wgrad_flush()`` issues them -- on whatever stream is current THEN (runners/holycow.py: the critic-backward
# stream, beside the encoders' backward).  The operand planes stay alive in the job list, which the caller keeps until the flushing stream has been
# joined (the planes were allocated on the backward pass's stream).  Same kernels, same operands, one contribution per parameter: bit-identical sums.
_WG_DEFER = {'active': False, 'jobs': []}


class wgrad_defer:
    def __enter__(self):
        self.prev = _WG_DEFER['active']
        _WG_DEFER['active'] = True

    def __exit__(self, *exc):
        _WG_DEFER['active'] = self.prev
        if exc[0] is not None:
            _WG_DEFER['jobs'] = []


def wgrad_flush():
    """issue the recorded weight-gradient launches on the current stream (inside nn.fused_grad_accumulation: their spectral-norm rules join its
    batched launch) -> the job list (operands): keep it until this stream has been joined"""
    jobs, _WG_DEFER['jobs'] = _WG_DEFER['jobs'], []
    prev, _WG_DEFER['active'] = _WG_DEFER['active'], False
    try:
        for args, kw in jobs:
            out = conv_wgrad16(*args, **kw)
            assert out is None or all(o is None for o in out), 'a deferred weight gradient accumulates: nothing is returned'
    finally:
        _WG_DEFER['active'] = prev
    return jobs


def conv_wgrad16(a: Act16, dy: Act16, *, ksize: int, upsample: bool = False, prec: int = PREC_BF16, splits: Optional[int] = None,
                 sn=None, accum: Optional[Tensor] = None, bias_grad: bool = False, bias_accum: Optional[Tensor] = None, kind: str = 'conv_wgrad'):
    """dw [Cout,Cin,k,k] = sum_pixels dy (x) up2?(a) (shifted by tap) on operand planes (a = what the forward conv consumed).
    ``sn`` = (w_orig, u, v, sig): the layer is spectrally normalised (forward used alpha = 1/sigma in the conv epilogue); the
    returned gradient is then w.r.t. W_orig: dw/sigma - <dw, W_orig>/sigma^2 u v^T.
    ``accum`` (with ``sn``): add that gradient to this tensor (the parameter's .grad) instead and return None.
    ``bias_grad``: return ``(dw, db)`` with db [Cout] = sum_pixels dy, produced by the same launch (the kernel streams dy anyway);
    ``bias_accum`` (the bias parameter's .grad): the launch adds db to it instead and db is returned as None."""
    n, h, w = dy.nhw
    cout, cin = dy.c, a.c
    assert a.nhw == ((n, h // 2, w // 2) if upsample else (n, h, w)), (a.hi.shape, dy.hi.shape, upsample)
    if (_WG_DEFER['active'] and sn is not None and accum is not None and (not bias_grad or bias_accum is not None)
            and SN_DEFER and _SN_DEFER['depth'] > 0):
        _WG_DEFER['jobs'].append(((a, dy), dict(ksize=ksize, upsample=upsample, prec=prec, splits=splits, sn=sn, accum=accum, bias_grad=bias_grad,
                                                bias_accum=bias_accum, kind=kind)))
        return (None, None) if bias_grad else None
    dev = dy.hi.device
    if splits is None:
        splits = default_splits(n, h, w, cin, cout, ksize, prec, bias_grad)
    ws = torch.empty(_lib.lib().lp_conv_wgrad_workspace_bytes(cin, cout, ksize, splits) // 4, dtype=torch.float32, device=dev)
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=dev)
    db = None
    if bias_grad:
        if bias_accum is not None:
            assert bias_accum.is_contiguous() and bias_accum.dtype == torch.float32 and bias_accum.numel() == cout
            db = bias_accum
        else:
            db = torch.empty(cout, dtype=torch.float32, device=dev)
    dot, ndot = None, 0
    if sn is not None:          # the reduction launch also takes <dw, W_orig> (per-block partials) for lp_sn_grad_apply
        _chk(sn[0], 'w_orig')
        ndot = _lib.lib().lp_conv_wgrad_dot_blocks(cin, cout, ksize)
        dot = torch.empty(ndot, dtype=torch.float32, device=dev)
    pl = 4 if prec == PREC_BF16X3 else 2
    nbytes = (a.hi.numel() + dy.hi.numel()) * pl + cout * cin * ksize * ksize * 4
    with _Timed(kind, 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, int(upsample), 0), nbytes, mm=3 if prec == PREC_BF16X3 else 1):
        check(_lib.lib().lp_conv16_wgrad(a.hi.data_ptr(), _p(a.lo), dy.hi.data_ptr(), _p(dy.lo), dw.data_ptr(), ws.data_ptr(), n, h, w, cin,
                                         cout, ksize, int(upsample), splits, prec, _p(db), int(bias_grad and bias_accum is not None), _p(dy.inv),
                                         None if sn is None else sn[0].data_ptr(), _p(dot), _stream()), 'lp_conv16_wgrad')
    dw = _sn_finish(dw, sn, accum, dot, ndot)
    return (dw, None if bias_accum is not None else db) if bias_grad else dw


# Launch diet (round 5): inside ``nn.fused_grad_accumulation`` the spectral-norm gradient rule of a conv weight whose result is ACCUMULATED into
# the parameter's .grad (nothing is returned to autograd) is not launched per layer; the jobs are collected and run by lp_sn_grad_apply_batch
# when the context is left (after every side stream is joined, before anything reads .grad).  LP_SN_DEFER=0: per-layer launches.
SN_DEFER = os.environ.get('LP_SN_DEFER', '1') != '0'
_SN_DEFER = {'depth': 0, 'jobs': []}


def sn_defer_begin():
    _SN_DEFER['depth'] += 1


def sn_defer_check(who: str):
    """ a reader of ``.grad`` -- the gradient exchange, an optimizer step -- must not run while deferred spectral-norm jobs are
    pending: the conv weights' gradients are incomplete until ``nn.fused_grad_accumulation`` is left.  Raises instead of reading them early."""
    if _WG_DEFER['jobs']:
        raise RuntimeError(f'{who}: {len(_WG_DEFER["jobs"])} deferred weight-gradient launches are pending (hipops.wgrad_defer without wgrad_flush)')
    if _SN_DEFER['jobs']:
        raise RuntimeError(f'{who}: {len(_SN_DEFER["jobs"])} deferred spectral-norm gradient jobs are pending -- .grad of the conv weights is '
                           'incomplete inside nn.fused_grad_accumulation; leave the context (or set LP_SN_DEFER=0) before reading gradients')


def sn_defer_end(discard: bool = False):
    """leave one level of deferral; the outermost level runs (or, after a failed backward, drops) the collected jobs"""
    _SN_DEFER['depth'] -= 1
    if _SN_DEFER['depth'] > 0:
        return
    jobs, _SN_DEFER['jobs'] = _SN_DEFER['jobs'], []
    if not jobs or discard:
        return
    import ctypes
    import struct
    assert _lib.lib().lp_sn_apply_desc_bytes() == 64
    # jobs that accumulate into the SAME tensor (two passes of the critic depositing on one parameter from one stream) must not share a launch:
    # a job joins the first round that does not hold its target yet; the rounds run one after the other on this stream
    rounds = []
    for job in jobs:
        key = job[6].data_ptr()
        for targets, members in rounds:
            if key not in targets:
                targets.add(key); members.append(job)
                break
        else:
            rounds.append(({key}, [job]))
    for _, members in rounds:
        blob = bytearray()
        for dw, u, v, sig, dot, ndot, accum in members:
            blob += struct.pack('<QQQQQQiiii', dw.data_ptr(), u.data_ptr(), v.data_ptr(), sig.data_ptr(), dot.data_ptr(), accum.data_ptr(), ndot,
                                dw.shape[0], dw.numel() // dw.shape[0], 0)
        buf = (ctypes.c_char * len(blob)).from_buffer(blob)
        check(_lib.lib().lp_sn_grad_apply_batch(ctypes.addressof(buf), len(members), _stream()), 'lp_sn_grad_apply_batch')
    # (the temporaries in `jobs` are released here, AFTER the launch was enqueued on the stream that allocated them or was joined with it)


def _sn_finish(dw, sn, accum, dot=None, ndot=0):
    if sn is None:
        return dw
    w_orig, u, v, sig = sn
    cout = dw.shape[0]
    if accum is not None and ndot > 0 and dot is not None and SN_DEFER and _SN_DEFER['depth'] > 0:
        assert accum.is_contiguous() and accum.dtype == torch.float32 and accum.numel() == dw.numel()
        _SN_DEFER['jobs'].append((dw, u, v, sig, dot, ndot, accum))
        return None
    if dot is None:
        dot = torch.empty(512, dtype=torch.float32, device=dw.device)      # per-block partials of <g, W>, taken by lp_sn_grad_apply
    if accum is not None:
        assert accum.is_contiguous() and accum.dtype == torch.float32 and accum.numel() == dw.numel()
    check(_lib.lib().lp_sn_grad_apply(dw.data_ptr(), w_orig.data_ptr(), u.data_ptr(), v.data_ptr(), sig.data_ptr(), dot.data_ptr(), ndot,
                                      _p(accum), cout, dw.numel() // cout, _stream()), 'lp_sn_grad_apply')
    return None if accum is not None else dw


# ---- reflection padding of the 3x3 ResBlock convs as a border correction of the zero-padded conv (csrc/reflect_border.hip) -----------------------
def reflect_border_fwd(a: Act16, w_orig: Tensor, alpha: Optional[Tensor], y: Tensor, *, prec: int, upsample: bool = False) -> Tensor:
    """y [N,H,W,Cout] (the zero-padded conv of up2?(a) with W_orig * alpha) += the taps that leave the image, applied to the mirrored pixels:
    afterwards y is the conv behind nn.ReflectionPad2d(1) (blocks.py:76-88 with --gen_padding / --dis_padding reflection).  In place."""
    _chk(y, 'y'); _chk(w_orig, 'w_orig')
    n, h, w, cout = y.shape
    assert a.inv is None and a.nhw == ((n, h // 2, w // 2) if upsample else (n, h, w)), (a.hi.shape, y.shape, upsample)
    assert tuple(w_orig.shape) == (cout, a.c, 3, 3), (w_orig.shape, cout, a.c)
    check(_lib.lib().lp_reflect_border_fwd(a.hi.data_ptr(), _p(a.lo), prec, n, h, w, a.c, a.hi.shape[3], int(upsample), w_orig.data_ptr(), cout,
                                           _p(alpha), y.data_ptr(), _stream()), 'lp_reflect_border_fwd')
    return y


def reflect_border_dgrad(dy: Tensor, w_orig: Tensor, alpha: Optional[Tensor], dx: Tensor, mask16: Optional[Act16] = None) -> Tensor:
    """dx [N,H,W,Cin] (the zero-padded data gradient) += the transposed border terms; ``mask16`` = planes of relu(x) when the forward applied ReLU
    in its prologue (the main launch masked its result by [x > 0] in its epilogue; the correction is masked the same way).  In place."""
    _chk(dy, 'dy'); _chk(dx, 'dx'); _chk(w_orig, 'w_orig')
    n, h, w, cout = dy.shape
    cin = dx.shape[3]
    assert tuple(dx.shape[:3]) == (n, h, w) and tuple(w_orig.shape) == (cout, cin, 3, 3), (dx.shape, dy.shape, w_orig.shape)
    assert mask16 is None or mask16.nhw == (n, h, w)
    check(_lib.lib().lp_reflect_border_dgrad(dy.data_ptr(), n, h, w, cout, w_orig.data_ptr(), cin, _p(alpha), None if mask16 is None else mask16.hi.data_ptr(),
                                             0 if mask16 is None else mask16.hi.shape[3], dx.data_ptr(), _stream()), 'lp_reflect_border_dgrad')
    return dx


def reflect_border_wgrad(a: Act16, dy: Tensor, *, prec: int, upsample: bool = False, sn=None, accum: Optional[Tensor] = None) -> Optional[Tensor]:
    """the border terms' share of the weight gradient, [Cout,Cin,3,3]; ``sn`` / ``accum`` as in ``conv_wgrad16`` (the spectral-norm gradient rule is
    linear in the raw gradient, so the share is passed through it on its own and added to the same .grad): None when accumulated."""
    _chk(dy, 'dy')
    n, h, w, cout = dy.shape
    assert a.inv is None and a.nhw == ((n, h // 2, w // 2) if upsample else (n, h, w)), (a.hi.shape, dy.shape, upsample)
    gw = torch.empty((cout, a.c, 3, 3), dtype=torch.float32, device=dy.device)
    nws = _lib.lib().lp_reflect_border_wgrad_workspace_bytes(n, h, w, a.c, cout) // 4
    ws = torch.empty(nws, dtype=torch.float32, device=dy.device) if nws else None
    check(_lib.lib().lp_reflect_border_wgrad(a.hi.data_ptr(), _p(a.lo), prec, n, h, w, a.c, a.hi.shape[3], int(upsample), dy.data_ptr(), cout,
                                             gw.data_ptr(), _p(ws), _stream()), 'lp_reflect_border_wgrad')
    return _sn_finish(gw, sn, accum)


def thin_wgrad_supported(cin: int, cout: int, ksize: int, pro: int, w: int) -> bool:
    return _THIN and bool(_lib.lib().lp_thin_wgrad_supported(cin, cout, ksize, pro, w))


def thin_wgrad(x: Tensor, dy: Tensor, *, ksize: int, pro: int = 0, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
               splits: Optional[int] = None, sn=None, accum: Optional[Tensor] = None, bias_grad: bool = False):
    """weight gradient of a conv with <= 4 channels on one side, fp32 NHWC tensors in (prologue of the wide input applied on the fly)"""
    _chk(x, 'x'); _chk(dy, 'dy')
    n, h, w, cout = dy.shape
    cin = x.shape[3]
    if splits is None:
        splits = default_splits(n, h, w, cin, cout)
    ws = torch.empty(_lib.lib().lp_conv_wgrad_workspace_bytes(cin, cout, ksize, splits) // 4, dtype=torch.float32, device=x.device)
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=x.device)
    db = None
    if bias_grad and _lib.lib().lp_thin_wgrad_has_dbias(cin, cout):
        db = torch.empty(cout, dtype=torch.float32, device=x.device)
    with _Timed('wgrad_thin', 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, 0, pro)):
        check(_lib.lib().lp_thin_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), _p(scale), _p(shift), n, h, w, cin, cout,
                                       ksize, pro, splits, _p(db), _stream()), 'lp_thin_wgrad')
    if bias_grad and db is None:
        db = dy.sum(dim=(0, 1, 2))
    dw = _sn_finish(dw, sn, accum)
    return (dw, db) if bias_grad else dw


def conv_wgrad(x: Tensor, dy: Tensor, *, ksize: int, upsample: bool = False, pro: int = 0, scale: Optional[Tensor] = None,
               shift: Optional[Tensor] = None, prec: int = PREC_BF16, splits: Optional[int] = None, sn=None,
               accum: Optional[Tensor] = None, bias_grad: bool = False):
    """Convenience form on fp32 NHWC tensors: packs act(x) and dy, then lp_conv16_wgrad (or the thin-channel kernel)."""
    _chk(x, 'x'); _chk(dy, 'dy')
    if not upsample and thin_wgrad_supported(x.shape[3], dy.shape[3], ksize, pro, dy.shape[2]):
        return thin_wgrad(x, dy, ksize=ksize, pro=pro, scale=scale, shift=shift, splits=splits, sn=sn, accum=accum, bias_grad=bias_grad)
    a = act_pack(x, pro=pro, scale=scale, shift=shift, prec=prec)
    d = act_pack(dy, pro=0, prec=prec, grad=True)
    return conv_wgrad16(a, d, ksize=ksize, upsample=upsample, prec=prec, splits=splits, sn=sn, accum=accum, bias_grad=bias_grad)


def linear_supported(b: int, k: int, fwd_only: bool = False) -> bool:
    return 1 <= b <= 64 and k % 4 == 0 and k <= (2048 if fwd_only else 1024)


def linear_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], alpha: Optional[Tensor]) -> Tensor:
    """y [B,N] = alpha * x W^T + bias (lp_linear_fwd: one pass over W, 1/sigma and bias fused)"""
    _chk(x, 'x'); _chk(w, 'w')
    b, k = x.shape
    n = w.shape[0]
    y = torch.empty((b, n), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_linear_fwd(x.data_ptr(), w.data_ptr(), _p(bias), _p(alpha), y.data_ptr(), b, n, k, _stream()), 'lp_linear_fwd')
    return y


def linear_bwd(x: Tensor, w: Tensor, g: Tensor, alpha: Optional[Tensor], want_dx: bool, want_dw: bool, want_db: bool):
    """-> (dx = alpha * g W | None, raw dw = g^T x | None, db | None) in one pass over W"""
    _chk(x, 'x'); _chk(w, 'w'); _chk(g, 'g')
    b, k = x.shape
    n = w.shape[0]
    dev = x.device
    dx = torch.empty((b, k), dtype=torch.float32, device=dev) if want_dx else None
    dw = torch.empty((n, k), dtype=torch.float32, device=dev) if want_dw else None
    db = torch.empty(n, dtype=torch.float32, device=dev) if want_db else None
    ws = torch.empty(_lib.lib().lp_linear_bwd_workspace_bytes(b, n, k) // 4, dtype=torch.float32, device=dev) if want_dx else None
    check(_lib.lib().lp_linear_bwd(x.data_ptr(), w.data_ptr(), g.data_ptr(), _p(alpha), _p(dx), _p(dw), _p(db), _p(ws), b, n, k, _stream()),
          'lp_linear_bwd')
    return dx, dw, db


def grid_crop_fwd(images: Tensor, boxes: Tensor, out_hw) -> Tensor:
    """images [N,C,H,W] fp32 NCHW, boxes [N,4] (t, b, l, r) -> crops [N,C,Ho,Wo] (bilinear, reflection, align_corners=False)"""
    _chk(images, 'images'); _chk(boxes, 'boxes')
    n, c, h, w = images.shape
    out = torch.empty((n, c) + tuple(out_hw), dtype=torch.float32, device=images.device)
    check(_lib.lib().lp_grid_crop_fwd(images.data_ptr(), boxes.data_ptr(), out.data_ptr(), n, c, h, w, out_hw[0], out_hw[1], _stream()), 'lp_grid_crop_fwd')
    return out


def grid_crop_bwd(dout: Tensor, boxes: Tensor, in_shape) -> Tensor:
    _chk(dout, 'dout'); _chk(boxes, 'boxes')
    n, c, h, w = in_shape
    dimg = torch.empty(in_shape, dtype=torch.float32, device=dout.device)
    check(_lib.lib().lp_grid_crop_bwd(dout.data_ptr(), boxes.data_ptr(), dimg.data_ptr(), n, c, h, w, dout.shape[2], dout.shape[3], _stream()),
          'lp_grid_crop_bwd')
    return dimg


# ---- MobileNetV2 pose encoder (forward): layers that are not dense contractions ------------------------------------------------
def stem_conv_s2(x: Tensor, w: Tensor) -> Tensor:
    """x [N,3,H,W] NCHW fp32, w [Cout,3,3,3] -> y [N,H/2,W/2,Cout] NHWC (3x3, stride 2, pad 1)"""
    _chk(x, 'x'); _chk(w, 'w')
    n, c, h, wd = x.shape
    assert c == 3 and tuple(w.shape[1:]) == (3, 3, 3), (x.shape, w.shape)
    y = torch.empty((n, h // 2, wd // 2, w.shape[0]), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_stem_conv_s2(x.data_ptr(), w.data_ptr(), y.data_ptr(), n, h, wd, w.shape[0], _stream()), 'lp_stem_conv_s2')
    return y


def dwconv3x3(x: Tensor, w: Tensor, stride: int, in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None) -> Tensor:
    """depthwise 3x3 (pad 1) of relu6(x*in_scale[c]+in_shift[c]) (or of x); x [N,H,W,C] NHWC, w [C,1,3,3]"""
    _chk(x, 'x'); _chk(w, 'w')
    n, h, wd, c = x.shape
    assert w.numel() == c * 9
    y = torch.empty((n, (h + stride - 1) // stride, (wd + stride - 1) // stride, c), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_dwconv3x3_fwd(x.data_ptr(), w.data_ptr(), _p(in_scale), _p(in_shift), y.data_ptr(), n, h, wd, c, stride, _stream()),
          'lp_dwconv3x3_fwd')
    return y


def pwconv(x: Tensor, w: Tensor, *, in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None, in_relu6: bool = False,
           in_res: Optional[Tensor] = None, want_x: bool = False, stats: bool = False):
    """fp32 1x1 conv y = a w^T on NHWC x, a = (relu6?)(x*in_scale+in_shift) (+ in_res).  -> (y, a | None, stats | None);
    ``stats`` = (partials, rows) for ``bn_finalize``"""
    _chk(x, 'x'); _chk(w, 'w')
    n, h, wd, k = x.shape
    cout = w.shape[0]
    assert w.numel() == cout * k
    pcount = n * h * wd
    y = torch.empty((n, h, wd, cout), dtype=torch.float32, device=x.device)
    xo = torch.empty_like(x) if want_x else None
    part, rows = None, 0
    if stats:
        rows = _lib.lib().lp_pwconv_stat_rows(pcount, k, cout)
        part = torch.empty(9 * rows * (cout // 4), dtype=torch.float32, device=x.device)
    if in_res is not None:
        _chk(in_res, 'in_res'); assert in_res.shape == x.shape
    check(_lib.lib().lp_pwconv_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), _p(in_scale), _p(in_shift), int(in_relu6), _p(in_res), _p(xo),
                                   _p(part), pcount, k, cout, _stream()), 'lp_pwconv_fwd')
    return y, xo, ((part, rows) if stats else None)


def dwconv3x3_stats(x: Tensor, w: Tensor, stride: int, in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None):
    """``dwconv3x3`` that also returns the BatchNorm partials of its output: (y, (partials, rows))"""
    _chk(x, 'x'); _chk(w, 'w')
    n, h, wd, c = x.shape
    rows = _lib.lib().lp_dwconv_stat_rows(n, h, wd, c, stride)
    assert rows > 0, c
    y = torch.empty((n, (h + stride - 1) // stride, (wd + stride - 1) // stride, c), dtype=torch.float32, device=x.device)
    part = torch.empty(9 * rows * (c // 4), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_dwconv3x3_stats_fwd(x.data_ptr(), w.data_ptr(), _p(in_scale), _p(in_shift), y.data_ptr(), part.data_ptr(), n, h, wd, c,
                                            stride, _stream()), 'lp_dwconv3x3_stats_fwd')
    return y, (part, rows)


def bn_finalize(stats, weight: Tensor, bias: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], momentum: float,
                eps: float) -> Tuple[Tensor, Tensor]:
    """train-mode BatchNorm (scale, shift) from the partials a conv launch left behind; updates the running statistics in place"""
    part, rows = stats
    c = weight.numel()
    out = torch.empty(2 * c, dtype=torch.float32, device=weight.device)
    check(_lib.lib().lp_bn_finalize(part.data_ptr(), rows, weight.data_ptr(), bias.data_ptr(), _p(running_mean), _p(running_var), out.data_ptr(),
                                    out[c:].data_ptr(), c, eps, momentum, _stream()), 'lp_bn_finalize')
    return out[:c], out[c:]


def affine_res(y: Tensor, scale: Tensor, shift: Tensor, res: Optional[Tensor] = None, prec: Optional[int] = None):
    """x = y*scale[c]+shift[c] (+res), NHWC; with ``prec`` also the operand planes of x -> (x, Act16)"""
    _chk(y, 'y')
    n, h, w, c = y.shape
    x = torch.empty_like(y)
    hi = lo = None
    if prec is not None:
        hi, lo = _alloc16(n, h, w, c, prec, y.device)
    check(_lib.lib().lp_affine_res(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), _p(res), x.data_ptr(), _p(hi), _p(lo), n * h * w, c,
                                   prec if prec is not None else 0, _stream()), 'lp_affine_res')
    return x if prec is None else (x, Act16(hi, lo, c, None))


def affine_relu6_mean(y: Tensor, scale: Tensor, shift: Tensor) -> Tensor:
    _chk(y, 'y')
    n, h, w, c = y.shape
    out = torch.empty((n, c), dtype=torch.float32, device=y.device)
    check(_lib.lib().lp_affine_relu6_mean(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), n, h * w, c, _stream()),
          'lp_affine_relu6_mean')
    return out


def bn_batch_affine(y: Tensor, weight: Tensor, bias: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor],
                    momentum: float, eps: float) -> Tuple[Tensor, Tensor]:
    """train-mode BatchNorm2d of y [N,H,W,C] as a per-channel (scale, shift), updating the running statistics in place"""
    n, h, w, c = y.shape
    _chk(y, 'y')
    p = n * h * w
    scale = torch.empty(2 * c, dtype=torch.float32, device=y.device)
    ws = torch.empty(_lib.lib().lp_bn_stats_workspace_bytes(p, c) // 4, dtype=torch.float32, device=y.device)
    check(_lib.lib().lp_bn_stats(y.data_ptr(), weight.data_ptr(), bias.data_ptr(), _p(running_mean), _p(running_var), scale.data_ptr(),
                                 scale[c:].data_ptr(), ws.data_ptr(), p, c, eps, momentum, _stream()), 'lp_bn_stats')
    return scale[:c], scale[c:]


def sn_grad_apply(g: Tensor, w_orig: Tensor, u: Tensor, v: Tensor, sig: Tensor, accum: Optional[Tensor] = None) -> Optional[Tensor]:
    """gradient w.r.t. W_orig of a spectrally normalised layer from the raw gradient ``g`` w.r.t. W/sigma (legacy-hook autograd,
    u and v constants): g/sigma - <g, W_orig>/sigma^2 u v^T, in place on ``g`` -- or added to ``accum`` (returns None)."""
    _chk(g, 'g'); _chk(w_orig, 'w_orig')
    rows = g.shape[0]
    cols = g.numel() // rows
    dot = torch.empty(512, dtype=torch.float32, device=g.device)
    if accum is not None:
        assert accum.is_contiguous() and accum.dtype == torch.float32 and accum.numel() == g.numel()
    check(_lib.lib().lp_sn_grad_apply(g.data_ptr(), w_orig.data_ptr(), u.data_ptr(), v.data_ptr(), sig.data_ptr(), dot.data_ptr(), 0,
                                      _p(accum), rows, cols, _stream()), 'lp_sn_grad_apply')
    return None if accum is not None else g


def instnorm_stats(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float
                   ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """x [N,H,W,C]; gamma/beta: [N,C] views (last dim contiguous) of the projector output.  -> mean, rstd, scale, shift [N,C]."""
    _chk(x, 'x')
    n, h, w, c = x.shape
    ab_stride = 0
    if gamma is not None:
        assert gamma.shape == (n, c) and beta.shape == (n, c) and gamma.stride(1) == 1 and beta.stride(1) == 1
        assert gamma.stride(0) == beta.stride(0)
        ab_stride = gamma.stride(0)
    mean, rstd, scale, shift = (torch.empty((n, c), dtype=torch.float32, device=x.device) for _ in range(4))
    ws = torch.empty(_lib.lib().lp_instnorm_workspace_bytes(n, h * w, c) // 4, dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_instnorm_stats(x.data_ptr(), _p(gamma), _p(beta), ab_stride, eps, mean.data_ptr(), rstd.data_ptr(),
                                       scale.data_ptr(), shift.data_ptr(), ws.data_ptr(), n, h * w, c, _stream()), 'lp_instnorm_stats')
    return mean, rstd, scale, shift


def adain_relu_bwd(dA: Tensor, x: Tensor, add: Optional[Tensor], gamma: Tensor, mean: Tensor, rstd: Tensor, scale: Tensor,
                   shift: Tensor, dgamma: Tensor, dbeta: Tensor, upsample: bool, amax: bool = False, planes: Optional[int] = None,
                   keep_dx: bool = True):
    """Backward of relu(AdaIN(x)) (+x2 upsample).  dgamma/dbeta: [N,C] views into the projector-output gradient (written).
    ``amax`` (here and below): the result will be packed as an fp16 gradient operand -- fold its max|.| into the kernel.
    ``planes`` = PREC_BF16 | PREC_BF16X3 (round 6): the result ALSO leaves as that mode's gradient operand planes, written by the same launch
    (lp_adain_relu_bwd_planes; no scale in those modes) -> (dx | None, Act16); ``keep_dx=False``: planes only."""
    _chk(dA, 'dA')
    x16 = x if isinstance(x, Act16) else None          # 16-bit-resident conv output (the generator's fp16 mode: no fp32 copy of x exists)
    if x16 is not None:
        assert x16.lo is None and x16.inv is None and x16.hi.shape[3] == x16.c, 'a 16-bit-resident x is ONE unscaled fp16 plane with C % 8 == 0'
        n, h, w, c = x16.hi.shape
    else:
        _chk(x, 'x')
        n, h, w, c = x.shape
    if planes is not None and not planes_direct_ok(planes, x, c):          # (geometry the fused form does not cover: the two-launch form)
        dx = adain_relu_bwd(dA, x, add, gamma, mean, rstd, scale, shift, dgamma, dbeta, upsample, amax=amax)
        return dx, act_pack(dx, prec=planes, grad=True)
    assert dA.shape == (n, h << int(upsample), w << int(upsample), c), (dA.shape, (n, h, w, c))
    assert gamma.stride(1) == 1 and dgamma.stride(1) == 1 and dbeta.stride(1) == 1
    assert gamma.stride(0) == dgamma.stride(0) == dbeta.stride(0)
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dA.device)          # (holds the masked gradient between the passes)
    ws = torch.empty(_lib.lib().lp_adain_bwd_workspace_bytes(n, h * w, c) // 4, dtype=torch.float32, device=dA.device)
    args = (dA.data_ptr(), (x if x16 is None else x16.hi).data_ptr(), _p(add), gamma.data_ptr(), gamma.stride(0), mean.data_ptr(), rstd.data_ptr(),
            scale.data_ptr(), shift.data_ptr(), dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), n, h, w, c, int(upsample))
    if planes is not None:
        o_hi, o_lo = _alloc16(n, h, w, c, planes, dA.device)
        check(_lib.lib().lp_adain_relu_bwd_planes(*args, o_hi.data_ptr(), _p(o_lo), int(keep_dx), _stream()), 'lp_adain_relu_bwd_planes')
        return (dx if keep_dx else None), Act16(o_hi, o_lo, c, None)
    fn, nm = (_lib.lib().lp_adain_relu_bwd, 'lp_adain_relu_bwd') if x16 is None else (_lib.lib().lp_adain_relu_bwd16, 'lp_adain_relu_bwd16')
    check(fn(*args, _p(_amax_attach(dx, amax)), _stream()), nm)
    return dx


PLANES_DIRECT = os.environ.get('LP_PLANES_DIRECT', '1') != '0'      # 0: gradient operands of the bf16 / bf16x3 modes through lp_act_pack again (A/B knob)


def planes_direct_ok(prec: int, x, c: int) -> bool:
    return PLANES_DIRECT and prec in (PREC_BF16, PREC_BF16X3) and not isinstance(x, Act16) and c % 8 == 0


def sum2x2_planes(x: Tensor, prec: int) -> 'Act16':
    """sum2x2 straight to the bf16 / bf16x3 gradient operand planes (no fp32 result, no pack launch)"""
    _chk(x, 'x')
    n, h2, w2, c = x.shape
    if not planes_direct_ok(prec, x, c):
        return act_pack(sum2x2(x, amax=prec == PREC_F16), prec=prec, grad=True)
    o_hi, o_lo = _alloc16(n, h2 // 2, w2 // 2, c, prec, x.device)
    check(_lib.lib().lp_sum2x2_planes(x.data_ptr(), None, o_hi.data_ptr(), _p(o_lo), n, h2 // 2, w2 // 2, c, _stream()), 'lp_sum2x2_planes')
    return Act16(o_hi, o_lo, c, None)


# backward of nn.ConvPoolFn in one pass over the pooled gradient (round 6, lp_pool_grad_pack; 0: where + act_pack + avgpool2_bwd + act_pack)
POOL_GRAD_FUSED = os.environ.get('LP_POOL_GRAD_FUSED', '1') != '0'


def pool_grad_pack(dy: Tensor, y_mask: Optional[Tensor], prec: int, want_dm: bool, want_lo: bool, want_up: bool):
    """dm = dy * [y_mask > 0] -> (dm fp32 | None, operand planes of dm | None, operand planes of 0.25 * nearest_up2(dm) at twice the resolution | None),
    one launch (fp16 mode: + the amax partials of dy when its producer did not leave them)"""
    _chk(dy, 'dy')
    n, h, w, c = dy.shape
    assert c % 8 == 0 and (y_mask is None or tuple(y_mask.shape) == tuple(dy.shape))
    if y_mask is not None:
        _chk(y_mask, 'y_mask')
    dev = dy.device
    dm = torch.empty_like(dy) if want_dm else None
    lo_hi, lo_lo = _alloc16(n, h, w, c, prec, dev) if want_lo else (None, None)
    up_hi, up_lo = _alloc16(n, 2 * h, 2 * w, c, prec, dev) if want_up else (None, None)
    part = sc = None
    npart, pstride = 0, 1
    if prec == PREC_F16:
        rec = getattr(dy, '_lp_amax', None)
        if rec is not None and rec[1] == dy._version and FUSE_AMAX:
            part, npart, pstride = rec[0], _lib.lib().lp_amax_slots(), _lib.lib().lp_amax_slot_stride()
            sc = torch.empty(4, dtype=torch.float32, device=dev)
        else:
            npart = _lib.lib().lp_amax_blocks()
            buf = torch.empty(npart + 4, dtype=torch.float32, device=dev)
            part, sc = buf[:npart], buf[npart:]
            check(_lib.lib().lp_amax_partial(dy.data_ptr(), dy.numel(), part.data_ptr(), _stream()), 'lp_amax_partial')
    check(_lib.lib().lp_pool_grad_pack(dy.data_ptr(), _p(y_mask), _p(dm), _p(lo_hi), _p(lo_lo), _p(up_hi), _p(up_lo), n, h, w, c, prec,
                                       _p(part), npart, pstride, _p(sc), _stream()), 'lp_pool_grad_pack')
    lo16 = Act16(lo_hi, lo_lo, c, None if sc is None else sc[1:2]) if want_lo else None
    up16 = Act16(up_hi, up_lo, c, None if sc is None else sc[3:4]) if want_up else None
    return dm, lo16, up16


def sum2x2(x: Tensor, amax: bool = False) -> Tensor:
    _chk(x, 'x')
    n, h2, w2, c = x.shape
    out = torch.empty((n, h2 // 2, w2 // 2, c), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_sum2x2(x.data_ptr(), out.data_ptr(), n, h2 // 2, w2 // 2, c, _p(_amax_attach(out, amax)), _stream()), 'lp_sum2x2')
    return out


def head_fwd(z: Tensor, want_t: bool = True) -> Tuple[Optional[Tensor], Tensor, Tensor]:
    """z [N,H,W,4] -> (tanh(z) NHWC, fake_rgbs NCHW [N,3,H,W], fake_segm NCHW [N,1,H,W])."""
    _chk(z, 'z')
    n, h, w, c = z.shape
    assert c == 4
    t = torch.empty_like(z) if want_t else None
    rgbs = torch.empty((n, 3, h, w), dtype=torch.float32, device=z.device)
    segm = torch.empty((n, 1, h, w), dtype=torch.float32, device=z.device)
    check(_lib.lib().lp_head_fwd(z.data_ptr(), _p(t), rgbs.data_ptr(), segm.data_ptr(), n, h, w, _stream()), 'lp_head_fwd')
    return t, rgbs, segm


def head_bwd(t: Tensor, d_rgbs: Tensor, d_segm: Optional[Tensor], amax: bool = False) -> Tensor:
    _chk(t, 't'); _chk(d_rgbs, 'd_rgbs')
    n, h, w, _ = t.shape
    dz = torch.empty_like(t)
    if d_segm is not None:
        _chk(d_segm, 'd_segm')
    check(_lib.lib().lp_head_bwd(t.data_ptr(), d_rgbs.data_ptr(), _p(d_segm), dz.data_ptr(), n, h, w, _p(_amax_attach(dz, amax)), _stream()),
          'lp_head_bwd')
    return dz


def tanh_head_fwd(z: Tensor, want_t: bool = True) -> Tuple[Optional[Tensor], Tensor]:
    """z [N,H,W,Cz], Cz = 3 | 4 (a fourth channel is launch padding) -> (tanh(z) NHWC | None, fake_rgbs NCHW [N,3,H,W] = tanh(z[..., :3])):
    the head of generators/FSTH.py -- no mask, no range shift."""
    _chk(z, 'z')
    n, h, w, cz = z.shape
    t = torch.empty_like(z) if want_t else None
    rgbs = torch.empty((n, 3, h, w), dtype=torch.float32, device=z.device)
    check(_lib.lib().lp_tanh_head_fwd(z.data_ptr(), _p(t), rgbs.data_ptr(), n, h, w, cz, _stream()), 'lp_tanh_head_fwd')
    return t, rgbs


def tanh_head_bwd(t: Tensor, d_rgbs: Tensor, amax: bool = False) -> Tensor:
    """dz [N,H,W,Cz] = d_rgbs (NCHW) * (1 - t^2), an exact zero in a padding channel"""
    _chk(t, 't'); _chk(d_rgbs, 'd_rgbs')
    n, h, w, cz = t.shape
    assert d_rgbs.shape == (n, 3, h, w), (d_rgbs.shape, t.shape)
    dz = torch.empty_like(t)
    check(_lib.lib().lp_tanh_head_bwd(t.data_ptr(), d_rgbs.data_ptr(), dz.data_ptr(), n, h, w, cz, _p(_amax_attach(dz, amax)), _stream()), 'lp_tanh_head_bwd')
    return dz


def norm_affine_grad(dgamma: Tensor, dbeta: Tensor, accum_gamma: Optional[Tensor] = None, accum_beta: Optional[Tensor] = None):
    """per-sample (dgamma, dbeta) [N,C] rows of ``adain_relu_bwd`` -> the gradients [C] of a batch-shared gamma / beta (nn.InstanceNorm2d(affine=True)),
    rows added in a fixed order.  ``accum_gamma`` / ``accum_beta`` (the parameters' .grad, both or neither): added to in place -> (None, None)."""
    n, c = dgamma.shape
    assert dbeta.shape == (n, c) and dgamma.dtype == dbeta.dtype == torch.float32 and dgamma.is_cuda and dbeta.is_cuda
    assert dgamma.stride(1) == 1 and dbeta.stride(1) == 1 and dgamma.stride(0) == dbeta.stride(0)
    assert (accum_gamma is None) == (accum_beta is None)
    accumulate = accum_gamma is not None
    if accumulate:
        og, ob = accum_gamma, accum_beta
        assert all(t.is_contiguous() and t.dtype == torch.float32 and t.numel() == c and t.is_cuda for t in (og, ob))
    else:
        og, ob = (torch.empty(c, dtype=torch.float32, device=dgamma.device) for _ in range(2))
    check(_lib.lib().lp_norm_affine_grad(dgamma.data_ptr(), dbeta.data_ptr(), dgamma.stride(0), og.data_ptr(), ob.data_ptr(), n, c, int(accumulate),
                                         _stream()), 'lp_norm_affine_grad')
    return (None, None) if accumulate else (og, ob)


def stickman_table(parts=PARTS):
    """polyline table of lp_stickman_render from ``parts`` = ((first point, last point, closed, RGB colour), ...) -> (seg [L][2] point indices with the
    segments of one part consecutive and a closed part's closing edge last, part_end [parts] exclusive ends of the runs, colour [parts][3], number of
    points the table names); host lists, checked here: non-empty runs, indices >= 0, the kernel's limits of 256 segments and 16 parts"""
    seg, part_end, colour = [], [], []
    for first, last, closed, rgb in parts:
        idx = list(range(int(first), int(last) + 1))
        pairs = list(zip(idx[:-1], idx[1:])) + ([(idx[-1], idx[0])] if closed else [])
        if first < 0 or not pairs:
            raise ValueError(f'stickman part ({first}, {last}, closed={closed}) has no segment or a negative point index')
        if len(rgb) != 3:
            raise ValueError(f'stickman part ({first}, {last}): the colour must be an RGB triple, got {rgb}')
        seg += [list(p) for p in pairs]
        part_end.append(len(seg))
        colour.append([float(c) for c in rgb])
    if not 1 <= len(part_end) <= 16 or len(seg) > 256:
        raise ValueError(f'stickman table with {len(part_end)} parts and {len(seg)} segments: 1 .. 16 parts and at most 256 segments are supported')
    assert part_end[-1] == len(seg)
    return seg, part_end, colour, 1 + max(max(p) for p in seg)


_STICKMAN_TABLES = {}


def _stickman_device_table(parts, device):
    """``stickman_table`` on ``device``, built once per (parts, device): three small tensors that every later launch (and graph replay) reads"""
    parts = tuple((int(f), int(l), bool(c), tuple(float(v) for v in rgb)) for f, l, c, rgb in parts)
    key = (parts, device)
    tab = _STICKMAN_TABLES.get(key)
    if tab is None:
        seg, part_end, colour, npoints = stickman_table(parts)
        tab = (torch.tensor(seg, dtype=torch.int32).to(device), torch.tensor(part_end, dtype=torch.int32).to(device),
               torch.tensor(colour, dtype=torch.float32).to(device), len(seg), len(part_end), npoints)
        _STICKMAN_TABLES[key] = tab
    return tab


def stickman_render(points: Tensor, size: int, width: Optional[float] = None, out: Optional[Tensor] = None, parts=PARTS) -> Tensor:
    """keypoints [..., P, 2] or [..., 2P] ((x, y) pairs in [0, 1]; fp32, on the GPU) -> stickmen [..., 3, S, S]: ``draw_stickman`` of
    dataloaders/synthetic_voxceleb2_stickmen.py as ONE launch on the current stream (lp_stickman_render).  ``width`` defaults to max(1, S / 64).
    ``out``: a contiguous fp32 tensor of the result's shape to write into -- it may be a view of a larger tensor.  Points are neither clamped nor
    checked (that would need a host sync), as on the host."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise ValueError('stickman_render: the keypoints must be a CUDA tensor (the stickman is rendered on the MI355X; the host renderer is '
                         'dataloaders.synthetic_voxceleb2_stickmen.draw_stickman)')
    if points.dtype != torch.float32:
        raise ValueError(f'stickman_render: fp32 keypoints are required, got {points.dtype}')
    size = int(size)
    if size < 1:
        raise ValueError(f'stickman_render: size must be >= 1, got {size}')
    width = max(1.0, size / 64.0) if width is None else float(width)
    if not width > 0:
        raise ValueError(f'stickman_render: width must be > 0, got {width}')
    seg, part_end, colour, nseg, nparts, npoints = _stickman_device_table(parts, points.device)
    if points.dim() >= 2 and points.shape[-1] == 2 and points.shape[-2] >= npoints:
        lead, p = tuple(points.shape[:-2]), points.shape[-2]
    elif points.dim() >= 1 and points.shape[-1] % 2 == 0 and points.shape[-1] // 2 >= npoints:
        lead, p = tuple(points.shape[:-1]), points.shape[-1] // 2
    else:
        raise ValueError(f'stickman_render: keypoints {tuple(points.shape)}: expected [..., P, 2] or [..., 2P] with P >= {npoints}, the points the '
                         'polyline table names')
    if p > 256:
        raise ValueError(f'stickman_render: at most 256 keypoints per image are supported, got {p}')
    n = 1
    for d in lead:
        n *= d
    shape = lead + (3, size, size)
    if n < 1:
        raise ValueError(f'stickman_render: keypoints {tuple(points.shape)} hold no image')
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=points.device)
    elif not (isinstance(out, torch.Tensor) and out.device == points.device and out.dtype == torch.float32 and tuple(out.shape) == shape
              and out.is_contiguous()):
        raise ValueError(f'stickman_render: out must be a contiguous fp32 tensor of shape {shape} on {points.device}, got '
                         f'{tuple(out.shape)} {out.dtype} {out.device} contiguous={out.is_contiguous()}')
    pts = points.detach().contiguous()
    check(_lib.lib().lp_stickman_render(pts.data_ptr(), n, p, seg.data_ptr(), part_end.data_ptr(), colour.data_ptr(), nseg, nparts, size, width,
                                        out.data_ptr(), _stream()), 'lp_stickman_render')
    return out


HARD_POINT_MIN, HARD_POINT_MAX = -4096, 8191          # the clamp of the hard stickman's integer points (csrc/stickman_hard.hip)
HARD_MAX_SIZE, HARD_MAX_THICKNESS = 4096, 8


def _hard_arguments(name, points, size, thickness, parts):
    """the checks ``stickman_render_hard`` and its host twin share -> (size, thickness, polyline table as host lists, leading shape, P)"""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise ValueError(f'{name}: fp32 keypoints are required, got {points.dtype if isinstance(points, torch.Tensor) else type(points).__name__}')
    size, thickness = int(size), int(thickness)
    if not 1 <= size <= HARD_MAX_SIZE:
        raise ValueError(f'{name}: size must be in 1 .. {HARD_MAX_SIZE}, got {size}')
    if not 1 <= thickness <= HARD_MAX_THICKNESS:
        raise ValueError(f'{name}: thickness must be in 1 .. {HARD_MAX_THICKNESS}, got {thickness}')
    table = stickman_table(parts)
    npoints = table[3]
    if points.dim() >= 2 and points.shape[-1] == 2 and points.shape[-2] >= npoints:
        lead, p = tuple(points.shape[:-2]), points.shape[-2]
    elif points.dim() >= 1 and points.shape[-1] % 2 == 0 and points.shape[-1] // 2 >= npoints:
        lead, p = tuple(points.shape[:-1]), points.shape[-1] // 2
    else:
        raise ValueError(f'{name}: keypoints {tuple(points.shape)}: expected [..., P, 2] or [..., 2P] with P >= {npoints}, the points the polyline '
                         'table names')
    if p > 256:
        raise ValueError(f'{name}: at most 256 keypoints per image are supported, got {p}')
    n = 1
    for d in lead:
        n *= d
    if n < 1:
        raise ValueError(f'{name}: keypoints {tuple(points.shape)} hold no image')
    return size, thickness, table, lead, p, n


def _hard_out(name, out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not isinstance(out, torch.Tensor):
        raise ValueError(f'{name}: out must be a tensor, got {type(out).__name__}')
    if not (out.device == device and out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous()):
        raise ValueError(f'{name}: out must be a contiguous fp32 tensor of shape {shape} on {device}, got '
                         f'{tuple(out.shape)} {out.dtype} {out.device} contiguous={out.is_contiguous()}')
    return out


def stickman_render_hard(points: Tensor, size: int, thickness: int = 2, out: Optional[Tensor] = None, parts=REFERENCE_PARTS) -> Tensor:
    """keypoints [..., P, 2] or [..., 2P] ((x, y) pairs in [0, 1]; fp32, on the GPU) -> stickmen [..., 3, S, S], fp32: the reference's
    ``draw_stickman`` (cv2.polylines of ``thickness`` on rounded integer keypoints, later parts over earlier ones) by the exact-integer definition in
    the header of csrc/stickman_hard.hip, as ONE launch on the current stream (lp_stickman_render_hard).  ``parts`` defaults to the reference's
    topology with the face oval (``REFERENCE_PARTS``; ``REFERENCE_PARTS_NO_OVAL`` without).  ``out``: a contiguous fp32 tensor of the result's shape
    to write into -- it may be a view of a larger tensor.  Points are clamped by the definition, never checked (no host sync); CPU tensors:
    ``stickman_render_hard_host``."""
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise ValueError('stickman_render_hard: the keypoints must be a CUDA tensor (the stickman is rendered on the MI355X; for CPU tensors call '
                         'stickman_render_hard_host)')
    size, thickness, _, lead, p, n = _hard_arguments('stickman_render_hard', points, size, thickness, parts)
    seg, part_end, colour, nseg, nparts, _ = _stickman_device_table(parts, points.device)
    out = _hard_out('stickman_render_hard', out, lead + (3, size, size), points.device)
    pts = points.detach().contiguous()
    check(_lib.lib().lp_stickman_render_hard(pts.data_ptr(), n, p, seg.data_ptr(), part_end.data_ptr(), colour.data_ptr(), nseg, nparts, size,
                                             thickness, out.data_ptr(), _stream()), 'lp_stickman_render_hard')
    return out


def stickman_render_hard_host(points: Tensor, size: int, thickness: int = 2, out: Optional[Tensor] = None, parts=REFERENCE_PARTS) -> Tensor:
    """``stickman_render_hard`` for CPU tensors: the same definition in numpy integer operations (int64 throughout), bit-identical to the kernel"""
    import numpy as np
    if not isinstance(points, torch.Tensor) or points.is_cuda:
        raise ValueError('stickman_render_hard_host: the keypoints must be a CPU tensor (on the GPU call stickman_render_hard)')
    size, thickness, (seg, part_end, colour, _), lead, p, n = _hard_arguments('stickman_render_hard_host', points, size, thickness, parts)
    out = _hard_out('stickman_render_hard_host', out, lead + (3, size, size), points.device)
    x = points.detach().contiguous().reshape(n, p, 2).numpy()
    with np.errstate(invalid='ignore', over='ignore'):
        r = (x * np.float32(size)).round()          # the fp32 product, rounded half to even
        r = np.where(r >= np.float32(HARD_POINT_MIN), np.minimum(r, np.float32(HARD_POINT_MAX)), np.float32(HARD_POINT_MIN))          # NaN -> lower bound
    pts = r.astype(np.int64)
    v, u = np.meshgrid(np.arange(size, dtype=np.int64), np.arange(size, dtype=np.int64), indexing='ij')          # v: row, u: column
    t2 = thickness * thickness
    hit = np.full((n, size, size), -1, dtype=np.int64)
    start = 0
    for part, end in enumerate(part_end):
        for i, j in seg[start:end]:
            a, b = pts[:, i, :, None, None], pts[:, j, :, None, None]          # [n, 2, 1, 1]
            dx, dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
            ex, ey = u[None] - a[:, 0], v[None] - a[:, 1]
            fx, fy = u[None] - b[:, 0], v[None] - b[:, 1]
            l2, s = dx * dx + dy * dy, ex * dx + ey * dy
            cross = dx * ey - dy * ex
            covered = np.where(s <= 0, 4 * (ex * ex + ey * ey) <= t2, np.where(s >= l2, 4 * (fx * fx + fy * fy) <= t2, 4 * cross * cross <= t2 * l2))
            hit[covered] = part
        start = end
    table = np.concatenate([np.asarray(colour, dtype=np.float32).reshape(-1, 3), np.zeros((1, 3), dtype=np.float32)])          # (-1: no part -> 0)
    img = np.ascontiguousarray(table[hit].transpose(0, 3, 1, 2))
    out.copy_(torch.from_numpy(img).reshape(out.shape))
    return out


IMAGE_QUALITY_COLUMNS =('ssim', 'psnr', 'l1', 'ssim_fg', 'psnr_fg', 'l1_fg')


def image_quality(x: Tensor, y: Tensor, mask: Optional[Tensor] = None) -> Tensor:
    """image-quality table [B, 6] (``IMAGE_QUALITY_COLUMNS``; fp32, on the device) of ``x`` [B, C, H, W] against ``y`` [B, C, H, W] or [B, K, C, H, W]
    (its frame 0 is taken), both clamped to [0, 1]: SSIM (11-tap Gaussian window, valid positions), PSNR and L1 over the whole frame and weighted by
    ``mask`` [B, H, W] (the ``_fg`` columns: NaN without a mask or where the weights sum to 0) -- the definition is the header comment of
    csrc/image_quality.hip.  One launch plus its fixed-order finish launch on the current stream (lp_image_quality), bit-reproducible.  All three
    tensors are read in place through their strides: a ``[:, 0]`` view of the images or an ``expand``ed mask is never materialised.  No gradient."""
    for name, t in (('x', x), ('y', y)) + ((('mask', mask),) if mask is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'image_quality: {name} must be a tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise ValueError(f'image_quality: {name} must be fp32, got {t.dtype}')
    if y.dim() == 5:
        y = y[:, 0]
    if x.dim() != 4 or y.dim() != 4:
        raise ValueError(f'image_quality: expected x [B, C, H, W] and y [B, C, H, W] or [B, K, C, H, W], got {tuple(x.shape)} and {tuple(y.shape)}')
    if x.shape != y.shape:
        raise ValueError(f'image_quality: shape mismatch between x {tuple(x.shape)} and y {tuple(y.shape)}')
    b, c, h, w = x.shape
    if mask is not None and tuple(mask.shape) != (b, h, w):
        raise ValueError(f'image_quality: shape mismatch between the mask {tuple(mask.shape)} and the images: expected {(b, h, w)}')
    if b < 1 or c < 1:
        raise ValueError(f'image_quality: empty batch {tuple(x.shape)}')
    if h < 11 or w < 11:
        raise ValueError(f'image_quality: H and W must be >= 11 (one 11 x 11 SSIM window), got {h} x {w}')
    if c > 4:
        raise ValueError(f'image_quality: at most 4 channels are supported, got C = {c}')
    for name, t in (('x', x), ('y', y)) + ((('mask', mask),) if mask is not None else ()):
        if not t.is_cuda or t.device != x.device:
            raise ValueError(f'image_quality: {name} is on {t.device}: all inputs must be CUDA tensors on one device (the table is computed on the MI355X)')
    import ctypes
    x, y = x.detach(), y.detach()
    sx, sy = (ctypes.c_longlong * 4)(*x.stride()), (ctypes.c_longlong * 4)(*y.stride())
    sm = None
    if mask is not None:
        mask = mask.detach()
        sm = (ctypes.c_longlong * 3)(*mask.stride())
    l = _lib.lib()
    work = torch.empty(l.lp_image_quality_workspace_bytes(b, h, w) // 4, dtype=torch.float32, device=x.device)
    out = torch.empty((b, 6), dtype=torch.float32, device=x.device)
    npix = b * h * w
    with _Timed('image_quality', 2.0 * 110 * c * npix, (b, h, w, c, 6, 11, 0, int(mask is not None)), (4 * npix * (2 * c + int(mask is not None)), 24 * b)):
        check(l.lp_image_quality(x.data_ptr(), ctypes.addressof(sx), y.data_ptr(), ctypes.addressof(sy), _p(mask),
                                 None if sm is None else ctypes.addressof(sm), b, c, h, w, work.data_ptr(), out.data_ptr(), _stream()), 'lp_image_quality')
    return out


AUG_COLUMNS = ('pose_a00', 'pose_a01', 'pose_a02', 'pose_a10', 'pose_a11', 'pose_a12',
               'target_a00', 'target_a01', 'target_a02', 'target_a10', 'target_a11', 'target_a12',
               'k00', 'k01', 'k02', 'k10', 'k11', 'k12', 'k20', 'k21', 'k22',
               'mul', 'add_r', 'add_g', 'add_b', 'alpha', 'gain', 'sigma', 'seed', 'reserved0', 'reserved1', 'reserved2')


def _aug_frame(name: str, t: Tensor):
    """[B, C, H, W] or [B, 1, C, H, W] -> (the 4-D view, was it 5-D)"""
    if t.dim() == 5 and t.shape[1] == 1:
        return t[:, 0], True
    if t.dim() != 4:
        raise ValueError(f'augment_triplet: {name} must be [B, C, H, W] or [B, 1, C, H, W], got shape {tuple(t.shape)}')
    return t, False


def augment_triplet(pose: Tensor, params: Tensor, target: Optional[Tensor] = None, segm: Optional[Tensor] = None):
    """(pose', target', segm') of the augmentation defined in the header comment of csrc/augment.hip: ``params`` [B, 32] (``AUG_COLUMNS``) holds per
    sample the inverse affine maps, the 3 x 3 filter and the pixelwise parameters.  ``pose`` / ``target``: [B, C, H, W] or [B, 1, C, H, W] of one
    shape, ``segm``: the same with its own channel count (at most 4 channels each); every result has its input's shape, an absent input gives None.
    ONE launch on the current stream (lp_augment_triplet), bit-reproducible; the inputs are read in place through their strides -- a ``[:, 0]``
    view or an ``expand``ed mask is never materialised.  No gradient."""
    given = [('pose', pose), ('params', params)] + ([('target', target)] if target is not None else []) + ([('segm', segm)] if segm is not None else [])
    for name, t in given:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'augment_triplet: {name} must be a tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise ValueError(f'augment_triplet: {name} must be fp32, got {t.dtype}')
    p4, p5 = _aug_frame('pose', pose)
    b, c, h, w = p4.shape
    t4 = s4 = None
    if target is not None:
        t4, t5 = _aug_frame('target', target)
        if t4.shape != p4.shape:
            raise ValueError(f'augment_triplet: shape mismatch between pose {tuple(pose.shape)} and target {tuple(target.shape)}')
    if segm is not None:
        s4, s5 = _aug_frame('segm', segm)
        if (s4.shape[0], s4.shape[2], s4.shape[3]) != (b, h, w):
            raise ValueError(f'augment_triplet: shape mismatch between pose {tuple(pose.shape)} and segm {tuple(segm.shape)}')
    if tuple(params.shape) != (b, len(AUG_COLUMNS)):
        raise ValueError(f'augment_triplet: params must be [B, 32] = {(b, len(AUG_COLUMNS))}, got {tuple(params.shape)}')
    if b < 1 or c < 1 or h < 1 or w < 1 or (s4 is not None and s4.shape[1] < 1):
        raise ValueError(f'augment_triplet: empty input {tuple(pose.shape)}')
    if c > 4 or (s4 is not None and s4.shape[1] > 4):
        raise ValueError(f'augment_triplet: at most 4 channels are supported, got C = {c}' + ('' if s4 is None else f', Cs = {s4.shape[1]}'))
    for name, t in given:
        if not t.is_cuda:
            raise ValueError(f'augment_triplet: {name} is on {t.device}: all inputs must be CUDA tensors (the host version is '
                             'augmentation.augment_triplet_host)')
        if t.device != pose.device:
            raise ValueError(f'augment_triplet: mixed devices: {name} is on {t.device}, pose on {pose.device}')
    import ctypes
    cs = 1 if s4 is None else s4.shape[1]
    par = params.detach().contiguous()
    srcs = [t if t is None else t.detach() for t in (p4, t4, s4)]
    strides = [None if t is None else (ctypes.c_longlong * 4)(*t.stride()) for t in srcs]
    outs = [None if t is None else torch.empty(t.shape, dtype=torch.float32, device=pose.device) for t in srcs]
    npix = b * h * w
    chans = c * (1 + int(t4 is not None)) + (cs if s4 is not None else 0)
    with _Timed('augment', 2.0 * npix * (9 * c + 8 * chans), (b, h, w, c, cs, 3, int(t4 is not None), int(s4 is not None)),
                (4 * npix * chans + 128 * b, 4 * npix * chans)):
        check(_lib.lib().lp_augment_triplet(_p(srcs[0]), ctypes.addressof(strides[0]),
                                            _p(srcs[1]), None if strides[1] is None else ctypes.addressof(strides[1]),
                                            _p(srcs[2]), None if strides[2] is None else ctypes.addressof(strides[2]),
                                            par.data_ptr(), b, c, cs, h, w, _p(outs[0]), _p(outs[1]), _p(outs[2]), _stream()), 'lp_augment_triplet')
    return (outs[0].unsqueeze(1) if p5 else outs[0],
            None if t4 is None else (outs[1].unsqueeze(1) if t5 else outs[1]),
            None if s4 is None else (outs[2].unsqueeze(1) if s5 else outs[2]))


AUG_EXTRA_COLUMNS = ('elastic_alpha', 'elastic_seed', 'median', 'saturation', 'jpeg_quality') + tuple(f'reserved{i}' for i in range(11))


def augment_extra(pose: Tensor, params_extra: Tensor, out: Optional[Tensor] = None):
    """pose' of the second augmentation stage defined in the header comment of csrc/augment_extra.hip: ``params_extra`` [B, 16]
    (``AUG_EXTRA_COLUMNS``) holds per sample the elastic amplitude and seed, the median switch, the saturation offset and the JPEG quality; the
    all-zero row returns an input in [0, 1] bit for bit.  ``pose``: [B, 3, H, W] or [B, 1, 3, H, W], read in place through its strides (a ``[:, 0]``
    view is never materialised); the result has its shape.  ``out``: a contiguous fp32 tensor of that shape on the same device, not sharing storage
    with ``pose`` (a slice of a larger buffer is fine), written and returned; None allocates.  ONE launch on the current stream
    (lp_augment_extra), bit-reproducible.  No gradient."""
    for name, t in (('pose', pose), ('params_extra', params_extra)) + ((('out', out),) if out is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'augment_extra: {name} must be a tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise ValueError(f'augment_extra: {name} must be fp32, got {t.dtype}')
    if pose.dim() == 5 and pose.shape[1] == 1:
        p4 = pose[:, 0]
    elif pose.dim() == 4:
        p4 = pose
    else:
        raise ValueError(f'augment_extra: pose must be [B, 3, H, W] or [B, 1, 3, H, W], got shape {tuple(pose.shape)}')
    b, c, h, w = p4.shape
    if c != 3:
        raise ValueError(f'augment_extra: pose must have 3 channels (saturation and JPEG are defined on RGB), got C = {c}')
    if tuple(params_extra.shape) != (b, len(AUG_EXTRA_COLUMNS)):
        raise ValueError(f'augment_extra: params_extra must be [B, 16] = {(b, len(AUG_EXTRA_COLUMNS))}, got {tuple(params_extra.shape)}')
    if b < 1 or h < 1 or w < 1:
        raise ValueError(f'augment_extra: empty input {tuple(pose.shape)}')
    if b > 65535 or (h + 15) // 16 > 65535:
        raise ValueError(f'augment_extra: B = {b} or H = {h} exceeds one launch grid (at most 65535 images and 65535 tiles of 16 rows)')
    if out is not None:
        if tuple(out.shape) != tuple(pose.shape):
            raise ValueError(f'augment_extra: shape mismatch between pose {tuple(pose.shape)} and out {tuple(out.shape)}')
        if not out.is_contiguous():
            raise ValueError('augment_extra: out must be contiguous')
    for name, t in (('pose', pose), ('params_extra', params_extra)) + ((('out', out),) if out is not None else ()):
        if not t.is_cuda:
            raise ValueError(f'augment_extra: {name} is on {t.device}: all tensors must be CUDA tensors (the host version is '
                             'augmentation.augment_extra_host)')
        if t.device != pose.device:
            raise ValueError(f'augment_extra: mixed devices: {name} is on {t.device}, pose on {pose.device}')
    if out is not None and out.untyped_storage().data_ptr() == pose.untyped_storage().data_ptr():
        raise ValueError('augment_extra: out shares its storage with pose (elastic and median read neighbouring tiles: not an in-place operation)')
    import ctypes
    p4 = p4.detach()
    par = params_extra.detach().contiguous()
    strides = (ctypes.c_longlong * 4)(*p4.stride())
    res = torch.empty(pose.shape, dtype=torch.float32, device=pose.device) if out is None else out
    npix = b * h * w
    with _Timed('augment_extra', 2.0 * npix * 3 * (12 + 32), (b, h, w, c, 16), (4 * npix * 3 + 64 * b, 4 * npix * 3)):
        check(_lib.lib().lp_augment_extra(p4.data_ptr(), ctypes.addressof(strides), par.data_ptr(), b, c, h, w, res.data_ptr(), _stream()),
              'lp_augment_extra')
    return res


def frames_prepare(buf: Tensor, table: Tensor, size: int):
    """(image, mask, product) of the frame preparation defined in the header comment of csrc/frames.hip: ``buf`` = the decoded uint8 frames of a
    batch, packed, on the device; ``table`` = int64 [R, 24] (``frames.COLUMNS``) on the HOST, one row per output image: an image view with its box
    and mode, a mask view with its box, and the slot of each output.  Every result is fp32 [slots, 3, size, size], None where no row asks for it.
    The table is checked here (ValueError naming the row: a box that is not square, a view outside ``buf``, a scale above 8) and copied to the
    device; then ONE launch on the current stream (lp_frames_prepare), bit-reproducible.  No gradient."""
    from latent_pose_reenactment_amd import frames
    if not (isinstance(buf, torch.Tensor) and buf.dtype == torch.uint8 and buf.dim() == 1):
        raise ValueError('frames_prepare: buf must be a 1-D uint8 tensor')
    if not buf.is_cuda:
        raise ValueError(f'frames_prepare: buf is on {buf.device}: it must be a CUDA tensor (the host version is frames.prepare_host)')
    size = int(size)
    counts = frames.check_table(table, buf.numel(), size)
    buf, table = buf.contiguous(), table.contiguous()
    with torch.cuda.device(buf.device):
        table_dev = (table if table.is_pinned() else table.pin_memory()).to(buf.device, non_blocking=True)
        outs = [torch.empty((c, 3, size, size), dtype=torch.float32, device=buf.device) if c else None for c in counts]
        check(_lib.lib().lp_frames_prepare(buf.data_ptr(), buf.numel(), table.data_ptr(), table_dev.data_ptr(), table.shape[0], size,
                                           _p(outs[0]), counts[0], _p(outs[1]), counts[1], _p(outs[2]), counts[2], _stream()), 'lp_frames_prepare')
    return tuple(outs)


def frames_pad(buf: Tensor, nbytes: int, plan: Tensor, weights: Tensor):
    """fills the workspace images of a ``frames.pad_plan`` in place (the definition: the header comment of csrc/frames_pad.hip) and returns ``buf``:
    ``buf`` = uint8 on the device, at least the plan's total size, its first ``nbytes`` the packed frames; ``plan`` int64 [P, 16] and ``weights``
    fp32 [P, 100] on the HOST.  Each plan row's crop through the border rule, blurred in the padded bands, faded to the median colour (a mask: to 0)
    and rounded, is written as a dense uint8 [n, n, C] image at its ``ws_off``; no other byte of ``buf`` changes.  The plan is checked here
    (ValueError naming the plan row: a view outside the head, pads or k the box does not give, a workspace image outside the tail, a crop above 1024);
    then a clear and three launches on the current stream (lp_frames_pad), bit-reproducible.  No gradient."""
    from latent_pose_reenactment_amd import frames
    if not (isinstance(buf, torch.Tensor) and buf.dtype == torch.uint8 and buf.dim() == 1 and buf.is_contiguous()):
        raise ValueError('frames_pad: buf must be a contiguous 1-D uint8 tensor')
    if not buf.is_cuda:
        raise ValueError(f'frames_pad: buf is on {buf.device}: it must be a CUDA tensor (the host version is frames.pad_host)')
    nbytes = int(nbytes)
    frames.check_plan(plan, weights, nbytes, buf.numel())
    plan, weights = plan.contiguous(), weights.contiguous()
    plans = plan.shape[0]
    with torch.cuda.device(buf.device):
        plan_dev = (plan if plan.is_pinned() else plan.pin_memory()).to(buf.device, non_blocking=True)
        weights_dev = (weights if weights.is_pinned() else weights.pin_memory()).to(buf.device, non_blocking=True)
        hist = torch.empty(plans * 768, dtype=torch.int32, device=buf.device)
        median = torch.empty(plans * 3, dtype=torch.float32, device=buf.device)
        check(_lib.lib().lp_frames_pad(buf.data_ptr(), buf.numel(), nbytes, plan.data_ptr(), plan_dev.data_ptr(), plans, weights_dev.data_ptr(),
                                       hist.data_ptr(), median.data_ptr(), _stream()), 'lp_frames_pad')
    return buf


VISUAL_SHEET_MAX_PANELS = 12


def _visual_sheet_check(panels, caption, out):
    """the argument rules of ``visual_sheet`` / ``visual_sheet_host`` (no device call) -> (panels as a list, N, H, W, Hc)"""
    if isinstance(panels, torch.Tensor) or not hasattr(panels, '__len__'):
        raise ValueError(f'visual_sheet: panels must be a sequence of 4-D fp32 tensors, got {type(panels).__name__}')
    panels = list(panels)
    if not 1 <= len(panels) <= VISUAL_SHEET_MAX_PANELS:
        raise ValueError(f'visual_sheet: 1 .. {VISUAL_SHEET_MAX_PANELS} panels are supported, got {len(panels)} (more than 12 panels do not fit one launch)'
                         if panels else 'visual_sheet: 1 .. 12 panels are supported, got 0')
    for i, t in enumerate(panels):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'visual_sheet: panel {i} must be a tensor, got {type(t).__name__}')
        if t.dtype != torch.float32:
            raise ValueError(f'visual_sheet: panel {i} must be fp32, got {t.dtype}')
        if t.dim() != 4:
            raise ValueError(f'visual_sheet: panel {i} must be 4-D [N, C, H, W], got shape {tuple(t.shape)}')
        if t.shape[1] not in (1, 3):
            raise ValueError(f'visual_sheet: panel {i} must have 1 or 3 channels, got C = {t.shape[1]}')
        if (t.shape[0], t.shape[2], t.shape[3]) != (panels[0].shape[0], panels[0].shape[2], panels[0].shape[3]):
            raise ValueError(f'visual_sheet: shape mismatch between panel 0 {tuple(panels[0].shape)} and panel {i} {tuple(t.shape)}: N, H and W are shared')
        if t.device != panels[0].device:
            raise ValueError(f'visual_sheet: panel {i} is on {t.device}, panel 0 on {panels[0].device}: '
                             + ('it is not on the GPU' if not t.is_cuda else 'all panels must be on one device'))
    n, _, h, w = panels[0].shape
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f'visual_sheet: empty panels {tuple(panels[0].shape)}')
    hc = 0
    if caption is not None:
        if not (isinstance(caption, torch.Tensor) and caption.dtype == torch.uint8 and caption.dim() == 2 and caption.shape[1] == len(panels) * w):
            raise ValueError(f'visual_sheet: the caption strip must be uint8 [Hc, P * W] = [Hc, {len(panels) * w}], got '
                             + (f'{tuple(caption.shape)} {caption.dtype}' if isinstance(caption, torch.Tensor) else type(caption).__name__))
        if caption.device != panels[0].device:
            raise ValueError(f'visual_sheet: the caption strip is on {caption.device}, the panels on {panels[0].device}')
        hc = caption.shape[0]
    if out is not None:
        shape = (hc + n * h, len(panels) * w, 3)
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and tuple(out.shape) == shape and out.is_contiguous()
                and out.device == panels[0].device):
            raise ValueError(f'visual_sheet: out must be a contiguous uint8 tensor of shape {shape} on {panels[0].device}')
    return panels, n, h, w, hc


def visual_sheet_host(panels, caption: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``visual_sheet`` in torch ops on the panels' own device -- the definition of csrc/visual_sheet.hip step for step: NaN -> 0, clamp to [0, 1],
    times 255 in fp32, truncated to uint8; a one-channel panel in all three channels; samples below each other, panels side by side, the strip on top"""
    panels, n, h, w, hc = _visual_sheet_check(panels, caption, out)
    cols = []
    for t in panels:
        q = t.detach().nan_to_num(nan=0.0).clamp(0, 1).mul(255).to(torch.uint8)          # (+-inf become the largest floats: the clamp's bounds)
        cols.append(q.expand(n, 3, h, w).permute(0, 2, 3, 1).reshape(n * h, w, 3))
    sheet = torch.cat(cols, dim=1)
    if hc:
        sheet = torch.cat((caption[:, :, None].expand(hc, caption.shape[1], 3), sheet), dim=0)
    if out is not None:
        return out.copy_(sheet)
    return sheet.contiguous()


def visual_sheet(panels, caption: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """uint8 sheet [Hc + N H, P W, 3] (HWC, on the panels' device) of ``panels``, a sequence of 1 .. 12 fp32 tensors or views [N, C, H, W] with C in
    {1, 3} and N, H, W shared: sample n in rows Hc + n H ..., panel p in columns p W ..., every value (uint8) floor(clamp(x, 0, 1) * 255), NaN -> 0
    (the header comment of csrc/visual_sheet.hip); ``caption``: uint8 [Hc, P W] greys put on top.  Panels on the GPU: ONE launch on the current stream
    (lp_visual_sheet), every panel read in place through its strides -- a ``[:n, 0]`` view of a batch tensor or an ``expand``ed mask is never
    materialised; CPU panels: ``visual_sheet_host``.  ``out``: a contiguous uint8 tensor of the result's shape to write into.  No gradient."""
    panels, n, h, w, hc = _visual_sheet_check(panels, caption, out)
    if not panels[0].is_cuda:
        return visual_sheet_host(panels, caption, out)
    import ctypes
    count = len(panels)
    panels = [t.detach() for t in panels]
    ptrs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in panels])
    strides = (ctypes.c_longlong * (4 * count))(*[s for t in panels for s in t.stride()])
    chans = (ctypes.c_int * count)(*[t.shape[1] for t in panels])
    if caption is not None:
        caption = caption.contiguous()
    with torch.cuda.device(panels[0].device):
        if out is None:
            out = torch.empty((hc + n * h, count * w, 3), dtype=torch.uint8, device=panels[0].device)
        check(_lib.lib().lp_visual_sheet(ctypes.addressof(ptrs), ctypes.addressof(strides), ctypes.addressof(chans), count, n, h, w, _p(caption), hc,
                                         out.data_ptr(), _stream()), 'lp_visual_sheet')
    return out


# ---- baseline JPEG of the drive output (csrc/jpeg.hip holds the definition) ------------------------------------------------------------------------
def _jpeg_refusal(rc, what):
    """the C ABI's refusals of an argument (checked before any device work) surface as ValueError; anything else as LpError"""
    if rc in (-1, -2):
        msg = _lib.lib().lp_last_error()
        raise ValueError(msg.decode() if msg else what)
    check(rc, what)


def _jpeg_frames(frames, who):
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f'{who}: frames must be a tensor, got {type(frames).__name__}')
    if frames.dtype != torch.uint8:
        raise ValueError(f'{who}: frames must be uint8, got {frames.dtype}')
    if frames.dim() != 4:
        raise ValueError(f'{who}: frames must be 4-D [T, H, W, 3], got shape {tuple(frames.shape)}')
    if frames.shape[3] != 3:
        raise ValueError(f'{who}: frames must be RGB [T, H, W, 3], got C = {frames.shape[3]}')
    t, h, w, _ = frames.shape
    if t < 1 or h < 1 or w < 1:
        raise ValueError(f'{who}: empty input {tuple(frames.shape)}: T, H and W must be >= 1')
    if h > 65535 or w > 65535:
        raise ValueError(f'{who}: H and W must be <= 65535 (a JPEG frame header holds them in 16 bits), got {h} x {w}')
    return t, h, w


def _jpeg_coefs(coefs, who):
    if not (isinstance(coefs, torch.Tensor) and coefs.dtype == torch.int16 and coefs.dim() == 5 and tuple(coefs.shape[3:]) == (3, 64)):
        raise ValueError(f'{who}: coefs must be an int16 tensor [T, rows, mcus, 3, 64], got '
                         f'{(coefs.dtype, tuple(coefs.shape)) if isinstance(coefs, torch.Tensor) else type(coefs).__name__}')
    t, rows, mcus = coefs.shape[:3]
    if t < 1 or rows < 1 or mcus < 1:
        raise ValueError(f'{who}: empty coefficient table {tuple(coefs.shape)}')
    return t, rows, mcus


def jpeg_transform_host(frames: Tensor, quality: int = 90) -> Tensor:
    """the quantised coefficients of csrc/jpeg.hip in torch ops on the frames' own device: int16 [T, rows, mcus, 3, 64] in zigzag order"""
    from .utils import mjpeg
    t, h, w = _jpeg_frames(frames, 'jpeg_transform_host')
    rows, mcus = (h + 7) // 8, (w + 7) // 8
    dev = frames.device
    q = torch.from_numpy(mjpeg.quant_tables(quality).astype('float32')).to(dev)[[0, 1, 1]]          # [3, 64]
    ys = torch.arange(8 * rows, device=dev).clamp(max=h - 1)
    xs = torch.arange(8 * mcus, device=dev).clamp(max=w - 1)
    rgb = frames.detach()[:, ys][:, :, xs].to(torch.float32)
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    planes = torch.stack((0.299 * R + 0.587 * G + 0.114 * B - 128.0, -0.168736 * R - 0.331264 * G + 0.5 * B,
                          0.5 * R - 0.418688 * G - 0.081312 * B), dim=1)                                 # [T, 3, 8 rows, 8 mcus]
    k = torch.arange(8, dtype=torch.float64)
    basis = torch.cos((2 * k[None, :] + 1) * k[:, None] * torch.pi / 16) * 0.5
    basis[0] = 0.125 ** 0.5
    basis = basis.to(torch.float32).to(dev)
    x = planes.reshape(t, 3, rows, 8, mcus, 8)
    d = torch.einsum('vn,tcrymn->tcrymv', basis, x)                    # rows first
    d = torch.einsum('uy,tcrymv->tcrumv', basis, d)                    # then columns
    d = d.permute(0, 2, 4, 1, 3, 5).reshape(t, rows, mcus, 3, 64)
    kq = torch.round(d / q)                                            # ties to even
    lo = torch.full((64,), -1023.0, device=dev)
    lo[0] = -1024.0
    kq = torch.maximum(torch.minimum(kq, torch.tensor(1023.0, device=dev)), lo)
    return kq[..., list(mjpeg.ZIGZAG)].to(torch.int16).contiguous()


def jpeg_entropy_host(coefs: Tensor, header: bytes):
    """the scan of csrc/jpeg.hip in numpy and Python integers: ``coefs`` int16 [T, rows, mcus, 3, 64] (any values: clamped as the definition
    says) -> (uint8 [total], int64 [T + 1]) on the CPU, every frame = ``header`` + scan + EOI"""
    import numpy as np
    from .utils import mjpeg
    t, rows, mcus = _jpeg_coefs(coefs, 'jpeg_entropy_host')
    c = coefs.detach().cpu().numpy().astype(np.int64)
    c[..., 1:] = np.clip(c[..., 1:], -1023, 1023)
    c[..., 0] = np.clip(c[..., 0], -1024, 1023)
    dc = [mjpeg.huffman_codes(mjpeg.DC_LUMA), mjpeg.huffman_codes(mjpeg.DC_CHROMA)]
    ac = [mjpeg.huffman_codes(mjpeg.AC_LUMA), mjpeg.huffman_codes(mjpeg.AC_CHROMA)]

    def extra(v, size):
        return (v if v >= 0 else v - 1) & ((1 << size) - 1)

    out, offsets = bytearray(), [0]
    for f in range(t):
        out += header
        for r in range(rows):
            acc, nbits, pred = 0, 0, [0, 0, 0]
            for m in range(mcus):
                for comp in range(3):
                    blk, tab = c[f, r, m, comp], int(comp > 0)
                    diff = int(blk[0]) - pred[comp]
                    pred[comp] = int(blk[0])
                    cat = abs(diff).bit_length()
                    code, length = dc[tab][cat]
                    acc, nbits = (((acc << length) | code) << cat) | extra(diff, cat), nbits + length + cat
                    last = 0
                    for k in np.flatnonzero(blk[1:]) + 1:
                        k, v, run = int(k), int(blk[k]), int(k) - last - 1
                        while run >= 16:
                            code, length = ac[tab][0xF0]
                            acc, nbits, run = (acc << length) | code, nbits + length, run - 16
                        size = abs(v).bit_length()
                        code, length = ac[tab][run << 4 | size]
                        acc, nbits = (((acc << length) | code) << size) | extra(v, size), nbits + length + size
                        last = k
                    if last != 63:
                        code, length = ac[tab][0x00]
                        acc, nbits = (acc << length) | code, nbits + length
            pad = -nbits % 8
            acc, nbits = (acc << pad) | ((1 << pad) - 1), nbits + pad
            out += acc.to_bytes(nbits // 8, 'big').replace(b'\xff', b'\xff\x00')
            out += bytes((0xFF, 0xD0 + r % 8)) if r < rows - 1 else b'\xff\xd9'
        offsets.append(len(out))
    return torch.frombuffer(out, dtype=torch.uint8).clone(), torch.tensor(offsets, dtype=torch.int64)


def jpeg_encode_host(frames: Optional[Tensor] = None, quality: int = 90, *, coefs: Optional[Tensor] = None):
    """``jpeg_encode`` in torch and numpy ops, on the CPU.  ``coefs`` (int16 [T, rows, mcus, 3, 64]) in place of ``frames`` encodes a chosen
    coefficient table as frames of 8 rows x 8 mcus pixels (the tests' way to the coder)"""
    from .utils import mjpeg
    quality = mjpeg.check_quality(quality, 'jpeg_encode_host')
    if coefs is None:
        _, h, w = _jpeg_frames(frames, 'jpeg_encode_host')
        coefs = jpeg_transform_host(frames, quality)
    else:
        _, rows, mcus = _jpeg_coefs(coefs, 'jpeg_encode_host')
        h, w = 8 * rows, 8 * mcus
    return jpeg_entropy_host(coefs, mjpeg.jpeg_header(h, w, quality))


def jpeg_transform(frames: Tensor, quality: int = 90) -> Tensor:
    """int16 [T, rows, mcus, 3, 64]: the quantised DCT coefficients of uint8 RGB ``frames`` [T, H, W, 3] in zigzag order (the header comment of
    csrc/jpeg.hip), ``frames`` read in place through its four strides.  The tables come from ``utils.mjpeg.quant_tables(quality)``, the integers of
    the DQT segments.  ONE launch on the current stream (lp_jpeg_transform), no atomics.  CPU frames: ``jpeg_transform_host``."""
    from .utils import mjpeg
    t, h, w = _jpeg_frames(frames, 'jpeg_transform')
    quality = mjpeg.check_quality(quality, 'jpeg_transform')
    if not frames.is_cuda:
        return jpeg_transform_host(frames, quality)
    import ctypes
    frames = frames.detach()
    qt = mjpeg.quant_tables(quality)
    strides = (ctypes.c_longlong * 4)(*frames.stride())
    rows, mcus = (h + 7) // 8, (w + 7) // 8
    with torch.cuda.device(frames.device):
        coefs = torch.empty((t, rows, mcus, 3, 64), dtype=torch.int16, device=frames.device)
        npix = t * rows * mcus * 64
        with _Timed('jpeg_transform', 2.0 * npix * 3 * (5 + 16), (t, h, w), (3 * t * h * w, 6 * npix)):
            _jpeg_refusal(_lib.lib().lp_jpeg_transform(frames.data_ptr(), ctypes.addressof(strides), t, h, w, qt.ctypes.data, coefs.data_ptr(),
                                                       _stream()), 'lp_jpeg_transform')
    return coefs


def jpeg_entropy(coefs: Tensor, header: bytes):
    """(uint8 [total], int64 [T + 1]) on the coefficients' device: every frame of ``coefs`` (int16 [T, rows, mcus, 3, 64], any values) as
    ``header`` + the Huffman-coded scan with its restart markers + EOI, back to back (the header comment of csrc/jpeg.hip).  Four launches
    (lp_jpeg_entropy_size), ONE device-to-host copy of one integer -- the total size --, one launch (lp_jpeg_entropy_write) into an output
    allocated at exactly that size.  Bit-identical from run to run.  CPU coefficients: ``jpeg_entropy_host``."""
    t, rows, mcus = _jpeg_coefs(coefs, 'jpeg_entropy')
    header = bytes(header)
    if not coefs.is_cuda:
        return jpeg_entropy_host(coefs, header)
    l = _lib.lib()
    need = l.lp_jpeg_entropy_scratch_bytes(t, rows, mcus)
    if need < 0:
        _jpeg_refusal(int(need), 'lp_jpeg_entropy_scratch_bytes')
    coefs = coefs.detach().contiguous()
    dev = coefs.device
    with torch.cuda.device(dev):
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        offsets = torch.empty(t + 1, dtype=torch.int64, device=dev)
        head = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(dev, non_blocking=True)
        with _Timed('jpeg_entropy_size', 0.0, (t, rows, mcus), 2.0 * coefs.numel() * 2):
            _jpeg_refusal(l.lp_jpeg_entropy_size(coefs.data_ptr(), t, rows, mcus, len(header), scratch.data_ptr(), need, offsets.data_ptr(),
                                                 _stream()), 'lp_jpeg_entropy_size')
        total = int(offsets[t].item())                                  # the one read-back
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        with _Timed('jpeg_entropy_write', 0.0, (t, rows, mcus), 2.0 * total):
            _jpeg_refusal(l.lp_jpeg_entropy_write(scratch.data_ptr(), need, t, rows, mcus, head.data_ptr(), len(header), out.data_ptr(), total,
                                                  _stream()), 'lp_jpeg_entropy_write')
    return out, offsets


def jpeg_encode(frames: Tensor, quality: int = 90):
    """(uint8 [total], int64 [T + 1]) on the frames' device: uint8 RGB ``frames`` [T, H, W, 3] (any strides: what ``drive.drive_frames`` returns)
    as T complete baseline JFIF files back to back, file t = bytes offsets[t] .. offsets[t + 1] (the header comment of csrc/jpeg.hip; 4:4:4, the
    Annex K tables at ``quality`` 1 .. 100, one restart interval per block row).  ``jpeg_transform`` + ``jpeg_entropy``: six launches and one
    read-back of one integer.  CPU frames: ``jpeg_encode_host``."""
    from .utils import mjpeg
    _, h, w = _jpeg_frames(frames, 'jpeg_encode')
    quality = mjpeg.check_quality(quality, 'jpeg_encode')
    if not frames.is_cuda:
        return jpeg_encode_host(frames, quality)
    return jpeg_entropy(jpeg_transform(frames, quality), mjpeg.jpeg_header(h, w, quality))


# ---- baseline PNG of the lossless outputs (csrc/png.hip holds the definition) ------------------------------------------------------------------------
PNG_SEG = 16384                     # bytes of the filtered stream per deflate segment
PNG_HEADER_BITS = 1222              # the dynamic block header of the definition: 17 + 19 x 3 + 287 x 4
_PNG_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_PNG_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def _png_frames(frames, who):
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f'{who}: frames must be a tensor, got {type(frames).__name__}')
    if frames.dtype != torch.uint8:
        raise ValueError(f'{who}: frames must be uint8, got {frames.dtype}')
    if frames.dim() != 4:
        raise ValueError(f'{who}: frames must be 4-D [T, H, W, C], got shape {tuple(frames.shape)}')
    t, h, w, c = frames.shape
    if c not in (1, 3):
        raise ValueError(f'{who}: frames must be grey or RGB [T, H, W, 1 or 3], got C = {c}')
    if t < 1 or h < 1 or w < 1:
        raise ValueError(f'{who}: empty input {tuple(frames.shape)}: T, H and W must be >= 1')
    return t, h, w, c


def _png_stream(filtered, who):
    if not (isinstance(filtered, torch.Tensor) and filtered.dtype == torch.uint8 and filtered.dim() == 2):
        raise ValueError(f'{who}: the filtered streams must be a uint8 tensor [T, L], got '
                         f'{(filtered.dtype, tuple(filtered.shape)) if isinstance(filtered, torch.Tensor) else type(filtered).__name__}')
    t, n = filtered.shape
    if t < 1 or n < 1:
        raise ValueError(f'{who}: empty stream table {tuple(filtered.shape)}: T and L must be >= 1')
    return t, n


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    import struct
    import zlib
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def _png_head(h: int, w: int, c: int) -> bytes:
    """the 45 bytes of a file that do not depend on the pixels: signature + IHDR (33), then IEND (12); their CRCs are computed here, on the host"""
    import struct
    return b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2 if c == 3 else 0, 0, 0, 0)) + _png_chunk(b'IEND', b'')


def _png_stream_head(n: int) -> bytes:
    """the head ``png_deflate`` gives a stream that comes without a shape: one grey row whose filtered bytes are the stream"""
    return _png_head(1, max(n - 1, 1), 1)


def png_filter_host(frames: Tensor) -> Tensor:
    """the filtered streams of csrc/png.hip in numpy: uint8 [T, H (1 + W C)], every row its filter type and its filtered bytes"""
    import numpy as np
    t, h, w, c = _png_frames(frames, 'png_filter_host')
    x = frames.detach().cpu().numpy().astype(np.int32)
    a, b, d = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, :, 1:] = x[:, :, :-1]
    b[:, 1:] = x[:, :-1]
    d[:, 1:, 1:] = x[:, :-1, :-1]
    p = a + b - d
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - d)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, d))
    cands = (np.stack((x, x - a, x - b, x - ((a + b) >> 1), x - paeth)) & 255).reshape(5, t, h, w * c)
    best = np.argmin(np.where(cands < 128, cands, 256 - cands).sum(-1), axis=0)          # the first minimum: ties to the lowest type
    rows = np.take_along_axis(cands, best[None, :, :, None], axis=0)[0]
    out = np.concatenate((best[:, :, None], rows), axis=-1).astype(np.uint8).reshape(t, h * (1 + w * c))
    return torch.from_numpy(out)


def png_code_lengths(hist):
    """steps 1 .. 4 of the code construction of csrc/png.hip: symbol counts -> code lengths <= 15 (a list as long as ``hist``)"""
    leaves = sorted((int(n), s) for s, n in enumerate(hist) if n > 0)
    m = len(leaves)
    lengths = [0] * len(hist)
    if m < 2:
        raise ValueError('png_code_lengths: at least two symbols must occur (a segment holds a byte and the end-of-block symbol)')
    weight = [n for n, _ in leaves]
    parent = [0] * (2 * m - 1)
    li = ii = 0
    for ni in range(m - 1):
        w = 0
        for _ in range(2):
            if li < m and (ii >= ni or weight[li] < weight[m + ii]):
                w += weight[li]
                parent[li] = m + ni
                li += 1
            else:
                w += weight[m + ii]
                parent[m + ii] = m + ni
                ii += 1
        weight.append(w)
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    cnt = [0] * (max(depth) + 2)
    for d in depth[:m]:
        cnt[d] += 1
    for deep in range(len(cnt) - 1, 15, -1):
        while cnt[deep] > 0:
            b = max(k for k in range(1, 15) if cnt[k] > 0)
            cnt[b] -= 1
            cnt[b + 1] += 2
            cnt[deep] -= 2
            cnt[deep - 1] += 1
    i = 0
    for length in range(min(15, len(cnt) - 1), 0, -1):
        for _ in range(cnt[length]):
            lengths[leaves[i][1]] = length
            i += 1
    return lengths


def png_canonical_codes(lengths):
    """RFC 1951 3.2.2: code lengths -> the codes, as integers whose most significant bit (of ``length`` bits) is sent first"""
    count = [0] * 17
    for length in lengths:
        count[length] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, length in enumerate(lengths):
        if length:
            codes[s] = nxt[length]
            nxt[length] += 1
    return codes


def _png_segment_host(f, final: bool) -> bytes:
    """one segment of the filtered stream (a numpy uint8 array of 1 .. PNG_SEG bytes) as its deflate bytes"""
    import numpy as np
    n = len(f)
    stored = bytes((int(final), n & 255, n >> 8, ~n & 255, (~n >> 8) & 255)) + f.tobytes()
    eq = np.zeros(n, dtype=bool)
    eq[1:] = f[1:] == f[:-1]
    idx = np.flatnonzero(~eq)                                     # position 0 is one of them
    run = np.append(idx[1:], n) - idx - 1                         # the stretch of eq behind each
    full, q = run // 258, run % 258
    per = 1 + full + np.where(q >= 3, 1, q)                       # tokens per item: its literal, the 258s, the remainder
    item = np.repeat(np.arange(len(idx)), per)
    k = np.arange(len(item)) - np.repeat(np.cumsum(per) - per, per)
    length = np.where((k >= 1) & (k <= full[item]), 258, np.where((k > full[item]) & (q[item] >= 3), q[item], 0))
    len_sym = np.zeros(259, dtype=np.int64)
    for i, base in enumerate(_PNG_LEN_BASE):
        len_sym[base:] = i
    ls = len_sym[length]
    is_match = length > 0
    sym = np.where(is_match, 257 + ls, f[idx][item])
    hist = np.bincount(sym, minlength=286)
    hist[256] += 1
    lengths = png_code_lengths(hist.tolist())
    codes = png_canonical_codes(lengths)
    rev = np.array([int(format(c, f'0{l}b')[::-1], 2) if l else 0 for c, l in zip(codes, lengths)], dtype=np.int64)
    lens = np.array(lengths, dtype=np.int64)
    eb = np.where(is_match, np.array(_PNG_LEN_EXTRA)[ls], 0)
    val = rev[sym] | np.where(is_match, (length - np.array(_PNG_LEN_BASE)[ls]) << lens[sym], 0)
    nbits = lens[sym] + np.where(is_match, eb + 1, 0)             # a match ends with the 1-bit distance code 0
    dyn_bits = PNG_HEADER_BITS + int(nbits.sum()) + lengths[256] + 3
    dyn_bytes = (dyn_bits + 7) // 8 + 4
    if dyn_bytes >= n + 5:
        return stored
    rev4 = lambda v: int(format(v, '04b')[::-1], 2)
    head_val = [0 | 2 << 1 | 29 << 3 | 0 << 8 | 15 << 13] + [0, 0, 0] + [4] * 16 + [rev4(l) for l in lengths] + [rev4(1)]
    head_bits = [17] + [3] * 19 + [4] * 287
    val = np.concatenate((np.array(head_val, dtype=np.int64), val, [rev[256], int(final)]))
    nbits = np.concatenate((np.array(head_bits, dtype=np.int64), nbits, [lengths[256], 3]))
    at = np.cumsum(nbits) - nbits
    bits = np.zeros(8 * (dyn_bytes - 4), dtype=np.uint8)
    for j in range(int(nbits.max())):
        sel = nbits > j
        bits[at[sel] + j] = (val[sel] >> j) & 1
    return np.packbits(bits, bitorder='little').tobytes() + b'\x00\x00\xff\xff'


def png_deflate_host(filtered: Tensor, head: Optional[bytes] = None):
    """the deflate and file stage of csrc/png.hip in numpy: ``filtered`` uint8 [T, L] (any bytes) -> (uint8 [total], int64 [T + 1]) on the CPU, every
    file = ``head[:33]`` + one IDAT (78 01, the segments, Adler-32) + ``head[33:]``; ``head`` defaults to one grey row of L - 1 pixels"""
    import struct
    import zlib
    t, n = _png_stream(filtered, 'png_deflate_host')
    head = _png_stream_head(n) if head is None else bytes(head)
    if len(head) != 45:
        raise ValueError(f'png_deflate_host: head must be the 45 bytes of _png_head, got {len(head)}')
    streams = filtered.detach().cpu().contiguous().numpy()
    out, offsets = bytearray(), [0]
    for f in streams:
        z = bytearray(b'\x78\x01')
        for first in range(0, n, PNG_SEG):
            z += _png_segment_host(f[first:first + PNG_SEG], first + PNG_SEG >= n)
        z += struct.pack('>I', zlib.adler32(f.tobytes()))
        out += head[:33] + _png_chunk(b'IDAT', bytes(z)) + head[33:]
        offsets.append(len(out))
    return torch.frombuffer(out, dtype=torch.uint8).clone(), torch.tensor(offsets, dtype=torch.int64)


def png_encode_host(frames: Tensor):
    """``png_encode`` in numpy, on the CPU: (uint8 [total], int64 [T + 1])"""
    _, h, w, c = _png_frames(frames, 'png_encode_host')
    return png_deflate_host(png_filter_host(frames), _png_head(h, w, c))


def png_filter(frames: Tensor) -> Tensor:
    """uint8 [T, H (1 + W C)]: the filtered streams of uint8 ``frames`` [T, H, W, C], C = 1 or 3 (the header comment of csrc/png.hip), ``frames`` read
    in place through its four strides.  ONE launch on the current stream (lp_png_filter).  CPU frames: ``png_filter_host``."""
    t, h, w, c = _png_frames(frames, 'png_filter')
    if not frames.is_cuda:
        return png_filter_host(frames)
    import ctypes
    frames = frames.detach()
    strides = (ctypes.c_longlong * 4)(*frames.stride())
    n = h * (1 + w * c)
    with torch.cuda.device(frames.device):
        if t * n > 2 ** 31 - 1:
            raise ValueError('png_filter: the filtered streams would exceed 2^31 - 1 bytes: encode fewer frames per call')
        filtered = torch.empty((t, n), dtype=torch.uint8, device=frames.device)
        with _Timed('png_filter', 0.0, (t, h, w, c), (2.0 * t * h * w * c, float(t * n))):
            _jpeg_refusal(_lib.lib().lp_png_filter(frames.data_ptr(), ctypes.addressof(strides), t, h, w, c, filtered.data_ptr(), _stream()),
                          'lp_png_filter')
    return filtered


def png_deflate(filtered: Tensor, head: Optional[bytes] = None):
    """(uint8 [total], int64 [T + 1]) on the streams' device: every row of ``filtered`` (uint8 [T, L], any bytes) as a PNG file whose IDAT holds
    its zlib stream (the header comment of csrc/png.hip); ``head``: the 45 bytes of ``_png_head(H, W, C)``, by default one grey row of L - 1 pixels.
    Two launches (lp_png_deflate_size), ONE device-to-host copy of one integer -- the total size --, one launch (lp_png_write) into an output
    allocated at exactly that size.  Bit-identical from run to run.  CPU streams: ``png_deflate_host``."""
    t, n = _png_stream(filtered, 'png_deflate')
    head = _png_stream_head(n) if head is None else bytes(head)
    if len(head) != 45:
        raise ValueError(f'png_deflate: head must be the 45 bytes of _png_head, got {len(head)}')
    if not filtered.is_cuda:
        return png_deflate_host(filtered, head)
    import ctypes
    l = _lib.lib()
    need = l.lp_png_deflate_scratch_bytes(t, n)
    if need < 0:
        _jpeg_refusal(int(need), 'lp_png_deflate_scratch_bytes')
    filtered = filtered.detach().contiguous()
    dev = filtered.device
    head_c = (ctypes.c_ubyte * 45)(*head)
    with torch.cuda.device(dev):
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        offsets = torch.empty(t + 1, dtype=torch.int64, device=dev)
        with _Timed('png_deflate_size', 0.0, (t, n), (float(t * n), float(need))):
            _jpeg_refusal(l.lp_png_deflate_size(filtered.data_ptr(), t, n, scratch.data_ptr(), need, offsets.data_ptr(), _stream()),
                          'lp_png_deflate_size')
        total = int(offsets[t].item())                                  # the one read-back
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        with _Timed('png_write', 0.0, (t, n), 2.0 * total):
            _jpeg_refusal(l.lp_png_write(scratch.data_ptr(), need, t, n, ctypes.addressof(head_c), offsets.data_ptr(), out.data_ptr(), total,
                                         _stream()), 'lp_png_write')
    return out, offsets


def png_encode(frames: Tensor):
    """(uint8 [total], int64 [T + 1]) on the frames' device: uint8 ``frames`` [T, H, W, C], C = 1 or 3 (any strides: what ``drive.drive_frames``
    returns) as T complete PNG files back to back, file t = bytes offsets[t] .. offsets[t + 1], every pixel kept exactly (the header comment of
    csrc/png.hip).  ``png_filter`` + ``png_deflate``: four launches and one read-back of one integer.  CPU frames: ``png_encode_host``."""
    _, h, w, c = _png_frames(frames, 'png_encode')
    if not frames.is_cuda:
        return png_encode_host(frames)
    return png_deflate(png_filter(frames), _png_head(h, w, c))


# ---- baseline JPEG decode of the loader's frames (csrc/jpeg_decode.hip holds the definition) ---------------------------------------------------------
class JpegDecoded(NamedTuple):
    """``buf`` uint8: frame f = dense [H, W, 3] RGB at ``offsets[f]``; ``status`` int32 [N] on the buffer's device (0 ok, 1 no code matches, 2 a run
    leaves its block, 3 a segment ends inside a code); the workspaces: ``coefs`` int16 [blocks, 64] in zigzag and scan order, ``planes`` uint8 (every
    frame's sample planes at its plane offset); ``frames`` the int64 [N, 24] table of the call (``utils.jpeg_parse.FRAME_COLUMNS``), on the host"""
    buf: Tensor
    offsets: Tensor
    status: Tensor
    coefs: Tensor
    planes: Tensor
    frames: Tensor


def _jpeg_packed(frames, offsets, who):
    """a list of ``utils.jpeg_parse.Descriptor`` or the packed form (``jpeg_parse.pack`` / ``merge``) -> the packed form as contiguous host tensors"""
    import numpy as np
    from .utils import jpeg_parse
    if isinstance(frames, (list, tuple)):
        if not frames or not all(isinstance(d, jpeg_parse.Descriptor) for d in frames):
            raise ValueError(f'{who}: a non-empty list of jpeg_parse.Descriptor (or the packed form of jpeg_parse.pack) is expected')
        if offsets is not None and len(offsets) != len(frames):
            raise ValueError(f'{who}: {len(offsets)} offsets for {len(frames)} frames')
        frames = jpeg_parse.pack(list(frames), None if offsets is None else [int(o) for o in offsets])
    elif not isinstance(frames, dict) or any(k not in frames for k in ('scan', 'seg', 'frames', 'qt', 'huffman', 'coef_blocks', 'plane_bytes')):
        raise ValueError(f'{who}: a list of jpeg_parse.Descriptor or the packed form of jpeg_parse.pack is expected, got {type(frames).__name__}')
    elif offsets is not None:
        raise ValueError(f'{who}: the packed form carries its destination offsets (column dst_off); offsets go with a list of descriptors')
    pk = dict(frames)
    for k, dt in (('scan', torch.uint8), ('seg', torch.int64), ('frames', torch.int64), ('qt', torch.uint8), ('huffman', torch.int32)):
        t = pk[k] if isinstance(pk[k], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pk[k]))
        if t.dtype != dt or t.is_cuda:
            raise ValueError(f'{who}: the packed table {k!r} must be a HOST {dt} tensor, got {t.dtype} on {t.device}')
        pk[k] = t.contiguous()
    n = pk['frames'].shape[0]
    if (pk['frames'].dim() != 2 or pk['frames'].shape[1] != jpeg_parse.NFRAME or n < 1 or pk['seg'].dim() != 2 or pk['seg'].shape[1] != jpeg_parse.NSEG
            or tuple(pk['qt'].shape) != (n, 4, 64) or tuple(pk['huffman'].shape) != (n, 8, jpeg_parse.HUFF_WORDS) or pk['scan'].dim() != 1):
        raise ValueError(f'{who}: the packed tables do not have the shapes of jpeg_parse.pack')
    return pk


def _jpeg_out(pk, out, device, who):
    """the destination buffer: ``out`` as given, or a dense one of the packed form's size on ``device``"""
    rows = pk['frames']
    need = int((rows[:, 10] + rows[:, 0] * rows[:, 1] * 3).max())
    if out is None:
        if not pk.get('out_bytes'):
            raise ValueError(f'{who}: destination offsets were given, so the buffer they point into (out) is needed too')
        return torch.empty(int(pk['out_bytes']), dtype=torch.uint8, device=device), need
    if not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.dim() == 1 and out.is_contiguous()):
        raise ValueError(f'{who}: out must be a contiguous 1-D uint8 tensor')
    if int(rows[:, 10].min()) < 0 or need > out.numel():
        bad = int(((rows[:, 10] < 0) | (rows[:, 10] + rows[:, 0] * rows[:, 1] * 3 > out.numel())).nonzero()[0])
        raise ValueError(f'{who}: frame {bad}: the destination ({int(rows[bad, 0] * rows[bad, 1] * 3)} bytes at {int(rows[bad, 10])}) lies outside '
                         f'the buffer of {out.numel()} bytes')
    return out, need


def jpeg_decode_host(frames, out: Optional[Tensor] = None, offsets=None) -> JpegDecoded:
    """``jpeg_decode`` in numpy integers on the CPU: the definition of csrc/jpeg_decode.hip step for step, from the same packed tables the device
    reads.  A frame whose stream does not decode gets its status; the other frames are not affected."""
    import numpy as np
    from .utils import jpeg_parse, mjpeg
    pk = _jpeg_packed(frames, offsets, 'jpeg_decode_host')
    buf, _ = _jpeg_out(pk, out, 'cpu', 'jpeg_decode_host')
    if buf.is_cuda:
        raise ValueError('jpeg_decode_host: out is on the GPU (the device version is jpeg_decode)')
    rows, seg, scan = pk['frames'].tolist(), pk['seg'].tolist(), pk['scan'].numpy()
    huff, qt = pk['huffman'].numpy(), pk['qt'].numpy().astype(np.int64)
    n = len(rows)
    coefs = np.zeros((int(pk['coef_blocks']), 64), dtype=np.int16)
    planes = np.zeros(int(pk['plane_bytes']), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    dst = buf.numpy()
    K = jpeg_parse.idct_table().astype(np.int64).reshape(8, 8)
    natural = np.array(mjpeg.ZIGZAG)
    for f, r in enumerate(rows):
        h, w, nc, hmax, vmax, mcux, mcuy, ri, coef_off, plane_off, dst_off, seg0, nseg = r[:13]
        nluma = hmax * vmax if nc == 3 else 1
        bpm = nluma + 2 if nc == 3 else 1
        total = mcux * mcuy
        tabs = [(t[:16].tolist(), t[16:32].tolist(), t[32:].view(np.uint8).tolist()) for t in huff[f]]
        # entropy: a segment at a time, as a lane of the kernel walks it
        for s in range(seg0, seg0 + nseg):
            first = (s - seg0) * ri
            count = min(ri, total - first) if ri else total
            data = bytes(scan[seg[s][1]:seg[s][2]])
            nbits = 8 * len(data)
            big, width = int.from_bytes(data + bytes(8), 'big'), nbits + 64
            used, st, pred = 0, 0, [0, 0, 0]

            def symbol(tab):
                nonlocal used
                word = (big >> (width - used - 16)) & 0xFFFF
                for l in range(16):
                    code = word >> (15 - l)
                    if code <= tab[0][l]:
                        used += l + 1
                        return tab[2][min(max(code + tab[1][l], 0), 255)]
                return -1

            def extend(size):
                nonlocal used
                v = (big >> (width - used - size)) & ((1 << size) - 1)
                used += size
                return v - (1 << size) + 1 if v < (1 << (size - 1)) else v

            for b in range(count * bpm):
                if st:
                    break                   # (coefs starts as zeros: what the kernel writes behind a failure)
                blk = coefs[coef_off + first * bpm + b]
                j = b % bpm
                c = 0 if j < nluma else j - nluma + 1
                sd = symbol(tabs[r[16 + c]])
                if sd < 0 or sd > 15:
                    st = 1
                    continue
                diff = extend(sd) if sd else 0
                if used > nbits:
                    st = 3
                    continue
                pred[c] = ((pred[c] + diff + 32768) & 0xFFFF) - 32768
                blk[0] = pred[c]
                k = 1
                for _ in range(63):
                    if k >= 64:
                        break
                    rs = symbol(tabs[4 + r[19 + c]])
                    if rs < 0:
                        st = 1
                        break
                    run, size = rs >> 4, rs & 15
                    if size == 0:
                        if used > nbits:
                            st = 3
                            break
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    if k > 63:
                        st = 2
                        break
                    a = extend(size)
                    if used > nbits:
                        st = 3
                        break
                    blk[k] = a
                    k += 1
            status[f] = max(status[f], st)
        # dequantise + IDCT, all blocks of the frame at once
        blocks = total * bpm
        comp = np.array([0 if j < nluma else j - nluma + 1 for j in range(bpm)] * total)
        F = np.zeros((blocks, 64), dtype=np.int64)
        F[:, natural] = coefs[coef_off:coef_off + blocks].astype(np.int64)
        F = np.clip(F * qt[f][np.array(r[13:16])[comp]], -32768, 32767).reshape(blocks, 8, 8)
        T = (np.einsum('ux,buv->bxv', K, F) + 512) >> 10
        S = np.clip(((np.einsum('vy,bxv->bxy', K, T) + 32768) >> 16) + 128, 0, 255).astype(np.uint8).reshape(total, bpm, 8, 8)
        ph0, pw0 = mcuy * (vmax if nc == 3 else 1) * 8, mcux * (hmax if nc == 3 else 1) * 8
        luma = S[:, :nluma].reshape(mcuy, mcux, ph0 // (8 * mcuy), pw0 // (8 * mcux), 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(ph0, pw0)
        planes[plane_off:plane_off + ph0 * pw0] = luma.reshape(-1)
        rgb = [luma[:h, :w].astype(np.int64)] * 3
        if nc == 3:
            chroma = []
            for c in (1, 2):
                p = S[:, nluma + c - 1].reshape(mcuy, mcux, 8, 8).transpose(0, 2, 1, 3).reshape(mcuy * 8, mcux * 8)
                at = plane_off + ph0 * pw0 + (c - 1) * p.size
                planes[at:at + p.size] = p.reshape(-1)
                x = p[:-(-h // vmax), :-(-w // hmax)].astype(np.int64)
                if vmax == 2:               # replicated edges give the edge rules: 3 cs + cs = 4 cs
                    x = np.stack([3 * x + np.concatenate([x[:1], x[:-1]]), 3 * x + np.concatenate([x[1:], x[-1:]])], axis=1).reshape(-1, x.shape[1])[:h]
                if hmax == 2:
                    lo, sh = (8, 4) if vmax == 2 else (1, 2)
                    even = (3 * x + np.concatenate([x[:, :1], x[:, :-1]], axis=1) + lo) >> sh
                    odd = (3 * x + np.concatenate([x[:, 1:], x[:, -1:]], axis=1) + lo + (1 if vmax == 1 else -1)) >> sh
                    x = np.stack([even, odd], axis=2).reshape(x.shape[0], -1)[:, :w]
                chroma.append(x - 128)
            cb, cr = chroma
            y = rgb[0]
            rgb = [y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)]
        dst[dst_off:dst_off + h * w * 3] = np.clip(np.stack(rgb, axis=2), 0, 255).astype(np.uint8).reshape(-1)
    return JpegDecoded(buf, pk['frames'][:, 10].clone(), torch.from_numpy(status), torch.from_numpy(coefs), torch.from_numpy(planes), pk['frames'])


def jpeg_decode(frames, out: Optional[Tensor] = None, offsets=None, device=None) -> JpegDecoded:
    """JPEG files -> uint8 RGB on the device (the header comment of csrc/jpeg_decode.hip).  ``frames``: a list of ``utils.jpeg_parse.Descriptor``
    (what ``jpeg_parse.parse`` returns for a supported file) or the packed form of ``jpeg_parse.pack`` / ``merge`` (the loader's collate function
    makes it in the worker).  Frame f is written as dense [H, W, 3] at ``offsets[f]`` of ``out`` (a 1-D uint8 tensor; the packed form carries the
    offsets in its table), no other byte of ``out`` changes; without ``out`` the frames are packed back to back into a new buffer on ``device``.
    A clear and THREE launches on the current stream (lp_jpeg_decode_entropy, lp_jpeg_decode_pixels), the tables copied from pinned memory without
    blocking; no host synchronisation: ``status`` stays on the device for the caller to read when it suits.  Arguments the C ABI refuses raise
    ValueError naming the frame.  A CPU ``out`` (or ``device`` 'cpu'): ``jpeg_decode_host``."""
    import ctypes
    from .utils import jpeg_parse
    device = torch.device(device if device is not None else (out.device if isinstance(out, torch.Tensor) else 'cuda'))
    if device.type != 'cuda':
        return jpeg_decode_host(frames, out, offsets)
    pk = _jpeg_packed(frames, offsets, 'jpeg_decode')
    if isinstance(out, torch.Tensor) and not out.is_cuda:
        raise ValueError(f'jpeg_decode: out is on {out.device} and device is {device}')
    n, nseg = pk['frames'].shape[0], pk['seg'].shape[0]
    blocks, plane_bytes = int(pk['coef_blocks']), int(pk['plane_bytes'])
    K = jpeg_parse.idct_table()
    l = _lib.lib()
    with torch.cuda.device(device):
        buf, _ = _jpeg_out(pk, out, device, 'jpeg_decode')
        dev = {k: (pk[k] if pk[k].is_pinned() else pk[k].pin_memory()).to(device, non_blocking=True) for k in ('scan', 'seg', 'frames', 'qt', 'huffman')}
        coefs = torch.empty((max(blocks, 1), 64), dtype=torch.int16, device=device)
        planes = torch.empty(max(plane_bytes, 1), dtype=torch.uint8, device=device)
        status = torch.empty(n, dtype=torch.int32, device=device)
        with _Timed('jpeg_decode_entropy', 0.0, (n, nseg), (pk['scan'].numel(), 128 * blocks)):
            _jpeg_refusal(l.lp_jpeg_decode_entropy(dev['scan'].data_ptr(), pk['scan'].numel(), pk['seg'].data_ptr(), dev['seg'].data_ptr(), nseg,
                                                   pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['huffman'].data_ptr(), coefs.data_ptr(),
                                                   blocks, status.data_ptr(), _stream()), 'lp_jpeg_decode_entropy')
        npix = int((pk['frames'][:, 0] * pk['frames'][:, 1]).sum())
        with _Timed('jpeg_decode_pixels', 0.0, (n, blocks), (128 * blocks + 2 * 64 * blocks, 64 * blocks + 3 * npix)):
            _jpeg_refusal(l.lp_jpeg_decode_pixels(coefs.data_ptr(), blocks, pk['frames'].data_ptr(), dev['frames'].data_ptr(), n, dev['qt'].data_ptr(),
                                                  K.ctypes.data_as(ctypes.c_void_p), planes.data_ptr(), plane_bytes, buf.data_ptr(), buf.numel(),
                                                  _stream()), 'lp_jpeg_decode_pixels')
    return JpegDecoded(buf, pk['frames'][:, 10].clone(), status, coefs, planes, pk['frames'])


def relu_bwd(dA: Tensor, x: Tensor) -> Tensor:
    _chk(dA, 'dA'); _chk(x, 'x')
    dx = torch.empty_like(x)
    check(_lib.lib().lp_relu_bwd(dA.data_ptr(), x.data_ptr(), dx.data_ptr(), x.numel(), _stream()), 'lp_relu_bwd')
    return dx


def avgpool2_fwd(x: Tensor, relu_in: bool, out16_prec: Optional[int] = None, relu_out: bool = False):
    """AvgPool2d(2) of relu?(x); ``relu_out``: y = relu(pool(x)).  ``out16_prec`` (PREC_F16 | PREC_BF16, C % 8 == 0): also the operand planes of y
    -> (y, Act16)"""
    _chk(x, 'x')
    n, h2, w2, c = x.shape
    y = torch.empty((n, h2 // 2, w2 // 2, c), dtype=torch.float32, device=x.device)
    fused = out16_prec is not None and out16_prec != PREC_BF16X3 and c % 8 == 0
    o_hi = torch.empty((n, h2 // 2, w2 // 2, c), dtype=torch.int16, device=x.device) if fused else None
    check(_lib.lib().lp_avgpool2_fwd(x.data_ptr(), y.data_ptr(), n, h2 // 2, w2 // 2, c, int(relu_in) | (2 if relu_out else 0), _p(o_hi),
                                     out16_prec if fused else 0, _stream()), 'lp_avgpool2_fwd')
    if out16_prec is None:
        return y
    return y, (Act16(o_hi, None, c, None) if fused else act_pack(y, pro=0, prec=out16_prec))


def avgpool2_fwd16(x: Act16, prec: int) -> Act16:
    """AvgPool2d(2) on operand planes (one-plane modes): planes in, planes out -- for no-grad chains that keep no fp32 activations"""
    n, h2, w2 = x.nhw
    c = x.c
    assert x.lo is None and c % 8 == 0 and x.hi.shape[3] == c and prec != PREC_BF16X3
    o_hi = torch.empty((n, h2 // 2, w2 // 2, c), dtype=torch.int16, device=x.hi.device)
    check(_lib.lib().lp_avgpool2_fwd16(x.hi.data_ptr(), o_hi.data_ptr(), n, h2 // 2, w2 // 2, c, prec, _stream()), 'lp_avgpool2_fwd16')
    return Act16(o_hi, None, c, None)


def avgpool2_bwd(dy: Tensor, x: Optional[Tensor], relu_in: bool, amax: bool = False, y_relu: Optional[Tensor] = None) -> Tensor:
    """backward of ``avgpool2_fwd``: ``x`` = the forward's input (read only with ``relu_in``); ``y_relu`` = the forward's OUTPUT when it applied
    ``relu_out`` (dy is masked by [y > 0]); with neither mask nothing of the forward needs to be kept"""
    _chk(dy, 'dy')
    assert not (relu_in and y_relu is not None)
    n, ho, wo, c = dy.shape
    h, w = 2 * ho, 2 * wo
    mask = None
    if relu_in:
        _chk(x, 'x'); assert tuple(x.shape) == (n, h, w, c)
        mask = x
    elif y_relu is not None:
        _chk(y_relu, 'y_relu'); assert tuple(y_relu.shape) == tuple(dy.shape)
        mask = y_relu
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
    check(_lib.lib().lp_avgpool2_bwd(dy.data_ptr(), _p(mask), dx.data_ptr(), n, h, w, c, int(relu_in) | (2 if y_relu is not None else 0),
                                     _p(_amax_attach(dx, amax)), _stream()), 'lp_avgpool2_bwd')
    return dx


class Tap16(NamedTuple):
    """a feature tap kept as 16-bit operand planes (of relu(y): what the next conv consumes anyway) instead of an fp32 tensor"""
    act: Act16
    prec: int

    def float(self):
        """decoded fp32 NHWC tensor (debug tapes / tests)"""
        return self.act.hi.view(torch.float16 if self.prec == PREC_F16 else torch.bfloat16).float()

    def detach(self):
        return self


def l1_sum(a: Tensor, b, relu_in: bool, coef: float = 1.0, want_sign: bool = False):
    """coef * sum |relu?(a) - relu?(b)| as a 0-d tensor (block partials + a one-block finalize launch).  ``want_sign``: -> (term, sgn)
    with sgn int8 [numel] = the sign pattern the backward needs (``l1_bwd(sign=...)`` then does not read a and b again)"""
    _chk(a, 'a')
    buf = torch.empty(_lib.lib().lp_l1_partial_blocks() + 1, dtype=torch.float32, device=a.device)
    out = buf[-1:]
    sgn = torch.empty(a.numel(), dtype=torch.int8, device=a.device) if want_sign else None
    if isinstance(b, Tap16):           # b = 16-bit operand planes of the other image's tap (same NHWC element order, no channel padding)
        assert tuple(b.act.hi.shape) == tuple(a.shape) and b.act.lo is None, (b.act.hi.shape, a.shape)
        check(_lib.lib().lp_l1_fwd_b16(a.data_ptr(), b.act.hi.data_ptr(), b.prec, buf.data_ptr(), a.numel(), int(relu_in), float(coef),
                                       out.data_ptr(), _p(sgn), _stream()), 'lp_l1_fwd_b16')
        return (out.reshape(()), sgn) if want_sign else out.reshape(())
    _chk(b, 'b')
    assert a.shape == b.shape
    check(_lib.lib().lp_l1_fwd(a.data_ptr(), b.data_ptr(), buf.data_ptr(), a.numel(), int(relu_in), float(coef), out.data_ptr(), _p(sgn),
                               _stream()), 'lp_l1_fwd')
    return (out.reshape(()), sgn) if want_sign else out.reshape(())


def l1_sum16(a: 'Tap16', b: 'Tap16', coef: float = 1.0, want_sign: bool = False):
    """coef * sum |a - b| for two taps held as the operand planes of relu(.) (same precision mode); ``want_sign`` as ``l1_sum`` with relu_in"""
    assert a.prec == b.prec and tuple(a.act.hi.shape) == tuple(b.act.hi.shape) and a.act.lo is None and b.act.lo is None
    dev = a.act.hi.device
    buf = torch.empty(_lib.lib().lp_l1_partial_blocks() + 1, dtype=torch.float32, device=dev)
    out = buf[-1:]
    numel = a.act.hi.numel()
    sgn = torch.empty(numel, dtype=torch.int8, device=dev) if want_sign else None
    check(_lib.lib().lp_l1_fwd_ab16(a.act.hi.data_ptr(), b.act.hi.data_ptr(), a.prec, buf.data_ptr(), numel, float(coef), out.data_ptr(), _p(sgn),
                                    _stream()), 'lp_l1_fwd_ab16')
    return (out.reshape(()), sgn) if want_sign else out.reshape(())


def avgpool2_bwd_m16(dy: Tensor, mask: Act16, amax: bool = False) -> Tensor:
    """backward of AvgPool2d(2)(relu(x)) with the ReLU mask read from the operand planes of relu(x)"""
    _chk(dy, 'dy')
    n, h, w = mask.nhw
    c = mask.c
    assert mask.hi.shape[3] == c and tuple(dy.shape) == (n, h // 2, w // 2, c)
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dy.device)
    check(_lib.lib().lp_avgpool2_bwd_m16(dy.data_ptr(), mask.hi.data_ptr(), dx.data_ptr(), n, h, w, c, _p(_amax_attach(dx, amax)), _stream()),
          'lp_avgpool2_bwd_m16')
    return dx


def l1_bwd(a: Optional[Tensor], b: Optional[Tensor], grad_out: Tensor, coef: float, relu_in: bool, add: Optional[Tensor] = None,
           amax: bool = False, sign: Optional[Tensor] = None, shape=None) -> Tensor:
    """gradient of coef * sum|relu?(a) - relu?(b)| w.r.t. a, times grad_out; ``add`` (same shape) is summed in.  ``sign`` (from
    ``l1_sum(want_sign=True)``) replaces a and b; ``shape`` is then the shape of the result"""
    if sign is None:
        _chk(a, 'a'); _chk(b, 'b')
        shape = a.shape
    if add is not None:
        _chk(add, 'add'); assert tuple(add.shape) == tuple(shape)
    g = grad_out.reshape(1).contiguous().float()
    da = torch.empty(tuple(shape), dtype=torch.float32, device=g.device)
    check(_lib.lib().lp_l1_bwd(_p(a), _p(b), g.data_ptr(), float(coef), _p(add), da.data_ptr(), da.numel(), int(relu_in), _p(sign),
                               _p(_amax_attach(da, amax)), _stream()), 'lp_l1_bwd')
    return da



# ---- ResNeXt-50 identity encoder: BatchNorm statistics, grouped 3x3 conv, stem, pooling (csrc/resnext.hip); BatchNorm backward (csrc/norm_bwd.hip) ----
def flat_hw(p: int) -> Tuple[int, int]:
    """(H, W) factorisation of P pixels for the 1x1 contractions (they do not care about the spatial structure): the widest W in
    {16, 8, 4} with H >= 2"""
    for w in (16, 8, 4):
        if p % w == 0 and p // w >= 2:
            return p // w, w
    raise ValueError(f'{p} pixels cannot be arranged as H x W with W in (16, 8, 4), H >= 2')


def flat16(a: Act16) -> Act16:
    """the same operand planes viewed as ONE image of P = N*H*W pixels (for 1x1 convs)"""
    c8 = a.hi.shape[-1]
    p = a.hi.numel() // c8
    h, w = flat_hw(p)
    return Act16(a.hi.view(1, h, w, c8), None if a.lo is None else a.lo.view(1, h, w, c8), a.c, a.inv)


def bn_train_stats(y: Tensor, gamma: Tensor, beta: Tensor, running_mean: Optional[Tensor], running_var: Optional[Tensor], momentum: float,
                   eps: float):
    """train-mode BatchNorm2d statistics of y [..., C] -> (mean, rstd, scale, shift) [C]; running statistics updated in place"""
    _chk(y, 'y')
    c = y.shape[-1]
    p = y.numel() // c
    out = torch.empty(4, c, dtype=torch.float32, device=y.device)
    ws = torch.empty(_lib.lib().lp_bn_train_stats_workspace_bytes(p, c) // 4, dtype=torch.float32, device=y.device)
    check(_lib.lib().lp_bn_train_stats(y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, momentum, _p(running_mean), _p(running_var),
                                       out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), p, c, _stream()),
          'lp_bn_train_stats')
    return out[0], out[1], out[2], out[3]


def _flat_pc(dA: Tensor, x, mask_src):
    """the [P][C] view of the norm-backward operands: -> (shape, P, C, data pointer of mask_src | None).  ``x`` / ``mask_src``: fp32 tensors of
    dA's shape or the 16-bit plane of that shape (``Act16``; x: one unscaled fp16 plane)"""
    _chk(dA, 'dA')
    for t, name in ((x, 'x'), (mask_src, 'mask_src')):
        if isinstance(t, Act16):
            assert t.hi.shape == dA.shape, (name, t.hi.shape, dA.shape)
        elif t is not None and t.dtype == torch.uint8:          # the one-bit pattern of bn_add_act(want_bits=True)
            assert name == 'mask_src' and t.is_cuda and t.is_contiguous() and dA.shape[-1] % 8 == 0 and \
                tuple(t.shape) == tuple(dA.shape[:-1]) + (dA.shape[-1] // 8,), (name, t.shape, dA.shape)
        elif t is not None:
            _chk(t, name); assert t.shape == dA.shape, (name, t.shape, dA.shape)
    c = dA.shape[-1]
    return dA.shape, dA.numel() // c, c, _p(mask_src.hi if isinstance(mask_src, Act16) else mask_src)


def norm_act_bwd(dA: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, scale: Tensor, shift: Tensor, *, mask_mode: int = 0,
                 mask_src: Optional[Tensor] = None, want_g: bool = False, act_hi: float = 0.0, frozen: bool = False, amax: bool = False):
    """backward of act(BatchNorm(x)) over x [..., C] treated as [P][C] (per-channel statistics [C]):
    -> (dx, dgamma [C], dbeta [C], g | None).  mask_mode 0: act = ReLU (act_hi = 6: ReLU6) of the layer's own affine; 1: no activation;
    2: ReLU pattern taken from ``mask_src`` (the residual block's output).  ``want_g``: also return the masked incoming gradient."""
    assert not isinstance(x, Act16) and not isinstance(mask_src, Act16), 'fp32 operands only (the 16-bit forms are bn_bwd16\'s)'
    _, p, c, mptr = _flat_pc(dA, x, mask_src)
    dx = torch.empty_like(x)
    dgb = torch.empty(2, c, dtype=torch.float32, device=x.device)
    g = torch.empty_like(x) if want_g else None
    ws = torch.empty(_lib.lib().lp_adain_bwd_workspace_bytes(1, p, c) // 4, dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_norm_act_bwd(dA.data_ptr(), x.data_ptr(), None, gamma.data_ptr(), c, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(),
                                     shift.data_ptr(), dx.data_ptr(), dgb[0].data_ptr(), dgb[1].data_ptr(), ws.data_ptr(), 1, p, 1, c, 0,
                                     mask_mode, mptr, _p(g), float(act_hi), int(frozen), _p(_amax_attach(dx, amax)), _stream()),
          'lp_norm_act_bwd')
    return dx, dgb[0], dgb[1], g


def pack_grouped(w: Tensor, mode: int, prec: int) -> WeightPack:
    """w [C, cg, 3, 3] (grouped conv, C/cg groups) -> the [9][CP][64] image of the block-diagonal formulation (lp_gconv16_fwd)"""
    _chk(w, 'w')
    c, cg = w.shape[0], w.shape[1]
    cp = _round_up(c, 128)
    hi = torch.empty((9, cp, 64), dtype=torch.int16, device=w.device)
    lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
    check(_lib.lib().lp_pack_grouped(w.data_ptr(), hi.data_ptr(), _p(lo), c, cg, cp, mode, _f16(prec), _stream()), 'lp_pack_grouped')
    return WeightPack(hi, lo, c, cg, cp, 64, 9)          # cols = the group size (logical contraction width per output channel)


def gconv16(a: Act16, pack: WeightPack, *, prec: int, amax: bool = False, stats: bool = False, want_y: bool = True, out16: bool = False):
    """grouped 3x3 conv (pad 1, stride 1) on operand planes a [N,H,W,C] -> y [N,H,W,C] fp32; with the mode-1 pack: the data gradient.
    ``stats``: -> (y, ConvStats | None) as ``conv16``.  ``out16``: the operand planes of y are a second output (y, Act16[, stats]);
    ``want_y=False`` (with ``out16``): no fp32 y is written, y is returned as None."""
    n, h, w = a.nhw
    c = a.c
    assert c == pack.rows and a.hi.shape[3] == c, (a.hi.shape, pack.rows)
    assert want_y or (out16 and not amax)
    dev = a.hi.device
    y = torch.empty((n, h, w, c), dtype=torch.float32, device=dev) if want_y else None
    o_hi = o_lo = None
    if out16:
        o_hi, o_lo = _alloc16(n, h, w, c, prec, dev)
    slots = _amax_attach(y, amax and prec == PREC_F16) if y is not None else None
    st_buf, st_rows, st_cap = None, None, 0
    if stats:
        import ctypes
        st_cap = _lib.lib().lp_conv16_stats_floats(n, h, w, c)
        st_buf = torch.empty(st_cap, dtype=torch.float32, device=dev)
        st_rows = ctypes.c_int(0)
    pl = 4 if prec == PREC_BF16X3 else 2
    nbytes = n * h * w * c * (pl + (4 if want_y else 0) + (pl if out16 else 0)) + pack.hi.numel() * pl
    with _Timed('gconv', 2.0 * n * h * w * c * pack.cols * 9, (n, h, w, pack.cols, c, 3, 0, 0), nbytes, mm=3 if prec == PREC_BF16X3 else 1):
        check(_lib.lib().lp_gconv16_fwd_planes(a.hi.data_ptr(), _p(a.lo), pack.hi.data_ptr(), _p(pack.lo), _p(y), _p(o_hi), _p(o_lo), _p(a.inv),
                                               n, h, w, c, pack.rows_p, pack.cols, prec, _p(slots), _p(st_buf), st_cap,
                                               None if st_rows is None else ctypes.addressof(st_rows), _stream()), 'lp_gconv16_fwd')
    out = (y,) if not out16 else (y, Act16(o_hi, o_lo, c, None))
    if stats:
        out = out + ((ConvStats(st_buf, st_rows.value, n) if st_rows.value > 0 else None),)
    return out[0] if len(out) == 1 else out


def bn_act16(y16: Act16, scale: Tensor, shift: Tensor, relu: bool = True) -> Act16:
    """operand planes of (relu?)(y*scale[c]+shift[c]) from a 16-BIT-RESIDENT conv output y16 (fp16 mode: the fp16 plane the conv epilogue
    wrote instead of fp32 y): ``act_pack`` pro 4 / 5 reading 2 B per element"""
    c = y16.c
    assert y16.lo is None and y16.inv is None and y16.hi.shape[-1] == c and c % 8 == 0
    hi = torch.empty_like(y16.hi)
    check(_lib.lib().lp_bn_act16(y16.hi.data_ptr(), scale.data_ptr(), shift.data_ptr(), hi.data_ptr(), y16.hi.numel() // c, c, int(relu),
                                 _stream()), 'lp_bn_act16')
    return Act16(hi, None, c, None)


def adain_act16(y16: Act16, scale: Tensor, shift: Tensor, relu: bool = True) -> Act16:
    """operand planes of (relu?)(y*scale[n,c]+shift[n,c]) from a 16-BIT-RESIDENT conv output y16 [N,H,W,C] (fp16 mode) with per-IMAGE affines
    [N, C] -- AdaIN + ReLU as the next conv's prologue (``act_pack`` pro 1 reading 2 B per element instead of 4)"""
    c = y16.c
    n = y16.hi.shape[0]
    assert y16.lo is None and y16.inv is None and y16.hi.shape[-1] == c and c % 8 == 0
    _chk(scale, 'scale'); _chk(shift, 'shift')
    assert tuple(scale.shape) == (n, c) and tuple(shift.shape) == (n, c), (scale.shape, shift.shape, (n, c))
    hi = torch.empty_like(y16.hi)
    check(_lib.lib().lp_adain_act16(y16.hi.data_ptr(), scale.data_ptr(), shift.data_ptr(), hi.data_ptr(), n, y16.hi.numel() // (n * c), c, int(relu),
                                    _stream()), 'lp_adain_act16')
    return Act16(hi, None, c, None)


def thin_wgrad16(x16: Act16, dy: Tensor, *, ksize: int, pro: int = 0, scale: Optional[Tensor] = None, shift: Optional[Tensor] = None,
                 splits: Optional[int] = None, sn=None, accum: Optional[Tensor] = None, bias_grad: bool = False):
    """``thin_wgrad`` of a conv with <= 4 OUTPUT channels whose wide input is a 16-bit-resident conv output (the generator head in the fp16 mode)"""
    _chk(dy, 'dy')
    n, h, w, cout = dy.shape
    cin = x16.c
    assert x16.lo is None and x16.inv is None and tuple(x16.hi.shape) == (n, h, w, cin)
    if splits is None:
        splits = default_splits(n, h, w, cin, cout)
    ws = torch.empty(_lib.lib().lp_conv_wgrad_workspace_bytes(cin, cout, ksize, splits) // 4, dtype=torch.float32, device=dy.device)
    dw = torch.empty((cout, cin, ksize, ksize), dtype=torch.float32, device=dy.device)
    with _Timed('wgrad_thin', 2.0 * n * h * w * cout * cin * ksize * ksize, (n, h, w, cin, cout, ksize, 0, pro)):
        check(_lib.lib().lp_thin_wgrad16(x16.hi.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), _p(scale), _p(shift), n, h, w, cin, cout,
                                         ksize, pro, splits, _stream()), 'lp_thin_wgrad16')
    dw = _sn_finish(dw, sn, accum)
    return (dw, dy.sum(dim=(0, 1, 2))) if bias_grad else dw


def y16_to_f32(y16: Act16) -> Tensor:
    """fp32 copy of a 16-bit-resident conv output (the rare consumers without a 16-bit form: statistics of a geometry the conv epilogue
    does not cover)"""
    return y16.hi.view(torch.float16)[..., :y16.c].float()


def norm_stats_finalize(st: ConvStats, n: int, c: int, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, *,
                        running_mean: Optional[Tensor] = None, running_var: Optional[Tensor] = None, momentum: float = 0.0):
    """(mean, rstd, scale, shift) [n, c] from the partials a conv epilogue wrote (``ConvStats``).  gamma/beta: [n, c] views (row stride
    free) or [c] (n == 1).  n == 1 with running statistics = train-mode BatchNorm."""
    dev = st.part.device
    out = torch.empty(4, n, c, dtype=torch.float32, device=dev)
    ab_stride = 0
    if gamma is not None:
        assert gamma.stride(-1) == 1 and beta.stride(-1) == 1
        ab_stride = gamma.stride(0) if gamma.dim() == 2 else c
        if beta.dim() == 2:
            assert beta.stride(0) == ab_stride
    assert n == st.images or n == 1, (n, st.images)
    rows = st.rows if n == st.images else st.rows * st.images       # n == 1 over several images: a BatchNorm over all pixels
    check(_lib.lib().lp_norm_stats_finalize(st.part.data_ptr(), rows, _p(gamma), _p(beta), ab_stride, eps, momentum, _p(running_mean),
                                            _p(running_var), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), n, c,
                                            _stream()), 'lp_norm_stats_finalize')
    if n == 1 and (gamma is None or gamma.dim() == 1):
        return out[0, 0], out[1, 0], out[2, 0], out[3, 0]
    return out[0], out[1], out[2], out[3]


def gconv_wgrad16(a: Act16, dy: Act16, group_size: int, *, prec: int, splits: Optional[int] = None) -> Tensor:
    """weight gradient [C, cg, 3, 3] of the grouped 3x3 conv (a = the planes the forward consumed, dy = packed output gradient)"""
    n, h, w = dy.nhw
    c = dy.c
    assert a.nhw == dy.nhw and a.c == c
    if splits is None:
        splits = max(1, min(512 // max(1, c // 64), (n * h * w + 127) // 128))
    ws = torch.empty(_lib.lib().lp_gconv_wgrad_workspace_bytes(c, splits) // 4, dtype=torch.float32, device=dy.hi.device)
    dw = torch.empty((c, group_size, 3, 3), dtype=torch.float32, device=dy.hi.device)
    pl = 4 if prec == PREC_BF16X3 else 2
    with _Timed('gconv_wgrad', 2.0 * n * h * w * c * group_size * 9, (n, h, w, group_size, c, 3, 0, 0), 2 * n * h * w * c * pl, mm=3 if prec == PREC_BF16X3 else 1):
        check(_lib.lib().lp_gconv16_wgrad(a.hi.data_ptr(), _p(a.lo), dy.hi.data_ptr(), _p(dy.lo), dw.data_ptr(), ws.data_ptr(), n, h, w, c,
                                          group_size, splits, prec, _p(dy.inv), _stream()), 'lp_gconv16_wgrad')
    return dw


def im2col_planes(x: Tensor, ksize: int, stride: int, pad: int, prec: int) -> Act16:
    """x [N,C,H,W] NCHW fp32 -> operand rows [N,Ho,Wo,K8] (K = C*k*k in nn.Conv2d weight order): a k x k conv becomes a 1x1 contraction"""
    _chk(x, 'x')
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    k = c * ksize * ksize
    hi, lo = _alloc16(n, ho, wo, k, prec, x.device)
    check(_lib.lib().lp_im2col_planes(x.data_ptr(), hi.data_ptr(), _p(lo), n, c, h, w, ksize, stride, pad, prec, _stream()), 'lp_im2col_planes')
    return Act16(hi, lo, k, None)


def bn_relu_maxpool(y: Tensor, scale: Tensor, shift: Tensor, prec: int, want_idx: bool = True):
    """MaxPool2d(3, 2, 1)(relu(y*scale[c]+shift[c])), y [N,H,W,C] -> (out fp32, its operand planes, argmax bytes | None)"""
    _chk(y, 'y')
    n, h, w, c = y.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty((n, ho, wo, c), dtype=torch.float32, device=y.device)
    hi, lo = _alloc16(n, ho, wo, c, prec, y.device)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=y.device) if want_idx else None
    check(_lib.lib().lp_bn_relu_maxpool_fwd(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), hi.data_ptr(), _p(lo), _p(idx),
                                            n, h, w, c, prec, _stream()), 'lp_bn_relu_maxpool_fwd')
    return out, Act16(hi, lo, c, None), idx


def maxpool_bwd(dout: Tensor, idx: Tensor, h: int, w: int) -> Tensor:
    _chk(dout, 'dout')
    n, ho, wo, c = dout.shape
    dA = torch.empty((n, h, w, c), dtype=torch.float32, device=dout.device)
    check(_lib.lib().lp_maxpool_bwd(dout.data_ptr(), idx.data_ptr(), dA.data_ptr(), n, h, w, c, _stream()), 'lp_maxpool_bwd')
    return dA


def bn_add_act(y: Tensor, scale: Tensor, shift: Tensor, res: Optional[Tensor] = None, res_scale: Optional[Tensor] = None,
               res_shift: Optional[Tensor] = None, relu: bool = True, prec: Optional[int] = None, want_out: bool = True, want_bits: bool = False):
    """out = relu?(y*scale[c]+shift[c] + (res | res*res_scale[c]+res_shift[c])) over [..., C]; with ``prec`` -> (out, Act16).
    ``res`` as ``Act16`` (bf16 / bf16x3 planes of the same mode as ``prec``): the residual is read from the operand planes (lp_bn_add_act_planes);
    ``want_out=False`` then skips the fp32 copy -> (None, Act16).  ``want_bits`` (with ``prec``): -> (out, Act16, bits), bits uint8 [..., C / 8] =
    the pattern "HI plane word > 0" as one bit per element (bit j of byte g: channel 8 g + j) -- what ``bn_bwd16`` (mask_mode 4) and
    ``conv16(res_bits=)`` read in the backward of a residual block."""
    assert not want_bits or prec is not None, 'want_bits: the pattern is the one of the operand planes'
    if isinstance(res, Act16):
        _chk(y, 'y')
        assert prec in (PREC_BF16, PREC_BF16X3) and res_scale is None and res.inv is None and (res.lo is not None) == (prec == PREC_BF16X3)
        assert tuple(res.hi.shape) == tuple(y.shape), (res.hi.shape, y.shape)
        c = y.shape[-1]
        out = torch.empty_like(y) if want_out else None
        hi = torch.empty(y.shape, dtype=torch.int16, device=y.device)
        lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
        bits = torch.empty(y.shape[:-1] + (c // 8,), dtype=torch.uint8, device=y.device) if want_bits else None
        check(_lib.lib().lp_bn_add_act_planes_bits(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.hi.data_ptr(), _p(res.lo), _p(out), hi.data_ptr(),
                                                   _p(lo), _p(bits), y.numel() // c, c, int(relu), prec, _stream()), 'lp_bn_add_act_planes')
        return (out, Act16(hi, lo, c, None), bits) if want_bits else (out, Act16(hi, lo, c, None))
    y16 = y if isinstance(y, Act16) else None
    if y16 is not None:          # 16-bit-resident conv output (fp16 mode)
        assert prec in (None, PREC_F16) and y16.lo is None and y16.inv is None
        shape, dev = y16.hi.shape, y16.hi.device
    else:
        _chk(y, 'y')
        shape, dev = y.shape, y.device
    c = shape[-1]
    p = 1
    for d in shape[:-1]:
        p *= d
    assert want_out or prec is not None
    out = torch.empty(shape, dtype=torch.float32, device=dev) if want_out else None
    hi = lo = None
    if prec is not None:
        hi = torch.empty(shape, dtype=torch.int16, device=dev)
        lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
    bits = torch.empty(tuple(shape[:-1]) + (c // 8,), dtype=torch.uint8, device=dev) if want_bits else None
    if res is not None:
        _chk(res, 'res'); assert res.shape == shape, (res.shape, shape)
    if y16 is not None:
        check(_lib.lib().lp_bn_add_act16_bits(y16.hi.data_ptr(), scale.data_ptr(), shift.data_ptr(), _p(res), _p(res_scale), _p(res_shift),
                                              _p(out), _p(hi), _p(bits), p, c, int(relu), _stream()), 'lp_bn_add_act16')
    else:
        check(_lib.lib().lp_bn_add_act_bits(y.data_ptr(), scale.data_ptr(), shift.data_ptr(), _p(res), _p(res_scale), _p(res_shift), _p(out),
                                            _p(hi), _p(lo), _p(bits), p, c, int(relu), prec if prec is not None else 0, _stream()), 'lp_bn_add_act')
    if want_bits:
        return out, Act16(hi, lo, c, None), bits
    return out if prec is None else (out, Act16(hi, lo, c, None))


def subsample2(x: Tensor) -> Tensor:
    """x [N,H,W,C] -> x[:, ::2, ::2] contiguous (fp32 or int16 planes with C*itemsize % 16 == 0)"""
    n, h, w, c = x.shape
    assert x.is_contiguous()
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=x.dtype, device=x.device)
    check(_lib.lib().lp_subsample2(x.data_ptr(), out.data_ptr(), n, h, w, c * x.element_size(), _stream()), 'lp_subsample2')
    return out


def subsample2_16(a: Act16) -> Act16:
    return Act16(subsample2(a.hi), None if a.lo is None else subsample2(a.lo), a.c, a.inv)


def zero_stuff2_16(a: Act16, h: int, w: int) -> Act16:
    """adjoint of ``subsample2`` on operand planes: [N,ceil(h/2),ceil(w/2),C8] -> [N,h,w,C8], zeros at the odd positions"""
    n, hs, ws_, c8 = a.hi.shape
    assert hs == (h + 1) // 2 and ws_ == (w + 1) // 2

    def one(t):
        out = torch.empty((n, h, w, c8), dtype=t.dtype, device=t.device)
        check(_lib.lib().lp_zero_stuff2(t.data_ptr(), out.data_ptr(), n, h, w, c8 * t.element_size(), _stream()), 'lp_zero_stuff2')
        return out
    return Act16(one(a.hi), None if a.lo is None else one(a.lo), a.c, a.inv)


def add_strided2(d: Tensor, s: Tensor) -> Tensor:
    """d[:, ::2, ::2] += s, in place (fp32 NHWC)"""
    _chk(d, 'd'); _chk(s, 's')
    n, h, w, c = d.shape
    assert s.shape == (n, (h + 1) // 2, (w + 1) // 2, c)
    check(_lib.lib().lp_add_strided2(d.data_ptr(), s.data_ptr(), n, h, w, c, _stream()), 'lp_add_strided2')
    return d


def proj_score_fwd(out: Tensor, embed: Optional[Tensor]):
    """critic head: out [N,H,W,C] -> (pooled = sum_hw relu(out) [N,C], dot = <pooled, embed> [N] | None), one launch"""
    _chk(out, 'out')
    n, h, w, c = out.shape
    if embed is not None:
        _chk(embed, 'embed'); assert tuple(embed.shape) == (n, c)
    pooled = torch.empty((n, c), dtype=torch.float32, device=out.device)
    dot = torch.empty((n,), dtype=torch.float32, device=out.device) if embed is not None else None
    check(_lib.lib().lp_proj_score_fwd(out.data_ptr(), _p(embed), pooled.data_ptr(), _p(dot), n, h * w, c, _stream()), 'lp_proj_score_fwd')
    return pooled, dot


def proj_score_bwd(out: Tensor, embed: Optional[Tensor], pooled: Tensor, g_pooled: Optional[Tensor], g_dot: Optional[Tensor], want_out: bool, want_embed: bool):
    n, h, w, c = out.shape
    for t, nm in ((g_pooled, 'g_pooled'), (g_dot, 'g_dot')):
        if t is not None:
            _chk(t, nm)
    d_out = torch.empty_like(out) if want_out else None
    d_embed = torch.empty_like(pooled) if (want_embed and g_dot is not None) else None
    check(_lib.lib().lp_proj_score_bwd(out.data_ptr(), _p(embed), pooled.data_ptr(), _p(g_pooled), _p(g_dot if embed is not None else None), _p(d_out),
                                       _p(d_embed), n, h * w, c, _stream()), 'lp_proj_score_bwd')
    return d_out, d_embed


def image_prep_fwd(x: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """x NCHW [N,3,H,W] in [-1, 1] -> ((x + 1) / 2 - mean) / std as NHWC [N,H,W,3] (one launch)"""
    _chk(x, 'x'); _chk(mean, 'mean'); _chk(std, 'std')
    n, c, h, w = x.shape
    assert c == 3 and mean.numel() == 3 and std.numel() == 3
    out = torch.empty((n, h, w, 3), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_image_prep_fwd(x.data_ptr(), mean.data_ptr(), std.data_ptr(), out.data_ptr(), n, h * w, _stream()), 'lp_image_prep_fwd')
    return out


def image_prep_bwd(g: Tensor, std: Tensor) -> Tensor:
    _chk(g, 'g')
    n, h, w, c = g.shape
    assert c == 3
    dx = torch.empty((n, 3, h, w), dtype=torch.float32, device=g.device)
    check(_lib.lib().lp_image_prep_bwd(g.data_ptr(), std.data_ptr(), dx.data_ptr(), n, h * w, _stream()), 'lp_image_prep_bwd')
    return dx


def spatial_mean(x: Tensor) -> Tensor:
    _chk(x, 'x')
    n, h, w, c = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_spatial_mean_fwd(x.data_ptr(), out.data_ptr(), n, h * w, c, _stream()), 'lp_spatial_mean_fwd')
    return out


def spatial_mean_bwd(g: Tensor, h: int, w: int) -> Tensor:
    _chk(g, 'g')
    n, c = g.shape
    dx = torch.empty((n, h, w, c), dtype=torch.float32, device=g.device)
    check(_lib.lib().lp_spatial_mean_bwd(g.data_ptr(), dx.data_ptr(), n, h * w, c, _stream()), 'lp_spatial_mean_bwd')
    return dx


# ---- MobileNetV2 backward: depthwise 3x3 ------------------------------------------------------------------------------------------
def dwconv3x3_dgrad(dy: Tensor, w: Tensor, h: int, wd: int, stride: int) -> Tensor:
    """gradient w.r.t. the activated input of ``dwconv3x3`` ([N,h,wd,C]) from dy [N,ceil(h/s),ceil(wd/s),C]"""
    _chk(dy, 'dy'); _chk(w, 'w')
    n, ho, wo, c = dy.shape
    assert ho == (h + stride - 1) // stride and wo == (wd + stride - 1) // stride and w.numel() == c * 9
    da = torch.empty((n, h, wd, c), dtype=torch.float32, device=dy.device)
    check(_lib.lib().lp_dwconv3x3_dgrad(dy.data_ptr(), w.data_ptr(), da.data_ptr(), n, h, wd, c, stride, _stream()), 'lp_dwconv3x3_dgrad')
    return da


def dwconv3x3_wgrad(x: Tensor, dy: Tensor, stride: int, in_scale: Optional[Tensor] = None, in_shift: Optional[Tensor] = None) -> Tensor:
    """weight gradient [C,1,3,3] of ``dwconv3x3`` (x = its raw input, activation relu6(x*in_scale+in_shift) recomputed on load)"""
    _chk(x, 'x'); _chk(dy, 'dy')
    n, h, wd, c = x.shape
    dw = torch.empty((c, 1, 3, 3), dtype=torch.float32, device=x.device)
    ws = torch.empty(_lib.lib().lp_dwconv3x3_wgrad_workspace_bytes(c) // 4, dtype=torch.float32, device=x.device)
    check(_lib.lib().lp_dwconv3x3_wgrad(x.data_ptr(), _p(in_scale), _p(in_shift), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), n, h, wd, c,
                                        stride, _stream()), 'lp_dwconv3x3_wgrad')
    return dw


def _mask16_mode(mask_mode: int, mask_src) -> int:
    """lp_bn_bwd16_h's mask mode for ``mask_src`` given as mode 2: 3 = its 16-bit planes (2 B per element), 4 = its one-bit pattern"""
    if isinstance(mask_src, Act16):
        assert mask_mode == 2, mask_mode
        return 3
    if mask_src is not None and mask_src.dtype == torch.uint8:
        assert mask_mode == 2, mask_mode
        return 4
    return mask_mode


def bn_bwd16(dA: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, scale: Tensor, shift: Tensor, *, prec: int, mask_mode: int = 0,
             mask_src: Optional[Tensor] = None, want_g: bool = False, act_hi: float = 0.0, frozen: bool = False):
    """backward of act(BatchNorm(x)) over x [..., C] written straight to the OPERAND PLANES of dy (what the weight / data gradient
    contractions consume): -> (Act16 of dy, dgamma [C], dbeta [C], g | None).  No fp32 dy, no masked-gradient temporary; in fp16 mode the
    planes carry the power-of-two scale of lp_bn_bwd16 (``Act16.inv``).  Arguments as ``norm_act_bwd``; ``x`` may be a 16-bit-resident
    conv output (``Act16``, fp16 mode) and ``mask_src`` (mask_mode 2) the operand planes of the activated tensor instead of its fp32 copy, or
    (uint8 [..., C / 8]) its one-bit pattern from ``bn_add_act(want_bits=True)``."""
    shape, p, c, mptr = _flat_pc(dA, x, mask_src)
    x16 = x if isinstance(x, Act16) else None          # 16-bit-resident conv output (fp16 mode)
    assert c % 8 == 0 and (x16 is None or (prec == PREC_F16 and x16.lo is None and x16.inv is None)), (c, prec)
    mask_mode = _mask16_mode(mask_mode, mask_src)
    dev = dA.device
    hi = torch.empty(shape, dtype=torch.int16, device=dev)
    lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
    small = torch.empty(2 + 2 * c, dtype=torch.float32, device=dev)
    sc, dg, db = small[:2], small[2:2 + c], small[2 + c:]
    g = torch.empty(shape, dtype=torch.float32, device=dev) if want_g else None
    ws = torch.empty(_lib.lib().lp_bn_bwd16_workspace_bytes(p, c) // 4, dtype=torch.float32, device=dev)
    check(_lib.lib().lp_bn_bwd16_h(dA.data_ptr(), None if x16 is not None else x.data_ptr(), None if x16 is None else x16.hi.data_ptr(), mptr,
                                   gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), hi.data_ptr(), _p(lo),
                                   sc.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), p, c, mask_mode, float(act_hi), int(frozen), prec,
                                   _p(g), _stream()), 'lp_bn_bwd16')
    return Act16(hi, lo, c, sc[1:] if prec == PREC_F16 else None), dg, db, g



def bn_bwd16_dual(dA: Tensor, xa, bn_a, xb, bn_b, *, prec: int, mask_src, frozen: bool = False):
    """``bn_bwd16`` of TWO BatchNorms that receive the same gradient and the same ReLU pattern -- out = relu(BN_a(xa) + BN_b(xb)): bn3 and the
    downsample BatchNorm of a residual block -- in one pass pair (lp_bn_bwd16_dual): dA and the pattern are read once per pass.  ``bn_a`` / ``bn_b``:
    (gamma, mean, rstd); ``mask_src`` as ``bn_bwd16``'s with mask_mode 2 (fp32, ``Act16`` or the uint8 bit pattern).  -> ((Act16, dgamma, dbeta) of a,
    the same of b), bit-identical to two ``bn_bwd16`` calls.  xa and xb must both be fp32 or both 16-bit resident."""
    shape, p, c, mptr = _flat_pc(dA, xa, mask_src)
    _flat_pc(dA, xb, None)
    x16 = isinstance(xa, Act16)
    assert x16 == isinstance(xb, Act16), 'bn_bwd16_dual: both x as fp32 or both 16-bit resident'
    assert c % 8 == 0 and (not x16 or (prec == PREC_F16 and xa.lo is None and xa.inv is None and xb.lo is None and xb.inv is None)), (c, prec)
    mask_mode = _mask16_mode(2, mask_src)
    dev = dA.device
    ws_floats = _lib.lib().lp_bn_bwd16_workspace_bytes(p, c) // 4
    res, args = [], []
    for x, (gamma, mean, rstd) in ((xa, bn_a), (xb, bn_b)):
        hi = torch.empty(shape, dtype=torch.int16, device=dev)
        lo = torch.empty_like(hi) if prec == PREC_BF16X3 else None
        small = torch.empty(2 + 2 * c, dtype=torch.float32, device=dev)
        sc, dg, db = small[:2], small[2:2 + c], small[2 + c:]
        ws = torch.empty(ws_floats, dtype=torch.float32, device=dev)
        args += [None if x16 else x.data_ptr(), x.hi.data_ptr() if x16 else None, gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), hi.data_ptr(), _p(lo),
                 sc.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr()]
        res.append((Act16(hi, lo, c, sc[1:] if prec == PREC_F16 else None), dg, db, ws))
    check(_lib.lib().lp_bn_bwd16_dual(dA.data_ptr(), mptr, *args, p, c, mask_mode, int(frozen), prec, _stream()), 'lp_bn_bwd16_dual')
    return res[0][:3], res[1][:3]
