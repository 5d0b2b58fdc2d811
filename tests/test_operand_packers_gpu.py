"""The operand packers -- lp_act_pack, lp_amax_partial, lp_pack_weights (+ _batch / _pairs), lp_pack_grouped -- against the independent restatement of
tests/operand_restatement.py (proved on the CPU by tests/test_operand_packers_cpu.py), WORD FOR WORD unless a test says otherwise.  Every other test
that decodes what these packers wrote, or requires another kernel to write "what lp_act_pack would write", inherits this anchor.

Two identifications, and no other excuse for any element:
  * a NaN is compared by NaN-ness only (the payload is the hardware's);
  * in LOGICAL channels +0 and -0 are the same word (fmaxf(-0, +0) may return either).  Pad channels, rows and columns must be exactly 0x0000.
Every 16-bit buffer a wrapper allocates is poisoned with 0x7fff (a NaN in both formats) before the kernel runs, so an unwritten word fails
(tests/guarded_alloc.py, which also fences every such buffer and checks the fences after each test).

Kept out of the bit-exact input sets, because their outcome rests on hardware modes nobody has measured on this part:
  * fp32 SUBNORMAL inputs (the denormal mode of the conversion instructions);
  * nothing else: the "grid" sets (operand_restatement.grid_set) make every affine exact in fp32 whether the compiler fuses it or not, the "random"
    sets use arbitrary normal fp32 values and rely on the restatement's correctly rounded fused multiply-add."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import operand_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0x7fff
PRECS = [0, 1, 2]


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def _lib():
    from latent_pose_reenactment_amd import _lib
    return _lib.lib()


from guarded_alloc import fence_fixture  # noqa: E402

# the shared harness (tests/guarded_alloc.py, fill A): every buffer a wrapper takes from torch.empty / empty_like is full of NaN-like words -- 0x7fff
# in the int16 planes, as before -- and now also sits between two fences that are checked when the test is over
poisoned_planes = fence_fixture('A')


def test_the_poison_reaches_the_wrappers_buffers():
    hi, lo = _ops()._alloc16(1, 2, 2, 3, 1, 'cuda')
    assert (hi == POISON).all() and (lo == POISON).all()


def words(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint16)


def check_words(got, want, prec, logical, what):
    """got == want word for word; NaN by NaN-ness (and never the poison), signed zeros identified where ``logical`` (bool, broadcastable) is set"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_w = R.is_nan_word(want, prec)
    ok = (got == want) | (nan_w & R.is_nan_word(got, prec) & (got != POISON))
    ok |= np.broadcast_to(logical, got.shape) & (((got | want) & np.uint16(0x7FFF)) == 0)
    if not ok.all():
        bad = np.argwhere(~ok)
        first = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} words differ; first at {first}: got 0x{int(got[first]):04x}, want 0x{int(want[first]):04x}')


def check_planes(a, want_hi, want_lo, prec, c, what):
    n, h, w, c8 = a.hi.shape
    logical = np.arange(c8) < c
    check_words(words(a.hi).reshape(n, h * w, c8), want_hi, prec, logical, what + ' hi')
    assert (a.lo is None) == (prec != 1)
    if a.lo is not None:
        check_words(words(a.lo).reshape(n, h * w, c8), want_lo, 0, logical, what + ' lo')


def affine_for(pro, rng, n, c, grid, x_shape):
    """(x, scale, shift) of a prologue: per image [N][C] for pro 1, per channel [C] for 3 .. 5, none for 0 / 2"""
    sshape = (n, c) if pro == 1 else (c,)
    if grid:
        x, sc, sf = R.grid_set(rng, x_shape, sshape)
    else:
        x, sc, sf = (rng.standard_normal(s).astype(np.float32) for s in (x_shape, sshape, sshape))
        x *= 3
    return (x, sc, sf) if pro in (1, 3, 4, 5) else (x, None, None)


def run_act_pack(x, pro, sc, sf, prec):
    dev = lambda t: None if t is None else torch.from_numpy(t).cuda()
    return _ops().act_pack(dev(x), pro=pro, scale=dev(sc), shift=dev(sf), prec=prec)


# ---- a. lp_act_pack --------------------------------------------------------------------------------------------------------------------
ACT_SHAPES = [
    (2, 4, 4, 64),        # vector loads, G = 8 a power of two: the group is fixed per thread
    (2, 16, 16, 24),      # G = 3, one block of 256 threads: the group is NOT fixed, the affine is reloaded per item
    (2, 32, 32, 24),      # G = 3, 3 blocks (stride 768): group fixed with a non-power-of-two G
    (3, 5, 7, 3),         # scalar loads, 5 pad channels
    (2, 8, 8, 12),        # vector-eligible C whose last group falls back to scalar loads with 4 pads
    (1, 9, 11, 70),       # C % 4 != 0, G = 9
]


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('pro', range(6))
@pytest.mark.parametrize('shape', ACT_SHAPES)
def test_act_pack_grid_set(shape, pro, prec):
    n, h, w, c = shape
    x, sc, sf = affine_for(pro, np.random.default_rng(100 + pro), n, c, True, shape)
    a = run_act_pack(x, pro, sc, sf, prec)
    want_hi, want_lo = R.planes(x, pro, sc, sf, prec)
    check_planes(a, want_hi, want_lo, prec, c, f'act_pack {shape} pro {pro} prec {prec}')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('pro', [1, 3, 4, 5])
@pytest.mark.parametrize('shape', [(2, 16, 16, 24), (1, 9, 11, 70)])
def test_act_pack_random_set(shape, pro, prec):
    """arbitrary normal fp32 inputs: the affine is one fused multiply-add, rounded once (the restatement's fma32)"""
    n, h, w, c = shape
    x, sc, sf = affine_for(pro, np.random.default_rng(200 + pro), n, c, False, shape)
    a = run_act_pack(x, pro, sc, sf, prec)
    want_hi, want_lo = R.planes(x, pro, sc, sf, prec)
    check_planes(a, want_hi, want_lo, prec, c, f'act_pack random {shape} pro {pro} prec {prec}')


def test_act_pack_grid_cap_second_trip():
    """(512, 32, 32, 72): the grid is capped at ceil(4096 / N) = 8 blocks per image for 9216 items, so a thread makes a SECOND trip through its loop
    and the clamped-load tail is live -- what the 256^2 training layers do; the smallest tensor that reaches it.  pro 1 (per-image affine), all modes."""
    n, h, w, c = 512, 32, 32, 72
    x, sc, sf = affine_for(1, np.random.default_rng(300), n, c, True, (n, h * w, c))
    xd, scd, sfd = (torch.from_numpy(t).cuda() for t in (x, sc, sf))
    q = R.act(x, 1, sc, sf)
    for prec in PRECS:
        a = _ops().act_pack(xd.view(n, h, w, c), pro=1, scale=scd, shift=sfd, prec=prec)
        hi, lo = R.split(q, prec)
        check_planes(a, hi, lo, prec, c, f'act_pack grid cap prec {prec}')
        del a


EDGE_WORDS_F16 = {7e4: 0x7BFF, np.inf: 0x7BFF, -np.inf: 0xFBFF, 65520.0: 0x7BFF, -65520.0: 0xFBFF, 65504.0: 0x7BFF, 2.0 ** -14: 0x0400, 2.0 ** -24: 0x0001,
                  2.0 ** -25: 0x0000, 3 * 2.0 ** -25: 0x0002, 5 * 2.0 ** -25: 0x0002, 1.75 * 2.0 ** -24: 0x0002, 1 + 2.0 ** -11: 0x3C00, 1 + 3 * 2.0 ** -11: 0x3C02,
                  1e-30: 0x0000}
EDGE_WORDS_BF16 = {1 + 2.0 ** -8: 0x3F80, 1 + 3 * 2.0 ** -8: 0x3F82, -(1 + 2.0 ** -8): 0xBF80, -(1 + 3 * 2.0 ** -8): 0xBF82, np.inf: 0x7F80, -np.inf: 0xFF80,
                   65520.0: 0x4780}


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('pro', [0, 2])
def test_act_pack_edge_tensor(pro, prec):
    """(1, 1, 64, 8): ties go to even in bf16 and fp16, 7e4 and +-inf saturate to +-65504 in fp16 (and stay infinite in bf16), a NaN is kept in every
    mode -- through relu(x) too --, results under 2^-14 round GRADUALLY to fp16 subnormals.  fp32-subnormal inputs are left out (module docstring).
    (This test found lp_act_pack's clamp returning its bound for a NaN -- -65504 / -3e38 under prologue 0, zero under the ReLUs -- and +-inf clamped to
    +-3e38 in the bf16 modes; the conversions themselves behaved as claimed.  DESIGN.md section 2.)"""
    e = R.edge_values(False)
    x = np.zeros((1, 1, 64, 8), dtype=np.float32)
    x.reshape(-1)[:len(e)] = e
    x.reshape(-1)[len(e):2 * len(e)] = e[::-1]
    a = run_act_pack(x, pro, None, None, prec)
    want_hi, want_lo = R.planes(x, pro, prec=prec)
    check_planes(a, want_hi, want_lo, prec, 8, f'act_pack edges pro {pro} prec {prec}')
    got = words(a.hi).reshape(-1)
    assert R.is_nan_word(got[np.isnan(x.reshape(-1))], prec).all() and np.isnan(x).sum() == 4
    if pro == 0:                                                     # the IEEE facts as literal words, independent of the restatement
        for v, word in (EDGE_WORDS_F16 if prec == 2 else EDGE_WORDS_BF16).items():
            idx = np.nonzero(x.reshape(-1) == np.float32(v))[0]
            assert len(idx) and (got[idx] == word).all(), (v, [hex(int(g)) for g in got[idx]], hex(word))


@pytest.mark.parametrize('prec', PRECS)
def test_act_pack_relu6_clamps_at_exactly_6(prec):
    x = np.zeros((1, 1, 8, 8), dtype=np.float32)
    x.reshape(-1)[:8] = [6.0, 6.0 + 2.0 ** -21, 5.96875, 7.0, 1e30, -1.0, 3.0, np.inf]
    sc, sf = np.ones(8, dtype=np.float32), np.zeros(8, dtype=np.float32)
    a = run_act_pack(x, 3, sc, sf, prec)
    want_hi, want_lo = R.planes(x, 3, sc, sf, prec)
    check_planes(a, want_hi, want_lo, prec, 8, f'relu6 prec {prec}')
    got = R.decode(words(a.hi), None if a.lo is None else words(a.lo), prec).reshape(-1)[:8]
    assert got.tolist() == [6.0, 6.0, 5.96875, 6.0, 6.0, 0.0, 3.0, 6.0]


def raw_act_pack(x, prec, in_scale=None, amax_part=None, amax_count=0, amax_stride=1, scale_out=None):
    """lp_act_pack through the raw ctypes ABI (prologue 0) into poisoned planes"""
    n, h, w, c = x.shape
    c8 = (c + 7) // 8 * 8
    hi = torch.empty((n, h, w, c8), dtype=torch.int16, device='cuda')
    lo = torch.empty_like(hi) if prec == 1 else None
    p = lambda t: None if t is None else t.data_ptr()
    rc = _lib().lp_act_pack(x.data_ptr(), None, None, 0, hi.data_ptr(), p(lo), n, h * w, c, prec, p(in_scale), p(amax_part), amax_count, amax_stride,
                            p(scale_out), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().lp_last_error()
    return _ops().Act16(hi, lo, c, None)


@pytest.mark.parametrize('prec', PRECS)
def test_act_pack_in_scale_through_the_raw_abi(prec):
    """hipops.act_pack never passes in_scale: one call through the C ABI with a device scalar 0.5"""
    x = R.grid_set(np.random.default_rng(400), (2, 5, 7, 12), (1,))[0]
    a = raw_act_pack(torch.from_numpy(x).cuda(), prec, in_scale=torch.tensor([0.5], device='cuda'))
    want_hi, want_lo = R.planes(x, 0, prec=prec, in_scale=0.5)
    assert not np.array_equal(want_hi, R.planes(x, 0, prec=prec)[0])
    check_planes(a, want_hi, want_lo, prec, 12, f'in_scale prec {prec}')


# ---- b. fp16 gradient scaling and lp_amax_partial ------------------------------------------------------------------------------------------
# the issue's sizes cover tail-only (1, 3), no tail (4), a tail behind one vector (5), the single-stride loop (1023, 4*1024*256+7: 262145 vectors against a
# stride of 1024 blocks x 256 threads = 262144); the 4-deep loop needs MORE than 3 strides of vectors, so 4*4*1024*256+7 is added for it
AMAX_NUMEL = [1, 3, 4, 5, 1023, 4 * 1024 * 256 + 7, 4 * 4 * 1024 * 256 + 7]


@pytest.mark.parametrize('numel', AMAX_NUMEL)
def test_amax_partial_is_the_exact_maximum(numel):
    """max(part) == max|x| exactly, every partial written; the maximum is a NEGATIVE value at the first element, the last one, inside the tail"""
    rng = np.random.default_rng(500)
    base = rng.uniform(-1, 1, size=numel).astype(np.float32)
    spots = {0, numel - 1}
    if numel % 4:
        spots.add(numel // 4 * 4)                                    # first element of the scalar tail
    nblocks = _lib().lp_amax_blocks()
    for pos in sorted(spots):
        x = base.copy()
        x[pos] = -3.5
        part = torch.full((nblocks,), -1.0, device='cuda')
        xd = torch.from_numpy(x).cuda()
        rc = _lib().lp_amax_partial(xd.data_ptr(), numel, part.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib().lp_last_error()
        p = part.cpu().numpy()
        assert (p >= 0).all(), 'a partial was not written'
        assert p.max() == np.float32(3.5) == np.abs(x).max(), (numel, pos, p.max())
        x[pos] = base[pos]
        if pos == 0:                                                 # and without the planted value: the plain maximum of the random data
            xd = torch.from_numpy(x).cuda()
            _lib().lp_amax_partial(xd.data_ptr(), numel, part.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert part.max().item() == float(np.abs(x).max())


@pytest.mark.parametrize('amax', [1.0, 0.75, 4096.0, 3e-30, 0.0])
def test_fp16_gradient_scale_and_planes(amax):
    """grad=True, fp16: s = amax_scale(max|x|) exactly -- through hipops (Act16.inv) and through the raw ABI (scale_out = {s, 1/s}) --, the planes are
    f16_sat(x * s) (a power-of-two product: exact), and the largest scaled magnitude decodes into [2^12, 2^13) whenever the exponent clamp (+-100,
    reached by 3e-30) does not bite.  The all-zero tensor gives s = 1 and all-zero planes."""
    rng = np.random.default_rng(600)
    shape = (2, 6, 5, 20)
    g = (rng.integers(-255, 256, size=shape) / 256.0).astype(np.float32)           # |g| < 1 on a 2^-8 grid; the smallest non-zero |x| stays a normal fp32
    x = (g * np.float32(amax)).astype(np.float32)
    x[1, 2, 3, 4] = -np.float32(amax)
    m = np.abs(x).max()
    assert m == np.float32(amax)
    s, inv = R.amax_scale(m)
    want = np.zeros((2, 30, 24), dtype=np.uint16)
    want[:, :, :20] = R.f16_sat(x.reshape(2, 30, 20) * s)
    xd = torch.from_numpy(x).cuda()
    a = _ops().act_pack(xd, prec=2, grad=True)
    assert a.inv is not None and a.inv[0].item() == float(inv)
    check_planes(a, want, None, 2, 20, f'grad planes amax {amax}')
    nblocks = _lib().lp_amax_blocks()
    part, so = torch.full((nblocks,), -1.0, device='cuda'), torch.full((2,), -1.0, device='cuda')
    assert _lib().lp_amax_partial(xd.data_ptr(), x.size, part.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    b = raw_act_pack(xd, 2, amax_part=part, amax_count=nblocks, amax_stride=1, scale_out=so)
    assert so.tolist() == [float(s), float(inv)]
    check_planes(b, want, None, 2, 20, f'grad planes (raw) amax {amax}')
    top = np.abs(R.decode(words(a.hi), None, 2)).max()
    if amax == 0.0:
        assert s == 1 and not (words(a.hi) & np.uint16(0x7FFF)).any()
    elif amax == 3e-30:
        assert s == np.float32(2.0 ** 100) and top == R.f16_decode(R.f16_sat(np.float32(3e-30) * s)).item()        # 13 - e = 111: clamped to 100
    else:
        assert 2.0 ** 12 <= top < 2.0 ** 13, top


# ---- c. lp_pack_weights ------------------------------------------------------------------------------------------------------------------
def grid_weights(rng, shape):
    """multiples of 2^-10 in [-2, 2): every tap sum of modes 2 .. 5 is exact in fp32 whatever the order; exact zeros and bf16 ties included"""
    w = (rng.integers(-2048, 2048, size=shape) / 1024.0).astype(np.float32)
    f = w.reshape(-1)
    f[:6] = [0.0, 1 + 2.0 ** -8, -(1 + 3 * 2.0 ** -8), 0.0, 1 + 2.0 ** -9 + 2.0 ** -10, -0.0]
    return w


def check_pack(pk, want_hi, want_lo, prec, what):
    logical = np.zeros(want_hi.shape, dtype=bool)
    logical[:, :pk.rows, :pk.cols] = True
    check_words(words(pk.hi), want_hi, prec, logical, what + ' hi')
    assert (pk.lo is None) == (prec != 1)
    if pk.lo is not None:
        check_words(words(pk.lo), want_lo, 0, logical, what + ' lo')


WEIGHT_SHAPES = [(70, 12, 3, True), (70, 12, 3, False), (130, 40, 3, False), (24, 16, 1, False), (4, 64, 3, False)]


WEIGHT_CASES = [(s, m) for s in WEIGHT_SHAPES for m in range(6) if s[2] == 3 or m < 2]          # modes 2 .. 5 are forms of a 3x3 weight


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('shape,mode', WEIGHT_CASES)
def test_pack_weights(shape, mode, prec):
    cout, cin, k, small_k = shape
    w = grid_weights(np.random.default_rng(700 + mode), (cout, cin, k, k))
    pk = _ops().pack_weights(torch.from_numpy(w).cuda(), mode, prec, small_k=small_k)
    want_hi, want_lo = R.weight_pack(w, mode, pk.rows_p, pk.cols_p, prec)
    assert pk.hi.shape == want_hi.shape and (pk.rows, pk.cols) == ((cout, cin) if mode in (0, 2, 4) else (cin, cout))
    check_pack(pk, want_hi, want_lo, prec, f'pack_weights {shape} mode {mode} prec {prec}')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('mode', [2, 4])
def test_pack_weights_random_tap_sums_by_value(mode, prec):
    """random normal weights: the fp32 tap sums depend on the order of the additions, so this one is VALUE-wise -- the decoded hi (+ lo) lies within
    half an operand ulp of the fp64 tap sum (bf16: 2^(e-8), fp16: 2^(e-11), hi + lo: 2^-16 |v|, csrc/lp_common.h) plus 3 * 2^-24 * sum|w| for the at most
    three fp32 additions (each rounds by half an ulp of a partial sum <= sum|w|).  Truncation would exceed the first term; pads are exact zeros."""
    rng = np.random.default_rng(800 + mode)
    w = rng.standard_normal((70, 12, 3, 3)).astype(np.float32)
    pk = _ops().pack_weights(torch.from_numpy(w).cuda(), mode, prec)
    ref = R.weight_values(w.astype(np.float64), mode)
    slack = 3 * 2.0 ** -24 * R.weight_values(np.abs(w).astype(np.float64), mode)      # sum|w| of the taps (mode 4: times the exact 1/4 the sum is scaled by)
    got = R.decode(words(pk.hi), None if pk.lo is None else words(pk.lo), prec)
    body = got[:, :70, :12]
    e = np.floor(np.log2(np.abs(ref) + slack))
    half_ulp = {0: 2.0 ** (e - 8), 1: 2.0 ** -16 * (np.abs(ref) + slack), 2: np.maximum(2.0 ** (e - 11), 2.0 ** -25)}[prec]
    err = np.abs(body - ref)
    print(f'[pack by value] mode {mode} prec {prec}: worst err / bound {float((err / (half_ulp + slack)).max()):.3f}')
    assert (err <= half_ulp + slack).all()
    got[:, :70, :12] = 0
    assert not got.any()
    for plane in (pk.hi, pk.lo):
        assert plane is None or not (words(plane)[:, 70:].any() or words(plane)[:, :, 12:].any())


# ---- d. PackBatch: lp_pack_weights_batch / lp_pack_weights_pairs -------------------------------------------------------------------------
@pytest.mark.parametrize('prec', [1, 2])
def test_pack_batch_against_the_restatement(prec):
    """one batch, ten entries, 8 .. 1280 chunks: three paired weights (ragged 3x3, ragged 1x1, a 4-row 3x3: first, middle and last entry of the pair
    kernel's binary search over tile0) and four singles through the batch kernel (a 1x1 forward pack, a forward-only small-k pack, a mode-2 and a
    large mode-4 image: first, middle and last entry of its search over chunk0) -- each held to weight_pack() directly"""
    ops = _ops()
    rng = np.random.default_rng(900)
    mk = lambda *s: torch.from_numpy(grid_weights(rng, s)).cuda()
    pairs = [mk(70, 130, 3, 3), mk(24, 16, 1, 1), mk(4, 64, 3, 3)]
    specs = [(mk(8, 8, 1, 1), 0, False), (mk(32, 8, 3, 3), 0, True)]
    specs += [(w, 0, False) for w in pairs]
    specs += [(mk(12, 70, 3, 3), 2, False)]
    specs += [(w, 1, w.shape[0] <= 32 and w.shape[2] == 3) for w in pairs]
    specs += [(mk(256, 320, 3, 3), 4, False)]
    pb = ops.PackBatch(specs, prec)
    assert pb.npair == 3 and pb.nsingle == 4 and len(specs) == 10
    sizes = [pk.taps * pk.rows_p * pk.cols_p for pk in pb.packs]
    assert max(sizes) > 100 * min(sizes)
    for pk in pb.packs:
        assert (pk.hi == POISON).all() and (pk.lo is None or (pk.lo == POISON).all())
    got = pb.update()
    for (w, mode, sk), pk in zip(specs, got):
        want_hi, want_lo = R.weight_pack(w.cpu().numpy(), mode, pk.rows_p, pk.cols_p, prec)
        check_pack(pk, want_hi, want_lo, prec, f'PackBatch {tuple(w.shape)} mode {mode} prec {prec}')


# ---- e. lp_pack_grouped ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('c,cg', [(64, 4), (128, 4), (128, 32), (64, 64)])
def test_pack_grouped(c, cg, mode, prec):
    w = grid_weights(np.random.default_rng(1000 + mode), (c, cg, 3, 3))
    pk = _ops().pack_grouped(torch.from_numpy(w).cuda(), mode, prec)
    want_hi, want_lo = R.grouped_pack(w, cg, pk.rows_p, mode, prec)
    in_group = R.grouped_values(np.ones_like(w), cg, pk.rows_p, mode) != 0          # the words that hold a weight; everything else must be 0x0000
    check_words(words(pk.hi), want_hi, prec, in_group, f'pack_grouped {c}/{cg} mode {mode} prec {prec} hi')
    if prec == 1:
        check_words(words(pk.lo), want_lo, 0, in_group, f'pack_grouped {c}/{cg} mode {mode} lo')


@pytest.mark.parametrize('prec', PRECS)
@pytest.mark.parametrize('mode', [0, 1])
def test_pack_grouped_pad_rows_through_the_raw_abi(mode, prec):
    """C = 192 into CP = 256 (hipops.pack_grouped only ever pads to the next multiple of 128): rows 192 .. 255 are zero words"""
    c, cg, cp = 192, 8, 256
    w = grid_weights(np.random.default_rng(1100 + mode), (c, cg, 3, 3))
    wd = torch.from_numpy(w).cuda()
    hi = torch.empty((9, cp, 64), dtype=torch.int16, device='cuda')
    lo = torch.empty_like(hi) if prec == 1 else None
    rc = _lib().lp_pack_grouped(wd.data_ptr(), hi.data_ptr(), None if lo is None else lo.data_ptr(), c, cg, cp, mode, int(prec == 2),
                                torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().lp_last_error()
    want_hi, want_lo = R.grouped_pack(w, cg, cp, mode, prec)
    in_group = R.grouped_values(np.ones_like(w), cg, cp, mode) != 0
    check_words(words(hi), want_hi, prec, in_group, f'pack_grouped raw mode {mode} prec {prec} hi')
    assert not words(hi)[:, c:].any()
    if lo is not None:
        check_words(words(lo), want_lo, 0, in_group, 'pack_grouped raw lo')
        assert not words(lo)[:, c:].any()
