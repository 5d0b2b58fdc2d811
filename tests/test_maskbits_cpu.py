"""CPU side of the one-bit ReLU pattern (LP_E_MASKBITS): the packing rule itself, and the boundary of the entry points that write and read it."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maskbits_ref as MB  # noqa: E402
from test_abi import kind, parse_header  # noqa: E402

NEW = ('lp_bn_add_act_bits', 'lp_bn_add_act_planes_bits', 'lp_bn_add_act16_bits', 'lp_conv16_fwd_gated', 'lp_bn_bwd16_dual')


def test_predicate_is_sign_clear_and_magnitude_nonzero():
    """every 16-bit word: (w - 1) < 0x7fff unsigned  <=>  sign bit clear and the other 15 bits not all zero.  Named cases: +0, -0, the smallest
    subnormal, 0x7fff (a NaN in bf16 and fp16: counts as positive, as the plane test of mask mode 3 does), 0x8001, quiet / signalling / negative NaNs"""
    w = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    want = ((w & 0x8000) == 0) & ((w & 0x7fff) != 0)
    assert np.array_equal(MB.positive(w), want)
    named = {0x0000: 0, 0x8000: 0, 0x0001: 1, 0x7fff: 1, 0x8001: 0, 0x7fc0: 1, 0x7f81: 1, 0x7e00: 1, 0x7c01: 1, 0xffc0: 0, 0xfe00: 0, 0x7f80: 1, 0x7c00: 1,
             0xff80: 0, 0x3f80: 1, 0xbf80: 0}
    for word, bit in named.items():
        assert int(MB.positive(np.array([word], dtype=np.uint16))[0]) == bit, hex(word)


def test_packing_order_bit_j_is_channel_8g_plus_j():
    w = np.zeros((3, 24), dtype=np.uint16)
    w[0, 0] = 0x3f80           # channel 0 -> byte 0 bit 0
    w[0, 7] = 0x0001           # channel 7 -> byte 0 bit 7
    w[1, 9] = 0x7fff           # channel 9 -> byte 1 bit 1
    w[2, 20] = 0x4000          # channel 20 -> byte 2 bit 4
    w[2, 21] = 0x8001          # negative: no bit
    w[2, 22] = 0x8000          # -0: no bit
    got = MB.pack(w)
    assert got.shape == (3, 3) and got.dtype == np.uint8
    want = np.zeros((3, 3), dtype=np.uint8)
    want[0, 0] = 0x81; want[1, 1] = 0x02; want[2, 2] = 0x10
    assert np.array_equal(got, want)
    # against the definition, on random words with the special ones mixed in
    rng = np.random.default_rng(5)
    r = rng.integers(0, 1 << 16, size=(37, 64), dtype=np.uint32).astype(np.uint16)
    special = rng.choice(np.array([0, 0x8000, 1, 0x7fff, 0x8001, 0x7fc0, 0xffc0], dtype=np.uint16), size=r.shape)
    r = np.where(rng.random(r.shape) < 0.3, special, r)
    byte = MB.pack(r)
    for p in (0, 17, 36):
        for g in range(8):
            for j in range(8):
                word = int(r[p, 8 * g + j])
                assert (int(byte[p, g]) >> j) & 1 == int(0 < word < 0x8000), (p, g, j, hex(word))


def test_new_entry_points_are_declared_exported_and_bound_alike():
    """the additive entry points: declared in include/lp_hip.h, listed in _lib.SIGNATURES with the same argument kinds, exported by the library --
    and the ABI version they were added under is still 12"""
    from latent_pose_reenactment_amd import _lib
    decls = parse_header()
    cmap = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_longlong: 'll', ctypes.c_char_p: 'ptr'}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in decls and name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert [cmap[a] for a in args] == [kind(p) for p in decls[name][1]], name
        assert cmap[res] == 'int'
    # each *_bits form = its base form + ONE pointer (the bit plane) in front of the sizes; the gated conv = lp_conv16_fwd_stats + one pointer behind res
    for base in ('lp_bn_add_act', 'lp_bn_add_act_planes', 'lp_bn_add_act16'):
        b, n = [kind(p) for p in decls[base][1]], [kind(p) for p in decls[base + '_bits'][1]]
        i = b.index('ll')
        assert n == b[:i] + ['ptr'] + b[i:], base
        assert 'bits' in decls[base + '_bits'][1][i]
    b, n = [kind(p) for p in decls['lp_conv16_fwd_stats'][1]], [kind(p) for p in decls['lp_conv16_fwd_gated'][1]]
    assert n == b[:7] + ['ptr'] + b[7:] and 'res_bits' in decls['lp_conv16_fwd_gated'][1][7]
    assert _lib.lib().lp_abi_version() == 12


def test_argument_validation_needs_no_gpu():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(16)          # a non-null pointer that is never dereferenced: validation comes first
    # bits without the HI plane they describe
    assert l.lp_bn_add_act_bits(one, one, one, None, None, None, one, None, None, one, 4, 8, 1, 0, None) != 0 and b'HI plane' in l.lp_last_error()
    # a gated residual needs the residual, no res_shift, Cout % 8 == 0
    common = (2, 4, 4, 32, 12, 32, 128, 1, 0, 0, 0, None, None, None, 0, None, 0, None, None, 0, None, None)
    assert l.lp_conv16_fwd_gated(one, None, one, None, one, None, one, one, None, None, *common) != 0 and b'res_bits' in l.lp_last_error()
    # mode 4 needs its source; the dual form takes modes 1 .. 4 only and both x of one kind
    assert l.lp_bn_bwd16_h(one, one, None, None, one, one, one, one, one, one, None, one, one, one, one, 4, 8, 4, 0.0, 0, 0, None, None) != 0
    args = [one, one, one, None, one, one, one, one, None, one, one, one, one, one, None, one, one, one, one, None, one, one, one, one]
    assert l.lp_bn_bwd16_dual(*args, 4, 8, 0, 0, 0, None) != 0 and b'mask mode' in l.lp_last_error()
    args[3] = one          # xa as a 16-bit plane, xb as fp32
    assert l.lp_bn_bwd16_dual(*args, 4, 8, 4, 0, 2, None) != 0 and b'both' in l.lp_last_error()
