"""The definition of csrc/jpeg_decode.hip restated in numpy integers, written from the header comment: one parsed file (``utils.jpeg_parse.parse``)
-> (coefficients int16 [blocks, 64] in zigzag and scan order, the sample planes over their block areas, the pixels uint8 [H, W, 3], the status).
It shares no code with the package's host twin (``hipops.jpeg_decode_host``), which is one of the things it is held against: the Huffman codes are
looked up as whole 16-bit windows in a table built from the DHT counts, the IDCT is written out term by term, the upsampling writes its edge
columns and rows explicitly.  ``idct_exact`` is the fp64 IDCT before rounding, the yardstick of the integer one."""
import functools
import math

import numpy as np

# T.81 Figure A.6, written out
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

K = [[int(np.rint(8192.0 * (math.sqrt(1.0 / 8.0) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16.0))) for x in range(8)] for u in range(8)]


@functools.lru_cache(maxsize=64)
def _window_table(bits, vals):
    """for every 16-bit window: (symbol << 8) | code length, -1 where no code of <= 16 bits is a prefix of it"""
    table = np.full(1 << 16, -1, dtype=np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            table[lo:lo + (1 << (16 - length))] = (vals[k] << 8) | length
            code += 1
            k += 1
        code <<= 1
    return table.tolist()


def _table(spec):
    bits, vals = spec
    return _window_table(tuple(int(b) for b in bits), tuple(int(v) for v in vals))


def entropy(d):
    """-> (int16 [blocks, 64], status)"""
    nluma = d.hmax * d.vmax if d.components == 3 else 1
    bpm = d.blocks_per_mcu
    total = d.mcux * d.mcuy
    coefs = np.zeros((total * bpm, 64), dtype=np.int64)
    dc = [_table(d.huffman[(0, t)]) for t in d.td]
    ac = [_table(d.huffman[(1, t)]) for t in d.ta]
    status = 0
    for s in range(len(d.seg) - 1):
        data = bytes(d.scan[d.seg[s]:d.seg[s + 1]])
        nbits = 8 * len(data)
        bits = int.from_bytes(data + bytes(8), 'big')
        width = nbits + 64
        pos = 0
        first = s * d.restart
        count = min(d.restart, total - first) if d.restart else total
        pred = [0] * d.components
        st = 0
        for m in range(first, first + count):
            for j in range(bpm):
                c = 0 if j < nluma else j - nluma + 1
                blk = coefs[m * bpm + j]
                e = dc[c][(bits >> (width - pos - 16)) & 0xFFFF]
                if e < 0 or (e >> 8) > 15:
                    st = 1
                    break
                pos += e & 255
                size = e >> 8
                diff = 0
                if size:
                    v = (bits >> (width - pos - size)) & ((1 << size) - 1)
                    pos += size
                    diff = v if v >= 1 << (size - 1) else v - (1 << size) + 1
                if pos > nbits:
                    st = 3
                    break
                pred[c] = ((pred[c] + diff + 32768) & 0xFFFF) - 32768          # kept in 16 bits
                blk[0] = pred[c]
                k = 1
                for _ in range(63):
                    if k >= 64:
                        break
                    e = ac[c][(bits >> (width - pos - 16)) & 0xFFFF]
                    if e < 0:
                        st = 1
                        break
                    pos += e & 255
                    run, size = (e >> 8) >> 4, (e >> 8) & 15
                    if size == 0:
                        if pos > nbits:
                            st = 3
                            break
                        if run == 15:
                            k += 16
                            continue
                        break
                    k += run
                    if k > 63:
                        st = 2
                        break
                    v = (bits >> (width - pos - size)) & ((1 << size) - 1)
                    pos += size
                    if pos > nbits:
                        st = 3
                        break
                    blk[k] = v if v >= 1 << (size - 1) else v - (1 << size) + 1
                    k += 1
                if st:
                    break
            if st:
                break
        status = max(status, st)
    return coefs.astype(np.int16), status


def dequantise(d, coefs):
    """-> int64 [blocks, 8, 8] (u, v) in natural order"""
    nluma = d.hmax * d.vmax if d.components == 3 else 1
    bpm = d.blocks_per_mcu
    F = np.zeros((len(coefs), 64), dtype=np.int64)
    for z in range(64):
        F[:, ZIGZAG[z]] = coefs[:, z]
    for j in range(bpm):
        q = d.qt[d.tq[0 if j < nluma else j - nluma + 1]].astype(np.int64)
        F[j::bpm] = np.minimum(np.maximum(F[j::bpm] * q, -32768), 32767)
    return F.reshape(-1, 8, 8)


def idct_integer(F):
    """-> S [blocks, x, y] before the level shift and the clamp"""
    n = len(F)
    T = np.zeros((n, 8, 8), dtype=np.int64)
    for x in range(8):
        for v in range(8):
            acc = np.full(n, 1 << 9, dtype=np.int64)
            for u in range(8):
                acc += K[u][x] * F[:, u, v]
            T[:, x, v] = acc >> 10
    S = np.zeros((n, 8, 8), dtype=np.int64)
    for x in range(8):
        for y in range(8):
            acc = np.full(n, 1 << 15, dtype=np.int64)
            for v in range(8):
                acc += K[v][y] * T[:, x, v]
            S[:, x, y] = acc >> 16
    return S


def idct_exact(F):
    """the orthonormal inverse DCT of F in fp64 -> [blocks, x, y], not rounded (K / 2^13 is the orthonormal basis and the two shifts take 2^26 off:
    this is what the integer S approximates)"""
    C = np.array([[(math.sqrt(1.0 / 8.0) if u == 0 else 0.5) * math.cos((2 * x + 1) * u * math.pi / 16.0) for x in range(8)] for u in range(8)])
    return np.einsum('ux,buv,vy->bxy', C, F.astype(np.float64), C)


def planes_of(d, S):
    """clamp(S + 128) -> the uint8 planes of the components over their block areas: [luma, (cb, cr)]"""
    smp = np.minimum(np.maximum(S + 128, 0), 255).astype(np.uint8)
    nluma = d.hmax * d.vmax if d.components == 3 else 1
    bpm = d.blocks_per_mcu
    out = [np.zeros(shape, dtype=np.uint8) for shape in d.plane_shapes]
    for m in range(d.mcux * d.mcuy):
        my, mx = divmod(m, d.mcux)
        for j in range(bpm):
            if j < nluma:
                c, fy, fx = 0, (d.vmax if d.components == 3 else 1), (d.hmax if d.components == 3 else 1)
                by, bx = my * fy + j // fx, mx * fx + j % fx
            else:
                c, by, bx = j - nluma + 1, my, mx
            out[c][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = smp[m * bpm + j]
    return out


def upsample(d, plane):
    """a chroma plane -> int64 [H, W]"""
    rows, n = -(-d.h // d.vmax), -(-d.w // d.hmax)
    x = plane[:rows, :n].astype(np.int64)
    if d.hmax == 1:
        return x
    if d.vmax == 1:
        out = np.zeros((rows, 2 * n), dtype=np.int64)
        out[:, 2::2] = (3 * x[:, 1:] + x[:, :-1] + 1) >> 2
        out[:, 1:-1:2] = (3 * x[:, :-1] + x[:, 1:] + 2) >> 2
        out[:, 0], out[:, 2 * n - 1] = x[:, 0], x[:, n - 1]
        return out[:, :d.w]
    out = np.zeros((2 * rows, 2 * n), dtype=np.int64)
    for i in range(rows):
        for half, nb in ((0, max(i - 1, 0)), (1, min(i + 1, rows - 1))):
            cs = 3 * x[i] + x[nb]
            row = out[2 * i + half]
            row[2::2] = (3 * cs[1:] + cs[:-1] + 8) >> 4
            row[1:-1:2] = (3 * cs[:-1] + cs[1:] + 7) >> 4
            row[0], row[2 * n - 1] = (4 * cs[0] + 8) >> 4, (4 * cs[n - 1] + 7) >> 4
    return out[:d.h, :d.w]


def colour(d, planes):
    y = planes[0][:d.h, :d.w].astype(np.int64)
    if d.components == 1:
        return np.stack([y, y, y], axis=2).astype(np.uint8)
    cb, cr = upsample(d, planes[1]) - 128, upsample(d, planes[2]) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.minimum(np.maximum(np.stack([r, g, b], axis=2), 0), 255).astype(np.uint8)


def decode(d):
    """-> dict: coefs, status, F, S, planes (list per component), pixels"""
    coefs, status = entropy(d)
    F = dequantise(d, coefs)
    S = idct_integer(F)
    planes = planes_of(d, S)
    return {'coefs': coefs, 'status': status, 'F': F, 'S': S, 'planes': planes, 'pixels': colour(d, planes)}
