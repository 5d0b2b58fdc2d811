"""The definition in the header comment of csrc/png.hip, restated one byte and one bit at a time in plain Python integers: slow, obvious, and
independent of ``hipops.png_encode_host`` (no numpy arithmetic, no zlib: the checksums are computed bit by bit too).  ``frames``: a nested sequence
or array [T][H][W][C] of integers 0 .. 255; every function returns Python ``bytes`` / lists."""
SEG = 16384
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ---- checksums -------------------------------------------------------------------------------------------------------------------------------------
def crc32(data):
    crc = 0xFFFFFFFF
    for byte in data:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0xEDB88320 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def adler32(data):
    a, b = 1, 0
    for byte in data:
        a = (a + byte) % 65521
        b = (b + a) % 65521
    return b << 16 | a


def be32(v):
    return bytes((v >> 24 & 255, v >> 16 & 255, v >> 8 & 255, v & 255))


def chunk(kind, data):
    return be32(len(data)) + kind + data + be32(crc32(kind + data))


# ---- filter ----------------------------------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def filter_frame(frame):
    """one frame [H][W][C] -> its filtered stream as a list of H (1 + W C) integers"""
    out = []
    prev = None
    for row in frame:
        cur = [int(v) for px in row for v in px]
        bpp = len(row[0])
        cands = [[], [], [], [], []]
        for j, x in enumerate(cur):
            a = cur[j - bpp] if j >= bpp else 0
            b = prev[j] if prev is not None else 0
            c = prev[j - bpp] if prev is not None and j >= bpp else 0
            for kind, pred in enumerate((0, a, b, (a + b) // 2, paeth(a, b, c))):
                cands[kind].append((x - pred) % 256)
        scores = [sum(v if v < 128 else 256 - v for v in cand) for cand in cands]
        kind = scores.index(min(scores))          # the first minimum: ties to the lowest type
        out += [kind] + cands[kind]
        prev = cur
    return out


# ---- tokens ----------------------------------------------------------------------------------------------------------------------------------------
def tokens(f):
    """the tokens of one segment: ('lit', byte) and ('match', length), in stream order, without the end-of-block symbol"""
    out = []
    i, n = 0, len(f)
    while i < n:
        if i == 0 or f[i] != f[i - 1]:
            out.append(('lit', f[i]))
            i += 1
            continue
        r = 0
        while i + r < n and f[i + r] == f[i + r - 1]:
            r += 1
        for _ in range(r // 258):
            out.append(('match', 258))
        q = r % 258
        if q >= 3:
            out.append(('match', q))
        else:
            out += [('lit', f[i])] * q
        i += r
    return out


def length_symbol(length):
    k = max(i for i in range(29) if LENGTH_BASE[i] <= length)
    return 257 + k, LENGTH_EXTRA[k], length - LENGTH_BASE[k]


# ---- the code --------------------------------------------------------------------------------------------------------------------------------------
def code_lengths(hist):
    """steps 1 .. 4 of the definition.  A node is (weight, 0 internal / 1 leaf, order, children); the two smallest by that key are merged"""
    nodes = [(n, 1, rank, s) for rank, (n, s) in enumerate(sorted((n, s) for s, n in enumerate(hist) if n > 0))]
    assert len(nodes) >= 2
    created = 0
    while len(nodes) > 1:
        first = min(nodes, key=lambda node: node[:3])
        nodes.remove(first)
        second = min(nodes, key=lambda node: node[:3])
        nodes.remove(second)
        nodes.append((first[0] + second[0], 0, created, (first, second)))
        created += 1
    depth_of = {}

    def descend(node, depth):
        if node[1] == 1:
            depth_of[node[3]] = depth
        else:
            for child in node[3]:
                descend(child, depth + 1)
    descend(nodes[0], 0)
    cnt = [0] * (max(depth_of.values()) + 2)
    for d in depth_of.values():
        cnt[d] += 1
    for deep in range(len(cnt) - 1, 15, -1):
        while cnt[deep] > 0:
            b = 14
            while cnt[b] == 0:
                b -= 1
            cnt[b] -= 1
            cnt[b + 1] += 2
            cnt[deep] -= 2
            cnt[deep - 1] += 1
    by_rank = [s for _, s in sorted((n, s) for s, n in enumerate(hist) if n > 0)]          # rarest first
    lengths = [0] * len(hist)
    i = 0
    for length in range(15, 0, -1):
        for _ in range(cnt[length] if length < len(cnt) else 0):
            lengths[by_rank[i]] = length
            i += 1
    assert i == len(by_rank)
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2"""
    bl_count = [0] * 16
    for length in lengths:
        if length:
            bl_count[length] += 1
    code, next_code = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, length in enumerate(lengths):
        if length:
            codes[s] = next_code[length]
            next_code[length] += 1
    return codes


class Bits:
    """the LSB-first bit stream of deflate"""

    def __init__(self):
        self.bits = []

    def field(self, value, n):          # least significant bit first
        for k in range(n):
            self.bits.append(value >> k & 1)

    def huffman(self, code, n):         # most significant bit first
        for k in range(n - 1, -1, -1):
            self.bits.append(code >> k & 1)

    def to_byte_boundary(self):
        while len(self.bits) % 8:
            self.bits.append(0)

    def bytes(self):
        assert len(self.bits) % 8 == 0
        return bytes(sum(bit << k for k, bit in enumerate(self.bits[i:i + 8])) for i in range(0, len(self.bits), 8))


def segment_info(f, final):
    """one segment -> {'bytes', 'stored', 'lengths', 'dyn_bytes'}"""
    f = [int(v) for v in f]
    n = len(f)
    toks = tokens(f)
    hist = [0] * 286
    for kind, v in toks:
        hist[v if kind == 'lit' else length_symbol(v)[0]] += 1
    hist[256] += 1
    lengths = code_lengths(hist)
    codes = canonical_codes(lengths)
    w = Bits()
    w.field(0, 1)            # BFINAL
    w.field(2, 2)            # BTYPE: dynamic
    w.field(29, 5)           # HLIT: 286 codes
    w.field(0, 5)            # HDIST: 1 code
    w.field(15, 4)           # HCLEN: 19 code-length codes
    for s in CLEN_ORDER:
        w.field(4 if s < 16 else 0, 3)
    for length in lengths + [1]:          # the 286 lengths and the one distance code, each as the 4-bit code of its value
        w.huffman(length, 4)
    for kind, v in toks:
        if kind == 'lit':
            w.huffman(codes[v], lengths[v])
        else:
            s, extra_bits, extra = length_symbol(v)
            w.huffman(codes[s], lengths[s])
            w.field(extra, extra_bits)
            w.huffman(0, 1)               # distance 1
    w.huffman(codes[256], lengths[256])
    w.field(1 if final else 0, 1)         # the empty stored block
    w.field(0, 2)
    w.to_byte_boundary()
    dynamic = w.bytes() + b'\x00\x00\xff\xff'
    stored = bytes((1 if final else 0, n & 255, n >> 8, (n ^ 0xFFFF) & 255, (n ^ 0xFFFF) >> 8)) + bytes(f)
    use_stored = len(dynamic) >= len(stored)
    return {'bytes': stored if use_stored else dynamic, 'stored': use_stored, 'lengths': lengths, 'dyn_bytes': len(dynamic), 'hist': hist}


def zlib_stream(f):
    f = [int(v) for v in f]
    out = b'\x78\x01'
    for first in range(0, len(f), SEG):
        out += segment_info(f[first:first + SEG], first + SEG >= len(f))['bytes']
    return out + be32(adler32(f))


def head(h, w, c):
    ihdr = be32(w) + be32(h) + bytes((8, 2 if c == 3 else 0, 0, 0, 0))
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr), chunk(b'IEND', b'')


def deflate_files(streams, h=None, w=None, c=1):
    """streams: [T][L] -> (bytes, offsets); without a shape: one grey row of L - 1 pixels, as hipops.png_deflate"""
    out, offsets = b'', [0]
    for f in streams:
        front, back = head(1, max(len(f) - 1, 1), 1) if h is None else head(h, w, c)
        out += front + chunk(b'IDAT', zlib_stream(f)) + back
        offsets.append(len(out))
    return out, offsets


def encode(frames):
    """frames [T][H][W][C] -> (bytes, offsets)"""
    h, w, c = len(frames[0]), len(frames[0][0]), len(frames[0][0][0])
    return deflate_files([filter_frame(frame) for frame in frames], h, w, c)
