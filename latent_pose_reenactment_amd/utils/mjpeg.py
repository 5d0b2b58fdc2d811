"""Host side of the Motion-JPEG output of drive.py (``--format avi``): the constants of baseline JPEG (ITU-T T.81 Annex K), the frame header that
every encoded frame starts with, and a RIFF AVI writer.  The pixels are encoded by ``hipops.jpeg_encode`` (csrc/jpeg.hip holds the definition);
nothing here touches a GPU, and numpy is the only dependency."""
import struct
from fractions import Fraction

import numpy as np

# Annex K.1 (luminance) and K.2 (chrominance), row-major with the vertical frequency as the row
K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# Annex K.3: BITS (the number of codes of length 1 .. 16) and HUFFVAL (the symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
    'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849'
    '4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5'
    'c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')))
# in the order of the DHT segments; (table class, table id)
HUFFMAN = ((0, 0, DC_LUMA), (1, 0, AC_LUMA), (0, 1, DC_CHROMA), (1, 1, AC_CHROMA))


def _zigzag():
    """zigzag position -> natural index (T.81 Figure A.6): the anti-diagonals in turn, odd ones downwards"""
    order = []
    for s in range(15):
        diag = [(u, s - u) for u in range(8) if 0 <= s - u < 8]
        order += [u * 8 + v for u, v in (diag if s % 2 else reversed(diag))]
    return tuple(order)


ZIGZAG = _zigzag()


def check_quality(quality, who='jpeg'):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f'{who}: quality must be an integer in 1 .. 100, got {quality!r}')
    return int(quality)


def quant_tables(quality):
    """uint8 [2, 64] in natural order: the Annex K tables under the IJG scaling rule, in integer arithmetic"""
    q = check_quality(quality, 'quant_tables')
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((k * s + 50) // 100, 1), 255) for k in base] for base in (K1, K2)], dtype=np.uint8)


def huffman_codes(spec):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) pair (T.81 Annex C)"""
    bits, vals = spec
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def code_table():
    """uint32 [2 * 12 + 2 * 256], (code << 5) | length by symbol, 0 where the table has none: DC luminance, DC chrominance, AC luminance, AC
    chrominance -- the layout of lp_jpeg_code_table"""
    t = np.zeros(2 * 12 + 2 * 256, dtype=np.uint32)
    for base, spec in ((0, DC_LUMA), (12, DC_CHROMA), (24, AC_LUMA), (24 + 256, AC_CHROMA)):
        for sym, (code, length) in huffman_codes(spec).items():
            t[base + sym] = (code << 5) | length
    return t


def _segment(marker, payload):
    return bytes((0xFF, marker)) + struct.pack('>H', len(payload) + 2) + payload


def jpeg_header(H, W, quality):
    """everything of a frame's file in front of its scan: SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS (csrc/jpeg.hip: per-frame layout)"""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f'jpeg_header: H and W must be in 1 .. 65535, got {H} x {W}')
    qt = quant_tables(quality)
    out = b'\xff\xd8' + _segment(0xE0, b'JFIF\0' + bytes((1, 1, 0)) + struct.pack('>HH', 1, 1) + bytes((0, 0)))
    for i in range(2):
        out += _segment(0xDB, bytes((i,)) + bytes(int(qt[i][n]) for n in ZIGZAG))
    out += _segment(0xC0, bytes((8,)) + struct.pack('>HH', H, W) + bytes((3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for cls, ident, (bits, vals) in HUFFMAN:
        out += _segment(0xC4, bytes((cls << 4 | ident,)) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack('>H', (W + 7) // 8))
    out += _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))
    return out


AVI_LIMIT = 2 ** 31 - 1          # a RIFF AVI without the OpenDML extension


class AviWriter:
    """Motion-JPEG AVI: RIFF 'AVI ' = LIST hdrl (avih, LIST strl (strh vids / MJPG, strf BITMAPINFOHEADER)) + LIST movi ('00dc' chunks, one JPEG
    file each, padded to even length) + idx1.  The frame count and the sizes are patched on ``close``; a file that would pass 2 GiB raises."""

    def __init__(self, path, H, W, fps=25):
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError(f'AviWriter: H and W must be >= 1, got {H} x {W}')
        if not fps > 0:
            raise ValueError(f'AviWriter: fps must be > 0, got {fps}')
        frac = Fraction(fps).limit_denominator(10000)
        self.rate, self.scale = frac.numerator, frac.denominator
        self.H, self.W, self.path = H, W, path
        self.index, self.largest = [], 0
        self.f = open(path, 'wb')
        self.f.write(self._headers())
        self.movi = self.f.tell() - 4          # idx1 offsets count from the 'movi' fourcc

    def _headers(self, riff=0, movi=0):
        n = len(self.index)
        strh = struct.pack('<4s4sIHHIIIIIIII4h', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0, n, self.largest, 0xFFFFFFFF, 0,
                           0, 0, min(self.W, 32767), min(self.H, 32767))
        strf = struct.pack('<IiiHH4sIiiII', 40, self.W, self.H, 1, 24, b'MJPG', self.W * self.H * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        usec = round(1e6 * self.scale / self.rate)
        avih = struct.pack('<14I', usec, self.largest * self.rate // self.scale, 0, 0x10, n, 0, 1, self.largest, self.W, self.H, 0, 0, 0, 0)
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        return (b'RIFF' + struct.pack('<I', riff) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl
                + b'LIST' + struct.pack('<I', movi) + b'movi')

    def add(self, data, offsets):
        """``data``: the uint8 buffer of ``hipops.jpeg_encode`` (a tensor on any device, or an array), ``offsets``: its int64 [T + 1] table"""
        if hasattr(data, 'detach'):
            data = data.detach().cpu().numpy()
        if hasattr(offsets, 'detach'):
            offsets = offsets.detach().cpu().numpy()
        data = memoryview(np.ascontiguousarray(data, dtype=np.uint8))
        offsets = [int(o) for o in offsets]
        if not offsets or offsets[0] < 0 or offsets[-1] > len(data) or any(b <= a for a, b in zip(offsets, offsets[1:])):
            raise ValueError(f'AviWriter.add: the offsets {offsets[:4]} ... do not describe frames inside {len(data)} bytes')
        for a, b in zip(offsets, offsets[1:]):
            size = b - a
            end = self.f.tell() + 8 + size + (size & 1)
            if end + 8 + 16 * (len(self.index) + 1) > AVI_LIMIT:
                raise ValueError(f'AviWriter: {self.path} would pass 2 GiB with frame {len(self.index)} (OpenDML is not written): '
                                 'split the sequence')
            self.index.append((self.f.tell() - self.movi, size))
            self.largest = max(self.largest, size)
            self.f.write(b'00dc' + struct.pack('<I', size))
            self.f.write(data[a:b])
            if size & 1:
                self.f.write(b'\0')

    def close(self):
        if self.f is None:
            return
        end = self.f.tell()
        self.f.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
        for at, size in self.index:
            self.f.write(b'00dc' + struct.pack('<III', 0x10, at, size))
        total = self.f.tell()
        self.f.seek(0)
        self.f.write(self._headers(riff=total - 8, movi=end - self.movi))
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
