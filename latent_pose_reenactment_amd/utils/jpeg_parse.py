"""Host side of the JPEG decode on the GPU (``--decode_jpeg_on_gpu``; csrc/jpeg_decode.hip holds the definition): ``parse`` reads the markers of a
file and returns a ``Descriptor`` -- the frame header, the tables and the scan as plain bit strings, one per restart interval, byte stuffing removed
-- or ``None`` for a well-formed file outside the supported set (the caller decodes that one with PIL); ``pack`` lays the descriptors of a batch out
as the tables lp_jpeg_decode_entropy / lp_jpeg_decode_pixels read.  Runs in the loader's worker processes: numpy is the only dependency, nothing
here touches a GPU.

Supported: baseline sequential DCT (SOF0), 8-bit samples, 1 or 3 components in one interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantisation
tables, Huffman table ids 0 .. 3, any DRI, grey / 4:4:4 / 4:2:2 (luma 2 x 1) / 4:2:0 (luma 2 x 2) with 1 x 1 chroma, no Adobe APP14 segment with a
transform other than 1 on a three-component file, and not the component ids 'R', 'G', 'B' without a JFIF or Adobe marker (libjpeg reads those as
RGB, not YCbCr).  Fill bytes (0xFF 0xFF) in front of a marker are legal."""
from typing import NamedTuple

import numpy as np

from .mjpeg import ZIGZAG

FRAME_COLUMNS = ('h', 'w', 'components', 'hmax', 'vmax', 'mcux', 'mcuy', 'restart', 'coef_off', 'plane_off', 'dst_off', 'first_seg', 'segments',
                 'tq0', 'tq1', 'tq2', 'td0', 'td1', 'td2', 'ta0', 'ta1', 'ta2', 'reserved0', 'reserved1')
NFRAME = len(FRAME_COLUMNS)
NSEG = 4                        # a segment row: frame, first byte, end byte (of the packed scan bytes), reserved
HUFF_WORDS = 96                 # a Huffman table on the device: maxcode[16], delta[16] (int32), the symbols (256 bytes)
_COEF_OFF, _PLANE_OFF, _DST_OFF, _FIRST_SEG = (FRAME_COLUMNS.index(n) for n in ('coef_off', 'plane_off', 'dst_off', 'first_seg'))
_NATURAL = np.array(ZIGZAG, dtype=np.int64)          # zigzag position -> natural index


class Descriptor(NamedTuple):
    h: int
    w: int
    components: int
    hmax: int                   # the luma sampling factors; chroma is 1 x 1
    vmax: int
    tq: tuple                   # per component: quantisation table, DC table, AC table
    td: tuple
    ta: tuple
    qt: np.ndarray              # uint8 [4, 64], natural order; zeros where the file defines none
    huffman: dict               # (class, id) -> (BITS uint8 [16], HUFFVAL uint8 [n])
    restart: int                # MCUs per restart interval, 0: none
    scan: np.ndarray            # uint8: the entropy-coded bytes of all segments, stuffing and markers removed
    seg: np.ndarray             # int64 [segments + 1]: segment s = scan[seg[s]:seg[s + 1]]

    @property
    def mcux(self):
        return -(-self.w // (8 * self.hmax))

    @property
    def mcuy(self):
        return -(-self.h // (8 * self.vmax))

    @property
    def blocks_per_mcu(self):
        return self.hmax * self.vmax + 2 if self.components == 3 else 1

    @property
    def blocks(self):
        return self.mcux * self.mcuy * self.blocks_per_mcu

    @property
    def plane_shapes(self):
        """the padded block area of every component: [(rows, columns)]"""
        luma = (self.mcuy * self.vmax * 8, self.mcux * self.hmax * 8)
        return [luma] + [(self.mcuy * 8, self.mcux * 8)] * (self.components - 1)

    @property
    def plane_bytes(self):
        return sum(r * c for r, c in self.plane_shapes)


def idct_table():
    """K[u][x] = rint(2^13 c(u) cos((2 x + 1) u pi / 16)), c(0) = sqrt(1 / 8), c(u > 0) = 1 / 2, formed in fp64: int32 [64], u the row"""
    u, x = np.arange(8, dtype=np.float64)[:, None], np.arange(8, dtype=np.float64)[None, :]
    c = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * c * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)).astype(np.int32).reshape(64)


def _u16(data, at):
    return (int(data[at]) << 8) | int(data[at + 1])


def _huffman(payload, tables):
    at = 0
    while at < len(payload):
        if at + 17 > len(payload):
            raise ValueError('jpeg_parse: a DHT table runs past its segment')
        cls, ident = int(payload[at]) >> 4, int(payload[at]) & 15
        if cls > 1 or ident > 3:
            raise ValueError(f'jpeg_parse: DHT class {cls} / id {ident} outside 0 .. 1 / 0 .. 3')
        bits = np.array(payload[at + 1:at + 17], dtype=np.uint8)
        n = int(bits.sum())
        if n > 256 or at + 17 + n > len(payload):
            raise ValueError('jpeg_parse: a DHT table runs past its segment')
        code = 0
        for length in range(1, 17):
            code = (code + int(bits[length - 1])) << 1
            if code > 1 << (length + 1):
                raise ValueError(f'jpeg_parse: the DHT counts over-subscribe the codes of length {length}')
        tables[(cls, ident)] = (bits, np.array(payload[at + 17:at + 17 + n], dtype=np.uint8))
        at += 17 + n


def _scan(data, at, restart):
    """the entropy-coded data from ``at`` on -> (unstuffed bytes, segment offsets, the marker that ends it)"""
    a = data[at:]
    ff = np.flatnonzero(a[:-1] == 0xFF)
    nxt = a[ff + 1]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    term = ff[(nxt != 0x00) & (nxt != 0xFF) & ~rst]
    if not len(term):
        raise ValueError('jpeg_parse: truncated: the scan ends without a marker (no EOI)')
    end = int(term[0])
    marker = int(a[end + 1])
    inside = ff < end
    ff, nxt, rst = ff[inside], nxt[inside], rst[inside]
    keep = np.ones(end, dtype=bool)
    keep[ff[nxt == 0x00] + 1] = False           # the stuffed zero behind a data 0xFF
    keep[ff[nxt == 0xFF]] = False               # a fill byte in front of a marker
    at_rst = ff[rst]
    keep[at_rst] = False
    keep[at_rst + 1] = False
    order = nxt[rst].astype(np.int64) - 0xD0
    if len(order) and not restart:
        raise ValueError('jpeg_parse: a restart marker in a scan without DRI')
    if not np.array_equal(order, np.arange(len(order)) % 8):
        bad = int(np.flatnonzero(order != np.arange(len(order)) % 8)[0])
        raise ValueError(f'jpeg_parse: RST out of order: restart marker {bad} of the scan is RST{int(order[bad])}, expected RST{bad % 8}')
    kept = np.concatenate(([0], np.cumsum(keep)))
    seg = np.concatenate(([0], kept[at_rst], [kept[end]])).astype(np.int64)
    return np.ascontiguousarray(a[:end][keep]), seg, marker, at + end


def parse(file_bytes):
    """-> ``Descriptor``, or None for a well-formed file outside the supported set; ValueError naming the cause for a malformed one"""
    data = np.frombuffer(bytes(file_bytes), dtype=np.uint8)
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise ValueError('jpeg_parse: not a JPEG file (no SOI)')
    at = 2
    qt = np.zeros((4, 64), dtype=np.uint8)
    have_q, tables, frame, restart, adobe, jfif = set(), {}, None, 0, None, False
    while True:
        if at >= len(data):
            raise ValueError('jpeg_parse: truncated: the file ends in front of the scan')
        if data[at] != 0xFF:
            raise ValueError(f'jpeg_parse: byte {at} is 0x{int(data[at]):02X} where a marker was expected')
        while at < len(data) and data[at] == 0xFF:           # fill bytes
            at += 1
        if at >= len(data):
            raise ValueError('jpeg_parse: truncated: the file ends inside a marker')
        marker = int(data[at])
        at += 1
        if marker == 0xD9:
            raise ValueError('jpeg_parse: EOI in front of any scan')
        if marker == 0x01 or 0xD0 <= marker <= 0xD8:
            raise ValueError(f'jpeg_parse: marker 0xFF{marker:02X} outside a scan')
        if at + 2 > len(data):
            raise ValueError(f'jpeg_parse: truncated: the file ends inside the length of segment 0xFF{marker:02X}')
        length = _u16(data, at)
        if length < 2 or at + length > len(data):
            raise ValueError(f'jpeg_parse: truncated: segment 0xFF{marker:02X} declares a length of {length} bytes, {len(data) - at} remain')
        payload = data[at + 2:at + length]
        at += length
        if marker in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC, 0xDC):
            return None                                      # extended, progressive, lossless, arithmetic coding, DNL
        if marker == 0xC0:
            if frame is not None:
                raise ValueError('jpeg_parse: a second SOF0')
            if len(payload) < 6 or len(payload) != 6 + 3 * int(payload[5]):
                raise ValueError('jpeg_parse: the SOF0 segment has not the length its component count gives')
            frame = (int(payload[0]), _u16(payload, 1), _u16(payload, 3),
                     [(int(payload[6 + 3 * c]), int(payload[7 + 3 * c]) >> 4, int(payload[7 + 3 * c]) & 15, int(payload[8 + 3 * c]))
                      for c in range(int(payload[5]))])
        elif marker == 0xDB:
            p = 0
            while p < len(payload):
                if int(payload[p]) >> 4:
                    return None                              # 16-bit quantisation table
                ident = int(payload[p]) & 15
                if ident > 3 or p + 65 > len(payload):
                    raise ValueError('jpeg_parse: a DQT table has an id above 3 or runs past its segment')
                qt[ident, _NATURAL] = payload[p + 1:p + 65]
                have_q.add(ident)
                p += 65
        elif marker == 0xC4:
            _huffman(payload, tables)
        elif marker == 0xDD:
            if len(payload) != 2:
                raise ValueError('jpeg_parse: a DRI segment of the wrong length')
            restart = _u16(payload, 0)
        elif marker == 0xEE and len(payload) >= 12 and bytes(payload[:5]) == b'Adobe':
            adobe = int(payload[11])
        elif marker == 0xE0 and len(payload) >= 5 and bytes(payload[:5]) == b'JFIF\0':
            jfif = True
        elif marker == 0xDA:
            break
    if frame is None:
        raise ValueError('jpeg_parse: SOS without a frame header (no SOF0)')
    precision, h, w, comps = frame
    if precision != 8 or h == 0 or len(comps) not in (1, 3):
        return None
    if w == 0:
        raise ValueError('jpeg_parse: a frame of width 0')
    if len(payload) < 1 or len(payload) != 4 + 2 * int(payload[0]):
        raise ValueError('jpeg_parse: the SOS segment has not the length its component count gives')
    ns = int(payload[0])
    if ns != len(comps) or any(int(payload[1 + 2 * c]) != comps[c][0] for c in range(ns)):
        return None                                          # not ONE interleaved scan of all components in frame order
    if (int(payload[1 + 2 * ns]), int(payload[2 + 2 * ns]), int(payload[3 + 2 * ns])) != (0, 63, 0):
        return None
    if len(comps) == 3:
        if adobe is not None and adobe != 1:
            return None
        if adobe is None and not jfif and tuple(c[0] for c in comps) == (0x52, 0x47, 0x42):
            return None                                      # component ids 'R', 'G', 'B' without a JFIF or Adobe marker: libjpeg reads them as RGB
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
        hmax, vmax = comps[0][1], comps[0][2]
    else:
        hmax = vmax = 1                                      # a one-component scan is not interleaved: its MCU is one block, whatever the factors
    tq = tuple(c[3] for c in comps)
    td = tuple(int(payload[2 + 2 * c]) >> 4 for c in range(ns))
    ta = tuple(int(payload[2 + 2 * c]) & 15 for c in range(ns))
    for c in range(ns):
        if tq[c] > 3 or tq[c] not in have_q:
            raise ValueError(f'jpeg_parse: missing table: component {c} uses quantisation table {tq[c]}, which the file does not define')
        if td[c] > 3 or (0, td[c]) not in tables:
            raise ValueError(f'jpeg_parse: missing table: component {c} uses DC Huffman table {td[c]}, which the file does not define')
        if ta[c] > 3 or (1, ta[c]) not in tables:
            raise ValueError(f'jpeg_parse: missing table: component {c} uses AC Huffman table {ta[c]}, which the file does not define')
    if np.any(qt[list(set(tq))] == 0):
        raise ValueError('jpeg_parse: a quantisation table holds a 0')
    mcus = -(-w // (8 * hmax)) * -(-h // (8 * vmax))
    scan, seg, marker, _ = _scan(data, at, restart)
    if marker == 0xDA:
        return None                                          # a second scan
    if marker != 0xD9:
        raise ValueError(f'jpeg_parse: marker 0xFF{marker:02X} inside the scan (only RSTn and EOI may follow entropy-coded data)')
    want = -(-mcus // restart) if restart else 1
    if len(seg) - 1 != want:
        raise ValueError(f'jpeg_parse: the scan holds {len(seg) - 1} restart intervals, the header gives {want}')
    return Descriptor(h, w, len(comps), hmax, vmax, tq, td, ta, qt, tables, restart, scan, seg)


def huffman_words(bits, vals):
    """int32 [96] of one table: maxcode[l] = the largest code of length l + 1 (-1: none), delta[l] = the index of that length's first symbol minus its
    first code (T.81 Annex F.2.2.3: symbol = vals[code + delta[l]] for the first l with code <= maxcode[l]), then the symbols, 256 bytes"""
    out = np.zeros(HUFF_WORDS, dtype=np.int32)
    out[:16] = -1
    code = k = 0
    for length in range(16):
        n = int(bits[length])
        if n:
            out[16 + length] = k - code
            code += n
            k += n
            out[length] = code - 1
        code <<= 1
    sym = np.zeros(256, dtype=np.uint8)
    sym[:len(vals)] = vals
    out[32:] = sym.view('<i4')
    return out


def pack(descriptors, dst_offsets=None):
    """the tables of one call for a list of descriptors -> dict of numpy arrays: ``scan`` uint8 (the segments of all frames back to back), ``seg``
    int64 [S, 4], ``frames`` int64 [N, 24] (``FRAME_COLUMNS``; coefficient and plane offsets assigned back to back, ``dst_off`` from ``dst_offsets``
    or dense back to back), ``qt`` uint8 [N, 4, 64], ``huffman`` int32 [N, 8, 96] (DC ids 0 .. 3, then AC), and the totals ``coef_blocks``,
    ``plane_bytes``, ``out_bytes`` (of the dense layout; 0 when offsets were given)"""
    n = len(descriptors)
    if n < 1:
        raise ValueError('jpeg_parse.pack: no descriptors')
    frames = np.zeros((n, NFRAME), dtype=np.int64)
    qt = np.zeros((n, 4, 64), dtype=np.uint8)
    huffman = np.zeros((n, 8, HUFF_WORDS), dtype=np.int32)
    huffman[:, :, :16] = -1
    segs, scans = [], []
    coef = plane = dst = byte = seg = 0
    for f, d in enumerate(descriptors):
        pad = (0,) * (3 - d.components)
        frames[f] = ([d.h, d.w, d.components, d.hmax, d.vmax, d.mcux, d.mcuy, d.restart, coef, plane,
                      dst if dst_offsets is None else int(dst_offsets[f]), seg, len(d.seg) - 1] + list(d.tq + pad) + list(d.td + pad) + list(d.ta + pad)
                     + [0, 0])
        qt[f] = d.qt
        for (cls, ident), (bits, vals) in d.huffman.items():
            huffman[f, 4 * cls + ident] = huffman_words(bits, vals)
        s = np.zeros((len(d.seg) - 1, NSEG), dtype=np.int64)
        s[:, 0], s[:, 1], s[:, 2] = f, byte + d.seg[:-1], byte + d.seg[1:]
        segs.append(s)
        scans.append(d.scan)
        coef += d.blocks
        plane += d.plane_bytes
        dst += d.h * d.w * 3
        byte += len(d.scan)
        seg += len(d.seg) - 1
    scan = np.concatenate(scans) if byte else np.zeros(0, dtype=np.uint8)
    return {'scan': scan, 'seg': np.concatenate(segs), 'frames': frames, 'qt': qt, 'huffman': huffman, 'coef_blocks': coef, 'plane_bytes': plane,
            'out_bytes': 0 if dst_offsets is not None else dst}


def merge(packs, dst_bases):
    """packed forms of several samples -> one (what the loader's collate function does): frame, segment, byte, coefficient and plane offsets rebased,
    ``dst_off`` moved by the sample's base in the batch buffer"""
    out = {k: [] for k in ('scan', 'seg', 'frames', 'qt', 'huffman')}
    nf = ns = nb = coef = plane = 0
    for p, base in zip(packs, dst_bases):
        frames, seg = p['frames'].copy(), p['seg'].copy()
        frames[:, _COEF_OFF] += coef
        frames[:, _PLANE_OFF] += plane
        frames[:, _DST_OFF] += int(base)
        frames[:, _FIRST_SEG] += ns
        seg[:, 0] += nf
        seg[:, 1:3] += nb
        for k, v in (('scan', p['scan']), ('seg', seg), ('frames', frames), ('qt', p['qt']), ('huffman', p['huffman'])):
            out[k].append(v)
        nf, ns, nb = nf + len(frames), ns + len(seg), nb + len(p['scan'])
        coef, plane = coef + p['coef_blocks'], plane + p['plane_bytes']
    merged = {k: np.concatenate(v) for k, v in out.items()}
    merged.update(coef_blocks=coef, plane_bytes=plane, out_bytes=0)
    return merged
