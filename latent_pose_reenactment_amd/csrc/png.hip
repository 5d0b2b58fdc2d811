// Baseline PNG encoder for the lossless outputs (drive.py --format png --png_encoder gpu, utils/visualize.save_png(..., encoder='gpu')): uint8 frames
// on the device -> complete PNG files, back to back in one device buffer.  Only the compressed bytes cross PCIe.
//
// Definition (restated byte by byte in Python by tests/png_restatement.py, in vectorised numpy by hipops.png_encode_host).  All of it is integer
// arithmetic: device, host twin and restatement agree bit for bit.
// Input: uint8 frames [T][H][W][C], C = 1 (grey, colour type 0) or 3 (RGB, colour type 2), read through four element strides.  Bit depth 8, no
// interlace.  Output: T PNG files back to back in one uint8 buffer and an int64 table offsets[T + 1] (file t = bytes offsets[t] .. offsets[t + 1]).
//
// Filter.  Per row the five PNG filters (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth; bpp = C; the row above row 0 and the pixel left of column 0 are
// zeros) are formed, each scored by the sum of |filtered byte as int8|; the lowest score wins, ties go to the lowest filter type.  The frame's
// filtered stream is L = H x (1 + W C) bytes: per row its type byte, then its filtered bytes.
//
// Segments.  The stream is cut into segments of SEG = 16384 bytes (the last one shorter).  Segments are independent: no match reaches before its
// segment's first byte, every segment has its own code and ends on a byte boundary.
//
// Tokens of a segment f[0 .. n).  eq[i] = (i > 0 and f[i] == f[i - 1]).  A maximal stretch of eq of length r becomes floor(r / 258) matches of
// length 258 at distance 1, then, with q = r mod 258, one match of length q when q >= 3 and q literals when q < 3.  Every other byte is a literal;
// one end-of-block symbol (256) closes the segment.  There are no other matches (no general LZ77).
//
// Code.  The 286 literal/length symbols of the tokens are counted (n + 1 <= 16385 in all; at least two symbols occur: f[0] and 256).
//   1. The symbols with a count > 0 are the leaves, sorted ascending by (count, symbol).
//   2. Huffman: repeat until one node is left: take out the two smallest nodes and put in an internal node of their summed weight.  "Smallest" is by
//      (weight, internal node before leaf, internal nodes in order of creation, leaves in sorted order) -- the two-queue method with ties going to
//      the queue of internal nodes.  cnt[d] = the number of leaves at depth d.
//   3. Limit to 15: for D = the largest depth down to 16, while cnt[D] > 0: b = the largest depth <= 14 with cnt[b] > 0; cnt[b] -= 1,
//      cnt[b + 1] += 2, cnt[D] -= 2, cnt[D - 1] += 1 (a leaf at depth b becomes an internal node over itself and one leaf of a deepest sibling pair,
//      the other sibling takes their parent's place: the Kraft sum stays exactly 1).
//   4. Lengths by rank: going through the sorted leaves from the first (rarest), the first cnt[15] get length 15, the next cnt[14] length 14, ...
//   5. Canonical codes by RFC 1951 3.2.2.
// The distance alphabet is always one code, symbol 0, length 1 (the single incomplete code RFC 1951 allows), also when the segment has no match.
//
// Block.  The simplest legal dynamic header: BFINAL = 0, BTYPE = 2, HLIT = 29, HDIST = 0, HCLEN = 15; the code-length alphabet has length 4 for
// symbols 0 .. 15 and 0 for 16, 17, 18 (a complete code: symbol s is the 4-bit code s); all 286 + 1 code lengths are sent as one 4-bit code each.
// That is 17 + 57 + 287 x 4 = 1222 bits.  The repeat symbols 16 / 17 / 18 and a trimmed HLIT are left out on purpose: under 1 % of a segment, and no
// serial sub-coder.  Body: a literal is its code; a match is the code of its length symbol, the extra bits of the length, and the 1-bit distance code
// 0; then the code of 256.  Huffman codes enter the LSB-first bit stream most significant bit first, every other field least significant bit first.
// The dynamic block is followed by an empty stored block: 3 header bits (BFINAL = 1 in the frame's last segment, BTYPE = 0), zero bits to the byte,
// 00 00 FF FF.  dyn = ceil((1222 + body bits + 3) / 8) + 4 bytes is known before anything is packed.
// Stored fallback.  If dyn >= n + 5 the segment is ONE stored block instead (never after an attempt): a byte BFINAL (1 in the frame's last
// segment), n and ~n as 16-bit little-endian, the n bytes.  A tie goes to stored.
//
// Frame: zlib header 78 01, the segments, Adler-32 of the filtered stream (big-endian).  File: the PNG signature and IHDR (33 bytes), ONE IDAT
// holding the whole zlib stream, IEND.  Signature, IHDR and IEND with their CRCs are built on the host once per call (hipops._png_head, 45 bytes,
// passed to the write kernel by value); the IDAT CRC-32 over "IDAT" + data is computed on the device from per-slice CRCs joined by
// crc(A B) = crc(A) x^(8 |B|) + crc(B) in GF(2) modulo the CRC polynomial.  A file is 8 + 25 + 12 + 6 + 12 + sum(segment bytes) bytes, at most
// 63 + sum(n + 5).
//
// Launches.  lp_png_filter: ONE launch, a workgroup of 256 lanes per row: five scores (a fixed-order reduction), then the chosen filter's bytes.
// lp_png_deflate_size: TWO launches over a scratch of lp_png_deflate_scratch_bytes().  It takes ANY byte stream [T][L], so that a test can hand in
// a constructed one.
//   segment  a workgroup per segment, the segment in LDS, a lane per slice of 64 positions.  Exclusive max / min scans over the lanes give every
//            lane the last non-eq position before and the first one behind its slice, so a position's role follows from the start and length of
//            its own stretch without a serial parse.  Histogram with integer LDS atomics (counts do not depend on order); a rank sort of the 286
//            keys by all lanes; steps 2 .. 5 by lane 0; a scan of the lanes' token bits; every lane packs its tokens at its bit offset into the
//            CLEARED output image in LDS with integer atomicOr (every bit has one writer).  Then the segment's byte count, CRC-32 (a lane per
//            65-byte slice, joined as above), x^(8 bytes) and its Adler sums (sum f[i], sum (n - i) f[i], mod 65521) go into the tables and the image
//            into the segment's scratch slice of 16400 bytes (SEG + 5 rounded up to 16).  Differing from the sketch in the issue, the Adler partials
//            are per segment and not per row: the stage then needs nothing but the stream.
//   layout   one workgroup, a lane per frame: the frame's size, Adler-32 and IDAT CRC from the segment tables, a scan over the frames: the output
//            position of every segment and offsets[T + 1]; offsets[T] is the total.
// The host reads offsets[T] -- ONE device-to-host copy of one integer per call -- and allocates the output at its exact size.
// lp_png_write: ONE launch, a workgroup per segment: its bytes; in front of a frame's first one the signature, IHDR, the IDAT length and type and
// 78 01; behind its last one Adler-32, the CRC and IEND.  Every index is checked against out_bytes.
//
// No floating point, no floating-point atomics, no fences between workgroups; integer atomicOr / atomicAdd / atomicXor in LDS are order-independent:
// the output is bit-identical from run to run and a frame's bytes do not depend on T.  Everything is refused before any device work.
#include <stdio.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

#define PG_SEG 16384
#define PG_THREADS 256
#define PG_SLICE (PG_SEG / PG_THREADS)          // 64 positions per lane
#define PG_STRIDE 16400                         // bytes of a segment's scratch slice: SEG + 5 rounded up to 16
#define PG_OUT_WORDS (PG_STRIDE / 4)
#define PG_CRC_SLICE 65                         // 256 x 65 >= SEG + 5
#define PG_SYMS 286
#define PG_HDR_BITS 1222
#define PG_ADLER 65521u
#define PG_POLY 0xedb88320u
#define PG_HEAD 45                              // signature + IHDR (33) and IEND (12), from the host
#define PG_OVERHEAD 63                          // bytes of a file that are not segment bytes
#define PG_MAX_ROW (1 << 22)                    // W x C: the scores stay below 2^31
#define PG_MAX_DEPTH 40

// RFC 1951 3.2.5: length 3 .. 258 -> (symbol - 257) | extra bits << 8 | extra value << 16
struct PgLen { unsigned e[256]; };
constexpr PgLen pg_make_len() {
    const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    PgLen l = {};
    for (int len = 3; len <= 258; ++len) {
        int k = 0;
        for (int i = 0; i < 29; ++i)
            if (base[i] <= len) k = i;
        l.e[len - 3] = (unsigned)k | ((unsigned)extra[k] << 8) | ((unsigned)(len - base[k]) << 16);
    }
    return l;
}
__constant__ PgLen pg_len = pg_make_len();

struct PgSrc { const unsigned char* p; long long st, sh, sw, sc; };
struct PgHead { unsigned char b[48]; };

// ---- the filter ------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pg_paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ __forceinline__ int pg_filtered(int type, int x, int a, int b, int c) {
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? ((a + b) >> 1) : pg_paeth(a, b, c);
    return (x - pred) & 255;
}
__device__ __forceinline__ int pg_abs8(int v) { return v < 128 ? v : 256 - v; }

// grid = T x H rows.  out[t][row] = type byte + the W C filtered bytes
__global__ void __launch_bounds__(PG_THREADS) png_filter_kernel(PgSrc s, unsigned char* __restrict__ out, int H, int W, int C) {
    __shared__ int s_w[PG_THREADS / 64][5];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int row = (int)(blockIdx.x % (unsigned)H);
    const long long t = blockIdx.x / (unsigned)H;
    const int nb = W * C;
    const unsigned char* __restrict__ cur = s.p + t * s.st + (long long)row * s.sh;
    const unsigned char* __restrict__ up = cur - s.sh;          // only read when row > 0
    int score[5] = {0, 0, 0, 0, 0};
    for (int j = tid; j < nb; j += PG_THREADS) {
        const int x = j / C, ch = j - x * C;
        const long long at = (long long)x * s.sw + (long long)ch * s.sc;
        const int v = cur[at];
        const int a = x > 0 ? cur[at - s.sw] : 0;
        const int b = row > 0 ? up[at] : 0;
        const int c = (row > 0 && x > 0) ? up[at - s.sw] : 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) score[f] += pg_abs8(pg_filtered(f, v, a, b, c));
    }
#pragma unroll
    for (int f = 0; f < 5; ++f) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) score[f] += __shfl_down(score[f], o, 64);
        if (lane == 0) s_w[wv][f] = score[f];
    }
    __syncthreads();
    int best = 0, best_score = 0x7fffffff;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        int sum = 0;
#pragma unroll
        for (int i = 0; i < PG_THREADS / 64; ++i) sum += s_w[i][f];
        if (sum < best_score) { best_score = sum; best = f; }
    }
    unsigned char* __restrict__ o = out + (t * H + row) * (long long)(nb + 1);
    if (tid == 0) o[0] = (unsigned char)best;
    for (int j = tid; j < nb; j += PG_THREADS) {
        const int x = j / C, ch = j - x * C;
        const long long at = (long long)x * s.sw + (long long)ch * s.sc;
        const int v = cur[at];
        const int a = x > 0 ? cur[at - s.sw] : 0;
        const int b = row > 0 ? up[at] : 0;
        const int c = (row > 0 && x > 0) ? up[at - s.sw] : 0;
        o[1 + j] = (unsigned char)pg_filtered(best, v, a, b, c);
    }
}

// ---- CRC-32 and Adler-32 pieces ----------------------------------------------------------------------------------------------------------------------
// a(x) b(x) mod P(x), reflected representation (bit 31 = x^0), as zlib's multmodp
__device__ __forceinline__ unsigned pg_mulmod(unsigned a, unsigned b) {
    unsigned p = 0;
    for (unsigned m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b >> 1) ^ (PG_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8 n) mod P
__device__ __forceinline__ unsigned pg_xpow8(unsigned n) {
    unsigned p = 0x80000000u, base = 0x00800000u;          // 1 and x^8
    for (; n; n >>= 1) {
        if (n & 1u) p = pg_mulmod(p, base);
        base = pg_mulmod(base, base);
    }
    return p;
}
// the CRC-32 `crc` of a message continued by one byte
__device__ __forceinline__ unsigned pg_crc_byte(unsigned crc, unsigned byte) {
    unsigned c = ~crc ^ byte;
#pragma unroll
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (PG_POLY & (0u - (c & 1u)));
    return ~c;
}

// ---- the segment kernel ----------------------------------------------------------------------------------------------------------------------------
// exclusive max scan over the 256 lanes (identity -1) and exclusive min scan from the far end (identity `top`); s_w: 4 ints each
__device__ __forceinline__ int pg_scan_max_before(int v, int* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc = max(inc, up);
    }
    __syncthreads();
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int prev = __shfl_up(inc, 1, 64);
    if (lane == 0) prev = -1;
    for (int i = 0; i < wv; ++i) prev = max(prev, s_w[i]);
    return prev;
}
__device__ __forceinline__ int pg_scan_min_behind(int v, int top, int* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int dn = __shfl_down(inc, o, 64);
        if (lane + o < 64) inc = min(inc, dn);
    }
    __syncthreads();
    if (lane == 0) s_w[wv] = inc;
    __syncthreads();
    int next = __shfl_down(inc, 1, 64);
    if (lane == 63) next = top;
    for (int i = wv + 1; i < PG_THREADS / 64; ++i) next = min(next, s_w[i]);
    return next;
}
// exclusive sum scan over the 256 lanes; total = the sum
__device__ __forceinline__ unsigned pg_scan_sum(unsigned v, unsigned* s_w, unsigned& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    unsigned base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < PG_THREADS / 64; ++i) {
        const unsigned w = s_w[i];
        if (i < wv) base += w;
        total += w;
    }
    return base + inc - v;
}

// the tokens that START in positions a .. b - 1 of the segment f[0 .. n): last = the last non-eq position before a, next = the first one from b on (n
// if none).  A position's role follows from the start and the length of its own stretch
template <class Sink> __device__ __forceinline__ void pg_walk(const unsigned char* f, int a, int b, int last, int next, Sink& sink) {
    int p = a, cur_s = 0, cur_e = -1;
    while (p < b) {
        const int v = f[p];
        if (p == 0 || v != f[p - 1]) {
            last = p;
            sink.literal(v);
            ++p;
            continue;
        }
        if (p >= cur_e) {          // a stretch this lane has not measured yet
            cur_s = last + 1;
            int j = p + 1;
            while (j < b && f[j] == f[j - 1]) ++j;
            cur_e = j < b ? j : next;
        }
        const int r = cur_e - cur_s, k = p - cur_s, full = (r / 258) * 258, q = r - full;
        if (k < full) {
            const int i = k / 258;
            if (k == i * 258) sink.match(258);
            p = cur_s + (i + 1) * 258;
        } else if (q >= 3) {
            if (k == full) sink.match(q);
            p = cur_e;
        } else {
            sink.literal(v);
            ++p;
        }
    }
}

struct PgHist {
    unsigned* hist;
    __device__ __forceinline__ void literal(int v) { atomicAdd(&hist[v], 1u); }
    __device__ __forceinline__ void match(int len) { atomicAdd(&hist[257 + (pg_len.e[len - 3] & 255u)], 1u); }
};
struct PgCount {
    const unsigned char* len;
    unsigned bits;
    __device__ __forceinline__ void literal(int v) { bits += len[v]; }
    __device__ __forceinline__ void match(int l) {
        const unsigned e = pg_len.e[l - 3];
        bits += len[257 + (e & 255u)] + ((e >> 8) & 255u) + 1u;
    }
};
// `n` bits (<= 32) of v at bit position `bit` of the cleared LSB-first image w (PG_OUT_WORDS words)
__device__ __forceinline__ void pg_put_at(unsigned* w, unsigned bit, unsigned v, int n) {
    const unsigned long long x = (unsigned long long)v << (bit & 31u);
    const unsigned i = bit >> 5;
    if (i < PG_OUT_WORDS && (unsigned)x) atomicOr(&w[i], (unsigned)x);
    if (i + 1 < PG_OUT_WORDS && (unsigned)(x >> 32)) atomicOr(&w[i + 1], (unsigned)(x >> 32));
    (void)n;
}
struct PgPack {
    unsigned* w;
    const unsigned char* len;
    const unsigned short* code;          // bit-reversed: ready for the LSB-first stream
    unsigned long long acc;
    unsigned idx;
    int fill;
    __device__ __forceinline__ PgPack(unsigned* words, unsigned bit, const unsigned char* l, const unsigned short* c)
        : w(words), len(l), code(c), acc(0), idx(bit >> 5), fill((int)(bit & 31u)) {}
    __device__ __forceinline__ void put(unsigned v, int n) {          // n <= 21
        acc |= (unsigned long long)v << fill;
        fill += n;
        if (fill >= 32) {
            if (idx < PG_OUT_WORDS) atomicOr(&w[idx], (unsigned)acc);
            acc >>= 32;
            fill -= 32;
            ++idx;
        }
    }
    __device__ __forceinline__ void literal(int v) { put(code[v], len[v]); }
    __device__ __forceinline__ void match(int l) {
        const unsigned e = pg_len.e[l - 3], sym = 257u + (e & 255u), eb = (e >> 8) & 255u;
        const int sl = len[sym];
        put((unsigned)code[sym] | ((e >> 16) << sl), sl + (int)eb + 1);          // the distance code: one 0 bit
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0 && idx < PG_OUT_WORDS && (unsigned)acc) atomicOr(&w[idx], (unsigned)acc);
    }
};

// grid = T x nseg.  Tables per segment: bytes, crc, x^(8 bytes), Adler sums A and B; data: the segment's bytes at seg x PG_STRIDE
__global__ void __launch_bounds__(PG_THREADS) png_segment_kernel(const unsigned char* __restrict__ stream, long long L, int nseg, unsigned* __restrict__ seg_bytes,
                                                                 unsigned* __restrict__ seg_crc, unsigned* __restrict__ seg_xp, unsigned* __restrict__ seg_a,
                                                                 unsigned* __restrict__ seg_b, unsigned* __restrict__ data) {
    __shared__ __attribute__((aligned(16))) unsigned char s_in[PG_SEG];
    __shared__ __attribute__((aligned(16))) unsigned s_out[PG_OUT_WORDS];
    __shared__ unsigned s_hist[PG_SYMS], s_key[PG_SYMS], s_sorted[PG_SYMS], s_iw[PG_SYMS];
    __shared__ unsigned short s_par[2 * PG_SYMS], s_code[PG_SYMS];
    __shared__ unsigned char s_dep[PG_SYMS], s_len[PG_SYMS + 2];
    __shared__ int s_cnt[PG_MAX_DEPTH];
    __shared__ unsigned s_w[PG_THREADS / 64];
    __shared__ unsigned s_m, s_crcacc, s_aacc, s_bacc;
    const int tid = threadIdx.x;
    const int sf = (int)(blockIdx.x % (unsigned)nseg);
    const long long frame = blockIdx.x / (unsigned)nseg;
    const long long first = (long long)sf * PG_SEG;
    const int n = (int)min((long long)PG_SEG, L - first);
    const bool final_seg = sf == nseg - 1;
    const unsigned char* __restrict__ src = stream + frame * L + first;
    for (int i = tid; i < n; i += PG_THREADS) s_in[i] = src[i];
    for (int i = tid; i < PG_OUT_WORDS; i += PG_THREADS) s_out[i] = 0u;
    for (int i = tid; i < PG_SYMS; i += PG_THREADS) { s_hist[i] = 0u; s_len[i] = 0; s_code[i] = 0; }
    if (tid < PG_MAX_DEPTH) s_cnt[tid] = 0;
    if (tid == 0) { s_m = 0u; s_crcacc = 0u; s_aacc = 0u; s_bacc = 0u; }
    __syncthreads();

    // the lane's slice, the non-eq positions around it, and the Adler sums of the slice
    const int a = min(tid * PG_SLICE, n), b = min(a + PG_SLICE, n);
    int my_last = -1, my_first = n;
    unsigned sa = 0, sb = 0;
    for (int p = a; p < b; ++p) {
        const unsigned v = s_in[p];
        sa += v;
        sb += (unsigned)(n - p) * v;          // <= 64 x 16384 x 255
        if (p == 0 || v != s_in[p - 1]) {
            my_last = p;
            if (my_first == n) my_first = p;
        }
    }
    atomicAdd(&s_aacc, sa);          // <= 16384 x 255
    atomicAdd(&s_bacc, sb % PG_ADLER);
    const int last = pg_scan_max_before(my_last, (int*)s_w);
    const int next = pg_scan_min_behind(my_first, n, (int*)s_w);

    PgHist hist = {s_hist};
    pg_walk(s_in, a, b, last, next, hist);
    if (tid == 0) atomicAdd(&s_hist[256], 1u);
    __syncthreads();

    // step 1: the sorted leaves, by rank (the keys differ: the symbol is part of them)
    for (int i = tid; i < PG_SYMS; i += PG_THREADS) s_key[i] = s_hist[i] ? (s_hist[i] << 9) | (unsigned)i : 0xffffffffu;
    __syncthreads();
    for (int i = tid; i < PG_SYMS; i += PG_THREADS) {
        const unsigned k = s_key[i];
        if (k != 0xffffffffu) {
            int rank = 0;
            for (int j = 0; j < PG_SYMS; ++j) rank += s_key[j] < k;
            s_sorted[rank] = k;
            atomicAdd(&s_m, 1u);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int m = (int)s_m;          // 2 .. 286
        // step 2: leaves are nodes 0 .. m - 1, internal nodes m .. 2 m - 2 in order of creation
        int li = 0, ii = 0;
        for (int ni = 0; ni < m - 1; ++ni) {
            unsigned w = 0;
#pragma unroll
            for (int pick = 0; pick < 2; ++pick) {
                if (li < m && (ii >= ni || (s_sorted[li] >> 9) < s_iw[ii])) {
                    w += s_sorted[li] >> 9;
                    s_par[li++] = (unsigned short)(m + ni);
                } else {
                    w += s_iw[ii];
                    s_par[m + ii++] = (unsigned short)(m + ni);
                }
            }
            s_iw[ni] = w;
        }
        // depths: the root is internal node m - 2
        int maxd = 0;
        s_dep[m - 2] = 0;
        for (int j = m - 3; j >= 0; --j) s_dep[j] = (unsigned char)(s_dep[s_par[m + j] - m] + 1);
        for (int i = 0; i < m; ++i) {
            const int d = min(s_dep[s_par[i] - m] + 1, PG_MAX_DEPTH - 1);          // <= 22 for 16385 counted symbols
            s_cnt[d] += 1;
            maxd = max(maxd, d);
        }
        // step 3
        for (int D = maxd; D > 15; --D)
            while (s_cnt[D] > 0) {
                int bb = 14;
                while (bb > 1 && s_cnt[bb] == 0) --bb;
                s_cnt[bb] -= 1;
                s_cnt[bb + 1] += 2;
                s_cnt[D] -= 2;
                s_cnt[D - 1] += 1;
            }
        // step 4
        int i = 0;
        for (int l = 15; l >= 1; --l)
            for (int c = s_cnt[l]; c > 0 && i < m; --c) s_len[s_sorted[i++] & 511u] = (unsigned char)l;
        // step 5
        unsigned nextc[16];
        unsigned code = 0;
        nextc[0] = 0;
#pragma unroll
        for (int l = 1; l <= 15; ++l) {
            code = (code + (l > 1 ? (unsigned)s_cnt[l - 1] : 0u)) << 1;
            nextc[l] = code;
        }
        for (int s = 0; s < PG_SYMS; ++s) {
            const int l = s_len[s];
            if (!l) continue;
            unsigned c = 0;
#pragma unroll
            for (int k = 1; k <= 15; ++k)
                if (k == l) c = nextc[k]++;
            s_code[s] = (unsigned short)(__brev(c) >> (32 - l));
        }
    }
    __syncthreads();

    PgCount cnt = {s_len, 0u};
    pg_walk(s_in, a, b, last, next, cnt);
    unsigned body;
    const unsigned at = pg_scan_sum(cnt.bits, s_w, body);
    const unsigned eob = PG_HDR_BITS + body;
    const unsigned dyn_bits = eob + s_len[256] + 3u;
    const unsigned dyn_bytes = ((dyn_bits + 7u) >> 3) + 4u;
    const bool stored = dyn_bytes >= (unsigned)n + 5u;          // (uniform)
    const unsigned nbytes = stored ? (unsigned)n + 5u : dyn_bytes;
    if (stored) {
        unsigned char* o = (unsigned char*)s_out;
        if (tid == 0) {
            o[0] = final_seg ? 1 : 0;
            o[1] = (unsigned char)(n & 255);
            o[2] = (unsigned char)(n >> 8);
            o[3] = (unsigned char)(~n & 255);
            o[4] = (unsigned char)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += PG_THREADS) o[5 + i] = s_in[i];
    } else {
        if (tid == 0) {
            // BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; the 19 code-length-code lengths in the order 16 17 18 0 8 7 ...: 0 0 0 and sixteen 4s
            pg_put_at(s_out, 0, 0u | (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13), 17);
            for (int k = 3; k < 19; ++k) pg_put_at(s_out, 17u + 3u * k, 4u, 3);
            pg_put_at(s_out, eob, s_code[256], s_len[256]);
            pg_put_at(s_out, eob + s_len[256], final_seg ? 1u : 0u, 3);
            pg_put_at(s_out, 8u * (dyn_bytes - 4u), 0xffff0000u, 32);
        }
        for (int i = tid; i < PG_SYMS + 1; i += PG_THREADS) {
            const unsigned l = i < PG_SYMS ? s_len[i] : 1u;          // the one distance code
            pg_put_at(s_out, 74u + 4u * i, __brev(l) >> 28, 4);
        }
        PgPack pack(s_out, PG_HDR_BITS + at, s_len, s_code);
        pg_walk(s_in, a, b, last, next, pack);
        pack.finish();
    }
    __syncthreads();

    // the CRC of the segment's bytes from the lanes' slices
    {
        const unsigned char* o = (const unsigned char*)s_out;
        const unsigned c0 = min((unsigned)tid * PG_CRC_SLICE, nbytes), c1 = min(c0 + PG_CRC_SLICE, nbytes);
        if (c1 > c0) {
            unsigned crc = 0;
            for (unsigned i = c0; i < c1; ++i) crc = pg_crc_byte(crc, o[i]);
            atomicXor(&s_crcacc, pg_mulmod(crc, pg_xpow8(nbytes - c1)));
        }
    }
    unsigned* __restrict__ dst = data + (size_t)blockIdx.x * PG_OUT_WORDS;
    for (unsigned i = tid; 4u * i < nbytes && i < PG_OUT_WORDS; i += PG_THREADS) dst[i] = s_out[i];
    __syncthreads();
    if (tid == 0) {
        seg_bytes[blockIdx.x] = nbytes;
        seg_crc[blockIdx.x] = s_crcacc;
        seg_xp[blockIdx.x] = pg_xpow8(nbytes);
        seg_a[blockIdx.x] = s_aacc % PG_ADLER;
        seg_b[blockIdx.x] = s_bacc % PG_ADLER;
    }
}

// layout: ONE workgroup, a lane per frame.  frame_sum[t] = {Adler-32, IDAT CRC}; seg_dst[segment] = where its bytes go; offsets[T + 1]
__global__ void __launch_bounds__(PG_THREADS) png_layout_kernel(const unsigned* __restrict__ seg_bytes, const unsigned* __restrict__ seg_crc,
                                                                const unsigned* __restrict__ seg_xp, const unsigned* __restrict__ seg_a,
                                                                const unsigned* __restrict__ seg_b, int T, long long L, int nseg,
                                                                long long* __restrict__ seg_dst, unsigned* __restrict__ frame_sum,
                                                                long long* __restrict__ offsets) {
    __shared__ long long s_w[PG_THREADS / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    long long carry = 0;
    for (int base = 0; base < T; base += PG_THREADS) {          // (uniform)
        const int t = base + threadIdx.x;
        const bool live = t < T;
        long long size = 0;
        if (live) {
            size = PG_OVERHEAD;
            unsigned crc = 0, ad_a = 1, ad_b = 0;
            const unsigned char idat[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
#pragma unroll
            for (int i = 0; i < 6; ++i) crc = pg_crc_byte(crc, idat[i]);
            for (int sgi = 0; sgi < nseg; ++sgi) {
                const size_t g = (size_t)t * nseg + sgi;
                const unsigned n = (unsigned)min((long long)PG_SEG, L - (long long)sgi * PG_SEG);
                size += seg_bytes[g];
                crc = pg_mulmod(crc, seg_xp[g]) ^ seg_crc[g];
                ad_b = (unsigned)(((unsigned long long)ad_b + (unsigned long long)n * ad_a + seg_b[g]) % PG_ADLER);
                ad_a = (ad_a + seg_a[g]) % PG_ADLER;
            }
            const unsigned adler = (ad_b << 16) | ad_a;
#pragma unroll
            for (int i = 0; i < 4; ++i) crc = pg_crc_byte(crc, (adler >> (24 - 8 * i)) & 255u);
            frame_sum[2 * t] = adler;
            frame_sum[2 * t + 1] = crc;
        }
        long long inc = size;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        __syncthreads();
        if (lane == 63) s_w[wv] = inc;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int i = 0; i < PG_THREADS / 64; ++i) {
            if (i < wv) before += s_w[i];
            total += s_w[i];
        }
        if (live) {
            long long at = carry + before + inc - size;
            offsets[t] = at;
            at += 33 + 8 + 2;
            for (int sgi = 0; sgi < nseg; ++sgi) {
                const size_t g = (size_t)t * nseg + sgi;
                seg_dst[g] = at;
                at += seg_bytes[g];
            }
        }
        carry += total;
    }
    if (threadIdx.x == 0) offsets[T] = carry;
}

// write: grid = T x nseg.  Every index is checked against out_bytes
__global__ void __launch_bounds__(PG_THREADS) png_write_kernel(const unsigned* __restrict__ seg_bytes, const long long* __restrict__ seg_dst,
                                                               const unsigned* __restrict__ frame_sum, const long long* __restrict__ offsets,
                                                               const unsigned* __restrict__ data, int nseg, PgHead head,
                                                               unsigned char* __restrict__ out, long long out_bytes) {
    const int tid = threadIdx.x;
    const int sf = (int)(blockIdx.x % (unsigned)nseg);
    const long long t = blockIdx.x / (unsigned)nseg;
    const unsigned nbytes = min(seg_bytes[blockIdx.x], (unsigned)PG_STRIDE);
    const long long dst = seg_dst[blockIdx.x];
    const unsigned char* __restrict__ src = (const unsigned char*)(data + (size_t)blockIdx.x * PG_OUT_WORDS);
    for (unsigned i = tid; i < nbytes; i += PG_THREADS) {
        const long long at = dst + i;
        if (at >= 0 && at < out_bytes) out[at] = src[i];
    }
    if (sf == 0 && tid < 43) {
        const long long o0 = offsets[t], idat = offsets[t + 1] - o0 - (PG_OVERHEAD - 6);          // the zlib stream's length
        unsigned char v;
        if (tid < 33) v = head.b[tid];
        else if (tid < 37) v = (unsigned char)((unsigned long long)idat >> (8 * (36 - tid)));
        else if (tid == 37) v = 'I';
        else if (tid == 38) v = 'D';
        else if (tid == 39) v = 'A';
        else if (tid == 40) v = 'T';
        else if (tid == 41) v = 0x78;
        else v = 0x01;
        const long long at = o0 + tid;
        if (at >= 0 && at < out_bytes) out[at] = v;
    }
    if (sf == nseg - 1 && tid >= 64 && tid < 64 + 20) {
        const int k = tid - 64;
        unsigned char v;
        if (k < 4) v = (unsigned char)(frame_sum[2 * t] >> (24 - 8 * k));
        else if (k < 8) v = (unsigned char)(frame_sum[2 * t + 1] >> (24 - 8 * (k - 4)));
        else v = head.b[33 + k - 8];
        const long long at = dst + nbytes + k;
        if (at >= 0 && at < out_bytes) out[at] = v;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
struct PgLayout { long long seg_bytes, seg_crc, seg_xp, seg_a, seg_b, seg_dst, frame_sum, data, total, segs; int nseg; };

static inline long long pg_up16(long long v) { return (v + 15) / 16 * 16; }

static int pg_refuse(const char* who, int code, const char* why) {
    static thread_local char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return lp_set_error(code, msg);
}

// NULL when the geometry is fine, the refusal otherwise
static const char* pg_layout(int T, long long L, PgLayout& P, int& code) {
    code = LP_ERR_ARG;
    if (T < 1 || L < 1) return "T and the stream length must be >= 1";
    code = LP_ERR_UNSUPPORTED;
    if (L > 0x7fffffffLL || (long long)T * L > 0x7fffffffLL) return "the filtered streams would exceed 2^31 - 1 bytes: encode fewer frames per call";
    P.nseg = (int)((L + PG_SEG - 1) / PG_SEG);
    P.segs = (long long)T * P.nseg;
    if (P.segs > 0x7fffffffLL / PG_STRIDE) return "the scratch would exceed 2^31 - 1 bytes: encode fewer frames per call";
    P.seg_bytes = 0;
    P.seg_crc = P.seg_bytes + pg_up16(P.segs * 4);
    P.seg_xp = P.seg_crc + pg_up16(P.segs * 4);
    P.seg_a = P.seg_xp + pg_up16(P.segs * 4);
    P.seg_b = P.seg_a + pg_up16(P.segs * 4);
    P.seg_dst = P.seg_b + pg_up16(P.segs * 4);
    P.frame_sum = P.seg_dst + pg_up16(P.segs * 8);
    P.data = P.frame_sum + pg_up16((long long)T * 8);
    P.total = P.data + P.segs * PG_STRIDE;
    if (P.total > 0x7fffffffLL) return "the scratch would exceed 2^31 - 1 bytes: encode fewer frames per call";
    return nullptr;
}

extern "C" int lp_png_filter(const unsigned char* frames, const long long* strides, int T, int H, int W, int C, unsigned char* filtered, void* stream) {
    const char* who = "lp_png_filter";
    if (!frames || !strides || !filtered) return pg_refuse(who, LP_ERR_ARG, "null pointer");
    if (T < 1 || H < 1 || W < 1) return pg_refuse(who, LP_ERR_ARG, "T >= 1, H >= 1 and W >= 1 are required");
    if (C != 1 && C != 3) return pg_refuse(who, LP_ERR_ARG, "C must be 1 (grey) or 3 (RGB)");
    if ((long long)W * C > PG_MAX_ROW) return pg_refuse(who, LP_ERR_UNSUPPORTED, "a row of more than 4194304 bytes (W x C)");
    if ((long long)T * H > 0x7fffffffLL) return pg_refuse(who, LP_ERR_UNSUPPORTED, "T x H exceeds one launch grid");
    const long long L = (long long)H * (1 + (long long)W * C);
    if (L > 0x7fffffffLL || (long long)T * L > 0x7fffffffLL)
        return pg_refuse(who, LP_ERR_UNSUPPORTED, "the filtered streams would exceed 2^31 - 1 bytes: encode fewer frames per call");
    const PgSrc s = {frames, strides[0], strides[1], strides[2], strides[3]};
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((long long)T * H)), dim3(PG_THREADS), 0, (hipStream_t)stream, s, filtered, H, W, C);
    return lp_check_launch("png_filter");
}

extern "C" long long lp_png_deflate_scratch_bytes(int T, long long L) {
    PgLayout P;
    int code;
    if (const char* why = pg_layout(T, L, P, code)) return pg_refuse("lp_png_deflate_scratch_bytes", code, why);
    return P.total;
}

extern "C" int lp_png_deflate_size(const unsigned char* filtered, int T, long long L, void* scratch, long long scratch_bytes, long long* offsets,
                                   void* stream) {
    const char* who = "lp_png_deflate_size";
    if (!filtered || !scratch || !offsets) return pg_refuse(who, LP_ERR_ARG, "null pointer");
    if ((uintptr_t)scratch & 15) return pg_refuse(who, LP_ERR_ARG, "scratch must be 16-byte aligned");
    PgLayout P;
    int code;
    if (const char* why = pg_layout(T, L, P, code)) return pg_refuse(who, code, why);
    if (scratch_bytes < P.total) return pg_refuse(who, LP_ERR_ARG, "scratch smaller than lp_png_deflate_scratch_bytes()");
    char* base = (char*)scratch;
    unsigned* seg_bytes = (unsigned*)(base + P.seg_bytes);
    unsigned* seg_crc = (unsigned*)(base + P.seg_crc);
    unsigned* seg_xp = (unsigned*)(base + P.seg_xp);
    unsigned* seg_a = (unsigned*)(base + P.seg_a);
    unsigned* seg_b = (unsigned*)(base + P.seg_b);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)P.segs), dim3(PG_THREADS), 0, st, filtered, L, P.nseg, seg_bytes, seg_crc, seg_xp, seg_a, seg_b,
                       (unsigned*)(base + P.data));
    hipLaunchKernelGGL(png_layout_kernel, dim3(1), dim3(PG_THREADS), 0, st, seg_bytes, seg_crc, seg_xp, seg_a, seg_b, T, L, P.nseg,
                       (long long*)(base + P.seg_dst), (unsigned*)(base + P.frame_sum), offsets);
    return lp_check_launch("png_deflate_size");
}

extern "C" int lp_png_write(const void* scratch, long long scratch_bytes, int T, long long L, const unsigned char* head, const long long* offsets,
                            unsigned char* out, long long out_bytes, void* stream) {
    const char* who = "lp_png_write";
    if (!scratch || !head || !offsets || !out) return pg_refuse(who, LP_ERR_ARG, "null pointer");
    if ((uintptr_t)scratch & 15) return pg_refuse(who, LP_ERR_ARG, "scratch must be 16-byte aligned");
    if (out_bytes < 1) return pg_refuse(who, LP_ERR_ARG, "out_bytes must be the total lp_png_deflate_size left in offsets[T]");
    if (out_bytes > 0x7fffffffLL) return pg_refuse(who, LP_ERR_UNSUPPORTED, "the output would exceed 2^31 - 1 bytes: encode fewer frames per call");
    PgLayout P;
    int code;
    if (const char* why = pg_layout(T, L, P, code)) return pg_refuse(who, code, why);
    if (scratch_bytes < P.total) return pg_refuse(who, LP_ERR_ARG, "scratch smaller than lp_png_deflate_scratch_bytes()");
    PgHead h = {};
    for (int i = 0; i < PG_HEAD; ++i) h.b[i] = head[i];
    const char* base = (const char*)scratch;
    hipLaunchKernelGGL(png_write_kernel, dim3((unsigned)P.segs), dim3(PG_THREADS), 0, (hipStream_t)stream, (const unsigned*)(base + P.seg_bytes),
                       (const long long*)(base + P.seg_dst), (const unsigned*)(base + P.frame_sum), offsets, (const unsigned*)(base + P.data), P.nseg, h,
                       out, out_bytes);
    return lp_check_launch("png_write");
}
