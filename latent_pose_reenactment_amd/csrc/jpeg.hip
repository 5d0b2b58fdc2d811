// Baseline JPEG encoder for the drive output (drive.py --format avi): uint8 RGB frames on the device -> complete JFIF files, back to back in one
// device buffer, which utils/mjpeg.AviWriter wraps into a Motion-JPEG AVI.  Only the compressed bytes cross PCIe.
//
// Definition (restated in fp64 / integers by tests/jpeg_restatement.py, in torch and numpy ops by hipops.jpeg_encode_host).
// Input: uint8 frames [T][H][W][3] (RGB), read through four element strides; H, W in 1 .. 65535.  rows = ceil(H / 8), mcus = ceil(W / 8).
// Output: T baseline-sequential JFIF files back to back in one uint8 buffer and an int64 table offsets[T + 1] (file t = bytes offsets[t] ..
// offsets[t + 1]).
//
// Per-frame layout: SOI, APP0 (JFIF 1.01, density 1:1, no units), DQT (table 0), DQT (table 1), SOF0 (8 bits, H, W, three components with 1 x 1
// sampling -- 4:4:4 --, component 1 on table 0, components 2 and 3 on table 1), four DHT (the Annex K.3 tables: DC luminance, AC luminance, DC
// chrominance, AC chrominance), DRI = mcus (one restart interval = one MCU row), SOS, the scan, EOI.  That is the segment order and the DHT / DRI
// content PIL writes with subsampling=0, restart_marker_rows=1.  The header is the same for every frame of a call: utils/mjpeg.jpeg_header
// builds it on the host once per (H, W, quality) and it is uploaded; this file never looks inside it.
//
// Quantisation tables: q[u][v] (u the vertical frequency) = clamp(floor((K[u][v] s + 50) / 100), 1, 255) in integer arithmetic, K = Annex K.1
// for table 0 and K.2 for table 1, s = 5000 / quality (integer division) below 50 and 200 - 2 quality from 50 on (IJG), quality an integer in
// 1 .. 100.  Computed ONCE on the host (utils/mjpeg.quant_tables) and handed to lp_jpeg_transform as 2 x 64 bytes in natural (row-major) order;
// the same integers go into the DQT segments in zigzag order.
//
// Coefficients: 8 x 8 blocks anchored at (0, 0); a block that overhangs the right or bottom edge replicates the last column / row.
//      Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,  Cr = 0.5 R - 0.418688 G - 0.081312 B
// in fp32 (JFIF; the + 128 of the chroma planes cancelled by the level shift).  Per plane and block the orthonormal DCT-II D = C X C^T,
// C[k][n] = a(k) cos((2 n + 1) k pi / 16), a(0) = sqrt(1 / 8), a(k) = 1 / 2: rows first, then columns, each an 8-term fp32 sum from n = 0.
// k = rint(D / q) (ties to even, fp32 division) as int16, clamped to -1023 .. 1023 (AC) and -1024 .. 1023 (DC): the clamp cannot bind for 8-bit
// input (|D| <= 8 x 128); it is there so that no value can index outside a code table.  Stored in zigzag order: coefs[T][rows][mcus][3][64].
//
// Scan: MCUs left to right, top to bottom; an MCU = one block each of Y, Cb, Cr.  The coder takes ANY int16 table of that shape and applies the
// same clamps first.  DC: the difference to the previous block of the same component, the predictors reset to 0 at the start of every restart
// interval (= MCU row); coded as the category's Huffman code followed by the category's extra bits (negative values: value - 1, low bits).
// AC, in zigzag order: (run, size) symbols followed by size extra bits, ZRL (0xF0) for every 16 zeros in front of a non-zero coefficient, EOB
// (0x00) unless coefficient 63 is non-zero.  Bits MSB first; at the end of an interval the last byte is filled with 1-bits; after every interval
// but the last RSTm, m = MCU-row index mod 8; after the last EOI.  Every 0xFF byte of entropy data, a padded last byte included, is followed by
// 0x00.
//
// Launches.  lp_jpeg_transform: ONE launch with the tile scheme of augment_extra.hip: a workgroup of 256 lanes = one frame x one 16 x 16 pixel
// tile = 2 x 2 blocks x 3 planes; the planes sit in LDS as [plane][16][16], the row and the column pass run from LDS with one value per lane and
// plane (the bank reasoning of augment_extra.hip holds: basis at a row stride of 9), the results leave as 16-bit stores.
// lp_jpeg_entropy_size: FOUR launches over a scratch of lp_jpeg_entropy_scratch_bytes():
//   count   a workgroup per interval, a lane per block: the block's exact bit count; a scan gives every block its bit offset inside the interval
//           and the interval its unstuffed byte length ceil(bits / 8).  The workgroup then clears the interval's words, the last one already
//           holding the 1-bits of the padding.  An interval owns a fixed slice of mcus x 3 x 52 words: a block has at most 22 + 63 x 26 = 1660 bits
//           (DC: 11 + 11; AC: 16 + 10 each) <= 52 x 32, so the worst case fits and only ceil(bits / 32) words of a slice are ever touched.
//   pack    a lane per block writes its codes at its bit offset: whole 32-bit words are assembled in a register and stored; the first and the last
//           word of a block, which it shares with its neighbours (or the padding), are combined with an integer atomicOr.  OR is commutative
//           and every bit has one writer, so the bytes do not depend on the order of arrival.
//   stuff   a workgroup per interval counts the 0xFF bytes: stuffed length = bytes + count.
//   layout  one workgroup scans header + stuffed length + 2 (RSTm or EOI) over the intervals of all frames: the output position of every interval
//           and offsets[T + 1]; offsets[T] is the total.
// The host reads offsets[T] -- ONE device-to-host copy of one integer per call -- and allocates the output at its exact size.
// lp_jpeg_entropy_write: ONE launch, a workgroup per interval: the header (first interval of a frame), the scan bytes with their stuffing (a scan
// over the 0xFF flags gives every byte its place) and the marker behind them.
//
// Every store is bounded by a size computed before it: the transform stores by (frame, block row, block column) inside the grid of the call; a
// block's bits end where the count pass measured them with the same walk; write checks every index against out_bytes and caps what it reads from
// the scratch at the slice.  No floating-point atomics; the integer atomicOr is order-independent: the output is bit-identical from run to run
// and a frame's bytes do not depend on T.  Everything is refused before any device work (LP_ERR_ARG / LP_ERR_UNSUPPORTED).
#include <math.h>
#include <stdio.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file, as in augment_extra.hip (tests/test_isa_lint.py).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define JP_TILE 16
#define JP_THREADS 256
#define JP_CSTRIDE 9
#define JP_BLOCK_WORDS 52          // ceil(1660 / 32): the longest block
#define JP_DC 12                   // DC categories 0 .. 11
#define JP_MAX_DIM 65535           // SOF0 holds H and W in 16 bits

// C[k][n] = a(k) cos((2 n + 1) k pi / 16), rounded to fp32
__constant__ float jp_dct[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f,
};

// ITU-T T.81 Figure A.6: zigzag position -> natural (row-major) index
struct JpZigzag { unsigned char pos[64]; };          // natural index -> zigzag position
constexpr JpZigzag jp_make_zigzag() {
    const unsigned char order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    JpZigzag z = {};
    for (int i = 0; i < 64; ++i) z.pos[order[i]] = (unsigned char)i;
    return z;
}
__constant__ JpZigzag jp_zigzag = jp_make_zigzag();

// ITU-T T.81 Annex K.3: BITS (codes per length 1 .. 16) and HUFFVAL of the four typical tables
struct JpSpec { unsigned char bits[16]; unsigned char vals[162]; int count; };
constexpr JpSpec jp_dc_spec[2] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12},
};
constexpr JpSpec jp_ac_spec[2] = {
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
      0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
      0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
      0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
      0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
      0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
      0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
      0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
      0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
      0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
      0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
      0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
      0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
     162},
};

// the code tables by symbol: (code << 5) | length, 0 for a symbol the table does not hold.  Annex C: the codes of one length are consecutive, the
// first code of the next length is (last + 1) << 1.  table[0 .. 23]: DC [2][12]; table[24 .. 535]: AC [2][256]
#define JP_LUT_WORDS (2 * JP_DC + 2 * 256)
struct JpLut { unsigned e[JP_LUT_WORDS]; };
constexpr void jp_fill(unsigned* dst, const JpSpec& s) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) dst[s.vals[k++]] = (code++ << 5) | (unsigned)len;
        code <<= 1;
    }
}
constexpr JpLut jp_make_lut() {
    JpLut l = {};
    for (int t = 0; t < 2; ++t) {
        jp_fill(l.e + t * JP_DC, jp_dc_spec[t]);
        jp_fill(l.e + 2 * JP_DC + t * 256, jp_ac_spec[t]);
    }
    return l;
}
static constexpr JpLut jp_lut_host = jp_make_lut();
__constant__ JpLut jp_lut = jp_make_lut();

struct JpQ { unsigned char q[128]; };          // [table][u * 8 + v]
struct JpSrc { const unsigned char* p; long long st, sh, sw, sc; };

// ---- the transform ---------------------------------------------------------------------------------------------------------------------------------
// one 1-D pass of one plane: sum_i coef[cbase + i] * plane[base + i step], i = 0 .. 7, added up from 0
__device__ __forceinline__ float jp_sum8(const float* __restrict__ plane, int base, int step, const float* __restrict__ coef, int cbase) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += coef[cbase + i] * plane[base + i * step];
    return acc;
}

__global__ void __launch_bounds__(JP_THREADS) jpeg_transform_kernel(JpSrc s, JpQ qt, short* __restrict__ coefs, int H, int W, int rows, int mcus) {
    __shared__ float s_d[3][JP_TILE * JP_TILE];          // the planes of the tile: [plane][row * 16 + column]
    __shared__ float s_c[8 * JP_CSTRIDE];                // the DCT basis: [k * 9 + n]
    const int tid = threadIdx.x, t = blockIdx.z;
    const int y0 = blockIdx.y * JP_TILE, x0 = blockIdx.x * JP_TILE;
    // lane -> pixel of the tile; beyond the edge: the last row / column (the replication of the definition)
    const int ty = tid >> 4, tx = tid & (JP_TILE - 1);
    const int y = min(y0 + ty, H - 1), x = min(x0 + tx, W - 1);
    const unsigned char* __restrict__ px = s.p + (long long)t * s.st + (long long)y * s.sh + (long long)x * s.sw;
    const float R = (float)px[0], G = (float)px[s.sc], B = (float)px[2 * s.sc];
    const int at = ty * JP_TILE + tx;
    if (tid < 64) s_c[(tid >> 3) * JP_CSTRIDE + (tid & 7)] = jp_dct[tid];
    s_d[0][at] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
    s_d[1][at] = -0.168736f * R - 0.331264f * G + 0.5f * B;
    s_d[2][at] = 0.5f * R - 0.418688f * G - 0.081312f * B;
    __syncthreads();
    const int ku = ty & 7, kv = tx & 7;          // the lane's frequency inside its block
    const int row = ty * JP_TILE + (tx & 8), col = (ty & 8) * JP_TILE + tx;
    float a[3];
    // rows: D1[y][v] = sum_n C[v][n] X[y][n]
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = jp_sum8(s_d[c], row, 1, s_c, kv * JP_CSTRIDE);
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s_d[c][at] = a[c];
    __syncthreads();
    // columns: D[u][v] = sum_n C[u][n] D1[n][v]
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = jp_sum8(s_d[c], col, JP_TILE, s_c, ku * JP_CSTRIDE);
    // a tile covers 2 x 2 blocks; the ones beyond the block grid (H or W <= 8 below a tile boundary) are not stored
    const int by = (y0 >> 3) + (ty >> 3), bx = (x0 >> 3) + (tx >> 3);
    if (by >= rows || bx >= mcus) return;
    const int n = ku * 8 + kv;
    const int lo = n == 0 ? -1024 : -1023;
    short* __restrict__ o = coefs + ((((size_t)t * rows + by) * mcus + bx) * 3) * 64 + jp_zigzag.pos[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q = (float)qt.q[(c ? 64 : 0) + n];
        const float k = fminf(fmaxf(rintf(a[c] / q), (float)lo), 1023.f);
        o[c * 64] = (short)(int)k;
    }
}

// ---- the entropy coder -----------------------------------------------------------------------------------------------------------------------------
// exclusive scan over the 256 lanes of a workgroup (every lane calls it); total = the sum
template <class T> __device__ __forceinline__ T jp_block_scan(T v, T* s_w, T& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();          // s_w may still be read from the call before
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < JP_THREADS / 64; ++i) {
        const T w = s_w[i];
        if (i < wv) base += w;
        total += w;
    }
    return base + inc - v;
}

__device__ __forceinline__ int jp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ __forceinline__ int jp_size(int v) { return 32 - __clz(abs(v)); }          // 0 for 0; callers pass |v| <= 2047
// the extra bits of a value of `size` bits: the value, or value - 1 for a negative one, low `size` bits
__device__ __forceinline__ unsigned jp_extra(int v, int size) { return (unsigned)(v + (v >> 31)) & ((1u << size) - 1u); }

struct JpCount {
    unsigned bits = 0;
    __device__ __forceinline__ void put(unsigned, int len) { bits += (unsigned)len; }
};

// MSB-first bit writer at a bit offset of a zeroed word array whose bytes are the stream: a word is assembled big-endian in a register and leaves
// byte-swapped.  The first word when the block starts inside it, and the last one when the block ends inside it, have other writers: atomicOr
struct JpPack {
    unsigned* w;          // the next word to leave
    unsigned acc;         // the bits gathered for it, from the top
    int fill;             // how many of its bits are accounted for (the neighbour's included)
    bool shared;          // the word has bits of the block in front
    __device__ __forceinline__ JpPack(unsigned* words, unsigned bit) : w(words + (bit >> 5)), acc(0), fill((int)(bit & 31)), shared((bit & 31) != 0) {}
    __device__ __forceinline__ void flush() {
        const unsigned v = __builtin_bswap32(acc);
        if (shared) atomicOr(w, v);
        else *w = v;
        ++w; shared = false;
    }
    // code: `len` bits (1 .. 26), nothing above them
    __device__ __forceinline__ void put(unsigned code, int len) {
        const int room = 32 - fill;
        if (len < room) {
            acc |= code << (room - len);
            fill += len;
        } else {
            const int rest = len - room;          // 0 .. 25
            acc |= code >> rest;
            flush();
            acc = rest ? code << (32 - rest) : 0u;
            fill = rest;
        }
    }
    __device__ __forceinline__ void finish() {
        if (fill > 0) atomicOr(w, __builtin_bswap32(acc));          // shared with the block behind, or with the padding
    }
};

// the symbols of one block: blk = its 64 coefficients in zigzag order (16-byte aligned), pred = the DC predictor, tab = 0 luminance, 1 chrominance
template <class Sink> __device__ __forceinline__ void jp_walk(const short* __restrict__ blk, int pred, int tab, const unsigned* __restrict__ s_lut, Sink& sink) {
    short c[64];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const s16x8_t v = *(const s16x8_t*)(blk + 8 * i);
#pragma unroll
        for (int j = 0; j < 8; ++j) c[8 * i + j] = v[j];
    }
    const unsigned* __restrict__ dc = s_lut + tab * JP_DC;
    const unsigned* __restrict__ ac = s_lut + 2 * JP_DC + tab * 256;
    const int diff = jp_clamp(c[0], -1024, 1023) - pred;
    const int cat = jp_size(diff);          // 0 .. 11
    const unsigned e = dc[cat];
    sink.put(((e >> 5) << cat) | jp_extra(diff, cat), (int)(e & 31u) + cat);
    int run = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) {
        const int v = jp_clamp(c[k], -1023, 1023);
        if (v == 0) { ++run; continue; }
        while (run >= 16) {
            const unsigned z = ac[0xF0];
            sink.put(z >> 5, (int)(z & 31u));
            run -= 16;
        }
        const int size = jp_size(v);          // 1 .. 10
        const unsigned s = ac[(run << 4) | size];
        sink.put(((s >> 5) << size) | jp_extra(v, size), (int)(s & 31u) + size);
        run = 0;
    }
    if (run > 0) {
        const unsigned z = ac[0x00];
        sink.put(z >> 5, (int)(z & 31u));
    }
}

__device__ __forceinline__ void jp_load_lut(unsigned* s_lut) {
    for (int i = threadIdx.x; i < JP_LUT_WORDS; i += JP_THREADS) s_lut[i] = jp_lut.e[i];
    __syncthreads();
}

// the DC predictor of block j (= mcu * 3 + component) of an interval: the previous MCU's block of the same component, 0 for the first MCU
__device__ __forceinline__ int jp_pred(const short* __restrict__ blk, int j) { return j < 3 ? 0 : jp_clamp(blk[-3 * 64], -1024, 1023); }

// count: grid = intervals.  blkoff[interval][j] = the bit offset of block j; ibytes[interval]; the interval's words cleared, padding in place
__global__ void __launch_bounds__(JP_THREADS) jpeg_count_kernel(const short* __restrict__ coefs, int nb, unsigned* __restrict__ blkoff,
                                                                unsigned* __restrict__ ibytes, unsigned* __restrict__ words, unsigned stride_words) {
    __shared__ unsigned s_lut[JP_LUT_WORDS];
    __shared__ unsigned s_w[JP_THREADS / 64];
    const int tid = threadIdx.x;
    const size_t first = (size_t)blockIdx.x * nb;
    jp_load_lut(s_lut);
    unsigned carry = 0;
    for (int base = 0; base < nb; base += JP_THREADS) {          // (uniform)
        const int j = base + tid;
        JpCount cnt;
        if (j < nb) {
            const short* blk = coefs + (first + j) * 64;
            jp_walk(blk, jp_pred(blk, j), j % 3 != 0, s_lut, cnt);
        }
        unsigned total;
        const unsigned excl = jp_block_scan(cnt.bits, s_w, total);
        if (j < nb) blkoff[first + j] = carry + excl;
        carry += total;
    }
    const unsigned tot = carry, nbytes = (tot + 7u) >> 3, nwords = (tot + 31u) >> 5;          // tot <= nb * 1660 <= 32 stride_words
    if (tid == 0) ibytes[blockIdx.x] = nbytes;
    unsigned* __restrict__ w = words + (size_t)blockIdx.x * stride_words;
    for (unsigned i = tid; i < nwords && i < stride_words; i += JP_THREADS) {
        unsigned v = 0;
        const unsigned pad = 8u * nbytes - tot;          // 0 .. 7 one-bits behind bit tot - 1, in its byte: in the last word
        if (i == nwords - 1 && pad) v = __builtin_bswap32(((1u << pad) - 1u) << (32u - (tot & 31u) - pad));
        w[i] = v;
    }
}

// pack: a lane per block
__global__ void __launch_bounds__(JP_THREADS) jpeg_pack_kernel(const short* __restrict__ coefs, int nb, long long blocks, const unsigned* __restrict__ blkoff,
                                                               unsigned* __restrict__ words, unsigned stride_words) {
    __shared__ unsigned s_lut[JP_LUT_WORDS];
    jp_load_lut(s_lut);
    const long long g = (long long)blockIdx.x * JP_THREADS + threadIdx.x;
    if (g >= blocks) return;
    const long long interval = g / nb;
    const int j = (int)(g - interval * nb);
    const short* blk = coefs + (size_t)g * 64;
    JpPack pack(words + (size_t)interval * stride_words, blkoff[g]);
    jp_walk(blk, jp_pred(blk, j), j % 3 != 0, s_lut, pack);
    pack.finish();
}

// stuff: grid = intervals.  istuffed[interval] = bytes + the number of 0xFF among them
__global__ void __launch_bounds__(JP_THREADS) jpeg_stuff_kernel(const unsigned* __restrict__ words, unsigned stride_words, const unsigned* __restrict__ ibytes,
                                                                unsigned* __restrict__ istuffed) {
    __shared__ unsigned s_w[JP_THREADS / 64];
    const unsigned nbytes = ibytes[blockIdx.x];
    const unsigned* __restrict__ w = words + (size_t)blockIdx.x * stride_words;
    unsigned n = 0;
    for (unsigned i = threadIdx.x; 4u * i < nbytes; i += JP_THREADS) {
        const unsigned v = w[i];
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) n += (4u * i + k < nbytes) && ((v >> (8u * k)) & 0xFFu) == 0xFFu;
    }
    unsigned total;
    (void)jp_block_scan(n, s_w, total);
    if (threadIdx.x == 0) istuffed[blockIdx.x] = nbytes + total;
}

// layout: ONE workgroup.  An interval's share of the file: the header in front of a frame's first one, its stuffed bytes, RSTm or EOI.
// idst[interval] = where its scan bytes start; offsets[t] = where frame t starts; offsets[T] = the total
__global__ void __launch_bounds__(JP_THREADS) jpeg_layout_kernel(const unsigned* __restrict__ istuffed, long long intervals, int rows, int header_bytes,
                                                                 long long* __restrict__ idst, long long* __restrict__ offsets) {
    __shared__ long long s_w[JP_THREADS / 64];
    long long carry = 0;
    for (long long base = 0; base < intervals; base += JP_THREADS) {          // (uniform)
        const long long i = base + threadIdx.x;
        const bool live = i < intervals;
        const bool head = live && i % rows == 0;
        const long long share = live ? (long long)istuffed[i] + 2 + (head ? header_bytes : 0) : 0;
        long long total;
        const long long at = carry + jp_block_scan(share, s_w, total);
        if (live) idst[i] = at + (head ? header_bytes : 0);
        if (head) offsets[i / rows] = at;
        carry += total;
    }
    if (threadIdx.x == 0) offsets[intervals / rows] = carry;
}

// write: grid = intervals.  Every index is checked against out_bytes
__global__ void __launch_bounds__(JP_THREADS) jpeg_write_kernel(const unsigned* __restrict__ words, unsigned stride_words, const unsigned* __restrict__ ibytes,
                                                                const long long* __restrict__ idst, int rows, const unsigned char* __restrict__ header,
                                                                int header_bytes, unsigned char* __restrict__ out, long long out_bytes) {
    __shared__ unsigned s_w[JP_THREADS / 64];
    const int tid = threadIdx.x;
    const int r = (int)(blockIdx.x % (unsigned)rows);
    const unsigned nbytes = min(ibytes[blockIdx.x], 4u * stride_words);
    const long long dst = idst[blockIdx.x];
    const unsigned* __restrict__ w = words + (size_t)blockIdx.x * stride_words;
    if (r == 0)
        for (int k = tid; k < header_bytes; k += JP_THREADS) {
            const long long at = dst - header_bytes + k;
            if (at >= 0 && at < out_bytes) out[at] = header[k];
        }
    unsigned carry = 0;
    for (unsigned base = 0; 4u * base < nbytes; base += JP_THREADS) {          // (uniform)
        const unsigned i = base + tid;
        const unsigned v = 4u * i < nbytes ? w[i] : 0u;
        unsigned n = 0;
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) n += (4u * i + k < nbytes) && ((v >> (8u * k)) & 0xFFu) == 0xFFu;
        unsigned total;
        const unsigned excl = jp_block_scan(n, s_w, total);
        long long at = dst + 4ll * i + carry + excl;
#pragma unroll
        for (unsigned k = 0; k < 4; ++k) {
            if (4u * i + k >= nbytes) break;
            const unsigned char b = (unsigned char)(v >> (8u * k));
            if (at >= 0 && at < out_bytes) out[at] = b;
            ++at;
            if (b == 0xFF) {
                if (at >= 0 && at < out_bytes) out[at] = 0;
                ++at;
            }
        }
        carry += total;
    }
    if (tid == 0) {
        const long long at = dst + nbytes + carry;
        if (at >= 0 && at + 1 < out_bytes) {
            out[at] = 0xFF;
            out[at + 1] = r == rows - 1 ? 0xD9 : (unsigned char)(0xD0 + (r & 7));
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
struct JpLayout { long long blkoff, ibytes, istuffed, idst, words, total, blocks, intervals; unsigned stride_words; };

static inline long long jp_up16(long long v) { return (v + 15) / 16 * 16; }

// NULL when the geometry is fine, the refusal otherwise
static const char* jp_layout(int T, int rows, int mcus, JpLayout& L, int& code) {
    code = LP_ERR_ARG;
    if (T < 1 || rows < 1 || mcus < 1) return "T, rows and mcus must be >= 1";
    if (rows > (JP_MAX_DIM + 7) / 8 || mcus > (JP_MAX_DIM + 7) / 8) return "rows or mcus above 8192: a JPEG frame holds at most 65535 x 65535 pixels";
    code = LP_ERR_UNSUPPORTED;
    L.intervals = (long long)T * rows;
    if (L.intervals > 0x7fffffffLL) return "T x rows exceeds one launch grid";
    L.blocks = L.intervals * mcus * 3;
    L.stride_words = (unsigned)mcus * 3u * JP_BLOCK_WORDS;
    if (L.blocks > 0x7fffffffLL / (4 * JP_BLOCK_WORDS)) return "the scratch would exceed 2^31 - 1 bytes: encode fewer frames per call";
    L.blkoff = 0;
    L.ibytes = L.blkoff + jp_up16(L.blocks * 4);
    L.istuffed = L.ibytes + jp_up16(L.intervals * 4);
    L.idst = L.istuffed + jp_up16(L.intervals * 4);
    L.words = L.idst + jp_up16(L.intervals * 8);
    L.total = L.words + L.intervals * (long long)L.stride_words * 4;
    if (L.total > 0x7fffffffLL) return "the scratch would exceed 2^31 - 1 bytes: encode fewer frames per call";
    return nullptr;
}

static int jp_refuse(const char* who, int code, const char* why) {
    static thread_local char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return lp_set_error(code, msg);
}

extern "C" int lp_jpeg_code_table(unsigned int* table) {
    if (!table) return lp_set_error(LP_ERR_ARG, "lp_jpeg_code_table: null pointer");
    for (int i = 0; i < JP_LUT_WORDS; ++i) table[i] = jp_lut_host.e[i];
    return JP_LUT_WORDS;
}

extern "C" int lp_jpeg_transform(const unsigned char* frames, const long long* strides, int T, int H, int W, const unsigned char* qtables, short* coefs,
                                 void* stream) {
    const char* who = "lp_jpeg_transform";
    if (!frames || !strides || !qtables || !coefs) return jp_refuse(who, LP_ERR_ARG, "null pointer");
    if (T < 1 || H < 1 || W < 1) return jp_refuse(who, LP_ERR_ARG, "T >= 1, H >= 1 and W >= 1 are required");
    if (H > JP_MAX_DIM || W > JP_MAX_DIM) return jp_refuse(who, LP_ERR_ARG, "H and W must be <= 65535 (the frame header holds them in 16 bits)");
    JpQ qt;
    for (int i = 0; i < 128; ++i) {
        if (qtables[i] < 1) return jp_refuse(who, LP_ERR_ARG, "a quantisation table entry is 0: the tables hold 1 .. 255 (quality 1 .. 100)");
        qt.q[i] = qtables[i];
    }
    const int rows = (H + 7) / 8, mcus = (W + 7) / 8;
    JpLayout L;
    int code;
    if (const char* why = jp_layout(T, rows, mcus, L, code)) return jp_refuse(who, code, why);
    if (T > 65535) return jp_refuse(who, LP_ERR_UNSUPPORTED, "T exceeds one launch grid (at most 65535 frames)");
    const JpSrc s = {frames, strides[0], strides[1], strides[2], strides[3]};
    const dim3 grid((unsigned)((W + JP_TILE - 1) / JP_TILE), (unsigned)((H + JP_TILE - 1) / JP_TILE), (unsigned)T), block(JP_THREADS);
    hipLaunchKernelGGL(jpeg_transform_kernel, grid, block, 0, (hipStream_t)stream, s, qt, coefs, H, W, rows, mcus);
    return lp_check_launch("jpeg_transform");
}

extern "C" long long lp_jpeg_entropy_scratch_bytes(int T, int rows, int mcus) {
    JpLayout L;
    int code;
    if (const char* why = jp_layout(T, rows, mcus, L, code)) return jp_refuse("lp_jpeg_entropy_scratch_bytes", code, why);
    return L.total;
}

extern "C" int lp_jpeg_entropy_size(const short* coefs, int T, int rows, int mcus, int header_bytes, void* scratch, long long scratch_bytes,
                                    long long* offsets, void* stream) {
    const char* who = "lp_jpeg_entropy_size";
    if (!coefs || !scratch || !offsets) return jp_refuse(who, LP_ERR_ARG, "null pointer");
    if (((uintptr_t)coefs & 15) || ((uintptr_t)scratch & 15)) return jp_refuse(who, LP_ERR_ARG, "coefs and scratch must be 16-byte aligned");
    if (header_bytes < 0 || header_bytes > 65536) return jp_refuse(who, LP_ERR_ARG, "header_bytes outside 0 .. 65536");
    JpLayout L;
    int code;
    if (const char* why = jp_layout(T, rows, mcus, L, code)) return jp_refuse(who, code, why);
    if (scratch_bytes < L.total) return jp_refuse(who, LP_ERR_ARG, "scratch smaller than lp_jpeg_entropy_scratch_bytes()");
    char* base = (char*)scratch;
    unsigned* blkoff = (unsigned*)(base + L.blkoff);
    unsigned* ibytes = (unsigned*)(base + L.ibytes);
    unsigned* istuffed = (unsigned*)(base + L.istuffed);
    long long* idst = (long long*)(base + L.idst);
    unsigned* words = (unsigned*)(base + L.words);
    const int nb = mcus * 3;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_count_kernel, dim3((unsigned)L.intervals), dim3(JP_THREADS), 0, st, coefs, nb, blkoff, ibytes, words, L.stride_words);
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)((L.blocks + JP_THREADS - 1) / JP_THREADS)), dim3(JP_THREADS), 0, st, coefs, nb, L.blocks, blkoff,
                       words, L.stride_words);
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)L.intervals), dim3(JP_THREADS), 0, st, words, L.stride_words, ibytes, istuffed);
    hipLaunchKernelGGL(jpeg_layout_kernel, dim3(1), dim3(JP_THREADS), 0, st, istuffed, L.intervals, rows, header_bytes, idst, offsets);
    return lp_check_launch("jpeg_entropy_size");
}

extern "C" int lp_jpeg_entropy_write(const void* scratch, long long scratch_bytes, int T, int rows, int mcus, const unsigned char* header,
                                     int header_bytes, unsigned char* out, long long out_bytes, void* stream) {
    const char* who = "lp_jpeg_entropy_write";
    if (!scratch || !out || (!header && header_bytes)) return jp_refuse(who, LP_ERR_ARG, "null pointer");
    if ((uintptr_t)scratch & 15) return jp_refuse(who, LP_ERR_ARG, "scratch must be 16-byte aligned");
    if (header_bytes < 0 || header_bytes > 65536) return jp_refuse(who, LP_ERR_ARG, "header_bytes outside 0 .. 65536");
    if (out_bytes < 1) return jp_refuse(who, LP_ERR_ARG, "out_bytes must be the total lp_jpeg_entropy_size left in offsets[T]");
    JpLayout L;
    int code;
    if (const char* why = jp_layout(T, rows, mcus, L, code)) return jp_refuse(who, code, why);
    if (scratch_bytes < L.total) return jp_refuse(who, LP_ERR_ARG, "scratch smaller than lp_jpeg_entropy_scratch_bytes()");
    const char* base = (const char*)scratch;
    hipLaunchKernelGGL(jpeg_write_kernel, dim3((unsigned)L.intervals), dim3(JP_THREADS), 0, (hipStream_t)stream, (const unsigned*)(base + L.words),
                       L.stride_words, (const unsigned*)(base + L.ibytes), (const long long*)(base + L.idst), rows, header, header_bytes, out, out_bytes);
    return lp_check_launch("jpeg_entropy_write");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
