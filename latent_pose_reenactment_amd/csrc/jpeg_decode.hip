// Baseline JPEG decoder for the image-folder loader (--decode_jpeg_on_gpu): the entropy-coded segments of a batch's files, as utils/jpeg_parse.py
// cut them out on the host, -> uint8 RGB frames at their offsets in the packed buffer that lp_frames_prepare consumes.  Only the compressed bytes
// cross PCIe.
//
// Definition (restated in numpy integers by tests/jpeg_decode_restatement.py, and by hipops.jpeg_decode_host for CPU tensors).  Everything after
// the Huffman decode is INTEGER arithmetic, so the device, the host twin and the restatement agree bit for bit: no tolerance and no tie flags.
// A float IDCT is not used: a DC-only block reconstructs to DC q / 8 + 128, an exact half-integer for one DC value in eight, and a float IDCT
// would turn smooth backgrounds into rounding ties.
//
// Supported files (utils/jpeg_parse.parse returns None for anything else and the loader decodes that file with PIL): baseline sequential DCT
// (SOF0), 8-bit samples; 1 or 3 components in ONE interleaved scan (Ss = 0, Se = 63, Ah = Al = 0); 8-bit quantisation tables; at most 4 DC and 4
// AC Huffman tables, standard or optimised; any DRI; sampling grey, 4:4:4, 4:2:2 (luma 2 x 1, chroma 1 x 1), 4:2:0 (luma 2 x 2, chroma 1 x 1);
// H and W in 1 .. 65535; no Adobe APP14 segment with transform != 1, and not the component ids 'R', 'G', 'B' without a JFIF or Adobe marker
// (libjpeg takes those for RGB); fill bytes (0xFF 0xFF) before markers are legal.
//
// Geometry: hmax x vmax = the luma factors (1 x 1 for grey); an MCU covers 8 hmax x 8 vmax pixels, mcux = ceil(W / (8 hmax)), mcuy =
// ceil(H / (8 vmax)); an MCU holds hmax vmax luma blocks (rows first) and, in colour, one block each of Cb and Cr.  A segment is one restart
// interval (DRI MCUs, the last one of a frame what remains), or the whole scan without DRI; the host removes the byte stuffing and the markers,
// the device never sees one.
//
// Entropy decode, per segment, MSB first; bits behind the segment's last byte read as 0.  Canonical Huffman codes from the DHT counts (T.81 Annex
// C; decoding by F.2.2.3: the first length l in 1 .. 16 whose l leading bits are <= maxcode[l]).  Per block: the DC symbol s (0 .. 15) and s more
// bits v, diff = v < 2^(s - 1) ? v - 2^s + 1 : v (the receive / extend rule), DC = predictor + diff kept in 16 bits, the predictors of all
// components 0 at the start of a segment; then at most 63 AC steps from k = 1: symbol (r, s); s = 0: r = 15 (ZRL) moves k by 16, anything else
// (EOB) ends the block; s > 0: k += r, coefficient k = extend(s more bits), k += 1; the block ends when k reaches 64.  Output: int16
// coefs[block][64] in zigzag order, block = the frame's first block + MCU index x blocks per MCU + the block's place in its MCU (scan order); the
// decoder itself zeroes whatever an EOB leaves unset.  A stream that does not decode gives its FRAME a status, the largest over its segments:
// 1 = no code of <= 16 bits matches (or a DC symbol above 15), 2 = a run leaves the block (k + r > 63), 3 = the segment ends inside a code (more
// bits used than the segment holds, checked after every symbol and before its coefficient is stored); the segment stops there: what it decoded
// stays, every coefficient behind it in the segment is 0.  0 = ok.
//
// Dequantise: F = clamp(coef q, -32768, 32767), in natural order (q the component's table).
// IDCT: K[u][x] = rint(2^13 c(u) cos((2 x + 1) u pi / 16)), c(0) = sqrt(1 / 8), c(u > 0) = 1 / 2: 64 integers formed in fp64 on the host
// (utils/jpeg_parse.idct_table) and handed over.  With u the vertical frequency and x the row:
//      T[x][v] = (sum_u K[u][x] F[u][v] + 2^9) >> 10,      S[x][y] = (sum_v K[v][y] T[x][v] + 2^15) >> 16,      sample = clamp(S + 128, 0, 255)
// Shifts are arithmetic; the accumulators are 64-bit in the definition.  Pass 1 fits 32 bits: |F| <= 2^15 and sum_u |K[u][x]| <= 2897 + 7 x 4096
// = 31569 < 2^15, so |sum| + 2^9 < 2^30 + 2^9; then |T| <= 2^20 + 1 and pass 2 (up to 31569 x 2^20 > 2^31) is accumulated in 64 bits.
// The samples of a component form a plane over its whole block area (8 mcuy vmax rows x 8 mcux hmax columns for luma, 8 mcuy x 8 mcux for
// chroma): uint8, in the caller's workspace -- luma, Cb, Cr back to back at the frame's plane offset.
//
// Upsampling: libjpeg's "fancy" triangle filter in integers, on the component's n = ceil(W / hmax) columns and ceil(H / vmax) rows; the rest of
// the block area is not part of it.
//   h2v1 (4:2:2), per row:  out[2i] = (3 in[i] + in[i - 1] + 1) >> 2,  out[2i + 1] = (3 in[i] + in[i + 1] + 2) >> 2,  out[0] = in[0],
//                           out[2n - 1] = in[n - 1]
//   h2v2 (4:2:0): with nb the row above for an even output row and the row below for an odd one (replicated at the top and bottom edge),
//                 cs[j] = 3 in[i][j] + nb[j]:  out[2j] = (3 cs[j] + cs[j - 1] + 8) >> 4,  out[2j + 1] = (3 cs[j] + cs[j + 1] + 7) >> 4,
//                 out[0] = (4 cs[0] + 8) >> 4,  out[2n - 1] = (4 cs[n - 1] + 7) >> 4
// Colour, with cb, cr minus 128:  R = Y + ((91881 cr + 32768) >> 16),  G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
// B = Y + ((116130 cb + 32768) >> 16), clamped to 0 .. 255; grey: R = G = B = Y.  Output: uint8 [H][W][3], dense, at the frame's destination
// offset -- what np.array(Image.open(f).convert('RGB')) occupies there on the PIL route.
//
// Deviation from libjpeg: PIL's decoder (libjpeg-turbo's integer "islow" IDCT) rounds some samples one level differently than any other accurate
// IDCT, and the colour matrix scales that by up to 1.772: measured against PIL 12.2 at most 3 levels in colour and 1 in grey
// (tests/test_jpeg_decode_cpu.py).
//
// Launches.  lp_jpeg_decode_entropy: a clear of the status words and ONE launch.  The unit of parallel work is one segment, and a segment is one
// serial chain -- every code's position depends on the lengths of all codes before it -- so the kernel is latency-bound by construction: what
// counts is how many chains are in flight, not lanes kept busy.  A LANE decodes a segment.  The lanes of a wave share one instruction stream and
// would diverge at every symbol (code length, run, EOB), so a wave is given ONE segment while the device has wave slots to spare: with S segments
// a wave takes per = ceil(S / 2048) of them (clamped to 64), in its first `per` lanes; 2048 = 256 CUs x 4 SIMDs x 2 waves, a quarter of the
// slots, so that every SIMD has chains of two waves to interleave.  A batch of 72 files without DRI is 72 waves of one lane on 72 CUs; with one
// interval per MCU row (about 2000 segments) it is still one lane per wave; beyond that lanes fill up.  A wave is a workgroup of its own (64
// threads), so that segments spread over the CUs.  The tables are read from global memory (3 KiB per frame, shared by all of its segments:
// L2 hits); the bit window is a 64-bit register refilled by single byte loads, every one clamped to the segment's end.
// Measured on the MI355X (scripts/jpeg_decode_micro.py): 72 restart-free scans of 450 x 450 4:2:0 frames take 86.6 ms, about 1.15 us per symbol:
// every symbol waits for dependent global loads (scan byte, maxcode words, symbol byte) that a wave with one chain cannot hide.  Tables in LDS
// and a prefetched word-wide refill are the next step; they are not built.
// EVERY loop is bounded by header counts: MCUs per segment, blocks per MCU, at most 63 AC steps per block, at most 16 bits per code, at most 8
// bytes per refill.  A corrupt stream therefore ends with a status; it never reads outside its segment and never spins.
// lp_jpeg_decode_pixels: TWO launches.  idct: a workgroup of 256 lanes = 4 blocks x 64 samples; dequantised block, K and the pass-1 result in
// LDS; the sample planes leave as bytes.  colour: a lane per output pixel, 32 x 8 pixels per workgroup; reads the planes (the chroma taps of the
// triangle filter straight from the plane: L1 / L2 hits) and stores the three bytes.  The planes take a round trip through the workspace (1.5
// to 3 bytes per pixel each way) -- that keeps the upsampling's neighbours across block borders simple; the launches are not fused.
// No atomics in the pixel launches, no floating point anywhere, bit-identical from run to run and independent of the other frames of the call;
// the one atomic is the entropy launch's integer atomicMax on the frame's status word (order-independent).  Nothing allocates or synchronises:
// capturable.  Everything is refused before any device work (LP_ERR_ARG / LP_ERR_UNSUPPORTED), naming the frame or segment -- two frames whose
// coefficient, plane or destination ranges overlap included: the independence of the frames rests on disjoint ranges.
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

#define JD_FRAME_COLS 24
#define JD_SEG_COLS 4
#define JD_HUFF_WORDS 96          // maxcode[16], delta[16], 256 symbol bytes
#define JD_MAX_DIM 65535
#define JD_WAVES 2048             // waves with one segment each before lanes fill up (header comment)
#define JD_THREADS 256

// the columns of a frame row (utils/jpeg_parse.FRAME_COLUMNS)
enum { JD_H, JD_W, JD_NC, JD_HMAX, JD_VMAX, JD_MCUX, JD_MCUY, JD_RI, JD_COEF, JD_PLANE, JD_DST, JD_SEG0, JD_NSEG, JD_TQ, JD_TD = JD_TQ + 3, JD_TA = JD_TD + 3 };

struct JdIdct { int k[64]; };

// T.81 Figure A.6: natural index -> zigzag position
struct JdZigzag { unsigned char pos[64]; };
constexpr JdZigzag jd_make_zigzag() {
    const unsigned char order[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    JdZigzag z = {};
    for (int i = 0; i < 64; ++i) z.pos[order[i]] = (unsigned char)i;
    return z;
}
__constant__ JdZigzag jd_zigzag = jd_make_zigzag();

// ---- entropy ---------------------------------------------------------------------------------------------------------------------------------------
// MSB-first window over the bytes [pos, end) of the scan: `cnt` valid bits at the top of `acc`; bytes behind `end` read as 0
struct JdBits {
    const unsigned char* __restrict__ p;
    long long pos, end;
    unsigned long long acc;
    int cnt;
    long long used;          // bits consumed
    __device__ __forceinline__ void refill() {          // afterwards cnt >= 57: a code (<= 16) and its extra bits (<= 15) fit
#pragma unroll 1
        for (int i = 0; i < 8 && cnt <= 56; ++i) {
            const unsigned long long b = pos < end ? p[pos] : 0u;
            ++pos;
            acc |= b << (56 - cnt);
            cnt += 8;
        }
    }
    __device__ __forceinline__ unsigned peek16() const { return (unsigned)(acc >> 48); }
    __device__ __forceinline__ void skip(int n) { acc <<= n; cnt -= n; used += n; }
    __device__ __forceinline__ int take(int n) {          // n in 1 .. 15
        const int v = (int)(acc >> (64 - n));
        skip(n);
        return v;
    }
};

// -> the symbol, or -1 when no code of <= 16 bits matches
__device__ __forceinline__ int jd_symbol(JdBits& b, const int* __restrict__ tab) {
    const unsigned w = b.peek16();
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int code = (int)(w >> (15 - l));
        if (code <= tab[l]) {
            const int at = min(max(code + tab[16 + l], 0), 255);
            b.skip(l + 1);
            return (int)((const unsigned char*)(tab + 32))[at];
        }
    }
    return -1;
}

__device__ __forceinline__ int jd_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

__global__ void __launch_bounds__(64) jpeg_decode_entropy_kernel(const unsigned char* __restrict__ scan, const long long* __restrict__ seg,
                                                                 const long long* __restrict__ frm, const int* __restrict__ huff,
                                                                 short* __restrict__ coefs, int* __restrict__ status, int nseg, int per) {
    if ((int)threadIdx.x >= per) return;
    const long long s = (long long)blockIdx.x * per + threadIdx.x;
    if (s >= nseg) return;
    const long long f = seg[s * JD_SEG_COLS];
    const long long* __restrict__ fr = frm + f * JD_FRAME_COLS;
    const int nc = (int)fr[JD_NC], nluma = nc == 3 ? (int)(fr[JD_HMAX] * fr[JD_VMAX]) : 1, bpm = nc == 3 ? nluma + 2 : 1;
    const long long total = fr[JD_MCUX] * fr[JD_MCUY], ri = fr[JD_RI];
    const long long first = (s - fr[JD_SEG0]) * ri;
    const long long n = ri ? min(ri, total - first) : total;
    const int* __restrict__ tabs = huff + f * 8 * JD_HUFF_WORDS;
    JdBits b = {scan, seg[s * JD_SEG_COLS + 1], seg[s * JD_SEG_COLS + 2], 0ull, 0, 0};
    const long long nbits = 8 * (b.end - b.pos);
    short* __restrict__ blk = coefs + (fr[JD_COEF] + first * bpm) * 64;
    int pred0 = 0, pred1 = 0, pred2 = 0, st = 0;
#pragma unroll 1
    for (long long m = 0; m < n; ++m) {
#pragma unroll 1
        for (int j = 0; j < bpm; ++j, blk += 64) {
            const uint4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) ((uint4*)blk)[i] = zero;
            if (st) continue;
            const int c = j < nluma ? 0 : j - nluma + 1;
            const int* __restrict__ dc = tabs + (int)fr[JD_TD + c] * JD_HUFF_WORDS;
            const int* __restrict__ ac = tabs + (4 + (int)fr[JD_TA + c]) * JD_HUFF_WORDS;
            b.refill();
            const int sd = jd_symbol(b, dc);
            if (sd < 0 || sd > 15) { st = 1; continue; }
            const int diff = sd ? jd_extend(b.take(sd), sd) : 0;
            if (b.used > nbits) { st = 3; continue; }
            const int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
            const int v = (int)(short)(pred + diff);
            if (c == 0) pred0 = v; else if (c == 1) pred1 = v; else pred2 = v;
            blk[0] = (short)v;
            int k = 1;
#pragma unroll 1
            for (int step = 0; step < 63 && k < 64; ++step) {
                b.refill();
                const int rs = jd_symbol(b, ac);
                if (rs < 0) { st = 1; break; }
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                    if (b.used > nbits) { st = 3; break; }
                    if (r != 15) break;
                    k += 16;
                    continue;
                }
                k += r;
                if (k > 63) { st = 2; break; }
                const int a = jd_extend(b.take(sz), sz);
                if (b.used > nbits) { st = 3; break; }
                blk[k] = (short)a;
                ++k;
            }
        }
    }
    if (st) atomicMax(status + f, st);
}

// ---- pixels ----------------------------------------------------------------------------------------------------------------------------------------
// idct: grid = (ceil(max blocks of a frame / 4), frames); lanes 64 b .. 64 b + 63 of a workgroup = block 4 blockIdx.x + b of frame blockIdx.y
__global__ void __launch_bounds__(JD_THREADS) jpeg_decode_idct_kernel(const short* __restrict__ coefs, const long long* __restrict__ frm,
                                                                      const unsigned char* __restrict__ qt, JdIdct K, unsigned char* __restrict__ planes) {
    __shared__ int s_k[64];
    __shared__ int s_f[4][64];
    __shared__ int s_t[4][64];
    const int tid = threadIdx.x, sub = tid >> 6, l = tid & 63;
    const long long f = blockIdx.y;
    const long long* __restrict__ fr = frm + f * JD_FRAME_COLS;
    const int nc = (int)fr[JD_NC], hmax = (int)fr[JD_HMAX], vmax = (int)fr[JD_VMAX], mcux = (int)fr[JD_MCUX], mcuy = (int)fr[JD_MCUY];
    const int nluma = nc == 3 ? hmax * vmax : 1, bpm = nc == 3 ? nluma + 2 : 1;
    const long long blocks = (long long)mcux * mcuy * bpm, bi = 4ll * blockIdx.x + sub;
    const bool live = bi < blocks;
    if (tid < 64) s_k[tid] = K.k[tid];
    long long mcu = 0;
    int j = 0, c = 0;
    if (live) {
        mcu = bi / bpm;
        j = (int)(bi - mcu * bpm);
        c = j < nluma ? 0 : j - nluma + 1;
        const int q = (int)qt[(f * 4 + fr[JD_TQ + c]) * 64 + l];
        const int v = (int)coefs[(fr[JD_COEF] + bi) * 64 + jd_zigzag.pos[l]] * q;
        s_f[sub][l] = min(max(v, -32768), 32767);
    }
    __syncthreads();
    const int x = l >> 3, y = l & 7;
    if (live) {
        int acc = 1 << 9;          // (32 bits: the header comment shows the range)
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += s_k[u * 8 + x] * s_f[sub][u * 8 + y];
        s_t[sub][l] = acc >> 10;
    }
    __syncthreads();
    if (!live) return;
    long long acc = 1ll << 15;
#pragma unroll
    for (int v = 0; v < 8; ++v) acc += (long long)s_k[v * 8 + y] * (long long)s_t[sub][x * 8 + v];
    const long long smp = (acc >> 16) + 128;
    const int my = (int)(mcu / mcux), mx = (int)(mcu - (long long)my * mcux);
    const long long pw0 = 8ll * mcux * hmax, ph0 = 8ll * mcuy * vmax, pwc = 8ll * mcux, phc = 8ll * mcuy;
    long long base, pw;
    int by, bx;
    if (c == 0) {
        base = fr[JD_PLANE]; pw = pw0;
        by = my * (nc == 3 ? vmax : 1) + (nc == 3 ? j / hmax : 0);
        bx = mx * (nc == 3 ? hmax : 1) + (nc == 3 ? j % hmax : 0);
    } else {
        base = fr[JD_PLANE] + pw0 * ph0 + (c - 1) * pwc * phc; pw = pwc;
        by = my; bx = mx;
    }
    planes[base + (8ll * by + x) * pw + 8ll * bx + y] = (unsigned char)min(max(smp, 0ll), 255ll);
}

// one chroma sample at output pixel (x, y): p = the plane, stride its row length, n x rows its samples (header comment: upsampling)
__device__ __forceinline__ int jd_chroma(const unsigned char* __restrict__ p, long long stride, int n, int rows, int x, int y, int hmax, int vmax) {
    if (hmax == 1) return (int)p[y * stride + x];
    const int j = x >> 1;
    if (vmax == 1) {
        const unsigned char* __restrict__ row = p + y * stride;
        const int in = (int)row[j];
        if (x & 1) return j == n - 1 ? in : (3 * in + (int)row[j + 1] + 2) >> 2;
        return j == 0 ? in : (3 * in + (int)row[j - 1] + 1) >> 2;
    }
    const int i = y >> 1;
    const unsigned char* __restrict__ r0 = p + i * stride;
    const unsigned char* __restrict__ r1 = p + ((y & 1) ? min(i + 1, rows - 1) : max(i - 1, 0)) * stride;
    const int cs = 3 * (int)r0[j] + (int)r1[j];
    if (x & 1) return j == n - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * (int)r0[j + 1] + (int)r1[j + 1] + 7) >> 4;
    return j == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * (int)r0[j - 1] + (int)r1[j - 1] + 8) >> 4;
}

// colour: grid = (ceil(max W / 32), ceil(max H / 8), frames), a lane per pixel
__global__ void __launch_bounds__(JD_THREADS) jpeg_decode_colour_kernel(const long long* __restrict__ frm, const unsigned char* __restrict__ planes,
                                                                        unsigned char* __restrict__ out) {
    const long long* __restrict__ fr = frm + (long long)blockIdx.z * JD_FRAME_COLS;
    const int H = (int)fr[JD_H], W = (int)fr[JD_W];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const int nc = (int)fr[JD_NC], hmax = (int)fr[JD_HMAX], vmax = (int)fr[JD_VMAX];
    const long long pw0 = 8ll * fr[JD_MCUX] * (nc == 3 ? hmax : 1), ph0 = 8ll * fr[JD_MCUY] * (nc == 3 ? vmax : 1);
    const unsigned char* __restrict__ p = planes + fr[JD_PLANE];
    const int Y = (int)p[y * pw0 + x];
    int R = Y, G = Y, B = Y;
    if (nc == 3) {
        const long long pwc = 8ll * fr[JD_MCUX], phc = 8ll * fr[JD_MCUY];
        const int n = (W + hmax - 1) / hmax, rows = (H + vmax - 1) / vmax;
        const int cb = jd_chroma(p + pw0 * ph0, pwc, n, rows, x, y, hmax, vmax) - 128;
        const int cr = jd_chroma(p + pw0 * ph0 + pwc * phc, pwc, n, rows, x, y, hmax, vmax) - 128;
        R = min(max(Y + ((91881 * cr + 32768) >> 16), 0), 255);
        G = min(max(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0), 255);
        B = min(max(Y + ((116130 * cb + 32768) >> 16), 0), 255);
    }
    unsigned char* __restrict__ o = out + fr[JD_DST] + ((long long)y * W + x) * 3;
    o[0] = (unsigned char)R;
    o[1] = (unsigned char)G;
    o[2] = (unsigned char)B;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
struct JdTotals { long long max_blocks, max_h, max_w, segments; };

struct JdRange { long long first, end; int frame; };

// 0 when no two ranges share an element; else the refusal naming the two frames.  The kernels write every frame's blocks, planes and pixels
// without looking at the other frames, so "independent of the other frames of the call" holds only for disjoint ranges
static int jd_disjoint(const char* who, const char* what, std::vector<JdRange>& r) {
    static thread_local char msg[320];
    std::sort(r.begin(), r.end(), [](const JdRange& a, const JdRange& b) { return a.first < b.first; });
    for (size_t i = 1; i < r.size(); ++i)
        if (r[i].first < r[i - 1].end) {
            snprintf(msg, sizeof msg, "%s: frames %d and %d overlap in the %s (%lld .. %lld and %lld .. %lld)", who, r[i - 1].frame, r[i].frame, what,
                     r[i - 1].first, r[i - 1].end, r[i].first, r[i].end);
            return lp_set_error(LP_ERR_ARG, msg);
        }
    return 0;
}

// the frame rows: 0 when every frame is one the kernels cover and lies inside the buffers given (a size < 0: that buffer is not part of the call)
static int jd_check_frames(const char* who, const long long* frm, int frames, long long coef_blocks, long long plane_bytes, long long out_bytes,
                           JdTotals& t) {
    static thread_local char msg[320];
    t = {0, 0, 0, 0};
    std::vector<JdRange> in_coefs, in_planes, in_out, in_segs;
    if (frames < 1) {
        snprintf(msg, sizeof msg, "%s: frames must be >= 1, got %d", who, frames);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    if (frames > 65535) {
        snprintf(msg, sizeof msg, "%s: %d frames exceed one launch grid (at most 65535 per call)", who, frames);
        return lp_set_error(LP_ERR_UNSUPPORTED, msg);
    }
    for (int f = 0; f < frames; ++f) {
        const long long* r = frm + (long long)f * JD_FRAME_COLS;
        const long long H = r[JD_H], W = r[JD_W], nc = r[JD_NC], hmax = r[JD_HMAX], vmax = r[JD_VMAX];
        if (H < 1 || W < 1 || H > JD_MAX_DIM || W > JD_MAX_DIM) {
            snprintf(msg, sizeof msg, "%s: frame %d: H and W must be in 1 .. 65535, got %lld x %lld", who, f, H, W);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        const bool grey = nc == 1 && hmax == 1 && vmax == 1;
        const bool colour = nc == 3 && ((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2));
        if (!grey && !colour) {
            snprintf(msg, sizeof msg, "%s: frame %d: %lld components with luma sampling %lld x %lld is not grey, 4:4:4, 4:2:2 or 4:2:0", who, f, nc, hmax, vmax);
            return lp_set_error(LP_ERR_UNSUPPORTED, msg);
        }
        if (r[JD_MCUX] != (W + 8 * hmax - 1) / (8 * hmax) || r[JD_MCUY] != (H + 8 * vmax - 1) / (8 * vmax)) {
            snprintf(msg, sizeof msg, "%s: frame %d: %lld x %lld MCUs are not those of a %lld x %lld frame", who, f, r[JD_MCUY], r[JD_MCUX], H, W);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        const long long mcus = r[JD_MCUX] * r[JD_MCUY], bpm = nc == 3 ? hmax * vmax + 2 : 1, blocks = mcus * bpm, ri = r[JD_RI];
        if (ri < 0 || ri > 65535 || r[JD_NSEG] != (ri ? (mcus + ri - 1) / ri : 1) || r[JD_SEG0] < 0) {
            snprintf(msg, sizeof msg, "%s: frame %d: %lld segments from %lld on do not cover %lld MCUs at a restart interval of %lld", who, f,
                     r[JD_NSEG], r[JD_SEG0], mcus, ri);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        for (int c = 0; c < 3; ++c)
            if (r[JD_TQ + c] < 0 || r[JD_TQ + c] > 3 || r[JD_TD + c] < 0 || r[JD_TD + c] > 3 || r[JD_TA + c] < 0 || r[JD_TA + c] > 3) {
                snprintf(msg, sizeof msg, "%s: frame %d: component %d names a table outside 0 .. 3", who, f, c);
                return lp_set_error(LP_ERR_ARG, msg);
            }
        if (r[JD_COEF] < 0 || r[JD_COEF] + blocks > coef_blocks) {
            snprintf(msg, sizeof msg, "%s: frame %d: its %lld blocks from %lld on lie outside the coefficient buffer of %lld blocks", who, f, blocks,
                     r[JD_COEF], coef_blocks);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        const long long pbytes = 64 * mcus * (nc == 3 ? hmax * vmax + 2 : 1);
        if (plane_bytes >= 0 && (r[JD_PLANE] < 0 || r[JD_PLANE] + pbytes > plane_bytes)) {
            snprintf(msg, sizeof msg, "%s: frame %d: its sample planes (%lld bytes at %lld) lie outside the workspace of %lld bytes", who, f, pbytes,
                     r[JD_PLANE], plane_bytes);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        if (out_bytes >= 0 && (r[JD_DST] < 0 || r[JD_DST] + H * W * 3 > out_bytes)) {
            snprintf(msg, sizeof msg, "%s: frame %d: the destination (%lld bytes at %lld) lies outside the buffer of %lld bytes", who, f, H * W * 3,
                     r[JD_DST], out_bytes);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        in_coefs.push_back({r[JD_COEF], r[JD_COEF] + blocks, f});
        in_segs.push_back({r[JD_SEG0], r[JD_SEG0] + r[JD_NSEG], f});
        if (plane_bytes >= 0) in_planes.push_back({r[JD_PLANE], r[JD_PLANE] + pbytes, f});
        if (out_bytes >= 0) in_out.push_back({r[JD_DST], r[JD_DST] + H * W * 3, f});
        t.max_blocks = blocks > t.max_blocks ? blocks : t.max_blocks;
        t.max_h = H > t.max_h ? H : t.max_h;
        t.max_w = W > t.max_w ? W : t.max_w;
        t.segments += r[JD_NSEG];
    }
    if (int rc = jd_disjoint(who, "coefficient buffer", in_coefs)) return rc;
    if (int rc = jd_disjoint(who, "segment table", in_segs)) return rc;
    if (int rc = jd_disjoint(who, "plane workspace", in_planes)) return rc;
    return jd_disjoint(who, "destination buffer", in_out);
}

extern "C" int lp_jpeg_decode_entropy(const unsigned char* scan, long long scan_bytes, const long long* seg_host, const long long* seg_dev, int segments,
                                      const long long* frames_host, const long long* frames_dev, int frames, const int* huffman, short* coefs,
                                      long long coef_blocks, int* status, void* stream) {
    const char* who = "lp_jpeg_decode_entropy";
    static thread_local char msg[320];
    if (!scan || !seg_host || !seg_dev || !frames_host || !frames_dev || !huffman || !coefs || !status) {
        snprintf(msg, sizeof msg, "%s: null pointer", who);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    if ((uintptr_t)coefs & 15) {
        snprintf(msg, sizeof msg, "%s: coefs must be 16-byte aligned", who);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    if (segments < 1 || scan_bytes < 0 || coef_blocks < 1) {
        snprintf(msg, sizeof msg, "%s: segments >= 1, scan_bytes >= 0 and coef_blocks >= 1 are required", who);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    JdTotals t;
    if (int rc = jd_check_frames(who, frames_host, frames, coef_blocks, -1, -1, t)) return rc;
    if (t.segments != segments) {
        snprintf(msg, sizeof msg, "%s: the frames hold %lld segments, the call gives %d", who, t.segments, segments);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    for (int s = 0; s < segments; ++s) {
        const long long* r = seg_host + (long long)s * JD_SEG_COLS;
        const long long f = r[0];
        if (f < 0 || f >= frames || s < frames_host[f * JD_FRAME_COLS + JD_SEG0] ||
            s >= frames_host[f * JD_FRAME_COLS + JD_SEG0] + frames_host[f * JD_FRAME_COLS + JD_NSEG]) {
            snprintf(msg, sizeof msg, "%s: segment %d is not one of the segments of its frame %lld", who, s, f);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        if (r[1] < 0 || r[1] > r[2] || r[2] > scan_bytes) {
            snprintf(msg, sizeof msg, "%s: segment %d (bytes %lld .. %lld) lies outside the scan buffer of %lld bytes", who, s, r[1], r[2], scan_bytes);
            return lp_set_error(LP_ERR_ARG, msg);
        }
    }
    const int per = (int)((segments + JD_WAVES - 1) / JD_WAVES) > 64 ? 64 : (segments + JD_WAVES - 1) / JD_WAVES;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, (size_t)frames * sizeof(int), st) != hipSuccess) return lp_set_error(LP_ERR_HIP, "lp_jpeg_decode_entropy: clearing the status failed");
    hipLaunchKernelGGL(jpeg_decode_entropy_kernel, dim3((unsigned)((segments + per - 1) / per)), dim3(64), 0, st, scan, seg_dev, frames_dev, huffman, coefs,
                       status, segments, per);
    return lp_check_launch("jpeg_decode_entropy");
}

extern "C" int lp_jpeg_decode_pixels(const short* coefs, long long coef_blocks, const long long* frames_host, const long long* frames_dev, int frames,
                                     const unsigned char* qtables, const int* idct_host, unsigned char* planes, long long plane_bytes,
                                     unsigned char* out, long long out_bytes, void* stream) {
    const char* who = "lp_jpeg_decode_pixels";
    static thread_local char msg[320];
    if (!coefs || !frames_host || !frames_dev || !qtables || !idct_host || !planes || !out) {
        snprintf(msg, sizeof msg, "%s: null pointer", who);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    if (coef_blocks < 1 || plane_bytes < 1 || out_bytes < 1) {
        snprintf(msg, sizeof msg, "%s: coef_blocks, plane_bytes and out_bytes must be >= 1", who);
        return lp_set_error(LP_ERR_ARG, msg);
    }
    JdTotals t;
    if (int rc = jd_check_frames(who, frames_host, frames, coef_blocks, plane_bytes, out_bytes, t)) return rc;
    JdIdct K;
    for (int i = 0; i < 64; ++i) {
        if (idct_host[i] < -4096 || idct_host[i] > 4096) {
            snprintf(msg, sizeof msg, "%s: IDCT table entry %d is %d, outside -4096 .. 4096 (2^13 c(u) cos(.))", who, i, idct_host[i]);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        K.k[i] = idct_host[i];
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_decode_idct_kernel, dim3((unsigned)((t.max_blocks + 3) / 4), (unsigned)frames), dim3(JD_THREADS), 0, st, coefs, frames_dev,
                       qtables, K, planes);
    hipLaunchKernelGGL(jpeg_decode_colour_kernel, dim3((unsigned)((t.max_w + 31) / 32), (unsigned)((t.max_h + 7) / 8), (unsigned)frames), dim3(JD_THREADS),
                       0, st, frames_dev, planes, out);
    return lp_check_launch("jpeg_decode_pixels");
}
