// The padded bands of out-of-frame crops: where a bounding box leaves its view, the reference's crop_with_padding
// (dataloaders/voxceleb2_segmentation_nolandmarks.py:283-367) does not use the border fill as it is: it blurs the padded band, and a strip one third
// of the band's width inside it, with a Gaussian of sigma = 0.016 n, and fades the band to the image's median colour (to 0 for a mask).  This file
// makes those crops on the device, as dense uint8 images in a workspace behind the packed frames; csrc/frames.hip then resamples them as plain
// in-view boxes of a rewritten table (frames.pad_plan), unchanged.
//
// Definition (restated in fp64 by tests/frames_pad_restatement.py, in fp32 torch ops by frames.pad_host).  cv2 is on none of the project's machines:
// THIS TEXT DECIDES.  It covers one view of one table row of frames.COLUMNS: an image (C = 3) or a mask (C = 1) whose box leaves the view:
//   pt = max(0, -t), pl = max(0, -l), pb = max(0, b - H), pr = max(0, r - W), at least one of them > 0.  All values are raw units 0 .. 255.
// Crop.  crop(j, i), 0 <= j, i < n, is the n x n crop through the border rule of csrc/frames.hip: an image is reflected without repeating the edge
//   (reflect-101, any number of periods, a 1-pixel axis maps to 0); a mask is 0 above the view and clamped elsewhere.  These are uint8 values: the
//   uint8 crop between the border fill and the blur is the only rounding of the reference's that is reproduced.
// Blur.  k = ((96 n + 1500) / 1000 in integer division) | 1 -- cv2's cvRound(6 sigma + 1) | 1 for uint8 with sigma = 0.016 n; cvRound meets no tie
//   for any integer n (96 n + 1000 = 1000 m + 500 would need 24 n = 250 m - 125, even = odd), so the integer form is exact.  R = (k - 1) / 2;
//   g[a] = exp(-a^2 / 2 sigma^2) / sum, -R <= a <= R, formed on the host in fp64 and handed over as fp32;
//   blur(j, i) = sum_a sum_b g[a] g[b] crop(rho(j + a), rho(i + b)), rho = reflect-101 on the CROP (0 .. n - 1; n = 1 maps to 0): cv2.GaussianBlur's
//   default border on the padded image.  The horizontal pass runs first, then the vertical; each adds its taps up in order from -R in fp32 (fused or
//   unfused multiply-adds).
// Weights.  mh = 1 - min(i / pl, (n - 1 - i) / pr), mv = 1 - min(j / pt, (n - 1 - j) / pb), a term whose pad is 0 being +inf; m = max(mh, mv);
//   a = clip(3 m + 1, 0, 1); f = clip(m, 0, 1) for an image, f = clip(mh, 0, 1) for a mask -- the reference fades a mask by its horizontal term
//   alone (:356), and that quirk is kept.  The divisions are fp32 divisions of exact integers; 3 m + 1 is one fp32 product and one fp32 sum.
// Blend, then fade.  x = crop + (blur - crop) a;  y = x + (fade - x) f, each one fp32 difference, product and sum; a weight of exactly 0 returns the
//   first operand and a weight of exactly 1 the second operand, exactly.  fade = 0 for a mask; for an image fade[c] is the median of the n^2 crop
//   values of channel c, (v[(N - 1) / 2] + v[N / 2]) / 2 over the sorted values, N = n^2: an integer or a half-integer.
// Round.  clamp(rint(y), 0, 255) as uint8, half to even (the reference rounds here too, :356-359).
//
// Deviations from the reference, on purpose: the median is taken over the crop BEFORE the blur (the reference takes it after the first blend, on
// floats; the two differ only by what the blur moves inside the bands); the blur is fp32 where cv2 runs its fixed-point uint8 kernel.
//
// Launches (lp_frames_pad; a plan row per affected view, frames.PLAN_COLUMNS): the histogram words are cleared, then
//   1. histogram: one workgroup per 8 crop rows of an image plan counts the crop's values per channel through the border rule -- LDS atomics on one
//      histogram per wave, then one integer global atomic per non-empty bin.  Integer counts do not depend on the order of the adds.
//   2. median: one workgroup per image plan scans its 3 x 256 counts and writes the three medians.
//   3. main: one workgroup per 16 x 16 tile of a crop.  A tile where a and f are 0 everywhere is a copy through the border rule and never stages a
//      halo (from the pads alone: the whole interior beyond 4/3 of each band): tiles at least twice each pad from the crop's edges are recognised
//      from integers and copied four at a time; any other tile forms a for its 16 columns and 16 rows in fp32 (32 lanes) and copies if none is
//      positive.  A tile that blurs stages the halo rows and columns its blurred rows and columns need -- at most (16 + 2 R)^2, all channels, as
//      uint8 in LDS, through rho and then the border rule; a wave reads consecutive bytes of one source row -- and runs the two passes one channel
//      at a time through an fp32 intermediate of (16 + 2 R) x 16.  At the supported n <= 1024 (k <= 99, R <= 49) that is 3 x 114^2 + 114 x 64
//      bytes plus the taps, the index rows and the finished tile: 48.5 KB, within the 64 KB csrc/frames.hip keeps to.
// Every source index goes through the border rule before it is used, every view is checked against the packed head and every workspace image
// against the tail of the buffer before any device work, so no plan row can make a kernel read or write outside buf, or write into the frames.
// The result of a plan row is a pure function of that row: bit-identical from run to run and independent of the other rows.
#include <stdio.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file, as in its neighbours (frames.hip, augment.hip, image_quality.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define FP_TILE 16
#define FP_THREADS 256
#define FP_COLS 16              // frames.PLAN_COLUMNS
#define FP_MAX_N 1024
#define FP_MAX_K 99
#define FP_WROW 100             // floats per weight row: g[-R .. R] first, zeros behind
#define FP_HIST_ROWS 8
#define FP_BATCH 8              // halo rows a lane loads before it stores them to LDS
#define FP_GROUP 4              // tiles along x that one workgroup copies where none of them needs the blur
#define FP_MAX_COORD (1LL << 30)
enum { FP_ROW, FP_VIEW, FP_OFF, FP_H, FP_W, FP_RS, FP_PS, FP_T, FP_L, FP_N, FP_PT, FP_PL, FP_PB, FP_PR, FP_K, FP_WS };

struct FpArgs {
    unsigned char* buf;
    const long long* plan;
    const float* weights;       // [plans][FP_WROW]
    unsigned int* hist;         // [plans][3][256]
    float* median;              // [plans][3]
};

__device__ __forceinline__ int fp_reflect101(int i, int n) {
    if ((unsigned int)i < (unsigned int)n) return i;          // inside: the common case, without the division
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

struct FpView {
    const unsigned char* base;  // buf + off
    long long rs, ps;
    int H, W, t, l, n;
};

__device__ __forceinline__ FpView fp_view(const unsigned char* buf, const long long* __restrict__ p) {
    FpView v;
    v.base = buf + p[FP_OFF]; v.rs = p[FP_RS]; v.ps = p[FP_PS];
    v.H = (int)p[FP_H]; v.W = (int)p[FP_W]; v.t = (int)p[FP_T]; v.l = (int)p[FP_L]; v.n = (int)p[FP_N];
    return v;
}

// crop(j, i) of channel c, 0 <= j, i < n: the border rule of csrc/frames.hip
template <bool MASK> __device__ __forceinline__ unsigned char fp_crop(const FpView& v, int j, int i, int c) {
    const int sy = v.t + j, sx = v.l + i;
    if (MASK) {
        if (sy < 0) return 0;
        return v.base[(long long)min(sy, v.H - 1) * v.rs + (long long)min(max(sx, 0), v.W - 1) * v.ps];
    }
    return v.base[(long long)fp_reflect101(sy, v.H) * v.rs + (long long)fp_reflect101(sx, v.W) * v.ps + c];
}

// 1 - min(i / p0, (n - 1 - i) / p1), a term whose pad is 0 being +inf
__device__ __forceinline__ float fp_side(int i, int n, int p0, int p1) {
    const float u = p0 > 0 ? (float)i / (float)p0 : INFINITY, w = p1 > 0 ? (float)(n - 1 - i) / (float)p1 : INFINITY;
    return __fsub_rn(1.f, fminf(u, w));
}

__device__ __forceinline__ float fp_clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// x + (y - x) w without contraction; w == 0 gives x, w == 1 gives y
__device__ __forceinline__ float fp_blend(float x, float y, float w) {
    if (w <= 0.f) return x;
    if (w >= 1.f) return y;
    return __fadd_rn(x, __fmul_rn(__fsub_rn(y, x), w));
}

__global__ void __launch_bounds__(FP_THREADS) frames_pad_hist_kernel(FpArgs a) {
    __shared__ unsigned int h[FP_THREADS / 64][3][256];
    const long long* __restrict__ p = a.plan + (size_t)blockIdx.y * FP_COLS;
    const FpView v = fp_view(a.buf, p);
    const int j0 = blockIdx.x * FP_HIST_ROWS;
    if (p[FP_VIEW] != 0 || j0 >= v.n) return;          // (uniform over the workgroup)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < (FP_THREADS / 64) * 3 * 256; e += FP_THREADS) (&h[0][0][0])[e] = 0u;
    __syncthreads();
    const int j1 = min(j0 + FP_HIST_ROWS, v.n);
    for (int e = lane; e < v.n * 3; e += 64) {          // a wave takes a row, its lanes consecutive bytes of it
        const int i = e / 3, c = e - i * 3;
        const unsigned char* __restrict__ col = v.base + (long long)fp_reflect101(v.l + i, v.W) * v.ps + c;
        unsigned char val[FP_HIST_ROWS / (FP_THREADS / 64)];          // the loads of the band's rows in flight before the first LDS atomic
#pragma unroll
        for (int u = 0; u < FP_HIST_ROWS / (FP_THREADS / 64); ++u) {
            const int j = j0 + wave + u * (FP_THREADS / 64);
            val[u] = j < j1 ? col[(long long)fp_reflect101(v.t + j, v.H) * v.rs] : (unsigned char)0;
        }
#pragma unroll
        for (int u = 0; u < FP_HIST_ROWS / (FP_THREADS / 64); ++u)
            if (j0 + wave + u * (FP_THREADS / 64) < j1) atomicAdd(&h[wave][c][val[u]], 1u);
    }
    __syncthreads();
    for (int e = tid; e < 3 * 256; e += FP_THREADS) {
        unsigned int s = 0u;
        for (int w = 0; w < FP_THREADS / 64; ++w) s += (&h[w][0][0])[e];
        if (s) atomicAdd(a.hist + (size_t)blockIdx.y * 768 + e, s);
    }
}

__global__ void __launch_bounds__(256) frames_pad_median_kernel(FpArgs a) {
    __shared__ unsigned int s[2][256];
    __shared__ int found[2];
    const long long* __restrict__ p = a.plan + (size_t)blockIdx.x * FP_COLS;
    if (p[FP_VIEW] != 0) return;
    const int tid = threadIdx.x;
    const unsigned int N = (unsigned int)(p[FP_N] * p[FP_N]), r0 = (N - 1u) / 2u, r1 = N / 2u;
    for (int c = 0; c < 3; ++c) {
        const unsigned int count = a.hist[(size_t)blockIdx.x * 768 + c * 256 + tid];
        int from = 0;
        s[0][tid] = count;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1, from ^= 1) {          // inclusive scan
            s[from ^ 1][tid] = s[from][tid] + (tid >= d ? s[from][tid - d] : 0u);
            __syncthreads();
        }
        const unsigned int incl = s[from][tid], excl = incl - count;
        if (excl <= r0 && r0 < incl) found[0] = tid;          // exactly one value holds each rank
        if (excl <= r1 && r1 < incl) found[1] = tid;
        __syncthreads();
        if (tid == 0) a.median[(size_t)blockIdx.x * 3 + c] = (float)(found[0] + found[1]) * 0.5f;
        __syncthreads();
    }
}

// the finished tile in LDS -> the dense [n][n][C] image; a lane takes consecutive bytes of a tile row
__device__ __forceinline__ void fp_store_tile(unsigned char* __restrict__ dst, const unsigned char* __restrict__ tile, int n, int C, int y0, int x0) {
    for (int e = threadIdx.x; e < FP_TILE * FP_TILE * C; e += FP_THREADS) {
        const int r = e / (FP_TILE * C), q = e - r * (FP_TILE * C);
        const int j = y0 + r, i = x0 + q / C;
        if (j < n && i < n) dst[((size_t)j * n + x0) * C + q] = tile[e];
    }
}

template <bool MASK> __device__ __forceinline__ void fp_tile(const FpArgs& a, const long long* __restrict__ p, unsigned char* lds) {
    constexpr int C = MASK ? 1 : 3;
    __shared__ unsigned int s_bits;
    const FpView v = fp_view(a.buf, p);
    const int n = v.n, k = (int)p[FP_K], R = (k - 1) / 2, F = FP_TILE + 2 * R;
    const int y0 = blockIdx.y * FP_TILE, x0 = blockIdx.x * FP_TILE;
    if (y0 >= n || x0 >= n) return;
    float* mid = (float*)lds;                                   // [F][16]  the horizontal pass of one channel
    float* g = mid + F * FP_TILE;                               // [FP_WROW]
    float* sm = g + FP_WROW;                                    // [2][16]  mh of the tile's columns, mv of its rows
    int* idx = (int*)(sm + 2 * FP_TILE);                        // [2][F]  the view column | row of a halo column | row (-1: a mask's band above the view)
    unsigned char* tile = (unsigned char*)(idx + 2 * F);        // [16][16][C]  the finished tile
    unsigned char* src = tile + FP_TILE * FP_TILE * 3;          // [C][F][F]  the halo, raw values
    unsigned char* __restrict__ dst = a.buf + p[FP_WS];
    const int tid = threadIdx.x, dy = tid >> 4, dx = tid & 15, j = y0 + dy, i = x0 + dx;

    // A tile at least twice each pad away from the crop's edges has m <= -1 everywhere, so a = f = 0 whatever the rounding: a copy, decided from
    // integers alone.  Such a tile also lies inside the view (crop column i >= 2 pl is view column i - pl >= 0, and so on for each side), so the
    // border rule is the identity there; the clamp that stands in for it costs two instructions.  Where the whole group of FP_GROUP tiles along x is
    // of this kind its first workgroup copies all of it, every load in flight before the first store, and the others leave at once.
    {
        const int pt = (int)p[FP_PT], pl = (int)p[FP_PL], pb = (int)p[FP_PB], pr = (int)p[FP_PR];
        const int y1 = min(y0 + FP_TILE, n) - 1, gx0 = (int)(blockIdx.x & ~(FP_GROUP - 1)) * FP_TILE, gx1 = min(gx0 + FP_GROUP * FP_TILE, n) - 1;
        if (y0 >= 2 * pt && gx0 >= 2 * pl && n - 1 - y1 >= 2 * pb && n - 1 - gx1 >= 2 * pr) {
            if (blockIdx.x & (FP_GROUP - 1)) return;
            constexpr int ROW = FP_GROUP * FP_TILE * C, TURNS = ROW * FP_TILE / FP_THREADS;
            const int width = (gx1 - gx0 + 1) * C;
            unsigned char val[TURNS];
#pragma unroll
            for (int it = 0; it < TURNS; ++it) {
                const int e = tid + it * FP_THREADS, r = e / ROW, q = e - r * ROW, pi = q / C;
                val[it] = 0;
                if (y0 + r <= y1 && q < width)
                    val[it] = v.base[(long long)min(max(v.t + y0 + r, 0), v.H - 1) * v.rs + (long long)min(max(v.l + gx0 + pi, 0), v.W - 1) * v.ps +
                                     (q - pi * C)];
            }
#pragma unroll
            for (int it = 0; it < TURNS; ++it) {
                const int e = tid + it * FP_THREADS, r = e / ROW, q = e - r * ROW;
                if (y0 + r <= y1 && q < width) dst[((size_t)(y0 + r) * n + gx0) * C + q] = val[it];
            }
            return;
        }
    }

    // m = max(mh, mv) and 3 m + 1 is monotone in fp32, so a > 0 at a pixel iff it is > 0 for its column's mh or for its row's mv (and f > 0 only
    // where a = 1): 32 lanes decide for the tile which columns and rows need the blur
    if (tid < 2 * FP_TILE) {
        const int axis = tid >> 4, at = (axis ? y0 : x0) + (tid & 15);
        float m = -INFINITY;
        if (at < n) m = axis ? fp_side(at, n, (int)p[FP_PT], (int)p[FP_PB]) : fp_side(at, n, (int)p[FP_PL], (int)p[FP_PR]);
        sm[tid] = m;
        const unsigned long long need = __ballot(__fadd_rn(__fmul_rn(3.f, m), 1.f) > 0.f);
        if (tid == 0) s_bits = (unsigned int)need;
    }
    __syncthreads();
    const unsigned int colbits = s_bits & 0xFFFFu, rowbits = s_bits >> 16;
    if (!s_bits) {          // a copy: no halo, no blur
        for (int e = tid; e < FP_TILE * FP_TILE * C; e += FP_THREADS) {
            const int r = e / (FP_TILE * C), q = e - r * (FP_TILE * C), pi = q / C;
            if (y0 + r < n && x0 + pi < n) dst[((size_t)(y0 + r) * n + x0) * C + q] = fp_crop<MASK>(v, y0 + r, x0 + pi, q - pi * C);
        }
        return;
    }
    float wa = 0.f, wf = 0.f;
    if (j < n && i < n) {
        const float mh = sm[dx], mv = sm[FP_TILE + dy], m = fmaxf(mh, mv);
        wa = fp_clip01(__fadd_rn(__fmul_rn(3.f, m), 1.f));
        wf = fp_clip01(MASK ? mh : m);
    }
    // a row that needs the blur needs every column, a column every row: groups glo .. ghi of 4 columns and rows rlo .. rhi of the tile are blurred,
    // which takes the halo columns 4 glo .. 4 ghi + 3 + 2 R and the halo rows rlo .. rhi + 2 R
    const unsigned int gbits = rowbits ? 0xFu : ((colbits & 0xFu ? 1u : 0u) | (colbits & 0xF0u ? 2u : 0u) | (colbits & 0xF00u ? 4u : 0u) | (colbits & 0xF000u ? 8u : 0u));
    const int glo = __ffs(gbits) - 1, ghi = 31 - __clz(gbits), ng = ghi - glo + 1;
    const int rlo = colbits ? 0 : __ffs(rowbits) - 1, rhi = colbits ? FP_TILE - 1 : 31 - __clz(rowbits);
    const int fx0 = 4 * glo, nfx = 4 * ng + 2 * R, fy0 = rlo, nfy = rhi - rlo + 1 + 2 * R;

    if (tid < FP_WROW) g[tid] = a.weights[(size_t)blockIdx.z * FP_WROW + tid];
    for (int e = tid; e < 2 * F; e += FP_THREADS) {          // halo column | row -> crop coordinate through rho -> view coordinate through the border rule
        const int axis = e >= F, f = e - axis * F;
        int s = (axis ? v.t : v.l) + fp_reflect101((axis ? y0 : x0) - R + f, n);
        if (MASK) s = axis ? (s < 0 ? -1 : min(s, v.H - 1)) : min(max(s, 0), v.W - 1);
        else s = fp_reflect101(s, axis ? v.H : v.W);
        idx[e] = s;
    }
    __syncthreads();
    {   // a wave takes a halo row, its lanes consecutive bytes of it
        const int wave = tid >> 6, lane = tid & 63;
        for (int e = lane; e < nfx * C; e += 64) {
            const int fx = fx0 + e / C, c = e % C;
            const unsigned char* __restrict__ col = v.base + (long long)idx[fx] * v.ps + c;
            for (int fy = fy0 + wave; fy < fy0 + nfy; fy += FP_BATCH * (FP_THREADS / 64)) {          // FP_BATCH loads in flight before the first LDS store
                unsigned char val[FP_BATCH];
#pragma unroll
                for (int u = 0; u < FP_BATCH; ++u) {
                    const int row = fy + u * (FP_THREADS / 64), sy = row < fy0 + nfy ? idx[F + row] : -1;
                    val[u] = sy < 0 ? (unsigned char)0 : col[(long long)sy * v.rs];
                }
#pragma unroll
                for (int u = 0; u < FP_BATCH; ++u) {
                    const int row = fy + u * (FP_THREADS / 64);
                    if (row < fy0 + nfy) src[(c * F + row) * F + fx] = val[u];
                }
            }
        }
    }
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const unsigned char* __restrict__ plane = src + c * F * F;
        // horizontal: an item = 4 neighbouring outputs of one halo row, fed by one sliding read of the row; output d adds g[s - d] row[s], s ascending
        for (int e = tid; e < nfy * ng; e += FP_THREADS) {
            const int fy = fy0 + e / ng, x = 4 * (glo + e % ng);
            const unsigned char* __restrict__ row = plane + fy * F + x;
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
            for (int s = 0; s < k + 3; ++s) {
                const float w0 = s < k ? g[s] : 0.f, val = (float)row[s];
                acc0 += w0 * val; acc1 += w1 * val; acc2 += w2 * val; acc3 += w3 * val;
                w3 = w2; w2 = w1; w1 = w0;
            }
            float* out = mid + fy * FP_TILE + x;
            out[0] = acc0; out[1] = acc1; out[2] = acc2; out[3] = acc3;
        }
        __syncthreads();
        if (j < n && i < n) {
            float crop;
            if (wa > 0.f) {
                float blur = 0.f;
                for (int q = 0; q < k; ++q) blur += g[q] * mid[(dy + q) * FP_TILE + dx];
                crop = (float)plane[(dy + R) * F + dx + R];
                const float fade = MASK ? 0.f : a.median[(size_t)blockIdx.z * 3 + c];
                crop = fp_blend(fp_blend(crop, blur, wa), fade, wf);
                crop = fminf(fmaxf(rintf(crop), 0.f), 255.f);
            } else {
                crop = (float)fp_crop<MASK>(v, j, i, c);          // a == 0 and f == 0: the crop as it is
            }
            tile[tid * C + c] = (unsigned char)crop;
        }
        __syncthreads();
    }
    fp_store_tile(dst, tile, n, C, y0, x0);
}

__global__ void __launch_bounds__(FP_THREADS) frames_pad_kernel(FpArgs a) {
    extern __shared__ __align__(16) unsigned char fp_lds[];
    const long long* __restrict__ p = a.plan + (size_t)blockIdx.z * FP_COLS;
    if (p[FP_VIEW] != 0) fp_tile<true>(a, p, fp_lds);
    else fp_tile<false>(a, p, fp_lds);
}

extern "C" int lp_frames_pad(unsigned char* buf, long long buf_bytes, long long head_bytes, const long long* plan_host, const long long* plan_dev,
                             int plans, const float* weights, unsigned int* hist, float* median, void* stream) {
    char msg[224];
    if (!buf || !plan_host || !plan_dev || !weights || !hist || !median) return lp_set_error(LP_ERR_ARG, "lp_frames_pad: null pointer");
    if (plans < 1 || plans > 65535) return lp_set_error(LP_ERR_ARG, "lp_frames_pad: 1 .. 65535 plan rows are required");
    if (head_bytes < 0 || head_bytes > buf_bytes) return lp_set_error(LP_ERR_ARG, "lp_frames_pad: the packed head must lie inside the buffer");
    long long end = head_bytes, nmax = 1, nmax_image = 0, kmax = 1;
    for (int i = 0; i < plans; ++i) {
        const long long* p = plan_host + (size_t)i * FP_COLS;
        const long long row = p[FP_ROW], view = p[FP_VIEW], off = p[FP_OFF], H = p[FP_H], W = p[FP_W], rs = p[FP_RS], ps = p[FP_PS], t = p[FP_T],
                        l = p[FP_L], n = p[FP_N], ws = p[FP_WS];
        if (view != 0 && view != 1) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): view %lld is neither 0 (image) nor 1 (mask)", i, row, view);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        const long long chans = view ? 1 : 3;
        if (n < 1) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): the crop has side %lld < 1", i, row, n);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        if (n > FP_MAX_N) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): a padded crop of %lld is above %d", i, row, n, FP_MAX_N);
            return lp_set_error(LP_ERR_UNSUPPORTED, msg);
        }
        if (H < 1 || W < 1 || H >= FP_MAX_COORD || W >= FP_MAX_COORD || t <= -FP_MAX_COORD || t >= FP_MAX_COORD || l <= -FP_MAX_COORD ||
            l >= FP_MAX_COORD || rs < 0 || ps < 0 || rs >= FP_MAX_COORD || ps >= FP_MAX_COORD || off < 0 ||
            off + (H - 1) * rs + (W - 1) * ps + chans > head_bytes) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): the view lies outside the packed head of %lld bytes", i, row, head_bytes);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        const long long pads[4] = {t < 0 ? -t : 0, l < 0 ? -l : 0, t + n > H ? t + n - H : 0, l + n > W ? l + n - W : 0};
        if (pads[0] != p[FP_PT] || pads[1] != p[FP_PL] || pads[2] != p[FP_PB] || pads[3] != p[FP_PR] || pads[0] + pads[1] + pads[2] + pads[3] == 0) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): the pads are not those of a box that leaves its view", i, row);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        if (p[FP_K] != (((96 * n + 1500) / 1000) | 1)) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): k %lld is not ((96 n + 1500) / 1000) | 1 for n %lld", i, row, p[FP_K], n);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        if (ws < end || (ws & 15) || ws + n * n * chans > buf_bytes) {
            snprintf(msg, sizeof msg, "lp_frames_pad: plan %d (row %lld): the workspace image at %lld (16-byte aligned, behind the head and the "
                     "images before it) does not fit the buffer of %lld bytes", i, row, ws, buf_bytes);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        end = ws + n * n * chans;
        nmax = n > nmax ? n : nmax;
        if (!view) nmax_image = n > nmax_image ? n : nmax_image;
        kmax = p[FP_K] > kmax ? p[FP_K] : kmax;
    }
    const int F = FP_TILE + (int)kmax - 1;
    const size_t lds = (size_t)F * FP_TILE * 4 + FP_WROW * 4 + 2 * FP_TILE * 4 + (size_t)2 * F * 4 + FP_TILE * FP_TILE * 3 + (size_t)3 * F * F;
    if (kmax > FP_MAX_K || lds > 65536) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_frames_pad: the tile halo exceeds LDS");
    FpArgs a = {buf, plan_dev, weights, hist, median};
    hipStream_t s = (hipStream_t)stream;
    if (nmax_image > 0) {
        if (hipMemsetAsync(hist, 0, (size_t)plans * 768 * sizeof(unsigned int), s) != hipSuccess)
            return lp_set_error(LP_ERR_HIP, "lp_frames_pad: clearing the histograms failed");
        hipLaunchKernelGGL(frames_pad_hist_kernel, dim3((unsigned)((nmax_image + FP_HIST_ROWS - 1) / FP_HIST_ROWS), (unsigned)plans), dim3(FP_THREADS),
                           0, s, a);
        hipLaunchKernelGGL(frames_pad_median_kernel, dim3((unsigned)plans), dim3(256), 0, s, a);
    }
    const unsigned tiles = (unsigned)((nmax + FP_TILE - 1) / FP_TILE);
    hipLaunchKernelGGL(frames_pad_kernel, dim3(tiles, tiles, (unsigned)plans), dim3(FP_THREADS), lds, s, a);
    return lp_check_launch("frames_pad");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
