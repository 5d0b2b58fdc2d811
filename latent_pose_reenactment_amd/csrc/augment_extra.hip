// Second stage of the pose-input augmentation, for the pose image only: elastic jitter, 3 x 3 median, saturation and JPEG block quantisation in ONE
// launch behind lp_augment_triplet (csrc/augment.hip) -- the four pixelwise augmenters of the reference (dataloaders/common/augmentation.py:44-81)
// that do not fit a 3 x 3 filter kernel: ElasticTransformation (:76), MedianBlur (:53), AddToSaturation (:67), JpegCompression (:68).  Opt-in
// (--use_extra_pixelwise_augs); the random draws are made by the loader and handed over as 16 floats per sample.
//
// Definition (restated in fp64 by tests/augment_extra_restatement.py, in fp32 torch ops by augmentation.augment_extra_host).
// x: logical B x 3 x H x W fp32 in [0, 1], any strides.  Per sample b a row p = params[b][0:16] (fp32; hipops.AUG_EXTRA_COLUMNS):
//    0  elastic_alpha   displacement amplitude in pixels; 0 = off
//    1  elastic_seed    an integer in [0, 2^24), exact in fp32 (clamped to that range, then truncated)
//    2  median          0 = off, anything else = on
//    3  saturation      d, added to the HSV saturation; 0 = off.  The loader draws (-20 .. 20) / 255
//    4  jpeg_quality    0 = off, otherwise an integer 1 .. 100 (clamped to that range, then truncated)
//    5 .. 15  reserved, 0
// The all-zero row is neutral.  A step at its neutral value is SKIPPED, not computed; the steps run in this fixed order; the final clamp to [0, 1]
// always runs, as in the first stage: a neutral row returns an input in [0, 1] bit for bit.  reflect101(i, n) is the border rule of augment.hip
// (reflected without repeating the edge, period 2 (n - 1), any number of periods, n == 1 maps everything to 0); mix32 is the hash of augment.hip.
//
// 1. Elastic.  For a pixel (y, x) INSIDE the frame, n = y W + x (mod 2^32), key = seed * 0x85EBCA6B (mod 2^32; another multiplier than the noise
//    step's 0x9E3779B9, so that equal seeds do not correlate), u(j) = (mix32((2 n + j) ^ key) >> 8) 2^-23 - 1 in [-1, 1), exact in fp32;
//      xs = x + alpha u(0), ys = y + alpha u(1);  x0 = floor(xs), fx = xs - x0, y0 = floor(ys), fy = ys - y0;
//      top = x(y0, x0) (1 - fx) + x(y0, x0 + 1) fx, bot = the same on row y0 + 1, E(y, x) = top (1 - fy) + bot fy, per channel,
//    every tap index through reflect101.  alpha == 0: E = x.  E is a pure function of the pixel index.
// 2. Median.  F(y, x) = the per-channel median of the nine values E(reflect101(y + i, H), reflect101(x + j, W)), i, j in {-1, 0, 1}.  Off: F = E.
// 3. Saturation (HSV-additive, value-preserving, continuous at grey).  Per pixel M = max and m = min over the three channels, S = (M - m) / M and
//    S = 0 when M == 0; s0 = 20 / 255; t = max(S, s0); g = clamp01(t + d) / t; c' = M - (M - c) g for every channel c.  A grey pixel (M == m) stays
//    grey, the maximum channel keeps its value.  For |d| <= s0 the map is Lipschitz with constant 3 + s0 in the sup norm (tests/test_augment_extra_gpu.py).
// 4. JPEG: baseline JPEG, 4:4:4, without the entropy coding (which is lossless).  In 8 x 8 blocks anchored at (0, 0); a block that overhangs the
//    right or bottom edge is filled by replicating the last column / row of the image of step 3.  (R, G, B) = 255 c';
//      Y = 0.299 R + 0.587 G + 0.114 B - 128,  Cb = -0.168736 R - 0.331264 G + 0.5 B,  Cr = 0.5 R - 0.418688 G - 0.081312 B
//    (JFIF, the + 128 of the chroma planes cancelled by the level shift).  Per plane and block the orthonormal DCT-II, D = C X C^T with
//    C[k][n] = a(k) cos((2 n + 1) k pi / 16), a(0) = sqrt(1 / 8), a(k) = 1 / 2: rows first, then columns, each an 8-term sum from n = 0; quantised
//    D' = q rint(D / q) (rint: ties to even); X' = C^T D' C, columns first, then rows, from k = 0; Y += 128;
//      R = Y + 1.402 Cr, G = Y - 0.344136 Cb - 0.714136 Cr, B = Y + 1.772 Cb;  result = (R, G, B) / 255.  Nothing is rounded to uint8.
//    q[u][v] (u the vertical frequency) = clamp(floor((base[u][v] scale + 50) / 100), 1, 255) in integer arithmetic, base = the Annex-K luminance
//    table for Y and the chrominance table for Cb, Cr, scale = 5000 / quality (integer division) below 50 and 200 - 2 quality from 50 on (IJG).
// Then clamp to [0, 1].
//
// Deviations from the reference, all on purpose:
//   * elastic: the reference smooths the displacement field with sigma = 0.15, which gives the nearest neighbour a weight of e^(-1 / 0.045), about
//     2e-10: the smoothing is dropped.  Bilinear taps (imgaug's default order is cubic), alpha drawn in (0.5, 3.5) as there;
//   * median: imgaug's k = (1, 3) leaves k = 3 as the only effect;
//   * saturation: the reference goes through uint8 HSV, where grey pixels have hue 0 and turn red when saturation is added.  That is not
//     reproduced: below S = s0 the gain is that of S = s0, so grey stays grey and the map is continuous;
//   * JPEG: imgaug goes through PIL's default 4:2:0 with "fancy" chroma upsampling, which reaches across blocks; here 4:4:4, float DCT, no uint8
//     rounding before or after (against PIL with subsampling=0: tests/test_augment_extra_cpu.py);
//   * a fixed order of the steps, fp32 throughout;
//   * still not provided: the simplex-noise edge blend (:60-62).
//
// One workgroup of 256 lanes = one image x one 16 x 16 output tile = 2 x 2 JPEG blocks per plane (the tile grid is the block grid); a lane owns one
// pixel with its three channels (saturation and the colour transforms need them together).  Lanes beyond the right / bottom edge take the last
// column / row -- the replication of step 4 -- and store nothing.  With the median on, the 18 x 18 x 3 halo tile of E is staged in LDS (bilinear
// taps straight from global memory through the border rule) and the median is a fixed 19-exchange selection network on nine LDS values; without
// it a lane computes E for its own pixel.  JPEG: the planes go to LDS as [plane][16][16] and the four 1-D passes (rows, columns, quantise,
// columns, rows) run with ONE OUTPUT VALUE PER LANE AND PLANE: an 8-term sum over LDS, a barrier, the write back, a barrier.  At a row stride of 16
// floats a 32-lane half (two tile rows) reads, in the row passes, four distinct addresses n, n + 8, n + 16, n + 24 (broadcast) and, in the column
// passes, sixteen consecutive ones; it writes 32 consecutive ones: no pass bank-conflicts and the rows need no padding.  The 8 x 8 basis sits in LDS
// at a row stride of 9 (lanes of eight different frequencies read eight different banks).  The finished tile goes through the same LDS planes to
// the store phase of augment.hip: a lane per channel x row x four pixels, one 16-byte store when W % 4 == 0 and the output is 16-byte aligned,
// pixel by pixel otherwise.  LDS: 3.9 + 3 + 0.3 = 7.2 KB.  Every step is skipped per workgroup when the row says so (uniform: the row belongs to the
// sample).  Every source index goes through the border rule and the source coordinate is clamped before it becomes an integer, so no parameter
// row -- NaN included -- can make the kernel read outside the image.  No atomics, no workspace, no table beyond the parameter rows (the basis and
// the two base tables are constants of this file): the result is a pure function of the inputs, bit-identical from run to run, independent of B.
#include <math.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file, as in augment.hip (tests/test_isa_lint.py).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define EX_TILE 16
#define EX_HALO (EX_TILE + 2)             // 18
#define EX_THREADS 256
#define EX_COLS 16
#define EX_KEY 0x85EBCA6Bu
#define EX_CSTRIDE 9

struct ExSrc { const float* p; long long sn, sc, sh, sw; };

// C[k][n] = a(k) cos((2 n + 1) k pi / 16), rounded to fp32
__constant__ float ex_dct[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f,
};

// ITU-T T.81 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major with the vertical frequency as the row
__constant__ unsigned char ex_qbase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99},
};

__device__ __forceinline__ int ex_reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// (the clamp keeps the float -> int conversion defined for any parameter row; NaN goes to the lower bound)
__device__ __forceinline__ int ex_floor_index(float f) { return (int)fminf(fmaxf(f, -1.0e9f), 1.0e9f); }

__device__ __forceinline__ unsigned ex_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// E(y, x) of the three channels; (y, x) inside the frame
__device__ __forceinline__ void ex_elastic(const float* __restrict__ img, const ExSrc& s, bool elastic, float alpha, unsigned key, int y, int x,
                                           int H, int W, float* e) {
    if (!elastic) {
        const float* q = img + (long long)y * s.sh + (long long)x * s.sw;
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = q[c * s.sc];
        return;
    }
    const unsigned n = (unsigned)y * (unsigned)W + (unsigned)x;
    const float ux = (float)(ex_mix32((2u * n) ^ key) >> 8) * 1.1920928955078125e-07f - 1.f;          // 2^-23
    const float uy = (float)(ex_mix32((2u * n + 1u) ^ key) >> 8) * 1.1920928955078125e-07f - 1.f;
    const float xs = (float)x + alpha * ux, ys = (float)y + alpha * uy;
    const float x0f = floorf(xs), y0f = floorf(ys);
    const float fx = xs - x0f, fy = ys - y0f;
    const int x0 = ex_floor_index(x0f), y0 = ex_floor_index(y0f);
    const long long xa = (long long)ex_reflect101(x0, W) * s.sw, xb = (long long)ex_reflect101(x0 + 1, W) * s.sw;
    const long long ya = (long long)ex_reflect101(y0, H) * s.sh, yb = (long long)ex_reflect101(y0 + 1, H) * s.sh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* q = img + c * s.sc;
        const float top = q[ya + xa] * (1.f - fx) + q[ya + xb] * fx, bot = q[yb + xa] * (1.f - fx) + q[yb + xb] * fx;
        e[c] = top * (1.f - fy) + bot * fy;
    }
}

#define EX_SORT2(a, b) { const float lo_ = fminf(a, b), hi_ = fmaxf(a, b); a = lo_; b = hi_; }

// the median of nine values: the 19-exchange selection network (the classic "opt_med9")
__device__ __forceinline__ float ex_median9(float* v) {
    EX_SORT2(v[1], v[2]); EX_SORT2(v[4], v[5]); EX_SORT2(v[7], v[8]);
    EX_SORT2(v[0], v[1]); EX_SORT2(v[3], v[4]); EX_SORT2(v[6], v[7]);
    EX_SORT2(v[1], v[2]); EX_SORT2(v[4], v[5]); EX_SORT2(v[7], v[8]);
    EX_SORT2(v[0], v[3]); EX_SORT2(v[5], v[8]); EX_SORT2(v[4], v[7]);
    EX_SORT2(v[3], v[6]); EX_SORT2(v[1], v[4]); EX_SORT2(v[2], v[5]);
    EX_SORT2(v[4], v[7]); EX_SORT2(v[4], v[2]); EX_SORT2(v[6], v[4]);
    EX_SORT2(v[4], v[2]);
    return v[4];
}

// one 1-D pass of one plane: sum_i coef[cbase + i cstep] * plane[base + i step], i = 0 .. 7, added up from 0
__device__ __forceinline__ float ex_sum8(const float* __restrict__ plane, int base, int step, const float* __restrict__ coef, int cbase, int cstep) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += coef[cbase + i * cstep] * plane[base + i * step];
    return acc;
}

template <bool VEC> __global__ void __launch_bounds__(EX_THREADS)
augment_extra_kernel(ExSrc s, const float* __restrict__ params, float* __restrict__ out, int H, int W) {
    __shared__ float s_e[3][EX_HALO * EX_HALO];          // E around the tile: [c][(row + 1) * 18 + column + 1]
    __shared__ float s_d[3][EX_TILE * EX_TILE];          // the planes of the tile: [plane][row * 16 + column]
    __shared__ float s_c[8 * EX_CSTRIDE];                // the DCT basis: [k * 9 + n]
    const int tid = threadIdx.x, b = blockIdx.z;
    const float* __restrict__ p = params + (size_t)b * EX_COLS;
    const float alpha = p[0], d = p[3], fq = p[4];
    // (uniform over the workgroup: properties of the sample)
    const bool elastic = alpha != 0.f, median = p[2] != 0.f, sat = d != 0.f, jpeg = fq != 0.f;
    const unsigned key = (unsigned)(int)fminf(fmaxf(p[1], 0.f), 16777215.f) * EX_KEY;
    const int y0 = blockIdx.y * EX_TILE, x0 = blockIdx.x * EX_TILE;
    const float* __restrict__ img = s.p + (long long)b * s.sn;

    // lane -> pixel of the tile; beyond the edge: the last row / column
    const int ty = tid >> 4, tx = tid & (EX_TILE - 1);
    const int tyc = min(ty, H - 1 - y0), txc = min(tx, W - 1 - x0);
    float v[3];
    if (median) {
        for (int r = tid; r < EX_HALO * EX_HALO; r += EX_THREADS) {
            const int i = r / EX_HALO, j = r - i * EX_HALO;
            float e[3];
            ex_elastic(img, s, elastic, alpha, key, ex_reflect101(y0 + i - 1, H), ex_reflect101(x0 + j - 1, W), H, W, e);
#pragma unroll
            for (int c = 0; c < 3; ++c) s_e[c][r] = e[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float m9[9];
#pragma unroll
            for (int ii = 0; ii < 3; ++ii)
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) m9[3 * ii + jj] = s_e[c][(tyc + ii) * EX_HALO + txc + jj];
            v[c] = ex_median9(m9);
        }
    } else {
        ex_elastic(img, s, elastic, alpha, key, y0 + tyc, x0 + txc, H, W, v);
    }

    if (sat) {
        const float M = fmaxf(v[0], fmaxf(v[1], v[2])), m = fminf(v[0], fminf(v[1], v[2]));
        const float S = M > 0.f ? (M - m) / M : 0.f;
        const float t = fmaxf(S, 20.f / 255.f);
        const float g = fminf(fmaxf(t + d, 0.f), 1.f) / t;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = M - (M - v[c]) * g;
    }

    const int at = ty * EX_TILE + tx;
    if (jpeg) {
        if (tid < 64) s_c[(tid >> 3) * EX_CSTRIDE + (tid & 7)] = ex_dct[tid];
        const int quality = (int)fminf(fmaxf(fq, 1.f), 100.f);
        const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        const int ku = ty & 7, kv = tx & 7;          // the lane's frequency (forward) or position (inverse) inside its block
        const float ql = (float)min(max(((int)ex_qbase[0][ku * 8 + kv] * scale + 50) / 100, 1), 255);
        const float qc = (float)min(max(((int)ex_qbase[1][ku * 8 + kv] * scale + 50) / 100, 1), 255);
        const float R = 255.f * v[0], G = 255.f * v[1], B = 255.f * v[2];
        s_d[0][at] = 0.299f * R + 0.587f * G + 0.114f * B - 128.f;
        s_d[1][at] = -0.168736f * R - 0.331264f * G + 0.5f * B;
        s_d[2][at] = 0.5f * R - 0.418688f * G - 0.081312f * B;
        __syncthreads();
        const int row = ty * EX_TILE + (tx & 8), col = (ty & 8) * EX_TILE + tx;
        float a[3];
        // rows, forward: D1[y][v] = sum_n C[v][n] X[y][n]
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = ex_sum8(s_d[c], row, 1, s_c, kv * EX_CSTRIDE, 1);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) s_d[c][at] = a[c];
        __syncthreads();
        // columns, forward: D[u][v] = sum_n C[u][n] D1[n][v]; quantise
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = ex_sum8(s_d[c], col, EX_TILE, s_c, ku * EX_CSTRIDE, 1);
        __syncthreads();
        s_d[0][at] = ql * rintf(a[0] / ql);
        s_d[1][at] = qc * rintf(a[1] / qc);
        s_d[2][at] = qc * rintf(a[2] / qc);
        __syncthreads();
        // columns, inverse: X1[y][v] = sum_k C[k][y] D'[k][v]
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = ex_sum8(s_d[c], col, EX_TILE, s_c, ku, EX_CSTRIDE);
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 3; ++c) s_d[c][at] = a[c];
        __syncthreads();
        // rows, inverse: X'[y][x] = sum_k C[k][x] X1[y][k]
#pragma unroll
        for (int c = 0; c < 3; ++c) a[c] = ex_sum8(s_d[c], row, 1, s_c, kv, EX_CSTRIDE);
        __syncthreads();
        const float Y = a[0] + 128.f;
        v[0] = (Y + 1.402f * a[2]) / 255.f;
        v[1] = (Y - 0.344136f * a[1] - 0.714136f * a[2]) / 255.f;
        v[2] = (Y + 1.772f * a[1]) / 255.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) s_d[c][at] = fminf(fmaxf(v[c], 0.f), 1.f);
    __syncthreads();

    // store: lane -> (channel, row, quad), as augment.hip
    const int c = tid >> 6, r = (tid >> 2) & (EX_TILE - 1), q = tid & 3;
    const int yd = y0 + r, xq = x0 + 4 * q;
    if (c >= 3 || yd >= H || xq >= W) return;
    const float* t4 = &s_d[c][r * EX_TILE + 4 * q];
    float* o = out + (((size_t)b * 3 + c) * H + yd) * (size_t)W + xq;
    if (VEC) {          // W % 4 == 0: the quad is whole and 16-byte aligned
        *(float4*)o = make_float4(t4[0], t4[1], t4[2], t4[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (xq + i < W) o[i] = t4[i];
    }
}

extern "C" int lp_augment_extra(const float* pose, const long long* pose_strides, const float* params, int B, int C, int H, int W, float* out,
                                void* stream) {
    if (!pose || !pose_strides || !params || !out) return lp_set_error(LP_ERR_ARG, "lp_augment_extra: null pointer");
    if (B < 1) return lp_set_error(LP_ERR_ARG, "lp_augment_extra: B >= 1 is required");
    if (C != 3) return lp_set_error(LP_ERR_ARG, "lp_augment_extra: C must be 3 (saturation and JPEG are defined on RGB)");
    if (H < 1 || W < 1) return lp_set_error(LP_ERR_ARG, "lp_augment_extra: H >= 1 and W >= 1 are required");
    const long long tiles_x = ((long long)W + EX_TILE - 1) / EX_TILE, tiles_y = ((long long)H + EX_TILE - 1) / EX_TILE;
    if (tiles_x > 0x7fffffffLL || tiles_y > 65535 || B > 65535)
        return lp_set_error(LP_ERR_UNSUPPORTED, "lp_augment_extra: B or H x W exceeds one launch grid");
    const ExSrc s = {pose, pose_strides[0], pose_strides[1], pose_strides[2], pose_strides[3]};
    const bool vec = W % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)B), block(EX_THREADS);
    if (vec) hipLaunchKernelGGL(augment_extra_kernel<true>, grid, block, 0, (hipStream_t)stream, s, params, out, H, W);
    else hipLaunchKernelGGL(augment_extra_kernel<false>, grid, block, 0, (hipStream_t)stream, s, params, out, H, W);
    return lp_check_launch("augment_extra");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
