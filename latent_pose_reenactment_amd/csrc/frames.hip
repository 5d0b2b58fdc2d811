// From decoded frames to network-ready tensors on the device: one launch crops a whole batch of uint8 frames of different sizes to their bounding
// boxes, resizes the crops to S x S, divides by 255 and multiplies image and segmentation -- the per-frame pixel work of the reference's
// SampleLoader.load_sample (dataloaders/voxceleb2_segmentation_nolandmarks.py:89-175: crop_with_padding, cv2.resize, / 255) and of
// `image * segmentation` (:237), with the decoding left to the loader's workers.
//
// Definition (restated in fp64 by tests/frames_restatement.py, in fp32 torch ops by frames.prepare_host).  cv2 is on none of the project's machines,
// so agreement with cv2 itself cannot be checked: THIS TEXT DECIDES.
// buf: uint8, the decoded frames packed back to back.  table: R rows of 24 int64 (frames.COLUMNS), one row per output image:
//    0 ..  9  image view and box: off, H, W, row stride, pixel stride, t, l, b, r, mode      (H == 0: the row has no image)
//   10 .. 18  mask view and box:  off, H, W, row stride, pixel stride, t, l, b, r            (H == 0: the row has no mask)
//   19 .. 21  image slot, mask slot, product slot (-1: that output is not written)           22, 23 reserved, 0
// View: value(y, x, c) = buf[off + y (row stride) + x (pixel stride) + c] for 0 <= y < H, 0 <= x < W; c < 3 for an image, c = 0 for a mask.  The
//   host expresses frame[1:-1, 1:-1] (the dataset's one-pixel grey border, :125) and "second channel of the segmentation PNG" (:77) through off and
//   the strides, without a copy.
// Box: integers in view coordinates, b and r exclusive, b - t == r - l =: n >= 1; it may leave the view on any side by any amount.  The crop is
//   crop(j, i) = value(t + j, l + i) for 0 <= j, i < n, a coordinate outside the view going through the border rule:
//   image: reflected without repeating the edge (cv2.BORDER_REFLECT101, :311): period 2 (H - 1), any number of periods, a 1-pixel axis maps to 0;
//   mask:  0 for t + j < 0 (whatever the column); otherwise both coordinates are clamped to the view (replicate left, right and below, :305-309).
// Resampling the n x n crop to S x S is separable: out(dy, dx) = sum_ky wy[dy][ky] sum_kx wx[dx][kx] crop(iy[dy][ky], ix[dx][kx]), the same taps and
// weights on both axes.  Per axis, for output d (all of it integer arithmetic up to the one division that forms a weight or the fraction f):
//   area   (mode 0, images with S <= n): taps j = floor(d n / S) .. ceil((d + 1) n / S) - 1, w_j = o_j / n with the integer overlap
//          o_j = min((j + 1) S, (d + 1) n) - max(j S, d n) of [j, j + 1) and [d n / S, (d + 1) n / S), both times S.  sum o_j = n; n == S is a copy.
//   cubic  (mode 1, images with S > n): x = (d + 0.5) n / S - 0.5 = ((2 d + 1) n - S) / (2 S); i = floor(x), f = x - i (an exact fraction);
//          taps i - 1 .. i + 2, Keys weights with A = -0.75 as cv2 forms them:  w0 = ((A (f + 1) - 5 A) (f + 1) + 8 A) (f + 1) - 4 A,
//          w1 = ((A + 2) f - (A + 3)) f f + 1,  w2 = ((A + 2) (1 - f) - (A + 3)) (1 - f) (1 - f) + 1,  w3 = 1 - w0 - w1 - w2.
//   linear (masks, always): the same x, i, f; taps i, i + 1 with weights 1 - f, f.
//   Cubic and linear tap indices are clamped to the CROP (0 .. n - 1), not to the view.  The mode of an image row is chosen by the host as the
//   reference chooses it (cv2.INTER_CUBIC if imsize > b - t else cv2.INTER_AREA, :135-136; cv2.resize's default, linear, for the mask, :170).
// The sums run over the raw values 0 .. 255 in fp32 -- the horizontal pass first, then the vertical pass, each adding its taps up in order from 0
// (fused or unfused multiply-adds) -- then a cubic result is clamped to [0, 255] (cv2 saturates) and the value is DIVIDED by 255 (a correctly
// rounded fp32 division): a row with n == S comes out as exactly v / 255.  Nothing is rounded back to uint8.
// Outputs, each fp32 [slots][3][S][S], contiguous: image[slot] = the resampled image; mask[slot] = the one resampled mask value in all 3 planes (the
// contiguous real_segm); product[slot] = image x mask, one fp32 multiplication of the two values of this same workgroup (target_rgbs).
//
// Deviation from the reference, on purpose: crop_with_padding also blurs the padded bands, and a thin band inside them, with a Gaussian of
// sigma = 0.016 n and fades them to the image's per-channel median (to 0 for masks) (:314-359).  This launch does not: padded bands carry the border
// rule's pixels as they are.  The blur and fade are opt-in and live in csrc/frames_pad.hip, which writes such crops as dense uint8 images that this
// launch then reads as plain in-view boxes of a rewritten table (frames.pad_plan).  Without it: for an already-cropped dataset (no bounding-box file) the reference's own arithmetic pads 1 pixel at the top and left
// and 2 at the bottom and right of every frame, so the deviation touches a one- to two-pixel rim; for boxes that leave a raw frame it touches the
// whole padded band.  uint8 rounding between the reference's steps (after the crop, after the resize) is not reproduced either.
//
// One workgroup = one 16 x 16 output tile of one row, all channels; the row is blockIdx.z.  The per-axis taps and weights of the tile are computed
// once (32 lanes), the tile's source footprint -- at most 130 x 130 per channel for the supported scale n / S <= 8 -- is staged from the uint8 view
// into LDS through the border rule (a wave reads consecutive bytes of one source row), the horizontal pass writes an LDS intermediate, the vertical
// pass the finished tile, and a lane stores four consecutive pixels of one channel of each output with one 16-byte store when S % 4 == 0.  A row with
// both views runs the mask first and keeps its tile in LDS, so image, mask and product leave in one trip.  Every source index goes through the border
// rule or a clamp before it is used and every view is checked against the buffer before the launch, so no table row can make the kernel read outside
// buf.  No atomics, no workspace: the result is a pure function of the row, bit-identical from run to run and independent of the other rows.
#include <stdio.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file, as in its neighbours (augment.hip, image_quality.hip): tests/test_isa_lint.py, spectral_norm.hip.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define FR_TILE 16
#define FR_THREADS 256
#define FR_TAPS 9               // ceil(8) + 1: the most source pixels one area output touches per axis
#define FR_COLS 24
#define FR_MAX_SCALE 8
#define FR_MAX_S 4096
#define FR_MAX_COORD (1LL << 30)
#define FR_AREA 0
#define FR_CUBIC 1
#define FR_LINEAR 2
#define FR_IMG 0
#define FR_MSK 10
#define FR_SLOTS 19

struct FrArgs {
    const unsigned char* buf;
    const long long* table;
    float* out[3];              // image, mask, product
    int S, fmax;                // fmax: rows and columns of the LDS footprint (the largest any row of this launch needs)
};

__device__ __forceinline__ int fr_reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

__host__ __device__ __forceinline__ int fr_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// first tap (crop coordinates, before the clamp) and number of taps of output d
__host__ __device__ __forceinline__ void fr_range(int mode, int n, int S, int d, int& first, int& count) {
    if (mode == FR_AREA) {
        first = (d * n) / S;
        count = ((d + 1) * n + S - 1) / S - first;
    } else {
        const int num = (2 * d + 1) * n - S;          // > -2 S
        const int q = num < 0 ? -1 : num / (2 * S);
        first = mode == FR_CUBIC ? q - 1 : q;
        count = mode == FR_CUBIC ? 4 : 2;
    }
}

__device__ __forceinline__ void fr_weights(int mode, int n, int S, int d, int first, int count, float* __restrict__ w) {
    if (mode == FR_AREA) {
        const float fn = (float)n;
        for (int k = 0; k < count; ++k) {
            const int j = first + k;
            const int hi = min((j + 1) * S, (d + 1) * n), lo = max(j * S, d * n);
            w[k] = (float)max(hi - lo, 0) / fn;
        }
        return;
    }
    const int num = (2 * d + 1) * n - S, den = 2 * S;
    const int q = num < 0 ? -1 : num / den;
    const float f = (float)(num - q * den) / (float)den;
    if (mode == FR_LINEAR) {
        w[0] = 1.f - f; w[1] = f;
        return;
    }
    const float A = -0.75f, g = f + 1.f, e = 1.f - f;
    w[0] = ((A * g - 5.f * A) * g + 8.f * A) * g - 4.f * A;
    w[1] = ((A + 2.f) * f - (A + 3.f)) * f * f + 1.f;
    w[2] = ((A + 2.f) * e - (A + 3.f)) * e * e + 1.f;
    w[3] = 1.f - w[0] - w[1] - w[2];
}

struct FrLds {
    float* mid;                 // [fmax][16]  the horizontal pass of one channel
    float* out;                 // [4][256]    the finished tile: image channels 0 .. 2, the mask at 3
    float* w;                   // [2][16][FR_TAPS]  x axis, y axis
    int* first;                 // [2][16]
    int* count;                 // [2][16]     0 for an output beyond S
    unsigned char* src;         // [3][fmax][fmax]  the footprint, raw values
};

// one view of one row -> s.out[plane0 ...]: C = 1 (mask rule) or 3 (image rule) channels of the 16 x 16 tile at (y0, x0).  Uniform over the workgroup.
template <bool MASK> __device__ __forceinline__ void fr_resample(const unsigned char* __restrict__ buf, const long long* __restrict__ v, int mode, int S,
                                                                 int fmax, int y0, int x0, const FrLds& s, int plane0) {
    constexpr int C = MASK ? 1 : 3;
    const int tid = threadIdx.x;
    const long long off = v[0], rs = v[3], ps = v[4];
    const int H = (int)v[1], W = (int)v[2], t = (int)v[5], l = (int)v[6], n = (int)(v[7] - v[5]);
    int f0, c0, f1, c1;
    fr_range(mode, n, S, x0, f0, c0); fr_range(mode, n, S, min(x0 + FR_TILE, S) - 1, f1, c1);
    const int lo_x = fr_clampi(f0, 0, n - 1), Fx = fr_clampi(f1 + c1 - 1, 0, n - 1) - lo_x + 1;
    fr_range(mode, n, S, y0, f0, c0); fr_range(mode, n, S, min(y0 + FR_TILE, S) - 1, f1, c1);
    const int lo_y = fr_clampi(f0, 0, n - 1), Fy = fr_clampi(f1 + c1 - 1, 0, n - 1) - lo_y + 1;
    if (Fx > fmax || Fy > fmax || c0 > FR_TAPS || c1 > FR_TAPS) {          // (the host sized fmax from this table: not reached; the tile is then 0)
        for (int c = 0; c < C; ++c) s.out[(plane0 + c) * 256 + tid] = 0.f;
        __syncthreads();
        return;
    }

    if (tid < 2 * FR_TILE) {
        const int axis = tid >> 4, d = (axis ? y0 : x0) + (tid & 15);
        int first = 0, count = 0;
        if (d < S) {
            fr_range(mode, n, S, d, first, count);
            fr_weights(mode, n, S, d, first, count, s.w + tid * FR_TAPS);
        }
        s.first[tid] = first; s.count[tid] = count;
    }
    {   // footprint rows lo_y .. lo_y + Fy - 1, columns lo_x .. lo_x + Fx - 1 of the crop: a wave takes a row, its lanes consecutive bytes of it
        const int wave = tid >> 6, lane = tid & 63;
        for (int e = lane; e < Fx * C; e += 64) {
            const int fx = e / C, c = e - fx * C;
            int sx = l + lo_x + fx;
            sx = MASK ? fr_clampi(sx, 0, W - 1) : fr_reflect101(sx, W);
            const unsigned char* __restrict__ col = buf + off + (long long)sx * ps + c;
            for (int fy = wave; fy < Fy; fy += FR_THREADS / 64) {
                const int sy = t + lo_y + fy;
                unsigned char px;
                if (MASK) px = sy < 0 ? (unsigned char)0 : col[(long long)min(sy, H - 1) * rs];
                else px = col[(long long)fr_reflect101(sy, H) * rs];
                s.src[(c * fmax + fy) * fmax + fx] = px;
            }
        }
    }
    __syncthreads();

    for (int c = 0; c < C; ++c) {
        const unsigned char* __restrict__ plane = s.src + c * fmax * fmax;
        for (int e = tid; e < Fy * FR_TILE; e += FR_THREADS) {
            const int fy = e >> 4, dx = e & 15;
            const int first = s.first[dx], count = s.count[dx];
            float acc = 0.f;
            for (int k = 0; k < count; ++k)
                acc += s.w[dx * FR_TAPS + k] * (float)plane[fy * fmax + fr_clampi(first + k, 0, n - 1) - lo_x];
            s.mid[e] = acc;
        }
        __syncthreads();
        {
            const int dy = tid >> 4, dx = tid & 15;
            const int first = s.first[FR_TILE + dy], count = s.count[FR_TILE + dy];
            float acc = 0.f;
            for (int k = 0; k < count; ++k)
                acc += s.w[(FR_TILE + dy) * FR_TAPS + k] * s.mid[(fr_clampi(first + k, 0, n - 1) - lo_y) * FR_TILE + dx];
            if (mode == FR_CUBIC) acc = fminf(fmaxf(acc, 0.f), 255.f);
            s.out[(plane0 + c) * 256 + tid] = acc / 255.f;
        }
        __syncthreads();
    }
}

template <bool VEC> __global__ void __launch_bounds__(FR_THREADS) frames_prepare_kernel(FrArgs a) {
    extern __shared__ __align__(16) unsigned char fr_lds[];
    FrLds s;
    s.mid = (float*)fr_lds;
    s.out = s.mid + a.fmax * FR_TILE;
    s.w = s.out + 4 * 256;
    s.first = (int*)(s.w + 2 * FR_TILE * FR_TAPS);
    s.count = s.first + 2 * FR_TILE;
    s.src = (unsigned char*)(s.count + 2 * FR_TILE);

    const long long* __restrict__ row = a.table + (size_t)blockIdx.z * FR_COLS;
    const int S = a.S, y0 = blockIdx.y * FR_TILE, x0 = blockIdx.x * FR_TILE;
    const long long slot_i = row[FR_SLOTS], slot_m = row[FR_SLOTS + 1], slot_p = row[FR_SLOTS + 2];
    const bool img = row[FR_IMG + 1] > 0 && (slot_i >= 0 || slot_p >= 0), msk = row[FR_MSK + 1] > 0 && (slot_m >= 0 || slot_p >= 0);
    if (msk) fr_resample<true>(a.buf, row + FR_MSK, FR_LINEAR, S, a.fmax, y0, x0, s, 3);
    if (img) fr_resample<false>(a.buf, row + FR_IMG, row[FR_IMG + 9] == FR_CUBIC ? FR_CUBIC : FR_AREA, S, a.fmax, y0, x0, s, 0);

    // lane -> (channel, row, quad)
    const int tid = threadIdx.x, c = tid >> 6, r = (tid >> 2) & (FR_TILE - 1), q = tid & 3;
    const int y = y0 + r, x = x0 + 4 * q;
    if (c >= 3 || y >= S || x >= S) return;
    float v[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (img) v[i] = s.out[c * 256 + r * FR_TILE + 4 * q + i];
        if (msk) m[i] = s.out[3 * 256 + r * FR_TILE + 4 * q + i];
    }
    const long long slots[3] = {img ? slot_i : -1, msk ? slot_m : -1, img && msk ? slot_p : -1};
    for (int o = 0; o < 3; ++o) {
        if (slots[o] < 0) continue;
        float w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = o == 0 ? v[i] : (o == 1 ? m[i] : v[i] * m[i]);
        float* p = a.out[o] + (((size_t)slots[o] * 3 + c) * S + y) * (size_t)S + x;
        if (VEC) {          // S % 4 == 0: the quad is whole and 16-byte aligned
            *(float4*)p = make_float4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < S) p[i] = w[i];
        }
    }
}

static int fr_footprint(int mode, long long n, int S) {
    const long long f = mode == FR_AREA ? (16 * n + S - 1) / S + 2 : (15 * n + S - 1) / S + 5;
    return (int)(f < n ? f : n);
}

extern "C" int lp_frames_prepare(const unsigned char* buf, long long buf_bytes, const long long* table_host, const long long* table_dev, int rows,
                                 int S, float* image, int n_image, float* mask, int n_mask, float* product, int n_product, void* stream) {
    char msg[192];
    if (!buf || !table_host || !table_dev) return lp_set_error(LP_ERR_ARG, "lp_frames_prepare: null pointer");
    if (rows < 1 || rows > 65535) return lp_set_error(LP_ERR_ARG, "lp_frames_prepare: 1 .. 65535 rows are required");
    if (S < 1 || S > FR_MAX_S) return lp_set_error(LP_ERR_ARG, "lp_frames_prepare: S must be in 1 .. 4096");
    if (n_image < 0 || n_mask < 0 || n_product < 0 || (n_image > 0 && !image) || (n_mask > 0 && !mask) || (n_product > 0 && !product))
        return lp_set_error(LP_ERR_ARG, "lp_frames_prepare: an output with slots needs its pointer");
    const long long counts[3] = {n_image, n_mask, n_product};
    int fmax = 1;
    for (int i = 0; i < rows; ++i) {
        const long long* r = table_host + (size_t)i * FR_COLS;
        const bool has[2] = {r[FR_IMG + 1] != 0, r[FR_MSK + 1] != 0};
        bool any = false;
        for (int o = 0; o < 3; ++o) {
            const long long sl = r[FR_SLOTS + o];
            if (sl < -1 || sl >= counts[o]) {
                snprintf(msg, sizeof msg, "lp_frames_prepare: row %d: slot %lld of output %d is outside 0 .. %lld", i, sl, o, counts[o] - 1);
                return lp_set_error(LP_ERR_ARG, msg);
            }
            any = any || sl >= 0;
            if (sl >= 0 && ((o != 1 && !has[0]) || (o != 0 && !has[1]))) {
                snprintf(msg, sizeof msg, "lp_frames_prepare: row %d asks for output %d without the view it needs", i, o);
                return lp_set_error(LP_ERR_ARG, msg);
            }
        }
        if (!any) {
            snprintf(msg, sizeof msg, "lp_frames_prepare: row %d writes no output", i);
            return lp_set_error(LP_ERR_ARG, msg);
        }
        for (int view = 0; view < 2; ++view) {
            if (!has[view]) continue;
            const long long* v = r + (view ? FR_MSK : FR_IMG);
            const long long off = v[0], H = v[1], W = v[2], rs = v[3], ps = v[4], t = v[5], l = v[6], n = v[7] - v[5];
            const int chans = view ? 1 : 3;
            if (n < 1 || n != v[8] - v[6]) {
                snprintf(msg, sizeof msg, "lp_frames_prepare: row %d: the box of view %d is not square with side >= 1", i, view);
                return lp_set_error(LP_ERR_ARG, msg);
            }
            if (H < 1 || W < 1 || H >= FR_MAX_COORD || W >= FR_MAX_COORD || t <= -FR_MAX_COORD || t >= FR_MAX_COORD || l <= -FR_MAX_COORD ||
                l >= FR_MAX_COORD || rs < 0 || ps < 0 || rs >= FR_MAX_COORD || ps >= FR_MAX_COORD || off < 0 ||
                off + (H - 1) * rs + (W - 1) * ps + chans > buf_bytes) {
                snprintf(msg, sizeof msg, "lp_frames_prepare: row %d: view %d lies outside the buffer of %lld bytes", i, view, buf_bytes);
                return lp_set_error(LP_ERR_ARG, msg);
            }
            if (n > (long long)FR_MAX_SCALE * S) {
                snprintf(msg, sizeof msg, "lp_frames_prepare: row %d: crop %lld -> %d is a scale above %d", i, n, S, FR_MAX_SCALE);
                return lp_set_error(LP_ERR_UNSUPPORTED, msg);
            }
            int mode = FR_LINEAR;
            if (!view) {
                mode = S <= n ? FR_AREA : FR_CUBIC;
                if (v[9] != mode) {
                    snprintf(msg, sizeof msg, "lp_frames_prepare: row %d: mode %lld for %lld -> %d (0 = area when S <= n, else 1 = cubic)", i, v[9], n, S);
                    return lp_set_error(LP_ERR_ARG, msg);
                }
            }
            const int f = fr_footprint(mode, n, S);
            fmax = f > fmax ? f : fmax;
        }
    }
    const size_t lds = (size_t)fmax * FR_TILE * 4 + 4 * 256 * 4 + 2 * FR_TILE * FR_TAPS * 4 + 4 * FR_TILE * 4 + (size_t)3 * fmax * fmax;
    if (fmax > 130 || lds > 65536) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_frames_prepare: the tile footprint exceeds LDS");
    FrArgs a = {buf, table_dev, {image, mask, product}, S, fmax};
    const unsigned tiles = (unsigned)((S + FR_TILE - 1) / FR_TILE);
    const bool vec = S % 4 == 0 && (((uintptr_t)image | (uintptr_t)mask | (uintptr_t)product) & 15) == 0;
    const dim3 grid(tiles, tiles, (unsigned)rows), block(FR_THREADS);
    if (vec) hipLaunchKernelGGL(frames_prepare_kernel<true>, grid, block, lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(frames_prepare_kernel<false>, grid, block, lds, (hipStream_t)stream, a);
    return lp_check_launch("frames_prepare");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
