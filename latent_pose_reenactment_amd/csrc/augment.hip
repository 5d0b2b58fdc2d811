// Augmentation of the pose-encoder input on the device: one launch resamples the triplet (pose image, target image, segmentation) and filters the pose
// image -- the reference's augmenter.augment_triplet (dataloaders/common/augmentation.py:123-142, called per sample by
// dataloaders/voxceleb2_segmentation_nolandmarks.py:243-246) with the random draws made by the loader and handed over as 32 floats per sample.
//
// Definition (restated in fp64 by tests/augment_restatement.py, in fp32 torch ops by augmentation.augment_triplet_host).
// pose, target: logical B x C x H x W fp32, segm: B x Cs x H x W fp32, any strides (a stride-0 expand included); C, Cs <= 4.  Per sample b a row
// p = params[b][0:32] (fp32; hipops.AUG_COLUMNS):
//    0 ..  5  Ap     2 x 3 INVERSE map of the pose image, row-major: (xs, ys) = Ap (xd, yd, 1) in pixel-index coordinates (centres at integers)
//    6 .. 11  At     the same for target and segm
//   12 .. 20  k      3 x 3 filter taps of the pose image, row-major, k[1][1] the centre
//   21        mul                                   22 .. 24  add[c] (C = 1 uses column 22; a fourth channel gets 0)
//   25        alpha  linear contrast 0.5 + alpha (v - 0.5)
//   26        gain   sigmoid contrast 1 / (1 + exp(gain (0.5 - v))); 0 = off
//   27        sigma  additive Gaussian noise, one value per pixel shared by the channels
//   28        seed   an integer in [0, 2^24), exact in fp32          29 .. 31 reserved, 0
// Neutral row: Ap = At = (1 0 0 / 0 1 0), k = (0 0 0 / 0 1 0 / 0 0 0), mul = 1, add = 0, alpha = 1, gain = sigma = seed = 0.
//
// warp(img, A, border)(yd, xd), for ANY integers yd, xd (the map is defined on the whole plane):
//   xs = A[0] xd + A[1] yd + A[2], ys = A[3] xd + A[4] yd + A[5];  x0 = floor(xs), fx = xs - x0, y0 = floor(ys), fy = ys - y0;
//   top = img(y0, x0) (1 - fx) + img(y0, x0 + 1) fx,  bot = the same on row y0 + 1,  value = top (1 - fy) + bot fy.
//   A tap index outside the image: border reflect101 -- reflected without repeating the edge, period 2 (n - 1), any number of periods, n == 1 maps
//   everything to 0 (what imgaug's mode="reflect" becomes on its cv2 backend: not checkable here, so this text decides); border zero -- the tap is 0.
//   When A is exactly the identity the resampling is skipped: the value is img(yd, xd) itself (through the border rule outside the frame).
// target' = warp(target, At, reflect101);  segm' = warp(segm, At, zero) (the reference resamples the mask as a heatmap with a constant-0 border,
// augmentation.py:135; bilinear here where imgaug takes bicubic, so the mask stays in [0, 1]).
// pose': w = warp(pose, Ap, reflect101); v = sum_ij k[i][j] w(yd + i - 1, xd + j - 1), added up row-major from 0 (no border rule of its own: w exists
// outside the frame); then, in this order: v mul; + add[c]; linear contrast; sigmoid contrast; + sigma z(b, yd, xd); clamp to [0, 1].
// A step whose parameter equals its neutral value exactly is SKIPPED, not computed (the filter when k is exactly the identity): a neutral row returns
// the three tensors bit for bit.  The clamp always runs -- the pose image is in [0, 1] by contract; values outside come back clamped.
// Noise, a pure function of (seed, yd, xd): n = yd W + xd, h(j) = mix32((2 n + j) ^ (seed * 0x9E3779B9)), all mod 2^32,
//   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;
//   u1 = ((h(0) >> 9) + 0.5) 2^-23, u2 = (h(1) >> 8) 2^-24 (both exact in fp32), z = sqrt(-2 ln u1) cos(2 pi u2) with the precise logf / cosf.
//
// Deviations from the reference (dataloaders/common/augmentation.py), all on purpose:
//   * ONE resampling with the composed map where the reference warps twice in uint8 (self.seq with the scale, :127, then shift_seq, :134);
//   * fp32 throughout, no uint8 quantisation (:116, :125, :130);
//   * a fixed order of the steps where the reference shuffles them (random_order=True, :79 and :103);
//   * one 3 x 3 filter slot per sample where SomeOf can chain blur, sharpen and emboss (:46-57);
//   * not provided: MedianBlur (:53), JpegCompression (:68), ElasticTransformation (:76), the simplex-noise edge blend (:60-62), AddToSaturation (:67).
//     (Not provided HERE: all but the edge blend are the opt-in second stage, one more launch on the pose image -- csrc/augment_extra.hip.)
//
// One workgroup = one role (pose | target | segm) x one image x one 16 x 16 output tile; role and image are blockIdx.z.  A lane owns one channel of
// four consecutive pixels of a row (C x 16 rows x 4 quads <= 256 lanes) and stores them with one 16-byte store when W % 4 == 0 (and the outputs are
// 16-byte aligned), pixel by pixel otherwise.  A pose workgroup whose sample has a filter stages the warped 18 x 18 x C halo tile in LDS once and takes
// the nine taps from there; every other workgroup skips the staging.  Every source index goes through the border rule and the source coordinate is
// clamped before it becomes an integer, so no parameter row -- NaN included -- can make the kernel read outside the images.  No atomics, no workspace:
// the result is a pure function of the inputs, bit-identical from run to run and independent of B.
#include <math.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file: four pixels times one broadcast tap is the "pair times a scalar" shape for which hipcc picks
// v_pk_*_f32 with op_sel:[0,1] (wrong beside the LDS-DMA convolution kernels on gfx950: tests/test_isa_lint.py, spectral_norm.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define AUG_TILE 16
#define AUG_HALO (AUG_TILE + 2)             // 18
#define AUG_THREADS 256
#define AUG_MAX_C 4
#define AUG_COLS 32

struct AugSrc { const float* p; long long sn, sc, sh, sw; };
struct AugArgs {
    AugSrc src[3];          // pose, target, segm
    float* out[3];
    int role[3];            // blockIdx.z / B -> role (the roles present, in order)
    int chan[3];            // channels per role
};

__device__ __forceinline__ int aug_reflect101(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// img(y, x) of one channel plane through the border rule
template <bool REFLECT> __device__ __forceinline__ float aug_tap(const float* __restrict__ p, long long sh, long long sw, int y, int x, int H, int W) {
    if (REFLECT) {
        y = aug_reflect101(y, H); x = aug_reflect101(x, W);
    } else if (y < 0 || y >= H || x < 0 || x >= W) {
        return 0.f;
    }
    return p[(long long)y * sh + (long long)x * sw];
}

// (the clamp keeps the float -> int conversion defined for any parameter row; NaN goes to the lower bound)
__device__ __forceinline__ int aug_floor_index(float f) { return (int)fminf(fmaxf(f, -1.0e9f), 1.0e9f); }

template <bool REFLECT> __device__ __forceinline__ float aug_warp(const float* __restrict__ p, long long sh, long long sw, const float* A, bool ident,
                                                                  int yd, int xd, int H, int W) {
    if (ident) return aug_tap<REFLECT>(p, sh, sw, yd, xd, H, W);
    const float fxd = (float)xd, fyd = (float)yd;
    const float xs = A[0] * fxd + A[1] * fyd + A[2], ys = A[3] * fxd + A[4] * fyd + A[5];
    const float x0f = floorf(xs), y0f = floorf(ys);
    const float fx = xs - x0f, fy = ys - y0f;
    const int x0 = aug_floor_index(x0f), y0 = aug_floor_index(y0f);
    const float v00 = aug_tap<REFLECT>(p, sh, sw, y0, x0, H, W), v01 = aug_tap<REFLECT>(p, sh, sw, y0, x0 + 1, H, W);
    const float v10 = aug_tap<REFLECT>(p, sh, sw, y0 + 1, x0, H, W), v11 = aug_tap<REFLECT>(p, sh, sw, y0 + 1, x0 + 1, H, W);
    const float top = v00 * (1.f - fx) + v01 * fx, bot = v10 * (1.f - fx) + v11 * fx;
    return top * (1.f - fy) + bot * fy;
}

__device__ __forceinline__ unsigned aug_mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float aug_noise(unsigned key, int yd, int xd, int W) {
    const unsigned n = (unsigned)yd * (unsigned)W + (unsigned)xd;
    const unsigned h0 = aug_mix32((2u * n) ^ key), h1 = aug_mix32((2u * n + 1u) ^ key);
    const float u1 = ((float)(h0 >> 9) + 0.5f) * 1.1920928955078125e-07f;          // 2^-23
    const float u2 = (float)(h1 >> 8) * 5.9604644775390625e-08f;                    // 2^-24
    return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}

__device__ __forceinline__ bool aug_is_identity(const float* A) {
    return A[0] == 1.f && A[1] == 0.f && A[2] == 0.f && A[3] == 0.f && A[4] == 1.f && A[5] == 0.f;
}

template <bool VEC> __global__ void __launch_bounds__(AUG_THREADS)
augment_triplet_kernel(AugArgs a, const float* __restrict__ params, int B, int H, int W) {
    __shared__ float s_w[AUG_MAX_C][AUG_HALO * AUG_HALO];          // the warped pose image around the tile: [c][(row + 1) * 18 + column + 1]
    const int tid = threadIdx.x;
    const int slot = blockIdx.z / B, b = blockIdx.z - slot * B;
    const int role = a.role[slot], C = a.chan[role];
    const AugSrc s = a.src[role];
    const float* __restrict__ p = params + (size_t)b * AUG_COLS;
    const int y0 = blockIdx.y * AUG_TILE, x0 = blockIdx.x * AUG_TILE;

    float A[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i] = p[(role == 0 ? 0 : 6) + i];
    const bool ident = aug_is_identity(A);
    const float* __restrict__ img = s.p + (long long)b * s.sn;

    float k[9];
    bool filt = false;          // (uniform over the workgroup: a property of the sample)
    if (role == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) { k[i] = p[12 + i]; filt = filt || k[i] != (i == 4 ? 1.f : 0.f); }
    }
    if (filt) {
        for (int r = tid; r < C * AUG_HALO * AUG_HALO; r += AUG_THREADS) {
            const int c = r / (AUG_HALO * AUG_HALO), q = r - c * (AUG_HALO * AUG_HALO);
            const int i = q / AUG_HALO, j = q - i * AUG_HALO;
            s_w[c][q] = aug_warp<true>(img + c * s.sc, s.sh, s.sw, A, ident, y0 + i - 1, x0 + j - 1, H, W);
        }
        __syncthreads();
    }

    // lane -> (channel, row, quad)
    const int c = tid >> 6, r = (tid >> 2) & (AUG_TILE - 1), q = tid & 3;
    const int yd = y0 + r, xq = x0 + 4 * q;
    if (c >= C || yd >= H || xq >= W) return;
    const float* __restrict__ plane = img + c * s.sc;
    float v[4];
    if (role == 0) {
        const float mul = p[21], add = c < 3 ? p[22 + c] : 0.f, alpha = p[25], gain = p[26], sigma = p[27];
        const unsigned key = (unsigned)(int)fminf(fmaxf(p[28], 0.f), 16777215.f) * 0x9E3779B9u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int xd = xq + i;
            float t;
            if (filt) {
                t = 0.f;
#pragma unroll
                for (int ii = 0; ii < 3; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 3; ++jj) t += k[3 * ii + jj] * s_w[c][(r + ii) * AUG_HALO + 4 * q + i + jj];
            } else {
                t = aug_warp<true>(plane, s.sh, s.sw, A, ident, yd, xd, H, W);
            }
            if (mul != 1.f) t = t * mul;
            if (add != 0.f) t = t + add;
            if (alpha != 1.f) t = 0.5f + alpha * (t - 0.5f);
            if (gain != 0.f) t = 1.f / (1.f + expf(gain * (0.5f - t)));
            if (sigma != 0.f) t = t + sigma * aug_noise(key, yd, xd, W);
            v[i] = fminf(fmaxf(t, 0.f), 1.f);
        }
    } else if (role == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = aug_warp<true>(plane, s.sh, s.sw, A, ident, yd, xq + i, H, W);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = aug_warp<false>(plane, s.sh, s.sw, A, ident, yd, xq + i, H, W);
    }

    float* o = a.out[role] + (((size_t)b * C + c) * H + yd) * (size_t)W + xq;
    if (VEC) {          // W % 4 == 0: the quad is whole and 16-byte aligned
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (xq + i < W) o[i] = v[i];
    }
}

extern "C" int lp_augment_triplet(const float* pose, const long long* pose_strides, const float* target, const long long* target_strides,
                                  const float* segm, const long long* segm_strides, const float* params, int B, int C, int Cs, int H, int W,
                                  float* pose_out, float* target_out, float* segm_out, void* stream) {
    if (!pose || !pose_strides || !params || !pose_out) return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: null pointer");
    if ((target != nullptr) != (target_strides != nullptr) || (target != nullptr) != (target_out != nullptr))
        return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: null pointer (target, its strides and its output are given or omitted together)");
    if ((segm != nullptr) != (segm_strides != nullptr) || (segm != nullptr) != (segm_out != nullptr))
        return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: null pointer (segm, its strides and its output are given or omitted together)");
    if (B < 1) return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: B >= 1 is required");
    if (C < 1 || C > AUG_MAX_C) return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: C must be in 1 .. 4");
    if (segm && (Cs < 1 || Cs > AUG_MAX_C)) return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: Cs must be in 1 .. 4");
    if (H < 1 || W < 1) return lp_set_error(LP_ERR_ARG, "lp_augment_triplet: H >= 1 and W >= 1 are required");
    AugArgs a = {};
    int roles = 0;
    a.src[0] = {pose, pose_strides[0], pose_strides[1], pose_strides[2], pose_strides[3]};
    a.out[0] = pose_out; a.chan[0] = C; a.role[roles++] = 0;
    if (target) {
        a.src[1] = {target, target_strides[0], target_strides[1], target_strides[2], target_strides[3]};
        a.out[1] = target_out; a.chan[1] = C; a.role[roles++] = 1;
    }
    if (segm) {
        a.src[2] = {segm, segm_strides[0], segm_strides[1], segm_strides[2], segm_strides[3]};
        a.out[2] = segm_out; a.chan[2] = Cs; a.role[roles++] = 2;
    }
    const long long tiles_x = ((long long)W + AUG_TILE - 1) / AUG_TILE, tiles_y = ((long long)H + AUG_TILE - 1) / AUG_TILE;
    if (tiles_x > 0x7fffffffLL || tiles_y > 65535 || (long long)roles * B > 65535)
        return lp_set_error(LP_ERR_UNSUPPORTED, "lp_augment_triplet: B or H x W exceeds one launch grid");
    const bool vec = W % 4 == 0 && (((uintptr_t)pose_out | (uintptr_t)target_out | (uintptr_t)segm_out) & 15) == 0;
    const dim3 grid((unsigned)tiles_x, (unsigned)tiles_y, (unsigned)(roles * B)), block(AUG_THREADS);
    if (vec) hipLaunchKernelGGL(augment_triplet_kernel<true>, grid, block, 0, (hipStream_t)stream, a, params, B, H, W);
    else hipLaunchKernelGGL(augment_triplet_kernel<false>, grid, block, 0, (hipStream_t)stream, a, params, B, H, W);
    return lp_check_launch("augment_triplet");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
