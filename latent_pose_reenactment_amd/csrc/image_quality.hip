// Image-quality table of a batch: SSIM, PSNR and L1 between two images, whole-frame and weighted by a foreground mask, from ONE pass over the pixels.
//
// Definition (restated in fp64 by tests/image_quality_restatement.py).  x, y: logical B x C x H x W fp32 with any strides, C <= 4, H, W >= 11;
// m (optional): B x H x W fp32 with any strides (a stride-0 expand included), used as given.  xh = clamp(x, 0, 1), yh = clamp(y, 0, 1), d = xh - yh.
// Per image:
//   l1   = mean |d|                         mse = mean d^2                    psnr = -10 log10(max(mse, 1e-10))   (identical images: 100 dB, not inf)
//   ssim = mean over channels and the (H - 10) x (W - 10) "valid" window positions (no padding) of
//            S = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),   C1 = 1e-4, C2 = 9e-4,
//          with f(.) the separable 11-tap Gaussian window (sigma 1.5, taps normalised to sum 1) and
//            mx = f(xh), my = f(yh), sxx = f(xh^2) - mx^2, syy = f(yh^2) - my^2, sxy = f(xh yh) - mx my
//   l1_fg = sum m |d| / (C sum m)           mse_fg = sum m d^2 / (C sum m)    psnr_fg = the psnr formula on mse_fg
//   ssim_fg = sum m_c S / (C sum m_c),  m_c = m at the window's centre pixel (h + 5, w + 5)
//   a weight sum of 0 gives NaN (0 / 0) in the columns that divide by it; without a mask the three _fg columns are NaN.
// out [B][6] = ssim, psnr, l1, ssim_fg, psnr_fg, l1_fg.
//
// One workgroup = one image x one 16 x 16 tile of window positions.  It stages the 26 x 26 patch of xh and yh (all channels) and of m in LDS once,
// then per channel runs the horizontal 11-tap pass over the five products (26 rows x 16 columns, into LDS) and the vertical pass (one window position
// per lane), forms S and accumulates.  The L1 / squared-error sums are taken while staging, every pixel by the one tile that owns it (a tile owns the
// first 16 rows / columns of its patch; the last tile of a row / column owns the rest).  The second moments are taken about a per-tile, per-channel
// pivot (the clamped pixel at the patch centre): f((x - p)^2) - f(x - p)^2 is the same variance without the cancellation of f(x^2) - mx^2 -- on a flat
// image every term is exactly 0.  The window taps are rounded from fp64 on the host and arrive as kernel arguments.
// Eight partial sums per workgroup go to the workspace; the finish kernel (one workgroup per image) adds them in a fixed order and writes the six
// columns.  No atomics, no fences: the table is a pure function of the inputs, bit-identical from run to run.  fp32 throughout.
#include <math.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file: two images times one broadcast tap is the "pair times a scalar" shape for which hipcc picks
// v_pk_*_f32 with op_sel:[0,1] (wrong beside the LDS-DMA convolution kernels on gfx950: tests/test_isa_lint.py, spectral_norm.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define IQ_TILE 16                          // window positions per tile side
#define IQ_TAPS 11
#define IQ_PATCH (IQ_TILE + IQ_TAPS - 1)    // 26
#define IQ_PIX (IQ_PATCH * IQ_PATCH)        // 676
#define IQ_THREADS 256                      // = IQ_TILE * IQ_TILE: one window position per lane in the vertical pass
#define IQ_MAX_C 4
#define IQ_PART 8                           // partial sums per workgroup: S, m_c S, d^2, |d|, m d^2, m |d|, m (owned pixels), m_c (windows)

struct IqSrc { const float* p; long long sn, sc, sh, sw; };
struct IqTaps { float g[IQ_TAPS]; };

__device__ __forceinline__ float iq_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// S of one window from the pivoted moments.  Every product and sum is rounded on its own (no contraction), so that two identical images give
// numerator == denominator bit for bit and S == 1 exactly.
__device__ __forceinline__ float iq_ssim_term(float fx, float fy, float exx, float eyy, float exy, float px, float py) {
#pragma clang fp contract(off)
    const float mx = fx + px, my = fy + py;
    const float sxx = exx - fx * fx, syy = eyy - fy * fy, sxy = exy - fx * fy;
    const float mxy = mx * my;
    const float n1 = (mxy + mxy) + 1e-4f, d1 = (mx * mx + my * my) + 1e-4f;
    const float n2 = (sxy + sxy) + 9e-4f, d2 = (sxx + syy) + 9e-4f;
    return (n1 * n2) / (d1 * d2);
}

template <bool MASK> __global__ void __launch_bounds__(IQ_THREADS)
image_quality_kernel(IqSrc x, IqSrc y, IqSrc m, int C, int H, int W, int tiles_x, int tiles_y, IqTaps taps, float* __restrict__ part) {
    __shared__ float s_x[IQ_MAX_C][IQ_PIX];           // xh - pivot
    __shared__ float s_y[IQ_MAX_C][IQ_PIX];
    __shared__ float s_m[IQ_PIX];
    __shared__ float s_h[5][IQ_PATCH * IQ_TILE];      // horizontal pass of x, y, x^2, y^2, x y: [patch row][window column]
    __shared__ float s_red[IQ_THREADS / 64][IQ_PART];
    const int tid = threadIdx.x;
    const int tiles = tiles_x * tiles_y;
    const int b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int h0 = ty * IQ_TILE, w0 = tx * IQ_TILE;
    const int oh = min(IQ_TILE, H - (IQ_TAPS - 1) - h0), ow = min(IQ_TILE, W - (IQ_TAPS - 1) - w0);          // live window positions (>= 1)
    const int ph = oh + IQ_TAPS - 1, pw = ow + IQ_TAPS - 1;                                                  // live patch: h0 + ph <= H, w0 + pw <= W
    const int own_h = ty == tiles_y - 1 ? ph : IQ_TILE, own_w = tx == tiles_x - 1 ? pw : IQ_TILE;            // pixels whose L1 / mse terms this tile adds

    const float* xb = x.p + (long long)b * x.sn + (long long)h0 * x.sh + (long long)w0 * x.sw;
    const float* yb = y.p + (long long)b * y.sn + (long long)h0 * y.sh + (long long)w0 * y.sw;
    float px[IQ_MAX_C], py[IQ_MAX_C];
#pragma unroll
    for (int c = 0; c < IQ_MAX_C; ++c) {
        px[c] = py[c] = 0.f;
        if (c < C) {
            px[c] = iq_clamp01(xb[c * x.sc + (ph >> 1) * x.sh + (pw >> 1) * x.sw]);
            py[c] = iq_clamp01(yb[c * y.sc + (ph >> 1) * y.sh + (pw >> 1) * y.sw]);
        }
    }

    float a_s = 0.f, a_ms = 0.f, a_sq = 0.f, a_abs = 0.f, a_msq = 0.f, a_mabs = 0.f, a_m = 0.f, a_mc = 0.f;
    for (int r = tid; r < IQ_PIX; r += IQ_THREADS) {
        const int i = r / IQ_PATCH, j = r - i * IQ_PATCH;
        const bool live = i < ph && j < pw, own = i < own_h && j < own_w;          // (own implies live)
        float mv = 0.f;
        if (MASK) {
            if (live) mv = m.p[(long long)b * m.sn + (long long)(h0 + i) * m.sh + (long long)(w0 + j) * m.sw];
            s_m[r] = mv;
            if (own) a_m += mv;
        }
#pragma unroll
        for (int c = 0; c < IQ_MAX_C; ++c) {
            if (c < C) {
                float xv = 0.f, yv = 0.f;          // outside the live patch: the pivot itself (read by dead window positions only)
                if (live) {
                    xv = iq_clamp01(xb[c * x.sc + i * x.sh + j * x.sw]);
                    yv = iq_clamp01(yb[c * y.sc + i * y.sh + j * y.sw]);
                    if (own) {
                        const float d = xv - yv, ad = fabsf(d), sq = d * d;
                        a_abs += ad; a_sq += sq;
                        if (MASK) { a_mabs += mv * ad; a_msq += mv * sq; }
                    }
                    xv -= px[c]; yv -= py[c];
                }
                s_x[c][r] = xv; s_y[c][r] = yv;
            }
        }
    }

    const int oi = tid >> 4, oj = tid & (IQ_TILE - 1);
    const bool win = oi < oh && oj < ow;
    float mc = 0.f;
#pragma unroll
    for (int c = 0; c < IQ_MAX_C; ++c) {
        if (c < C) {
            __syncthreads();          // the patch is staged (c == 0) / the previous channel's vertical pass has read s_h
            for (int o = tid; o < IQ_PATCH * IQ_TILE; o += IQ_THREADS) {
                const int i = o >> 4, j = o & (IQ_TILE - 1);
                const float* rx = &s_x[c][i * IQ_PATCH + j];
                const float* ry = &s_y[c][i * IQ_PATCH + j];
                float hx = 0.f, hy = 0.f, hxx = 0.f, hyy = 0.f, hxy = 0.f;
#pragma unroll
                for (int k = 0; k < IQ_TAPS; ++k) {
                    const float g = taps.g[k], xv = rx[k], yv = ry[k];
                    hx += g * xv; hy += g * yv; hxx += g * (xv * xv); hyy += g * (yv * yv); hxy += g * (xv * yv);
                }
                s_h[0][o] = hx; s_h[1][o] = hy; s_h[2][o] = hxx; s_h[3][o] = hyy; s_h[4][o] = hxy;
            }
            __syncthreads();
            float fx = 0.f, fy = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
            for (int k = 0; k < IQ_TAPS; ++k) {
                const float g = taps.g[k];
                const int o = (oi + k) * IQ_TILE + oj;
                fx += g * s_h[0][o]; fy += g * s_h[1][o]; exx += g * s_h[2][o]; eyy += g * s_h[3][o]; exy += g * s_h[4][o];
            }
            if (win) {
                const float S = iq_ssim_term(fx, fy, exx, eyy, exy, px[c], py[c]);
                a_s += S;
                if (MASK) {
                    if (c == 0) { mc = s_m[(oi + (IQ_TAPS >> 1)) * IQ_PATCH + oj + (IQ_TAPS >> 1)]; a_mc += mc; }
                    a_ms += mc * S;
                }
            }
        }
    }

    float acc[IQ_PART] = {a_s, a_ms, a_sq, a_abs, a_msq, a_mabs, a_m, a_mc};
#pragma unroll
    for (int q = 0; q < IQ_PART; ++q) {
        float v = acc[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) s_red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid < IQ_PART) part[(size_t)blockIdx.x * IQ_PART + tid] = (s_red[0][tid] + s_red[1][tid]) + (s_red[2][tid] + s_red[3][tid]);
}

__device__ __forceinline__ float iq_psnr(float mse) { return mse <= 1e-10f ? 100.f : -10.f * log10f(mse); }

// one workgroup per image: the tiles' partial sums in a fixed order -> the six columns
__global__ void __launch_bounds__(IQ_THREADS)
image_quality_finish_kernel(const float* __restrict__ part, int tiles, int C, int H, int W, int has_mask, float* __restrict__ out) {
    __shared__ float s_red[IQ_THREADS / 64][IQ_PART];
    const int tid = threadIdx.x, b = blockIdx.x;
    float acc[IQ_PART];
#pragma unroll
    for (int q = 0; q < IQ_PART; ++q) acc[q] = 0.f;
    for (int j = tid; j < tiles; j += IQ_THREADS) {
        const float* p = part + ((size_t)b * tiles + j) * IQ_PART;
#pragma unroll
        for (int q = 0; q < IQ_PART; ++q) acc[q] += p[q];
    }
#pragma unroll
    for (int q = 0; q < IQ_PART; ++q) {
        float v = acc[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((tid & 63) == 0) s_red[tid >> 6][q] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    float s[IQ_PART];
#pragma unroll
    for (int q = 0; q < IQ_PART; ++q) s[q] = (s_red[0][q] + s_red[1][q]) + (s_red[2][q] + s_red[3][q]);
    const float npix = (float)((long long)C * H * W), nwin = (float)((long long)C * (H - (IQ_TAPS - 1)) * (W - (IQ_TAPS - 1)));
    float* o = out + (size_t)b * 6;
    o[0] = s[0] / nwin;
    o[1] = iq_psnr(s[2] / npix);
    o[2] = s[3] / npix;
    const float nan = __int_as_float(0x7fc00000);
    if (has_mask) {
        const float wsum = (float)C * s[6];
        o[3] = s[1] / ((float)C * s[7]);
        o[4] = s[6] == 0.f ? nan : iq_psnr(s[4] / wsum);
        o[5] = s[5] / wsum;
    } else {
        o[3] = o[4] = o[5] = nan;
    }
}

static long long iq_tiles(int H, int W) {
    const long long ty = (H - (IQ_TAPS - 1) + IQ_TILE - 1) / IQ_TILE, tx = (W - (IQ_TAPS - 1) + IQ_TILE - 1) / IQ_TILE;
    return ty * tx;
}

extern "C" long long lp_image_quality_workspace_bytes(int B, int H, int W) {
    if (B < 1 || H < IQ_TAPS || W < IQ_TAPS) return 0;
    return (long long)B * iq_tiles(H, W) * IQ_PART * (long long)sizeof(float);
}

extern "C" int lp_image_quality(const float* x, const long long* stride_x, const float* y, const long long* stride_y, const float* mask,
                                const long long* stride_m, int B, int C, int H, int W, float* workspace, float* out, void* stream) {
    if (!x || !stride_x || !y || !stride_y || !workspace || !out || (mask && !stride_m)) return lp_set_error(LP_ERR_ARG, "lp_image_quality: null pointer");
    if (B < 1) return lp_set_error(LP_ERR_ARG, "lp_image_quality: B >= 1 is required");
    if (C < 1 || C > IQ_MAX_C) return lp_set_error(LP_ERR_ARG, "lp_image_quality: C must be in 1 .. 4");
    if (H < IQ_TAPS || W < IQ_TAPS) return lp_set_error(LP_ERR_ARG, "lp_image_quality: H >= 11 and W >= 11 are required (one 11 x 11 window)");
    const long long tiles = iq_tiles(H, W);
    if (tiles * B > 0x7fffffffLL) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_image_quality: B * H * W exceeds one launch grid");
    const int tiles_x = (W - (IQ_TAPS - 1) + IQ_TILE - 1) / IQ_TILE, tiles_y = (int)(tiles / tiles_x);
    const IqSrc sx = {x, stride_x[0], stride_x[1], stride_x[2], stride_x[3]}, sy = {y, stride_y[0], stride_y[1], stride_y[2], stride_y[3]};
    IqSrc sm = {nullptr, 0, 0, 0, 0};
    if (mask) sm = {mask, stride_m[0], 0, stride_m[1], stride_m[2]};
    IqTaps taps;          // Gaussian window, sigma 1.5, normalised in fp64, rounded once
    double g[IQ_TAPS], sum = 0.0;
    for (int k = 0; k < IQ_TAPS; ++k) { const double d = k - IQ_TAPS / 2; g[k] = exp(-d * d / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < IQ_TAPS; ++k) taps.g[k] = (float)(g[k] / sum);
    const dim3 grid((unsigned)(tiles * B)), block(IQ_THREADS);
    if (mask) hipLaunchKernelGGL(image_quality_kernel<true>, grid, block, 0, (hipStream_t)stream, sx, sy, sm, C, H, W, tiles_x, tiles_y, taps, workspace);
    else hipLaunchKernelGGL(image_quality_kernel<false>, grid, block, 0, (hipStream_t)stream, sx, sy, sm, C, H, W, tiles_x, tiles_y, taps, workspace);
    hipLaunchKernelGGL(image_quality_finish_kernel, dim3((unsigned)B), block, 0, (hipStream_t)stream, (const float*)workspace, (int)tiles, C, H, W,
                       mask ? 1 : 0, out);
    return lp_check_launch("image_quality");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
