// Kernels of the stickman-to-image generator (generators/FSTH.py) that the AdaIN decoder did not have yet:
//   * the plain tanh head: fake_rgbs = tanh(z[..., :3]) as an NHWC -> NCHW transpose, and its backward -- lp_head_fwd/bwd without the mask composition;
//   * the reduction of the per-sample (dgamma, dbeta) rows that lp_adain_relu_bwd(_planes) writes to the batch-shared gradient of an
//     nn.InstanceNorm2d(affine=True).
// All three are streaming kernels: one pass over their operands, plain C++.
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

namespace {
inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
}

// one thread per pixel: the pixel's Cz floats in (one 16-byte load for Cz = 4), three planes out (each coalesced over the pixels)
template <int CZ> __global__ void tanh_head_fwd_kernel(const float* __restrict__ z, float* __restrict__ t, float* __restrict__ rgbs, int N, int HW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N * HW) return;
    const int n = (int)(i / HW), pix = (int)(i % HW);
    float v0, v1, v2;
    if (CZ == 4) { const float4 zv = ((const float4*)z)[i]; v0 = zv.x; v1 = zv.y; v2 = zv.z; }
    else { const float* zp = z + i * 3; v0 = zp[0]; v1 = zp[1]; v2 = zp[2]; }
    const float t0 = tanhf(v0), t1 = tanhf(v1), t2 = tanhf(v2);
    if (t) {
        if (CZ == 4) { float4 tv; tv.x = t0; tv.y = t1; tv.z = t2; tv.w = 0.f; ((float4*)t)[i] = tv; }      // (the padding channel carries no value)
        else { float* tp = t + i * 3; tp[0] = t0; tp[1] = t1; tp[2] = t2; }
    }
    float* r = rgbs + (size_t)n * 3 * HW + pix;
    r[0] = t0; r[HW] = t1; r[2 * (size_t)HW] = t2;
}

template <int CZ> __global__ void tanh_head_bwd_kernel(const float* __restrict__ t, const float* __restrict__ d_rgbs, float* __restrict__ dz, int N, int HW,
                                                        float* __restrict__ amax) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float am = 0.f;
    if (i < (long long)N * HW) {
        const int n = (int)(i / HW), pix = (int)(i % HW);
        float t0, t1, t2;
        if (CZ == 4) { const float4 tv = ((const float4*)t)[i]; t0 = tv.x; t1 = tv.y; t2 = tv.z; }
        else { const float* tp = t + i * 3; t0 = tp[0]; t1 = tp[1]; t2 = tp[2]; }
        const float* dr = d_rgbs + (size_t)n * 3 * HW + pix;
        float4 o;
        o.x = dr[0] * (1.f - t0 * t0);
        o.y = dr[HW] * (1.f - t1 * t1);
        o.z = dr[2 * (size_t)HW] * (1.f - t2 * t2);
        o.w = 0.f;                                                                      // padding channel: an exact zero
        if (CZ == 4) ((float4*)dz)[i] = o;
        else { float* dp = dz + i * 3; dp[0] = o.x; dp[1] = o.y; dp[2] = o.z; }
        am = lp_amax4(0.f, o);
    }
    if (amax) lp_amax_commit(am, amax, blockIdx.x);       // (all lanes: the wave reduction is a cross-lane shuffle)
}

extern "C" int lp_tanh_head_fwd(const float* z, float* t, float* fake_rgbs, int N, int H, int W, int Cz, void* stream) {
    if (!z || !fake_rgbs) return lp_set_error(LP_ERR_ARG, "lp_tanh_head_fwd: null pointer");
    if (Cz != 3 && Cz != 4) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_tanh_head_fwd: Cz must be 3 or 4 (RGB, or RGB + one padding channel)");
    if (N < 1 || H < 1 || W < 1) return lp_set_error(LP_ERR_ARG, "lp_tanh_head_fwd: empty tensor");
    const long long total = (long long)N * H * W;
    if (Cz == 4) hipLaunchKernelGGL(tanh_head_fwd_kernel<4>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, z, t, fake_rgbs, N, H * W);
    else hipLaunchKernelGGL(tanh_head_fwd_kernel<3>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, z, t, fake_rgbs, N, H * W);
    return lp_check_launch("tanh_head_fwd");
}

extern "C" int lp_tanh_head_bwd(const float* t, const float* d_rgbs, float* dz, int N, int H, int W, int Cz, float* amax_slots, void* stream) {
    if (!t || !d_rgbs || !dz) return lp_set_error(LP_ERR_ARG, "lp_tanh_head_bwd: null pointer");
    if (Cz != 3 && Cz != 4) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_tanh_head_bwd: Cz must be 3 or 4 (RGB, or RGB + one padding channel)");
    if (N < 1 || H < 1 || W < 1) return lp_set_error(LP_ERR_ARG, "lp_tanh_head_bwd: empty tensor");
    const long long total = (long long)N * H * W;
    if (Cz == 4) hipLaunchKernelGGL(tanh_head_bwd_kernel<4>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, t, d_rgbs, dz, N, H * W, amax_slots);
    else hipLaunchKernelGGL(tanh_head_bwd_kernel<3>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, t, d_rgbs, dz, N, H * W, amax_slots);
    return lp_check_launch("tanh_head_bwd");
}

// thread j < C: gamma channel j; C <= j < 2C: beta channel j - C.  The N rows are added in the order 0 .. N-1 by ONE thread per channel, so the
// sum does not depend on the launch geometry or on timing: two runs give the same bits.
__global__ void norm_affine_grad_kernel(const float* __restrict__ dgamma, const float* __restrict__ dbeta, int ab_stride, float* __restrict__ out_gamma,
                                        float* __restrict__ out_beta, int N, int C, int accumulate) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 2 * C) return;
    const int c = j < C ? j : j - C;
    const float* src = (j < C ? dgamma : dbeta) + c;
    float* dst = (j < C ? out_gamma : out_beta) + c;
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += src[(size_t)n * ab_stride];
    *dst = accumulate ? *dst + s : s;
}

extern "C" int lp_norm_affine_grad(const float* dgamma, const float* dbeta, int ab_stride, float* out_gamma, float* out_beta, int N, int C,
                                   int accumulate, void* stream) {
    if (!dgamma || !dbeta || !out_gamma || !out_beta) return lp_set_error(LP_ERR_ARG, "lp_norm_affine_grad: null pointer");
    if (N < 1 || C < 1 || ab_stride < C) return lp_set_error(LP_ERR_ARG, "lp_norm_affine_grad: N, C >= 1 and a row stride >= C are required");
    hipLaunchKernelGGL(norm_affine_grad_kernel, dim3(cdiv(2LL * C, 256)), dim3(256), 0, (hipStream_t)stream, dgamma, dbeta, ab_stride, out_gamma, out_beta,
                       N, C, accumulate);
    return lp_check_launch("norm_affine_grad");
}
