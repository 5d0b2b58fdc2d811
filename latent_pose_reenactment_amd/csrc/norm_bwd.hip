// Backward of act(norm(x)) for gfx950 (fp64 restatement: tests/emu_ops.norm_act_bwd), three bandwidth-bound passes:
//   pass 1 (partial):  g = dA * activation mask; per (pixel split, channel)  S1 = sum g, S2 = sum g*xhat
//   pass 2 (finalize): dgamma = S2, dbeta = S1, coefficients of dx = ca*g + cb*x + cc
//   pass 3 (apply):    dx from g, x and the coefficients
// in two forms that share the mask, the coefficient rule, the loaders and the plane stores below:
//   * adain_bwd_*  (lp_norm_act_bwd, lp_adain_relu_bwd*): per-image statistics [N][C] (a BatchNorm over [P][C] is one image of P pixels),
//                  optional 2x2 sum of dA (x2 nearest upsample), fp32 dx (holds g between the passes), optional bf16 (hi + lo) planes
//   * bn_bwd16_*   (lp_bn_bwd16, lp_bn_bwd16_h): per-channel statistics [C], dx written STRAIGHT to operand planes, g recomputed in pass 3
// mask_mode 0: the activation's own pattern 0 < x*scale+shift < act_hi (ReLU: act_hi = inf; ReLU6: 6);  1: no mask (a plain norm);
// 2: mask_src > 0 (the ReLU sits behind a residual add: mask_src = the block output, fp32);  3: the same from a 16-bit operand plane;
// 4: the same from ONE BIT per element (bn_bwd16_* only): mask_src = bytes [P][C / 8], bit j of byte g = channel 8 g + j, as lp_bn_add_act_bits
// writes them from the HI plane it stores (mode 3's predicate, evaluated once in the forward).
// X16: x is a 16-BIT-RESIDENT conv output (the unscaled fp16 plane the conv epilogue left instead of fp32 y; C % 8 == 0).
#include "lp_common.h"
#include "lp_hip.h"
#include "lp_internal.h"

// ------------------------------------------------------------------------------------------------------------------
// shared pieces
// ------------------------------------------------------------------------------------------------------------------
// g *= activation mask, W (4 | 8) consecutive channels at element offset off; a, b: scale / shift of these channels.  A 16-bit
// plane element is > 0  <=>  sign clear and magnitude non-zero.
template <int W>
__device__ __forceinline__ void norm_mask(float (&g)[W], const float (&xs)[W], const float* a, const float* b, int mask_mode, float act_hi,
                                          const void* mask_src, size_t off) {
    typedef short __attribute__((ext_vector_type(W))) s16xw_t;
    if (mask_mode == 2) {
#pragma unroll
        for (int q = 0; q < W; q += 4) {
            const float4 m = *(const float4*)((const float*)mask_src + off + q);
            g[q] = m.x > 0.f ? g[q] : 0.f; g[q + 1] = m.y > 0.f ? g[q + 1] : 0.f; g[q + 2] = m.z > 0.f ? g[q + 2] : 0.f; g[q + 3] = m.w > 0.f ? g[q + 3] : 0.f;
        }
    } else if (mask_mode == 3) {
        const s16xw_t m = *(const s16xw_t*)((const uint16_t*)mask_src + off);
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] = ((unsigned)((uint16_t)m[j]) - 1u) < 0x7fffu ? g[j] : 0.f;
    } else if (mask_mode == 4) {            // (off % W == 0 and C % 8 == 0: W = 4 reads the low or the high nibble of its group's byte)
        const unsigned m = (unsigned)((const unsigned char*)mask_src)[off >> 3] >> (W == 4 ? (unsigned)(off & 4) : 0u);
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] = ((m >> j) & 1u) ? g[j] : 0.f;
    } else if (mask_mode == 0) {
#pragma unroll
        for (int j = 0; j < W; ++j) { const float t = fmaf(xs[j], a[j], b[j]); g[j] = (t > 0.f && t < act_hi) ? g[j] : 0.f; }
    }
}

// fp64 merge of the S split partials of one (image, channel) by one wave (lane 0 holds the result): K floats per partial,
// {S1, S2} or {S1, S2, max|g|, max|xhat|}; q = the channel's partial of split 0, `step` floats from one split to the next
struct NormBwdSums { float S1, S2, gm, xm; };
template <int K> __device__ __forceinline__ NormBwdSums norm_bwd_merge(const float* q, size_t step, int S, int lane) {
    double a1 = 0, a2 = 0;
    float gm = 0.f, xm = 0.f;
    for (int s = lane; s < S; s += 64) {
        const float* e = q + s * step;
        a1 += e[0]; a2 += e[1];
        if (K == 4) { gm = fmaxf(gm, e[2]); xm = fmaxf(xm, e[3]); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        a1 += __shfl_down(a1, o, 64); a2 += __shfl_down(a2, o, 64);
        if (K == 4) { gm = fmaxf(gm, __shfl_down(gm, o, 64)); xm = fmaxf(xm, __shfl_down(xm, o, 64)); }
    }
    return {(float)a1, (float)a2, gm, xm};
}

// dx = ca*g + cb*x + cc over P pixels (inv_p = 1/P) -> coef[0..3); returns ca.  frozen: the statistics are constants (running
// statistics, eval mode)
__device__ __forceinline__ float norm_bwd_coef(float gamma, float r, float m, float S1, float S2, float inv_p, int frozen, float* coef) {
    const float ca = gamma * r;
    const float cb = frozen ? 0.f : -ca * r * S2 * inv_p;
    const float cc = frozen ? 0.f : -ca * S1 * inv_p - cb * m;
    coef[0] = ca; coef[1] = cb; coef[2] = cc;
    return ca;
}

// ------------------------------------------------------------------------------------------------------------------
// per-image form: backward of relu(AdaIN(x)) [+ x2 nearest upsample] / act(BatchNorm(x)) with fp32 dx
//   pass 1 writes g = sum2x2?(dA) * mask into dx (as temporary); g_copy (|NULL): g is also written there (the identity branch of
//   the residual block receives exactly that)
// ------------------------------------------------------------------------------------------------------------------
template <bool X16>
__global__ __launch_bounds__(256) void adain_bwd_partial_kernel(const float* __restrict__ dA, const void* __restrict__ x,
                                                                const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                                float* __restrict__ g_out, float* __restrict__ part, int H, int W, int C,
                                                                int ups, int S, int PB, int mask_mode, const float* __restrict__ mask_src,
                                                                float* __restrict__ g_copy, float act_hi) {
    __shared__ float sh[2][16][64];
    const int n = blockIdx.z, cb = blockIdx.y, s = blockIdx.x;
    const int cq = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = cb * 64 + cq * 4;
    const int HW = H * W;
    const int p0 = s * PB, p1 = min(HW, p0 + PB);
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    if (c < C) {                                       // C % 4 == 0 required (checked on host)
        const float4 mu = *(const float4*)(mean + (size_t)n * C + c), rs = *(const float4*)(rstd + (size_t)n * C + c);
        const float4 sc = *(const float4*)(scale + (size_t)n * C + c), sf = *(const float4*)(shift + (size_t)n * C + c);
        const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, r4[4] = {rs.x, rs.y, rs.z, rs.w}, a4[4] = {sc.x, sc.y, sc.z, sc.w}, b4[4] = {sf.x, sf.y, sf.z, sf.w};
#pragma unroll 2
        for (int pix = p0 + pl; pix < p1; pix += 16) {
            const size_t e = ((size_t)n * HW + pix) * C + c;
            const float4 xv = lp_ldx4<X16>(x, e);
            float4 gv;
            if (ups) {
                int yy = pix / W, xx = pix % W;
                const float* b = dA + (((size_t)n * 2 * H + 2 * yy) * 2 * W + 2 * xx) * C + c;
                float4 a0 = *(const float4*)b, a1 = *(const float4*)(b + C), a2 = *(const float4*)(b + (size_t)2 * W * C),
                       a3 = *(const float4*)(b + (size_t)2 * W * C + C);
                gv.x = (a0.x + a1.x) + (a2.x + a3.x); gv.y = (a0.y + a1.y) + (a2.y + a3.y);
                gv.z = (a0.z + a1.z) + (a2.z + a3.z); gv.w = (a0.w + a1.w) + (a2.w + a3.w);
            } else gv = *(const float4*)(dA + e);
            float g[4] = {gv.x, gv.y, gv.z, gv.w};
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
            norm_mask<4>(g, xs, a4, b4, mask_mode, act_hi, mask_src, e);
            gv = make_float4(g[0], g[1], g[2], g[3]);
            *(float4*)(g_out + e) = gv;
            if (g_copy) *(float4*)(g_copy + e) = gv;
#pragma unroll
            for (int j = 0; j < 4; ++j) { s1[j] += g[j]; s2[j] += g[j] * ((xs[j] - m4[j]) * r4[j]); }
        }
    }
    for (int j = 0; j < 4; ++j) { sh[0][pl][cq * 4 + j] = s1[j]; sh[1][pl][cq * 4 + j] = s2[j]; }
    __syncthreads();
    if (threadIdx.x < 128) {
        int which = threadIdx.x >> 6, ch = threadIdx.x & 63;
        float a = 0.f;
        for (int k = 0; k < 16; ++k) a += sh[which][k][ch];
        int cg = cb * 64 + ch;
        if (cg < C) part[(((size_t)n * S + s) * C + cg) * 2 + which] = a;
    }
}

__global__ __launch_bounds__(256) void adain_bwd_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma, int ab_stride,
                                          const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dgamma,
                                          float* __restrict__ dbeta, float* __restrict__ coef, int N, int C, int S, float inv_hw, int frozen) {
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;          // one wave per (n, c)
    if (idx >= N * C) return;
    int n = idx / C, c = idx % C;
    const NormBwdSums t = norm_bwd_merge<2>(part + ((size_t)n * S * C + c) * 2, (size_t)C * 2, S, lane);
    if (lane != 0) return;
    if (dgamma) dgamma[(size_t)n * ab_stride + c] = t.S2;
    if (dbeta) dbeta[(size_t)n * ab_stride + c] = t.S1;
    norm_bwd_coef(gamma ? gamma[(size_t)n * ab_stride + c] : 1.f, rstd[idx], mean[idx], t.S1, t.S2, inv_hw, frozen, coef + (size_t)idx * 3);
}

// o_hi (, o_lo) | NULL: the result ALSO goes out as bf16 (hi + lo) operand planes [N][HW][C] (C % 8 == 0) -- what lp_act_pack(grad) would write in
// the bf16 / bf16x3 modes (no gradient scale there) -- and with keep_dx == 0 ONLY as planes (the generator's backward in its bf16x3 default;
// a conv's gradient operand then costs no fp32 round trip and no pack launch)
template <bool X16>
__global__ void adain_bwd_apply_kernel(float* __restrict__ dx /* holds g */, const void* __restrict__ x, const float* __restrict__ add,
                                       const float* __restrict__ coef, long long total4, int HW, int C, float* __restrict__ amax,
                                       uint16_t* __restrict__ o_hi, uint16_t* __restrict__ o_lo, int keep_dx) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int C4 = C >> 2;
    float am = 0.f;
    for (; i < total4; i += stride) {
        int c = (int)(i % C4) * 4;
        int n = (int)(i / ((long long)C4 * HW));
        const float* cf = coef + ((size_t)n * C + c) * 3;
        float4 g = ((const float4*)dx)[i], xv = lp_ldx4<X16>(x, (size_t)i * 4), o;
        o.x = fmaf(cf[0], g.x, fmaf(cf[1], xv.x, cf[2]));
        o.y = fmaf(cf[3], g.y, fmaf(cf[4], xv.y, cf[5]));
        o.z = fmaf(cf[6], g.z, fmaf(cf[7], xv.z, cf[8]));
        o.w = fmaf(cf[9], g.w, fmaf(cf[10], xv.w, cf[11]));
        if (add) { float4 a = ((const float4*)add)[i]; o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w; }
        if (keep_dx) ((float4*)dx)[i] = o;
        if (o_hi) lp_store_bf16_planes4(o, o_hi, o_lo, (size_t)i * 4);
        am = lp_amax4(am, o);
    }
    if (amax) lp_amax_commit(am, amax, blockIdx.x);
}

extern "C" long long lp_adain_bwd_workspace_bytes(int N, int HW, int C) {
    const int PB = lp_stat_split_pix(N, HW, C);
    long long S = (HW + PB - 1) / PB;
    return (long long)N * S * C * 2 * 4 + (long long)N * C * 3 * 4;
}

struct NormActBwdParams {
    const float* dA; const void* x; const float* add; const float* gamma; int ab_stride;
    const float* mean; const float* rstd; const float* scale; const float* shift;
    float* dx; float* dgamma; float* dbeta; float* workspace;
    int N, H, W, C, upsample;
    int x16 = 0;                                                        // x is an fp16 plane
    int mask_mode = 0; const float* mask_src = nullptr; float* g_copy = nullptr; float act_hi = 0.f; int frozen_stats = 0;
    float* amax_slots = nullptr;
    uint16_t* o_hi = nullptr; uint16_t* o_lo = nullptr; int keep_dx = 1;
    void* stream;
};

template <bool X16> static int norm_act_bwd_launch(const NormActBwdParams& p) {
    const int HW = p.H * p.W;
    const int PB = lp_stat_split_pix(p.N, HW, p.C);
    int S = (HW + PB - 1) / PB;
    float* part = p.workspace;
    float* coef = p.workspace + (size_t)p.N * S * p.C * 2;
    hipStream_t st = (hipStream_t)p.stream;
    hipLaunchKernelGGL(adain_bwd_partial_kernel<X16>, dim3(S, (p.C + 63) / 64, p.N), dim3(256), 0, st, p.dA, p.x, p.mean, p.rstd, p.scale, p.shift,
                       p.dx, part, p.H, p.W, p.C, p.upsample, S, PB, p.mask_mode, p.mask_src, p.g_copy, p.act_hi > 0.f ? p.act_hi : 3.0e38f);
    int rc = lp_check_launch("adain_bwd_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(adain_bwd_finalize_kernel, dim3((unsigned)(((long long)p.N * p.C + 3) / 4)), dim3(256), 0, st, part, p.gamma, p.ab_stride,
                       p.mean, p.rstd, p.dgamma, p.dbeta, coef, p.N, p.C, S, 1.0f / (float)HW, p.frozen_stats);
    rc = lp_check_launch("adain_bwd_finalize");
    if (rc) return rc;
    long long total4 = (long long)p.N * HW * p.C / 4;
    int blocks = (int)((total4 + 255) / 256); if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(adain_bwd_apply_kernel<X16>, dim3(blocks), dim3(256), 0, st, p.dx, p.x, p.add, coef, total4, HW, p.C, p.amax_slots,
                       p.o_hi, p.o_lo, p.keep_dx);
    return lp_check_launch("adain_bwd_apply");
}

static int norm_act_bwd_impl(const NormActBwdParams& p) {
    if (!p.dA || !p.x || !p.mean || !p.rstd || !p.scale || !p.shift || !p.dx || !p.workspace) return lp_set_error(LP_ERR_ARG, "lp_norm_act_bwd: null pointer");
    if (p.C & 3) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_norm_act_bwd: C must be a multiple of 4");
    if (p.mask_mode < 0 || p.mask_mode > 2 || (p.mask_mode == 2 && !p.mask_src)) return lp_set_error(LP_ERR_ARG, "lp_norm_act_bwd: bad mask mode");
    if ((long long)p.H * p.W >= (1ll << 30)) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_norm_act_bwd: H*W < 2^30");
    return p.x16 ? norm_act_bwd_launch<true>(p) : norm_act_bwd_launch<false>(p);
}

extern "C" int lp_norm_act_bwd(const float* dA, const float* x, const float* add, const float* gamma, int ab_stride, const float* mean,
                               const float* rstd, const float* scale, const float* shift, float* dx, float* dgamma, float* dbeta,
                               float* workspace, int N, int H, int W, int C, int upsample, int mask_mode, const float* mask_src,
                               float* g_copy, float act_hi, int frozen_stats, float* amax_slots, void* stream) {
    NormActBwdParams p;
    p.dA = dA; p.x = x; p.add = add; p.gamma = gamma; p.ab_stride = ab_stride; p.mean = mean; p.rstd = rstd; p.scale = scale; p.shift = shift;
    p.dx = dx; p.dgamma = dgamma; p.dbeta = dbeta; p.workspace = workspace; p.N = N; p.H = H; p.W = W; p.C = C; p.upsample = upsample;
    p.mask_mode = mask_mode; p.mask_src = mask_src; p.g_copy = g_copy; p.act_hi = act_hi; p.frozen_stats = frozen_stats;
    p.amax_slots = amax_slots; p.stream = stream;
    return norm_act_bwd_impl(p);
}

extern "C" int lp_adain_relu_bwd(const float* dA, const float* x, const float* add, const float* gamma, int ab_stride, const float* mean,
                                 const float* rstd, const float* scale, const float* shift, float* dx, float* dgamma, float* dbeta,
                                 float* workspace, int N, int H, int W, int C, int upsample, float* amax_slots, void* stream) {
    return lp_norm_act_bwd(dA, x, add, gamma, ab_stride, mean, rstd, scale, shift, dx, dgamma, dbeta, workspace, N, H, W, C, upsample, 0,
                           nullptr, nullptr, 0.f, 0, amax_slots, stream);
}

// lp_adain_relu_bwd whose result goes out as bf16 (out_lo == NULL) / bf16 hi + lo operand planes [N][H][W][C] (C % 8 == 0) -- the gradient operand
// of the conv below, in the bf16 / bf16x3 modes (no gradient scale) -- and, with keep_dx != 0, also as fp32 dx.  dx must always be given: it holds
// the masked gradient between the passes.
extern "C" int lp_adain_relu_bwd_planes(const float* dA, const float* x, const float* add, const float* gamma, int ab_stride, const float* mean,
                                        const float* rstd, const float* scale, const float* shift, float* dx, float* dgamma, float* dbeta,
                                        float* workspace, int N, int H, int W, int C, int upsample, uint16_t* out_hi, uint16_t* out_lo,
                                        int keep_dx, void* stream) {
    if (!out_hi) return lp_set_error(LP_ERR_ARG, "lp_adain_relu_bwd_planes: null pointer");
    if (C & 7) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_adain_relu_bwd_planes: C must be a multiple of 8");
    NormActBwdParams p;
    p.dA = dA; p.x = x; p.add = add; p.gamma = gamma; p.ab_stride = ab_stride; p.mean = mean; p.rstd = rstd; p.scale = scale; p.shift = shift;
    p.dx = dx; p.dgamma = dgamma; p.dbeta = dbeta; p.workspace = workspace; p.N = N; p.H = H; p.W = W; p.C = C; p.upsample = upsample;
    p.o_hi = out_hi; p.o_lo = out_lo; p.keep_dx = keep_dx; p.stream = stream;
    return norm_act_bwd_impl(p);
}

// lp_adain_relu_bwd with x held as a 16-bit-resident conv output (fp16 plane [N][H][W][C], C % 8 == 0): the generator's fp16 mode keeps
// no fp32 copy of its conv outputs; x-hat and the ReLU pattern are recomputed from the SAME fp16 values the forward normalised
extern "C" int lp_adain_relu_bwd16(const float* dA, const uint16_t* x16, const float* add, const float* gamma, int ab_stride, const float* mean,
                                   const float* rstd, const float* scale, const float* shift, float* dx, float* dgamma, float* dbeta,
                                   float* workspace, int N, int H, int W, int C, int upsample, float* amax_slots, void* stream) {
    if (C & 7) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_adain_relu_bwd16: C must be a multiple of 8");
    NormActBwdParams p;
    p.dA = dA; p.x = x16; p.x16 = 1; p.add = add; p.gamma = gamma; p.ab_stride = ab_stride; p.mean = mean; p.rstd = rstd; p.scale = scale; p.shift = shift;
    p.dx = dx; p.dgamma = dgamma; p.dbeta = dbeta; p.workspace = workspace; p.N = N; p.H = H; p.W = W; p.C = C; p.upsample = upsample;
    p.amax_slots = amax_slots; p.stream = stream;
    return norm_act_bwd_impl(p);
}

// ------------------------------------------------------------------------------------------------------------------
// per-channel form straight to operand planes
// The embedder's conv -> BatchNorm -> ReLU chains only ever consume the BatchNorm input gradient dy as the 16-bit operand of the weight /
// data gradient contractions, so it is never written in fp32:
//   pass 1 (partial):  also max|g|, max|xhat| per (pixel split, channel); g is recomputed in pass 3, not stored
//   pass 2 (finalize): also a per-channel BOUND of |dy|  (|ca| * (max|g| + |S1|/P + max|xhat| * |S2|/P)) from which the fp16 gradient scale is
//                      taken (a power of two putting the bound into [2^12, 2^13): the true amax is at most the bound, so the scaled planes
//                      cannot overflow)
//   pass 3 (apply):    recomputes g from dA and the mask, writes dy * s as operand planes (hi [, lo]); block 0 publishes {s, 1/s}
// 8 B read in pass 1 and 8 B read + 2 B written in pass 3 per element (fp16 mode), against 30 B for partial + apply + lp_act_pack on fp32 dy.
// X16: 6 B read per element and pass instead of 8 B.
// ------------------------------------------------------------------------------------------------------------------
// block reduction of pass 1: the 16 pixel lanes of each of the block's 64 channels -> part[s][c] = {S1, S2, max|g|, max|xhat|}.  Ends with no
// barrier: a second call in the same kernel needs one before it
__device__ __forceinline__ void bn_bwd16_partial_store(float (&sh)[4][16][64], const float (&s1)[4], const float (&s2)[4], const float (&gm)[4],
                                                       const float (&xm)[4], float* __restrict__ part, int s, int cb, int C) {
    const int cq = threadIdx.x & 15, pl = threadIdx.x >> 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) { sh[0][pl][cq * 4 + j] = s1[j]; sh[1][pl][cq * 4 + j] = s2[j]; sh[2][pl][cq * 4 + j] = gm[j]; sh[3][pl][cq * 4 + j] = xm[j]; }
    __syncthreads();
    const int which = threadIdx.x >> 6, ch = threadIdx.x & 63;
    float a = 0.f;
    if (which < 2) { for (int k = 0; k < 16; ++k) a += sh[which][k][ch]; }
    else { for (int k = 0; k < 16; ++k) a = fmaxf(a, sh[which][k][ch]); }
    const int cg = cb * 64 + ch;
    if (cg < C) part[((size_t)s * C + cg) * 4 + which] = a;
}

template <bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_partial_kernel(const float* __restrict__ dA, const void* __restrict__ x, const void* __restrict__ mask_src,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ scale, const float* __restrict__ shift,
                                                               float* __restrict__ part, long long P, int C, int mask_mode, float act_hi, int PB) {
    __shared__ float sh[4][16][64];
    const int cb = blockIdx.y, s = blockIdx.x;
    const int cq = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = cb * 64 + cq * 4;
    const long long p0 = (long long)s * PB, p1 = min(P, p0 + PB);
    float s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0}, gm[4] = {0, 0, 0, 0}, xm[4] = {0, 0, 0, 0};
    if (c < C) {
        const float4 mu = *(const float4*)(mean + c), rs = *(const float4*)(rstd + c);
        const float4 sc = *(const float4*)(scale + c), sf = *(const float4*)(shift + c);
        const float m4[4] = {mu.x, mu.y, mu.z, mu.w}, r4[4] = {rs.x, rs.y, rs.z, rs.w}, a4[4] = {sc.x, sc.y, sc.z, sc.w}, b4[4] = {sf.x, sf.y, sf.z, sf.w};
#pragma unroll 4
        for (long long pix = p0 + pl; pix < p1; pix += 16) {
            const float4 gv = *(const float4*)(dA + pix * C + c), xv = lp_ldx4<X16>(x, pix * C + c);
            float g[4] = {gv.x, gv.y, gv.z, gv.w};
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
            norm_mask<4>(g, xs, a4, b4, mask_mode, act_hi, mask_src, pix * C + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (xs[j] - m4[j]) * r4[j];
                s1[j] += g[j]; s2[j] = fmaf(g[j], xh, s2[j]);
                gm[j] = fmaxf(gm[j], fabsf(g[j])); xm[j] = fmaxf(xm[j], fabsf(xh));
            }
        }
    }
    bn_bwd16_partial_store(sh, s1, s2, gm, xm, part, s, cb, C);
}

// DUAL form of pass 1: two BatchNorms (a, b) that receive the SAME masked gradient g = dA * mask -- bn3 and the downsample BatchNorm of a
// residual block's first bottleneck.  dA and the mask are read once, each BN's x once; per BN the partials, the per-thread accumulation order and
// the block reduction are those of the single form, so everything downstream is bit-identical to two separate calls.  Mask modes 1 .. 4 (a
// pattern that does not depend on x).
template <bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_partial2_kernel(const float* __restrict__ dA, const void* __restrict__ xa, const void* __restrict__ xb,
                                                                const void* __restrict__ mask_src, const float* __restrict__ mean_a,
                                                                const float* __restrict__ rstd_a, const float* __restrict__ mean_b,
                                                                const float* __restrict__ rstd_b, float* __restrict__ part_a, float* __restrict__ part_b,
                                                                long long P, int C, int mask_mode, int PB) {
    __shared__ float sh[4][16][64];
    const int cb = blockIdx.y, s = blockIdx.x;
    const int cq = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int c = cb * 64 + cq * 4;
    const long long p0 = (long long)s * PB, p1 = min(P, p0 + PB);
    float s1[4] = {0, 0, 0, 0}, gm[4] = {0, 0, 0, 0};
    float s2a[4] = {0, 0, 0, 0}, xma[4] = {0, 0, 0, 0}, s2b[4] = {0, 0, 0, 0}, xmb[4] = {0, 0, 0, 0};
    if (c < C) {
        const float4 mua = *(const float4*)(mean_a + c), rsa = *(const float4*)(rstd_a + c), mub = *(const float4*)(mean_b + c), rsb = *(const float4*)(rstd_b + c);
        const float ma[4] = {mua.x, mua.y, mua.z, mua.w}, ra[4] = {rsa.x, rsa.y, rsa.z, rsa.w}, mb[4] = {mub.x, mub.y, mub.z, mub.w}, rb[4] = {rsb.x, rsb.y, rsb.z, rsb.w};
#pragma unroll 4
        for (long long pix = p0 + pl; pix < p1; pix += 16) {
            const float4 gv = *(const float4*)(dA + pix * C + c), xva = lp_ldx4<X16>(xa, pix * C + c), xvb = lp_ldx4<X16>(xb, pix * C + c);
            float g[4] = {gv.x, gv.y, gv.z, gv.w};
            const float xsa[4] = {xva.x, xva.y, xva.z, xva.w}, xsb[4] = {xvb.x, xvb.y, xvb.z, xvb.w};
            norm_mask<4>(g, xsa, ma, ma, mask_mode, 0.f, mask_src, pix * C + c);      // (modes 1 .. 4: x, scale and shift are not looked at)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xha = (xsa[j] - ma[j]) * ra[j], xhb = (xsb[j] - mb[j]) * rb[j];
                s1[j] += g[j]; gm[j] = fmaxf(gm[j], fabsf(g[j]));
                s2a[j] = fmaf(g[j], xha, s2a[j]); xma[j] = fmaxf(xma[j], fabsf(xha));
                s2b[j] = fmaf(g[j], xhb, s2b[j]); xmb[j] = fmaxf(xmb[j], fabsf(xhb));
            }
        }
    }
    bn_bwd16_partial_store(sh, s1, s2a, gm, xma, part_a, s, cb, C);
    __syncthreads();
    bn_bwd16_partial_store(sh, s1, s2b, gm, xmb, part_b, s, cb, C);
}

// one wave per channel: merges the S partials; coef[c] = {ca, cb, cc}, bound[c] >= max|dy| of the channel
__global__ __launch_bounds__(256) void bn_bwd16_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                float* __restrict__ coef, float* __restrict__ bound, int C, int S, float inv_p, int frozen) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= C) return;
    const NormBwdSums t = norm_bwd_merge<4>(part + (size_t)c * 4, (size_t)C * 4, S, lane);
    if (lane != 0) return;
    dgamma[c] = t.S2; dbeta[c] = t.S1;
    const float ca = norm_bwd_coef(gamma[c], rstd[c], mean[c], t.S1, t.S2, inv_p, frozen, coef + c * 3);
    bound[c] = frozen ? fabsf(ca) * t.gm : fabsf(ca) * (t.gm + fabsf(t.S1) * inv_p + t.xm * fabsf(t.S2) * inv_p);
}

// prologue of pass 3: in fp16 mode every block derives the same power-of-two scale from the per-channel bounds (C floats, L2 resident);
// block 0 publishes {s, 1/s} ({1, 1} in the bf16 modes).  Returns s.
template <bool F16> __device__ __forceinline__ float bn_bwd16_out_scale(const float* bound, int C, float* out_scale) {
    float sc_out = 1.f, inv = 1.f;
    if (F16) {
        __shared__ float shm[4];
        float m = 0.f;
        for (int j = threadIdx.x; j < C; j += 256) m = fmaxf(m, bound[j]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o, 64));
        if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
        amax_to_scale(m, sc_out, inv);
    }
    if (out_scale && blockIdx.x == 0 && threadIdx.x == 0) { out_scale[0] = sc_out; out_scale[1] = inv; }
    return sc_out;
}

// pass 3 for 8 consecutive channels at element offset off: cf = their 24 coefficients {ca, cb, cc}, a / b = their scale / shift,
// planes = dy * post.  g_out (|NULL): the masked incoming gradient itself (what the identity branch of a residual block receives).
template <int PREC, bool X16>
__device__ __forceinline__ void bn_bwd16_apply_item(const float* dA, const void* x, const void* mask_src,
                                                    const float* a, const float* b, const float* cf, float post, uint16_t* hi,
                                                    uint16_t* lo, float* g_out, size_t off, int mask_mode, float act_hi) {
    constexpr bool SPLIT = (PREC == LP_PREC_BF16X3), F16 = (PREC == LP_PREC_F16);
    const float4 g0 = *(const float4*)(dA + off), g1 = *(const float4*)(dA + off + 4);
    float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, xs[8];
    load8<X16>(x, off, xs);
    norm_mask<8>(g, xs, a, b, mask_mode, act_hi, mask_src, off);
    if (g_out) {
        *(float4*)(g_out + off) = make_float4(g[0], g[1], g[2], g[3]);
        *(float4*)(g_out + off + 4) = make_float4(g[4], g[5], g[6], g[7]);
    }
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(cf[j * 3], g[j], fmaf(cf[j * 3 + 1], xs[j], cf[j * 3 + 2])) * post;
    store_op8<F16, SPLIT>(v, hi, lo, off);
}

// pass 3, one (pixel, 8-channel group) item per thread and iteration, coefficients re-read per item (40 scalars per 8 elements): the
// form for C/8 > 256 channel groups
template <int PREC, bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_apply_kernel(const float* __restrict__ dA, const void* __restrict__ x, const void* __restrict__ mask_src,
                                                             const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ coef,
                                                             const float* __restrict__ bound, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                                             float* __restrict__ out_scale, long long items, int C, int mask_mode, float act_hi,
                                                             float* __restrict__ g_out) {
    const float sc_out = bn_bwd16_out_scale<PREC == LP_PREC_F16>(bound, C, out_scale);
    const int G = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % G) * 8;
        bn_bwd16_apply_item<PREC, X16>(dA, x, mask_src, scale + c, shift + c, coef + c * 3, sc_out, hi, lo, g_out, (size_t)i * 8, mask_mode, act_hi);
    }
}

// pass 3 for C/8 <= 256 channel groups (every layer of the two encoders): a thread keeps ONE group of 8 channels -- its 40 coefficients
// (ca, cb, cc, scale, shift) are loaded once as float4s -- and walks the pixels of its block (256 / (C/8) pixels per iteration, the
// lanes of a pixel contiguous: coalesced 32 B per lane)
template <int PREC, bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_apply_rows_kernel(const float* __restrict__ dA, const void* __restrict__ x, const void* __restrict__ mask_src,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ coef,
                                                                  const float* __restrict__ bound, uint16_t* __restrict__ hi, uint16_t* __restrict__ lo,
                                                                  float* __restrict__ out_scale, long long P, int C, int rows, int PB, int mask_mode, float act_hi,
                                                                  float* __restrict__ g_out) {
    const float sc_out = bn_bwd16_out_scale<PREC == LP_PREC_F16>(bound, C, out_scale);
    const int G = C >> 3;
    const int cg = threadIdx.x % G, r = threadIdx.x / G;
    if (r >= rows) return;
    const int c = cg * 8;
    float cf[24], a8[8], b8[8];
#pragma unroll
    for (int j = 0; j < 6; ++j) { const float4 q = *(const float4*)(coef + (size_t)c * 3 + j * 4); cf[j * 4] = q.x; cf[j * 4 + 1] = q.y; cf[j * 4 + 2] = q.z; cf[j * 4 + 3] = q.w; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float4 q = *(const float4*)(scale + c + j * 4), t = *(const float4*)(shift + c + j * 4);
        a8[j * 4] = q.x; a8[j * 4 + 1] = q.y; a8[j * 4 + 2] = q.z; a8[j * 4 + 3] = q.w;
        b8[j * 4] = t.x; b8[j * 4 + 1] = t.y; b8[j * 4 + 2] = t.z; b8[j * 4 + 3] = t.w;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { cf[j * 3] *= sc_out; cf[j * 3 + 1] *= sc_out; cf[j * 3 + 2] *= sc_out; }      // power of two: exact
    const long long p0 = (long long)blockIdx.x * PB, p1 = min(P, p0 + PB);
#pragma unroll 2
    for (long long pix = p0 + r; pix < p1; pix += rows)
        bn_bwd16_apply_item<PREC, X16>(dA, x, mask_src, a8, b8, cf, 1.f, hi, lo, g_out, (size_t)pix * C + c, mask_mode, act_hi);
}

// DUAL form of pass 3 (see bn_bwd16_partial2_kernel): g from dA and the mask once, then dy of BN a and of BN b from its own x and coefficients
template <int PREC, bool X16>
__device__ __forceinline__ void bn_bwd16_apply_item2(const float* dA, const void* xa, const void* xb, const void* mask_src, const float* cfa,
                                                     const float* cfb, float post_a, float post_b, uint16_t* hi_a, uint16_t* lo_a, uint16_t* hi_b,
                                                     uint16_t* lo_b, size_t off, int mask_mode) {
    constexpr bool SPLIT = (PREC == LP_PREC_BF16X3), F16 = (PREC == LP_PREC_F16);
    const float4 g0 = *(const float4*)(dA + off), g1 = *(const float4*)(dA + off + 4);
    float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, xs[8], v[8];
    load8<X16>(xa, off, xs);
    norm_mask<8>(g, xs, cfa, cfa, mask_mode, 0.f, mask_src, off);      // (modes 1 .. 4: x, scale and shift are not looked at)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(cfa[j * 3], g[j], fmaf(cfa[j * 3 + 1], xs[j], cfa[j * 3 + 2])) * post_a;
    store_op8<F16, SPLIT>(v, hi_a, lo_a, off);
    load8<X16>(xb, off, xs);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaf(cfb[j * 3], g[j], fmaf(cfb[j * 3 + 1], xs[j], cfb[j * 3 + 2])) * post_b;
    store_op8<F16, SPLIT>(v, hi_b, lo_b, off);
}

struct BnBwd16Dual {          // what pass 3 needs of one of the two BatchNorms
    const void* x; const float* coef; const float* bound; uint16_t* hi; uint16_t* lo; float* out_scale;
};

template <int PREC, bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_apply2_kernel(const float* __restrict__ dA, const void* __restrict__ mask_src, BnBwd16Dual a, BnBwd16Dual b,
                                                              long long items, int C, int mask_mode) {
    const float sa = bn_bwd16_out_scale<PREC == LP_PREC_F16>(a.bound, C, a.out_scale);
    __syncthreads();                                                          // (the scale prologue's shared scratch is used again)
    const float sb = bn_bwd16_out_scale<PREC == LP_PREC_F16>(b.bound, C, b.out_scale);
    const int G = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % G) * 8;
        bn_bwd16_apply_item2<PREC, X16>(dA, a.x, b.x, mask_src, a.coef + c * 3, b.coef + c * 3, sa, sb, a.hi, a.lo, b.hi, b.lo, (size_t)i * 8, mask_mode);
    }
}

template <int PREC, bool X16>
__global__ __launch_bounds__(256) void bn_bwd16_apply2_rows_kernel(const float* __restrict__ dA, const void* __restrict__ mask_src, BnBwd16Dual a, BnBwd16Dual b,
                                                                   long long P, int C, int rows, int PB, int mask_mode) {
    const float sa = bn_bwd16_out_scale<PREC == LP_PREC_F16>(a.bound, C, a.out_scale);
    __syncthreads();
    const float sb = bn_bwd16_out_scale<PREC == LP_PREC_F16>(b.bound, C, b.out_scale);
    const int G = C >> 3;
    const int cg = threadIdx.x % G, r = threadIdx.x / G;
    if (r >= rows) return;
    const int c = cg * 8;
    float cfa[24], cfb[24];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const float4 q = *(const float4*)(a.coef + (size_t)c * 3 + j * 4), t = *(const float4*)(b.coef + (size_t)c * 3 + j * 4);
        cfa[j * 4] = q.x * sa; cfa[j * 4 + 1] = q.y * sa; cfa[j * 4 + 2] = q.z * sa; cfa[j * 4 + 3] = q.w * sa;      // power of two: exact
        cfb[j * 4] = t.x * sb; cfb[j * 4 + 1] = t.y * sb; cfb[j * 4 + 2] = t.z * sb; cfb[j * 4 + 3] = t.w * sb;
    }
    const long long p0 = (long long)blockIdx.x * PB, p1 = min(P, p0 + PB);
#pragma unroll 2
    for (long long pix = p0 + r; pix < p1; pix += rows)
        bn_bwd16_apply_item2<PREC, X16>(dA, a.x, b.x, mask_src, cfa, cfb, 1.f, 1.f, a.hi, a.lo, b.hi, b.lo, (size_t)pix * C + c, mask_mode);
}

extern "C" long long lp_bn_bwd16_workspace_bytes(long long P, int C) {
    const int PB = lp_stat_split_pix(1, P, C);
    const long long S = (P + PB - 1) / PB;
    return (S * C * 4 + (long long)C * 4) * (long long)sizeof(float);
}

struct BnBwd16Params {
    const float* dA; const void* x; int x16; const void* mask_src;
    const float* gamma; const float* mean; const float* rstd; const float* scale; const float* shift;
    uint16_t* out_hi; uint16_t* out_lo; float* out_scale; float* dgamma; float* dbeta; float* workspace;
    long long P; int C, mask_mode; float act_hi; int frozen_stats, prec;
    float* g_out; hipStream_t stream;
};

// the three passes for one instantiation (operand precision, x as fp32 or fp16 plane)
template <int PREC, bool X16> static int bn_bwd16_launch(const BnBwd16Params& p) {
    const long long P = p.P;
    const int C = p.C, G = C >> 3;
    const int PB = lp_stat_split_pix(1, P, C);
    const int S = (int)((P + PB - 1) / PB);
    float* part = p.workspace;
    float* coef = p.workspace + (size_t)S * C * 4;
    float* bound = coef + (size_t)C * 3;
    const float hi_ = p.act_hi > 0.f ? p.act_hi : 3.0e38f;
    hipLaunchKernelGGL(bn_bwd16_partial_kernel<X16>, dim3(S, (C + 63) / 64), dim3(256), 0, p.stream, p.dA, p.x, p.mask_src, p.mean, p.rstd, p.scale,
                       p.shift, part, P, C, p.mask_mode, hi_, PB);
    int rc = lp_check_launch("bn_bwd16_partial");
    if (rc) return rc;
    hipLaunchKernelGGL(bn_bwd16_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, p.stream, part, p.gamma, p.mean, p.rstd, p.dgamma, p.dbeta, coef,
                       bound, C, S, 1.0f / (float)P, p.frozen_stats);
    rc = lp_check_launch("bn_bwd16_finalize");
    if (rc) return rc;
    if (G <= 256) {
        const int rows = 256 / G;
        long long ppb = (P + 4095) / 4096;                                   // <= 4096 workgroups, >= 4 pixel rows per thread where P allows
        if (ppb < 4ll * rows) ppb = 4ll * rows;
        ppb = (ppb + rows - 1) / rows * rows;
        hipLaunchKernelGGL((bn_bwd16_apply_rows_kernel<PREC, X16>), dim3((unsigned)((P + ppb - 1) / ppb)), dim3(256), 0, p.stream, p.dA, p.x, p.mask_src,
                           p.scale, p.shift, coef, bound, p.out_hi, p.out_lo, p.out_scale, P, C, rows, (int)ppb, p.mask_mode, hi_, p.g_out);
    } else {
        const long long items = P * G, blocks = (items + 255) / 256;
        hipLaunchKernelGGL((bn_bwd16_apply_kernel<PREC, X16>), dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, p.stream, p.dA, p.x,
                           p.mask_src, p.scale, p.shift, coef, bound, p.out_hi, p.out_lo, p.out_scale, items, C, p.mask_mode, hi_, p.g_out);
    }
    return lp_check_launch("bn_bwd16_apply");
}

static int bn_bwd16_impl(const BnBwd16Params& p) {
    if (!p.dA || !p.x || !p.gamma || !p.mean || !p.rstd || !p.scale || !p.shift || !p.out_hi || !p.out_scale || !p.dgamma || !p.dbeta || !p.workspace)
        return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: null pointer");
    if (p.C & 7) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_bn_bwd16: C must be a multiple of 8");
    if (p.mask_mode < 0 || p.mask_mode > 4 || (p.mask_mode >= 2 && !p.mask_src)) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: bad mask mode");
    if (p.prec == LP_PREC_BF16X3 && !p.out_lo) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: bf16x3 needs the lo plane");
    if (p.x16 && p.prec != LP_PREC_F16) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_bn_bwd16_h: 16-bit x exists in the fp16 mode only");
    if (p.P < 1) return LP_OK;
    if (p.x16) return bn_bwd16_launch<LP_PREC_F16, true>(p);
    if (p.prec == LP_PREC_BF16) return bn_bwd16_launch<LP_PREC_BF16, false>(p);
    if (p.prec == LP_PREC_BF16X3) return bn_bwd16_launch<LP_PREC_BF16X3, false>(p);
    if (p.prec == LP_PREC_F16) return bn_bwd16_launch<LP_PREC_F16, false>(p);
    return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: unknown precision mode");
}

// x as fp32 (x16 = NULL) or as the fp16 plane a conv epilogue wrote instead of fp32 y (x = NULL, fp16 mode); mask modes 0 / 1 / 2 as
// lp_bn_bwd16 (2: mask_src fp32 > 0) and 3: mask_src = a 16-bit OPERAND PLANE [P][C] whose elements are > 0 (the block output's planes:
// 2 B instead of 4 B per element for the ReLU pattern behind the residual add) and 4: mask_src = the same pattern as one bit per element
// (bytes [P][C / 8] from lp_bn_add_act_bits)
extern "C" int lp_bn_bwd16_h(const float* dA, const float* x, const uint16_t* x16, const void* mask_src, const float* gamma, const float* mean,
                             const float* rstd, const float* scale, const float* shift, uint16_t* out_hi, uint16_t* out_lo, float* out_scale,
                             float* dgamma, float* dbeta, float* workspace, long long P, int C, int mask_mode, float act_hi, int frozen_stats,
                             int prec, float* g_out, void* stream) {
    BnBwd16Params p;
    p.dA = dA; p.x = x16 ? (const void*)x16 : (const void*)x; p.x16 = x16 != nullptr; p.mask_src = mask_src;
    p.gamma = gamma; p.mean = mean; p.rstd = rstd; p.scale = scale; p.shift = shift;
    p.out_hi = out_hi; p.out_lo = out_lo; p.out_scale = out_scale; p.dgamma = dgamma; p.dbeta = dbeta; p.workspace = workspace;
    p.P = P; p.C = C; p.mask_mode = mask_mode; p.act_hi = act_hi; p.frozen_stats = frozen_stats; p.prec = prec;
    p.g_out = g_out; p.stream = (hipStream_t)stream;
    return bn_bwd16_impl(p);
}

extern "C" int lp_bn_bwd16(const float* dA, const float* x, const float* mask_src, const float* gamma, const float* mean, const float* rstd,
                           const float* scale, const float* shift, uint16_t* out_hi, uint16_t* out_lo, float* out_scale, float* dgamma,
                           float* dbeta, float* workspace, long long P, int C, int mask_mode, float act_hi, int frozen_stats, int prec,
                           float* g_out, void* stream) {
    if (!x) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: null pointer");
    if (mask_mode >= 3) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16: mask modes 3 (16-bit plane) and 4 (bit pattern) are lp_bn_bwd16_h's");
    return lp_bn_bwd16_h(dA, x, nullptr, mask_src, gamma, mean, rstd, scale, shift, out_hi, out_lo, out_scale, dgamma, dbeta, workspace, P, C,
                         mask_mode, act_hi, frozen_stats, prec, g_out, stream);
}

// the passes of the dual form for one instantiation: two partial sets, two finalize launches (the single form's kernel), one apply
template <int PREC, bool X16> static int bn_bwd16_dual_launch(const float* dA, const void* mask_src, const BnBwd16Params& a, const BnBwd16Params& b) {
    const long long P = a.P;
    const int C = a.C, G = C >> 3;
    const int PB = lp_stat_split_pix(1, P, C);
    const int S = (int)((P + PB - 1) / PB);
    float* part[2] = {a.workspace, b.workspace};
    float* coef[2] = {a.workspace + (size_t)S * C * 4, b.workspace + (size_t)S * C * 4};
    float* bound[2] = {coef[0] + (size_t)C * 3, coef[1] + (size_t)C * 3};
    hipLaunchKernelGGL(bn_bwd16_partial2_kernel<X16>, dim3(S, (C + 63) / 64), dim3(256), 0, a.stream, dA, a.x, b.x, mask_src, a.mean, a.rstd, b.mean, b.rstd,
                       part[0], part[1], P, C, a.mask_mode, PB);
    int rc = lp_check_launch("bn_bwd16_partial2");
    if (rc) return rc;
    const BnBwd16Params* q[2] = {&a, &b};
    for (int k = 0; k < 2; ++k) {
        hipLaunchKernelGGL(bn_bwd16_finalize_kernel, dim3((C + 3) / 4), dim3(256), 0, a.stream, part[k], q[k]->gamma, q[k]->mean, q[k]->rstd, q[k]->dgamma,
                           q[k]->dbeta, coef[k], bound[k], C, S, 1.0f / (float)P, a.frozen_stats);
        rc = lp_check_launch("bn_bwd16_finalize");
        if (rc) return rc;
    }
    const BnBwd16Dual da = {a.x, coef[0], bound[0], a.out_hi, a.out_lo, a.out_scale}, db = {b.x, coef[1], bound[1], b.out_hi, b.out_lo, b.out_scale};
    if (G <= 256) {          // (the grid rule of bn_bwd16_launch)
        const int rows = 256 / G;
        long long ppb = (P + 4095) / 4096;
        if (ppb < 4ll * rows) ppb = 4ll * rows;
        ppb = (ppb + rows - 1) / rows * rows;
        hipLaunchKernelGGL((bn_bwd16_apply2_rows_kernel<PREC, X16>), dim3((unsigned)((P + ppb - 1) / ppb)), dim3(256), 0, a.stream, dA, mask_src, da, db, P, C,
                           rows, (int)ppb, a.mask_mode);
    } else {
        const long long items = P * G, blocks = (items + 255) / 256;
        hipLaunchKernelGGL((bn_bwd16_apply2_kernel<PREC, X16>), dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, a.stream, dA, mask_src, da, db,
                           items, C, a.mask_mode);
    }
    return lp_check_launch("bn_bwd16_apply2");
}

// Two BatchNorm backwards over the SAME incoming gradient and ReLU pattern in one pass pair: out = relu(BN_a(xa) + BN_b(xb)) (bn3 and the
// downsample BatchNorm of a residual block).  Per BN the arguments and results of lp_bn_bwd16_h (each with its own workspace of
// lp_bn_bwd16_workspace_bytes), bit-identical to two lp_bn_bwd16_h calls; dA and the pattern are read once per pass instead of twice.
// xa / xb: both fp32 (xa16 = xb16 = NULL) or both fp16 planes (xa = xb = NULL, fp16 mode).  mask_mode 1 .. 4 (a pattern that does not depend on x).
extern "C" int lp_bn_bwd16_dual(const float* dA, const void* mask_src, const float* xa, const uint16_t* xa16, const float* gamma_a, const float* mean_a,
                                const float* rstd_a, uint16_t* hi_a, uint16_t* lo_a, float* out_scale_a, float* dgamma_a, float* dbeta_a,
                                float* workspace_a, const float* xb, const uint16_t* xb16, const float* gamma_b, const float* mean_b,
                                const float* rstd_b, uint16_t* hi_b, uint16_t* lo_b, float* out_scale_b, float* dgamma_b, float* dbeta_b,
                                float* workspace_b, long long P, int C, int mask_mode, int frozen_stats, int prec, void* stream) {
    if ((xa16 != nullptr) != (xb16 != nullptr)) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_bn_bwd16_dual: both x as fp32 or both as fp16 planes");
    const bool x16 = xa16 != nullptr;
    BnBwd16Params a, b;
    a.dA = dA; a.x = x16 ? (const void*)xa16 : (const void*)xa; a.x16 = x16; a.mask_src = mask_src; a.gamma = gamma_a; a.mean = mean_a; a.rstd = rstd_a;
    a.scale = a.shift = nullptr; a.out_hi = hi_a; a.out_lo = lo_a; a.out_scale = out_scale_a; a.dgamma = dgamma_a; a.dbeta = dbeta_a; a.workspace = workspace_a;
    a.P = P; a.C = C; a.mask_mode = mask_mode; a.act_hi = 0.f; a.frozen_stats = frozen_stats; a.prec = prec; a.g_out = nullptr; a.stream = (hipStream_t)stream;
    b = a;
    b.x = x16 ? (const void*)xb16 : (const void*)xb; b.gamma = gamma_b; b.mean = mean_b; b.rstd = rstd_b; b.out_hi = hi_b; b.out_lo = lo_b;
    b.out_scale = out_scale_b; b.dgamma = dgamma_b; b.dbeta = dbeta_b; b.workspace = workspace_b;
    for (const BnBwd16Params* q : {&a, &b})
        if (!dA || !q->x || !q->gamma || !q->mean || !q->rstd || !q->out_hi || !q->out_scale || !q->dgamma || !q->dbeta || !q->workspace)
            return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16_dual: null pointer");
    if (C & 7) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_bn_bwd16_dual: C must be a multiple of 8");
    if (mask_mode < 1 || mask_mode > 4 || (mask_mode >= 2 && !mask_src)) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16_dual: mask mode 1 .. 4");
    if (prec == LP_PREC_BF16X3 && (!lo_a || !lo_b)) return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16_dual: bf16x3 needs the lo planes");
    if (x16 && prec != LP_PREC_F16) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_bn_bwd16_dual: 16-bit x exists in the fp16 mode only");
    if (P < 1) return LP_OK;
    if (x16) return bn_bwd16_dual_launch<LP_PREC_F16, true>(dA, mask_src, a, b);
    if (prec == LP_PREC_BF16) return bn_bwd16_dual_launch<LP_PREC_BF16, false>(dA, mask_src, a, b);
    if (prec == LP_PREC_BF16X3) return bn_bwd16_dual_launch<LP_PREC_BF16X3, false>(dA, mask_src, a, b);
    if (prec == LP_PREC_F16) return bn_bwd16_dual_launch<LP_PREC_F16, false>(dA, mask_src, a, b);
    return lp_set_error(LP_ERR_ARG, "lp_bn_bwd16_dual: unknown precision mode");
}
