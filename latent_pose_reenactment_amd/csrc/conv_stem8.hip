// First layer of the stickman-conditioned nets (embedders/FSTH.py, discriminators/FSTH.py of the reference) for gfx950: a 3x3 (zero padding) or
// 1x1 conv from 5..8 input channels to Cout % 64 == 0, whose input is the channel-wise concatenation of TWO fp32 tensors (stickman, image) in any
// channel order -- the embedder sees (s0 s1 s2 r0 r1 r2), the critic the interleaved (s0 r0 s1 r1 s2 r2).  The concatenated tensor is never
// written: every kernel here gathers its pixels from the two sources through a channel map and element strides (NCHW, NHWC or a 5-D view alike).
//
//   forward      one pixel padded to 8 x 16-bit channels is ONE 16-byte LDS word, and for v_mfma_f32_16x16x32 a lane's 8 k-values are then one
//                tap of one pixel = one ds_read_b128.  k = 8 * tap + channel: a k-step covers 4 taps, 9 taps need 3 k-steps (the last one has
//                three empty tap slots).  A wave takes 16 consecutive pixels of an image row (M) x 64 output channels (4 N tiles).  bf16x3: hi + lo
//                planes of the input in LDS and 3 MFMAs per k-step.  The layer is bound by its output write (64 x 256^2 x 64 fp32 = 1.07 GB): the
//                16 x 64 block goes through a wave-private LDS tile so that a pixel's channels leave as 256-byte runs, as fp32 y and / or as the
//                operand planes of (relu?)(y) for the second stem conv (bit-identical to lp_act_pack of y).
//   weight grad  fp32 on the VALU by the kernel the <= 4 channel convs of conv_thin.hip use (wgrad_rows_kernel of thin_rows.h: the work is a
//                bandwidth-bound reduction over pixels: dy is streamed once, 64 channels per wave; the gathered input rows are broadcast from LDS,
//                two 16-byte words per pixel).  Per-workgroup partial slabs + the fixed-order reduction of conv_thin.hip: the same sum in every
//                run.  The bias gradient comes from the same pass over dy.
//   data grad    to the IMAGE source only (the stickman has no gradient): 4 lanes share a pixel, each takes a quarter of the output channels of
//                every tap from the fp32 dy rows (64 contiguous bytes per quad and load) against fp32 W_orig in LDS, then a 2-step quad reduction.
#include "lp_common.h"
#include "lp_hip.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file (see csrc/spectral_norm.hip: the op_sel forms hipcc picks for "vector times broadcast scalar" -- exactly the
// shape of the weight-gradient FMAs below -- are wrong beside the LDS-DMA convolution kernels on gfx950; tests/test_isa_lint.py).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "thin_rows.h"      // (inside the region: the shared device code compiled into this file's kernels takes the attribute too)

struct Stem8Src {
    const float* p;
    long long sn, sc, sy, sx;      // element strides of (image, channel, row, column)
};

// cmap: nibble c (conv input channel c) = (source << 3) | channel inside that source
__device__ __forceinline__ float stem8_load(const Stem8Src& a, const Stem8Src& b, unsigned cmap, int c, int n, int y, int x) {
    const unsigned e = (cmap >> (4 * c)) & 15u;
    const Stem8Src& s = (e & 8u) ? b : a;
    return s.p[(long long)n * s.sn + (long long)(e & 7u) * s.sc + (long long)y * s.sy + (long long)x * s.sx];
}

struct Stem8FwdParams {
    Stem8Src a, b; unsigned cmap;
    const uint16_t* w_hi; const uint16_t* w_lo; float* y; const float* bias; const float* alpha; uint16_t* o_hi; uint16_t* o_lo;
    int N, H, W, Cin, Cout, CinP, CoutP, o_relu;
};

// MODE = LP_PREC_BF16 | LP_PREC_BF16X3 | LP_PREC_F16
template <int MODE> struct Stem8Geom { static constexpr int RB = (MODE == LP_PREC_BF16X3) ? 2 : 4; };

template <int MODE, int KS>
__global__ __launch_bounds__(256) void conv_stem8_fwd_kernel(Stem8FwdParams p) {
    constexpr bool F16 = MODE == LP_PREC_F16, X3 = MODE == LP_PREC_BF16X3;
    constexpr int PAD = KS / 2, T = KS * KS, KSTEPS = (T + 3) / 4, RB = Stem8Geom<MODE>::RB, ROWS = RB + 2 * PAD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    const int RW = p.W + 2 * PAD;
    uint16_t* halo_hi = (uint16_t*)smraw;                                          // [ROWS][RW][8] 16-bit: one 16-byte word per pixel
    uint16_t* halo_lo = halo_hi + (size_t)ROWS * RW * 8;                           // (X3 only)
    float* tbase = (float*)(smraw + (size_t)ROWS * RW * 16 * (X3 ? 2 : 1));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* Tl = tbase + wave * (16 * 68);                                           // this wave's 16 x 64 output block (+4 pad)
    const int co0 = blockIdx.y * 64;
    const int kg = lane >> 4, m = lane & 15;
    // k-step ks, lane group kg -> tap ks * 4 + kg -> halo offset (pixels) relative to (row r, pixel x0 + m); B fragments = 8 channels of that tap
    int aoff[KSTEPS];
    s16x8_t bh[KSTEPS][4], bl[KSTEPS][4];
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) {
        const int t = ks * 4 + kg;
        aoff[ks] = t < T ? (t / KS) * RW + (t % KS) : -1;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            const size_t idx = ((size_t)(t < T ? t : 0) * p.CoutP + co0 + nt * 16 + m) * p.CinP;       // pack layout [tap][CoutP][CinP], zero padded
            const s16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
            bh[ks][nt] = t < T ? *(const s16x8_t*)(p.w_hi + idx) : z;
            if (X3) bl[ks][nt] = t < T ? *(const s16x8_t*)(p.w_lo + idx) : z;
        }
    }
    const float alpha = p.alpha ? *p.alpha : 1.f;
    const int pq = lane >> 2, cq = (lane & 3) * 16;                                  // store phase: pixel of the block, first of 16 channels
    float bias16[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) bias16[j] = p.bias ? p.bias[co0 + cq + j] : 0.f;
    const int gpi = (p.H + RB - 1) / RB, segs = p.W >> 4;
    for (int grp = blockIdx.x; grp < p.N * gpi; grp += gridDim.x) {
        const int n = grp / gpi, y0 = (grp % gpi) * RB;
        __syncthreads();
        for (int i = tid; i < ROWS * RW; i += 256) {
            const int r = i / RW, hx = i - r * RW;
            const int iy = y0 + r - PAD, ix = hx - PAD;
            s16x8_t vh = {0, 0, 0, 0, 0, 0, 0, 0}, vl = {0, 0, 0, 0, 0, 0, 0, 0};
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) {
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c < p.Cin) {
                        const float v = stem8_load(p.a, p.b, p.cmap, c, n, iy, ix);
                        const uint16_t h = lp_f32_to_op16<F16>(v);
                        vh[c] = (short)h;
                        if (X3) vl[c] = (short)lp_f32_to_op16<false>(v - lp_op16_to_f32<false>(h));
                    }
            }
            *(s16x8_t*)(halo_hi + (size_t)i * 8) = vh;
            if (X3) *(s16x8_t*)(halo_lo + (size_t)i * 8) = vl;
        }
        __syncthreads();
        const int nrow = min(RB, p.H - y0);
        for (int sgi = wave; sgi < nrow * segs; sgi += 4) {
            const int r = sgi / segs, x0 = (sgi - r * segs) << 4;
            const size_t hb = (size_t)r * RW + x0 + m;
            s16x8_t ah[KSTEPS], al[KSTEPS];
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) {
                const s16x8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
                const size_t o = (hb + (aoff[ks] >= 0 ? aoff[ks] : 0)) * 8;
                ah[ks] = *(const s16x8_t*)(halo_hi + o);
                if (aoff[ks] < 0) ah[ks] = z;
                if (X3) { al[ks] = *(const s16x8_t*)(halo_lo + o); if (aoff[ks] < 0) al[ks] = z; }
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
                if (X3) {          // the small cross terms first, the hi x hi products last
#pragma unroll
                    for (int ks = 0; ks < KSTEPS; ++ks) {
                        acc = mfma16t<false>(al[ks], bh[ks][nt], acc);
                        acc = mfma16t<false>(ah[ks], bl[ks][nt], acc);
                    }
                }
#pragma unroll
                for (int ks = 0; ks < KSTEPS; ++ks) acc = mfma16t<F16>(ah[ks], bh[ks][nt], acc);
#pragma unroll
                for (int q = 0; q < 4; ++q) Tl[(kg * 4 + q) * 68 + nt * 16 + m] = acc[q];      // C: row = (lane>>4)*4 + q (pixel), col = lane&15
            }
            // (wave-private block: the LDS writes above are ordered before the reads below by the compiler's lgkmcnt wait)
            rows_store_tile<F16, X3>(Tl, pq, cq, alpha, bias16, (size_t)(n * p.H + y0 + r) * p.W + x0 + pq, p.y, p.o_hi, p.o_lo, p.Cout, co0, p.o_relu);
        }
    }
}

static size_t stem8_fwd_lds(int W, int ksize, int prec) {
    const bool x3 = prec == LP_PREC_BF16X3;      // hi + lo planes of the rows (16 bytes per pixel each), then the four waves' 16 x 68 fp32 tiles
    return rows_lds_bytes(x3 ? 2 : 4, ksize / 2, W, x3 ? 32 : 16) + (size_t)4 * 16 * 68 * sizeof(float);
}

// one answer for the three operand modes and for forward + weight gradient (the callers route a layer as a whole): the widest staging decides
static bool stem8_shape_ok(int Cin, int Cout, int ksize, int W) {
    if (Cin < 5 || Cin > 8 || Cout < 64 || (Cout % 64) != 0 || (ksize != 1 && ksize != 3) || W < 16 || (W % 16) != 0) return false;
    if (stem8_fwd_lds(W, ksize, LP_PREC_BF16X3) > 64 * 1024 || stem8_fwd_lds(W, ksize, LP_PREC_F16) > 64 * 1024) return false;
    return RowsWgGeom<8>::lds_bytes(ksize, W) <= 64 * 1024;      // weight gradient: fp32 rows, 32 bytes per pixel
}

// the channel map must name, for every conv input channel, an existing channel of one of the two sources
static bool stem8_cmap_ok(unsigned cmap, int Cin, int Ca, int Cb, bool have_a, bool have_b) {
    for (int c = 0; c < Cin; ++c) {
        const unsigned e = (cmap >> (4 * c)) & 15u;
        const int ch = (int)(e & 7u);
        if (e & 8u) { if (!have_b || ch >= Cb) return false; }
        else if (!have_a || ch >= Ca) return false;
    }
    return true;
}

static Stem8Src stem8_src(const float* ptr, const long long* st) {
    Stem8Src s; s.p = ptr; s.sn = st ? st[0] : 0; s.sc = st ? st[1] : 0; s.sy = st ? st[2] : 0; s.sx = st ? st[3] : 0;
    return s;
}

extern "C" int lp_stem8_supported(int Cin, int Cout, int ksize, int W) { return stem8_shape_ok(Cin, Cout, ksize, W) ? 1 : 0; }

extern "C" int lp_stem8_fwd(const float* xa, const long long* stride_a, int Ca, const float* xb, const long long* stride_b, int Cb, int cmap,
                            const uint16_t* w_hi, const uint16_t* w_lo, float* y, const float* bias, const float* alpha, int N, int H, int W, int Cin,
                            int Cout, int CinP, int CoutP, int ksize, int prec, uint16_t* out_hi, uint16_t* out_lo, int out_relu, void* stream) {
    if (!w_hi || (!xa && !xb) || (xa && !stride_a) || (xb && !stride_b)) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: null pointer");
    if (prec != LP_PREC_BF16 && prec != LP_PREC_BF16X3 && prec != LP_PREC_F16) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: unknown operand mode");
    if (prec == LP_PREC_BF16X3 && (!w_lo || (out_hi && !out_lo))) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: bf16x3 needs the lo planes");
    if (!y && !out_hi) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: neither y nor operand planes requested");
    if (N < 1 || H < 1) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: empty tensor");
    if (!stem8_shape_ok(Cin, Cout, ksize, W)) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stem8_fwd: needs 5 <= Cin <= 8, Cout % 64 == 0, 1x1 | 3x3, W % 16 == 0, rows that fit LDS");
    if (CinP < 8 || (CinP % 8) != 0 || CoutP < Cout) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: weight pack geometry");
    if (!stem8_cmap_ok((unsigned)cmap, Cin, Ca, Cb, xa != nullptr, xb != nullptr)) return lp_set_error(LP_ERR_ARG, "lp_stem8_fwd: channel map names a channel outside its source");
    Stem8FwdParams p;
    p.a = stem8_src(xa, stride_a); p.b = stem8_src(xb, stride_b); p.cmap = (unsigned)cmap;
    p.w_hi = w_hi; p.w_lo = w_lo; p.y = y; p.bias = bias; p.alpha = alpha; p.o_hi = out_hi; p.o_lo = prec == LP_PREC_BF16X3 ? out_lo : nullptr;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.CinP = CinP; p.CoutP = CoutP; p.o_relu = out_relu;
    using Kernel = void (*)(Stem8FwdParams);
    static const Kernel kernels[3][2] = {{conv_stem8_fwd_kernel<LP_PREC_BF16, 1>, conv_stem8_fwd_kernel<LP_PREC_BF16, 3>},      // [operand mode][3x3]
                                         {conv_stem8_fwd_kernel<LP_PREC_BF16X3, 1>, conv_stem8_fwd_kernel<LP_PREC_BF16X3, 3>},
                                         {conv_stem8_fwd_kernel<LP_PREC_F16, 1>, conv_stem8_fwd_kernel<LP_PREC_F16, 3>}};
    static_assert(LP_PREC_BF16 == 0 && LP_PREC_BF16X3 == 1 && LP_PREC_F16 == 2, "the kernel table is indexed by the operand mode");
    const dim3 grid(rows_groups(N, H, prec == LP_PREC_BF16X3 ? 2 : 4, 4096), Cout / 64);
    hipLaunchKernelGGL(kernels[prec][ksize == 3], grid, dim3(256), stem8_fwd_lds(W, ksize, prec), (hipStream_t)stream, p);
    return lp_check_launch("conv_stem8_fwd");
}

// ------------------------------------------------------------------------------------------------------------------
// Weight + bias gradient:  dw[co][ci][tap] = sum_{n,y,x} dy[n,y,x,co] * x[n, y+ky-1, x+kx-1, ci],  db[co] = sum dy[n,y,x,co]
// ------------------------------------------------------------------------------------------------------------------
// source policy of wgrad_rows_kernel (thin_rows.h): the 5..8 channels of a pixel gathered from the two sources
struct Stem8Gather {
    Stem8Src a, b; unsigned cmap;
    __device__ __forceinline__ void load(const float*, int Cin, int n, int y, int x, int, int, float (&v)[8]) const {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < Cin) v[c] = stem8_load(a, b, cmap, c, n, y, x);
    }
};

static int stem8_wgrad_groups(int N, int H) { return rows_groups(N, H, RowsWgGeom<8>::RB, 512); }

extern "C" long long lp_stem8_wgrad_workspace_bytes(int N, int H, int Cout, int ksize) {
    if (N < 1 || H < 1 || Cout < 1 || (ksize != 1 && ksize != 3)) return 0;
    return (long long)stem8_wgrad_groups(N, H) * ((long long)ksize * ksize * 8 + 1) * Cout * (long long)sizeof(float);
}

extern "C" int lp_stem8_wgrad(const float* xa, const long long* stride_a, int Ca, const float* xb, const long long* stride_b, int Cb, int cmap,
                              const float* dy, float* dw, float* dbias, float* workspace, int N, int H, int W, int Cin, int Cout, int ksize,
                              void* stream) {
    if (!dy || !dw || !workspace || (!xa && !xb) || (xa && !stride_a) || (xb && !stride_b)) return lp_set_error(LP_ERR_ARG, "lp_stem8_wgrad: null pointer");
    if (N < 1 || H < 1) return lp_set_error(LP_ERR_ARG, "lp_stem8_wgrad: empty tensor");
    if (!stem8_shape_ok(Cin, Cout, ksize, W)) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stem8_wgrad: needs 5 <= Cin <= 8, Cout % 64 == 0, 1x1 | 3x3, W % 16 == 0, rows that fit LDS");
    if (!stem8_cmap_ok((unsigned)cmap, Cin, Ca, Cb, xa != nullptr, xb != nullptr)) return lp_set_error(LP_ERR_ARG, "lp_stem8_wgrad: channel map names a channel outside its source");
    Stem8Gather src;
    src.a = stem8_src(xa, stride_a); src.b = stem8_src(xb, stride_b); src.cmap = (unsigned)cmap;
    const int T = ksize * ksize, G = stem8_wgrad_groups(N, H);
    RowsWgParams p;      // thin = the gathered input (8-channel slabs, zero padded), wide = dy; the bias partials follow the G slabs
    p.x = nullptr; p.x16 = nullptr; p.scale = nullptr; p.shift = nullptr; p.pro = 0;
    p.dy = dy; p.dw = dw; p.dbias = dbias;
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.G = G;
    p.part = workspace; p.bpart = workspace + (size_t)G * T * 8 * Cout;
    const auto kernel = ksize == 3 ? wgrad_rows_kernel<3, true, 8, true, Stem8Gather> : wgrad_rows_kernel<1, true, 8, true, Stem8Gather>;
    hipLaunchKernelGGL(kernel, dim3(G, Cout / 64), dim3(256), RowsWgGeom<8>::lds_bytes(ksize, W), (hipStream_t)stream, p, src);
    int rc = lp_check_launch("wgrad_stem8");
    if (rc) return rc;
    return lp_wgrad_rows_reduce(p.part, p.bpart, dw, dbias, G, T, 8, Cin, Cout, true, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------------------------
// Data gradient w.r.t. the image source:  dx[n, ch, y, x] = alpha * sum_{tap, co} dy[n, y-ky+1, x-kx+1, co] * W[co][ci(ch)][tap]
// ------------------------------------------------------------------------------------------------------------------
struct Stem8DgParams {
    const float* dy; const float* w; const float* alpha; float* dx;
    long long sn, sc, sy, sx;      // element strides of dx (image, channel, row, column)
    int ci[4];                     // conv input channel of image channel j (|-1)
    int N, H, W, Cin, Cout, nimg;
};

template <int KS>
__global__ __launch_bounds__(256) void dgrad_stem8_kernel(Stem8DgParams p) {
    constexpr int T = KS * KS, PAD = KS / 2;
    extern __shared__ __attribute__((aligned(16))) float wl[];          // [tap][co][4 image channels]
    for (int i = threadIdx.x; i < T * p.Cout * 4; i += 256) {
        const int j = i & 3, co = (i >> 2) % p.Cout, t = (i >> 2) / p.Cout;
        wl[i] = p.ci[j] >= 0 ? p.w[((size_t)co * p.Cin + p.ci[j]) * T + t] : 0.f;
    }
    __syncthreads();
    const int q = threadIdx.x & 3;
    const long long npix = (long long)p.N * p.H * p.W;
    const long long pix = (long long)blockIdx.x * 64 + (threadIdx.x >> 2);
    const bool live = pix < npix;
    const long long pp = live ? pix : 0;
    const int n = (int)(pp / ((long long)p.H * p.W));
    const int rem = (int)(pp - (long long)n * p.H * p.W);
    const int y = rem / p.W, x = rem - y * p.W;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
            const int sy = y - ky + PAD, sx = x - kx + PAD;
            if (!live || sy < 0 || sy >= p.H || sx < 0 || sx >= p.W) continue;
            const float* d = p.dy + ((size_t)(n * p.H + sy) * p.W + sx) * p.Cout;
            const float* wt = wl + (size_t)(ky * KS + kx) * p.Cout * 4;
            for (int co = q * 4; co < p.Cout; co += 16) {
                const float4 g = *(const float4*)(d + co);
                const float4 w0 = *(const float4*)(wt + (co + 0) * 4), w1 = *(const float4*)(wt + (co + 1) * 4);
                const float4 w2 = *(const float4*)(wt + (co + 2) * 4), w3 = *(const float4*)(wt + (co + 3) * 4);
                a0 = fmaf(g.x, w0.x, a0); a1 = fmaf(g.x, w0.y, a1); a2 = fmaf(g.x, w0.z, a2); a3 = fmaf(g.x, w0.w, a3);
                a0 = fmaf(g.y, w1.x, a0); a1 = fmaf(g.y, w1.y, a1); a2 = fmaf(g.y, w1.z, a2); a3 = fmaf(g.y, w1.w, a3);
                a0 = fmaf(g.z, w2.x, a0); a1 = fmaf(g.z, w2.y, a1); a2 = fmaf(g.z, w2.z, a2); a3 = fmaf(g.z, w2.w, a3);
                a0 = fmaf(g.w, w3.x, a0); a1 = fmaf(g.w, w3.y, a1); a2 = fmaf(g.w, w3.z, a2); a3 = fmaf(g.w, w3.w, a3);
            }
        }
    // the four lanes of a pixel hold disjoint output-channel quarters: butterfly sum (every lane of the wave takes part), lane j stores image channel j
    a0 += __shfl_xor(a0, 1, 64); a1 += __shfl_xor(a1, 1, 64); a2 += __shfl_xor(a2, 1, 64); a3 += __shfl_xor(a3, 1, 64);
    a0 += __shfl_xor(a0, 2, 64); a1 += __shfl_xor(a1, 2, 64); a2 += __shfl_xor(a2, 2, 64); a3 += __shfl_xor(a3, 2, 64);
    const float alpha = p.alpha ? *p.alpha : 1.f;
    const float v = q == 0 ? a0 : q == 1 ? a1 : q == 2 ? a2 : a3;
    if (live && q < p.nimg) p.dx[(long long)n * p.sn + (long long)q * p.sc + (long long)y * p.sy + (long long)x * p.sx] = v * alpha;
}

extern "C" int lp_stem8_dgrad(const float* dy, const float* w, const float* alpha, float* dx, const long long* stride_dx, int Cb, int cmap, int N,
                              int H, int W, int Cin, int Cout, int ksize, void* stream) {
    if (!dy || !w || !dx || !stride_dx) return lp_set_error(LP_ERR_ARG, "lp_stem8_dgrad: null pointer");
    if (N < 1 || H < 1 || W < 1) return lp_set_error(LP_ERR_ARG, "lp_stem8_dgrad: empty tensor");
    if (Cin < 5 || Cin > 8 || Cout < 16 || (Cout % 16) != 0 || Cout > 256 || (ksize != 1 && ksize != 3))
        return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stem8_dgrad: needs 5 <= Cin <= 8, Cout % 16 == 0, Cout <= 256, 1x1 | 3x3");
    if (Cb < 1 || Cb > 4) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stem8_dgrad: the image source has 1..4 channels");
    Stem8DgParams p;
    p.dy = dy; p.w = w; p.alpha = alpha; p.dx = dx;
    p.sn = stride_dx[0]; p.sc = stride_dx[1]; p.sy = stride_dx[2]; p.sx = stride_dx[3];
    for (int j = 0; j < 4; ++j) p.ci[j] = -1;
    for (int c = 0; c < Cin; ++c) {
        const unsigned e = ((unsigned)cmap >> (4 * c)) & 15u;
        if (e & 8u) {
            const int ch = (int)(e & 7u);
            if (ch >= Cb) return lp_set_error(LP_ERR_ARG, "lp_stem8_dgrad: channel map names a channel outside the image source");
            if (p.ci[ch] >= 0) return lp_set_error(LP_ERR_ARG, "lp_stem8_dgrad: an image channel appears twice in the channel map");
            p.ci[ch] = c;
        }
    }
    p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.nimg = Cb;
    const long long npix = (long long)N * H * W;
    const size_t lds = (size_t)ksize * ksize * Cout * 4 * sizeof(float);
    dim3 grid((unsigned)((npix + 63) / 64));
    if (ksize == 3) hipLaunchKernelGGL(dgrad_stem8_kernel<3>, grid, dim3(256), lds, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(dgrad_stem8_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, p);
    return lp_check_launch("dgrad_stem8");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
