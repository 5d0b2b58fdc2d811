// What the thin-channel convs (conv_thin.hip: <= 4 channels on one side) and the two-source first layer (conv_stem8.hip: 5..8 gathered input
// channels) share: both stage a few image rows of the THIN operand in LDS (one or two 16-byte words per pixel, zero border) and stream the WIDE
// operand, 64 channels per wave.
//   rows_lds_bytes / rows_groups   host side: the staged-rows LDS size and the number of row groups a launch walks
//   rows_store_tile                store phase of the MFMA forward kernels: a wave's 16 pixel x 64 channel block leaves LDS as fp32 y and / or
//                                  as the operand planes of (relu?)(y)
//   wgrad_rows_kernel              fp32 weight gradient as a reduction over pixels, one partial slab per workgroup
// Included INSIDE the translation unit's function-attribute region where it has one (conv_stem8.hip compiles without packed fp32 arithmetic):
// the functions here take the attributes of the place of inclusion.
#pragma once
#include "lp_common.h"

// LDS bytes of rb image rows with their pad-pixel border at ``bytes`` per staged pixel
static inline size_t rows_lds_bytes(int rb, int pad, int W, int bytes) { return (size_t)(rb + 2 * pad) * (W + 2 * pad) * bytes; }

// row groups (rb rows of one image each) of a launch = its grid.x: at most ``cap`` workgroups, which then stride over the groups
static inline int rows_groups(int N, int H, int rb, long long cap) {
    const long long g = (long long)N * ((H + rb - 1) / rb);
    return (int)(g > cap ? cap : g);
}

// Store phase of a wave's 16 x 64 output block T (fp32 accumulators, row stride 68): lane (pq, cq) takes 16 channels of pixel pq,
// o = fmaf(acc, alpha, bias), and writes them as 64 bytes of y (unless NULL) and / or as the operand planes of (relu?)(o) (o_hi NULL: none;
// X3: hi + lo), bit-identical to lp_act_pack of y.  ``pix`` = the lane's pixel index in the [N][H][W] image, co0 = first channel of the block.
template <bool F16, bool X3>
__device__ __forceinline__ void rows_store_tile(const float* T, int pq, int cq, float alpha, const float (&bias16)[16], size_t pix, float* y,
                                                uint16_t* o_hi, uint16_t* o_lo, int Cout, int co0, int o_relu) {
    float o[16];
#pragma unroll
    for (int j4 = 0; j4 < 4; ++j4) {
        const float4 v = *(const float4*)(T + pq * 68 + cq + j4 * 4);
        o[j4 * 4 + 0] = fmaf(v.x, alpha, bias16[j4 * 4 + 0]); o[j4 * 4 + 1] = fmaf(v.y, alpha, bias16[j4 * 4 + 1]);
        o[j4 * 4 + 2] = fmaf(v.z, alpha, bias16[j4 * 4 + 2]); o[j4 * 4 + 3] = fmaf(v.w, alpha, bias16[j4 * 4 + 3]);
        if (y) *(float4*)(y + pix * Cout + co0 + cq + j4 * 4) = make_float4(o[j4 * 4], o[j4 * 4 + 1], o[j4 * 4 + 2], o[j4 * 4 + 3]);
    }
    if (o_hi) {
        s16x8_t h0, h1, l0, l1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float q0 = o_relu ? fmaxf(o[j], 0.f) : o[j], q1 = o_relu ? fmaxf(o[8 + j], 0.f) : o[8 + j];
            const uint16_t u0 = lp_f32_to_op16<F16>(q0), u1 = lp_f32_to_op16<F16>(q1);
            h0[j] = (short)u0; h1[j] = (short)u1;
            if (X3) {
                l0[j] = (short)lp_f32_to_op16<false>(q0 - lp_op16_to_f32<false>(u0));
                l1[j] = (short)lp_f32_to_op16<false>(q1 - lp_op16_to_f32<false>(u1));
            }
        }
        uint16_t* od = o_hi + pix * Cout + co0 + cq;
        *(s16x8_t*)od = h0; *(s16x8_t*)(od + 8) = h1;
        if (X3) {
            uint16_t* ol = o_lo + pix * Cout + co0 + cq;
            *(s16x8_t*)ol = l0; *(s16x8_t*)(ol + 8) = l1;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Weight gradient with the thin operand in LDS and the wide operand streamed:
//
//   dw[co][ci][tap] = sum_{n,y,x} dy[n,y,x,co] * act(x)[n, y+ky-1, x+kx-1, ci]
//
// One workgroup walks a strided set of 4-row groups.  The thin operand's rows (with the 1-pixel border, zero padded, channels padded to TW = 4 | 8
// = one | two 16-byte LDS words per pixel) are staged in LDS and read back as wave-wide BROADCASTS; the wide operand is streamed from HBM exactly
// once, 64 consecutive channels per wave (256-byte rows); wave w takes the pixels x = w, w+4, ...
//   THIN_X:  thin = input x (no prologue),  wide = dy;                 acc[tap][ci] += dy[p][co] * x[p + tap][ci]
//   !THIN_X: thin = dy (Cout <= 4),  wide = act(x) (AdaIN/ReLU prologue applied on the fly);
//                                                                       acc[tap][co] += act(x)[q][ci] * dy[q - tap][co]
// Partial sums per workgroup go to the workspace, part[wg][tap][slab thin c][wide c], and are reduced in a fixed order by lp_wgrad_rows_reduce
// (conv_thin.hip; deterministic, no atomics).
// ------------------------------------------------------------------------------------------------------------------
struct RowsWgParams {
    const float* x; const float* dy; float* part; float* dw;
    const uint16_t* x16;             // !THIN_X only: the wide operand as a 16-bit-resident fp16 plane [N][H][W][Cin] instead of fp32 x (NULL: fp32)
    float* bpart; float* dbias;      // NULL | [G][Cout] partial column sums of dy (THIN_X only) and the bias gradient they reduce to
    const float* scale; const float* shift;
    int N, H, W, Cin, Cout, pro, G;
};

// Source policies of the thin operand: load(thin, thinC, n, y, x, H, W, v) fills v[0 .. thinC) with the channels of pixel (y, x) of image n, a
// pixel inside the H x W image (the rest of v is zero on entry).  RowsContig: a contiguous NHWC tensor ``thin`` of thinC <= 4 channels.
struct RowsContig {
    __device__ __forceinline__ void load(const float* thin, int thinC, int n, int y, int x, int H, int W, float (&v)[4]) const {
        const float* src = thin + ((size_t)(n * H + y) * W + x) * thinC;
        v[0] = src[0];
        if (thinC > 1) v[1] = src[1];
        if (thinC > 2) v[2] = src[2];
        if (thinC > 3) v[3] = src[3];
    }
};

// TW: staged values per pixel (4 | 8).  FULL: all TW of them are live (else <= TW - 1: the last FMA per tap is skipped).  The cross-wave sum at the
// end runs in rounds of TC taps (TW = 8: 9 x 8 x 4 x 64 floats do not fit LDS); the slab's thin extent is the live channel count for TW = 4 and 8
// (zero padded) for TW = 8.
template <int TW> struct RowsWgGeom {
    static constexpr int RB = 4;
    static constexpr int taps_per_round(int T) { return TW == 4 ? T : 4; }
    static size_t lds_bytes(int ksize, int W) {
        const size_t stage = rows_lds_bytes(RB, ksize / 2, W, TW * 4), red = (size_t)4 * taps_per_round(ksize * ksize) * TW * 64 * sizeof(float);
        return stage > red ? stage : red;
    }
};

template <int KS, bool THIN_X, int TW, bool FULL, class SRC>
__global__ __launch_bounds__(256) void wgrad_rows_kernel(RowsWgParams p, SRC src) {
    constexpr int T = KS * KS, PAD = KS / 2, TC = RowsWgGeom<TW>::taps_per_round(T);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, ph = tid >> 6;
    const int thinC = THIN_X ? p.Cin : p.Cout, wideC = THIN_X ? p.Cout : p.Cin;
    const int slabC = TW == 4 ? thinC : TW;
    const int wc = blockIdx.y * 64 + lane;                               // this lane's channel of the wide operand
    const float* thin = THIN_X ? p.x : p.dy;
    const float* wide = THIN_X ? p.dy : p.x;
    const int RW = p.W + 2 * PAD;                                        // staged row width (pixels)
    float bsum = 0.f;                                                    // THIN_X: column sum of dy (bias gradient)
    float acc[T][TW];             // (scalar FMAs: v_pk_fma_f32 pairs measured 1.4x SLOWER here)
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int c = 0; c < TW; ++c) acc[t][c] = 0.f;

    // a block iteration = RB consecutive rows of one image (+ border rows of the thin operand); the wide operand's loads are
    // issued UB at a time before they are used, so every wave keeps UB x 256 B in flight (the kernel is a pure HBM stream)
    constexpr int RB = RowsWgGeom<TW>::RB, UB = (KS == 1) ? 16 : 8;
    const int gpi = (p.H + RB - 1) / RB;                                 // row groups per image
    for (int grp = blockIdx.x; grp < p.N * gpi; grp += gridDim.x) {
        const int n = grp / gpi, y0 = (grp % gpi) * RB;
        __syncthreads();                                                 // previous group fully consumed
        for (int i = tid; i < (RB + 2 * PAD) * RW; i += 256) {
            const int r = i / RW, hx = i % RW;
            const int iy = y0 + r - PAD, ix = hx - PAD;
            float v[TW];
#pragma unroll
            for (int c = 0; c < TW; ++c) v[c] = 0.f;
            if (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) src.load(thin, thinC, n, iy, ix, p.H, p.W, v);
#pragma unroll
            for (int c = 0; c < TW; c += 4) *(float4*)(sm + (size_t)i * TW + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
        }
        __syncthreads();
        float sc = 1.f, sh = 0.f;
        if (!THIN_X && p.pro == 1) { sc = p.scale[(size_t)n * p.Cin + wc]; sh = p.shift[(size_t)n * p.Cin + wc]; }
        const int nrow = min(RB, p.H - y0);
        const int npx = nrow * p.W;                                      // pixels of the group, row-major; this wave: ph, ph+4, ...
        const float* wbase = wide + (size_t)(n * p.H + y0) * p.W * wideC + wc;
        const uint16_t* wbase16 = (!THIN_X && p.x16) ? p.x16 + (size_t)(n * p.H + y0) * p.W * wideC + wc : nullptr;
        for (int j0 = ph; j0 < npx; j0 += 4 * UB) {
            float av[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + 4 * u;
                if (!THIN_X && wbase16) av[u] = lp_op16_to_f32<true>(wbase16[(size_t)(j < npx ? j : 0) * wideC]);
                else av[u] = wbase[(size_t)(j < npx ? j : 0) * wideC];          // unconditional load, masked below
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int j = j0 + 4 * u;
                float a = av[u];
                if (!THIN_X && p.pro != 0) a = fmaxf(fmaf(a, sc, sh), 0.f);
                a = j < npx ? a : 0.f;
                if (THIN_X) bsum += a;
                const int rr = j / p.W, xx = j - rr * p.W;
                const int jr = j < npx ? rr : 0;
#pragma unroll
                for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        // THIN_X: x pixel (y+ky-1, xx+kx-1) -> staged row rr+ky, column xx+kx.   else: dy pixel (y-ky+1, xx-kx+1)
                        // -> staged row rr+2-ky (rows y0-1..), column xx-kx+2
                        const int r = jr + (THIN_X ? ky : (KS - 1 - ky)), c = THIN_X ? (xx + kx) : (xx + KS - 1 - kx);
                        const float* q = sm + ((size_t)r * RW + c) * TW;
                        float* ac = acc[ky * KS + kx];
#pragma unroll
                        for (int c4 = 0; c4 < TW; c4 += 4) {
                            const float4 v = *(const float4*)(q + c4);
                            ac[c4 + 0] = fmaf(a, v.x, ac[c4 + 0]);
                            ac[c4 + 1] = fmaf(a, v.y, ac[c4 + 1]);
                            ac[c4 + 2] = fmaf(a, v.z, ac[c4 + 2]);
                            if (FULL || c4 + 4 < TW) ac[c4 + 3] = fmaf(a, v.w, ac[c4 + 3]);
                        }
                    }
            }
        }
    }
    // sum the four pixel phases (waves) through LDS, TC taps per round, then one partial slab per workgroup: part[wg][tap][slab c][wide c]
#pragma unroll
    for (int t0 = 0; t0 < T; t0 += TC) {
        __syncthreads();
#pragma unroll
        for (int tt = 0; tt < TC; ++tt)
            if (t0 + tt < T) {
#pragma unroll
                for (int c = 0; c < TW; ++c) sm[((ph * TC + tt) * TW + c) * 64 + lane] = acc[t0 + tt][c];
            }
        __syncthreads();
        for (int i = tid; i < TC * TW * 64; i += 256) {
            const float s = (sm[i] + sm[TC * TW * 64 + i]) + (sm[2 * TC * TW * 64 + i] + sm[3 * TC * TW * 64 + i]);
            const int l = i & 63, c = (i >> 6) & (TW - 1), tt = i / (TW * 64);
            if ((TC == T || t0 + tt < T) && c < slabC) p.part[(((size_t)blockIdx.x * T + t0 + tt) * slabC + c) * wideC + blockIdx.y * 64 + l] = s;
        }
    }
    if (THIN_X && p.bpart) {
        __syncthreads();
        sm[tid] = bsum;
        __syncthreads();
        if (tid < 64) p.bpart[(size_t)blockIdx.x * wideC + blockIdx.y * 64 + tid] = (sm[tid] + sm[64 + tid]) + (sm[128 + tid] + sm[192 + tid]);
    }
}
