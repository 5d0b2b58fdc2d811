// Grouped 3x3 conv (stride 1, pad 1) with groups of 4, 8 or 16 channels (ResNeXt conv2 of layers 1-3, forward and data gradient) on
// 16-channel MFMA blocks, with the weights in registers and persistent workgroups that stream pixel tiles.
//
//   y[n,oy,ox,co] = alpha2 * sum_{tap,ci} a[n, oy+dy-1, ox+dx-1, ci] * img[tap][co][ci - 64*(co/64)]
//
// `img` is the [9][CP][64] image of lp_pack_grouped (mode 0: forward, mode 1: data gradient; both are read the same way).  For groups of
// <= 16 channels every group lies inside one aligned 16-channel block, so a 16 (co) x 16 (pixel) output tile contracts over 16 ci x 9 taps
// = 144 values.  The pixel fragments are FIVE reads with K = [tap 2s: 16 ci | tap 2s+1: 16 ci] (the second half of step 4 is unused); each of them
// is multiplied once per tap, with the other tap's half of the weight fragment zeroed: NINE k-steps of the 16x16x32 MFMA, taps in the order 0 .. 8,
// against the 18 that the block-diagonal form of conv_dma.hip spends on the same 16 x 16 outputs.  One MFMA per tap (and not one per tap PAIR,
// which the K layout would allow) keeps the fp32 result of every output equal, bit for bit, to conv_dma_kernel's: the same products enter the
// accumulator in the same groups and order, so training runs do not depend on which of the two kernels a layer ran on.  The statistics partials
// follow the same rule (same 64-pixel row blocks, same order of the shifted sums and merges).  Computed from the shape, the 64 x 64 x 128 launch
// holds about 23 us of bf16x3 matrix-pipe time this way (13 us with five steps) inside a launch that its bytes bound at about 49 us; the measured
// launch times are in DESIGN 4.12.
// As in conv_dma_kernel, where a zero weight meets every channel of a 64-channel block, a zero weight here meets a finite-or-not pixel value: a
// NaN or Inf in one tap's pixel reaches the outputs that read the fragment's other tap (0 x Inf = NaN), and the unused half of step 4 re-reads tap 8.
//
// Operands: the WEIGHTS are the A operand (lane l: row co = l & 15, k-group l >> 4 = (tap 2s + (l >> 5), channel half (l >> 4) & 1)),
// loaded once per wave from the weight image and kept in registers (5 two-tap fragments, x2 in bf16x3); the PIXELS are the B operand (lane l: pixel
// l & 15 of the tile row, shifted by the tap of its k-group).  The accumulator then holds, in lane l, pixel l & 15 and the four consecutive
// output channels 4 (l >> 4) .. +3: one float4 of y per lane, no LDS transpose.
//
// A workgroup (4 waves; wave w owns channels co0 + 16 w .. +15 of the 64-channel block) walks a strided list of 4 x 16 pixel tiles.  The
// (4+2) x (16+2) halo of a tile -- 128 B (64 channels) per pixel and plane -- is staged by LDS-DMA into one of two buffers; the halo of the
// next tile is in flight while this one multiplies and stores.  One `vmcnt(0)` + barrier per tile: the wave's output stores of the previous
// tile share the counter with the DMA and their number depends on the optional outputs, so the wait is a drain, placed where only those
// stores and the (long issued) DMA of the tile about to be multiplied are outstanding.
//
// LDS image of a buffer: pixel hp (row-major in the 6 x 18 halo) owns 128 B = 8 slots of 16 B; slot s holds the 8-channel group
// s ^ (2 * ((hp >> 1) & 3)) -- the key leaves bit 0 (the half a lane's k-group selects) alone.  scripts/gconv_rows_emu.py restates all of
// this index arithmetic and checks every wave-wide read in the bank model of scripts/lds_swizzle_sim.py (4 LDS cycles: conflict free).
#include "lp_common.h"
#include "conv_common.h"
#include "lp_hip.h"
#include "lp_internal.h"

// (the epilogue's float4 arithmetic: keep hipcc from the packed fp32 forms that are wrong beside the LDS-DMA kernels, tests/test_isa_lint.py)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

static __device__ __attribute__((aligned(64))) unsigned int gr_zero_page[16];      // what out-of-image DMA lanes read

// Inside the attribute region the header forms of these (__syncthreads, __shfl_xor, make_float4) stay CALLS: hipcc does not inline a function
// built with other target features.  The same operations from builtins:
static __device__ __forceinline__ void gr_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
static __device__ __forceinline__ float gr_shfl_xor(float v, int lane, int o) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((lane ^ o) << 2, __builtin_bit_cast(int, v)));
}

struct GconvRowsParams {
    const uint16_t* a_hi; const uint16_t* a_lo; const uint16_t* w_hi; const uint16_t* w_lo;
    float* y; uint16_t* o_hi; uint16_t* o_lo; const float* alpha2; float* amax; float* stats;
    int N, H, W, C, CP;
    int tiles_x, tiles_y, ntiles;      // 4 x 16 tiles per image row / column, tiles of the whole batch (order: x, y, image)
    int nblk, wgs, xcd;                // 64-channel blocks; workgroups per block; 1: workgroup id & 7 = XCD, each XCD owns a contiguous tile range
};

namespace gr {
constexpr int TH = 4, TW = 16, HH = TH + 2, HW = TW + 2, HALO_PX = HH * HW;      // 108 halo pixels
constexpr int PIECES = (HALO_PX * 128 + 1023) / 1024;                             // 14 DMA instructions (8 pixels each) per plane
constexpr int PLANE = PIECES * 1024;
constexpr int KIT = (PIECES + 3) / 4;                                             // DMA instructions per wave and plane
__host__ __device__ constexpr int key(int hp) { return ((hp >> 1) & 3) << 1; }
}

template <int PREC>
__global__ __launch_bounds__(256, PREC == LP_PREC_BF16X3 ? 2 : 4) void gconv_rows_kernel(GconvRowsParams p) {
    using namespace gr;
    constexpr bool SPLIT = (PREC == LP_PREC_BF16X3), F16 = (PREC == LP_PREC_F16);
    constexpr int BUF = PLANE * (SPLIT ? 2 : 1);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int kb = lane >> 4, px = lane & 15;

    // ---- workgroup -> (channel block, strided tile list)
    int blk, t0, tstep, tend;
    {
        const int id = (int)blockIdx.x;
        if (p.xcd) {
            const int x = id & 7, j = id >> 3, per = (p.ntiles + 7) >> 3;
            blk = j % p.nblk;
            tstep = p.wgs >> 3;
            t0 = x * per + j / p.nblk;
            tend = min(x * per + per, p.ntiles);
        } else {
            blk = id % p.nblk;
            tstep = p.wgs;
            t0 = id / p.nblk;
            tend = p.ntiles;
        }
    }
    if (t0 >= tend) return;                                  // (uniform)
    const int co0 = blk * 64;

    // ---- the wave's weight fragments: row co0 + 16 w + (l & 15), columns 16 w + 8 ((l >> 4) & 1) .. +7 of tap 2 s + (l >> 5)
    s16x8_t whi[5], wlo[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int tap = 2 * s + (lane >> 5);
        whi[s] = (s16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        wlo[s] = (s16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        if (tap < 9) {
            const size_t off = ((size_t)tap * p.CP + co0 + 16 * wave + px) * 64 + 16 * wave + 8 * (kb & 1);
            whi[s] = *(const s16x8_t*)(p.w_hi + off);
            if (SPLIT) wlo[s] = *(const s16x8_t*)(p.w_lo + off);
        }
    }
    const float alpha = p.alpha2 ? *p.alpha2 : 1.f;

    // ---- halo read offsets: tile row r, step s -> halo pixel (r + dy) * 18 + (l & 15) + dx of the lane's tap (the zero half of step 4 reads
    // tap 8 again: finite data times the zero weights), channel group 2 w + ((l >> 4) & 1)
    int r_off[TH][5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int tap = min(2 * s + (lane >> 5), 8);
#pragma unroll
        for (int r = 0; r < TH; ++r) {
            const int hp = (r + tap / 3) * HW + px + tap % 3;
            r_off[r][s] = hp * 128 + (((2 * wave + (kb & 1)) ^ key(hp)) << 4);
        }
    }

    // ---- halo DMA geometry (tile independent): piece q = 4 k + wave covers halo pixels 8 q .. 8 q + 7; lane -> pixel 8 q + lane / 8, slot lane % 8
    int d_hy[KIT], d_hx[KIT], d_c[KIT];
#pragma unroll
    for (int k = 0; k < KIT; ++k) {
        const int hp = (4 * k + wave) * 8 + (lane >> 3);
        d_hy[k] = hp < HALO_PX ? hp / HW : -(1 << 20);        // (pixels past the halo: always out of the image -> zero page)
        d_hx[k] = hp % HW;
        d_c[k] = co0 + (((lane & 7) ^ key(hp)) << 3);
    }
    const uint16_t* zero16 = (const uint16_t*)gr_zero_page;
    const unsigned lds0 = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(uintptr_t)smem);
    auto decode = [&](int t, int& n, int& y0, int& x0) {
        x0 = (t % p.tiles_x) * TW; t /= p.tiles_x;
        y0 = (t % p.tiles_y) * TH; n = t / p.tiles_y;
    };
    auto issue = [&](int t, int buf) {
        int n, y0, x0;
        decode(t, n, y0, x0);
#pragma unroll
        for (int k = 0; k < KIT; ++k) {
            const int q = 4 * k + wave;
            if (q < PIECES) {                                 // (wave-uniform)
                const int iy = y0 - 1 + d_hy[k], ix = x0 - 1 + d_hx[k];
                const bool ok = iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
                const size_t off = ok ? ((size_t)(n * p.H + iy) * p.W + ix) * p.C + d_c[k] : 0;
                const unsigned d = lds0 + (unsigned)(buf * BUF + q * 1024);
                lp_glds16(ok ? (p.a_hi + off) : zero16, d);
                if (SPLIT) lp_glds16(ok ? (p.a_lo + off) : zero16, d + PLANE);
            }
        }
    };

    float am = 0.f;
    issue(t0, 0);
    int buf = 0;
    for (int t = t0; t < tend; t += tstep, buf ^= 1) {
        lp_wait_vm0();                                       // this wave's pieces of tile t have landed (and its stores of the previous tile)
        gr_barrier();                                        // ... everybody's; and every wave is done reading the other buffer
        if (t + tstep < tend) issue(t + tstep, buf ^ 1);
        int n, y0, x0;
        decode(t, n, y0, x0);
        const unsigned char* Hb = smem + buf * BUF;
        float st_ref[4] = {0.f, 0.f, 0.f, 0.f}, st_d[4] = {0.f, 0.f, 0.f, 0.f}, st_q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < TH; ++r) {
            f32x4_t acc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            int lhalf = lane >> 5;
            asm volatile("" : "+v"(lhalf));                  // (opaque per row: the masked fragments below are made where they are used, not kept in 72 more registers)
            // One MFMA (three in bf16x3) PER TAP, taps in the order 0 .. 8, the tap's 16 channels in one half of K and zero weights in the other:
            // every output then receives its products in the groups and in the order in which conv_dma_kernel's block-diagonal form adds them
            // (tap by tap: lo x hi, hi x lo, hi x hi), so y is the same fp32 number bit for bit and the step computes what it computed before.
            // The pixel fragment of step s already holds tap 2 s in its low and tap 2 s + 1 in its high lanes: one LDS read serves both taps.
#pragma unroll
            for (int s = 0; s < 5; ++s) {
                const s16x8_t bh = *(const s16x8_t*)(Hb + r_off[r][s]);
                s16x8_t bl;
                if (SPLIT) bl = *(const s16x8_t*)(Hb + PLANE + r_off[r][s]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    if (2 * s + h > 8) continue;
                    const s16x8_t zero = (s16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
                    const s16x8_t mh = (lhalf == h) ? whi[s] : zero;
                    if (SPLIT) {
                        const s16x8_t ml = (lhalf == h) ? wlo[s] : zero;
                        acc = mfma16t<false>(mh, bl, acc);
                        acc = mfma16t<false>(ml, bh, acc);
                    }
                    acc = mfma16t<F16>(mh, bh, acc);
                }
            }
            const int oy = y0 + r, ox = x0 + px;
            float4 v;
            v.x = fmaf(acc[0], alpha, 0.f); v.y = fmaf(acc[1], alpha, 0.f); v.z = fmaf(acc[2], alpha, 0.f); v.w = fmaf(acc[3], alpha, 0.f);
            if (p.stats) {
                // shifted sums in the order of conv16_epilogue, whose lane (channel quad, rsub) walks the pixels (py, 4 k + rsub), py outer: here the
                // four lanes px = 4 k + rsub hold them, and each of them runs the whole sequence (whole 16 x 16 patches only: every lane is live)
                const float o4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xv = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((lane & 48) | (4 * k + (px & 3))) << 2, __builtin_bit_cast(int, o4[j])));
                        if (r == 0 && k == 0) st_ref[j] = xv;
                        const float d = xv - st_ref[j];
                        st_d[j] += d; st_q[j] = fmaf(d, d, st_q[j]);
                    }
            }
            if (oy < p.H && ox < p.W) {
                const size_t e = (((size_t)n * p.H + oy) * p.W + ox) * p.C + co0 + 16 * wave + 4 * kb;
                if (p.y) *(float4*)(p.y + e) = v;
                am = lp_amax4(am, v);
                if (p.o_hi) {
                    const float o[4] = {v.x, v.y, v.z, v.w};
                    ushort4 oh, ol;
                    uint16_t* ohp = (uint16_t*)&oh; uint16_t* olp = (uint16_t*)&ol;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        ohp[j] = lp_f32_to_op16<F16>(o[j]);
                        if (SPLIT) olp[j] = lp_f32_to_op16<false>(o[j] - lp_op16_to_f32<false>(ohp[j]));
                    }
                    *(ushort4*)(p.o_hi + e) = oh;
                    if (SPLIT) *(ushort4*)(p.o_lo + e) = ol;
                }
            }
        }
        if (p.stats) {
            // lane: {16, mean, M2} of its 4 channels over the 16 pixels px = rsub (mod 4) of the tile; rsub 0 merges rsub 1, then the pair 2, 3
            // (Chan et al., equal counts), as conv16_epilogue's lanes do; pixel lane 0 writes the wave's 16 channels of the row block that
            // conv_dma_kernel's 16 x 16 tile gives these 64 pixels: (16 x 16 patch, row quarter) -- same partials, same place, same bits
            float cnt = 16.f, mean[4], m2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { mean[j] = st_ref[j] + st_d[j] / cnt; m2[j] = fmaxf(st_q[j] - st_d[j] * st_d[j] / cnt, 0.f); }
#pragma unroll
            for (int o = 1; o < 4; o <<= 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float mb = gr_shfl_xor(mean[j], lane, o), qb = gr_shfl_xor(m2[j], lane, o);
                    const float d = mb - mean[j];
                    mean[j] = fmaf(d, 0.5f, mean[j]); m2[j] += qb + d * d * (cnt * 0.5f);
                }
                cnt *= 2.f;
            }
            if (px == 0) {
                const int ty = y0 >> 2;
                const int rb = ((n * (p.tiles_y >> 2) + (ty >> 2)) * p.tiles_x + (x0 >> 4)) * 4 + (ty & 3);
                float* o = p.stats + ((size_t)rb * p.C + co0 + 16 * wave + 4 * kb) * 3;
#pragma unroll
                for (int j = 0; j < 4; ++j) { o[j * 3 + 0] = cnt; o[j * 3 + 1] = mean[j]; o[j * 3 + 2] = m2[j]; }
            }
        }
    }
    if (p.amax) lp_amax_commit(am, p.amax, blockIdx.x);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// -> 1: launched; 0: this layer stays on conv_dma_kernel; < 0: error.  p: the parameter block lp_gconv16_fwd_planes filled (p.stats /
// p.stats_rows are updated as launch_conv16 does: statistics the geometry does not cover are dropped and reported as 0 rows).
int lp_gconv_rows_launch(Conv16Params& c, int group_size, int prec, hipStream_t s) {
    const int mode = lp_knobs().gconv_rows, wgs_cap = lp_knobs().gconv_rows_wgs;
    if (mode == 0 || !(group_size == 4 || group_size == 8 || group_size == 16)) return 0;
    if (prec != LP_PREC_BF16 && prec != LP_PREC_BF16X3 && prec != LP_PREC_F16) return 0;
    const bool exact = (c.W % gr::TW == 0) && (c.H % gr::TH == 0);      // whole 4 x 16 tiles: nothing multiplied for nothing, one tile = one statistics row block
    if (mode != 2 && !exact) return 0;
    const bool patches = (c.W % 16 == 0) && (c.H % 16 == 0);            // statistics: the row blocks and sums of conv_dma_kernel's 16 x 16 tiles
    if (c.stats && !patches && (c.H * c.W) % 64 == 0) return 0;         // (maps whose statistics the old route may cover otherwise)
    GconvRowsParams p;
    p.a_hi = c.a_hi; p.a_lo = c.a_lo; p.w_hi = c.w_hi; p.w_lo = c.w_lo; p.y = c.y; p.o_hi = c.o_hi; p.o_lo = c.o_lo; p.alpha2 = c.alpha2; p.amax = c.amax;
    p.N = c.N; p.H = c.H; p.W = c.W; p.C = c.Cout; p.CP = c.CoutP;
    p.tiles_x = (c.W + gr::TW - 1) / gr::TW; p.tiles_y = (c.H + gr::TH - 1) / gr::TH; p.ntiles = c.N * p.tiles_x * p.tiles_y;
    p.nblk = c.Cout / 64;
    c.stats_rows = 0;
    if (c.stats) {
        const long long rows = (long long)c.N * (c.H * c.W / 64);
        if (patches && rows * c.Cout * 3 <= c.stats_cap) c.stats_rows = c.H * c.W / 64; else c.stats = nullptr;
    }
    p.stats = c.stats;
    // workgroups: enough to fill the chip at the kernel's occupancy (bf16x3: 2 per CU, 56 KB of LDS each; one-plane modes: 4, <= 128 registers)
    const int occ = prec == LP_PREC_BF16X3 ? 2 : 4;
    static int cus = 0;
    if (!cus) { int dev = 0; if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256; }
    int wgs = (cus * occ + p.nblk - 1) / p.nblk;
    if (wgs_cap > 0 && wgs > wgs_cap) wgs = wgs_cap;
    if (wgs > p.ntiles) wgs = p.ntiles;
    p.xcd = (wgs >= 8 && p.ntiles >= 16) ? 1 : 0;
    if (p.xcd) wgs &= ~7;
    p.wgs = wgs;
    const dim3 grid((unsigned)(p.nblk * wgs));
    const size_t lds = 2 * gr::PLANE * (prec == LP_PREC_BF16X3 ? 2 : 1);
    if (prec == LP_PREC_BF16X3) hipLaunchKernelGGL(gconv_rows_kernel<LP_PREC_BF16X3>, grid, dim3(256), lds, s, p);
    else if (prec == LP_PREC_F16) hipLaunchKernelGGL(gconv_rows_kernel<LP_PREC_F16>, grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(gconv_rows_kernel<LP_PREC_BF16>, grid, dim3(256), lds, s, p);
    const int rc = lp_check_launch("gconv_rows");
    return rc ? rc : 1;
}
