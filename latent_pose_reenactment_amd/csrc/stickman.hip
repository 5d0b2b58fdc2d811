// Stickman rasteriser of the keypoint-driven (FSTH) family: [N][P][2] keypoints in [0, 1] -> [N][3][S][S] images, every polyline segment a soft line
// (1 on the segment, falling to 0 over `width` pixels), one colour per part, parts combined by a per-channel maximum -- the definition of
// dataloaders/synthetic_voxceleb2_stickmen.draw_stickman, with the polyline table (segments, part runs, colours) as an argument.
//
// One workgroup = one image x 256 "quads" (4 consecutive pixels of a row; a row has ceil(S / 4) of them).  The image's segments are staged in LDS once
// as (a, b - a, 1 / max(|b - a|^2, 1e-12)) in pixel units; every lane then walks the same segment at the same time (LDS broadcast reads), keeps the
// minimum SQUARED distance of a part for its four pixels, and takes one sqrt per part.  No atomics, no cross-lane traffic: the result is a pure function
// of the inputs.  Each lane stores its quad with one 16-byte store per colour plane when S % 4 == 0 (and `out` is 16-byte aligned); otherwise
// pixel by pixel.
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file: four pixels times one broadcast segment is exactly the "pair times a scalar" shape for which hipcc picks
// v_pk_*_f32 with op_sel:[0,1] (wrong beside the LDS-DMA convolution kernels on gfx950: tests/test_isa_lint.py, spectral_norm.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define STICK_MAX_POINTS 256
#define STICK_MAX_SEGS 256
#define STICK_MAX_PARTS 16
#define STICK_THREADS 256

template <bool VEC> __global__ void __launch_bounds__(STICK_THREADS)
stickman_kernel(const float* __restrict__ points, int P, const int* __restrict__ seg, const int* __restrict__ part_end, const float* __restrict__ colour,
                int L, int parts, int S, int tiles, float inv_width, float* __restrict__ out) {
    __shared__ float4 s_seg[STICK_MAX_SEGS];          // ax, ay, bx - ax, by - ay (pixels)
    __shared__ float s_inv[STICK_MAX_SEGS];           // 1 / max(|b - a|^2, 1e-12)
    __shared__ int s_end[STICK_MAX_PARTS];
    __shared__ float s_col[STICK_MAX_PARTS * 3];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const float scale = (float)(S - 1);
    if (tid < L) {
        // (indices are the caller's to check; clamped here so that a bad table reads a wrong point, never memory outside the image's points)
        const int ia = min(max(seg[2 * tid], 0), P - 1), ib = min(max(seg[2 * tid + 1], 0), P - 1);
        const float* pn = points + (size_t)n * P * 2;
        const float ax = pn[2 * ia] * scale, ay = pn[2 * ia + 1] * scale;
        const float bx = pn[2 * ib] * scale, by = pn[2 * ib + 1] * scale;
        const float dx = bx - ax, dy = by - ay;
        s_seg[tid] = make_float4(ax, ay, dx, dy);
        s_inv[tid] = 1.f / fmaxf(dx * dx + dy * dy, 1e-12f);
    }
    if (tid < parts) s_end[tid] = min(max(part_end[tid], 0), L);
    if (tid < parts * 3) s_col[tid] = colour[tid];
    __syncthreads();

    const int Q = (S + 3) >> 2;                         // quads per row
    const long long q = (long long)tile * STICK_THREADS + tid;
    if (q >= (long long)S * Q) return;
    const int y = (int)(q / Q), x0 = (int)(q - (long long)y * Q) * 4;
    const float py = (float)y;
    float px[4], r[4], g[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { px[i] = (float)(x0 + i); r[i] = g[i] = b[i] = 0.f; }

    int s = 0;
    for (int part = 0; part < parts; ++part) {
        const int end = s_end[part];
        float m[4] = {3.0e38f, 3.0e38f, 3.0e38f, 3.0e38f};          // minimum squared distance to the part's segments
        for (; s < end; ++s) {
            const float4 sg = s_seg[s];
            const float inv = s_inv[s];
            const float ey = py - sg.y, eyd = ey * sg.w;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ex = px[i] - sg.x;
                const float t = fminf(fmaxf((ex * sg.z + eyd) * inv, 0.f), 1.f);
                const float cx = ex - t * sg.z, cy = ey - t * sg.w;
                m[i] = fminf(m[i], cx * cx + cy * cy);
            }
        }
        const float cr = s_col[3 * part], cg = s_col[3 * part + 1], cb = s_col[3 * part + 2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float line = fminf(fmaxf(1.f - sqrtf(m[i]) * inv_width, 0.f), 1.f);          // (an empty part: sqrt(3e38) * inv_width -> 0)
            r[i] = fmaxf(r[i], line * cr); g[i] = fmaxf(g[i], line * cg); b[i] = fmaxf(b[i], line * cb);
        }
    }

    const size_t plane = (size_t)S * S;
    float* o = out + (size_t)n * 3 * plane + (size_t)y * S + x0;
    if (VEC) {          // S % 4 == 0: the quad is whole and 16-byte aligned
        *(float4*)o = make_float4(r[0], r[1], r[2], r[3]);
        *(float4*)(o + plane) = make_float4(g[0], g[1], g[2], g[3]);
        *(float4*)(o + 2 * plane) = make_float4(b[0], b[1], b[2], b[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x0 + i < S) { o[i] = r[i]; o[plane + i] = g[i]; o[2 * plane + i] = b[i]; }
    }
}

extern "C" int lp_stickman_render(const float* points, int N, int P, const int* seg, const int* part_end, const float* colour, int L, int parts, int S,
                                  float width, float* out, void* stream) {
    if (!points || !seg || !part_end || !colour || !out) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: null pointer");
    if (N < 1) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: N >= 1 is required");
    if (P < 1 || P > STICK_MAX_POINTS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: P must be in 1 .. 256");
    if (L < 1 || L > STICK_MAX_SEGS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: L must be in 1 .. 256");
    if (parts < 1 || parts > STICK_MAX_PARTS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: parts must be in 1 .. 16");
    if (S < 1) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: S >= 1 is required");
    if (!(width > 0.f)) return lp_set_error(LP_ERR_ARG, "lp_stickman_render: width > 0 is required");
    const long long quads = (long long)S * ((S + 3) / 4);
    const long long tiles = (quads + STICK_THREADS - 1) / STICK_THREADS;
    if (tiles * N > 0x7fffffffLL) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stickman_render: N * S * S exceeds one launch grid");
    const bool vec = S % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)(tiles * N)), block(STICK_THREADS);
    if (vec) hipLaunchKernelGGL(stickman_kernel<true>, grid, block, 0, (hipStream_t)stream, points, P, seg, part_end, colour, L, parts, S, (int)tiles,
                                1.f / width, out);
    else hipLaunchKernelGGL(stickman_kernel<false>, grid, block, 0, (hipStream_t)stream, points, P, seg, part_end, colour, L, parts, S, (int)tiles,
                            1.f / width, out);
    return lp_check_launch("stickman_render");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
