// Panel sheet of a batch for the training visuals: P image tensors side by side, one row of panels per sample, an optional caption strip on top,
// quantised to uint8 in ONE launch -- what the reference builds on the host with torch.cat over .cpu() copies before TensorBoard quantises it
// (utils/visualize.py: make_visual).
//
// Definition (restated in numpy fp32 and integer arithmetic by tests/visual_sheet_restatement.py, in torch ops by hipops.visual_sheet_host).
// Panel p: logical [N][C_p][H][W] fp32, C_p in {1, 3}, read in place: value(n, c, y, x) = ptr_p[n sn + c sc + y sh + x sw] (element strides, 0 allowed:
//   the [:, 0] view of a 5-D batch tensor, the stride-0 expand of a segmentation).  N, H, W are shared by all panels.
// Caption strip (optional): uint8 [Hc][P W] greys.
// Output: uint8 [Hc + N H][P W][3], contiguous HWC.
//   out[r][j][c]                  = strip[r][j]                          for r < Hc                      (the grey in all three channels)
//   out[Hc + n H + y][p W + x][c] = q(value_p(n, C_p == 3 ? c : 0, y, x))                                (a one-channel panel in all three channels)
// Value rule: q(v) = (uint8) floor(min(max(v, 0), 1) * 255), the multiplication in fp32 -- drive_frames' clamp(0, 1).mul(255).byte().  The clamp
//   returns the bound for NaN (fmaxf / fminf keep the operand that is a number): NaN -> 0; -0.0, a denormal and -inf -> 0; 1 and +inf -> 255.
//
// blockIdx.y is the panel, so its pointer, strides, channel count and load form are uniform over the workgroup.  A lane takes 4 consecutive pixels of
// one output row of that panel: consecutive lanes read consecutive 16 bytes per channel (one 16-byte load where the host found every quad of the panel
// aligned: column stride 1, base and the other strides multiples of 16 bytes, and the quad whole; scalar loads otherwise) and write consecutive
// 12 bytes (three 32-bit words when W % 4 == 0 and the output is 4-byte aligned, bytes otherwise).  Every source index is formed from (n, y, x)
// inside the logical shape.  No LDS, no atomics, no workspace: a pure function of the inputs, bit-identical from run to run, capturable.
#include <stdint.h>
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file, as in its neighbours (augment.hip, image_quality.hip, frames.hip): tests/test_isa_lint.py, spectral_norm.hip.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define VS_MAX_P 12
#define VS_THREADS 256

struct VsPanel { const float* p; long long sn, sc, sh, sw; int C, vec; };
struct VsArgs {
    VsPanel panel[VS_MAX_P];
    const unsigned char* strip;
    unsigned char* out;
    int P, N, H, W, Hc, quads;          // quads = ceil(W / 4)
    long long lanes;                    // (Hc + N H) * quads: the lanes one panel needs
};

__device__ __forceinline__ unsigned vs_q(float v) { return (unsigned)(fminf(fmaxf(v, 0.f), 1.f) * 255.f); }

template <bool WORDS> __global__ void __launch_bounds__(VS_THREADS) visual_sheet_kernel(VsArgs a) {
    const long long lane = (long long)blockIdx.x * VS_THREADS + threadIdx.x;
    if (lane >= a.lanes) return;
    const int p = blockIdx.y;
    const long long r = lane / a.quads;                       // output row
    const int x = (int)(lane - r * a.quads) * 4;              // first column inside the panel
    const int W = a.W, live = min(4, W - x);
    unsigned q[4][3];
    if (r < a.Hc) {
        const unsigned char* __restrict__ s = a.strip + (size_t)r * ((size_t)a.P * W) + (size_t)p * W + x;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i][0] = q[i][1] = q[i][2] = i < live ? s[i] : 0u;
    } else {
        const VsPanel& pn = a.panel[p];
        const long long ry = r - a.Hc;
        const long long n = ry / a.H, y = ry - n * a.H;
        const float* __restrict__ src = pn.p + n * pn.sn + y * pn.sh + (long long)x * pn.sw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (c < pn.C) {
                const float* __restrict__ sc = src + c * pn.sc;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (pn.vec && live == 4) {
                    const float4 t = *(const float4*)sc;
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < live) v[i] = sc[i * pn.sw];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i][c] = vs_q(v[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) q[i][c] = q[i][0];
            }
        }
    }
    unsigned char* __restrict__ o = a.out + ((size_t)r * ((size_t)a.P * W) + (size_t)p * W + x) * 3;
    if (WORDS) {          // W % 4 == 0: the quad is whole, its 12 bytes start at a multiple of 4
        unsigned* __restrict__ o4 = (unsigned*)o;
        o4[0] = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
        o4[1] = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
        o4[2] = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < live) {
                o[3 * i] = (unsigned char)q[i][0]; o[3 * i + 1] = (unsigned char)q[i][1]; o[3 * i + 2] = (unsigned char)q[i][2];
            }
    }
}

extern "C" int lp_visual_sheet(const float* const* panels, const long long* strides, const int* channels, int P, int N, int H, int W,
                               const unsigned char* caption, int Hc, unsigned char* out, void* stream) {
    if (!panels || !strides || !channels || !out) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: null pointer");
    if (P < 1 || P > VS_MAX_P) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: P must be in 1 .. 12");
    if (N < 1) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: N >= 1 is required");
    if (H < 1) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: H >= 1 is required");
    if (W < 1) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: W >= 1 is required");
    if (Hc < 0) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: Hc >= 0 is required");
    if (Hc > 0 && !caption) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: Hc > 0 needs the caption strip (null pointer)");
    VsArgs a;
    for (int p = 0; p < P; ++p) {
        const long long* s = strides + 4 * p;
        if (!panels[p]) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: null pointer (a panel)");
        if (channels[p] != 1 && channels[p] != 3) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: C must be 1 or 3 for every panel");
        if (s[0] < 0 || s[1] < 0 || s[2] < 0 || s[3] < 0) return lp_set_error(LP_ERR_ARG, "lp_visual_sheet: negative stride");
        const bool vec = s[3] == 1 && ((uintptr_t)panels[p] & 15) == 0 && s[0] % 4 == 0 && s[1] % 4 == 0 && s[2] % 4 == 0;
        a.panel[p] = {panels[p], s[0], s[1], s[2], s[3], channels[p], vec ? 1 : 0};
    }
    for (int p = P; p < VS_MAX_P; ++p) a.panel[p] = {nullptr, 0, 0, 0, 0, 1, 0};
    a.strip = caption; a.out = out;
    a.P = P; a.N = N; a.H = H; a.W = W; a.Hc = Hc; a.quads = (W + 3) / 4;
    a.lanes = ((long long)Hc + (long long)N * H) * a.quads;
    const long long blocks = (a.lanes + VS_THREADS - 1) / VS_THREADS;
    if (blocks > 0x7fffffffLL) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_visual_sheet: (Hc + N * H) * W exceeds one launch grid");
    const dim3 grid((unsigned)blocks, (unsigned)P), block(VS_THREADS);
    if (W % 4 == 0 && ((uintptr_t)out & 3) == 0) hipLaunchKernelGGL(visual_sheet_kernel<true>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(visual_sheet_kernel<false>, grid, block, 0, (hipStream_t)stream, a);
    return lp_check_launch("visual_sheet");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
