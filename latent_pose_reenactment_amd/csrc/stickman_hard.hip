// Hard-edged stickman rasteriser of the keypoint loaders (dataloaders/voxceleb2.py, dataloaders/voxceleb2_FSTH_crop.py): [N][P][2] keypoints in
// [0, 1] -> [N][3][S][S] images, the reference's SampleLoader.draw_stickman (consecutive cv2.polylines calls of thickness T on rounded integer
// keypoints) restated so that every step is exact in integers.  cv2 is not the definition: this text is (tests/stickman_hard_restatement.py restates
// it with Python integers; hipops.stickman_render_hard_host with numpy integers).
//
// DEFINITION
//   The integer point.  A coordinate x (fp32) becomes X = clamp(rint(x * S)) with the product formed in fp32, the rounding half to even (rintf) and
//   the clamp to [-4096, 8191] (S <= 4096).  A NaN maps to the lower bound -4096: the clamp is written `r >= -4096 ? min(r, 8191) : -4096`, whose
//   comparison is false for a NaN (+inf -> 8191, -inf -> -4096).  With pixels in [0, 4095] every coordinate difference is below 2^14 in magnitude,
//   so d.d, e.d, d x e and 4 |e|^2 below fit int32 (|d.d| <= 2 * 12287^2 < 2^29); only 4 (d x e)^2 (< 2^60) and T^2 (d.d) need 64 bits.
//   Coverage.  Pixel P = (u, v) = (column, row), segment A -> B, d = B - A, e = P - A, L2 = d.d, s = e.d, thickness T.  The segment covers P iff
//       4 |e|^2 <= T^2                          when L2 = 0 or s <= 0      (round cap at A)
//       4 |P - B|^2 <= T^2                      when s >= L2               (round cap at B)
//       4 (d_x e_y - d_y e_x)^2 <= T^2 L2       otherwise                  (the body)
//   i.e. the distance from P to the segment is at most T / 2.
//   Colour.  A pixel takes the colour of the LAST part in table order with a covering segment (painter's order: consecutive polylines calls
//   overwrite), 0 where none covers it.  Output fp32 [N][3][S][S]; with colours in {0, 1} every value is exactly 0 or 1.
//
// KERNEL.  One workgroup = one image x 256 "quads" (4 consecutive pixels of a row; a row has ceil(S / 4) of them), as in stickman.hip.  While staging,
// thread l < L rounds the two ends of segment l and tests the segment's bounding box, grown by ceil(T / 2), against the rows the workgroup covers and
// the columns of the image (32-bit compares); the survivors are compacted IN ORDER into LDS (wave ballots + a prefix over the four waves' counts),
// each as three 16-byte records: (ax, ay, dx, dy), (L2, part, K) and the grown box.  K = floor(sqrt(floor(T^2 L2 / 4))), found ONCE per segment
// while staging (double sqrt, corrected in 64-bit integers): for an integer c, 4 c^2 <= T^2 L2 iff c^2 <= floor(T^2 L2 / 4) iff |c| <= K, so the
// body's test is one 32-bit compare per pixel and no lane pays a 64-bit multiply; likewise 4 |e|^2 <= T^2 iff |e|^2 <= floor(T^2 / 4).  Every lane
// then walks the compacted list -- all lanes read the same record at the same time (LDS broadcast) -- and rejects a segment on its quad's box before
// any multiply.  The products that are left have operands below 2^14: 24-bit multiplies (full rate).  No atomics, no workspace, no cross-lane
// traffic beyond the ballots: bit-identical from run to run, capturable.  One 16-byte store per colour plane when S % 4 == 0 and `out` is 16-byte
// aligned; otherwise pixel by pixel.
#include "lp_hip.h"
#include "lp_common.h"
#include "lp_internal.h"

// No packed fp32 arithmetic in this file either (stickman.hip; tests/test_isa_lint.py): the fp32 that is left is the point's product and rounding.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#define HARD_MAX_POINTS 256
#define HARD_MAX_SEGS 256
#define HARD_MAX_PARTS 16
#define HARD_THREADS 256
#define HARD_MAX_S 4096
#define HARD_MAX_T 8
#define HARD_LO (-4096.f)
#define HARD_HI 8191.f

__device__ __forceinline__ int hard_point(float x, float fs) {
    const float r = rintf(x * fs);
    return (int)(r >= HARD_LO ? fminf(r, HARD_HI) : HARD_LO);          // (false for a NaN: the lower bound)
}

template <bool VEC> __global__ void __launch_bounds__(HARD_THREADS)
stickman_hard_kernel(const float* __restrict__ points, int P, const int* __restrict__ seg, const int* __restrict__ part_end,
                     const float* __restrict__ colour, int L, int parts, int S, int tiles, int T, float* __restrict__ out) {
    __shared__ int4 s_a[HARD_MAX_SEGS];               // ax, ay, dx, dy
    __shared__ int4 s_b[HARD_MAX_SEGS];               // L2, part, K = floor(sqrt(floor(T^2 L2 / 4))), unused
    __shared__ int4 s_box[HARD_MAX_SEGS];             // min x - h, max x + h, min y - h, max y + h with h = ceil(T / 2)
    __shared__ int s_end[HARD_MAX_PARTS];
    __shared__ float s_col[HARD_MAX_PARTS * 3];
    __shared__ int s_cnt[HARD_THREADS / 64];
    const int tid = threadIdx.x;
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    const int Q = (S + 3) >> 2;                         // quads per row
    const int T2 = T * T, R = T2 >> 2, h = (T + 1) >> 1;          // R: |e|^2 <= R iff 4 |e|^2 <= T^2
    const long long q_first = (long long)tile * HARD_THREADS;
    const long long q_last = min(q_first + HARD_THREADS, (long long)S * Q) - 1;
    const int row_first = (int)(q_first / Q), row_last = (int)(q_last / Q);          // the rows this workgroup covers

    if (tid < parts) s_end[tid] = min(max(part_end[tid], 0), L);
    if (tid < parts * 3) s_col[tid] = colour[tid];
    __syncthreads();

    bool keep = false;
    int4 a = make_int4(0, 0, 0, 0), b = a, box = a;
    if (tid < L) {
        // (indices are the caller's to check; clamped here so that a bad table reads a wrong point, never memory outside the image's points)
        const int ia = min(max(seg[2 * tid], 0), P - 1), ib = min(max(seg[2 * tid + 1], 0), P - 1);
        const float* pn = points + (size_t)n * P * 2;
        const float fs = (float)S;
        const int ax = hard_point(pn[2 * ia], fs), ay = hard_point(pn[2 * ia + 1], fs);
        const int bx = hard_point(pn[2 * ib], fs), by = hard_point(pn[2 * ib + 1], fs);
        const int dx = bx - ax, dy = by - ay;
        const int L2 = dx * dx + dy * dy;
        int part = 0;
        while (part < parts - 1 && tid >= s_end[part]) ++part;
        a = make_int4(ax, ay, dx, dy);
        box = make_int4(min(ax, bx) - h, max(ax, bx) + h, min(ay, by) - h, max(ay, by) + h);
        keep = tid < s_end[parts - 1] && box.w >= row_first && box.z <= row_last && box.y >= 0 && box.x <= S - 1;
        if (keep) {          // (only a segment that can touch this workgroup's rows pays for its threshold)
            const unsigned long long m = ((unsigned long long)T2 * (unsigned long long)L2) >> 2;          // < 2^33: exact in a double
            unsigned long long K = (unsigned long long)sqrt((double)m);
            while (K * K > m) --K;                          // (the double sqrt may be one off at a perfect square's edge: settled in integers)
            while ((K + 1) * (K + 1) <= m) ++K;
            b = make_int4(L2, part, (int)K, 0);
        }
    }
    const unsigned long long mask = __ballot(keep);
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, count = 0;
#pragma unroll
    for (int w = 0; w < HARD_THREADS / 64; ++w) {
        const int c = s_cnt[w];
        if (w < wave) base += c;
        count += c;
    }
    if (keep) {
        const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
        s_a[pos] = a; s_b[pos] = b; s_box[pos] = box;
    }
    __syncthreads();

    const long long q = q_first + tid;
    if (q > q_last) return;
    const int y = (int)(q / Q), x0 = (int)(q - (long long)y * Q) * 4;
    int hit[4] = {-1, -1, -1, -1};          // the last part that covers the pixel

    for (int s = 0; s < count; ++s) {
        const int4 bb = s_box[s];
        if (y < bb.z || y > bb.w || x0 + 3 < bb.x || x0 > bb.y) continue;
        const int4 sa = s_a[s], sb = s_b[s];
        const int dx = sa.z, dy = sa.w, L2 = sb.x, part = sb.y, K = sb.z;
        const int ey = y - sa.y, fy = ey - dy;
        const int eyd = __mul24(ey, dy), dxey = __mul24(dx, ey), ey2 = __mul24(ey, ey), fy2 = __mul24(fy, fy);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ex = x0 + i - sa.x;
            const int sdot = __mul24(ex, dx) + eyd;
            const int cross = dxey - __mul24(dy, ex);
            const bool at_a = sdot <= 0;                                     // (L2 = 0: d = 0, so s = 0 and the first case applies)
            const int px = at_a ? ex : ex - dx, py2 = at_a ? ey2 : fy2;          // the cap's centre: A, else B
            const bool cap = __mul24(px, px) + py2 <= R;
            const bool body = abs(cross) <= K;
            const bool covered = (at_a || sdot >= L2) ? cap : body;
            if (covered) hit[i] = part;
        }
    }

    float r[4], g[4], bl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = hit[i];
        r[i] = p < 0 ? 0.f : s_col[3 * p]; g[i] = p < 0 ? 0.f : s_col[3 * p + 1]; bl[i] = p < 0 ? 0.f : s_col[3 * p + 2];
    }
    const size_t plane = (size_t)S * S;
    float* o = out + (size_t)n * 3 * plane + (size_t)y * S + x0;
    if (VEC) {          // S % 4 == 0: the quad is whole and 16-byte aligned
        *(float4*)o = make_float4(r[0], r[1], r[2], r[3]);
        *(float4*)(o + plane) = make_float4(g[0], g[1], g[2], g[3]);
        *(float4*)(o + 2 * plane) = make_float4(bl[0], bl[1], bl[2], bl[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x0 + i < S) { o[i] = r[i]; o[plane + i] = g[i]; o[2 * plane + i] = bl[i]; }
    }
}

extern "C" int lp_stickman_render_hard(const float* points, int N, int P, const int* seg, const int* part_end, const float* colour, int L, int parts,
                                       int S, int T, float* out, void* stream) {
    if (!points || !seg || !part_end || !colour || !out) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: null pointer");
    if (N < 1) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: N >= 1 is required");
    if (P < 1 || P > HARD_MAX_POINTS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: P must be in 1 .. 256");
    if (L < 1 || L > HARD_MAX_SEGS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: L must be in 1 .. 256");
    if (parts < 1 || parts > HARD_MAX_PARTS) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: parts must be in 1 .. 16");
    if (S < 1 || S > HARD_MAX_S) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: S must be in 1 .. 4096");
    if (T < 1 || T > HARD_MAX_T) return lp_set_error(LP_ERR_ARG, "lp_stickman_render_hard: thickness T must be in 1 .. 8");
    const long long quads = (long long)S * ((S + 3) / 4);
    const long long tiles = (quads + HARD_THREADS - 1) / HARD_THREADS;
    if (tiles * N > 0x7fffffffLL) return lp_set_error(LP_ERR_UNSUPPORTED, "lp_stickman_render_hard: N * S * S exceeds one launch grid");
    const bool vec = S % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const dim3 grid((unsigned)(tiles * N)), block(HARD_THREADS);
    if (vec) hipLaunchKernelGGL(stickman_hard_kernel<true>, grid, block, 0, (hipStream_t)stream, points, P, seg, part_end, colour, L, parts, S,
                                (int)tiles, T, out);
    else hipLaunchKernelGGL(stickman_hard_kernel<false>, grid, block, 0, (hipStream_t)stream, points, P, seg, part_end, colour, L, parts, S,
                            (int)tiles, T, out);
    return lp_check_launch("stickman_render_hard");
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
