"""CPU emulation of the index arithmetic of gconv_rows_kernel (csrc/gconv_rows.hip), every formula restated literally: the weight-fragment
gather from the [9][CP][64] image of lp_pack_grouped (modes 0 and 1), the tap-pair k mapping of the pixel fragments with one MFMA per tap (the other tap's half of K multiplies zero weights), the
LDS-DMA pieces with their XOR-swizzled source channel groups, the halo reads, the MFMA 16x16x32 fragment layouts (weights = A, pixels = B),
the accumulator-to-(pixel, channel) map, the workgroup -> tile walk of the host code and the statistics row-block assignment (that of conv_dma_kernel's 16 x 16 tiles) -- in fp64
against F.conv2d(groups) / F.conv_transpose2d(groups) (gate 1e-12), and every wave-wide halo read in the bank model of
scripts/lds_swizzle_sim.py (4 LDS cycles = conflict free).  No GPU needed.   python scripts/gconv_rows_emu.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lds_swizzle_sim import cycles  # noqa: E402

TH, TW = 4, 16
HH, HW = TH + 2, TW + 2
HALO_PX = HH * HW
PIECES = (HALO_PX * 128 + 1023) // 1024
PLANE_E = PIECES * 512                                  # 16-bit elements of one plane
LANE = np.arange(64)


def key(hp):
    return ((hp >> 1) & 3) << 1


def pack_grouped(w, C, cg, CP, mode):
    """pack_grouped_kernel (csrc/resnext.hip): w [C][cg][9] -> img [9][CP][64]"""
    img = np.zeros((9, CP, 64))
    for t in range(9):
        for row in range(C):
            for cl in range(64):
                other = (row & ~63) + cl
                if other < C and other // cg == row // cg:
                    co, ci = (other, row) if mode else (row, other)
                    ts = 8 - t if mode else t
                    img[t, row, cl] = w[co, ci % cg, ts]
    return img


def mfma(afrag, bfrag, acc):
    """D[m][n] += sum_k A[m][k] B[k][n]; lane l holds A[l & 15][8 (l >> 4) + j], B[8 (l >> 4) + j][l & 15], D[4 (l >> 4) + reg][l & 15]"""
    A = np.zeros((16, 32)); B = np.zeros((32, 16))
    for j in range(8):
        A[LANE & 15, 8 * (LANE >> 4) + j] = afrag[:, j]
        B[8 * (LANE >> 4) + j, LANE & 15] = bfrag[:, j]
    D = A @ B
    for reg in range(4):
        acc[:, reg] += D[4 * (LANE >> 4) + reg, LANE & 15]


def launch_geometry(N, H, W, C, wgs_cap, occ, cus=256):
    """lp_gconv_rows_launch: -> (tiles_x, tiles_y, ntiles, nblk, wgs, xcd, grid)"""
    tiles_x, tiles_y = (W + TW - 1) // TW, (H + TH - 1) // TH
    ntiles = N * tiles_x * tiles_y
    nblk = C // 64
    wgs = (cus * occ + nblk - 1) // nblk
    if wgs_cap > 0 and wgs > wgs_cap:
        wgs = wgs_cap
    wgs = min(wgs, ntiles)
    xcd = 1 if (wgs >= 8 and ntiles >= 16) else 0
    if xcd:
        wgs &= ~7
    return tiles_x, tiles_y, ntiles, nblk, wgs, xcd, nblk * wgs


def emulate(N, H, W, C, cg, mode, wgs_cap=0, occ=4, seed=0):
    rng = np.random.default_rng(seed)
    CP = (C + 127) // 128 * 128
    a = rng.standard_normal((N, H, W, C))
    w = rng.standard_normal((C, cg, 9))
    img = pack_grouped(w, C, cg, CP, mode).reshape(-1)
    af = a.reshape(-1)
    tiles_x, tiles_y, ntiles, nblk, wgs, xcd, grid = launch_geometry(N, H, W, C, wgs_cap, occ)
    y = np.full((N, H, W, C), np.nan)
    written = np.zeros((N, H, W, C), dtype=int)
    patches = W % 16 == 0 and H % 16 == 0                # statistics are offered for whole 16 x 16 patches
    stat_rows = {}                                       # (row block, channel) -> set of pixels (image, y, x)
    worst, longest = 0, 0
    for wg in range(grid):
        if xcd:
            x, j, per = wg & 7, wg >> 3, (ntiles + 7) >> 3
            blk, tstep, t0, tend = j % nblk, wgs >> 3, x * per + j // nblk, min(x * per + per, ntiles)
        else:
            blk, tstep, t0, tend = wg % nblk, wgs, wg // nblk, ntiles
        if t0 >= tend:
            continue
        co0 = blk * 64
        longest = max(longest, len(range(t0, tend, tstep)))
        # weight fragments
        wfrag = np.zeros((4, 5, 64, 8))
        for wave in range(4):
            for s in range(5):
                tap = 2 * s + (LANE >> 5)
                off = (tap * CP + co0 + 16 * wave + (LANE & 15)) * 64 + 16 * wave + 8 * ((LANE >> 4) & 1)
                for j in range(8):
                    wfrag[wave, s, :, j] = np.where(tap < 9, img[np.minimum(off + j, img.size - 1)], 0.0)
        lds = [np.full(PLANE_E, np.nan), np.full(PLANE_E, np.nan)]
        buf = 0
        for t in range(t0, tend, tstep):
            r_ = t
            x0 = (r_ % tiles_x) * TW; r_ //= tiles_x
            y0 = (r_ % tiles_y) * TH; n = r_ // tiles_y
            # LDS-DMA: piece q = 4 k + wave, lane -> halo pixel 8 q + lane / 8, slot lane % 8 <- channel group slot ^ key(pixel)
            for wave in range(4):
                for k in range((PIECES + 3) // 4):
                    q = 4 * k + wave
                    if q >= PIECES:
                        continue
                    hp = q * 8 + (LANE >> 3)
                    hy = np.where(hp < HALO_PX, hp // HW, -(1 << 20)); hx = hp % HW
                    ch = co0 + (((LANE & 7) ^ key(hp)) << 3)
                    iy, ix = y0 - 1 + hy, x0 - 1 + hx
                    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
                    off = np.where(ok, ((n * H + iy) * W + ix) * C + ch, 0)
                    dst = q * 512 + LANE * 8
                    for j in range(8):
                        lds[buf][dst + j] = np.where(ok, af[off + j], 0.0)
            for wave in range(4):
                for r in range(TH):
                    acc = np.zeros((64, 4))
                    for s in range(5):
                        tap = np.minimum(2 * s + (LANE >> 5), 8)
                        hp = (r + tap // 3) * HW + (LANE & 15) + tap % 3
                        boff = hp * 128 + (((2 * wave + ((LANE >> 4) & 1)) ^ key(hp)) << 4)
                        assert boff.max() + 16 <= HALO_PX * 128
                        worst = max(worst, cycles(list(boff)))
                        bfrag = np.stack([lds[buf][boff // 2 + j] for j in range(8)], axis=1)
                        for h in range(2):               # one MFMA per tap, taps in the order 0 .. 8: the other half of K gets zero weights
                            if 2 * s + h <= 8:
                                mfma(np.where(((LANE >> 5) == h)[:, None], wfrag[wave, s], 0.0), bfrag, acc)
                    oy, ox = y0 + r, x0 + (LANE & 15)
                    for lane in range(64):
                        if oy < H and ox[lane] < W:
                            c = co0 + 16 * wave + 4 * (lane >> 4)
                            y[n, oy, ox[lane], c:c + 4] = acc[lane]
                            written[n, oy, ox[lane], c:c + 4] += 1
                            if patches:                  # row block of conv_dma_kernel's 16 x 16 tiles: (patch, row quarter)
                                ty = y0 >> 2
                                rb = ((n * (tiles_y >> 2) + (ty >> 2)) * tiles_x + (x0 >> 4)) * 4 + (ty & 3)
                                for j in range(4):
                                    stat_rows.setdefault((rb, c + j), set()).add((n, oy, int(ox[lane])))
            buf ^= 1
    assert (written == 1).all(), 'every output written exactly once'
    x_t = torch.from_numpy(a).permute(0, 3, 1, 2)
    w_t = torch.from_numpy(w).reshape(C, cg, 3, 3)
    ref = (F.conv_transpose2d(x_t, w_t, None, 1, 1, 0, C // cg) if mode else F.conv2d(x_t, w_t, None, 1, 1, 1, C // cg)).permute(0, 2, 3, 1).numpy()
    err = np.abs(y - ref).max() / np.abs(ref).max()
    if patches:                                          # statistics: [image][H W / 64 row blocks][C], 64 pixels of ONE image each, every pixel once
        rows = H * W // 64
        assert len(stat_rows) == N * rows * C
        for (rb, c), pix in stat_rows.items():
            assert len(pix) == 64 and {q[0] for q in pix} == {rb // rows}, (rb, c)
    return err, worst, longest


CASES = [(1, 2, 2, 64, 4, 0), (3, 5, 7, 128, 8, 0), (2, 16, 16, 128, 4, 0), (1, 8, 24, 64, 16, 0), (1, 12, 20, 192, 4, 0), (4, 16, 16, 256, 8, 0),
         (2, 32, 32, 128, 16, 1), (2, 32, 32, 128, 16, 3), (2, 32, 32, 128, 16, 24)]

if __name__ == '__main__':
    ok = True
    for (N, H, W, C, cg, cap) in CASES:
        for mode in (0, 1):
            err, worst, longest = emulate(N, H, W, C, cg, mode, wgs_cap=cap, occ=2 if mode else 4,      # (workgroups per CU of the bf16x3 / one-plane launch geometry: both are walked, one per pack mode)
                                          seed=N + H + W + C + cg + mode)
            good = err < 1e-12 and worst == 4
            ok &= good
            print(f'({N}, {H}, {W}, {C}, {cg}) wgs cap {cap} mode {mode}: rel err {err:.2e}  worst halo read {worst} LDS cycles  longest walk {longest} tiles  '
                  + ('ok' if good else 'FAILED'), flush=True)
    print('GCONV_ROWS_EMU_OK' if ok else 'GCONV_ROWS_EMU_FAILED')
    sys.exit(0 if ok else 1)
