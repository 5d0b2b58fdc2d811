"""Restatement of the panel sheet of the training visuals (the yardstick of tests/test_visual_sheet_cpu.py and tests/test_visual_sheet_gpu.py), written
from the definition in the header comment of csrc/visual_sheet.hip, in numpy fp32 and integer arithmetic -- one pixel at a time where the layout is
concerned, so that it shares no indexing trick with the kernel or with hipops.visual_sheet_host.

  q(v) = (uint8) floor(min(max(v, 0), 1) * 255), the product rounded once to fp32; NaN -> 0.
  out[r][j][c]                  = strip[r][j]                               r < Hc
  out[Hc + n H + y][p W + x][c] = q(panel_p[n][C_p == 3 ? c : 0][y][x])"""
import numpy as np

F = np.float32


def quantise(x):
    """the value rule on an array of any shape -> uint8"""
    x = np.asarray(x, dtype=F)
    v = np.where(np.isnan(x), F(0), x)          # the clamp of the definition returns the bound for NaN
    v = np.minimum(np.maximum(v, F(0)), F(1))
    prod = (v * F(255)).astype(F)               # one fp32 multiplication
    return np.floor(prod).astype(np.int64).astype(np.uint8)


def sheet(panels, caption=None):
    """panels: arrays [N, C, H, W] (C in {1, 3}); caption: uint8 [Hc, P W] or None -> uint8 [Hc + N H, P W, 3]"""
    panels = [np.asarray(p, dtype=F) for p in panels]
    n, _, h, w = panels[0].shape
    hc = 0 if caption is None else int(caption.shape[0])
    out = np.zeros((hc + n * h, len(panels) * w, 3), dtype=np.uint8)
    for r in range(hc):
        for j in range(len(panels) * w):
            for c in range(3):
                out[r, j, c] = caption[r, j]
    for p, img in enumerate(panels):
        q = quantise(img)
        for s in range(n):
            for y in range(h):
                for x in range(w):
                    for c in range(3):
                        out[hc + s * h + y, p * w + x, c] = q[s, c if img.shape[1] == 3 else 0, y, x]
    return out


def boundary_values():
    """for every k in 0 .. 255 the fp32 value nearest k / 255 and its two fp32 neighbours -> float32 [256, 3] (below, nearest, above)"""
    rows = []
    for k in range(256):
        c = F(k / 255.0)
        rows.append([np.nextafter(c, F(-np.inf), dtype=F), c, np.nextafter(c, F(np.inf), dtype=F)])
    return np.array(rows, dtype=F)


DENORMAL = F(1e-42)
SPECIALS = np.array([0.0, 1.0, -3.0, np.inf, -np.inf, np.nan, -0.0, DENORMAL], dtype=F)
SPECIALS_Q = np.array([0, 255, 0, 255, 0, 0, 0, 0], dtype=np.uint8)          # the closed forms


def salted_uniform(shape, seed):
    """inputs of the GPU cases: uniform in [-0.5, 1.5] with the 256 x 3 boundary values and the special values scattered in (each at least once when
    the array has room; a small array takes as many as fit)"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.5, 1.5, size=shape).astype(F)
    salt = np.concatenate([boundary_values().reshape(-1), SPECIALS])
    flat = x.reshape(-1)
    k = min(flat.size, salt.size)
    where = rng.permutation(flat.size)[:k]
    flat[where] = salt[rng.permutation(salt.size)[:k]]
    return flat.reshape(shape)
