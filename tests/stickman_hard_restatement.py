"""The hard-edged stickman (header comment of csrc/stickman_hard.hip) restated with Python integers: no numpy, no torch arithmetic, unbounded ints, one
pixel and one segment at a time.  The yardstick of tests/test_stickman_hard_cpu.py (the host twin), tests/test_stickman_hard_gpu.py (the kernel)
and the keypoint loaders' tests; compared with exact equality.

  point:     X = clamp(rint(fp32(x * S)), -4096, 8191): the product rounded to fp32 (it is exact in a double: 24 + 13 bits), then to the nearest
             integer, ties to even (Python's round); NaN -> -4096, +inf -> 8191, -inf -> -4096
  coverage:  P = (u, v), segment A -> B, d = B - A, e = P - A, L2 = d.d, s = e.d:
                 4 |e|^2 <= T^2                   if L2 == 0 or s <= 0
                 4 |P - B|^2 <= T^2               if s >= L2
                 4 (dx ey - dy ex)^2 <= T^2 L2    otherwise
  colour:    the colour of the last part in table order with a covering segment; 0 where there is none"""
import math
import struct

import torch

LO, HI = -4096, 8191


def fp32(v):
    """a double rounded to the nearest fp32 (ties to even), as a double; beyond the fp32 range: +-inf"""
    try:
        return struct.unpack('f', struct.pack('f', v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


def integer_point(x, size):
    """x: an fp32 value held in a Python float"""
    if math.isnan(x):
        return LO
    r = fp32(x * float(size))
    if math.isinf(r):
        return HI if r > 0 else LO
    return min(max(round(r), LO), HI)


def covers(u, v, ax, ay, bx, by, t):
    dx, dy, ex, ey = bx - ax, by - ay, u - ax, v - ay
    l2, s = dx * dx + dy * dy, ex * dx + ey * dy
    if l2 == 0 or s <= 0:
        return 4 * (ex * ex + ey * ey) <= t * t
    if s >= l2:
        return 4 * ((u - bx) ** 2 + (v - by) ** 2) <= t * t
    return 4 * (dx * ey - dy * ex) ** 2 <= t * t * l2


def render_one(points, size, parts, thickness):
    """points: [[x, y], ...] Python floats (fp32 values) -> nested lists [3][S][S] of Python floats"""
    pts = [(integer_point(x, size), integer_point(y, size)) for x, y in points]
    img = [[[0.0] * size for _ in range(size)] for _ in range(3)]
    half = (thickness + 1) // 2
    for first, last, closed, colour in parts:          # painter's order: a later part (and a later segment) overwrites
        idx = list(range(first, last + 1))
        for i, j in list(zip(idx[:-1], idx[1:])) + ([(idx[-1], idx[0])] if closed else []):
            (ax, ay), (bx, by) = pts[i], pts[j]
            # (only the pixels of the segment's box grown by ceil(T / 2) can be covered: a pixel within T / 2 of the segment lies in it)
            for v in range(max(0, min(ay, by) - half), min(size - 1, max(ay, by) + half) + 1):
                for u in range(max(0, min(ax, bx) - half), min(size - 1, max(ax, bx) + half) + 1):
                    if covers(u, v, ax, ay, bx, by, thickness):
                        for c in range(3):
                            img[c][v][u] = float(colour[c])
    return img


def render(points, size, parts, thickness=2):
    """points: fp32 tensor [..., P, 2] or [..., 2P] -> fp32 tensor [..., 3, S, S]"""
    points = points.detach().cpu()
    assert points.dtype == torch.float32
    if points.shape[-1] != 2 or points.dim() < 2 or points.shape[-2] < 1 + max(p[1] for p in parts):
        points = points.reshape(*points.shape[:-1], points.shape[-1] // 2, 2)
    lead = tuple(points.shape[:-2])
    flat = points.reshape(-1, points.shape[-2], 2).tolist()          # (fp32 -> Python floats: exact)
    imgs = [render_one(p, size, parts, thickness) for p in flat]
    return torch.tensor(imgs, dtype=torch.float32).reshape(*lead, 3, size, size)
