"""fp64 restatement of the stickman (the yardstick of tests/test_stickman_gpu.py), written from the definition and taking the same polyline table as
lp_stickman_render (hipops.stickman_table): with p = points * (S - 1), pixel (x, y) = (column, row), for every segment (a, b) of a part
    t = clamp(<pix - a, b - a> / max(|b - a|^2, 1e-12), 0, 1),  d = |pix - (a + t (b - a))|,  line = clamp(1 - min_d_of_the_part / width, 0, 1)
    img[c] = max(0, max over parts of line * colour[part][c])
Test infrastructure only: plain torch on the host, never on the product path."""
import torch


def render(points, size, seg, part_end, colour, width=None):
    """points [..., P, 2] (any float dtype; taken to fp64 as they are) -> fp64 [..., 3, S, S]"""
    width = max(1.0, size / 64.0) if width is None else float(width)
    pts = points.detach().double().cpu()
    lead = tuple(pts.shape[:-2])
    pts = pts.reshape(-1, pts.shape[-2], 2)
    ys, xs = torch.meshgrid(torch.arange(size, dtype=torch.float64), torch.arange(size, dtype=torch.float64), indexing='ij')
    pix = torch.stack([xs, ys], -1)                                     # [S, S, 2]
    out = torch.zeros(pts.shape[0], 3, size, size, dtype=torch.float64)
    for n in range(pts.shape[0]):
        p = pts[n] * (size - 1)
        start = 0
        for part, end in enumerate(part_end):
            a = torch.stack([p[i] for i, _ in seg[start:end]])          # [L, 2]
            b = torch.stack([p[j] for _, j in seg[start:end]])
            start = end
            ab = b - a
            e = pix[None] - a[:, None, None]                            # [L, S, S, 2]
            t = ((e * ab[:, None, None]).sum(-1) / ab.pow(2).sum(-1).clamp_min(1e-12)[:, None, None]).clamp(0.0, 1.0)
            d = (e - t[..., None] * ab[:, None, None]).pow(2).sum(-1).sqrt().min(0)[0]
            line = (1.0 - d / width).clamp(0.0, 1.0)
            for c in range(3):
                out[n, c] = torch.maximum(out[n, c], line * colour[part][c])
    return out.reshape(lead + (3, size, size))
