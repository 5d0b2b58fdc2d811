"""lp_visual_sheet on the MI355X (``hipops.visual_sheet``: one launch for the whole sheet).  Every comparison is exact equality of uint8:
  (a) against the numpy restatement (tests/visual_sheet_restatement.py) on the smallest shapes where the kernel's paths differ: H in {1, 3, 8},
      W in {1, 4, 6, 7, 16, 33} (whole quads, tails, W < 4), N in {1, 3}, P in {1, 2, 5, 12} with one- and three-channel panels mixed, with and
      without a caption strip (Hc in {0, 5}); inputs uniform in [-0.5, 1.5] with the 256 x 3 boundary values and the special values scattered in;
  (b) layouts in one call -- contiguous, ``[:, 0]`` of a 5-D tensor, a stride-0 expanded mask, channels-last, column stride 2, a view 4 bytes off
      16-byte alignment, a row stride that is no multiple of 4 -- against the same call on ``.contiguous()`` copies and against the restatement;
  (c) against the stock torch device chain on NaN-free input;
  (d) the bytes around an output that is a slice of a larger buffer stay what they were (word and byte stores), and the call captured in a
      single-stream graph and replayed after the inputs were overwritten in place gives the new inputs' sheet."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import visual_sheet_restatement as VR          # noqa: E402


def channels(p, n):
    return 1 if (p + n) % 2 == 1 else 3


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h', [1, 3, 8])
@pytest.mark.parametrize('w', [1, 4, 6, 7, 16, 33])
def test_against_the_restatement(h, w):
    from latent_pose_reenactment_amd import hipops as ops
    rng = np.random.RandomState(1000 * h + w)
    for n in (1, 3):
        for count in (1, 2, 5, 12):
            panels = [VR.salted_uniform((n, channels(p, n), h, w), 7 * p + n + 100 * count + 1000 * h + w) for p in range(count)]
            dev = [torch.from_numpy(p).cuda() for p in panels]
            for hc in (0, 5):
                strip = rng.randint(0, 256, size=(hc, count * w)).astype(np.uint8) if hc else None
                got = ops.visual_sheet(dev, caption=None if strip is None else torch.from_numpy(strip).cuda())
                assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (hc + n * h, count * w, 3)
                want = VR.sheet(panels, strip)
                assert np.array_equal(got.cpu().numpy(), want), (h, w, n, count, hc)
                assert torch.equal(got, ops.visual_sheet(dev, caption=None if strip is None else torch.from_numpy(strip).cuda()))


def test_special_values_and_every_boundary_value():
    from latent_pose_reenactment_amd import hipops as ops
    x = torch.from_numpy(VR.SPECIALS.copy()).reshape(1, 1, 1, -1).cuda()
    assert np.array_equal(ops.visual_sheet([x])[0, :, 0].cpu().numpy(), VR.SPECIALS_Q)
    b = VR.boundary_values()
    got = ops.visual_sheet([torch.from_numpy(b.copy()).reshape(1, 1, 256, 3).cuda()])
    assert np.array_equal(got[..., 2].cpu().numpy(), VR.quantise(b))
    got = ops.visual_sheet([torch.from_numpy(np.ascontiguousarray(b.T)).reshape(1, 3, 1, 256).cuda()])          # (whole quads, 16-byte loads)
    assert np.array_equal(got[0].cpu().numpy(), VR.quantise(b))


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w', [8, 6])
def test_layouts_in_one_call(w):
    from latent_pose_reenactment_amd import hipops as ops
    n, h = 2, 5

    def dev(shape, seed):
        return torch.from_numpy(VR.salted_uniform(shape, seed)).cuda()
    five = dev((n + 1, 2, 3, h, w), 1)
    mask = dev((n, 1, 1, h, w), 2).expand(n, 1, 3, h, w)
    views = [dev((n, 3, h, w), 3),                                   # contiguous
             five[:n, 0],                                            # [:, 0] of a 5-D tensor
             mask[:, 0],                                             # stride-0 expanded mask
             dev((n, h, w, 3), 4).permute(0, 3, 1, 2),               # channels-last
             dev((n, 3, h, 2 * w), 5)[..., ::2],                     # column stride 2
             dev((n, 3, h, w + 1), 6)[..., 1:],                      # first element 4 bytes off 16-byte alignment
             dev((n, 3, h, w + 1), 7)[..., :w],                      # aligned base, row stride no multiple of 4
             dev((n, 1, h, w), 8),                                   # one channel
             five[1:, 1, :1]]                                        # one channel of a 5-D tensor, offset base
    assert views[2].stride(1) == 0 and views[3].stride(3) == 3 and views[4].stride(3) == 2 and views[5].data_ptr() % 16 == 4
    assert views[6].data_ptr() % 16 == 0 and views[6].stride(2) % 4 != 0
    strip = torch.from_numpy(np.random.RandomState(9).randint(0, 256, size=(3, len(views) * w)).astype(np.uint8)).cuda()
    got = ops.visual_sheet(views, caption=strip)
    assert torch.equal(got, ops.visual_sheet([v.contiguous() for v in views], caption=strip))
    assert np.array_equal(got.cpu().numpy(), VR.sheet([v.contiguous().cpu().numpy() for v in views], strip.cpu().numpy()))


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------------------------
def torch_chain(panels, strip=None):
    """the same sheet composed from stock torch device ops: per panel clamp, mul, byte, permute, expand, then cat"""
    cols = []
    for t in panels:
        n, c, h, w = t.shape
        cols.append(t.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).expand(n, h, w, 3).reshape(n * h, w, 3))
    sheet = torch.cat(cols, dim=1)
    return sheet if strip is None else torch.cat((strip[:, :, None].expand(-1, -1, 3), sheet), dim=0)


@pytest.mark.parametrize('n, h, w', [(2, 16, 16), (3, 7, 33)])
def test_against_the_torch_device_chain(n, h, w):
    from latent_pose_reenactment_amd import hipops as ops
    panels = [torch.from_numpy(np.nan_to_num(VR.salted_uniform((n, 1 if p == 2 else 3, h, w), 20 + p), nan=0.25, posinf=np.inf, neginf=-np.inf)).cuda()
              for p in range(4)]
    strip = torch.from_numpy(np.random.RandomState(5).randint(0, 256, size=(4, 4 * w)).astype(np.uint8)).cuda()
    assert torch.equal(ops.visual_sheet(panels, caption=strip), torch_chain(panels, strip))
    assert torch.equal(ops.visual_sheet(panels), torch_chain(panels))
    assert torch.equal(ops.visual_sheet(panels, caption=strip).cpu(), ops.visual_sheet_host([p.cpu() for p in panels], strip.cpu()))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w, offset', [(8, 32), (8, 17), (7, 32), (33, 3)])
def test_nothing_outside_the_output_is_written(w, offset):
    from latent_pose_reenactment_amd import hipops as ops
    n, h, count, hc = 3, 3, 5, 5
    panels = [torch.from_numpy(VR.salted_uniform((n, channels(p, 0), h, w), 30 + p)).cuda() for p in range(count)]
    strip = torch.from_numpy(np.random.RandomState(6).randint(0, 256, size=(hc, count * w)).astype(np.uint8)).cuda()
    shape = (hc + n * h, count * w, 3)
    size = shape[0] * shape[1] * shape[2]
    big = torch.full((offset + size + 64,), 0xA5, dtype=torch.uint8, device='cuda')
    out = big[offset:offset + size].view(shape)
    assert ops.visual_sheet(panels, caption=strip, out=out) is out
    torch.cuda.synchronize()
    assert bool((big[:offset] == 0xA5).all()) and bool((big[offset + size:] == 0xA5).all())
    assert np.array_equal(out.cpu().numpy(), VR.sheet([p.cpu().numpy() for p in panels], strip.cpu().numpy()))


def test_captured_in_a_graph_and_replayed_on_new_inputs():
    from latent_pose_reenactment_amd import hipops as ops
    n, h, w = 2, 6, 12
    base = torch.from_numpy(VR.salted_uniform((n, 2, 3, h, w), 40)).cuda()
    mask = torch.from_numpy(VR.salted_uniform((n, 1, 1, h, w), 41)).cuda()
    views = [base[:, 0], mask.expand(n, 1, 3, h, w)[:, 0], base[:, 1, 1:2]]
    strip = torch.from_numpy(np.random.RandomState(42).randint(0, 256, size=(5, 3 * w)).astype(np.uint8)).cuda()
    out = torch.zeros((5 + n * h, 3 * w, 3), dtype=torch.uint8, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.visual_sheet(views, caption=strip, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    first = out.clone()
    assert np.array_equal(first.cpu().numpy(), VR.sheet([v.contiguous().cpu().numpy() for v in views], strip.cpu().numpy()))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream: the launch is the graph's only node
        ops.visual_sheet(views, caption=strip, out=out)
    base.copy_(torch.from_numpy(VR.salted_uniform((n, 2, 3, h, w), 43)).cuda())
    mask.copy_(torch.from_numpy(VR.salted_uniform((n, 1, 1, h, w), 44)).cuda())
    strip.copy_(255 - strip)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = VR.sheet([v.contiguous().cpu().numpy() for v in views], strip.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), want) and not torch.equal(out, first)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
