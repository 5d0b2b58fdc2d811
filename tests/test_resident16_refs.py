"""CPU proof of the fp64 restatements that tests/test_resident16_gpu.py holds the 16-bit-resident and planes-only kernels to.
Pins emu_ops.adain_relu_bwd, plane_positive, l1_planes, avgpool2 and avgpool2_bwd_mask against torch autograd in fp64 (no GPU needed)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_ops  # noqa: E402


def rel(a, b):
    a = a.detach().double(); b = b.detach().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize('with_add', [False, True])
@pytest.mark.parametrize('ups', [0, 1])
@pytest.mark.parametrize('shape', [(3, 5, 7, 8), (2, 4, 4, 72)])          # an odd map; two channel blocks
def test_adain_relu_bwd_equals_autograd(shape, ups, with_add):
    """relu(instance_norm(x) * gamma + beta) [+ x2 nearest upsample] differentiated by autograd: both sides fp64, gate 1e-12"""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(4)
    x = (torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    gamma = torch.randn(n, c, generator=g, dtype=torch.float64).requires_grad_(True)
    beta = torch.randn(n, c, generator=g, dtype=torch.float64).requires_grad_(True)
    mean = x.mean((2, 3), keepdim=True); var = x.var((2, 3), unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-4)
    a = torch.relu((x - mean) * rstd * gamma[:, :, None, None] + beta[:, :, None, None])
    if ups:
        a = a.repeat_interleave(2, 2).repeat_interleave(2, 3)
    dA = torch.randn(a.shape, generator=g, dtype=torch.float64)
    add = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) if with_add else None
    a.backward(dA)
    m, r = mean.detach().reshape(n, c), rstd.detach().reshape(n, c)
    scale = gamma.detach() * r
    shift = beta.detach() - m * scale
    dx, dg, db = emu_ops.adain_relu_bwd(nhwc(dA), nhwc(x.detach()), None if add is None else nhwc(add), gamma.detach(), m, r, scale, shift,
                                        bool(ups))
    want_dx = x.grad if add is None else x.grad + add
    assert dx.shape == (n, h, w, c) and dg.shape == (n, c) and db.shape == (n, c)
    assert rel(dx, nhwc(want_dx)) < 1e-12
    assert rel(dg, gamma.grad) < 1e-12
    assert rel(db, beta.grad) < 1e-12


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_plane_positive_equals_decoded_positive_on_every_pattern(dtype):
    """all 65536 bit patterns: the undecoded predicate is [decoded > 0] everywhere except on the NaNs with a clear sign bit (a NaN is not > 0;
    the planes the kernels read hold none: lp_act_pack writes NaN only for a NaN input)"""
    bits = torch.arange(65536, dtype=torch.int32)
    stored = bits.to(torch.int16)                                   # the planes are int16 tensors: patterns >= 0x8000 are negative there
    assert torch.equal(stored.to(torch.int32) & 0xffff, bits)
    dec = stored.view(dtype).double()
    got = emu_ops.plane_positive(stored)
    assert torch.equal(got, emu_ops.plane_positive(bits))           # the same from the sign-extended and the zero-extended integer
    nan = torch.isnan(dec)
    assert int(nan.sum()) == (2 * 1023 if dtype == torch.float16 else 2 * 127)
    assert torch.equal(got[~nan], (dec > 0)[~nan])
    diff = got != (dec > 0)
    assert torch.equal(diff, nan & (bits < 0x8000))
    for pattern, want in ((0x0000, False), (0x8000, False), (0x0001, True), (0x8001, False), (0x7bff, True), (0xffff, False)):
        assert bool(got[pattern]) == want, hex(pattern)


def _taps(shape, seed):
    """pre-activations of two taps with exact ties, exact zeros and a <= 0 against b > 0"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(shape, generator=g, dtype=torch.float64)
    b = torch.randn(shape, generator=g, dtype=torch.float64)
    fa, fb = a.view(-1), b.view(-1)
    fa[0:8] = fb[0:8].abs() + 0.5; fb[0:8] = fa[0:8]               # ties at positive values
    fa[8:12] = 0.0; fb[8:12] = 0.0                                  # ties at zero
    fa[12:16] = 0.0; fb[12:16] = 0.7                                # a == 0 below b
    fa[16:20] = -0.3; fb[16:20] = 0.7                               # a < 0 below b
    fa[20:24] = 0.7; fb[20:24] = 0.0                                # a above b == 0
    return a, b


@pytest.mark.parametrize('shape', [(2, 6, 10, 8), (1, 4, 4, 72)])
def test_l1_planes_equals_autograd(shape):
    """F.l1_loss(relu(a), relu(b)) differentiated w.r.t. the pre-activation a: the int8 pattern / numel is exactly that gradient"""
    a, b = _taps(shape, 7)
    a.requires_grad_(True)
    loss = F.l1_loss(torch.relu(a), torch.relu(b))
    loss.backward()
    term, sgn = emu_ops.l1_planes(torch.relu(a.detach()), torch.relu(b))
    assert sgn.dtype == torch.int8 and sgn.shape == (a.numel(),)
    assert abs(term.item() - loss.item()) <= 1e-12 * abs(loss.item())
    assert torch.equal(sgn.double() / a.numel(), a.grad.flatten())
    s = sgn.view(-1)
    assert int(s[0:16].abs().sum()) == 0 and int(s[16:20].abs().sum()) == 0 and bool((s[20:24] == 1).all())
    assert set(s.tolist()) == {-1, 0, 1}


@pytest.mark.parametrize('relu_in,relu_out', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('shape', [(3, 6, 10, 8), (1, 4, 4, 72)])
def test_avgpool2_and_its_masked_backward_equal_autograd(shape, relu_in, relu_out):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64)
    x.view(-1)[0:64:3] = 0.0                                        # exact zeros: no gradient through the ReLU there
    x[0, 0, 0:2, 0:2] = torch.tensor([[1.0, -1.0], [0.5, -0.5]], dtype=torch.float64)      # a window whose mean is exactly 0
    x.requires_grad_(True)
    y = F.avg_pool2d(torch.relu(x) if relu_in else x, 2)
    if relu_out:
        y = torch.relu(y)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    got = emu_ops.avgpool2(nhwc(x.detach()), relu_in, relu_out)
    assert got.shape == (n, h // 2, w // 2, c)
    assert rel(got, nhwc(y)) < 1e-12
    if relu_in and not relu_out:
        dx = emu_ops.avgpool2_bwd_mask(nhwc(dy), nhwc(x.detach()))
        assert torch.equal(dx, nhwc(x.grad))                        # (x 0.25 and a 0/1 mask: exact on both sides)
        assert torch.equal(dx, emu_ops.avgpool2_bwd_mask(nhwc(dy), nhwc(x.detach()) > 0))
        assert int((dx[nhwc(x.detach()) == 0] != 0).sum()) == 0
