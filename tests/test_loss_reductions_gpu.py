"""GPU parity tests of the loss reductions of csrc/elementwise.hip against fp64 torch-CPU autograd of the reference expressions:
  * dice (criterions/dice.py DiceFn: lp_reduce_dice / _bwd) -- 256 block partials and a double-precision finalize, the 1-vs-C channel
    broadcast, sizes with a tail and below one block, weight and upstream gradient != 1;
  * hinge (criterions/adversarial.py HingeGFn / HingeDFn: lp_reduce_hinge / _bwd) -- the 64-lane loop over B scores, scores exactly at
    the hinge (+-1, where relu's subgradient is 0) and on both sides, and the calls that ask for only some of the gradients."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def report(name, err, tol):
    print(f'[parity] {name}: rel-L2 {err:.3e} (tol {tol:.0e})')
    assert err < tol, f'{name}: rel-L2 {err:.3e} >= {tol}'


def _dice_ref(fake, real, weight):
    """criterions/dice.py of the reference: numerator and sum(real^2) over the broadcast shape, sum(fake^2) over fake's own elements"""
    return -torch.log((2 * fake * real).sum() / ((fake ** 2).sum() + (real ** 2).sum())) * weight


DICE_CASES = [
    # B, Cf, Cr, H, W
    (8, 1, 3, 256, 256),          # full step size, the reference's 1-vs-3 broadcast
    (8, 3, 3, 256, 256),
    (3, 1, 3, 37, 41),            # B * HW = 4551: not a multiple of 256
    (3, 2, 2, 37, 41),
    (2, 1, 3, 5, 7),              # 70 elements: most of the 256 partial blocks are empty
    (1, 1, 1, 1, 3),
]


@pytest.mark.parametrize('weight,gout', [(1.0, 1.0), (0.37, 2.5)])
@pytest.mark.parametrize('case', DICE_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_dice_loss_and_gradient(case, weight, gout):
    from latent_pose_reenactment_amd.criterions.dice import DiceFn
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    b, cf, cr, h, w = case
    g = torch.Generator().manual_seed(b * 1000 + cf * 100 + cr * 10 + h)
    fake = torch.sigmoid(torch.randn(b, cf, h, w, generator=g, dtype=torch.float64) * 2).float()
    real = torch.rand(b, cr, h, w, generator=g, dtype=torch.float64).float()
    f = fake.cuda().requires_grad_(True)
    loss = DiceFn.apply(f, real.cuda(), weight)
    loss.backward(torch.tensor(gout, device='cuda'))
    torch.cuda.synchronize()
    f64 = fake.double().requires_grad_(True)
    ref = _dice_ref(f64, real.double(), weight)
    ref.backward(torch.tensor(gout, dtype=torch.float64))
    report(f'dice loss {case} w={weight}', rel(loss, ref), 1e-5)
    report(f'dice dfake {case} w={weight} g={gout}', rel(f.grad, f64.grad), 1e-5)


def _scores(b, g):
    """B critic scores: exactly +-1 (the hinge points) in a third of them, the rest on both sides of the hinges"""
    s = torch.randn(b, generator=g, dtype=torch.float64) * 2
    k = torch.arange(b)
    s[k % 6 == 1] = 1.0
    s[k % 6 == 4] = -1.0
    return s.float()


@pytest.mark.parametrize('b', [1, 8, 63, 64, 65, 200])
def test_hinge_losses_and_gradients(b):
    from latent_pose_reenactment_amd import _lib
    from latent_pose_reenactment_amd.criterions.adversarial import HingeDFn, HingeGFn
    g = torch.Generator().manual_seed(b)
    real, fd, fg = _scores(b, g).view(b, 1), _scores(b, g).view(b, 1), _scores(b, g).view(b, 1)
    if b == 1:
        real[0], fd[0] = 1.0, -1.0                         # both hinge points even with one score
    gG, gD = 0.7, 1.3
    # fp64 reference: torch's relu backward gives 0 exactly at the hinge
    r64, d64, g64 = (t.double().requires_grad_(True) for t in (real, fd, fg))
    lG64 = -g64.mean()
    lD64 = torch.relu(1 - r64).mean() + torch.relu(1 + d64).mean()
    (lG64 * gG + lD64 * gD).backward()
    # all three gradients
    r, d, f = (t.cuda().requires_grad_(True) for t in (real, fd, fg))
    lG, lD = HingeGFn.apply(f), HingeDFn.apply(r, d)
    (lG * gG + lD * gD).backward()
    torch.cuda.synchronize()
    report(f'hinge loss_G B={b}', rel(lG, lG64), 1e-6)
    report(f'hinge loss_D B={b}', rel(lD, lD64), 1e-6)
    for name, got, want in (('d_fake_G', f.grad, g64.grad), ('d_real', r.grad, r64.grad), ('d_fake_D', d.grad, d64.grad)):
        assert torch.equal(got.cpu() == 0, want == 0), (name, b, 'subgradient at the hinge / inactive side')
        report(f'hinge {name} B={b}', rel(got, want), 1e-6)
    # loss_D with only one of its inputs requiring a gradient
    for need_real in (True, False):
        r1 = real.cuda().requires_grad_(need_real)
        d1 = fd.cuda().requires_grad_(not need_real)
        HingeDFn.apply(r1, d1).backward(torch.tensor(gD, device='cuda'))
        torch.cuda.synchronize()
        got, want = (r1.grad, r64.grad) if need_real else (d1.grad, d64.grad)
        assert (d1.grad if need_real else r1.grad) is None
        assert torch.equal(got.cpu() == 0, want == 0) and rel(got, want) < 1e-6, ('partial', need_real, b)
    # one lp_reduce_hinge_bwd call that writes all three gradients
    rc, dc, fc = real.cuda().reshape(-1), fd.cuda().reshape(-1), fg.cuda().reshape(-1)
    ug, ud = torch.tensor([gG], device='cuda'), torch.tensor([gD], device='cuda')
    outs = [torch.full((b,), float('nan'), device='cuda') for _ in range(3)]
    _lib.check(_lib.lib().lp_reduce_hinge_bwd(rc.data_ptr(), dc.data_ptr(), ug.data_ptr(), ud.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                              outs[2].data_ptr(), b, torch.cuda.current_stream().cuda_stream), 'lp_reduce_hinge_bwd')
    torch.cuda.synchronize()
    for name, got, want in zip(('d_real', 'd_fake_D', 'd_fake_G'), outs, (r64.grad, d64.grad, g64.grad)):
        want = want.reshape(-1)
        assert torch.equal(got.cpu() == 0, want == 0) and rel(got, want) < 1e-6, ('one call', name, b)
