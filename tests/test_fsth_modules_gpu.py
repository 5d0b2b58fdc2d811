"""GPU parity of the FSTH plugin family against the fixtures the reference wrote (tests/golden/make_golden_fsth.py), toy geometry:
  * both conv embedders x {sum, max}, the stickman-conditioned critic (with the discarded loss_G gradients under ``keep_reference_waste``) and the
    l1_rgb criterion, LP_PREC=bf16x3, gates of tests/test_discriminator_criterions.py (forward 2e-4, gradients 5e-3, spectral-norm buffers 1e-5);
  * one ``runners.holycow.train_step`` of embedder FSTH + generator FSTH_plus + discriminator FSTH (adversarial, featmat, l1_rgb, dice; Adam) against
    the recorded reference iteration, gates of tests/test_train_step.py; eager launches, which is what train.py selects by default (--hip_graph off);
  * one ``drive_frames`` call with the FSTH embedder + FSTH_plus on a batch carrying ``dec_keypoints``."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

from test_fsth_cpu import fixture, plugin, reference_states, sd_of, toy_args          # noqa: E402


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def gate(errs, what):
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:8]
    print(f'[parity] {what}: worst', [(k, f'{v:.2e}') for k, v in worst])
    bad = {k: v for k, v in errs.items() if v >= (1e-5 if k.startswith('buf.') else 5e-3 if 'grad' in k or k.startswith('gG') else 2e-4)}
    assert not bad, bad


@pytest.mark.parametrize('avg', ['sum', 'max'])
@pytest.mark.parametrize('name', ['FSTH', 'no_pose_encoder'])
def test_embedder_vs_reference_golden(name, avg, monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    z = fixture(f'fsth_embedder_{name}_small.npz')
    E = plugin('embedders', name).Wrapper.get_net(toy_args(avg))
    E.load_state_dict(sd_of(z, f'{avg}.sd.'), strict=True)
    E = E.cuda().train()
    rgbs = torch.from_numpy(z[f'{avg}.enc_rgbs']).cuda().requires_grad_(True)
    dd = dict(enc_rgbs=rgbs)
    if name == 'FSTH':
        dd['enc_stickmen'] = torch.from_numpy(z[f'{avg}.enc_stickmen']).cuda()
    E(dd)
    assert tuple(dd['embeds'].shape) == (2, 8) and tuple(dd['embeds_elemwise'].shape) == (2, 3, 8)
    ((dd['embeds'] * torch.from_numpy(z[f'{avg}.r1']).cuda()).sum() + (dd['embeds_elemwise'] * torch.from_numpy(z[f'{avg}.r2']).cuda()).sum()).backward()
    errs = {'embeds': rel(dd['embeds'], z[f'{avg}.embeds']), 'embeds_elemwise': rel(dd['embeds_elemwise'], z[f'{avg}.embeds_elemwise']),
            'grad_enc_rgbs': rel(rgbs.grad, z[f'{avg}.grad_enc_rgbs'])}
    for k, p in E.named_parameters():
        errs['grad.' + k] = rel(p.grad, z[f'{avg}.grad.{k}'])
    for k, v in E.state_dict().items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['buf.' + k] = rel(v, z[f'{avg}.sd_after.{k}'])
    gate(errs, f'embedder {name} {avg} (bf16x3)')


def test_critic_three_passes_and_losses_vs_reference_golden(monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    from criterions import adversarial, featmat, dice, dis_embed
    z = fixture('fsth_discriminator_small.npz')
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(toy_args())
    D.load_state_dict(sd_of(z, 'sd.'), strict=True)
    D = D.cuda().train()
    D.keep_reference_waste = True      # this test also compares the (discarded) D-parameter gradients of loss_G
    fake = torch.from_numpy(z['fake']).cuda().requires_grad_(True)
    dd = dict(fake_rgbs=fake, target_rgbs=torch.from_numpy(z['real']).cuda(), dec_stickmen=torch.from_numpy(z['dec_stickmen']).cuda(),
              label=torch.from_numpy(z['label']).cuda())
    D(dd)
    errs = {k: rel(dd[k], z[k]) for k in ('fake_score_G', 'fake_score_D', 'real_score', 'real_embedding')}
    for i, (f, r) in enumerate(zip(dd['fake_features'], dd['real_features'])):
        assert tuple(f.shape) == z[f'fake_feat{i}'].shape
        errs[f'fake_feat{i}'] = rel(f, z[f'fake_feat{i}']); errs[f'real_feat{i}'] = rel(r, z[f'real_feat{i}'])
    dd['fake_segm'] = torch.from_numpy(z['fake_segm']).cuda().requires_grad_(True)
    dd['real_segm'] = torch.from_numpy(z['real_segm']).cuda()
    dd['embeds_elemwise'] = torch.from_numpy(z['embeds_elemwise']).cuda().requires_grad_(True)
    lg, ld = adversarial.Criterion('gan')(dd)
    fm = featmat.Criterion(10.0)(dd)['feature_matching']
    dc = dice.Criterion(1.0)(dd)['segmentation_dice']
    de = dis_embed.Criterion(1e-2)(dd)['embedding_matching']
    for v, k in ((lg['adversarial_G'], 'loss_adv_G'), (ld['adversarial_D'], 'loss_adv_D'), (fm, 'loss_fm'), (dc, 'loss_dice'), (de, 'loss_dis_embed')):
        errs[k] = rel(v, z[k])
    (lg['adversarial_G'] + fm + dc + de).backward(retain_graph=True)
    errs['gG_fake'] = rel(fake.grad, z['gG_fake']); errs['gG_fake_segm'] = rel(dd['fake_segm'].grad, z['gG_fake_segm'])
    errs['gG_elemwise'] = rel(dd['embeds_elemwise'].grad, z['gG_elemwise'])
    for k, p in D.named_parameters():
        errs['gradG.' + k] = rel(p.grad, z['gradG.' + k])
    D.zero_grad()
    ld['adversarial_D'].backward()
    for k, p in D.named_parameters():
        errs['gradD.' + k] = rel(p.grad, z['gradD.' + k])
    for k, v in D.state_dict().items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['buf.' + k] = rel(v, z['sd_after.' + k])
    gate(errs, 'FSTH discriminator + cheap criterions (bf16x3)')
    # fine-tuning variant, from the buffers the train forward left
    Df = plugin('discriminators', 'FSTH').Wrapper.get_net(toy_args())
    Df.enable_finetuning({'embeds': torch.zeros(1, 8)})
    Df.load_state_dict(sd_of(z, 'ft_sd.'), strict=True)
    Df = Df.cuda().train()
    d2 = dict(fake_rgbs=fake.detach(), target_rgbs=dd['target_rgbs'], dec_stickmen=dd['dec_stickmen'], label=torch.zeros(2, dtype=torch.long).cuda())
    with torch.no_grad():
        Df(d2)
    for k in ('fake_score_G', 'real_score', 'real_embedding'):
        assert rel(d2[k], z['ft_' + k]) < 2e-4, k


def test_l1_rgb_vs_reference_golden():
    z = fixture('fsth_discriminator_small.npz')
    crit = plugin('criterions', 'l1_rgb').Wrapper.get_net(argparse.Namespace(l1_weight=30.0, device='cuda'))
    fake = torch.from_numpy(z['l1_fake']).cuda().requires_grad_(True)
    out = crit({'fake_rgbs': fake, 'target_rgbs': torch.from_numpy(z['l1_target']).cuda()})
    assert set(out) == {'l1_rgb'}
    out['l1_rgb'].backward()
    e_loss, e_grad = rel(out['l1_rgb'], z['l1_loss']), rel(fake.grad, z['l1_grad'])
    print(f'[parity] l1_rgb: loss {e_loss:.2e} grad {e_grad:.2e}')
    assert e_loss < 1e-5 and e_grad < 1e-5


# ---- one training iteration ------------------------------------------------------------------------------------------------------------------------
def summary(v):
    r = torch.randn(v.shape, generator=torch.Generator().manual_seed(77))
    return np.array([float(v.double().norm()), float((v.double() * r.double()).sum())])


def build_step(z, monkeypatch, prec):
    monkeypatch.setenv('LP_PREC', prec)
    from criterions import adversarial, featmat, dice
    from runners import holycow
    a = toy_args(device='cuda', optimizer='Adam', lr_gen=5e-4, lr_dis=8e-4, beta1=0.0, finetune=False, num_gpus=1)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a)
    G = plugin('generators', 'FSTH_plus').Wrapper.get_net(a)
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(a)
    st = reference_states(z)
    E.load_state_dict(st['E']); G.load_state_dict(st['G']); D.load_state_dict(st['D'])
    crits = [adversarial.Criterion('gan'), featmat.Criterion(10.0), plugin('criterions', 'l1_rgb').Criterion(30.0), dice.Criterion(1.0)]
    tm = holycow.TrainingModule(E, G, D, crits, [], {})          # deep-copies E and G as EMA models
    opt_G = holycow.get_optimizer(E, G, a)
    opt_D = plugin('discriminators', 'FSTH').Wrapper.get_optimizer(D, a)
    tm.train()
    data = {k[len('init.in.'):]: torch.from_numpy(z[k]).cuda() for k in z.files if k.startswith('init.in.') and 'segm' not in k and 'label' not in k}
    target = {'real_segm': torch.from_numpy(z['init.in.real_segm']).cuda(), 'label': torch.from_numpy(z['init.in.label']).cuda()}
    return tm, opt_G, opt_D, a, data, target, holycow, st


# (tests/test_train_step.py: losses, state tensors rel-L2 with Adam, Adam sign-flip fraction among the elements that moved by > lr/2 in the reference)
GATES = {'bf16x3': (5e-5, 5e-5, 2e-2), 'f16': (2e-3, 4e-2, 0.2)}


@pytest.mark.parametrize('prec', ['bf16x3', 'f16'])
def test_one_iteration_matches_reference_run_epoch(prec, monkeypatch):
    """Adam with beta1 = 0 moves every element by at most lr whatever the gradient's magnitude: two correct implementations can differ by 2 lr on an
    element whose gradient is ~0 and never by more (the absolute bound below), plus the fraction of elements whose update direction differs"""
    z = fixture('fsth_train_step_small.npz')
    tm, opt_G, opt_D, a, data, target, holycow, st = build_step(z, monkeypatch, prec)
    _, lG, lD = holycow.train_step(tm, data, target, opt_G, opt_D, a)
    torch.cuda.synchronize()
    g_loss, g_state, g_flip = GATES[prec]
    errs, flips = {}, {}
    assert set(lG) == {'adversarial_G', 'feature_matching', 'l1_rgb', 'segmentation_dice'} and set(lD) == {'adversarial_D'}
    for name, v in {**lG, **lD}.items():
        errs['loss.' + name] = rel(v, z[f'loss.{name}'])
    mods = (('E', tm.embedder, a.lr_gen), ('G', tm.generator, a.lr_gen), ('D', tm.discriminator, a.lr_dis),
            ('E_ema', tm.running_averages['embedder'], a.lr_gen), ('G_ema', tm.running_averages['generator'], a.lr_gen))
    for nm, mod, lr in mods:
        init = st[nm[0]]
        for k, v in mod.state_dict().items():
            want = z[f'after.{nm}.{k}']
            v = v.detach().cpu()
            if want.shape != tuple(v.shape):          # (stored as norm + seeded projection: too large for the fixture)
                errs[f'{nm}.{k}'] = rel(summary(v), want)
                continue
            errs[f'{nm}.{k}'] = rel(v, want)
            if v.dtype == torch.float32 and (k.endswith('weight_orig') or k.endswith('constant') or k.endswith('weight')) and not nm.endswith('_ema'):
                ref_delta = want - init[k].numpy()
                got_delta = v.numpy() - init[k].numpy()
                if np.linalg.norm(ref_delta) > 1e-7 * max(1.0, np.linalg.norm(want)):
                    assert np.abs(got_delta - ref_delta).max() <= 2.02 * lr, (nm, k, np.abs(got_delta - ref_delta).max(), lr)
                    moved = np.abs(ref_delta) > 0.5 * lr
                    if moved.any():
                        flips[f'{nm}.{k}'] = float((np.sign(got_delta[moved]) != np.sign(ref_delta[moved])).mean())
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print(f'[parity] FSTH train step (Adam, {prec}): worst', [(k, f'{v:.2e}') for k, v in worst],
          'Adam direction flips (worst tensors):', sorted(((round(v, 4), k) for k, v in flips.items()), reverse=True)[:3])
    bad = {k: v for k, v in errs.items() if v >= (g_loss if k.startswith('loss.') else g_state)}
    assert not bad, bad
    assert flips and float(np.mean(list(flips.values()))) <= g_flip, flips


def test_drive_frames_with_the_fsth_embedder_and_keypoints(monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    import drive                      # (the entry script disables autograd globally at import, like the reference's drive.py)
    torch.set_grad_enabled(True)
    z = fixture('fsth_train_step_small.npz')
    a = toy_args(device='cuda')
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a)
    G = plugin('generators', 'FSTH_plus').Wrapper.get_net(a)
    st = reference_states(z)
    E.load_state_dict(st['E']); G.load_state_dict(st['G'])
    E.eval(); G.eval()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ident = {'enc_rgbs': torch.from_numpy(z['init.in.enc_rgbs'])[:1].cuda(), 'enc_stickmen': torch.from_numpy(z['init.in.enc_stickmen'])[:1].cuda()}
        E(ident)          # the identity to drive: its embedding moves into the generator (train.py's fine-tuning bootstrap)
        boot = {'embeds': ident['embeds']}
        G.enable_finetuning(boot); E.enable_finetuning()
        batch = {'pose_input_rgbs': torch.rand(3, 1, 3, 32, 32, generator=g).cuda(), 'dec_keypoints': torch.rand(3, 1, 6, generator=g).cuda()}
        grid = drive.drive_frames(E, G, batch)
        assert grid.shape == (3, 32, 64, 3) and grid.dtype == torch.uint8 and grid.is_cuda
        direct = {'dec_keypoints': batch['dec_keypoints']}
        G(direct)
        assert torch.equal(batch['fake_rgbs'], direct['fake_rgbs'])
        want = direct['fake_rgbs'].permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()
        assert torch.equal(grid[:, :, 32:], want)
