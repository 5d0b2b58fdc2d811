"""GPU checks of the stickman-to-image generator (generators/FSTH.py):
  * the new kernels through the C ABI against fp64 -- tanh head forward / backward (odd extents no block size divides, with and without the padding
    channel) and the batch-shared affine-gradient reduction -- at 1e-6 rel-L2, what tests/test_loss_reductions_gpu.py applies to fp32 kernels;
  * the module against the fixture the reference wrote (toy geometry, bf16x3): train forward, every parameter gradient, d embeds, the spectral-norm
    buffers, the eval forward and the fine-tuning leg;
  * a mid geometry -- the smallest at which the real routes engage (thin stem, 4x4 stride-2 conv + pool, epilogue statistics, phase-form up convs)
    -- against the fp64 restatement with the taped ReLU patterns replayed, as tests/test_fsth_full_gpu.py does;
  * one runner train step against the recorded reference iteration (scheme and bf16x3 GATES of tests/test_fsth_modules_gpu.py);
  * a 2-iteration train.py run.
Module outputs and gradients are gated at the project's contract, 1e-3 rel-L2; spectral-norm buffers (fp32 power iteration) at the 1e-5 of
tests/test_fsth_modules_gpu.py.  The worst figure of every test is printed.
Measured on an MI355X (bf16x3): kernels <= 6.5e-8; toy fake_rgbs 2.1e-5, worst gradient 4.4e-5 (fine-tuning leg 3.7e-5 / 5.7e-5); mid fake_rgbs 1.7e-5,
worst tie-masked gradient 7.1e-5 (untied 2.0e-2); train step: worst state tensor 3.7e-5, no Adam direction flips."""
import os
import subprocess
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

import fsth_restatement as R          # noqa: E402
import fsth_generator_restatement as GR          # noqa: E402
from test_fsth_cpu import fixture, plugin, sd_of          # noqa: E402
from test_fsth_generator_cpu import gen_args, grad_figure, null_gradient, step_states          # noqa: E402
from test_fsth_full_gpu import UNIT, check_tie_condition          # noqa: E402
from test_fsth_modules_gpu import GATES          # noqa: E402

GATE = 1e-3          # module outputs and gradients (README)
KERNEL = 1e-6          # fp32 streaming kernels against fp64


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ---- kernels -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,h,w,cz', [(2, 5, 7, 3), (2, 5, 7, 4), (1, 64, 64, 4)])
def test_tanh_head_forward_backward_vs_fp64(n, h, w, cz):
    from latent_pose_reenactment_amd import hipops as ops
    g = torch.Generator().manual_seed(n * 1000 + h * 10 + cz)
    z = (torch.randn(n, h, w, cz, generator=g) * 1.5).cuda()
    d = torch.randn(n, 3, h, w, generator=g).cuda()
    t, rgbs = ops.tanh_head_fwd(z)
    t64 = torch.tanh(z.double()[..., :3])
    _, rgbs_only = ops.tanh_head_fwd(z, want_t=False)
    dz = ops.tanh_head_bwd(t, d, amax=True)
    torch.cuda.synchronize()
    dz64 = d.double().permute(0, 2, 3, 1) * (1 - t64 * t64)
    errs = {'fake_rgbs': rel(rgbs, t64.permute(0, 3, 1, 2)), 't': rel(t[..., :3], t64), 'dz': rel(dz[..., :3], dz64)}
    print(f'[kernel] tanh head {(n, h, w, cz)}: {errs}')
    assert tuple(rgbs.shape) == (n, 3, h, w) and torch.equal(rgbs, rgbs_only) and torch.equal(rgbs, t[..., :3].permute(0, 3, 1, 2))
    assert all(v < KERNEL for v in errs.values()), errs
    if cz == 4:
        assert torch.count_nonzero(dz[..., 3]) == 0 and torch.count_nonzero(t[..., 3]) == 0          # the padding channel: exact zeros
    slots, version = dz._lp_amax
    assert version == dz._version and float(slots.max()) == float(dz.abs().max()) > 0          # folded max|dz|: the same float
    assert torch.equal(ops.tanh_head_bwd(t, d), dz)          # (without the folded maximum: the same values)


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('n,c', [(1, 8), (3, 20), (8, 512)])
def test_norm_affine_grad_vs_fp64_and_bit_reproducible(n, c, accumulate):
    from latent_pose_reenactment_amd import hipops as ops
    g = torch.Generator().manual_seed(n * 100 + c)
    wide = torch.randn(n, 3 * c + 5, generator=g).cuda()          # rows inside a wider buffer, like the slices of the projector-output gradient
    dg, db = wide[:, 2:2 + c], wide[:, c + 3:2 * c + 3]
    base_g, base_b = torch.randn(c, generator=g).cuda(), torch.randn(c, generator=g).cuda()

    def run():
        if not accumulate:
            return ops.norm_affine_grad(dg, db)
        ag, ab = base_g.clone(), base_b.clone()
        assert ops.norm_affine_grad(dg, db, ag, ab) == (None, None)
        return ag, ab
    og, ob = run()
    og2, ob2 = run()
    torch.cuda.synchronize()
    want_g = dg.double().sum(0) + (base_g.double() if accumulate else 0)
    want_b = db.double().sum(0) + (base_b.double() if accumulate else 0)
    errs = {'dgamma': rel(og, want_g), 'dbeta': rel(ob, want_b)}
    print(f'[kernel] norm_affine_grad {(n, c)} accumulate={accumulate}: {errs}')
    assert all(v < KERNEL for v in errs.values()), errs
    assert torch.equal(og, og2) and torch.equal(ob, ob2)          # fixed summation order: the same bits
    if not accumulate:          # ... and the order is rows 0 .. n-1
        seq = dg[0].clone()
        for i in range(1, n):
            seq = seq + dg[i]
        assert torch.equal(og, seq)


# ---- the module against the reference's fixture, toy geometry, bf16x3 -----------------------------------------------------------------------------------
def gate(errs, what):
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    outs = [(k, f'{v:.2e}') for k, v in errs.items() if k.endswith('fake_rgbs')]
    print(f'[parity] {what}: outputs {outs}; worst', [(k, f'{v:.2e}') for k, v in worst])
    bad = {k: v for k, v in errs.items() if v >= (1e-5 if k.startswith('buf.') else GATE)}
    assert not bad, bad


def toy_generator(z, prefix, monkeypatch, finetuned=False):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    G = plugin('generators', 'FSTH').Wrapper.get_net(gen_args())
    if finetuned:
        G.enable_finetuning()
    G.load_state_dict(sd_of(z, prefix), strict=True)
    return G.cuda()


def test_generator_vs_reference_golden(monkeypatch):
    z = fixture('fsth_generator_small.npz')
    G = toy_generator(z, 'sd.', monkeypatch).train()
    embeds = torch.from_numpy(z['embeds']).cuda().requires_grad_(True)
    stick, r = torch.from_numpy(z['dec_stickmen']).cuda(), torch.from_numpy(z['r']).cuda()
    dd = dict(embeds=embeds, dec_stickmen=stick)
    G(dd)
    assert set(dd) == {'embeds', 'dec_stickmen', 'fake_rgbs'} and tuple(dd['fake_rgbs'].shape) == (2, 3, 32, 32)
    (dd['fake_rgbs'] * r).sum().backward()
    errs = {'fake_rgbs': rel(dd['fake_rgbs'], z['fake_rgbs']), 'grad_embeds': rel(embeds.grad, z['grad_embeds'])}
    for k, p in G.named_parameters():
        assert p.grad is not None, k
        errs['grad.' + k] = grad_figure(k, p.grad, z, 'grad.')
    for k, v in G.state_dict().items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['buf.' + k] = rel(v, z['sd_after.' + k])
    G.eval()
    bufs = {k: v.clone() for k, v in G.state_dict().items() if k.endswith('_u') or k.endswith('_v')}
    with torch.no_grad():
        de = dict(embeds=embeds.detach(), dec_stickmen=stick)
        G(de)
        again = dict(embeds=embeds.detach(), dec_stickmen=stick)
        G(again)          # (cached packs)
    errs['eval_fake_rgbs'] = rel(de['fake_rgbs'], z['eval_fake_rgbs'])
    assert torch.equal(de['fake_rgbs'], again['fake_rgbs'])
    assert all(torch.equal(G.state_dict()[k], v) for k, v in bufs.items())          # eval: no power iteration
    # the fine-tuning bootstrap on the GPU, from the buffers the train forward left: project(e_hat) in eval mode -> the reference's [1, C] values
    G.train()
    G.enable_finetuning({'embeds': torch.from_numpy(z['e_hat']).cuda()})
    assert G.training and list(G.state_dict()) == list(z['ft_sd_keys'])
    for k, v in G.state_dict().items():
        if not (k.endswith('_u') or k.endswith('_v') or k.endswith('weight_orig')) and 'decoder_blocks' in k and z['ft_sd.' + k].ndim == 2:
            errs['ft_sd.' + k] = rel(v, z['ft_sd.' + k])
    gate(errs, 'generator FSTH, toy geometry (bf16x3)')
    with pytest.raises(ValueError, match='bottleneck'):          # 16 / 2^3: a 2 x 2 bottleneck
        G({'dec_stickmen': stick[..., :16, :16].contiguous()})


def test_finetuned_generator_vs_reference_golden(monkeypatch):
    z = fixture('fsth_generator_small.npz')
    G = toy_generator(z, 'ft_sd.', monkeypatch, finetuned=True).train()
    assert [k for k, _ in G.named_parameters()] == list(z['ft_param_order'])
    dd = dict(dec_stickmen=torch.from_numpy(z['dec_stickmen']).cuda())
    G(dd)          # no ``embeds``: the projector is not run
    (dd['fake_rgbs'] * torch.from_numpy(z['r']).cuda()).sum().backward()
    errs = {'ft_fake_rgbs': rel(dd['fake_rgbs'], z['ft_fake_rgbs'])}
    params = dict(G.named_parameters())
    assert params['project.weight_orig'].grad is None and params['project.bias'].grad is None
    names = [k[len('ft_grad.'):] for k in z.files if k.startswith('ft_grad.')]
    assert sum(params[k].dim() == 2 and params[k].shape[0] == 1 for k in names) == 22
    for k in names:
        errs['ft_grad.' + k] = grad_figure(k, params[k].grad, z, 'ft_grad.')
    for k, v in G.state_dict().items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['buf.' + k] = rel(v, z['ft_sd_after.' + k])          # (the projector's buffers stay: it is out of the power iteration)
    gate(errs, 'fine-tuned generator FSTH, toy geometry (bf16x3)')


# ---- mid geometry against the fp64 restatement, tie-masked ---------------------------------------------------------------------------------------------
def count_calls(monkeypatch, mod, name, key):
    calls, real = [], getattr(mod, name)

    def counted(*a, **k):
        calls.append(key(a, k))
        return real(*a, **k)
    monkeypatch.setattr(mod, name, counted)
    return calls


def run_vs_fp64(monkeypatch, size, what, nc=64, mx=128, emb=64, nd=3, nr=1):
    """image ``size``, num_channels ``nc``, max ``mx``, embed ``emb``, ``nd`` downsample + ``nr`` residual blocks, B = 2, bf16x3 -> (forward error,
    tie-masked gradient errors, untied errors, route counters).  The defaults are the mid geometry; the full geometry (256, 64, 512, 512, 4, 4) is
    measured by hand with this same code (its fp64 side is too slow for the suite)."""
    from latent_pose_reenactment_amd import hipops as ops, nn as lpnn
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    a = gen_args(image_size=size, num_channels=nc, max_num_channels=mx, embed_channels=emb, gen_num_downsample_blocks=nd, gen_num_residual_blocks=nr,
                 device='cuda')
    torch.manual_seed(0)
    G = plugin('generators', 'FSTH').Wrapper.get_net(a).train()
    with torch.no_grad():          # gamma / beta off their ones / zeros initial values
        for k, p in G.named_parameters():
            if k.startswith('down_blocks') and p.dim() == 1 and '.block.' in k and not k.endswith('weight_orig'):
                p.add_(0.3 * torch.randn_like(p))
    g = torch.Generator().manual_seed(5)
    mod = plugin('dataloaders', 'synthetic_voxceleb2_stickmen')
    stick = torch.stack([mod.draw_stickman(mod.face_keypoints(g), size) for _ in range(2)])[:, None]
    embeds0 = torch.randn(2, emb, generator=g)
    r = torch.randn(2, 3, size, size, generator=g)
    with torch.no_grad():
        for _ in range(3):                  # settle the power iterations
            G({'embeds': embeds0.cuda(), 'dec_stickmen': stick.cuda()})
    sd = {k: v.detach().cpu().clone() for k, v in G.state_dict().items()}
    routes = {'thin_conv': count_calls(monkeypatch, ops, 'thin_conv', lambda a_, k: k.get('ksize')),
              'conv16': count_calls(monkeypatch, ops, 'conv16', lambda a_, k: ('pool' if k.get('phase_dgrad') and k.get('res') is not None else
                                                                                'phase_dgrad' if k.get('phase_dgrad') else 'phase' if k.get('phase') else
                                                                                'stats' if k.get('stats') else 'plain')),
              'finalize': count_calls(monkeypatch, ops, 'norm_stats_finalize', lambda a_, k: 1),
              'instnorm': count_calls(monkeypatch, ops, 'instnorm_stats', lambda a_, k: 1),
              'reduce': count_calls(monkeypatch, ops, 'norm_affine_grad', lambda a_, k: 1)}
    embeds = embeds0.clone().cuda().requires_grad_(True)
    dd = {'embeds': embeds, 'dec_stickmen': stick.cuda()}
    G._debug = {}
    G(dd)
    masks = [(pl > 0).permute(0, 3, 1, 2).cpu() for pl in G._debug['relu_planes']]          # int16 > 0 <=> value > 0
    G._debug = None
    params = dict(G.named_parameters())
    grads = torch.autograd.grad((dd['fake_rgbs'] * r.cuda()).sum(), [embeds] + list(params.values()))
    torch.cuda.synchronize()
    counts = {k: list(v) for k, v in routes.items()}
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def oracle(replay):
        st = {k: v.double() if v.is_floating_point() else v.clone() for k, v in sd.items()}
        for k in params:
            st[k].requires_grad_(True)
        e = embeds0.double().requires_grad_(True)
        taps = []
        R.RELU_REPLAY = None if replay is None else list(replay)
        try:
            out = GR.generator_forward(st, e, stick.double(), training=True, taps=taps)
        finally:
            left = None if R.RELU_REPLAY is None else len(R.RELU_REPLAY)
            R.RELU_REPLAY = None
        assert not left, f'{left} recorded ReLU sites were not consumed by the restatement'
        return out, torch.autograd.grad((out * r.double()).sum(), [e] + [st[k] for k in params]), taps
    out, g_true, taps = oracle(None)
    assert len(taps) == len(masks) == 1 + 2 * (nd - 1) + 2 * nr + 2 * nd + 1
    masks = [m[:, :t.shape[1]] for m, t in zip(masks, taps)]          # (operand planes carry channels rounded up to 8)
    check_tie_condition(masks, taps, UNIT['bf16x3'], what)
    _, g_tied, _ = oracle(masks)
    names = ['d_embeds'] + list(params)

    def table(ref):
        t = {}
        for n_, a_, c_ in zip(names, grads, ref):
            if n_ != 'd_embeds' and null_gradient(n_):          # true gradient zero: on the scale of the layer's weight gradient
                scale = ref[names.index(n_[:-4] + 'weight_orig')].norm()
                t[n_] = ((a_.double().cpu() - c_).norm() / scale).item()
            else:
                t[n_] = rel(a_, c_)
        return t
    return {'fake_rgbs': rel(dd['fake_rgbs'], out)}, table(g_tied), table(g_true), counts


def test_mid_geometry_vs_fp64_restatement_with_routes(monkeypatch):
    from latent_pose_reenactment_amd import _lib, nn as lpnn
    assert _lib.lib().lp_thin_conv_supported(3, 64, 3, 64) == 1 and _lib.lib().lp_thin_conv_supported(3, 64, 1, 32) == 1
    assert [lpnn.phase_conv(True, s, False) for s in (16, 32, 64)] == [True] * 3
    errs, gerr, untied, counts = run_vs_fp64(monkeypatch, 64, 'generator FSTH, mid geometry (bf16x3)')
    worst = sorted(gerr.items(), key=lambda kv: -kv[1])[:4]
    print(f'[parity-mid] generator FSTH 64 x 64 (bf16x3): forward {errs}; tie-masked grads worst {[(n, f"{v:.2e}") for n, v in worst]} over {len(gerr)} '
          f'tensors; untied worst {max(untied.values()):.3e} ({max(untied, key=untied.get)}); routes '
          f'{ {k: (len(v) if k != "conv16" else {x: v.count(x) for x in set(v)}) for k, v in counts.items()} }')
    # routes: thin stem (3x3 on the stickman, 1x1 on its pooled copy; the third thin launch is the head's data gradient -- the stickman itself gets
    # none), one 4x4 stride-2 conv + pool launch per encoder stage (their data gradients are phase-form launches), the three up convs in their
    # phase forms forward and backward, statistics from conv epilogues, one affine reduction per InstanceNorm
    assert counts['thin_conv'] == [3, 1, 3], counts['thin_conv']
    c16 = counts['conv16']
    assert (c16.count('pool'), c16.count('phase'), c16.count('phase_dgrad')) == (3, 3 + 3, 3), {x: c16.count(x) for x in set(c16)}
    assert len(counts['finalize']) >= 1 and len(counts['reduce']) == 4
    assert all(v < GATE for v in errs.values()), errs
    assert all(v < GATE for v in gerr.values()), worst


# ---- one training iteration of the runner ------------------------------------------------------------------------------------------------------------
def test_one_iteration_matches_reference_run_epoch(monkeypatch):
    """scheme of tests/test_fsth_modules_gpu.py::test_one_iteration_matches_reference_run_epoch, bf16x3.
    The generator's ``null_gradient`` biases (true gradient exactly zero: their conv feeds only instance norms) are moved by Adam on rounding noise
    alone -- the reference by up to 0.02 lr (|g| ~ 2e-7 against eps 1e-5), these kernels by up to 0.07 lr (bf16x3 gradient operands: 2^-17 against fp32's
    2^-24) -- so the post-step difference of such a 4-element bias says nothing relative to ITS OWN norm (measured: down_block.4.bias 1.4e-4,
    skip.0.bias 5.5e-5 of it).  They are measured with their layer instead: the difference relative to the norm of the layer's weight, under the same
    gate, and under the scheme's absolute bound of 2 lr for elements whose gradient is ~0."""
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    from criterions import adversarial, featmat
    from runners import holycow
    z = fixture('fsth_generator_train_step_small.npz')
    a = gen_args(device='cuda', optimizer='Adam', lr_gen=5e-4, lr_dis=8e-4, beta1=0.0, finetune=False, num_gpus=1)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a)
    G = plugin('generators', 'FSTH').Wrapper.get_net(a)
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(a)
    st = step_states(z)
    E.load_state_dict(st['E']); G.load_state_dict(st['G']); D.load_state_dict(st['D'])
    crits = [adversarial.Criterion('gan'), featmat.Criterion(10.0), plugin('criterions', 'l1_rgb').Criterion(30.0)]
    tm = holycow.TrainingModule(E, G, D, crits, [], {})
    opt_G = holycow.get_optimizer(E, G, a)
    opt_D = plugin('discriminators', 'FSTH').Wrapper.get_optimizer(D, a)
    tm.train()
    data = {k[len('init.in.'):]: torch.from_numpy(z[k]).cuda() for k in z.files if k.startswith('init.in.') and 'segm' not in k and 'label' not in k}
    target = {'real_segm': torch.from_numpy(z['init.in.real_segm']).cuda(), 'label': torch.from_numpy(z['init.in.label']).cuda()}
    all_data, lG, lD = holycow.train_step(tm, data, target, opt_G, opt_D, a)
    torch.cuda.synchronize()
    assert 'fake_segm' not in all_data
    g_loss, g_state, g_flip = GATES['bf16x3']
    errs, flips = {}, {}
    assert set(lG) == {'adversarial_G', 'feature_matching', 'l1_rgb'} and set(lD) == {'adversarial_D'}
    for name, v in {**lG, **lD}.items():
        errs['loss.' + name] = rel(v, z[f'loss.{name}'])
    mods = (('E', tm.embedder, a.lr_gen), ('G', tm.generator, a.lr_gen), ('D', tm.discriminator, a.lr_dis),
            ('E_ema', tm.running_averages['embedder'], a.lr_gen), ('G_ema', tm.running_averages['generator'], a.lr_gen))
    for nm, mod, lr in mods:
        init = st[nm[0]]
        for k, v in mod.state_dict().items():
            want = z[f'after.{nm}.{k}']
            v = v.detach().cpu()
            errs[f'{nm}.{k}'] = rel(v, want)
            if nm.startswith('G') and null_gradient(k):
                errs[f'{nm}.{k}'] = float(np.linalg.norm(v.numpy() - want) / np.linalg.norm(z[f'after.{nm}.{k[:-4]}weight_orig']))
                assert np.abs(v.numpy() - want).max() <= 2.02 * lr, (nm, k)
            if v.dtype == torch.float32 and (k.endswith('weight_orig') or k.endswith('weight')) and not nm.endswith('_ema'):
                ref_delta = want - init[k].numpy()
                got_delta = v.numpy() - init[k].numpy()
                if np.linalg.norm(ref_delta) > 1e-7 * max(1.0, np.linalg.norm(want)):
                    assert np.abs(got_delta - ref_delta).max() <= 2.02 * lr, (nm, k, np.abs(got_delta - ref_delta).max(), lr)
                    moved = np.abs(ref_delta) > 0.5 * lr
                    if moved.any():
                        flips[f'{nm}.{k}'] = float((np.sign(got_delta[moved]) != np.sign(ref_delta[moved])).mean())
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:6]
    print(f'[parity] FSTH generator train step (Adam, bf16x3): worst', [(k, f'{v:.2e}') for k, v in worst],
          'Adam direction flips (worst tensors):', sorted(((round(v, 4), k) for k, v in flips.items()), reverse=True)[:3])
    bad = {k: v for k, v in errs.items() if v >= (g_loss if k.startswith('loss.') else g_state)}
    assert not bad, bad
    assert flips and float(np.mean(list(flips.values()))) <= g_flip, flips


# ---- entry point ---------------------------------------------------------------------------------------------------------------------------------------
def test_train_entry_two_iterations(tmp_path):
    cmd = [sys.executable, os.path.join(PKG, 'train.py'), '--embedder', 'FSTH', '--generator', 'FSTH', '--discriminator', 'FSTH',
           '--criterions', 'adversarial, featmat, l1_rgb', '--runner', 'holycow', '--dataloader', 'synthetic_voxceleb2_stickmen',
           '--image_size', '64', '--num_channels', '8', '--max_num_channels', '32', '--embed_channels', '16', '--num_labels', '20',
           '--dis_num_blocks', '5', '--embed_num_blocks', '4', '--gen_num_downsample_blocks', '3', '--gen_num_residual_blocks', '1',
           '--batch_size', '2', '--synthetic_dataset_len', '4', '--n_frames_for_encoder', '2', '--num_epochs', '1', '--num_gpus', '1',
           '--log_frequency_loss', '1', '--experiments_dir', str(tmp_path), '--experiment_name', 'fsth_generator']
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ckpts = sorted(os.listdir(os.path.join(str(tmp_path), 'fsth_generator', 'checkpoints')))
    assert ckpts == ['model_00000002.pth'], ckpts
    ck = torch.load(os.path.join(str(tmp_path), 'fsth_generator', 'checkpoints', ckpts[-1]), map_location='cpu', weights_only=False)
    assert ck['args'].iteration == 2 and ck['args'].generator == 'FSTH'
    sd = ck['generator']
    assert 'project.weight_orig' in sd and 'down_blocks.1.block.4.weight' in sd and 'decoder_blocks.7.weight_orig' in sd
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    line = [l for l in r.stdout.splitlines() if 'Epoch 0 (iteration' in l][-1]
    assert 'Loss_l1_rgb' in line and 'Loss_segmentation_dice' not in line, line
