#!/usr/bin/env python3
"""Golden fixtures of the stickman-to-image generator (generators/FSTH.py), made by importing the REAL reference like make_golden_fsth.py (whose
helpers and toy geometry this script shares).  Nothing of the reference travels: the outputs are plain .npz files under tests/golden/.
Run:  python tests/golden/make_golden_fsth_generator.py [generator] [train_step]          (CPU only, ~2 min)

  fsth_generator_small.npz             image 32, num_channels 4, max_num_channels 16, embed_channels 8, 3 downsample + 2 residual blocks, B = 2 (the
                                       per-sample affine and the batch-shared gamma / beta reduction both need two samples): state dict, parameter
                                       order, inputs, train-mode fake_rgbs, gradients of a random-projection loss w.r.t. embeds and every parameter,
                                       the spectral-norm buffers after the forward, the eval-mode output, and the fine-tuning leg (state dict after
                                       enable_finetuning, its output, the gradients of the [1, C] parameters)
  fsth_generator_train_step_small.npz  one runners/holycow.run_epoch iteration of embedder FSTH + generator FSTH + discriminator FSTH with
                                       adversarial + featmat + l1_rgb and Adam, recorded as make_golden_fsth.make_train_step records its step

Seeds: the one with the LARGEST ReLU tie margin (min |pre-ReLU| / rms over all ReLU sites of the train forward) of the search range; recorded."""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_fsth as M          # noqa: E402  (puts the reference on sys.path, stubs cv2 / yamlenv)
from make_golden_fsth import MARGIN, OUT, TieMargin, npy, sd_np, stick_images          # noqa: E402

from generators import FSTH as ref_gen          # noqa: E402

GEN = dict(gen_num_downsample_blocks=3, gen_num_residual_blocks=2)


def gen_args():
    a = M.small_args()
    for k, v in GEN.items():
        setattr(a, k, v)
    return a


def make_generator():
    args = gen_args()
    B, E, S = 2, args.embed_channels, args.image_size

    def build(seed):
        torch.manual_seed(seed)
        G = ref_gen.Wrapper.get_net(args)
        g = torch.Generator().manual_seed(seed)
        return G, g, torch.randn(B, E, generator=g), stick_images((B, 1, 3, S, S), g)

    best = (-1.0, None, 0)
    for seed in range(0, 300):
        G, g, embeds, stick = build(seed)
        G.train()
        tm = TieMargin(G)
        with torch.no_grad():
            G(dict(embeds=embeds, dec_stickmen=stick))
        sites = len(tm.margins)
        best = max(best, (tm.close(), seed, sites))
    margin, seed, sites = best
    print(f'generator FSTH: seed {seed}, ReLU tie margin {margin:.2e} over {sites} sites')
    assert margin > MARGIN and sites == 16
    G, g, embeds, stick = build(seed)
    G.train()
    out = dict(cfg=np.array([S, args.num_channels, args.max_num_channels, E, GEN['gen_num_downsample_blocks'], GEN['gen_num_residual_blocks']]),
               seed=np.array(seed), margin=np.array(margin), relu_sites=np.array(sites), num_affine_params=np.array(G.get_num_affine_params()))
    out.update(sd_np(G, 'sd.'))
    out['sd_keys'] = np.array(list(G.state_dict()))
    out['param_order'] = np.array([k for k, _ in G.named_parameters()])
    r = torch.randn(B, 3, S, S, generator=g)
    e_hat = torch.randn(1, E, generator=g)
    embeds.requires_grad_(True)
    dd = dict(embeds=embeds, dec_stickmen=stick)
    G(dd)
    assert set(dd) == {'embeds', 'dec_stickmen', 'fake_rgbs'}
    (dd['fake_rgbs'] * r).sum().backward()
    out.update(embeds=npy(embeds), dec_stickmen=npy(stick), r=npy(r), e_hat=npy(e_hat), fake_rgbs=npy(dd['fake_rgbs']), grad_embeds=npy(embeds.grad))
    for k, p in G.named_parameters():
        out[f'grad.{k}'] = npy(p.grad)
    out.update({k: v for k, v in sd_np(G, 'sd_after.').items() if k.endswith('_u') or k.endswith('_v')})
    # eval mode, from the buffers the train forward left: no power iteration, the statistics still per sample
    def twin():          # (a net that ran a forward cannot be deep-copied: the spectral-norm hook leaves non-leaf tensors behind)
        T = ref_gen.Wrapper.get_net(args)
        T.load_state_dict(G.state_dict())
        return T
    Ge = twin().eval()
    with torch.no_grad():
        de = dict(embeds=embeds.detach(), dec_stickmen=stick)
        Ge(de)
    out['eval_fake_rgbs'] = npy(de['fake_rgbs'])
    # fine-tuning leg, from the same buffers: the AdaIN parameters become [1, C] nn.Parameters holding project(e_hat) (taken in eval mode)
    Gf = twin().train()
    Gf.enable_finetuning({'embeds': e_hat.clone()})
    assert Gf.finetuning and Gf.training
    out.update(sd_np(Gf, 'ft_sd.'))
    out['ft_sd_keys'] = np.array(list(Gf.state_dict()))
    out['ft_param_order'] = np.array([k for k, _ in Gf.named_parameters()])
    df = dict(dec_stickmen=stick)
    Gf(df)
    (df['fake_rgbs'] * r).sum().backward()
    out['ft_fake_rgbs'] = npy(df['fake_rgbs'])
    for k, p in Gf.named_parameters():
        if p.grad is not None and p.grad.abs().max() > 0:          # (the projector is not run: no gradient)
            out[f'ft_grad.{k}'] = npy(p.grad)
    out.update({k: v for k, v in sd_np(Gf, 'ft_sd_after.').items() if k.endswith('_u') or k.endswith('_v')})
    np.savez_compressed(os.path.join(OUT, 'fsth_generator_small.npz'), **out)
    print('fsth_generator_small.npz', len(out), 'arrays; G params', sum(p.numel() for p in G.parameters()), 'n_aff', G.get_num_affine_params())


def make_train_step():
    """make_golden_fsth.make_train_step with generators/FSTH.py in the generator's place and without dice (there is no fake_segm)"""
    for name in ('tqdm',):
        if name not in sys.modules:
            m = types.ModuleType(name); m.tqdm = lambda x, *a, **k: x; sys.modules[name] = m
    from runners import holycow as ref_runner
    ref_emb, ref_dis = M.ref_emb_fsth, M.ref_dis
    args = gen_args()
    args.optimizer = 'Adam'; args.lr_gen = 5e-4; args.lr_dis = 8e-4; args.beta1 = 0.0
    args.finetune = False; args.num_gpus = 1; args.detailed_metrics = True; args.gan_type = 'gan'

    def build(seed):
        torch.manual_seed(seed)
        E, G, D = ref_emb.Wrapper.get_net(args), ref_gen.Wrapper.get_net(args), ref_dis.Wrapper.get_net(args)
        g = torch.Generator().manual_seed(seed)
        data = {'enc_rgbs': torch.rand(2, 2, 3, 32, 32, generator=g), 'enc_stickmen': stick_images((2, 2, 3, 32, 32), g),
                'target_rgbs': torch.rand(2, 1, 3, 32, 32, generator=g), 'dec_stickmen': stick_images((2, 1, 3, 32, 32), g)}
        target = {'real_segm': torch.rand(2, 1, 1, 32, 32, generator=g).expand(2, 1, 3, 32, 32).contiguous(), 'label': torch.tensor([3, 1])}
        return E, G, D, data, target

    best = (-1.0, None)
    for seed in range(11, 211):
        E, G, D, data, target = build(seed)
        tE, tG, tD = ref_emb.Wrapper.get_net(args), ref_gen.Wrapper.get_net(args), ref_dis.Wrapper.get_net(args)
        for twin, src in ((tE, E), (tG, G), (tD, D)):
            twin.load_state_dict(src.state_dict()); twin.train()
        tm_ = TieMargin(tE, tG, tD)
        hook = tE.down_blocks.register_forward_hook(lambda _m, _i, o: tm_.see(o))
        with torch.no_grad():
            d0 = dict(data); tE(d0); tG(d0); d0.update(target); tD(d0)
            tm_.see(d0['fake_features'][-1]); tm_.see(d0['real_features'][-1])
        hook.remove()
        best = max(best, (tm_.close(), seed))
    margin, seed = best
    E, G, D, data, target = build(seed)
    print(f'train step FSTH generator: seed {seed}, ReLU tie margin {margin:.2e}')
    crits = [M.ref_adv.Criterion('gan'), M.ref_fm.Criterion(10.0), M.ref_l1.Criterion(30.0)]
    tm = ref_runner.TrainingModule(E, G, D, crits, [], {})
    opt_G = ref_runner.get_optimizer(tm.embedder, tm.generator, args)
    opt_D = ref_dis.Wrapper.get_optimizer(tm.discriminator, args)
    tm.train()
    out = dict(margin=np.array(margin), seed=np.array(seed))
    for nm, mod in (('E', tm.embedder), ('G', tm.generator), ('D', tm.discriminator)):
        out.update(sd_np(mod, f'init.{nm}.'))
    for k, v in {**data, **target}.items():
        out['init.in.' + k] = npy(v)
    captured = {}
    orig_fwd = tm.embedder.forward

    def rec_fwd(d):
        orig_fwd(d)
        captured['embeds'] = d['embeds'].detach().clone(); captured['elemwise'] = d['embeds_elemwise'].detach().clone()
    tm.embedder.forward = rec_fwd
    meters = []
    BaseMeter = ref_runner.Meter

    class RecordingMeter(BaseMeter):          # run_epoch does not return its Meter
        def __init__(self):
            super().__init__()
            meters.append(self)
    ref_runner.Meter = RecordingMeter
    try:
        ref_runner.run_epoch([(data, target)], tm, opt_G, opt_D, 0, args, phase='train', writer=None)
    finally:
        ref_runner.Meter = BaseMeter
    meter = meters[0]
    out['embeds'] = npy(captured['embeds']); out['embeds_elemwise'] = npy(captured['elemwise'])
    for key in meter.keys():
        if key.startswith('Loss_'):
            out['loss.' + key[len('Loss_'):]] = np.array(meter.get_last(key))
    for nm, mod in (('E', tm.embedder), ('G', tm.generator), ('D', tm.discriminator), ('E_ema', tm.running_averages['embedder']),
                    ('G_ema', tm.running_averages['generator'])):
        out.update(sd_np(mod, f'after.{nm}.'))
    np.savez_compressed(os.path.join(OUT, 'fsth_generator_train_step_small.npz'), **out)
    print('fsth_generator_train_step_small.npz', len(out), 'arrays; losses', {k: float(v) for k, v in out.items() if k.startswith('loss.')})


if __name__ == '__main__':
    torch.set_num_threads(1)
    for w in (sys.argv[1:] or ['generator', 'train_step']):
        globals()['make_' + w]()
    for f in ('fsth_generator_small.npz', 'fsth_generator_train_step_small.npz'):
        path = os.path.join(OUT, f)
        if os.path.exists(path):
            print(f, os.path.getsize(path), 'bytes')
