#!/usr/bin/env python3
"""Golden fixtures of the FSTH plugin family (embedders/FSTH.py, embedders/no_pose_encoder.py, discriminators/FSTH.py, criterions/l1_rgb.py), made by
importing the REAL reference from /root/reference (build container only), like make_golden.py.  Nothing of the reference travels: the outputs are
plain .npz files (inputs + expected outputs) under tests/golden/.
Run:  python tests/golden/make_golden_fsth.py [embedders] [discriminator] [train_step]          (CPU only, ~1 min)

Toy geometry: image 32, num_channels 4, max_num_channels 16, embed_channels 8, embed_num_blocks 4 (maps 32 -> 16 -> 8 -> 4 -> 2: every conv sees
W >= 4), dis_num_blocks 5, 5 labels.  Seeds are chosen by a ReLU-tie-margin search (smallest |pre-ReLU| relative to its tensor's RMS over every
ReLU of the train forward; the fixture records it): two correct fp32 implementations may disagree on the mask of an element whose pre-activation
is ~1e-7, which in these tiny nets is a visible gradient change."""
import argparse
import os
import sys
import types

import numpy as np
import torch
from torch import nn

REF = '/root/reference'
OUT = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-4

for name in ('cv2', 'yamlenv'):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules['cv2'].setNumThreads = lambda *_: None
sys.modules['cv2'].ocl = types.SimpleNamespace(setUseOpenCL=lambda *_: None)
sys.path.insert(0, REF)
os.chdir(REF)

from embedders import FSTH as ref_emb_fsth, no_pose_encoder as ref_emb_nopose            # noqa: E402
from discriminators import FSTH as ref_dis                                                  # noqa: E402
from generators import FSTH_plus as ref_gen                                                 # noqa: E402
from criterions import adversarial as ref_adv, featmat as ref_fm, dice as ref_dice, dis_embed as ref_de, l1_rgb as ref_l1      # noqa: E402

SMALL = dict(image_size=32, num_channels=4, max_num_channels=16, embed_channels=8, in_channels=3, out_channels=3, num_labels=5, dis_num_blocks=5,
             embed_num_blocks=4)


def npy(t):
    return t.detach().cpu().numpy().copy()


def sd_np(module, prefix):
    return {f'{prefix}{k}': npy(v) for k, v in module.state_dict().items()}


def small_args(average_function='sum'):
    a = argparse.Namespace(**SMALL)
    a.embed_padding = 'zero'; a.dis_padding = 'zero'; a.gen_padding = 'zero'; a.average_function = average_function; a.device = 'cpu'
    a.norm_layer = 'in'; a.gen_constant_input_size = 4; a.gen_num_residual_blocks = 2
    a.pose_embedding_size = 6          # = 2 * number of keypoints of this toy (136 in the 68-landmark configuration)
    return a


class TieMargin:
    """records min |x| / rms(x) over the inputs of every nn.ReLU of ``modules`` and over the tensors handed to ``see`` (functional ReLUs)"""

    def __init__(self, *modules):
        self.margins = []
        self.hooks = [m.register_forward_pre_hook(lambda _m, inp: self.see(inp[0])) for mod in modules for m in mod.modules() if isinstance(m, nn.ReLU)]

    def see(self, x):
        self.margins.append((x.detach().abs().min() / x.detach().pow(2).mean().sqrt()).item())

    def close(self):
        for h in self.hooks:
            h.remove()
        return min(self.margins)


def stick_images(shape, g):
    """a stand-in for rendered stickmen: sparse images in [0, 1] (most pixels exactly 0, like drawn lines)"""
    return torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) < 0.15)


# ---- embedders ---------------------------------------------------------------------------------------------------------------------------------
def embedder_margin(wrapper, args, sd, data):
    twin = wrapper.get_net(args); twin.load_state_dict(sd); twin.train()
    tm = TieMargin(twin)
    hook = twin.down_blocks.register_forward_hook(lambda _m, _i, out: tm.see(out))          # the functional torch.relu behind the blocks
    with torch.no_grad():
        twin(dict(data))
    hook.remove()
    return tm.close()


def make_embedders():
    for ename, wrapper in (('FSTH', ref_emb_fsth.Wrapper), ('no_pose_encoder', ref_emb_nopose.Wrapper)):
        out = dict(cfg=np.array([SMALL[k] for k in ('image_size', 'num_channels', 'max_num_channels', 'embed_channels', 'embed_num_blocks')]))
        for avg in ('sum', 'max'):
            args = small_args(avg)
            for seed in range(2, 400):
                torch.manual_seed(seed)
                E = wrapper.get_net(args)
                g = torch.Generator().manual_seed(seed)
                rgbs = torch.rand(2, 3, 3, 32, 32, generator=g)
                stick = stick_images((2, 3, 3, 32, 32), g)
                margin = embedder_margin(wrapper, args, E.state_dict(), dict(enc_rgbs=rgbs, enc_stickmen=stick))
                if margin > MARGIN:
                    break
            else:
                raise RuntimeError('no seed with a safe ReLU tie margin found')
            print(f'embedder {ename} {avg}: seed {seed}, ReLU tie margin {margin:.2e}')
            pre = f'{avg}.'
            out[pre + 'margin'] = np.array(margin)
            out.update(sd_np(E, pre + 'sd.'))
            out[pre + 'param_order'] = np.array([k for k, _ in E.named_parameters()])
            rgbs.requires_grad_(True); stick.requires_grad_(True)
            r1, r2 = torch.randn(2, 8, generator=g), torch.randn(2, 3, 8, generator=g)
            E.train()
            dd = dict(enc_rgbs=rgbs, enc_stickmen=stick)
            E(dd)
            ((dd['embeds'] * r1).sum() + (dd['embeds_elemwise'] * r2).sum()).backward()
            out.update({pre + 'enc_rgbs': npy(rgbs), pre + 'r1': npy(r1), pre + 'r2': npy(r2), pre + 'embeds': npy(dd['embeds']),
                        pre + 'embeds_elemwise': npy(dd['embeds_elemwise']), pre + 'grad_enc_rgbs': npy(rgbs.grad)})
            if stick.grad is not None:          # (no_pose_encoder does not read the stickmen)
                out.update({pre + 'enc_stickmen': npy(stick), pre + 'grad_enc_stickmen': npy(stick.grad)})
            for k, p in E.named_parameters():
                out[f'{pre}grad.{k}'] = npy(p.grad)
            out.update({k: v for k, v in sd_np(E, pre + 'sd_after.').items() if k.endswith('_u') or k.endswith('_v')})
        np.savez_compressed(os.path.join(OUT, f'fsth_embedder_{ename}_small.npz'), **out)
        print(f'fsth_embedder_{ename}_small.npz', len(out), 'arrays')


# ---- discriminator + cheap criterions (what make_golden.make_discriminator records, plus dec_stickmen and l1_rgb) ------------------------------------
def make_discriminator():
    args = small_args()
    for seed in range(3, 400):
        torch.manual_seed(seed)
        D = ref_dis.Wrapper.get_net(args)
        g = torch.Generator().manual_seed(seed)
        fake = torch.rand(2, 3, 32, 32, generator=g)
        real = torch.rand(2, 1, 3, 32, 32, generator=g)
        stick = stick_images((2, 1, 3, 32, 32), g)
        label = torch.tensor([3, 1])
        twin = ref_dis.Wrapper.get_net(args); twin.load_state_dict(D.state_dict()); twin.train()
        tm = TieMargin(twin)
        with torch.no_grad():
            d0 = dict(fake_rgbs=fake, target_rgbs=real, dec_stickmen=stick, label=label)
            twin(d0)
            tm.see(d0['fake_features'][-1]); tm.see(d0['real_features'][-1])          # the functional torch.relu in front of the projection head
        margin = tm.close()
        if margin > MARGIN:
            break
    else:
        raise RuntimeError('no seed with a safe ReLU tie margin found')
    print(f'discriminator FSTH: seed {seed}, ReLU tie margin {margin:.2e}')
    D.train()
    out = dict(cfg=np.array([args.image_size, args.dis_num_blocks, args.num_labels]), margin=np.array(margin))
    out.update(sd_np(D, 'sd.'))
    out['param_order'] = np.array([k for k, _ in D.named_parameters()])
    fake.requires_grad_(True)
    dd = dict(fake_rgbs=fake, target_rgbs=real, dec_stickmen=stick, label=label)
    D(dd)
    out.update(fake=npy(fake), real=npy(real), dec_stickmen=npy(stick), label=label.numpy())
    for k in ('fake_score_G', 'fake_score_D', 'real_score', 'real_embedding'):
        out[k] = npy(dd[k])
    for i, (f, r) in enumerate(zip(dd['fake_features'], dd['real_features'])):
        out[f'fake_feat{i}'] = npy(f)
        out[f'real_feat{i}'] = npy(r)
    dd['fake_segm'] = torch.rand(2, 1, 32, 32, generator=g).requires_grad_(True)
    dd['real_segm'] = torch.rand(2, 1, 1, 32, 32, generator=g).expand(2, 1, 3, 32, 32)
    dd['embeds_elemwise'] = torch.randn(2, 8, args.embed_channels, generator=g).requires_grad_(True)
    out.update(fake_segm=npy(dd['fake_segm']), real_segm=npy(dd['real_segm']), embeds_elemwise=npy(dd['embeds_elemwise']))
    lg, ld = ref_adv.Criterion('gan')(dd)
    fm = ref_fm.Criterion(10.0)(dd)
    dc = ref_dice.Criterion(1.0)(dd)
    de = ref_de.Criterion(1e-2)(dd)
    out.update(loss_adv_G=npy(lg['adversarial_G']), loss_adv_D=npy(ld['adversarial_D']), loss_fm=npy(fm['feature_matching']),
               loss_dice=npy(dc['segmentation_dice']), loss_dis_embed=npy(de['embedding_matching']))
    loss_G = lg['adversarial_G'] + fm['feature_matching'] + dc['segmentation_dice'] + de['embedding_matching']
    loss_G.backward(retain_graph=True)
    out.update(gG_fake=npy(fake.grad), gG_fake_segm=npy(dd['fake_segm'].grad), gG_elemwise=npy(dd['embeds_elemwise'].grad))
    for k, p in D.named_parameters():
        out[f'gradG.{k}'] = npy(p.grad)
    D.zero_grad()
    ld['adversarial_D'].backward()
    for k, p in D.named_parameters():
        out[f'gradD.{k}'] = npy(p.grad)
    out.update(sd_np(D, 'sd_after.'))
    # fine-tuning variant of the embedding (FSTH.py:110-136): 1 x E matrix with the default spectral-norm eps
    Df = ref_dis.Wrapper.get_net(args)
    Df.load_state_dict(D.state_dict())
    Df.train()
    e_hat = torch.randn(1, args.embed_channels, generator=g)
    Df.enable_finetuning({'embeds': e_hat.clone()})
    out.update(sd_np(Df, 'ft_sd.'))
    dd2 = dict(fake_rgbs=fake.detach(), target_rgbs=real, dec_stickmen=stick, label=torch.zeros(2, dtype=torch.long))
    Df(dd2)
    out.update(ft_fake_score_G=npy(dd2['fake_score_G']), ft_real_score=npy(dd2['real_score']), ft_real_embedding=npy(dd2['real_embedding']))
    # criterions/l1_rgb.py on its own
    f2 = torch.rand(2, 3, 32, 32, generator=g).requires_grad_(True)
    t2 = torch.rand(2, 1, 3, 32, 32, generator=g)
    l1 = ref_l1.Criterion(30.0)({'fake_rgbs': f2, 'target_rgbs': t2})['l1_rgb']
    l1.backward()
    out.update(l1_fake=npy(f2), l1_target=npy(t2), l1_loss=npy(l1), l1_grad=npy(f2.grad))
    np.savez_compressed(os.path.join(OUT, 'fsth_discriminator_small.npz'), **out)
    print('fsth_discriminator_small.npz', len(out), 'arrays; D params', sum(p.numel() for p in D.parameters()))


BIG, BIG_SEED = 4096, 77


def seeded_like(key, v):
    """values of a tensor too large to store (> BIG elements): uniform(-1, 1) / sqrt(fan_in) from a generator seeded by BIG_SEED and the key's bytes --
    tests/fsth_restatement.py draws the same"""
    g = torch.Generator().manual_seed(BIG_SEED + sum(key.encode()))
    return (torch.rand(v.shape, generator=g) * 2 - 1) / float(v.shape[-1]) ** 0.5


def summary(v):
    """(norm, dot with a seeded direction) of a tensor too large to store"""
    r = torch.randn(v.shape, generator=torch.Generator().manual_seed(BIG_SEED))
    return np.array([float(v.double().norm()), float((v.double() * r.double()).sum())])


# ---- one full training iteration of the reference runner on the FSTH configuration ------------------------------------------------------------------
def make_train_step():
    """runners/holycow.run_epoch for ONE meta-training batch: embedder FSTH, generator FSTH_plus, discriminator FSTH, criterions adversarial, featmat,
    l1_rgb, dice; Adam; the reference's own TrainingModule / get_optimizer.  Records losses, the embedder's outputs, post-step weights, EMA and
    spectral-norm buffers, as make_golden.make_train_step does."""
    for name in ('tqdm',):
        if name not in sys.modules:
            m = types.ModuleType(name); m.tqdm = lambda x, *a, **k: x; sys.modules[name] = m
    from runners import holycow as ref_runner
    args = small_args()
    args.optimizer = 'Adam'; args.lr_gen = 5e-4; args.lr_dis = 8e-4; args.beta1 = 0.0
    args.finetune = False; args.num_gpus = 1; args.detailed_metrics = True; args.gan_type = 'gan'
    def build(seed):
        torch.manual_seed(seed)
        E, G, D = ref_emb_fsth.Wrapper.get_net(args), ref_gen.Wrapper.get_net(args), ref_dis.Wrapper.get_net(args)
        with torch.no_grad():
            G.constant.constant.copy_(torch.randn_like(G.constant.constant))
            for k, v in G.state_dict().items():          # the projector's wide layers are not stored: both sides draw them from BIG_SEED
                if v.numel() > BIG:
                    v.copy_(seeded_like(k, v))
        g = torch.Generator().manual_seed(seed)
        data = {'enc_rgbs': torch.rand(2, 2, 3, 32, 32, generator=g), 'enc_stickmen': stick_images((2, 2, 3, 32, 32), g),
                'target_rgbs': torch.rand(2, 1, 3, 32, 32, generator=g), 'dec_stickmen': stick_images((2, 1, 3, 32, 32), g),
                'dec_keypoints': torch.rand(2, 1, args.pose_embedding_size, generator=g)}
        target = {'real_segm': torch.rand(2, 1, 1, 32, 32, generator=g).expand(2, 1, 3, 32, 32).contiguous(), 'label': torch.tensor([3, 1])}
        return E, G, D, data, target

    # the step's forward has ~10x the ReLU inputs of one module (encoder, generator, three critic passes): no seed clears MARGIN, so the seed with
    # the LARGEST tie margin of the search range is taken (twins with the same weights and buffers, no gradient)
    best = (-1.0, None)
    for seed in range(11, 211):
        E, G, D, data, target = build(seed)
        tE, tG, tD = ref_emb_fsth.Wrapper.get_net(args), ref_gen.Wrapper.get_net(args), ref_dis.Wrapper.get_net(args)
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
    print(f'train step FSTH: seed {seed}, ReLU tie margin {margin:.2e}')
    crits = [ref_adv.Criterion('gan'), ref_fm.Criterion(10.0), ref_l1.Criterion(30.0), ref_dice.Criterion(1.0)]
    tm = ref_runner.TrainingModule(E, G, D, crits, [], {})
    opt_G = ref_runner.get_optimizer(tm.embedder, tm.generator, args)
    opt_D = ref_dis.Wrapper.get_optimizer(tm.discriminator, args)
    tm.train()
    out = dict(margin=np.array(margin))
    for nm, mod in (('E', tm.embedder), ('G', tm.generator), ('D', tm.discriminator)):
        out.update({k: (v if v.size <= BIG else np.array(v.shape)) for k, v in sd_np(mod, f'init.{nm}.').items()})      # (> BIG: shape only, see seeded_like)
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
        for k, v in mod.state_dict().items():          # (> BIG elements: norm and a seeded projection instead of the values)
            out[f'after.{nm}.{k}'] = npy(v) if v.numel() <= BIG else summary(v)
    np.savez_compressed(os.path.join(OUT, 'fsth_train_step_small.npz'), **out)
    print('fsth_train_step_small.npz', len(out), 'arrays; losses', {k: float(v) for k, v in out.items() if k.startswith('loss.')})


if __name__ == '__main__':
    torch.set_num_threads(1)
    for w in (sys.argv[1:] or ['embedders', 'discriminator', 'train_step']):
        globals()['make_' + w]()
    for f in ('fsth_embedder_FSTH_small.npz', 'fsth_embedder_no_pose_encoder_small.npz', 'fsth_discriminator_small.npz', 'fsth_train_step_small.npz'):
        path = os.path.join(OUT, f)
        if os.path.exists(path):
            print(f, os.path.getsize(path), 'bytes')
