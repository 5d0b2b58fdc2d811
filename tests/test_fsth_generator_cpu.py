"""CPU checks of the stickman-to-image generator (generators/FSTH.py) against the fixtures the reference wrote (tests/golden/
make_golden_fsth_generator.py): the test-local restatement (tests/fsth_generator_restatement.py, the fp64 yardstick of the GPU tests) pinned to the
reference's outputs, gradients and spectral-norm buffers at 1e-5 rel-L2 -- the TOL of tests/test_fsth_cpu.py, for the same kind of comparison --;
the plugin's state-dict layout, parameter order, flags, refusals, fine-tuning structure and checkpoint path; the argument checks of the new entry
points."""
import argparse
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import fsth_restatement as R          # noqa: E402
import fsth_generator_restatement as GR          # noqa: E402
from test_fsth_cpu import fixture, plugin, sd_of, toy_args          # noqa: E402

TOL = 1e-5


def gen_args(**kw):
    base = dict(gen_num_downsample_blocks=3, gen_num_residual_blocks=2)
    base.update(kw)
    return toy_args(**base)


def null_gradient(k):
    """biases whose conv feeds only instance norms (every later layer reads the sum through an InstanceNorm / AdaIN, the 1x1 skips pass a
    per-channel constant on as a per-channel constant): their true gradient is exactly zero and the reference records fp32 rounding noise"""
    return k == 'down_block.4.bias' or k.endswith('skip.0.bias') or k.endswith('skip.1.bias')


def grad_figure(k, got, z, prefix):
    """rel-L2 of a parameter gradient against the fixture; a ``null_gradient`` bias is measured against the gradient norm of its own layer's weight
    instead of against the noise (the absolute error on the scale of that layer's gradients, held to the same bound)"""
    want = torch.from_numpy(z[prefix + k]).double()
    scale = torch.from_numpy(z[prefix + k[:-4] + 'weight_orig']).double().norm() if null_gradient(k) else want.norm()
    return ((got.detach().double().cpu() - want).norm() / scale.clamp_min(1e-30)).item()


def ada_keys(keys):
    """state-dict keys of the [1, C] AdaIN parameters (``...block.N.weight`` / ``decoder_blocks.N.weight``: no ``_orig``, inside the decoder)"""
    return [k for k in keys if k.startswith('decoder_blocks.') and k.rsplit('.', 1)[-1] in ('weight', 'bias') and (k.rsplit('.', 1)[0] + '.weight_orig') not in keys]


# ---- the restatement against the reference's numbers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_restated_generator_reproduces_the_reference(dtype):
    z = fixture('fsth_generator_small.npz')
    assert float(z['margin']) > 1e-4 and int(z['relu_sites']) == 16
    sd = GR.state_dict_from(z, 'sd.', dtype)
    assert GR.num_affine_params(sd) == int(z['num_affine_params']) == 272
    assert sum(t.numel() for t in sd.values() if t.requires_grad) == 23839
    embeds = torch.from_numpy(z['embeds']).to(dtype).requires_grad_(True)
    stick, r = torch.from_numpy(z['dec_stickmen']).to(dtype), torch.from_numpy(z['r']).to(dtype)
    taps = []
    out = GR.generator_forward(sd, embeds, stick, training=True, taps=taps)
    assert len(taps) == 16 and tuple(out.shape) == (2, 3, 32, 32)
    (out * r).sum().backward()
    errs = {'fake_rgbs': R.rel_l2(out, z['fake_rgbs']), 'grad_embeds': R.rel_l2(embeds.grad, z['grad_embeds'])}
    params = [k for k, t in sd.items() if t.requires_grad]
    assert sorted(params) == sorted(z['param_order'])
    for k in params:
        assert sd[k].grad is not None, f'{k} received no gradient'
        errs['grad.' + k] = grad_figure(k, sd[k].grad, z, 'grad.')
    for k, t in sd.items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['after.' + k] = R.rel_l2(t, z['sd_after.' + k])
    # eval mode from the buffers the train forward left (sd holds them now): no power iteration
    with torch.no_grad():
        before = {k: t.clone() for k, t in sd.items() if k.endswith('_u')}
        errs['eval_fake_rgbs'] = R.rel_l2(GR.generator_forward(sd, embeds.detach(), stick, training=False), z['eval_fake_rgbs'])
        assert all(torch.equal(sd[k], v) for k, v in before.items())
        # enable_finetuning: project(e_hat) in eval mode, sliced bias-then-weight per AdaIN in module order
        e_hat = torch.from_numpy(z['e_hat']).to(dtype)
        rows = F.linear(e_hat, R.sn_weight(sd, 'project.', False), sd['project.bias'])
        ft_keys = list(z['ft_sd_keys'])
        off = 0
        for k in ada_keys(ft_keys):
            if k.endswith('.weight'):
                c = z['ft_sd.' + k].shape[1]
                errs['ft_sd.' + k[:-6] + 'bias'] = R.rel_l2(rows[:, off:off + c], z['ft_sd.' + k[:-6] + 'bias'])
                errs['ft_sd.' + k] = R.rel_l2(rows[:, off + c:off + 2 * c], z['ft_sd.' + k])
                off += 2 * c
        assert off == 272
    # fine-tuning leg: the [1, C] parameters replace the projector
    sdf = GR.state_dict_from(z, 'ft_sd.', dtype)
    outf = GR.generator_forward(sdf, None, stick, training=True)
    (outf * r).sum().backward()
    errs['ft_fake_rgbs'] = R.rel_l2(outf, z['ft_fake_rgbs'])
    ft_grads = [k[len('ft_grad.'):] for k in z.files if k.startswith('ft_grad.')]
    assert set(ada_keys(list(sdf))) <= set(ft_grads) and len(ada_keys(list(sdf))) == 2 * 11 and not any(k.startswith('project.') for k in ft_grads)
    for k in ft_grads:
        errs['ft_grad.' + k] = grad_figure(k, sdf[k].grad, z, 'ft_grad.')
    for k, t in sdf.items():
        if k.endswith('_u') or k.endswith('_v'):
            errs['ft_after.' + k] = R.rel_l2(t, z['ft_sd_after.' + k])
    worst = max(errs, key=errs.get)
    print(f'[restatement] generator FSTH {dtype}: worst {worst} {errs[worst]:.2e} over {len(errs)} figures')
    assert errs[worst] < TOL, (worst, errs[worst])


def test_relu_replay_reproduces_the_plain_forward():
    """replaying the forward's own activation patterns changes nothing (the hook the tie-masked GPU comparisons rest on)"""
    z = fixture('fsth_generator_small.npz')
    stick, embeds = torch.from_numpy(z['dec_stickmen']).double(), torch.from_numpy(z['embeds']).double()
    taps = []
    a = GR.generator_forward(GR.state_dict_from(z, 'sd.', torch.float64, False), embeds, stick, taps=taps)
    R.RELU_REPLAY = [t > 0 for t in taps]
    try:
        b = GR.generator_forward(GR.state_dict_from(z, 'sd.', torch.float64, False), embeds, stick)
        assert R.RELU_REPLAY == []
    finally:
        R.RELU_REPLAY = None
    assert torch.equal(a, b)


# ---- the plugin: layout, order, flags, refusals ------------------------------------------------------------------------------------------------------
def test_state_dict_layout_parameter_order_and_finetuning_structure():
    z = fixture('fsth_generator_small.npz')
    want = sd_of(z, 'sd.')
    G = plugin('generators', 'FSTH').Wrapper.get_net(gen_args())
    sd = G.state_dict()
    assert list(sd) == list(z['sd_keys']) and all(sd[k].shape == want[k].shape for k in sd)
    assert [k for k, _ in G.named_parameters()] == list(z['param_order'])
    assert G.get_num_affine_params() == 272 and sum(p.numel() for p in G.parameters()) == 23839 and G.finetuning is False
    assert all(m.eps == 1e-4 for m in G.modules() if hasattr(m, 'weight_u'))
    for k in ('down_block.1.weight_orig', 'down_block.4.bias', 'skip.0.weight_orig', 'down_blocks.1.block.0.weight', 'down_blocks.0.block.7.weight_v',
              'down_blocks.0.skip.0.bias', 'decoder_blocks.1.block.7.weight_orig', 'decoder_blocks.2.block.4.weight_u', 'decoder_blocks.4.skip.1.bias',
              'decoder_blocks.8.bias', 'project.weight_orig'):
        assert k in sd, k
    assert sd['decoder_blocks.8.weight_orig'].shape == (3, 4, 3, 3) and sd['project.weight_orig'].shape == (272, 8)
    # the train forward's buffers, then the fine-tuning bootstrap of the reference's e_hat: same keys, order and values
    state = dict(want)
    state.update({k[len('sd_after.'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd_after.')})
    G.load_state_dict(state, strict=True)
    G.train()
    G.enable_finetuning({'embeds': torch.from_numpy(z['e_hat'])})
    assert G.finetuning is True and G.training
    ft = sd_of(z, 'ft_sd.')
    sdf = G.state_dict()
    assert list(sdf) == list(z['ft_sd_keys']) and [k for k, _ in G.named_parameters()] == list(z['ft_param_order'])
    for k in ft:
        assert sdf[k].shape == ft[k].shape and R.rel_l2(sdf[k], ft[k]) < 1e-6, k
    names = [k for k, _ in G.named_parameters()]
    assert names.index('decoder_blocks.0.block.0.weight') + 1 == names.index('decoder_blocks.0.block.0.bias')          # weight before bias
    assert sdf['decoder_blocks.5.weight'].shape == (1, 4) and sdf['decoder_blocks.3.block.5.bias'].shape == (1, 8)
    # a second call copies new values into the SAME parameters
    held = dict(G.named_parameters())
    G.enable_finetuning({'embeds': torch.from_numpy(z['e_hat']) * 2})
    again = dict(G.named_parameters())
    assert list(again) == names and all(again[k] is held[k] for k in names)
    assert not torch.equal(G.state_dict()['decoder_blocks.5.weight'], ft['decoder_blocks.5.weight'])
    G.load_state_dict(ft, strict=True)
    # ... and without a data_dict the new parameters are random (utils.load_model_from_checkpoint restructures a module that way)
    G2 = plugin('generators', 'FSTH').Wrapper.get_net(gen_args())
    G2.enable_finetuning()
    assert list(G2.state_dict()) == list(z['ft_sd_keys'])
    G2.load_state_dict(ft, strict=True)
    with pytest.raises(RuntimeError, match='HIP'):          # one backend: no CPU fallback
        G2({'dec_stickmen': torch.zeros(1, 1, 3, 32, 32)})


def test_full_geometry_counts():
    a = toy_args(image_size=256, num_channels=64, max_num_channels=512, embed_channels=512, gen_num_downsample_blocks=4, gen_num_residual_blocks=4)
    G = plugin('generators', 'FSTH').Wrapper.get_net(a)
    assert G.get_num_affine_params() == 13056 and sum(p.numel() for p in G.parameters()) == 37909443


def test_flags_and_refused_values():
    from utils.argparse_utils import MyArgumentParser
    W = plugin('generators', 'FSTH').Wrapper
    p = MyArgumentParser()
    W.get_args(p)
    a = p.parse_args([])
    assert (a.gen_padding, a.gen_num_downsample_blocks, a.gen_num_residual_blocks, a.norm_layer) == ('zero', 4, 4, 'in')
    with pytest.raises(NotImplementedError, match='--gen_padding'):
        W.get_net(gen_args(gen_padding='reflection'))
    with pytest.raises(Exception, match='padding'):
        W.get_net(gen_args(gen_padding='circular'))
    with pytest.raises(NotImplementedError, match='norm_layer'):
        W.get_net(gen_args(norm_layer='bn'))
    with pytest.raises(ValueError, match='gen_num_downsample_blocks'):
        W.get_net(gen_args(gen_num_downsample_blocks=1))
    with pytest.raises(NotImplementedError, match='out_channels'):
        W.get_net(gen_args(out_channels=4))
    G = W.get_net(gen_args())
    with pytest.raises(RuntimeError, match='HIP'):
        G({'embeds': torch.zeros(1, 8), 'dec_stickmen': torch.zeros(1, 1, 3, 32, 32)})


# ---- checkpoint path -------------------------------------------------------------------------------------------------------------------------------
def step_states(z, which='init'):
    return {nm: {k[len(f'{which}.{nm}.'):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f'{which}.{nm}.')} for nm in ('E', 'G', 'D')}


def test_reference_written_state_round_trips_through_load_model_from_checkpoint():
    from utils import utils
    st = step_states(fixture('fsth_generator_train_step_small.npz'))
    args = gen_args(embedder='FSTH', generator='FSTH', discriminator='FSTH', runner='holycow', inference=True, finetune=False)
    ck = {'embedder': st['E'], 'generator': st['G'], 'discriminator': st['D'], 'running_averages': {}, 'args': argparse.Namespace(**vars(args))}
    E, G, D, *_ = utils.load_model_from_checkpoint(ck, args)
    assert type(G).__module__.endswith('fsth_generator') and G.finetuning is False
    for name, mod in (('embedder', E), ('generator', G), ('discriminator', D)):
        sd = mod.state_dict()
        assert list(sd) == list(ck[name]), name
        assert all(torch.equal(sd[k], v) for k, v in ck[name].items()), name
    # ... into fine-tuning: the AdaIN parameters appear (random until the bootstrap), everything saved is kept
    args_ft = argparse.Namespace(**vars(args)); args_ft.finetune = True
    _, G2, D2, *_ = utils.load_model_from_checkpoint(ck, args_ft)
    sd2 = G2.state_dict()
    assert G2.finetuning and D2.embed.weight_orig.shape == (1, 8) and len(sd2) == len(st['G']) + 22
    assert all(torch.equal(sd2[k], v) for k, v in st['G'].items())
    # ... and a checkpoint written AFTER fine-tuning
    zg, zd, ze = fixture('fsth_generator_small.npz'), fixture('fsth_discriminator_small.npz'), fixture('fsth_embedder_FSTH_small.npz')
    saved = argparse.Namespace(**vars(args_ft))
    ck_ft = {'embedder': sd_of(ze, 'sum.sd.'), 'generator': sd_of(zg, 'ft_sd.'), 'discriminator': sd_of(zd, 'ft_sd.'), 'running_averages': {}, 'args': saved}
    _, G3, *_ = utils.load_model_from_checkpoint(ck_ft, args_ft)
    sd3 = G3.state_dict()
    assert G3.finetuning and list(sd3) == list(zg['ft_sd_keys']) and all(torch.equal(sd3[k], v) for k, v in ck_ft['generator'].items())


# ---- ABI: argument validation of the new entry points comes before any device work ---------------------------------------------------------------------
def test_new_entry_points_validate_before_device_work():
    import ctypes
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    for rc in (l.lp_tanh_head_fwd(None, None, ptr, 1, 2, 2, 4, None), l.lp_tanh_head_fwd(ptr, None, None, 1, 2, 2, 3, None),
               l.lp_tanh_head_bwd(None, ptr, ptr, 1, 2, 2, 4, None, None), l.lp_tanh_head_bwd(ptr, ptr, None, 1, 2, 2, 3, None, None),
               l.lp_norm_affine_grad(None, ptr, 8, ptr, ptr, 2, 8, 0, None), l.lp_norm_affine_grad(ptr, ptr, 8, ptr, None, 2, 8, 1, None)):
        assert rc == -1 and b'null' in l.lp_last_error()
    # an unsupported channel count is refused with host pointers only (nothing is dereferenced)
    for cz in (1, 2, 5, 8):
        assert l.lp_tanh_head_fwd(ptr, ptr, ptr, 1, 2, 2, cz, None) == -2 and b'Cz' in l.lp_last_error()
        assert l.lp_tanh_head_bwd(ptr, ptr, ptr, 1, 2, 2, cz, None, None) == -2 and b'Cz' in l.lp_last_error()
    assert l.lp_norm_affine_grad(ptr, ptr, 4, ptr, ptr, 2, 8, 0, None) == -1          # rows that overlap
    for name in ('lp_tanh_head_fwd', 'lp_tanh_head_bwd', 'lp_norm_affine_grad'):
        assert name in _lib.SIGNATURES
