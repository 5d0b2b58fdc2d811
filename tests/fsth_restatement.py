"""Test-local torch restatement of the FSTH plugin family's nets -- the conv embedders (embedders/FSTH.py, embedders/no_pose_encoder.py) and the
stickman-conditioned projection critic (discriminators/FSTH.py) -- written from their description, in plain torch ops on a state dict of any dtype
(fp32: what the reference computes; fp64: the yardstick of the full-size GPU tests).  tests/test_fsth_cpu.py pins it to the reference-made fixtures
first (forward values and gradients to 1e-5 rel-L2).

Architecture (every conv spectrally normalised with eps 1e-4, legacy hook: one in-place power iteration per training forward, sigma = u . W v with
u, v constants for autograd):
  stem        main: ZeroPad(1) conv3x3 -> ReLU -> ZeroPad(1) conv3x3 -> AvgPool2   (state-dict keys down_block.1 / down_block.4)
              skip: conv1x1 -> AvgPool2                                             (skip.0);   out = main + skip
  ResBlock    norm 'none': x = relu_(x) IN PLACE (so the skip branch / identity add and any stored reference to x see relu(x));
              main: conv3x3(x) -> ReLU -> conv3x3 [-> AvgPool2]   (block.2 / block.5);  skip: conv1x1(x) [-> AvgPool2] (skip.0) | x
  embedder    stem on cat([stickmen, rgbs], channel dim of the 5-D tensors) = (s0 s1 s2 r0 r1 r2) | rgbs alone; down blocks; ReLU; sum over H x W ->
              embeds_elemwise [B, K, E]; embeds = mean | max over K
  critic      stem on cat([stickmen, image], dim=2 of the 4-D tensors).view(b, -1, h, w) = INTERLEAVED (s0 r0 s1 r1 s2 r2); blocks (the first
              min(log2(size) - 2, n) - 1 pool, the rest do not); features = every block input after its in-place ReLU + the last output; ReLU; sum over
              H x W; score = linear(pooled) [+ <pooled, embed(label)>]; three passes per forward (fake, fake.detach + embed.detach, real), each with
              its own power iteration; the label embedding is power-iterated once per forward (eps 1e-4; 1e-12 after enable_finetuning)."""
import math

import torch
import torch.nn.functional as F


# Tie-masked comparisons (tests/test_fsth_full_gpu.py): when a list, every ReLU site consumes the next recorded activation pattern (bool, NCHW) instead
# of taking its own sign -- the gradients are then compared on the piecewise-linear branch the code under test actually took.  None: true ReLUs.
RELU_REPLAY = None


def relu(x):
    if RELU_REPLAY is None:
        return torch.relu(x)
    return x * RELU_REPLAY.pop(0).to(x.dtype)


def _normalize(x, eps):
    return x / x.norm().clamp_min(eps)


def sn_weight(sd, prefix, training, eps=1e-4):
    """effective weight W_orig / sigma of the layer ``prefix``; training: the (u, v) entries of ``sd`` take one power-iteration step in place"""
    w = sd[prefix + 'weight_orig']
    wm = w.reshape(w.shape[0], -1)
    u, v = sd[prefix + 'weight_u'], sd[prefix + 'weight_v']
    if training:
        with torch.no_grad():
            v = _normalize(wm.t().mv(u), eps)
            u = _normalize(wm.mv(v), eps)
            sd[prefix + 'weight_u'], sd[prefix + 'weight_v'] = u, v
    sigma = torch.dot(u.detach(), wm.mv(v.detach()))
    return w / sigma


def _conv(sd, prefix, x, training, pad):
    return F.conv2d(x, sn_weight(sd, prefix, training), sd[prefix + 'bias'], 1, pad)


def stem(sd, x, training, taps):
    h = _conv(sd, 'down_block.1.', x, training, 1)
    taps.append(h)
    h = _conv(sd, 'down_block.4.', relu(h), training, 1)
    return F.avg_pool2d(h, 2) + F.avg_pool2d(_conv(sd, 'skip.0.', x, training, 0), 2)


def res_block(sd, prefix, x, downsample, training, taps):
    """``x``: the block input AFTER its in-place ReLU"""
    h = _conv(sd, prefix + 'block.2.', x, training, 1)
    taps.append(h)
    h = _conv(sd, prefix + 'block.5.', relu(h), training, 1)
    s = _conv(sd, prefix + 'skip.0.', x, training, 0) if (prefix + 'skip.0.weight_orig') in sd else x
    if downsample:
        h, s = F.avg_pool2d(h, 2), F.avg_pool2d(s, 2)
    return h + s


def embedder_forward(sd, enc_rgbs, enc_stickmen, average_function, training=True, taps=None):
    """-> (embeds [B, E], embeds_elemwise [B, K, E]); ``enc_stickmen`` None: embedders/no_pose_encoder.py.  ``taps``: receives the pre-activation
    tensor of every ReLU site in execution order (NCHW)"""
    taps = [] if taps is None else taps
    x = enc_rgbs if enc_stickmen is None else torch.cat([enc_stickmen, enc_rgbs], 2)
    b, k, c, h, w = x.shape
    out = stem(sd, x.reshape(-1, c, h, w), training, taps)
    nblocks = 1 + max(int(key.split('.')[1]) for key in sd if key.startswith('down_blocks.'))
    for i in range(nblocks):
        taps.append(out)
        out = res_block(sd, f'down_blocks.{i}.', relu(out), True, training, taps)
    taps.append(out)
    elem = relu(out).reshape(b, k, out.shape[1], -1).sum(3)
    if average_function == 'sum':
        embeds = elem.mean(1)
    elif average_function == 'max':
        embeds = elem.max(1)[0]
    else:
        raise ValueError(average_function)
    return embeds, elem


def critic_input(stickmen, image):
    b, _, h, w = stickmen.shape
    return torch.cat([stickmen, image], dim=2).view(b, -1, h, w)


def critic_pass(sd, x, embed, image_size, training, taps):
    nblocks = 1 + max(int(key.split('.')[1]) for key in sd if key.startswith('blocks.'))
    dis_num_blocks = nblocks + 1
    num_down = min(int(math.log(image_size, 2)) - 2, dis_num_blocks)
    out = stem(sd, x, training, taps)
    feats = []
    for i in range(nblocks):
        taps.append(out)
        out = relu(out)
        feats.append(out)
        out = res_block(sd, f'blocks.{i}.', out, i + 1 < num_down, training, taps)
    feats.append(out)
    taps.append(out)
    pooled = relu(out).reshape(out.shape[0], out.shape[1], -1).sum(2)
    score = F.linear(pooled, sn_weight(sd, 'linear.', training), sd['linear.bias'])[:, 0]
    if embed is not None:
        score = (pooled * embed).sum(1) + score
    return score, feats


def critic_forward(sd, fake, real, stickmen, label, image_size, training=True, finetuning=False, taps=None):
    """-> dict with the reference's outputs (fake_score_G, fake_score_D, real_score, real_embedding, fake_features, real_features)"""
    taps = [] if taps is None else taps
    embed = F.embedding(label, sn_weight(sd, 'embed.', training, 1e-12 if finetuning else 1e-4))
    fake_in = critic_input(stickmen, fake)
    fake_score_G, fake_features = critic_pass(sd, fake_in, embed, image_size, training, taps)
    fake_score_D, _ = critic_pass(sd, fake_in.detach(), embed.detach(), image_size, training, taps)
    real_score, real_features = critic_pass(sd, critic_input(stickmen, real), embed, image_size, training, taps)
    return dict(fake_score_G=fake_score_G, fake_score_D=fake_score_D, real_score=real_score, real_embedding=embed, fake_features=fake_features,
                real_features=real_features)


def critic_losses(out, fm_weight=10.0):
    """(adversarial_G, feature_matching, adversarial_D) of criterions/adversarial.py ('gan': hinge) and criterions/featmat.py"""
    adv_g = -out['fake_score_G'].mean()
    adv_d = torch.relu(1. - out['real_score']).mean() + torch.relu(1. + out['fake_score_D']).mean()
    fm = sum(F.l1_loss(a, b.detach()) for a, b in zip(out['fake_features'], out['real_features'])) / len(out['fake_features']) * fm_weight
    return adv_g, fm, adv_d


def state_dict_from(z, prefix, dtype=torch.float32, requires_grad=True):
    """the arrays ``prefix*`` of an .npz fixture as a state dict of ``dtype`` (parameters as leaves that require grad)"""
    sd = {}
    for k in z.files:
        if k.startswith(prefix):
            t = torch.from_numpy(z[k]).to(dtype)
            name = k[len(prefix):]
            if requires_grad and (name.endswith('weight_orig') or name.endswith('bias')):
                t.requires_grad_(True)
            sd[name] = t
    return sd


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
