"""Test-local torch restatement of the stickman-to-image generator (generators/FSTH.py), written from its description, in plain torch ops on a state
dict of any dtype (fp32: what the reference computes; fp64: the yardstick of the GPU tests).  tests/test_fsth_generator_cpu.py pins it to the
reference-made fixture first (outputs, every gradient and the spectral-norm buffers to 1e-5 rel-L2).

Architecture (every conv and the projector spectrally normalised with eps 1e-4, legacy hook -- ``fsth_restatement.sn_weight``):
  stem      ``fsth_restatement.stem`` on dec_stickmen[:, 0]: ZeroPad(1) conv3x3 (down_block.1) -> ReLU -> ZeroPad(1) conv3x3 (down_block.4) -> AvgPool2,
            plus conv1x1 (skip.0) -> AvgPool2; no ReLU in front
  encoder   down_blocks.{i}: InstanceNorm(eps 1e-4, affine: block.0) -> ReLU -> conv3x3 without bias (block.3) -> InstanceNorm (block.4) -> ReLU ->
            conv3x3 without bias (block.7) -> AvgPool2, plus conv1x1 with bias (skip.0) -> AvgPool2 on the RAW block input (the norm makes a new
            tensor: the in-place ReLU does not reach it); channels double up to the widest conv of the state dict
  decoder   AdaIN residual blocks (block.3 / block.7, identity skip) while ``block.3`` exists, then up blocks: AdaIN -> ReLU -> nearest x2 ->
            conv3x3 (block.4) -> AdaIN -> ReLU -> conv3x3 (block.8), plus nearest x2 -> conv1x1 with bias (skip.1); then AdaIN -> ReLU ->
            ZeroPad(1) conv3x3 with bias (decoder_blocks.{nb + 3}) -> tanh = fake_rgbs
  AdaIN     InstanceNorm(eps 1e-4) * weight[:, :, None, None] + bias[:, :, None, None]; weight / bias are slices of project(embeds), consumed in
            module order, per layer C biases then C weights -- or, after enable_finetuning, the [1, C] entries ``...{weight,bias}`` of the state dict

ReLU sites go through ``fsth_restatement.relu``: set ``fsth_restatement.RELU_REPLAY`` to replay recorded activation patterns (tie-masked tests)."""
import torch
import torch.nn.functional as F

import fsth_restatement as R

EPS = 1e-4


def _conv(sd, prefix, x, training, pad):
    return F.conv2d(x, R.sn_weight(sd, prefix, training), sd.get(prefix + 'bias'), 1, pad)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode='nearest')


class _Affine:
    """hands out (weight, bias) [B | 1, C] per AdaIN in module order"""

    def __init__(self, sd, embeds, training):
        self.sd = sd
        self.finetuned = 'decoder_blocks.0.block.0.weight' in sd
        self.rows, self.off = None, 0
        if not self.finetuned:
            self.rows = F.linear(embeds, R.sn_weight(sd, 'project.', training), sd['project.bias'])

    def take(self, prefix, c):
        if self.finetuned:
            return self.sd[prefix + 'weight'], self.sd[prefix + 'bias']
        bias, weight = self.rows[:, self.off:self.off + c], self.rows[:, self.off + c:self.off + 2 * c]
        self.off += 2 * c
        return weight, bias


def _adain_relu(x, affine, prefix, taps):
    w, b = affine.take(prefix, x.shape[1])
    y = F.instance_norm(x, eps=EPS) * w[:, :, None, None] + b[:, :, None, None]
    taps.append(y)
    return R.relu(y)


def _in_relu(sd, prefix, x, taps):
    y = F.instance_norm(x, weight=sd[prefix + 'weight'], bias=sd[prefix + 'bias'], eps=EPS)
    taps.append(y)
    return R.relu(y)


def num_affine_params(sd):
    """2 C per AdaIN layer, from the conv shapes of a state dict"""
    n, i = 0, 0
    while True:
        for k1, k2 in (('3', '7'), ('4', '8')):
            w = sd.get(f'decoder_blocks.{i}.block.{k1}.weight_orig')
            if w is not None:
                n += 2 * (w.shape[1] + w.shape[0])
                break
        else:
            return n + 2 * sd[f'decoder_blocks.{i + 3}.weight_orig'].shape[1]
        i += 1


def generator_forward(sd, embeds, dec_stickmen, training=True, taps=None):
    """-> fake_rgbs [B, 3, S, S].  ``embeds`` is ignored for a fine-tuned state dict.  ``taps``: receives the pre-activation tensor of every ReLU site
    in execution order (NCHW).  training: the (u, v) entries of ``sd`` take one power-iteration step in place (the projector's only when it runs)."""
    taps = [] if taps is None else taps
    x = dec_stickmen[:, 0] if dec_stickmen.dim() > 4 else dec_stickmen
    affine = _Affine(sd, embeds, training)
    out = R.stem(sd, x, training, taps)
    i = 0
    while f'down_blocks.{i}.block.3.weight_orig' in sd:
        p = f'down_blocks.{i}.'
        h = _conv(sd, p + 'block.3.', _in_relu(sd, p + 'block.0.', out, taps), training, 1)
        h = _conv(sd, p + 'block.7.', _in_relu(sd, p + 'block.4.', h, taps), training, 1)
        out = F.avg_pool2d(h, 2) + F.avg_pool2d(_conv(sd, p + 'skip.0.', out, training, 0), 2)
        i += 1
    i = 0
    while True:
        p = f'decoder_blocks.{i}.'
        if p + 'block.3.weight_orig' in sd:          # residual block
            h = _conv(sd, p + 'block.3.', _adain_relu(out, affine, p + 'block.0.', taps), training, 1)
            h = _conv(sd, p + 'block.7.', _adain_relu(h, affine, p + 'block.4.', taps), training, 1)
            out = h + out
        elif p + 'block.4.weight_orig' in sd:          # up block
            h = _conv(sd, p + 'block.4.', _up(_adain_relu(out, affine, p + 'block.0.', taps)), training, 1)
            h = _conv(sd, p + 'block.8.', _adain_relu(h, affine, p + 'block.5.', taps), training, 1)
            out = h + _conv(sd, p + 'skip.1.', _up(out), training, 0)
        else:
            break
        i += 1
    h = _adain_relu(out, affine, f'decoder_blocks.{i}.', taps)
    return torch.tanh(_conv(sd, f'decoder_blocks.{i + 3}.', h, training, 1))


def state_dict_from(z, prefix, dtype=torch.float32, requires_grad=True):
    """the arrays ``prefix*`` of an .npz fixture as a state dict of ``dtype``; every parameter (``weight_orig``, ``bias``, the norms' / fine-tuned
    AdaINs' ``weight``) is a leaf that requires grad"""
    sd = {}
    for k in z.files:
        if k.startswith(prefix):
            t = torch.from_numpy(z[k]).to(dtype)
            name = k[len(prefix):]
            if requires_grad and name.rsplit('.', 1)[-1] in ('weight_orig', 'bias', 'weight'):
                t.requires_grad_(True)
            sd[name] = t
    return sd
