"""Host code of the stickman-to-image generator (generators/FSTH.py of the reference): an encoder-decoder that turns a rendered stickman into an image.

  encoder   the FSTH family's stem (conv3x3 -> ReLU -> conv3x3 -> AvgPool2d + 1x1 skip, no ReLU in front) on ``dec_stickmen[:, 0]``, then
            ``gen_num_downsample_blocks - 1`` down ResBlocks with nn.InstanceNorm2d(eps 1e-4, affine=True): the norm makes a new tensor, so the 1x1
            skip reads the RAW block input (the norm-'none' blocks of the critic read relu(x)); gamma / beta are shared by the batch, the statistics
            are per sample in train and eval mode alike
  decoder   nn._DecoderFunction on the encoder output as a per-sample input: AdaIN residual blocks at the bottleneck width, one AdaIN up block per
            encoder stage, AdaIN -> ReLU -> conv3x3 (3 rows) -> tanh; ``fake_rgbs`` is the raw tanh (lp_tanh_head_*), there is no ``fake_segm``
  projector one spectrally normalised Linear (eps 1e-4) on ``embeds`` alone

The encoder is a composition of the autograd pieces the critic is made of (nn.hip_conv with epilogue statistics, nn.ConvPoolFn, nn.AvgPool2Fn) plus
``InNormReluFn`` below: relu(InstanceNorm(x)) straight to the conv's operand planes, backward lp_adain_relu_bwd + lp_norm_affine_grad (the per-sample
rows reduced to the batch-shared gamma / beta gradient in a fixed order).  The stickman is data: the stem's data gradient is never computed."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import hipops as ops
from . import nn as lpnn
from .fsth import refuse_reflection, stickmen
from .nn import (ADAIN_EPS, SN_EPS_CONV, AvgPool2Fn, ConvPoolFn, DecoderArgs, Generator, SNBatch, SNLinearFn, SNWeight, _DecoderFunction, _Indexed,
                 _accum_target, as_nchw_view, hip_conv, phantom, to_nhwc)
from ._lib import PREC_F16


class InNormReluFn(torch.autograd.Function):
    """operand planes of relu(InstanceNorm(x) * gamma + beta), gamma / beta [C] shared by the batch (blocks.py:58-60,72-73 with norm_layer 'in').
    Forward: the per-sample statistics (from the partials ``cs`` the producing conv's epilogue left, else lp_instnorm_stats) and ONE lp_act_pack
    with prologue 1 -- the planes go to ``holder``, the returned tensor is a phantom that carries the autograd edge to the consuming conv.
    Backward: lp_adain_relu_bwd on the conv's data gradient (per-sample dgamma / dbeta rows), then lp_norm_affine_grad sums the rows -- into the
    parameters' ``.grad`` inside ``nn.fused_grad_accumulation``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, cs, prec, holder):
        xd = x.detach().contiguous()
        n, _, _, c = xd.shape
        g2, b2 = gamma.detach().reshape(1, c).expand(n, c), beta.detach().reshape(1, c).expand(n, c)          # (row stride 0)
        st = ops.norm_stats_finalize(cs, n, c, g2, b2, ADAIN_EPS) if cs is not None else ops.instnorm_stats(xd, g2, b2, ADAIN_EPS)
        holder.append(ops.act_pack(xd, pro=1, scale=st[2], shift=st[3], prec=prec))
        ctx.x, ctx.st, ctx.gamma = xd, st, gamma.detach()
        ctx.affine = (gamma, beta)
        ctx.f16 = prec == PREC_F16
        return phantom(xd.shape, xd.device)

    @staticmethod
    def backward(ctx, dA):
        x, (mean, rstd, scale, shift) = ctx.x, ctx.st
        n, _, _, c = x.shape
        rows = torch.empty(2, n, c, dtype=torch.float32, device=x.device)          # the kernel's dgamma / dbeta share one row stride with gamma
        gfull = ctx.gamma.reshape(1, c).expand(n, c).contiguous()
        dx = ops.adain_relu_bwd(dA.contiguous(), x, None, gfull, mean, rstd, scale, shift, rows[0], rows[1], False, amax=ctx.f16)
        ag, ab = (_accum_target(p) for p in ctx.affine)
        if ag is None or ab is None:
            ag = ab = None
        dg, db = ops.norm_affine_grad(rows[0], rows[1], ag, ab)
        return dx, dg, db, None, None, None


class _AdaSlot(nn.Module):
    """place of an AdaptiveNorm2d in the decoder's module tree: no parameters until ``enable_finetuning`` makes ``weight`` / ``bias`` [1, C] ones"""

    def __init__(self, num_features):
        super().__init__()
        self.num_features = num_features
        self.weight = self.bias = None


class _AdaBlockParams(nn.Module):
    """blocks.ResBlock(norm_layer='adain') with its two AdaIN slots in their Sequential positions: block.{0, 3, 4, 7} | upsample: block.{0, 4, 5, 8}"""

    def __init__(self, cin, cout, upsample):
        super().__init__()
        self.i1, n1, self.i2 = ('4', '5', '8') if upsample else ('3', '4', '7')
        self.block = _Indexed(**{'_0': _AdaSlot(cin), '_' + self.i1: SNWeight((cout, cin, 3, 3), False, SN_EPS_CONV), '_' + n1: _AdaSlot(cout),
                                 '_' + self.i2: SNWeight((cout, cout, 3, 3), False, SN_EPS_CONV)})
        self.n1 = n1
        self.has_skip = cin != cout or upsample
        if self.has_skip:
            self.skip_key = '1' if upsample else '0'
            self.skip = _Indexed(**{'_' + self.skip_key: SNWeight((cout, cin, 1, 1), True, SN_EPS_CONV)})
        self.cin, self.cout, self.upsample = cin, cout, upsample

    def convs(self):
        return getattr(self.block, self.i1), getattr(self.block, self.i2), (getattr(self.skip, self.skip_key) if self.has_skip else None)

    def slots(self):
        return [self.block._modules['0'], self.block._modules[self.n1]]


class _InDownBlock(nn.Module):
    """parameters of blocks.ResBlock(norm_layer='in', downsample=True): block.0 / block.4 InstanceNorm2d(affine), block.3 / block.7 conv3x3 without
    bias, skip.0 conv1x1 with bias (the norm modules only hold gamma / beta: the arithmetic is InNormReluFn's)"""

    def __init__(self, cin, cout):
        super().__init__()
        self.block = _Indexed(_0=nn.InstanceNorm2d(cin, eps=ADAIN_EPS, affine=True), _3=SNWeight((cout, cin, 3, 3), False, SN_EPS_CONV),
                              _4=nn.InstanceNorm2d(cout, eps=ADAIN_EPS, affine=True), _7=SNWeight((cout, cout, 3, 3), False, SN_EPS_CONV))
        self.skip = _Indexed(_0=SNWeight((cout, cin, 1, 1), True, SN_EPS_CONV))
        self.cin, self.cout = cin, cout

    def sn_layers(self):
        return [self.block._modules['3'], self.block._modules['7'], self.skip._modules['0']]


# smallest bottleneck map: the decoder's input never was smaller than the 4 x 4 learned constant, and every encoder stage then pools a map of >= 8 x 8
# -- what the conv + pool launch needs for its skip conv on the POOLED input (the weight-gradient kernels cover W >= 4)
MIN_BOTTLENECK = 4


class GeneratorFSTH(Generator):
    """Drop-in for generators/FSTH.py::Generator of the reference: same constructor arguments, state-dict keys and order, ``named_parameters()``
    order, ``get_num_affine_params``, ``enable_finetuning`` and ``forward(data_dict)`` contract (reads ``embeds`` and ``dec_stickmen``, writes
    ``fake_rgbs`` only).  A batch without ``dec_stickmen`` has them rendered on the device from ``dec_keypoints`` at ``image_size`` (fsth.stickmen).
    Operand mode: ``nn.generator_prec()`` for encoder and decoder alike."""

    def __init__(self, padding, in_channels, out_channels, num_channels, max_num_channels, embed_channels, norm_layer, gen_num_downsample_blocks,
                 gen_num_residual_blocks, prec=None, image_size=None):
        nn.Module.__init__(self)
        self.image_size = image_size          # side of the stickman rendered for a batch that carries ``dec_keypoints`` only
        refuse_reflection(padding, '--gen_padding')
        if norm_layer != 'in':
            raise NotImplementedError(f"--norm_layer {norm_layer}: the FSTH generator on the HIP path implements norm_layer 'in' only")
        if gen_num_downsample_blocks < 2:
            raise ValueError('--gen_num_downsample_blocks must be >= 2 (the net has no down block to take its bottleneck width from otherwise)')
        if gen_num_residual_blocks < 0:
            raise ValueError('--gen_num_residual_blocks must be >= 0')
        if out_channels != 3:
            raise NotImplementedError(f'out_channels {out_channels}: the tanh head kernels write exactly the three RGB planes (out_channels == 3)')
        self.reflect = False
        nd = gen_num_downsample_blocks
        self.down_block = _Indexed(_1=SNWeight((num_channels, in_channels, 3, 3), True, SN_EPS_CONV),
                                   _4=SNWeight((num_channels, num_channels, 3, 3), True, SN_EPS_CONV))
        self.skip = _Indexed(_0=SNWeight((num_channels, in_channels, 1, 1), True, SN_EPS_CONV))
        downs, cin = {}, num_channels
        for i in range(nd - 1):
            cout = min(cin * 2, max_num_channels)
            downs[f'_{i}'] = _InDownBlock(cin, cout)
            cin = cout
        self.down_blocks = _Indexed(**downs)
        self.blocks_cfg = [(cin, cin, False)] * gen_num_residual_blocks
        for i in range(nd - 1, -1, -1):
            cout = min(int(num_channels * 2 ** i), max_num_channels)
            self.blocks_cfg.append((cin, cout, True))
            cin = cout
        nb = len(self.blocks_cfg)
        dec = {f'_{i}': _AdaBlockParams(*cfg) for i, cfg in enumerate(self.blocks_cfg)}
        dec[f'_{nb}'] = _AdaSlot(cin)          # nb + 1: ReLU, nb + 2: padding, nb + 3: the head conv, nb + 4: Tanh
        dec[f'_{nb + 3}'] = SNWeight((out_channels, cin, 3, 3), True, SN_EPS_CONV)
        self.decoder_blocks = _Indexed(**dec)
        self.num_affine_params = lpnn.decoder_layout(self.blocks_cfg, MIN_BOTTLENECK, False).n_affine          # (the same for every input size)
        self.project = SNWeight((self.num_affine_params, embed_channels), True, SN_EPS_CONV)
        self.embed_channels = embed_channels
        self.num_downsample = nd
        self.finetuning = False
        self.prec = lpnn.generator_prec() if prec is None else prec
        self.infer_prec = self.prec if (prec is not None or os.environ.get('LP_PREC_G') or lpnn.default_prec() != PREC_F16) else PREC_F16
        self.f16_tail = 0

    # ---- module tree --------------------------------------------------------------------------------------------------------------------------
    def _stem(self):
        return self.down_block._modules['1'], self.down_block._modules['4'], self.skip._modules['0']

    def _head(self):
        return self.decoder_blocks._modules[str(len(self.blocks_cfg) + 3)]

    def _decoder_in_size(self):
        """side of the bottleneck map, known from the first forward on"""
        return self.__dict__['_bott_size']

    def _ada_slots(self):
        """the AdaIN layers in module order -- the order the projector's output is consumed in (per layer: C biases, then C weights)"""
        nb = len(self.blocks_cfg)
        return [s for i in range(nb) for s in self.decoder_blocks._modules[str(i)].slots()] + [self.decoder_blocks._modules[str(nb)]]

    def _encoder_sn_layers(self):
        return list(self._stem()) + [l for blk in self.down_blocks._modules.values() for l in blk.sn_layers()]

    def _sn_layers(self):
        """ONE batched power iteration: decoder convs (block order), head conv, encoder convs, and -- unless the AdaIN parameters are trainable, when
        ``forward`` does not run it -- the projector"""
        cached = self.__dict__.get('_sn_layer_cache')
        if cached is None or cached[1] != self.finetuning:
            cached = (self._decoder_sn_layers() + self._encoder_sn_layers() + ([] if self.finetuning else [self.project]), self.finetuning)
            self.__dict__['_sn_layer_cache'] = cached
        return cached

    # ---- the 3-row head conv is launched zero-padded to the 4 rows the head kernels take ------------------------------------------------------------
    def _head_pad(self):
        head = self._head()
        w, b = head.weight_orig, head.bias
        pad = self.__dict__.get('_head_pad_buf')
        if pad is None or pad[0].device != w.device or pad[0].shape[1:] != w.shape[1:]:
            pad = (torch.zeros((4,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device), torch.zeros(4, dtype=torch.float32, device=w.device))
            self.__dict__['_head_pad_buf'] = pad
        with torch.no_grad():
            pad[0][:3].copy_(w)
            pad[1][:3].copy_(b)
        return pad

    def _pack_sources(self, weights, head_pad):
        return weights[:-2] + [head_pad[0], head_pad[1]]

    def prepare_step(self):
        """as ``Generator.prepare_step``; the weight packs need the bottleneck size (which up blocks run in their phase forms), known from the first
        forward on"""
        if not (self.training and torch.is_grad_enabled() and next(self.parameters()).is_cuda):
            return
        states = self._sn_update()
        self.__dict__['_prepared_sn'] = states
        if self.__dict__.get('_bott_size') is not None:
            weights, _ = self._conv_weights(states)
            if any(w.requires_grad for w in weights):
                pad = self._head_pad()
                self.__dict__['_prepared_packs'] = (pad, self._train_packs_update(self._pack_sources(weights, pad)))

    # ---- projector / fine-tuning ----------------------------------------------------------------------------------------------------------------
    def enable_finetuning(self, data_dict=None):
        """generators/FSTH.py:152-181 of the reference: the projector runs ONCE on ``embeds`` (1 x E; random without a ``data_dict``) in eval mode (no
        power iteration) under no_grad, and every AdaIN's weight and bias become ``nn.Parameter``s of shape [1, C] (``weight`` registered first);
        ``forward`` then skips the projector.  A second call copies new values into the existing parameters."""
        ref = next(iter(self.parameters()))
        embeds = torch.rand(1, self.embed_channels).to(ref) if data_dict is None else data_dict['embeds'].to(ref)
        if embeds.shape != (1, self.embed_channels):
            raise ValueError(f'enable_finetuning takes one identity: embeds 1 x {self.embed_channels}, got {tuple(embeds.shape)}')
        p = self.project
        with torch.no_grad():
            if ref.is_cuda:
                sb = self.__dict__.get('_project_sn')
                if sb is None or sb.layers[0] is not p:
                    sb = self.__dict__['_project_sn'] = SNBatch([p])
                affine = SNLinearFn.apply(embeds.contiguous(), p.weight_orig, p.bias, *sb.update(False)[0])
            else:
                # (a module still on the CPU -- utils.load_model_from_checkpoint builds and restructures its modules there before their state is
                #  loaded: one 1 x E row, outside autograd, in plain torch)
                w = p.weight_orig
                affine = F.linear(embeds, w / torch.dot(p.weight_u, torch.mv(w, p.weight_v)), p.bias)
            off = 0
            for slot in self._ada_slots():
                c = slot.num_features
                bias, weight = affine[:, off:off + c], affine[:, off + c:off + 2 * c]
                off += 2 * c
                if self.finetuning:
                    slot.weight.copy_(weight)
                    slot.bias.copy_(bias)
                else:
                    slot.weight = nn.Parameter(weight.clone())
                    slot.bias = nn.Parameter(bias.clone())
        self.finetuning = True

    def _affine(self, data_dict, batch, states):
        if self.finetuning:
            row = torch.cat([t for slot in self._ada_slots() for t in (slot.bias, slot.weight)], dim=1)
            return row.expand(batch, -1)
        embeds = data_dict['embeds']
        if not embeds.is_cuda:
            raise RuntimeError('the generator runs on the MI355X HIP path only (no CPU fallback); move the model and inputs to cuda')
        p = self.project
        return SNLinearFn.apply(embeds, p.weight_orig, p.bias, *states[-1])

    # ---- encoder ------------------------------------------------------------------------------------------------------------------------------
    def _encoder_packs(self, training_pass):
        """per-forward dict cache of the encoder convs' 16-bit packs (``nn.cached_pack``); inference: kept while the weights do not change"""
        if training_pass:
            return {}
        from .optim import WEIGHTS_GENERATION
        key = (WEIGHTS_GENERATION[0],) + tuple((l.weight_orig.data_ptr(), l.weight_orig._version) for l in self._encoder_sn_layers())
        cache = self.__dict__.get('_enc_pack_cache')
        if cache is None or cache[0] != key:
            cache = self.__dict__['_enc_pack_cache'] = (key, {})
        return cache[1]

    def _encode(self, stick, sn_of, prec, packs, debug):
        """stem + InstanceNorm down blocks on the logical N x C x S x S stickman -> NHWC [N, s, s, C_bottleneck]"""
        def tape(a16):
            if debug is not None:
                debug.setdefault('relu_planes', []).append(a16.hi)

        def cv(x, layer, **kw):
            return hip_conv(x, layer.weight_orig, layer.bias, prec=prec, packs=packs.setdefault(prec, {}), sn=sn_of[id(layer)], **kw)

        def conv2_pool(h, h16, c2, sk, x_pooled):
            """AvgPool2d(conv3x3(relu-planes h16) + conv1x1(x)) as ONE 4x4 stride-2 launch; the 1x1 skip conv commutes with the pool and runs on the
            pooled input (nn.ConvPoolFn)"""
            s_lo = cv(x_pooled, sk, ksize=1)
            return ConvPoolFn.apply(h, c2.weight_orig, c2.bias, s_lo, prec, packs.setdefault(prec, {}), sn_of[id(c2)], h16, False, None)
        stick = stick.detach()
        d0, d2, sk = self._stem()
        xn = to_nhwc(stick)
        h, h16 = cv(xn, d0, ksize=3, emit16=1, want_y=False)
        tape(h16)
        x = conv2_pool(h, h16, d2, sk, to_nhwc(F.avg_pool2d(stick, 2)))
        for blk in self.down_blocks._modules.values():
            n0, c1, n1, c2 = (blk.block._modules[k] for k in ('0', '3', '4', '7'))
            assert not ops.thin_wgrad_supported(blk.cin, blk.cout, 3, 0, x.shape[2]), 'the normalised block input exists as operand planes only'
            hold = []
            p0 = InNormReluFn.apply(x, n0.weight, n0.bias, None, prec, hold)
            tape(hold[0])
            stats = []
            h1 = cv(p0, c1, ksize=3, x16=hold[0], stats=stats)
            a1 = []
            p1 = InNormReluFn.apply(h1, n1.weight, n1.bias, stats[0] if stats else None, prec, a1)
            tape(a1[0])
            x = conv2_pool(p1, a1[0], c2, blk.skip._modules['0'], AvgPool2Fn.apply(x, False))
        return x

    # ---- forward ------------------------------------------------------------------------------------------------------------------------------
    def forward(self, data_dict):
        if data_dict.get('dec_stickmen') is None and data_dict.get('dec_keypoints') is not None and self.image_size is None:
            raise RuntimeError('a batch with dec_keypoints only needs the frame size to render at: construct the generator with image_size '
                               '(generators/FSTH.py passes --image_size)')
        stick = stickmen(data_dict, 'dec', self.image_size)
        if stick.dim() > 4:
            stick = stick[:, 0]
        if not (stick.is_cuda and next(self.parameters()).is_cuda):
            raise RuntimeError('the generator runs on the MI355X HIP path only (no CPU fallback); move the model and inputs to cuda')
        size = stick.shape[-1]
        if stick.shape[-2] != size or size % (1 << self.num_downsample) or size >> self.num_downsample < MIN_BOTTLENECK:
            raise ValueError(f'dec_stickmen {tuple(stick.shape)}: square frames with a side that is a multiple of 2^{self.num_downsample} and at least '
                             f'{MIN_BOTTLENECK << self.num_downsample} (a bottleneck map of {MIN_BOTTLENECK} x {MIN_BOTTLENECK}) are required')
        self.__dict__['_bott_size'] = size >> self.num_downsample
        states = self.__dict__.pop('_prepared_sn', None)          # prepare_step() ran ahead: use its result
        if states is None or not (self.training and torch.is_grad_enabled()):
            states = self._sn_update()
        affine = self._affine(data_dict, stick.shape[0], states)
        weights, sn = self._conv_weights(states)
        enc_layers = self._encoder_sn_layers()
        nd = len(self._layout().conv_idx)
        sn_of = {id(l): s for l, s in zip(enc_layers, states[nd:nd + len(enc_layers)])}
        need_grad = torch.is_grad_enabled() and (affine.requires_grad or any(p.requires_grad for p in self.parameters()))
        prec = self.prec if need_grad else self.infer_prec
        precs = self.block_precs(prec)
        prepared = self.__dict__.pop('_prepared_packs', None)
        if not torch.is_grad_enabled():
            prepared = None
        pad = prepared[0] if prepared is not None else self._head_pad()
        packs, packsT = self._decoder_packs(weights, self._pack_sources(weights, pad), prec, precs, need_grad, None if prepared is None else prepared[1])
        debug = getattr(self, '_debug', None)
        x = self._encode(stick, sn_of, prec, self._encoder_packs(need_grad and self.training), debug)
        # identity-skip blocks add their fp32 input: residual blocks on maps the 16-bit-resident outputs would cover switch those outputs off
        res_blocks = any(not up for _, _, up in self.blocks_cfg)
        y16 = lpnn.G_Y16 and self.training and need_grad and not (res_blocks and self._bott_size >= lpnn.Y16_MIN_MAP)
        cfg = DecoderArgs(layout=self._layout(), prec=prec, precs=precs, need_grad=need_grad, sn=sn, packs=packs, packsT=packsT, debug=debug, y16=y16,
                          head_pad=pad)
        rgbs, _ = _DecoderFunction.apply(cfg, affine, as_nchw_view(x), *weights)
        data_dict['fake_rgbs'] = rgbs
