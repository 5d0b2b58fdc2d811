"""What an assignment of operand modes to the identity encoder's contractions itself costs, with no kernel involved: the orchestration of
embedders/resnext_hip.py run through the mode-aware emulation (tests/emu_modes.py, ``rounding()`` on) in fp64, against the stock layers in
exact fp64 (oracle/backbones_ref.py), on the net and the frames of tests/test_resnext_hip.py.  Every contraction rounds its operands
according to the ``prec`` that call receives, 16-bit-resident conv outputs are rounded to fp16, the planes residual to its planes, fp32
results to fp32 (see emu_modes).  The gates of test_resnext_hip.py::test_resnext_operand_mode_assignments_vs_fp64 are 3x these
predictions; scripts/embedder_rounding_study.py prints them.  TEST INFRASTRUCTURE ONLY.

``CASES``: name -> (environment, module switches of resnext_hip).  ``select`` applies one through a pytest ``MonkeyPatch`` -- the GPU test and
the study choose an assignment through the same table."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MODE_ENV = ('LP_PREC', 'LP_PREC_E', 'LP_E_HEAD_F16', 'LP_E_F16_TAIL')


def _default(tail, head=None, **switches):
    """the default assignment (bf16x3 head, fp16 tail of ``tail`` bottlenecks), optionally with layer kinds of the head moved to fp16"""
    env = {'LP_E_F16_TAIL': str(tail)}
    if head:
        env['LP_E_HEAD_F16'] = head
    return env, switches


CASES = {
    'bf16x3': ({'LP_PREC_E': 'bf16x3'}, {}),
    'f16': ({'LP_PREC_E': 'f16'}, {}),
    'f16-Y16=0': ({'LP_PREC_E': 'f16'}, {'Y16': False}),
    'bf16': ({'LP_PREC_E': 'bf16'}, {}),
    'bf16-RES16=0': ({'LP_PREC_E': 'bf16'}, {'RES16': False}),
    'bf16x3-RES16=0': ({'LP_PREC_E': 'bf16x3'}, {'RES16': False}),
    'bf16x3-RES16=0-MASK16=0': ({'LP_PREC_E': 'bf16x3'}, {'RES16': False, 'MASK16': False}),
    **{f'tail{t}': _default(t) for t in (0, 1, 2, 3, 4, 6)},
    'tail2-head-conv2': _default(2, 'conv2'),
    'tail2-head-conv1,conv3': _default(2, 'conv1,conv3'),
    'tail2-head-conv1,conv2,conv3': _default(2, 'conv1,conv2,conv3'),
    **{f'tail{t}-{sw}=0': _default(t, **{sw: False}) for t in (2, 3) for sw in ('RES16', 'MASK16', 'Y16')},
    'tail2-RES16=0-MASK16=0': _default(2, RES16=False, MASK16=False),
}


def select(mp, case):
    """apply CASES[case]: the four mode variables are removed from the environment first (unset = the default assignment)"""
    from embedders import resnext_hip
    env, switches = CASES[case]
    for k in MODE_ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    for k in ('Y16', 'RES16', 'MASK16'):          # (module constants read from LP_E_* at import)
        mp.setattr(resnext_hip, k, switches.get(k, True))


def install(mp, layer):
    """route the HIP path of the identity encoder through an emulation layer (emu_ops | emu_modes)"""
    from embedders import resnext_hip
    from latent_pose_reenactment_amd import hipops
    mp.setattr(resnext_hip, 'ops', layer)
    mp.setattr(hipops, 'PackBatch', layer.PackBatch)
    mp.setattr(hipops, 'pack_grouped', layer.pack_grouped)


def make_net(num_classes, seed, layers):
    """the net of test_resnext_hip._nets, on the CPU in fp32 (same seed -> same parameters and buffers)"""
    from embedders.backbones import ResNeXt
    torch.manual_seed(seed)
    m = ResNeXt(list(layers), 32, 4, num_classes)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5); mod.bias.data.uniform_(-0.3, 0.3)
            mod.running_mean.uniform_(-0.2, 0.2); mod.running_var.uniform_(0.5, 1.5)
    return m


def loss_weights(n, num_classes, seed=11):
    return torch.randn(n, num_classes, generator=torch.Generator().manual_seed(seed))


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def errors(m, ref, y, yr):
    """(logits, all gradients, worst floating-point buffer) of net ``m`` against ``ref``, rel-L2; + the six worst parameter gradients"""
    num = sum((p.grad.double().cpu() - q.grad.double().cpu()).norm() ** 2 for p, q in zip(m.parameters(), ref.parameters()))
    den = sum(q.grad.double().cpu().norm() ** 2 for q in ref.parameters())
    berr = [rel(b, q) for (_, b), (_, q) in zip(m.named_buffers(), ref.named_buffers()) if b.dtype.is_floating_point]
    worst = sorted(((rel(p.grad, q.grad), k) for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters())), reverse=True)[:6]
    return dict(logits=rel(y, yr), grads=float((num / den) ** 0.5), buffers=max(berr), worst=worst)


def predict(case, train, layers=(2, 2, 1, 1), num_classes=32, seed=7, frames=(8, 128, 3)):
    """errors() of the rounding emulation of CASES[case] against exact fp64 (CPU)"""
    import emu_modes
    from embedders import resnext_hip
    from oracle import backbones_ref as BR
    from test_resnext_hip import structured_frames
    with pytest.MonkeyPatch.context() as mp:
        select(mp, case)
        install(mp, emu_modes)
        ref = make_net(num_classes, seed, layers).double()
        m = copy.deepcopy(ref)
        ref.train(train); m.train(train)
        x = structured_frames(*frames).double()
        r = loss_weights(frames[0], num_classes).double()
        yr = BR.resnext_forward(ref, x)
        (yr * r).sum().backward()
        m._hip_structure()
        emu_modes.reset()
        try:
            with emu_modes.rounding():
                y = resnext_hip.ResNeXtFunction.apply(m, x, *[p for _, p in m.named_parameters()])
                (y * r).sum().backward()
        finally:
            emu_modes.reset()
        return errors(m, ref, y, yr)
