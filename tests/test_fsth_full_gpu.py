"""Full geometry of the FSTH plugin family on the GPU -- widths 64 .. 512, 256 x 256, 6 embedder blocks / 7 critic blocks, 2 identities x 4 frames --
against the test-local restatement (tests/fsth_restatement.py, pinned to the reference by tests/test_fsth_cpu.py) evaluated in fp64 on the CPU.

Forward (embeds, embeds_elemwise; the three scores and all features): 1e-3 plain rel-L2, in the default precision assignment and in bf16x3.
Gradients: every parameter gradient < 1e-3 TIE-MASKED -- the fp64 restatement replays the ReLU patterns the HIP run taped, so both sides differentiate
the same piecewise-linear branch.  So that the masking cannot hide a wrong kernel it is held to a condition computed from the fp64 side alone: per ReLU
site, the number of elements whose taped sign differs from the fp64 sign must not exceed 4 x the number of fp64 pre-activations with
|x| < u * rms(site), u = the operand unit of the mode (2^-17 bf16x3, 2^-11 f16): only elements that close to zero can legitimately flip (two rounded
operands per product, error carried through up to 11 layers: sqrt(11) ~ 3.3 < 4).  The untied error and the fp32-restatement-vs-fp64 floor are printed."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import fsth_restatement as R          # noqa: E402
from test_fsth_cpu import plugin, toy_args          # noqa: E402

UNIT = {'bf16x3': 2.0 ** -17, 'f16': 2.0 ** -11}


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def full_args(**kw):
    return toy_args(image_size=256, num_channels=64, max_num_channels=512, embed_channels=512, embed_num_blocks=6, dis_num_blocks=7, num_labels=100,
                    device='cuda', **kw)


def with_tape(fn):
    """run ``fn`` (a forward through the HIP modules) while recording the activation pattern of every ReLU site -> (result, masks NCHW, CPU)"""
    from latent_pose_reenactment_amd import nn as lpnn
    lpnn.RELU_TAPE = []
    try:
        out = fn()
        masks = [m.permute(0, 3, 1, 2).cpu() for m in lpnn.RELU_TAPE]
    finally:
        lpnn.RELU_TAPE = None
    return out, masks


def check_tie_condition(masks, taps, unit, what):
    """per ReLU site: elements whose taped sign differs from the fp64 sign vs 4 x the fp64 pre-activations within ``unit`` * rms of zero"""
    assert len(masks) == len(taps), (len(masks), len(taps))
    rows = []
    for i, (m, x) in enumerate(zip(masks, taps)):
        x = x.detach()
        assert tuple(m.shape) == tuple(x.shape), (i, m.shape, x.shape)
        flipped = int((m != (x > 0)).sum())
        near = int((x.abs() < unit * x.pow(2).mean().sqrt()).sum())
        rows.append((i, x.numel(), flipped, near))
    print(f'[tie-condition] {what}: (site, elements, sign flips vs fp64, fp64 |x| < u rms) = {rows}')
    bad = [r for r in rows if r[2] > 4 * r[3]]
    assert not bad, f'{what}: ReLU sites whose taped pattern differs from fp64 beyond what rounding near zero explains: {bad}'


def stick_frames(n, size, seed):
    mod = plugin('dataloaders', 'synthetic_voxceleb2_stickmen')
    g = torch.Generator().manual_seed(seed)
    return torch.stack([mod.draw_stickman(mod.face_keypoints(g), size) for _ in range(n)])


def count_stem8_launches(monkeypatch):
    """-> list that receives one entry per two-source forward launch (so a test can tell which route ran)"""
    from latent_pose_reenactment_amd import hipops
    calls, real = [], hipops.stem8_conv

    def counted(*a, **k):
        calls.append(k.get('ksize'))
        return real(*a, **k)
    monkeypatch.setattr(hipops, 'stem8_conv', counted)
    return calls


# ``stem8``: the first convs on the two-source kernels (LP_STEM8=1) instead of the default generic route
@pytest.mark.parametrize('prec,avg,stem8', [('default', 'sum', False), ('default', 'max', False), ('bf16x3', 'sum', False), ('default', 'sum', True)])
def test_embedder_fsth_full_geometry_vs_fp64_restatement(prec, avg, stem8, monkeypatch):
    from latent_pose_reenactment_amd import hipops
    monkeypatch.setattr(hipops, '_STEM8', stem8)
    launches = count_stem8_launches(monkeypatch)
    monkeypatch.delenv('LP_PREC_E_FSTH', raising=False)
    if prec == 'default':
        monkeypatch.delenv('LP_PREC', raising=False)
    else:
        monkeypatch.setenv('LP_PREC', prec)
    from latent_pose_reenactment_amd import fsth, nn as lpnn
    mode = {v: k for k, v in lpnn.PREC_NAMES.items()}[fsth.embedder_prec()]
    torch.manual_seed(0)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(full_args(average_function=avg)).train()
    g = torch.Generator().manual_seed(2)
    b, k = 2, 4
    rgbs0 = torch.rand(b, k, 3, 256, 256, generator=g)
    stick = stick_frames(b * k, 256, 4).reshape(b, k, 3, 256, 256)
    r1, r2 = torch.randn(b, 512, generator=g), torch.randn(b, k, 512, generator=g)
    with torch.no_grad():
        for _ in range(3):                  # settle the power iterations
            E({'enc_rgbs': rgbs0.cuda(), 'enc_stickmen': stick.cuda()})
    sd = {kk: v.detach().cpu().clone() for kk, v in E.state_dict().items()}
    rgbs = rgbs0.clone().cuda().requires_grad_(True)
    dd = {'enc_rgbs': rgbs, 'enc_stickmen': stick.cuda()}
    _, masks = with_tape(lambda: E(dd))
    params = dict(E.named_parameters())
    loss = (dd['embeds'] * r1.cuda()).sum() + (dd['embeds_elemwise'] * r2.cuda()).sum()
    grads = torch.autograd.grad(loss, [rgbs] + list(params.values()))
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def oracle(replay, dtype=torch.float64):
        st = {kk: v.to(dtype) if v.is_floating_point() else v.clone() for kk, v in sd.items()}
        for kk in params:
            st[kk].requires_grad_(True)
        x = rgbs0.to(dtype).requires_grad_(True)
        taps = []
        R.RELU_REPLAY = None if replay is None else list(replay)
        try:
            embeds, elem = R.embedder_forward(st, x, stick.to(dtype), avg, training=True, taps=taps)
        finally:
            left = None if R.RELU_REPLAY is None else len(R.RELU_REPLAY)
            R.RELU_REPLAY = None
        assert not left, f'{left} recorded ReLU sites were not consumed by the restatement'
        l = (embeds * r1.to(dtype)).sum() + (elem * r2.to(dtype)).sum()
        gr = torch.autograd.grad(l, [x] + [st[kk] for kk in params])
        return embeds, elem, gr, taps
    assert bool(launches) == stem8, launches
    embeds, elem, g_true, taps = oracle(None)
    assert len(taps) == 12          # stem + 5 blocks x (input, hidden) + the ReLU behind the blocks
    check_tie_condition(masks, taps, UNIT[mode], f'embedder FSTH {avg} ({mode})')
    del taps
    _, _, g_tied, _ = oracle(masks)
    e32, l32, g32, _ = oracle(None, torch.float32)
    errs = {'embeds': rel(dd['embeds'], embeds), 'embeds_elemwise': rel(dd['embeds_elemwise'], elem)}
    names = ['d_enc_rgbs'] + list(params)
    gerr = {n: rel(a, t) for n, a, t in zip(names, grads, g_tied)}
    untied = {n: rel(a, t) for n, a, t in zip(names, grads, g_true)}
    floor = {n: rel(a, t) for n, a, t in zip(names, g32, g_true)}
    worst = sorted(gerr.items(), key=lambda kv: -kv[1])[:4]
    print(f'[parity-256] embedder FSTH {avg} prec={prec} stem8={stem8} (operands {mode}): forward {errs}; fp32 restatement vs fp64: embeds {rel(e32, embeds):.2e} '
          f'elemwise {rel(l32, elem):.2e}; tie-masked grads worst {[(n, round(v, 6)) for n, v in worst]} over {len(gerr)} tensors; untied worst '
          f'{max(untied.values()):.3e} ({max(untied, key=untied.get)}); fp32 restatement untied floor {max(floor.values()):.3e}')
    assert all(v < 1e-3 for v in errs.values()), errs
    assert all(v < 1e-3 for v in gerr.values()), worst


@pytest.mark.parametrize('prec,stem8', [('default', False), ('bf16x3', False), ('default', True)])
def test_critic_fsth_full_geometry_vs_fp64_restatement(prec, stem8, monkeypatch):
    """three passes with their own power iterations, adversarial + feature-matching losses, both backward passes; the stickman shared by the passes"""
    from latent_pose_reenactment_amd import hipops
    monkeypatch.setattr(hipops, '_STEM8', stem8)
    launches = count_stem8_launches(monkeypatch)
    for kk in ('LP_D_DPASS_PREC', 'LP_D_DPASS_FROM', 'LP_D_GPASS_PREC', 'LP_D_GPASS_FROM'):
        monkeypatch.delenv(kk, raising=False)
    if prec == 'default':
        monkeypatch.delenv('LP_PREC', raising=False)
    else:
        monkeypatch.setenv('LP_PREC', prec)
    from latent_pose_reenactment_amd import nn as lpnn
    mode = {v: k for k, v in lpnn.PREC_NAMES.items()}[lpnn.default_prec()]
    torch.manual_seed(0)
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(full_args()).train()
    D.keep_reference_waste = True          # pass 1 also deposits (later discarded) weight gradients, as the reference does
    g = torch.Generator().manual_seed(2)
    fake0, real = torch.rand(2, 3, 256, 256, generator=g), torch.rand(2, 1, 3, 256, 256, generator=g)
    stick = stick_frames(2, 256, 6)[:, None]
    label = torch.tensor([17, 3])
    inputs = lambda f: {'fake_rgbs': f, 'target_rgbs': real.cuda(), 'dec_stickmen': stick.cuda(), 'label': label.cuda()}
    with torch.no_grad():
        for _ in range(3):                  # settle the power iterations
            D(inputs(fake0.cuda()))
    sd = {kk: v.detach().cpu().clone() for kk, v in D.state_dict().items()}
    fake = fake0.clone().cuda().requires_grad_(True)
    dd = inputs(fake)
    _, masks = with_tape(lambda: D(dd))
    # feature matching on the common branch of its own discontinuity: |f - r| = s * (f - r) with the sign pattern s of the HIP features on both sides
    signs = [torch.sign(f.detach() - r.detach()).cpu() for f, r in zip(dd['fake_features'], dd['real_features'])]

    def losses(d, dev, dtype):
        lg = -d['fake_score_G'].mean() + 10.0 * sum((s.to(dev, dtype) * (f - r.detach())).mean()
                                                    for s, f, r in zip(signs, d['fake_features'], d['real_features'])) / len(signs)
        ld = torch.relu(1.0 - d['real_score']).mean() + torch.relu(1.0 + d['fake_score_D']).mean()
        return lg, ld
    lg, ld = losses(dd, 'cuda', torch.float32)
    params = dict(D.named_parameters())
    gG = torch.autograd.grad(lg, [fake] + list(params.values()), retain_graph=True, allow_unused=True)
    gD = torch.autograd.grad(ld, list(params.values()), allow_unused=True)
    torch.cuda.synchronize()
    torch.set_num_threads(min(16, os.cpu_count() or 1))

    def oracle(replay, dtype=torch.float64):
        st = {kk: v.to(dtype) if v.is_floating_point() else v.clone() for kk, v in sd.items()}
        for kk in params:
            st[kk].requires_grad_(True)
        f = fake0.to(dtype).requires_grad_(True)
        taps = []
        R.RELU_REPLAY = None if replay is None else list(replay)
        try:
            out = R.critic_forward(st, f, real[:, 0].to(dtype), stick[:, 0].to(dtype), label, 256, training=True, taps=taps)
        finally:
            left = None if R.RELU_REPLAY is None else len(R.RELU_REPLAY)
            R.RELU_REPLAY = None
        assert not left, f'{left} recorded ReLU sites were not consumed by the restatement'
        olg, old = losses(out, 'cpu', dtype)
        oG = torch.autograd.grad(olg, [f] + [st[kk] for kk in params], retain_graph=True, allow_unused=True)
        oD = torch.autograd.grad(old, [st[kk] for kk in params], allow_unused=True)
        return out, olg, old, oG, oD, taps
    assert bool(launches) == stem8, launches
    out, olg, old, oG_true, oD_true, taps = oracle(None)
    assert len(taps) == 3 * 14          # per pass: stem + 6 blocks x (input, hidden) + the ReLU in front of the head
    check_tie_condition(masks, taps, UNIT[mode], f'critic FSTH ({mode})')
    del taps
    _, _, _, oG, oD, _ = oracle(masks)
    o32, lg32, ld32, oG32, oD32, _ = oracle(None, torch.float32)
    errs = {'loss_G': rel(lg, olg), 'loss_D': rel(ld, old)}
    for kk in ('fake_score_G', 'fake_score_D', 'real_score'):
        errs[kk] = rel(dd[kk], out[kk])
    for i, (a, c, e, f2) in enumerate(zip(dd['fake_features'], out['fake_features'], dd['real_features'], out['real_features'])):
        errs[f'fake_feat{i}'], errs[f'real_feat{i}'] = rel(a, c), rel(e, f2)
    assert len(dd['fake_features']) == 7

    def table(mine_G, mine_D, ref_G, ref_D):
        t = {'G.d_fake': rel(mine_G[0], ref_G[0])}
        for (kk, _), a, c in zip(params.items(), mine_G[1:], ref_G[1:]):
            if a is not None and c is not None and c.abs().max() > 0:
                t['G.' + kk] = rel(a, c)
        for (kk, _), a, c in zip(params.items(), mine_D, ref_D):
            if a is not None and c is not None and c.abs().max() > 0:
                t['D.' + kk] = rel(a, c)
        return t
    gerr, untied, floor = table(gG, gD, oG, oD), table(gG, gD, oG_true, oD_true), table(oG32, oD32, oG_true, oD_true)
    worst = sorted(gerr.items(), key=lambda kv: -kv[1])[:4]
    print(f'[parity-256] critic FSTH prec={prec} stem8={stem8} (default operands {mode}): forward worst {max(errs.values()):.2e} ({max(errs, key=errs.get)}); '
          f'fp32 restatement vs fp64 scores {rel(o32["fake_score_G"], out["fake_score_G"]):.2e}; tie-masked grads worst '
          f'{[(n, round(v, 6)) for n, v in worst]} over {len(gerr)} tensors; untied worst {max(untied.values()):.3e} ({max(untied, key=untied.get)}); '
          f'fp32 restatement untied floor {max(floor.values()):.3e}')
    assert all(v < 1e-3 for v in errs.values()), errs
    assert all(v < 1e-3 for v in gerr.values()), worst
