"""GPU parity tests of the spectral-norm kernels (csrc/spectral_norm.hip and the <G, W_orig> partials of csrc/conv_wgrad.hip's reductions)
against fp64 torch-CPU references written out here:
  * the batched power iteration (lp_sn_power_iter through nn.SNBatch) on one table of every SN layer of the full-size generator and critic
    (label embedding included) plus synthetic edge layers -- legacy torch.nn.utils.spectral_norm update, eval mode, determinism, and
    scratch isolation between the layers of one table;
  * the SN gradient rule  dW_orig = G/sigma - (<G, W_orig>/sigma^2) u v^T  standalone (lp_sn_grad_apply), fused into every weight-gradient
    reduction route, and batched (lp_sn_grad_apply_batch).
The SN gradient is orthogonal to W_orig when sigma = u^T W_orig v; that check is sensitive to a wrong <G, W_orig> where a rel-L2 gate is not."""
import os
import random
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {0: 1e-2, 1: 3e-5, 2: 1e-3}          # test_hip_ops.test_conv_wgrad's rel-L2 gates per operand mode (bf16, bf16x3, f16)
SN_TOL = 3e-5                              # power iteration: fp32 mat-vecs vs fp64
ORTHO_FACTOR = 16                          # orthogonality bound = this x the fp32 torch evaluation of the same formula


def _ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def report(name, err, tol):
    print(f'[parity] {name}: rel-L2 {err:.3e} (tol {tol:.0e})')
    assert err < tol, f'{name}: rel-L2 {err:.3e} >= {tol}'


def _cpu_threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# power iteration
# ---------------------------------------------------------------------------------------------------------------------------------------
def _layer(w, eps, gen, name):
    """the attributes nn.SNBatch reads from an SNWeight, on the GPU, with a seeded (u, v)"""
    rows, cols = w.shape[0], w[0].numel()
    u = F.normalize(torch.randn(rows, generator=gen, dtype=torch.float64), dim=0).float()
    v = F.normalize(torch.randn(cols, generator=gen, dtype=torch.float64), dim=0).float()
    return SimpleNamespace(weight_orig=w, weight_u=u.cuda(), weight_v=v.cuda(), eps=eps, name=name)


def _misaligned(rows, cols, gen):
    """a contiguous [rows][cols] weight whose storage starts 1 float past a 16-byte boundary (the kernels' scalar fallback)"""
    base = torch.empty(rows * cols + 4, dtype=torch.float32, device='cuda')
    assert base.data_ptr() % 16 == 0
    w = base[1:1 + rows * cols].view(rows, cols)
    w.copy_(torch.randn(rows, cols, generator=gen).cuda() / cols ** 0.5)
    assert w.is_contiguous() and w.data_ptr() % 16 == 4
    return w


def _edge_layers(gen):
    out = []
    for rows, cols in [(5, 1), (33, 1), (7, 3), (64, 27), (300, 27), (31, 130), (257, 130),          # cols % 4 != 0: scalar paths
                       (1, 64), (31, 64), (32, 64), (33, 64), (257, 64), (1, 4), (33, 4608),          # row-block and r + 4 <= r1 tails
                       (40, 764), (40, 768), (40, 772), (35, 1020), (35, 1024), (35, 1028), (3, 2044)]:   # c + 192 < C4 boundaries
        out.append(_layer(torch.randn(rows, cols, generator=gen).cuda() / cols ** 0.5, 1e-4, gen, f'edge{rows}x{cols}'))
    for rows, cols in [(1, 1), (1, 2), (2, 1), (3, 1)]:             # scratch of 4 floats or fewer: next to the neighbour's first partials
        out.append(_layer(torch.randn(rows, cols, generator=gen).cuda(), 1e-4, gen, f'tiny{rows}x{cols}'))
    for rows, cols in [(33, 64), (70, 1028)]:
        out.append(_layer(_misaligned(rows, cols, gen), 1e-12, gen, f'misaligned{rows}x{cols}'))
    # norms below eps: v = W^T u / eps and u = W v / eps are not unit vectors (excluded from the invariants)
    out.append(_layer(torch.randn(8, 12, generator=gen).cuda() * 1e-3, 1e-2, gen, 'below_eps8x12'))
    return out


@pytest.fixture(scope='module')
def sn_table():
    """every SNWeight layer of the full-size generator and critic (label embedding 98000 x 512 included) plus the edge layers, one table;
    (layers, fp64 CPU copies of their [rows][cols] weights)"""
    from latent_pose_reenactment_amd.discriminators.no_landmarks import Discriminator
    from latent_pose_reenactment_amd.nn import Generator
    torch.manual_seed(0)
    G = Generator('zero', 3, 4, 64, 512, 512, 256, 'in', 4, 2, 256)
    D = Discriminator('zero', 3, 3, 64, 512, 512, 7, 256, 98000)
    gen = torch.Generator().manual_seed(1234)
    layers = []
    for tag, mods in (('G', G._sn_layers()[0]), ('D', D._conv_sn_layers() + [D.embed])):
        for i, m in enumerate(mods):
            layers.append(_layer(m.weight_orig.detach().cuda().contiguous(), m.eps, gen, f'{tag}{i}:{tuple(m.weight_orig.shape)}'))
    del G, D
    edge = _edge_layers(gen)
    order = list(range(len(layers) + len(edge)))
    layers += edge
    random.Random(5).shuffle(order)                  # the edge layers sit between real ones
    layers = [layers[i] for i in order]
    yield layers, [l.weight_orig.reshape(l.weight_orig.shape[0], -1).double().cpu() for l in layers]


def _state(layers):
    return [(l.weight_u.clone(), l.weight_v.clone()) for l in layers]


def _restore(layers, st):
    for l, (u, v) in zip(layers, st):
        l.weight_u.copy_(u); l.weight_v.copy_(v)


def _ref_update(w, u, v, eps, training):
    """the legacy torch.nn.utils.spectral_norm update (fp64)"""
    if training:
        v = F.normalize(w.t() @ u, dim=0, eps=eps)
        u = F.normalize(w @ v, dim=0, eps=eps)
    return u, v, u @ (w @ v)


def _run(sb, training):
    with torch.no_grad():
        states = sb.update(training)
    torch.cuda.synchronize()
    return [(uo.clone(), vo.clone(), sig.clone()) for uo, vo, sig in states]


def test_power_iteration_train_matches_fp64_legacy_update(sn_table):
    from latent_pose_reenactment_amd.nn import SNBatch
    _cpu_threads()
    layers, w64 = sn_table
    st0 = _state(layers)
    sb = SNBatch(layers)
    ref = [(u.double().cpu(), v.double().cpu()) for u, v in st0]
    worst = {}
    for step in range(3):
        got = _run(sb, True)
        for i, (l, w) in enumerate(zip(layers, w64)):
            u, v, sigma = _ref_update(w, ref[i][0], ref[i][1], l.eps, True)
            ref[i] = (u, v)
            uo, vo, sig = got[i]
            errs = {'weight_u': rel(l.weight_u, u), 'weight_v': rel(l.weight_v, v), 'u_used': rel(uo, u), 'v_used': rel(vo, v),
                    'sigma': rel(sig[0], sigma), 'inv_sigma': rel(sig[1], 1 / sigma)}
            for k, e in errs.items():
                assert e < SN_TOL, (step, l.name, k, e)
                if e >= worst.get(k, (0.0, ''))[0]:
                    worst[k] = (e, l.name)
            if l.name.startswith('below_eps'):
                continue
            u_g, v_g = uo.double().cpu(), vo.double().cpu()
            assert abs(u_g.norm().item() - 1) < 1e-5 and abs(v_g.norm().item() - 1) < 1e-5, (step, l.name)
            assert rel(sig[0], (w @ v_g).norm()) < SN_TOL, (step, l.name, 'sigma != |W v|')
    for k, (e, name) in worst.items():
        report(f'sn_power_iter train {k} (worst layer {name}, {len(layers)} layers x 3 steps)', e, SN_TOL)
    _restore(layers, st0)


def test_power_iteration_eval_keeps_u_v_and_gives_sigma(sn_table):
    from latent_pose_reenactment_amd.nn import SNBatch
    _cpu_threads()
    layers, w64 = sn_table
    st0 = _state(layers)
    got = _run(SNBatch(layers), False)
    worst = 0.0
    for l, w, (u0, v0), (uo, vo, sig) in zip(layers, w64, st0, got):
        assert torch.equal(l.weight_u, u0) and torch.equal(l.weight_v, v0), l.name
        assert torch.equal(uo, u0) and torch.equal(vo, v0), l.name
        u64, v64 = u0.double().cpu(), v0.double().cpu()
        _, _, sigma = _ref_update(w, u64, v64, l.eps, False)
        scale = (u64.norm() * (w @ v64).norm()).clamp_min(1e-30).item()      # sigma of an unconverged (u, v) can be a small difference
        worst = max(worst, abs(sig[0].item() - sigma.item()) / scale, abs(sig[0].item() * sig[1].item() - 1))
    report(f'sn_power_iter eval sigma = u^T W v, |error| / (|u| |W v|) ({len(layers)} layers)', worst, SN_TOL)


def _check_table_layout(sb, layers):
    """every descriptor's u / v copies and scratch ([row blocks][cols] partials, [rows] W v, [col blocks] norm partials) are 16-byte aligned,
    inside their set's buffers and disjoint from every other layer's"""
    import struct
    from latent_pose_reenactment_amd import _lib
    rb = _lib.lib().lp_sn_row_block()
    st = _state(layers)
    with torch.no_grad():
        sb.update(True)                                  # builds the buffer sets
    _restore(layers, st)
    for table, _, (sig, uo, vo, scratch) in sb.sets:
        blob = table.cpu().numpy().tobytes()
        spans = {'u': [], 'v': [], 'part': []}
        for i, l in enumerate(layers):
            w, u, v, uout, vout, sout, part, rows, cols, eps, _ = struct.unpack_from('<QQQQQQQiifi', blob, 72 * i)
            assert (w, u, v, rows, cols) == (l.weight_orig.data_ptr(), l.weight_u.data_ptr(), l.weight_v.data_ptr(), l.weight_orig.shape[0],
                                             l.weight_orig[0].numel()), l.name
            nrb = (rows + rb - 1) // rb
            for key, ptr, n, buf in (('u', uout, rows, uo), ('v', vout, cols, vo), ('part', part, nrb * cols + rows + (cols + 63) // 64, scratch)):
                assert ptr % 16 == 0 and buf.data_ptr() <= ptr and ptr + 4 * n <= buf.data_ptr() + 4 * buf.numel(), (l.name, key)
                spans[key].append((ptr, ptr + 4 * n, l.name))
        for key, sp in spans.items():
            sp.sort()
            for (a0, a1, na), (b0, b1, nb) in zip(sp, sp[1:]):
                assert a1 <= b0, f'{key} slices of {na} and {nb} overlap'


def test_power_iteration_is_deterministic_and_layers_do_not_share_scratch(sn_table):
    """two updates from one state are bit-identical; so is every layer's result when the table holds the layers in another order
    (a layer whose scratch slice overlapped a neighbour's would change with its neighbours)"""
    from latent_pose_reenactment_amd.nn import SNBatch
    layers, _ = sn_table
    st0 = _state(layers)
    sb = SNBatch(layers)
    _check_table_layout(sb, layers)
    runs = []
    for _ in range(2):
        _restore(layers, st0)
        runs.append((_run(sb, True), _state(layers)))
    perm = list(range(len(layers)))
    random.Random(11).shuffle(perm)
    shuffled = [layers[i] for i in perm]
    _restore(layers, st0)
    out = _run(SNBatch(shuffled), True)
    back = [None] * len(layers)
    for j, i in enumerate(perm):
        back[i] = out[j]
    runs.append((back, _state(layers)))
    _restore(layers, st0)
    ref_out, ref_st = runs[0]
    for k, (o, s) in enumerate(runs[1:]):
        for i, l in enumerate(layers):
            assert all(torch.equal(a, b) for a, b in zip(o[i], ref_out[i])), ('same state' if k == 0 else 'shuffled table', l.name)
            assert torch.equal(s[i][0], ref_st[i][0]) and torch.equal(s[i][1], ref_st[i][1]), ('same state' if k == 0 else 'shuffled', l.name)
    print(f'[parity] sn_power_iter: bit-identical over 2 runs and a shuffled table of {len(layers)} layers')


# ---------------------------------------------------------------------------------------------------------------------------------------
# SN gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
def _top_sv(w, steps=30):
    """the top singular vectors (u, v) of W [rows][cols] by fp64 power iteration"""
    v = F.normalize(torch.ones(w.shape[1], dtype=torch.float64) + torch.arange(w.shape[1], dtype=torch.float64) * 1e-3, dim=0)
    for _ in range(steps):
        u = F.normalize(w @ v, dim=0)
        v = F.normalize(w.t() @ u, dim=0)
    u = F.normalize(w @ v, dim=0)
    return u, v


def _sn_inputs(w64):
    """fp32 device operands (w, u, v, sig = [sigma, 1/sigma]) with (u, v) the top singular vectors of W, and the fp64 (w, u, v, sig) the
    reference uses: the same fp32 values, sigma = u^T W v of them (the case the orthogonality holds in)"""
    u64, v64 = _top_sv(w64)
    wf, uf, vf = w64.float(), u64.float(), v64.float()
    wd, ud, vd = wf.double(), uf.double(), vf.double()
    sigma = (ud @ (wd @ vd)).item()
    sig = torch.tensor([sigma, 1.0 / sigma], dtype=torch.float64).float()
    return (wf.cuda(), uf.cuda(), vf.cuda(), sig.cuda()), (wd, ud, vd, sig.double())


def _sn_ref(g64, w64, u64, v64, sig64):
    """fp64 autograd of W_orig / (u^T W_orig v) with u, v constants, upstream g; evaluated at the fp32 sigma the kernel is given"""
    w = w64.clone().requires_grad_(True)
    sigma = u64 @ (w.reshape(w.shape[0], -1) @ v64)
    sigma = sigma + (sig64[0] - sigma.detach())                # value = the fp32 sigma handed to the kernel, gradient of u^T W v
    (w / sigma).backward(g64)
    return w.grad


def _ortho(dw, w):
    dw, w = dw.detach().double().cpu().reshape(-1), w.detach().double().cpu().reshape(-1)
    return abs((dw @ w).item()) / (dw.norm() * w.norm()).clamp_min(1e-300).item()


def _ortho_floor(g, w, u, v, sig):
    """orthogonality of the same formula evaluated in fp32 by torch: the largest over two summation orders of <G, W>, each also taken
    1 ulp up and down (a single evaluation can cancel its rounding errors by chance; the kernels sum in yet another order)"""
    g, w, u, v, sig = (t.detach().float().cpu() for t in (g, w, u, v, sig))
    g2, w2 = g.reshape(g.shape[0], -1), w.reshape(w.shape[0], -1)
    a = sig[1]
    inf = torch.tensor(float('inf'))
    out = 0.0
    for d0 in (torch.dot(g2.reshape(-1), w2.reshape(-1)), (g2 * w2).sum(dim=1).sum()):
        for d in (d0, torch.nextafter(d0, inf), torch.nextafter(d0, -inf)):
            dw = a * g2 - (d * a * a) * torch.outer(u, v)
            out = max(out, _ortho(dw, w2))
    return max(out, 1e-9)


def _check_ortho(name, dw, g_raw, w, u, v, sig):
    got, floor = _ortho(dw, w), _ortho_floor(g_raw, w, u, v, sig)
    print(f'[ortho] {name}: |<dW, W>|/(|dW||W|) {got:.3e}  fp32-torch floor {floor:.3e}  (bound {ORTHO_FACTOR} x floor)')
    assert got < ORTHO_FACTOR * floor, f'{name}: orthogonality {got:.3e} >= {ORTHO_FACTOR} x {floor:.3e}'


def _g_with_uv(gen, rows, cols, u64, v64, beta):
    """random G plus a component along u v^T of beta x |random part| (beta = 0: the correction term is small)"""
    g = torch.randn(rows, cols, generator=gen, dtype=torch.float64)
    return g + beta * g.norm() * torch.outer(u64, v64)


SN_STANDALONE_SHAPES = [(1, 3), (37, 27), (64, 576), (513, 1031), (512, 4608), (700, 1000)]   # totals: < 1024, not % 1024, > 512 * 1024


@pytest.mark.parametrize('beta', [0.0, 0.7])
@pytest.mark.parametrize('shape', SN_STANDALONE_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_sn_grad_apply_standalone(shape, beta):
    ops = _ops()
    _cpu_threads()
    rows, cols = shape
    gen = torch.Generator().manual_seed(rows * 7 + cols)
    w64 = torch.randn(rows, cols, generator=gen, dtype=torch.float64) / cols ** 0.5
    (w, u, v, sig), (wd, ud, vd, sd) = _sn_inputs(w64)
    g32 = _g_with_uv(gen, rows, cols, ud, vd, beta).float()
    ref = _sn_ref(g32.double(), wd, ud, vd, sd)
    g = g32.cuda()
    out = ops.sn_grad_apply(g, w, u, v, sig)                                 # in place on g
    acc0 = torch.randn(rows, cols, generator=gen).cuda()
    acc = acc0.clone()
    g2 = g32.cuda()
    assert ops.sn_grad_apply(g2, w, u, v, sig, accum=acc) is None
    torch.cuda.synchronize()
    assert out.data_ptr() == g.data_ptr() and torch.equal(g2.cpu(), g32), 'accum form must leave g untouched'
    report(f'sn_grad_apply {shape} beta={beta} in place', rel(out, ref), 1e-5)
    report(f'sn_grad_apply {shape} beta={beta} accum', rel(acc, acc0.double().cpu() + ref), 1e-5)
    _check_ortho(f'sn_grad_apply {shape} beta={beta}', out, g32, w, u, v, sig)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _act_ref(x, pro, scale, shift, ups):
    a = x
    if pro == 1:
        a = torch.relu(x * scale[:, :, None, None] + shift[:, :, None, None])
    elif pro == 2:
        a = torch.relu(x)
    if ups:
        a = a.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return a


# (N, H(out), W, Cin, Cout, ks, ups, pro), route.  Reduction routes (conv_wgrad.hip): tiled <=> Cout * ceil(Cin / 128) >= 512;
# otherwise flat<32> <=> ceil(9|1 * Cout * Cin / 256) < 400, else flat<256>.  3x3 layers with W >= 16, H >= 8 and >= 32 16x8 tiles run
# wgrad3_pipe; 1x1 layers without a bias gradient run wgrad1x1; <= 4 channels on a side run thin_wgrad (no fused dot: _sn_finish, ndot = 0).
FUSED_CASES = [
    ((2, 8, 8, 128, 512, 3, 0, 1), 'conv_wgrad_kernel<COB 128> + tiled (512 * 1 >= 512)'),
    ((2, 8, 8, 64, 64, 3, 0, 1), 'conv_wgrad_kernel + flat<32> (36864 / 256 = 144 < 400)'),
    ((8, 4, 4, 128, 128, 3, 0, 1), 'conv_wgrad_kernel<COB 128> + flat<256> (147456 / 256 = 576 >= 400)'),
    ((2, 16, 16, 64, 128, 1, 0, 0), 'wgrad1x1 + flat<32> (8192 / 256 = 32 < 400)'),
    ((1, 16, 16, 128, 512, 1, 0, 0), 'wgrad1x1 + tiled (512 * 1 >= 512)'),
    ((4, 32, 32, 128, 128, 3, 0, 1), 'wgrad3_pipe (2*4*4 = 32 tiles) + flat<256> (576 >= 400)'),
    ((2, 64, 64, 64, 64, 3, 0, 2), 'wgrad3_pipe (64 tiles) + flat<32> (144 < 400)'),
    ((2, 16, 16, 128, 64, 3, 1, 1), 'upsampled conv_wgrad_kernel (4 tiles) + flat<32> (288 < 400)'),
    ((2, 64, 64, 64, 64, 3, 1, 1), 'upsampled wgrad3_pipe (64 tiles) + flat<32> (144 < 400)'),
    ((2, 16, 16, 3, 64, 3, 0, 0), 'thin_wgrad (Cin = 3): standalone _sn_finish'),
    ((2, 20, 12, 128, 4, 3, 0, 2), 'thin_wgrad (Cout = 4): standalone _sn_finish'),
]


@pytest.mark.parametrize('prec', [1, 0, 2])
@pytest.mark.parametrize('case,route', FUSED_CASES, ids=[str(c[0]) for c in FUSED_CASES])
def test_conv_wgrad_fused_sn(case, route, prec):
    ops = _ops()
    _cpu_threads()
    n, h, w, cin, cout, ks, ups, pro = case
    thin = not ups and ops.thin_wgrad_supported(cin, cout, ks, pro, w)
    assert thin == route.startswith('thin'), (case, route)
    if not thin:
        nd = _lib_dot_blocks(cin, cout, ks)
        assert nd == _route_blocks(cin, cout, ks, route), (case, route, nd)
    g = torch.Generator().manual_seed(11 + prec)
    hin, win = (h // 2, w // 2) if ups else (h, w)
    x = torch.randn(n, cin, hin, win, generator=g, dtype=torch.float64)
    scale = torch.randn(n, cin, generator=g, dtype=torch.float64)
    shift = torch.randn(n, cin, generator=g, dtype=torch.float64) * 0.5
    dy = torch.randn(n, cout, h, w, generator=g, dtype=torch.float64)
    wz = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    F.conv2d(_act_ref(x, pro, scale, shift, ups), wz, None, 1, ks // 2).backward(dy)
    graw = wz.grad                                                        # raw weight gradient (fp64)
    # W_orig with a large share along G: <G, W_orig> and the u v^T correction are not negligible
    w64 = (0.5 * torch.randn(cout, cin * ks * ks, generator=g, dtype=torch.float64) / (cin * ks * ks) ** 0.5
           + graw.reshape(cout, -1) / graw.norm() * cout ** 0.5)
    (wf, u, v, sig), (wd, ud, vd, sd) = _sn_inputs(w64)
    wf = wf.reshape(cout, cin, ks, ks).contiguous()
    ref = _sn_ref(graw, wd.reshape(cout, cin, ks, ks), ud, vd, sd)
    f32 = lambda t: t.float().cuda().contiguous()
    kw = dict(ksize=ks, upsample=bool(ups), pro=pro, scale=f32(scale), shift=f32(shift), prec=prec)
    xs, dys = f32(_nhwc(x)), f32(_nhwc(dy))
    fused = ops.conv_wgrad(xs, dys, sn=(wf, u, v, sig), **kw)
    acc0 = torch.randn(cout, cin, ks, ks, generator=g).cuda()
    acc = acc0.clone()
    assert ops.conv_wgrad(xs, dys, sn=(wf, u, v, sig), accum=acc, **kw) is None
    raw = ops.conv_wgrad(xs, dys, **kw)
    unfused = ops.sn_grad_apply(raw.clone(), wf, u, v, sig)
    acc_u = acc0.clone()
    ops.sn_grad_apply(raw.clone(), wf, u, v, sig, accum=acc_u)
    torch.cuda.synchronize()
    tag = f'conv_wgrad+sn {case} prec={prec} [{route}]'
    report(tag, rel(fused, ref), TOL[prec])
    report(tag + ' accum', rel(acc, acc0.double().cpu() + ref), TOL[prec])
    report(tag + ' fused vs unfused', rel(fused, unfused), 2e-6)
    report(tag + ' accum fused vs unfused', rel(acc, acc_u), 2e-6)
    _check_ortho(tag, fused, raw, wf, u, v, sig)


def _lib_dot_blocks(cin, cout, ks):
    from latent_pose_reenactment_amd import _lib
    return _lib.lib().lp_conv_wgrad_dot_blocks(cin, cout, ks)


def _route_blocks(cin, cout, ks, route):
    """the number of <dw, W_orig> partials the named reduction writes (one per block)"""
    t = ks * ks
    if 'tiled' in route:
        return cout * ((cin + 127) // 128)
    fo = 32 if 'flat<32>' in route else 256
    return (t * cout * cin + fo - 1) // fo


@pytest.mark.parametrize('prec', [1, 0, 2])
@pytest.mark.parametrize('up', [False, True])
def test_reflect_border_wgrad_sn(up, prec):
    """reflect_border_wgrad: the border share of the weight gradient goes through the standalone SN rule (_sn_finish, ndot = 0)"""
    ops = _ops()
    n, h, w_, cin, cout = 2, 16, 12, 64, 32
    torch.manual_seed(21 + prec + 3 * up)
    hs, ws = (h // 2, w_ // 2) if up else (h, w_)
    x = torch.randn(n, hs, ws, cin, device='cuda')
    a = ops.act_pack(x, pro=2, prec=prec)
    # the operand planes decoded to fp64: exactly what the kernel reads (tests/test_reflect_border.py)
    hi = a.hi[..., :a.c]
    if prec == 2:
        xt = hi.view(torch.float16).double()
    else:
        xt = (hi.to(torch.int32) << 16).view(torch.float32).double()
        if prec == 1:
            xt = xt + (a.lo[..., :a.c].to(torch.int32) << 16).view(torch.float32).double()
    xt = xt.permute(0, 3, 1, 2).cpu()
    if up:
        xt = F.interpolate(xt, scale_factor=2, mode='nearest')
    dy = torch.randn(n, h, w_, cout, device='cuda')
    wz = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(F.pad(xt, (1, 1, 1, 1), mode='reflect'), wz) - F.conv2d(xt, wz, padding=1)).backward(dy.permute(0, 3, 1, 2).double().cpu())
    graw = wz.grad
    w64 = torch.randn(cout, cin * 9, dtype=torch.float64) * 0.05 + graw.reshape(cout, -1) / graw.norm() * cout ** 0.5
    (wf, u, v, sig), (wd, ud, vd, sd) = _sn_inputs(w64)
    wf = wf.reshape(cout, cin, 3, 3).contiguous()
    ref = _sn_ref(graw, wd.reshape(cout, cin, 3, 3), ud, vd, sd)
    got = ops.reflect_border_wgrad(a, dy, prec=prec, upsample=up, sn=(wf, u, v, sig))
    raw = ops.reflect_border_wgrad(a, dy, prec=prec, upsample=up)
    acc0 = torch.randn(cout, cin, 3, 3, device='cuda')
    acc = acc0.clone()
    assert ops.reflect_border_wgrad(a, dy, prec=prec, upsample=up, sn=(wf, u, v, sig), accum=acc) is None
    torch.cuda.synchronize()
    tag = f'reflect_border_wgrad+sn up={up} prec={prec}'
    report(tag, rel(got, ref), 1e-5)
    report(tag + ' accum', rel(acc, acc0.double().cpu() + ref), 1e-5)
    _check_ortho(tag, got, raw, wf, u, v, sig)


def test_sn_grad_apply_batch_is_bit_identical_to_per_job_launches(monkeypatch):
    """sn_defer_begin / sn_defer_end: 45 deferred jobs (two SN_BATCH_MAX = 40 chunks) of mixed sizes -- one under 1024 elements, one over
    2^20, several ending inside a 1024-element block -- accumulate exactly what one lp_sn_grad_apply per job gives with the same partials"""
    ops = _ops()
    _cpu_threads()
    monkeypatch.setattr(ops, 'SN_DEFER', True)                                # (LP_SN_DEFER=0 would turn the batch off)
    gen = torch.Generator().manual_seed(77)
    shapes = [(64, 576), (37, 27), (128, 1152), (3, 5), (256, 2304), (512, 9), (33, 1031), (16, 64)] * 5 + \
             [(1, 3), (1100, 1000), (255, 4), (1024, 1), (7, 300)]
    assert len(shapes) == 45 and any(r * c < 1024 for r, c in shapes) and any(r * c > 1 << 20 for r, c in shapes[40:])
    jobs = []
    for k, (rows, cols) in enumerate(shapes):
        w64 = torch.randn(rows, cols, generator=gen, dtype=torch.float64) / cols ** 0.5
        (w, u, v, sig), (wd, ud, vd, sd) = _sn_inputs(w64)
        g = torch.randn(rows, cols, generator=gen).cuda()
        chunk = [64, 333, 1024, 4096][k % 4]                                  # ndot = ceil(total / chunk): from 1 to ~1100 partials
        prods = (g * w).reshape(-1)
        dot = torch.stack([c.sum() for c in prods.split(chunk)]).contiguous()
        acc0 = torch.randn(rows, cols, generator=gen).cuda()
        jobs.append(dict(g=g, sn=(w, u, v, sig), dot=dot, acc0=acc0, ref64=(wd, ud, vd, sd)))
    ops.sn_defer_begin()
    try:
        accs = []
        for j in jobs:
            acc = j['acc0'].clone()
            assert ops._sn_finish(j['g'], j['sn'], acc, j['dot'], j['dot'].numel()) is None
            accs.append(acc)
        assert len(ops._SN_DEFER['jobs']) == 45
    finally:
        ops.sn_defer_end()
    assert not ops._SN_DEFER['jobs']
    refs = []
    for j in jobs:                                                            # outside the deferral: one lp_sn_grad_apply per job
        acc = j['acc0'].clone()
        assert ops._sn_finish(j['g'], j['sn'], acc, j['dot'], j['dot'].numel()) is None
        refs.append(acc)
    torch.cuda.synchronize()
    worst = 0.0
    for k, (j, a, r) in enumerate(zip(jobs, accs, refs)):
        assert torch.equal(a, r), (k, shapes[k], (a - r).abs().max().item())
        wd, ud, vd, sd = j['ref64']
        worst = max(worst, rel(a, j['acc0'].double().cpu() + _sn_ref(j['g'].double().cpu(), wd, ud, vd, sd)))
    report('sn_grad_apply_batch (45 jobs, bit-identical to per-job launches) vs fp64', worst, 1e-5)
