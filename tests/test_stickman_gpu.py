"""GPU checks of the device stickman (csrc/stickman.hip -> hipops.stickman_render -> fsth.stickmen -> the three FSTH nets and drive.py):
  * the kernel against the fp64 restatement (tests/stickman_restatement.py) on sizes with whole and with ragged 16-byte rows, default and given line
    widths, 1 and 3 images, and three keypoint sets (seeded faces; zero-length segments and points on the image corners; all points equal).
    Gate: max-abs error <= 8 * 2^-23 * S / width -- eight times the fp32 rounding scale of a distance measured in pixels, over the line width;
    a real defect (half a pixel of offset, a missing closing edge, a wrong colour or width) moves values by >= 0.1.  The host's own fp32
    draw_stickman is held to the same gate on the same inputs first;
  * the wrapper: ``out=`` a slice of a larger tensor, refused inputs; capture into a graph and replay on new keypoints;
  * embedder, generator and critic (toy geometry, bf16x3): a keypoints-only batch is bit-identical to the batch that carries the rendered stickmen,
    outputs and parameter gradients; stickmen in the batch win; nothing is cached in the batch between forwards; neither key -> KeyError;
  * drive_frames on a keypoint track.
Every case prints its ratio to the gate (``[stickman]`` lines).  Not measured on an MI355X yet; on the host, the fp32 draw_stickman sits at
3-8 % of the gate and the kernel's arithmetic restated in fp32 torch at 3-4 %."""
import copy
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import stickman_restatement as SR          # noqa: E402
from test_fsth_cpu import plugin, toy_args          # noqa: E402

S_TOY = 32


def loader():
    return plugin('dataloaders', 'synthetic_voxceleb2_stickmen')


def keypoint_sets(n):
    """the three sets of the kernel test, each [n, 68, 2]"""
    mod = loader()
    faces = torch.stack([mod.face_keypoints(torch.Generator().manual_seed(40 + i)) for i in range(n)])
    edge = faces.clone()
    edge[:, 5] = edge[:, 4]; edge[:, 37] = edge[:, 36]          # zero-length segments
    edge[:, 0] = torch.tensor([0.0, 0.0]); edge[:, 16] = torch.tensor([1.0, 1.0]); edge[:, 8] = torch.tensor([0.0, 1.0])          # image corners
    return {'faces': faces, 'degenerate+corners': edge, 'all-equal': torch.full((n, 68, 2), 0.5)}


def keypoints(b, k, seed):
    mod = loader()
    g = torch.Generator().manual_seed(seed)
    return torch.stack([mod.face_keypoints(g) for _ in range(b * k)]).reshape(b, k, 136)


# ---- kernel ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('size,width', [(8, None), (10, None), (22, None), (64, None), (96, None), (96, 1.0), (64, 2.5)])
def test_kernel_vs_fp64_restatement(size, width, n):
    from latent_pose_reenactment_amd import hipops as ops
    mod = loader()
    seg, part_end, colour, _ = ops.stickman_table(mod.PARTS)
    w = max(1.0, size / 64.0) if width is None else width
    gate = 8 * 2.0 ** -23 * size / w
    for name, pts in keypoint_sets(n).items():
        want = SR.render(pts, size, seg, part_end, colour, width)
        host = torch.stack([mod.draw_stickman(p, size, width) for p in pts])
        got = ops.stickman_render(pts.cuda(), size, width)
        flat = ops.stickman_render(pts.reshape(n, 136).cuda(), size, width)
        torch.cuda.synchronize()
        e_host = (host.double() - want).abs().max().item()
        e_dev = (got.cpu().double() - want).abs().max().item()
        print(f'[stickman] S {size} width {w} N {n} {name}: device / gate {e_dev / gate:.3f}, host fp32 / gate {e_host / gate:.3f} (gate {gate:.2e})')
        assert e_host <= gate, (name, e_host, gate)          # the yardstick holds the host's own renderer
        assert tuple(got.shape) == (n, 3, size, size) and got.dtype == torch.float32
        assert e_dev <= gate, (name, e_dev, gate)
        assert torch.equal(got, flat)          # [..., P, 2] and [..., 2P] are one input
        assert want.max() > 0.9 or name == 'all-equal'


# ---- wrapper -----------------------------------------------------------------------------------------------------------------------------------------
def test_out_may_be_a_slice_of_a_larger_tensor_and_bad_inputs_are_refused():
    from latent_pose_reenactment_amd import hipops as ops
    b, k, s = 2, 3, 22
    pts = keypoints(b, k, 7).cuda()
    fresh = ops.stickman_render(pts, s)
    assert tuple(fresh.shape) == (b, k, 3, s, s)
    big = torch.full((b + 1, k, 3, s, s), -1.0, device='cuda')
    ret = ops.stickman_render(pts[1], s, out=big[1])
    assert ret.data_ptr() == big[1].data_ptr()
    assert torch.equal(big[1], fresh[1]) and bool((big[0] == -1).all()) and bool((big[2] == -1).all())          # the neighbours are untouched
    single = ops.stickman_render(pts[0, 0].view(68, 2), s)
    assert tuple(single.shape) == (3, s, s) and torch.equal(single, fresh[0, 0])
    with pytest.raises(ValueError, match='CUDA'):
        ops.stickman_render(pts.cpu(), s)
    with pytest.raises(ValueError, match='fp32'):
        ops.stickman_render(pts.double(), s)
    wide = torch.empty(k, 3, s, 2 * s, device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        ops.stickman_render(pts[0], s, out=wide[..., :s])
    with pytest.raises(ValueError, match='out must be'):
        ops.stickman_render(pts[0], s, out=torch.empty(k, 3, s, s, device='cuda', dtype=torch.float64))
    with pytest.raises(ValueError, match='P >= 68'):
        ops.stickman_render(pts[..., :100], s)
    with pytest.raises(ValueError, match='width'):
        ops.stickman_render(pts, s, width=0.0)


def test_capture_and_replay_on_new_keypoints():
    from latent_pose_reenactment_amd import hipops as ops
    s = 64
    first, second = keypoints(2, 2, 1).cuda(), keypoints(2, 2, 2).cuda()
    static_in = first.clone()
    static_out = torch.zeros(2, 2, 3, s, s, device='cuda')
    ops.stickman_render(static_in, s, out=static_out)          # eager: the polyline table reaches the device outside the capture
    want_first, want_second = ops.stickman_render(first, s), ops.stickman_render(second, s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.stickman_render(static_in, s, out=static_out)
    static_out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_first)
    static_in.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_second) and not torch.equal(want_first, want_second)


# ---- the three consumers, toy geometry, bf16x3 -----------------------------------------------------------------------------------------------------------
def run_embedder(E, state, batch, r):
    E.load_state_dict(state)
    E.zero_grad(set_to_none=True)
    dd = dict(batch)
    E(dd)
    ((dd['embeds'] * r[0]).sum() + (dd['embeds_elemwise'] * r[1]).sum()).backward()
    torch.cuda.synchronize()
    assert set(dd) == set(batch) | {'embeds', 'embeds_elemwise'}          # nothing rendered is left in the batch
    return [dd['embeds'].detach(), dd['embeds_elemwise'].detach()] + [p.grad.clone() for p in E.parameters()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_embedder_renders_from_keypoints(monkeypatch):
    from latent_pose_reenactment_amd import hipops as ops
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    torch.manual_seed(0)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(toy_args(device='cuda')).train()
    state = copy.deepcopy(E.state_dict())
    g = torch.Generator().manual_seed(3)
    rgbs = torch.rand(2, 3, 3, S_TOY, S_TOY, generator=g).cuda()
    r = (torch.randn(2, 8, generator=g).cuda(), torch.randn(2, 3, 8, generator=g).cuda())
    kp, other = keypoints(2, 3, 11).cuda(), keypoints(2, 3, 12).cuda()
    stick, stick_other = ops.stickman_render(kp, S_TOY), ops.stickman_render(other, S_TOY)
    from_kp = run_embedder(E, state, {'enc_rgbs': rgbs, 'enc_keypoints': kp}, r)
    from_stick = run_embedder(E, state, {'enc_rgbs': rgbs, 'enc_stickmen': stick}, r)
    assert all(p.grad is not None for p in E.parameters()) and same(from_kp, from_stick)
    # both keys: the stickmen are used
    both = run_embedder(E, state, {'enc_rgbs': rgbs, 'enc_keypoints': kp, 'enc_stickmen': stick_other}, r)
    from_other = run_embedder(E, state, {'enc_rgbs': rgbs, 'enc_stickmen': stick_other}, r)
    assert same(both, from_other) and not torch.equal(both[0], from_kp[0])
    # two forwards on one dict object, keypoints changed in place between them: the second forward sees the second pose
    E.eval()
    with torch.no_grad():
        dd = {'enc_rgbs': rgbs, 'enc_keypoints': kp.clone()}
        E(dd)
        first = dd['embeds'].clone()
        dd['enc_keypoints'].copy_(other)
        E(dd)
        fresh = {'enc_rgbs': rgbs, 'enc_stickmen': stick_other}
        E(fresh)
        assert torch.equal(dd['embeds'], fresh['embeds']) and not torch.equal(dd['embeds'], first) and 'enc_stickmen' not in dd
        with pytest.raises(KeyError, match='enc_stickmen.*enc_keypoints'):
            E({'enc_rgbs': rgbs})


def test_generator_renders_from_keypoints(monkeypatch):
    from latent_pose_reenactment_amd import hipops as ops
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    torch.manual_seed(0)
    G = plugin('generators', 'FSTH').Wrapper.get_net(toy_args(device='cuda', gen_num_downsample_blocks=3)).train()
    state = copy.deepcopy(G.state_dict())
    g = torch.Generator().manual_seed(4)
    embeds = torch.randn(2, 8, generator=g).cuda()
    kp, other = keypoints(2, 1, 21).cuda(), keypoints(2, 1, 22).cuda()
    stick, stick_other = ops.stickman_render(kp, S_TOY), ops.stickman_render(other, S_TOY)

    def run(batch):
        G.load_state_dict(state)
        dd = dict(batch, embeds=embeds)
        with torch.no_grad():
            G(dd)
        torch.cuda.synchronize()
        assert set(dd) == set(batch) | {'embeds', 'fake_rgbs'}
        return dd['fake_rgbs']
    from_kp = run({'dec_keypoints': kp})
    assert tuple(from_kp.shape) == (2, 3, S_TOY, S_TOY)
    assert torch.equal(from_kp, run({'dec_stickmen': stick}))
    assert torch.equal(from_kp, run({'dec_keypoints': kp.reshape(2, 136)}))          # B x 136: one frame per sample without the frame axis
    both = run({'dec_keypoints': kp, 'dec_stickmen': stick_other})
    assert torch.equal(both, run({'dec_stickmen': stick_other})) and not torch.equal(both, from_kp)
    G.eval()
    with torch.no_grad():
        dd = {'embeds': embeds, 'dec_keypoints': kp.clone()}
        G(dd)
        first = dd['fake_rgbs'].clone()
        dd['dec_keypoints'].copy_(other)
        G(dd)
        fresh = {'embeds': embeds, 'dec_stickmen': stick_other}
        G(fresh)
        assert torch.equal(dd['fake_rgbs'], fresh['fake_rgbs']) and not torch.equal(dd['fake_rgbs'], first) and 'dec_stickmen' not in dd
        with pytest.raises(KeyError, match='dec_stickmen.*dec_keypoints'):
            G({'embeds': embeds})
        G.image_size = None          # a generator built without its frame size says what it lacks
        with pytest.raises(RuntimeError, match='image_size'):
            G({'embeds': embeds, 'dec_keypoints': kp})


@pytest.mark.parametrize('early_real', [False, True])
def test_critic_renders_from_keypoints(monkeypatch, early_real):
    from latent_pose_reenactment_amd import hipops as ops
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    torch.manual_seed(0)
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(toy_args(device='cuda')).train()
    D.keep_reference_waste = True          # the generator-side pass deposits its parameter gradients too
    state = copy.deepcopy(D.state_dict())
    g = torch.Generator().manual_seed(5)
    fake0, real = torch.rand(2, 3, S_TOY, S_TOY, generator=g).cuda(), torch.rand(2, 1, 3, S_TOY, S_TOY, generator=g).cuda()
    label = torch.tensor([1, 3]).cuda()
    kp, other = keypoints(2, 1, 31).cuda(), keypoints(2, 1, 32).cuda()
    stick, stick_other = ops.stickman_render(kp, S_TOY), ops.stickman_render(other, S_TOY)

    def run(batch):
        D.load_state_dict(state)
        D.zero_grad(set_to_none=True)
        fake = fake0.clone().requires_grad_(True)
        dd = dict(batch, fake_rgbs=fake, target_rgbs=real, label=label)
        if early_real:          # the runner's order: weights prepared ahead, the real pass started before the generator has run
            D.prepare_step()
            D.start_real_pass({k: v for k, v in dd.items() if k != 'fake_rgbs'})
        D(dd)
        (dd['fake_score_G'].sum() + 2 * dd['fake_score_D'].sum() + 3 * dd['real_score'].sum()).backward()
        torch.cuda.synchronize()
        assert ('dec_stickmen' in dd) == ('dec_stickmen' in batch)          # nothing rendered is left in the batch
        return ([dd[k].detach() for k in ('fake_score_G', 'fake_score_D', 'real_score')] + [f.detach() for f in dd['fake_features']]
                + [f.detach() for f in dd['real_features']] + [fake.grad.clone()] + [p.grad.clone() for p in D.parameters() if p.grad is not None])
    from_kp = run({'dec_keypoints': kp})
    from_stick = run({'dec_stickmen': stick})
    assert len(from_kp) > 12 and same(from_kp, from_stick)
    both = run({'dec_keypoints': kp, 'dec_stickmen': stick_other})
    assert same(both, run({'dec_stickmen': stick_other})) and not torch.equal(both[0], from_kp[0])
    if early_real:
        return
    D.eval()
    with torch.no_grad():
        dd = {'fake_rgbs': fake0, 'target_rgbs': real, 'label': label, 'dec_keypoints': kp.clone()}
        D(dd)
        first = dd['fake_score_G'].clone()
        dd['dec_keypoints'].copy_(other)
        D(dd)
        fresh = {'fake_rgbs': fake0, 'target_rgbs': real, 'label': label, 'dec_stickmen': stick_other}
        D(fresh)
        assert torch.equal(dd['fake_score_G'], fresh['fake_score_G']) and torch.equal(dd['real_score'], fresh['real_score'])
        assert not torch.equal(dd['fake_score_G'], first) and 'dec_stickmen' not in dd
        with pytest.raises(KeyError, match='dec_stickmen.*dec_keypoints'):
            D({'fake_rgbs': fake0, 'target_rgbs': real, 'label': label})


# ---- driving ------------------------------------------------------------------------------------------------------------------------------------------
def test_drive_frames_on_a_keypoint_track(monkeypatch):
    from latent_pose_reenactment_amd import hipops as ops
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    import drive                      # (the entry script disables autograd globally at import, like the reference's drive.py)
    torch.set_grad_enabled(True)
    torch.manual_seed(0)
    a = toy_args(device='cuda', gen_num_downsample_blocks=3)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a).eval()
    G = plugin('generators', 'FSTH').Wrapper.get_net(a).eval()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        ident = {'enc_rgbs': torch.rand(1, 2, 3, S_TOY, S_TOY, generator=g).cuda(), 'enc_keypoints': keypoints(1, 2, 41).cuda()}
        E(ident)
        G.enable_finetuning({'embeds': ident['embeds']}); E.enable_finetuning()
        track = keypoints(3, 1, 42).cuda()          # a driving sequence: T x 1 x 136
        batch = {'dec_keypoints': track}
        grid = drive.drive_frames(E, G, batch)
        assert tuple(grid.shape) == (3, S_TOY, 2 * S_TOY, 3) and grid.dtype == torch.uint8 and grid.is_cuda
        to_u8 = lambda img: img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()
        assert torch.equal(grid[:, :, :S_TOY], to_u8(ops.stickman_render(track, S_TOY)[:, 0]))
        assert torch.equal(grid[:, :, S_TOY:], to_u8(batch['fake_rgbs'])) and int(grid[:, :, :S_TOY].max()) > 200
        direct = {'dec_stickmen': ops.stickman_render(track, S_TOY)}
        G(direct)
        assert torch.equal(batch['fake_rgbs'], direct['fake_rgbs'])
        # with the driver's image in the batch the left panel is that image, as before
        rgb = torch.rand(3, 1, 3, S_TOY, S_TOY, generator=g).cuda()
        grid2 = drive.drive_frames(E, G, {'dec_keypoints': track, 'pose_input_rgbs': rgb})
        assert torch.equal(grid2[:, :, :S_TOY], to_u8(rgb[:, 0])) and torch.equal(grid2[:, :, S_TOY:], grid[:, :, S_TOY:])
