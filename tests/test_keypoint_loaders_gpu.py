"""The keypoint loaders on the GPU (``--device cuda``: one lp_frames_prepare launch and one lp_stickman_render_hard launch per batch) on the temporary
tree of tests/keypoint_tree.py:
  * both loaders against their CPU route, meta-training and fine-tuning: the images per sample under that sample's gate (frames_restatement.gate, the
    gate of tests/test_frames_gpu.py's loader comparison; the worst fraction is printed), stickmen and keypoints exactly equal;
  * training from ``voxceleb2_FSTH_crop`` at the geometry of tests/test_fsth_full_gpu.py (256 x 256, widths 64 .. 512, 6 embedder / 7 critic blocks,
    2 samples x 4 encoder frames), embedder FSTH + discriminator FSTH with the generators FSTH_plus and FSTH: two eager iterations with finite
    losses; and the captured step (``--hip_graph``: runners.holycow.GraphedTrainStep) replayed on the SECOND batch against the eager step on that
    batch -- ``fake_rgbs`` within 1e-4 rel-L2, the tolerance of tests/test_train_step.py::test_hipgraph_replay_equals_eager, whose optimizer
    (RAdam) and operand mode (bf16x3) the comparison takes as well;
  * ``drive.drive_frames`` on an inference batch of each loader, with both generators."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoint_tree as KT          # noqa: E402
import frames_restatement as FR          # noqa: E402
from test_fsth_cpu import plugin, toy_args          # noqa: E402

pytestmark = pytest.mark.gpu
GENERATORS = ('FSTH_plus', 'FSTH')


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return KT.build_tree(tmp_path_factory.mktemp('voxceleb2_keypoints_gpu'))


@pytest.mark.parametrize('plugin_name', KT.PLUGINS)
def test_loader_on_the_device_equals_its_cpu_route(tree, plugin_name):
    split = 'square.csv' if plugin_name == 'voxceleb2' else 'all.csv'
    videos = KT.SQUARE if plugin_name == 'voxceleb2' else tuple(KT.VIDEOS)
    one = 'id00/vidB' if plugin_name == 'voxceleb2' else 'id02/vidA'
    for flags, paths in ((dict(split=split), videos), (dict(finetune=True, val_split_path=KT.Path(one), batch_size=4), [one] * 4)):
        device = list(KT.loader_for(plugin_name, KT.make_args(tree, device='cuda', **flags)))
        host = list(KT.loader_for(plugin_name, KT.make_args(tree, device='cpu', **flags)))
        assert len(device) == len(host) >= 1
        s, worst = 0, 0.0
        for (dd, dt), (hd, ht) in zip(device, host):
            assert set(dd) == set(hd) and set(dt) == set(ht) == {'label'} and torch.equal(dt['label'].cpu(), ht['label'])
            for key in hd:
                assert dd[key].is_cuda and dd[key].is_contiguous() and dd[key].shape == hd[key].shape and dd[key].dtype == torch.float32, key
            for key in ('enc_stickmen', 'dec_stickmen', 'dec_keypoints'):
                assert torch.equal(dd[key].cpu(), hd[key]), key          # exactly equal
            # the stickmen of a batch are views of ONE buffer, filled by one launch
            assert dd['enc_stickmen'].untyped_storage().data_ptr() == dd['dec_stickmen'].untyped_storage().data_ptr()
            assert dd['target_rgbs'].data_ptr() == dd['pose_input_rgbs'].data_ptr()
            for b in range(hd['enc_rgbs'].shape[0]):
                h, w, _ = KT.VIDEOS[paths[s]]
                n = KT.box(plugin_name, h, w)[2]
                gate = FR.gate(n, KT.SIZE, FR.mode_for(n, KT.SIZE))
                for key in ('enc_rgbs', 'pose_input_rgbs', 'target_rgbs'):
                    err = (dd[key][b].cpu().double() - hd[key][b].double()).abs().max().item()
                    worst = max(worst, err / gate)
                    assert err <= gate, (paths[s], key, err, gate)
                s += 1
        print(f'[keypoint loaders] {plugin_name} on the device vs its CPU route ({"fine-tuning" if "finetune" in flags else "meta-training"}): '
              f'images worst difference / gate {worst:.2f}; stickmen and keypoints equal')


# ---- training at the geometry of tests/test_fsth_full_gpu.py ---------------------------------------------------------------------------------------------
def full_args(**kw):
    return toy_args(image_size=256, num_channels=64, max_num_channels=512, embed_channels=512, embed_num_blocks=6, dis_num_blocks=7, num_labels=100,
                    device='cuda', pose_embedding_size=136, gen_num_downsample_blocks=4, gen_num_residual_blocks=2, lr_gen=5e-4, lr_dis=8e-4,
                    beta1=0.0, finetune=False, num_gpus=1, **kw)


def build(generator, optimizer):
    from criterions import adversarial, featmat
    from runners import holycow
    a = full_args(optimizer=optimizer)
    torch.manual_seed(0)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a)
    G = plugin('generators', generator).Wrapper.get_net(a)
    D = plugin('discriminators', 'FSTH').Wrapper.get_net(a)
    crits = [adversarial.Criterion('gan'), featmat.Criterion(10.0), plugin('criterions', 'l1_rgb').Criterion(30.0)]
    tm = holycow.TrainingModule(E, G, D, crits, [], {})
    opt_G = holycow.get_optimizer(E, G, a)
    opt_D = plugin('discriminators', 'FSTH').Wrapper.get_optimizer(D, a)
    tm.train()
    return tm, opt_G, opt_D, a, holycow


def two_batches(tree):
    loader = KT.loader_for('voxceleb2_FSTH_crop', KT.make_args(tree, 'all.csv', device='cuda', image_size=256, n_frames_for_encoder=4, batch_size=2))
    batches = list(loader)[:2]
    assert all(tuple(d['enc_stickmen'].shape) == (2, 4, 3, 256, 256) and tuple(d['dec_keypoints'].shape) == (2, 1, 136) for d, _ in batches)
    assert not torch.equal(batches[0][0]['dec_stickmen'], batches[1][0]['dec_stickmen'])
    return batches


def finite(losses):
    return all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in losses.values())


@pytest.mark.parametrize('generator', GENERATORS)
def test_two_eager_training_iterations_from_the_crop_loader(tree, generator, monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    tm, opt_G, opt_D, a, holycow = build(generator, 'Adam')
    for data, target in two_batches(tree):
        all_data, lG, lD = holycow.train_step(tm, dict(data), dict(target), opt_G, opt_D, a)
        torch.cuda.synchronize()
        assert set(lG) == {'adversarial_G', 'feature_matching', 'l1_rgb'} and set(lD) == {'adversarial_D'}
        assert finite(lG) and finite(lD), (lG, lD)
        assert tuple(all_data['fake_rgbs'].shape) == (2, 3, 256, 256) and bool(torch.isfinite(all_data['fake_rgbs']).all())
        print(f'[keypoint loaders] eager step, generator {generator}: ' + ', '.join(f'{k} {float(v):.4g}' for k, v in {**lG, **lD}.items()))


@pytest.mark.parametrize('generator', GENERATORS)
def test_captured_step_replays_with_the_second_batchs_stickmen(tree, generator, monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    (d1, t1), (d2, t2) = two_batches(tree)
    ta, oGa, oDa, a, holycow = build(generator, 'RAdam')
    tb, oGb, oDb, _, _ = build(generator, 'RAdam')
    for _ in range(3):
        holycow.train_step(ta, dict(d1), dict(t1), oGa, oDa, a)
    eager, lG, lD = holycow.train_step(ta, dict(d2), dict(t2), oGa, oDa, a)
    want = eager['fake_rgbs'].detach().clone()
    graphed = holycow.GraphedTrainStep(tb, oGb, oDb, a, dict(d1), dict(t1), warmup_steps=3)
    graphed.load_batch(d2, t2)
    graphed()
    torch.cuda.synchronize()
    for key in ('enc_stickmen', 'dec_stickmen', 'dec_keypoints', 'enc_rgbs', 'target_rgbs'):
        assert torch.equal(graphed.data[key], d2[key]) and not torch.equal(graphed.data[key], d1[key]), key
    got = graphed.all_data['fake_rgbs']
    err = ((got.double() - want.double()).norm() / want.double().norm()).item()
    print(f'[keypoint loaders] captured step on the second batch vs eager, generator {generator}: fake_rgbs rel-L2 {err:.2e} (gate 1e-4)')
    assert finite(graphed.losses_G) and finite(graphed.losses_D) and finite(lG) and finite(lD)
    assert err < 1e-4, err


# ---- driving -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('generator', GENERATORS)
@pytest.mark.parametrize('plugin_name', KT.PLUGINS)
def test_drive_frames_on_an_inference_batch(tree, plugin_name, generator, monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    monkeypatch.delenv('LP_PREC_G', raising=False)
    import drive                      # (the entry script disables autograd globally at import, like the reference's drive.py)
    torch.set_grad_enabled(True)
    s = 32
    video = 'id00/vidB' if plugin_name == 'voxceleb2' else 'id02/vidA'
    # what drive.py builds from a checkpoint's args: finetune = inference = True
    loader = KT.loader_for(plugin_name, KT.make_args(tree, finetune=True, inference=True, val_split_path=KT.Path(video), batch_size=3, image_size=s,
                                                     device='cuda'))
    batch, _ = next(iter(loader))
    torch.manual_seed(0)
    a = toy_args(device='cuda', pose_embedding_size=136, gen_num_downsample_blocks=3)
    E = plugin('embedders', 'FSTH').Wrapper.get_net(a).eval()
    G = plugin('generators', generator).Wrapper.get_net(a).eval()
    with torch.no_grad():
        ident = {'enc_rgbs': batch['enc_rgbs'][:1], 'enc_stickmen': batch['enc_stickmen'][:1]}
        E(ident)
        G.enable_finetuning({'embeds': ident['embeds']}); E.enable_finetuning()
        batch = copy.copy(batch)
        grid = drive.drive_frames(E, G, batch)
        assert tuple(grid.shape) == (3, s, 2 * s, 3) and grid.dtype == torch.uint8 and grid.is_cuda
        to_u8 = lambda img: img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()
        assert torch.equal(grid[:, :, :s], to_u8(batch['pose_input_rgbs'][:, 0])) and torch.equal(grid[:, :, s:], to_u8(batch['fake_rgbs']))
        assert tuple(batch['fake_rgbs'].shape) == (3, 3, s, s) and bool(torch.isfinite(batch['fake_rgbs']).all())
