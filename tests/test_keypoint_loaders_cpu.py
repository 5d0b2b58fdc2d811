"""The keypoint loaders (``--dataloader voxceleb2`` and ``--dataloader voxceleb2_FSTH_crop``) on the CPU route, on the temporary tree of
tests/keypoint_tree.py (JPEG frames of 20 x 20, 32 x 32 and 24 x 32, landmark files of 68 x 2 and 68 x 3): the contract in the meta-training and
``--finetune`` forms with ``--inference`` on and off, ``dec_keypoints`` against the formulas in float64, the boxes as stated integers (and the
reference's own cut within one pixel of them), the table rows, the images against ``frames.prepare_host`` on the same bytes, the stickmen against
the integer restatement with exact equality, the refusals, determinism of ``part='val'`` and independence of the number of workers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoint_tree as KT          # noqa: E402
import stickman_hard_restatement as HR          # noqa: E402
from keypoint_tree import K, SIZE          # noqa: E402

CONTRACT = {'enc_rgbs', 'enc_stickmen', 'target_rgbs', 'pose_input_rgbs', 'dec_stickmen', 'dec_keypoints'}


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return KT.build_tree(tmp_path_factory.mktemp('voxceleb2_keypoints'))


def parts_of(oval=True):
    from latent_pose_reenactment_amd import hipops
    return hipops.REFERENCE_PARTS if oval else hipops.REFERENCE_PARTS_NO_OVAL


def same_batches(a, b):
    assert len(a) == len(b)
    for (da, ta), (db, tb) in zip(a, b):
        assert set(da) == set(db) and all(torch.equal(da[k], db[k]) for k in da) and torch.equal(ta['label'], tb['label'])


@pytest.mark.parametrize('inference', [False, True])
@pytest.mark.parametrize('plugin', KT.PLUGINS)
def test_meta_training_contract_and_values(tree, plugin, inference):
    split = 'square.csv' if plugin == 'voxceleb2' else 'all.csv'
    videos = KT.SQUARE if plugin == 'voxceleb2' else tuple(KT.VIDEOS)
    # (under --inference an augmentation flag that is on is ignored, as in the reference)
    loader = KT.loader_for(plugin, KT.make_args(tree, split, inference=inference, use_affine_scale=inference))
    batches = list(loader)
    assert len(batches) == len(loader) == (len(videos) + 1) // 2 and len(loader.dataset) == len(videos)
    seen = 0
    for data, target in batches:
        b = target['label'].shape[0]
        assert set(data) == CONTRACT and set(target) == {'label'} and target['label'].dtype == torch.int64
        shapes = {key: tuple(v.shape) for key, v in data.items()}
        assert shapes == {'enc_rgbs': (b, K, 3, SIZE, SIZE), 'enc_stickmen': (b, K, 3, SIZE, SIZE), 'target_rgbs': (b, 1, 3, SIZE, SIZE),
                          'pose_input_rgbs': (b, 1, 3, SIZE, SIZE), 'dec_stickmen': (b, 1, 3, SIZE, SIZE), 'dec_keypoints': (b, 1, 136)}
        assert all(v.dtype == torch.float32 and v.is_contiguous() for v in data.values())
        assert torch.equal(data['target_rgbs'], data['pose_input_rgbs'])          # the same image
        assert target['label'].tolist() == list(range(seen, seen + b))          # the dataframe's index
        for s in range(b):
            video = videos[seen + s]
            ids = KT.sampled(tree, video)
            for k, name in enumerate(ids):
                image = data['enc_rgbs'][s, k] if k < K else data['target_rgbs'][s, 0]
                stick = data['enc_stickmen'][s, k] if k < K else data['dec_stickmen'][s, 0]
                assert torch.equal(image, KT.host_image(tree, plugin, video, name)), (video, name)
                kp = torch.from_numpy(KT.keypoints64(tree, plugin, video, name).astype(np.float32))
                assert torch.equal(stick, HR.render(kp, SIZE, parts_of(), 2)), (video, name)
                assert float(stick.max()) == 1.0
                if k == K:
                    assert torch.equal(data['dec_keypoints'][s, 0], kp)
        seen += b
    assert seen == len(videos)


@pytest.mark.parametrize('inference', [False, True])
@pytest.mark.parametrize('plugin', KT.PLUGINS)
def test_finetune_serves_the_one_image_under_both_names(tree, plugin, inference):
    video = 'id00/vidB' if plugin == 'voxceleb2' else 'id02/vidA'          # (the crop plugin: the 24 x 32 video)
    args = KT.make_args(tree, finetune=True, inference=inference, val_split_path=KT.Path(video), batch_size=3)
    loader = KT.loader_for(plugin, args)
    assert args.num_labels == 1 and len(loader.dataset) == len(KT.NAMES)
    batches = list(loader)
    assert [t['label'].tolist() for _, t in batches] == [[0, 0, 0], [0]]
    names = iter(KT.NAMES)
    for data, target in batches:
        b = target['label'].shape[0]
        assert set(data) == CONTRACT and all(v.dtype == torch.float32 for v in data.values())
        assert all(tuple(data[key].shape) == (b, 1, 3, SIZE, SIZE) for key in CONTRACT - {'dec_keypoints'}) and tuple(data['dec_keypoints'].shape) == (b, 1, 136)
        assert torch.equal(data['enc_rgbs'], data['target_rgbs']) and torch.equal(data['enc_rgbs'], data['pose_input_rgbs'])
        assert torch.equal(data['enc_stickmen'], data['dec_stickmen'])
        for s in range(b):
            name = next(names)
            kp = torch.from_numpy(KT.keypoints64(tree, plugin, video, name).astype(np.float32))
            assert torch.equal(data['dec_keypoints'][s, 0], kp)
            assert torch.equal(data['enc_rgbs'][s, 0], KT.host_image(tree, plugin, video, name))
            assert torch.equal(data['dec_stickmen'][s, 0], HR.render(kp, SIZE, parts_of(), 2))


def test_the_square_crop_box_and_the_reference_cut():
    from latent_pose_reenactment_amd.dataloaders import voxceleb2_FSTH_crop as crop
    stated = {20: (4, 2, 16), 32: (6, 3, 26), 224: (45, 22, 179), 256: (51, 25, 205)}
    for side, (t, l, n) in stated.items():
        assert crop.crop_box(side, side) == (t, l, n) == KT.box('voxceleb2_FSTH_crop', side, side)
        assert abs(KT.reference_cut_width(side) - n) <= 1, (side, KT.reference_cut_width(side), n)          # the documented deviation
        assert 0 <= l and l + n <= side and t + n == side
    assert KT.reference_cut_width(256) == 204          # (the README's example)
    assert crop.crop_box(24, 32) == (5, 6, 19) and crop.crop_box(32, 24) == (6, -1, 26)          # the second leaves its frame: the border rule


@pytest.mark.parametrize('plugin', KT.PLUGINS)
def test_table_rows_and_raw_batch(tree, plugin):
    from latent_pose_reenactment_amd import frames
    split = 'square.csv' if plugin == 'voxceleb2' else 'all.csv'
    loader = KT.loader_for(plugin, KT.make_args(tree, split))
    raw = next(iter(loader.loader))
    b = raw['label'].shape[0]
    assert raw['buf'].dtype == torch.uint8 and raw['table'].dtype == torch.int64 and tuple(raw['table'].shape) == (b * (K + 1), frames.NCOLS)
    assert frames.check_table(raw['table'], raw['buf'].numel(), SIZE) == (b * (K + 1), 0, 0)          # images only: no mask, no product
    assert raw['keypoints'].dtype == torch.float32 and tuple(raw['keypoints'].shape) == (b * (K + 1), 136) and raw['frames'] == K
    col = {name: c for c, name in enumerate(frames.COLUMNS)}
    videos = KT.SQUARE if plugin == 'voxceleb2' else tuple(KT.VIDEOS)
    offset = 0
    for s in range(b):
        h, w, _ = KT.VIDEOS[videos[s]]
        t, l, n = KT.box(plugin, h, w)
        for k, name in enumerate(KT.sampled(tree, videos[s])):
            slot = s * K + k if k < K else b * K + s
            row = raw['table'][(raw['table'][:, col['image_slot']] == slot).nonzero().item()].tolist()
            assert row[:10] == [offset, h, w, 3 * w, 3, t, l, t + n, l + n, frames.mode_for(n, SIZE)], (s, k)          # the whole frame is the view
            assert torch.equal(raw['buf'][offset:offset + h * w * 3], torch.from_numpy(KT.decode(tree, videos[s], name)).reshape(-1))
            assert torch.equal(raw['keypoints'][slot], torch.from_numpy(KT.keypoints64(tree, plugin, videos[s], name).astype(np.float32)))
            offset += h * w * 3
    assert offset == raw['buf'].numel()


def test_refusals_name_the_file_or_the_flag(tree):
    with pytest.raises(ValueError, match=r'id02/vidA/0000\d.*24 x 32.*square'):          # a frame that is not square under `voxceleb2`
        list(KT.loader_for('voxceleb2', KT.make_args(tree, 'all.csv', batch_size=5)))
    for plugin in KT.PLUGINS:
        with pytest.raises(ValueError, match=r'short/landmarks/id09/vidA/0000\d\.npy.*\(60, 2\).*68'):          # a 60-row landmark file
            list(KT.loader_for(plugin, KT.make_args(tree / 'short', 'short.csv')))
        for flag in ('use_pixelwise_augs', 'use_affine_scale', 'use_affine_shift'):
            with pytest.raises(NotImplementedError, match=f'Keypoints augmentation is NYI.*{flag}'):
                KT.loader_for(plugin, KT.make_args(tree, **{flag: True}))
        with pytest.raises(ValueError, match='stickman_thickness'):
            KT.loader_for(plugin, KT.make_args(tree, stickman_thickness=9))


@pytest.mark.parametrize('plugin', KT.PLUGINS)
def test_val_is_deterministic_and_workers_do_not_change_batches(tree, plugin):
    loader = KT.loader_for(plugin, KT.make_args(tree))
    first = list(loader)
    same_batches(first, list(loader))          # two iterations over part='val'
    same_batches(first, list(KT.loader_for(plugin, KT.make_args(tree, num_workers=2))))
    train = list(KT.loader_for(plugin, KT.make_args(tree), part='train'))          # shuffled, random frames: the contract alone
    assert len(train) == 2 and all(set(d) == CONTRACT for d, _ in train)


def test_oval_and_thickness_reach_the_stickmen(tree):
    plain = next(iter(KT.loader_for('voxceleb2', KT.make_args(tree))))[0]
    bare = next(iter(KT.loader_for('voxceleb2', KT.make_args(tree, draw_oval=False, stickman_thickness=3))))[0]
    kp = plain['dec_keypoints']
    assert torch.equal(bare['dec_keypoints'], kp)
    assert torch.equal(bare['dec_stickmen'], HR.render(kp, SIZE, parts_of(False), 3)) and not torch.equal(bare['dec_stickmen'], plain['dec_stickmen'])


def test_flags_are_the_references_plus_two():
    class Parser:
        def __init__(self):
            self.flags = {}

        def add(self, name, **kw):
            self.flags[name] = kw
    for plugin in KT.PLUGINS:
        import importlib
        p = importlib.import_module(f'dataloaders.{plugin}').Dataset.get_args(Parser())
        assert {'--data_root', '--img_dir', '--kp_dir', '--draw_oval', '--n_frames_for_encoder', '--use_pixelwise_augs', '--use_affine_scale',
                '--use_affine_shift', '--num_labels', '--stickman_thickness'} <= set(p.flags)
        assert p.flags['--stickman_thickness']['default'] == 2 and p.flags['--draw_oval']['default'] is True
        assert '--blur_padded_bands' not in p.flags and '--decode_jpeg_on_gpu' not in p.flags and '--segm_dir' not in p.flags
