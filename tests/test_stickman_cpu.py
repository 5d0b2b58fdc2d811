"""CPU checks of the device stickman's host side (no GPU): the polyline table hipops builds from PARTS, the argument checks of lp_stickman_render
(they run before any device work, like the other entry points': tests/test_abi.py), and dataloaders/synthetic_voxceleb2_keypoints.py against
dataloaders/synthetic_voxceleb2_stickmen.py -- the same samples, bit for bit, with the poses left undrawn."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_fsth_cpu import data_args, plugin          # noqa: E402
import stickman_restatement as SR          # noqa: E402


def test_polyline_table_from_parts():
    from latent_pose_reenactment_amd import hipops as ops
    mod = plugin('dataloaders', 'synthetic_voxceleb2_stickmen')
    assert ops.PARTS == mod.PARTS
    seg, part_end, colour, npoints = ops.stickman_table(mod.PARTS)
    assert len(seg) == 63 and len(part_end) == len(colour) == 9 and part_end[-1] == 63 and npoints == 68
    assert all(0 <= i < 68 and 0 <= j < 68 for i, j in seg)
    assert part_end == sorted(part_end) and len(set(part_end)) == 9          # non-empty runs
    start = 0
    for (first, last, closed, rgb), end, col in zip(mod.PARTS, part_end, colour):
        run = [tuple(s) for s in seg[start:end]]
        chain = [(i, i + 1) for i in range(first, last)]
        assert run == chain + ([(last, first)] if closed else []), (first, last, run)
        assert col == list(rgb)
        start = end
    assert [tuple(s) for s in seg].count((41, 36)) == 1 and [tuple(s) for s in seg].count((47, 42)) == 1          # the four closing edges
    assert [tuple(s) for s in seg].count((59, 48)) == 1 and [tuple(s) for s in seg].count((67, 60)) == 1
    assert sum(closed for _, _, closed, _ in mod.PARTS) == 4 and len(seg) == 68 - 9 + 4
    # a custom table goes through the same checks
    assert ops.stickman_table(((0, 2, True, (1, 0, 0)),))[:2] == ([[0, 1], [1, 2], [2, 0]], [3])
    with pytest.raises(ValueError, match='no segment'):
        ops.stickman_table(((3, 3, False, (1, 0, 0)),))
    with pytest.raises(ValueError, match='parts'):
        ops.stickman_table(tuple((i, i + 1, False, (1, 0, 0)) for i in range(17)))


def test_the_restatement_is_the_host_renderer_in_fp64():
    """the fp64 yardstick of the GPU tests and the host's fp32 draw_stickman state the same image (the gate the GPU test applies to both)"""
    from latent_pose_reenactment_amd import hipops as ops
    mod = plugin('dataloaders', 'synthetic_voxceleb2_stickmen')
    seg, part_end, colour, _ = ops.stickman_table(mod.PARTS)
    pts = mod.face_keypoints(torch.Generator().manual_seed(2))
    for size, width in ((10, None), (64, 2.5)):
        want = SR.render(pts, size, seg, part_end, colour, width)
        err = (mod.draw_stickman(pts, size, width).double() - want).abs().max().item()
        assert err <= 8 * 2.0 ** -23 * size / (max(1.0, size / 64.0) if width is None else width), (size, width, err)
        assert want.max() > 0.9 and (want > 0).double().mean() < 0.6


def test_argument_checks_come_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    buf = (ctypes.c_float * 16)()
    ptr = ctypes.addressof(buf)

    def call(points=ptr, N=1, P=68, seg=ptr, part_end=ptr, colour=ptr, L=63, parts=9, S=8, width=1.0, out=ptr):
        return l.lp_stickman_render(points, N, P, seg, part_end, colour, L, parts, S, width, out, None)
    assert l.lp_stickman_render(None, 1, 68, None, None, None, 63, 9, 8, 1.0, None, None) == -1
    assert b'lp_stickman_render' in l.lp_last_error() and b'null' in l.lp_last_error()
    for null in ('points', 'seg', 'part_end', 'colour', 'out'):
        assert call(**{null: None}) == -1 and b'null' in l.lp_last_error(), null
    # host pointers only: every one of these is refused before anything is dereferenced or launched
    for bad in (dict(N=0), dict(N=-3), dict(P=0), dict(P=257), dict(L=0), dict(L=257), dict(parts=0), dict(parts=17), dict(S=0), dict(width=0.0),
                dict(width=-1.0), dict(width=float('nan'))):
        assert call(**bad) == -1, bad
        assert b'lp_stickman_render' in l.lp_last_error(), (bad, l.lp_last_error())


def test_wrapper_refuses_host_tensors_without_a_gpu():
    from latent_pose_reenactment_amd import hipops as ops
    with pytest.raises(ValueError, match='CUDA'):
        ops.stickman_render(torch.rand(68, 2), 16)


def test_stickmen_helper_prefers_the_stickmen_and_names_both_keys():
    from latent_pose_reenactment_amd import fsth
    stick = torch.zeros(1, 1, 3, 8, 8)
    assert fsth.stickmen({'dec_stickmen': stick, 'dec_keypoints': torch.rand(1, 1, 136)}, 'dec', 8) is stick          # no launch, no GPU needed
    with pytest.raises(KeyError, match='enc_stickmen.*enc_keypoints'):
        fsth.stickmen({'dec_stickmen': stick}, 'enc', 8)
    with pytest.raises(ValueError):
        fsth.stickmen({}, 'pose', 8)


@pytest.mark.parametrize('seed,index,finetune', [(5, 2, False), (5, 0, True), (11, 3, False), (0, 5, False)])
def test_keypoint_loader_is_the_stickmen_loader_undrawn(seed, index, finetune):
    base = plugin('dataloaders', 'synthetic_voxceleb2')
    sm = plugin('dataloaders', 'synthetic_voxceleb2_stickmen')
    kp = plugin('dataloaders', 'synthetic_voxceleb2_keypoints')
    a = data_args(random_seed=seed, finetune=finetune, image_size=32)
    for part in ('train', 'val'):
        bdata, btarget = base.Dataset.get_dataset(a, part)[index]
        sdata, starget = sm.Dataset.get_dataset(a, part)[index]
        kdata, ktarget = kp.Dataset.get_dataset(a, part)[index]
        k = 1 if finetune else 3
        assert set(kdata) == set(bdata) | {'enc_keypoints', 'dec_keypoints'} and 'enc_stickmen' not in kdata and 'dec_stickmen' not in kdata
        assert tuple(kdata['enc_keypoints'].shape) == (k, 136) and tuple(kdata['dec_keypoints'].shape) == (1, 136)
        assert kdata['enc_keypoints'].dtype == kdata['dec_keypoints'].dtype == torch.float32
        for key in bdata:          # every key of synthetic_voxceleb2, in both loaders
            assert torch.equal(kdata[key], bdata[key]) and torch.equal(sdata[key], bdata[key]), key
        assert torch.equal(ktarget['real_segm'], btarget['real_segm']) and ktarget['label'] == btarget['label'] == starget['label']
        assert torch.equal(kdata['dec_keypoints'], sdata['dec_keypoints'])
        for f in range(k):          # the stickmen loader draws exactly these keypoints
            assert torch.equal(sm.draw_stickman(kdata['enc_keypoints'][f].view(68, 2), 32), sdata['enc_stickmen'][f]), f
        assert torch.equal(sm.draw_stickman(kdata['dec_keypoints'][0].view(68, 2), 32), sdata['dec_stickmen'][0])
    assert len(kp.Dataset.get_dataset(a, 'train')) == len(sm.Dataset.get_dataset(a, 'train'))


def test_keypoint_loader_through_the_dataloader_plugin_interface():
    kp = plugin('dataloaders', 'synthetic_voxceleb2_keypoints')
    ds = kp.Dataset.get_dataset(data_args(), 'train')
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert tuple(batch[0]['enc_keypoints'].shape) == (2, 3, 136) and tuple(batch[0]['dec_keypoints'].shape) == (2, 1, 136)
