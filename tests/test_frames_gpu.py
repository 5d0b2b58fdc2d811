"""lp_frames_prepare on the MI355X (``hipops.frames_prepare``: one launch from the packed uint8 frames of a batch to image, mask and product) against
the fp64 restatement (tests/frames_restatement.py) on the case list of tests/test_frames_cpu.py, the bit-exact properties of the definition, the
wrapper's refusals, and the loader end to end: ``Dataloader('voxceleb2_segmentation_nolandmarks')`` on the device against ``frames.prepare_host``,
one train.py iteration on a tree of image folders, and ``drive.drive_frames`` on an ``--inference`` batch.

Gate (frames_restatement.gate): per element (n_y + n_x + 8) 2^-24 W -- see tests/test_frames_cpu.py.  Case list: S in {8, 16, 20, 64} (tile tails,
S % 4 != 0, several tiles); 16 -> 16 and 20 -> 20 (exact), 32 -> 16 and 48 -> 16 (integer area), 37 -> 16, 45 -> 20, 127 -> 16 and 130 -> 64 (fractional,
scale near 8), 11 -> 16, 5 -> 8, 1 -> 8, 63 -> 64 (cubic); boxes out on each single side and on all four; a 3 x 3 view with the box 5 pixels out; mask
rows with the top band and each replicated side; strided views (border removed, channel 1 of 3, a one-channel frame); all of them mixed in one call.
Measured on the MI355X, worst error / gate: area 0.14, cubic 0.15, linear 0.14, product 0.06; the loader on the device against
``prepare_host``: 0.21."""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for _p in (PKG, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import frames_restatement as FR          # noqa: E402
from test_frames_cpu import FRAMES, call, check_against_restatement, check_exact_copy, check_refusals          # noqa: E402
from test_voxceleb2_loader_cpu import PATHS, build_tree, loader_for, make_args, tolerance, video_split          # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


@pytest.mark.parametrize('size', [8, 16, 20, 64])
def test_kernel_against_the_restatement(ops, size):
    worst = check_against_restatement(ops.frames_prepare, size, device='cuda')
    print(f'[frames] lp_frames_prepare, S {size}: worst error / gate ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))


def test_copy_is_exact_and_refusals_name_the_cause(ops):
    check_exact_copy(ops.frames_prepare, device='cuda')
    check_refusals(ops.frames_prepare, device='cuda')
    with pytest.raises(ValueError, match='CUDA'):
        ops.frames_prepare(torch.from_numpy(FRAMES.buf), torch.tensor(call(16)[1], dtype=torch.int64), 16)


@pytest.mark.parametrize('size', [16, 20])
def test_product_is_exact_and_a_row_alone_gives_the_same_bits(ops, size):
    _, rows = call(size)
    buf = torch.from_numpy(FRAMES.buf).cuda()
    table = torch.tensor(rows, dtype=torch.int64)
    image, mask, product = ops.frames_prepare(buf, table, size)
    again = ops.frames_prepare(buf, table, size)
    for a, b in zip((image, mask, product), again):
        assert torch.equal(a, b)                                                                 # bit-identical from run to run
    assert torch.equal(mask[:, 0], mask[:, 1]) and torch.equal(mask[:, 0], mask[:, 2])
    for r in rows:
        if r[FR.PRODUCT_SLOT] >= 0:
            assert torch.equal(product[r[FR.PRODUCT_SLOT]], image[r[FR.IMAGE_SLOT]] * mask[r[FR.MASK_SLOT]])
        # the same row in a table of its own (another footprint bound, another grid): the same bits
        alone = FR.row(r[FR.IMG_OFF:FR.IMG_MODE + 1] if r[FR.IMG_H] else None, r[FR.MSK_OFF:FR.MSK_R + 1] if r[FR.MSK_H] else None,
                       *(0 if r[c] >= 0 else -1 for c in (FR.IMAGE_SLOT, FR.MASK_SLOT, FR.PRODUCT_SLOT)))
        one = ops.frames_prepare(buf, torch.tensor([alone], dtype=torch.int64), size)
        for o, (col, full) in enumerate(((FR.IMAGE_SLOT, image), (FR.MASK_SLOT, mask), (FR.PRODUCT_SLOT, product))):
            if r[col] >= 0:
                assert torch.equal(one[o][0], full[r[col]])


# ---- the loader, end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return build_tree(tmp_path_factory.mktemp('voxceleb2_gpu'))


def test_loader_on_the_device_equals_prepare_host(tree):
    """the same raw batches through the launch and through the fp32 host definition: meta-training (image, mask, product) and fine-tuning with the
    bounding-box file; per sample under that sample's gate"""
    split = video_split(tree)
    for flags, paths in ((dict(val_split_path=split), PATHS), (dict(finetune=True, val_split_path=Path('id02/vidA'), batch_size=5), ['id02/vidA'] * 5)):
        device = list(loader_for(make_args(tree, device='cuda', **flags), 'val'))
        host = list(loader_for(make_args(tree, device='cpu', **flags), 'val'))
        assert len(device) == len(host) >= 1
        s, worst = 0, 0.0
        for (dd, dt), (hd, ht) in zip(device, host):
            assert set(dd) == set(hd) and set(dt) == set(ht) and torch.equal(dt['label'].cpu(), ht['label'])
            for key in ('enc_rgbs', 'pose_input_rgbs', 'target_rgbs'):
                assert dd[key].is_cuda and dd[key].is_contiguous() and dd[key].shape == hd[key].shape
            assert torch.equal(dd['target_rgbs'], dd['pose_input_rgbs'] * dt['real_segm'])
            for b in range(hd['enc_rgbs'].shape[0]):
                g_img, g_msk, g_prod = tolerance(paths[s])
                for got, want, gate in ((dd['enc_rgbs'], hd['enc_rgbs'], g_img), (dd['pose_input_rgbs'], hd['pose_input_rgbs'], g_img),
                                        (dt['real_segm'], ht['real_segm'], g_msk), (dd['target_rgbs'], hd['target_rgbs'], g_prod)):
                    err = (got[b].cpu().double() - want[b].double()).abs().max().item()
                    worst = max(worst, err / gate)
                    assert err <= gate, (paths[s], err, gate)
                s += 1
        print(f'[frames] loader on the device vs prepare_host ({"fine-tuning" if "finetune" in flags else "meta-training"}): worst difference / gate {worst:.2f}')


def test_one_training_iteration_on_image_folders(tree, tmp_path):
    """train.py on the tree, at the smallest geometry tests/test_train_entry_gpu.py trains (128 px, 4 samples x 2 encoder frames): 6 videos, batch 4,
    drop_last -> one iteration, which must finish with finite losses"""
    from test_train_entry_gpu import COMMON
    common = list(COMMON)
    for flag in ('--dataloader', '--synthetic_dataset_len'):
        at = common.index(flag)
        del common[at:at + 2]
    cmd = [sys.executable, os.path.join(PKG, 'train.py')] + common + [
        '--dataloader', 'voxceleb2_segmentation_nolandmarks', '--data_root', str(tree), '--train_split_path', str(video_split(tree)),
        '--bboxes_dir', str(tree / 'bboxes.npy'), '--num_workers', '0', '--use_affine_shift', '--experiments_dir', str(tmp_path),
        '--experiment_name', 'folders', '--log_frequency_loss', '1']
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / 'folders' / 'checkpoints')) == ['model_00000001.pth']
    line = [l for l in r.stdout.splitlines() if 'Epoch 0 (iteration' in l][-1]
    losses = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Loss_\w+) ([-+.\deE]+|nan|inf) \(avg', line)}
    print(f'[frames] train.py on image folders, one iteration: {losses}')
    assert len(losses) >= 5 and all(math.isfinite(v) for v in losses.values()), losses


def test_drive_frames_on_an_inference_batch(tree, monkeypatch):
    monkeypatch.setenv('LP_PREC', 'bf16x3')
    import tiny_embedder
    tiny_embedder.register()
    import drive                      # (the entry script disables autograd globally at import, like the reference's drive.py)
    torch.set_grad_enabled(True)
    with torch.no_grad():
        E, G, saved_args = drive.load_for_inference(os.path.join(ROOT, 'tests', 'golden', 'reference_checkpoint_small.pth'), tree, 'cuda:0')
        for key, value in vars(make_args(tree, finetune=True, inference=True, val_split_path=Path('id01/vidB'), batch_size=2, device='cuda:0')).items():
            if key not in ('image_size', 'num_labels'):
                setattr(saved_args, key, value)
        batches = list(loader_for(saved_args, 'val'))
        size = saved_args.image_size
        assert [b[0]['pose_input_rgbs'].shape[0] for b in batches] == [2, 2, 1]
        data, _ = batches[0]
        assert set(data) == {'enc_rgbs', 'pose_input_rgbs'} and data['pose_input_rgbs'].is_cuda
        grid = drive.drive_frames(E, G, data)
        assert tuple(grid.shape) == (2, size, 2 * size, 3) and grid.dtype == torch.uint8
        to_u8 = lambda img: img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()
        assert torch.equal(grid[:, :, :size], to_u8(data['pose_input_rgbs'][:, 0])) and int(grid[:, :, :size].max()) > 100
