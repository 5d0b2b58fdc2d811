"""lp_frames_pad on the MI355X (``hipops.frames_pad``: the padded, blurred, faded crops of a batch's out-of-frame boxes, written as dense uint8 images
into the workspace behind the packed frames) against the fp64 restatement (tests/frames_pad_restatement.py) on the case list of
tests/test_frames_pad_cpu.py under the rule derived there: uint8 values EXACTLY equal, except where the fp64 value before the rounding lies within
tau = (2 k + 32) 2^-24 255 of a half-integer (flagged; may differ by 1; at most 2 % of a case).  Then the bit-exact properties -- all cases mixed in
one call against each case alone, two runs, the guard bytes before, between and behind the workspace images, the packed head -- and the loader end to
end: ``frames.prepare`` with the flag on the device against ``prepare_host`` with the flag, and one train.py iteration with ``--blur_padded_bands``.

Measured on the MI355X (``-s`` prints every case): no value differs outside the flagged ones (0 mismatches in all 40 cases); the worst flagged
share is 1.948 % (150 / 200 / 10 / -60 as a mask: the replicated edge of the disc fading over a 60-pixel band passes many exact half-integers), then
1.110 % (100 / 127 / -9 / -20 mask) and 0.854 % (40 / 64 / -10 / -12 mask); every image case is under 0.17 %; of the flagged values at most 102 of a
case differ, by 1.  ``frames.prepare`` with the flag on the device against ``prepare_host`` with the flag: worst difference 0.21 of the bound,
meta-training and fine-tuning alike."""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for _p in (PKG, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import frames_restatement as FR          # noqa: E402
import frames_pad_restatement as FP      # noqa: E402
from test_frames_pad_cpu import CASES, KINDS, SIZE, case, compare, extra_tolerance, workspace_of          # noqa: E402
from test_voxceleb2_loader_cpu import K, PATHS, build_tree, loader_for, make_args, tolerance, video_split          # noqa: E402
from test_voxceleb2_loader_cpu import SIZE as LOADER_SIZE          # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope='module')
def ops():
    from latent_pose_reenactment_amd import hipops
    return hipops


def device_pad(ops, buf, rows):
    """-> (the whole device buffer after the launches, as numpy: head, workspace, GUARD bytes behind it; plan; rewritten table)"""
    from latent_pose_reenactment_amd import frames
    table2, plan, weights, total = frames.pad_plan(torch.tensor(rows, dtype=torch.int64), buf.size, SIZE)
    dev = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device='cuda')
    dev[:buf.size] = torch.from_numpy(buf).cuda()
    assert ops.frames_pad(dev, buf.size, plan, weights) is dev
    return dev.cpu().numpy(), plan.tolist(), table2


_ALONE = {}


def alone(ops, spec, kind):
    if (spec, kind) not in _ALONE:
        c = case(spec)
        out, plan, _ = device_pad(ops, c.buf, [c.row(kind)])
        _ALONE[spec, kind] = (out, plan)
    return _ALONE[spec, kind]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('spec', CASES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_kernel_against_the_restatement(ops, spec, kind):
    c, chans = case(spec), 3 if kind == 'image' else 1
    out, plan = alone(ops, spec, kind)
    compare(workspace_of(out, c.buf.size, c.n, chans), spec, kind)
    ws, end = plan[0][15], plan[0][15] + c.n * c.n * chans
    assert np.array_equal(out[:c.buf.size], c.buf) and (out[c.buf.size:ws] == FILL).all() and (out[end:] == FILL).all() and out.size == end + GUARD


def test_mixed_in_one_call_two_runs_guards_and_head(ops):
    """every case, as an image and as a mask, in ONE buffer and ONE call: each workspace image holds the bytes its case gives alone (another grid,
    another LDS size, other neighbours), twice; no byte outside the workspace images changes"""
    chunks, rows, base, slots = [], [], 0, [0, 0]
    for spec in CASES:
        c = case(spec)
        for kind in KINDS:
            rows.append(c.row(kind, slots[kind == 'mask'], base))
            slots[kind == 'mask'] += 1
        chunks.append(c.buf)
        base += c.buf.size
    buf = np.concatenate(chunks)
    first, plan, _ = device_pad(ops, buf, rows)
    second, _, _ = device_pad(ops, buf, rows)
    assert np.array_equal(first, second)                                                 # bit-identical from run to run
    assert len(plan) == 2 * len(CASES) and np.array_equal(first[:buf.size], buf)         # the packed head
    written = np.zeros(first.size, dtype=bool)
    written[:buf.size] = True
    for p, (spec, kind) in zip(plan, ((s, k) for s in CASES for k in KINDS)):
        c, chans = case(spec), 3 if kind == 'image' else 1
        nbytes = c.n * c.n * chans
        out, one = alone(ops, spec, kind)
        assert p[15] % 16 == 0 and not written[p[15]:p[15] + nbytes].any()
        assert np.array_equal(first[p[15]:p[15] + nbytes], out[one[0][15]:one[0][15] + nbytes]), (spec, kind)
        written[p[15]:p[15] + nbytes] = True
    guards = first[~written]
    assert guards.size >= GUARD + 1 and not written[buf.size] and (guards == FILL).all()          # before, between and behind the images


def test_refusals_name_the_cause(ops):
    from latent_pose_reenactment_amd import frames
    c = case((12, 17, 0, -3))
    _, plan, weights, total = frames.pad_plan(torch.tensor([c.row('image')], dtype=torch.int64), c.buf.size, SIZE)
    dev = torch.zeros(total, dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError, match='CUDA'):
        ops.frames_pad(dev.cpu(), c.buf.size, plan, weights)
    with pytest.raises(ValueError, match=r'plan 0 \(row 0\).*does not fit'):
        ops.frames_pad(dev[:total - 1], c.buf.size, plan, weights)
    tampered = plan.clone()
    tampered[0, 10] = 1
    with pytest.raises(ValueError, match=r'plan 0 \(row 0\).*pads'):
        ops.frames_pad(dev, c.buf.size, tampered, weights)
    with pytest.raises(ValueError, match='HOST'):
        ops.frames_pad(dev, c.buf.size, plan.cuda(), weights)
    # the library's own checks, past the wrapper's: the same refusals, before any device work
    from latent_pose_reenactment_amd import _lib
    scratch, weights_dev = torch.zeros(768 + 3, dtype=torch.int32, device='cuda'), weights.cuda()
    for col, value, code in ((10, 1, -1), (14, 5, -1), (15, 8, -1), (9, 2000, -2)):
        bad = plan.clone()
        bad[0, col] = value
        bad_dev = bad.cuda()
        rc = _lib.lib().lp_frames_pad(dev.data_ptr(), dev.numel(), c.buf.size, bad.data_ptr(), bad_dev.data_ptr(), 1, weights_dev.data_ptr(),
                                      scratch.data_ptr(), scratch[768:].data_ptr(), None)
        assert rc == code and b'plan 0 (row 0)' in _lib.lib().lp_last_error(), (col, rc, _lib.lib().lp_last_error())
    torch.cuda.synchronize()
    assert not dev.any()


# ---- the loader, end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return build_tree(tmp_path_factory.mktemp('voxceleb2_pad_gpu'))


def test_prepare_with_the_flag_on_the_device_equals_prepare_host(tree):
    """the same raw batches through the pad launches + the prepare launch and through the fp32 host definition, both with the flag: per sample under
    that sample's ``tolerance``, widened only at outputs fed by flagged workspace bytes (``extra_tolerance``: there the two uint8 images may differ
    by 1)"""
    from latent_pose_reenactment_amd import frames
    split = video_split(tree)
    for flags, paths in ((dict(val_split_path=split), PATHS), (dict(finetune=True, val_split_path=Path('id02/vidA'), batch_size=5), ['id02/vidA'] * 5)):
        loader = loader_for(make_args(tree, device='cpu', blur_padded_bands=True, **flags), 'val')
        assert loader.blur_padded_bands
        s0, worst, widened, per_sample = 0, 0.0, 0, 1 if 'finetune' in flags else K + 1
        for raw in loader.loader:
            (dd, dt), (hd, ht) = frames.prepare(raw, LOADER_SIZE, 'cuda', True), frames.prepare(raw, LOADER_SIZE, 'cpu', True)
            plain = frames.prepare(raw, LOADER_SIZE, 'cuda')
            assert set(dd) == set(hd) and set(dt) == set(ht) and torch.equal(dd['target_rgbs'], dd['pose_input_rgbs'] * dt['real_segm'])
            assert not torch.equal(plain[0]['enc_rgbs'], dd['enc_rgbs'])                 # every frame of the tree is at least one pixel out
            flat = lambda d: d['enc_rgbs'].reshape(-1, 3, LOADER_SIZE, LOADER_SIZE) if 'finetune' in flags else \
                torch.cat([d['enc_rgbs'].reshape(-1, 3, LOADER_SIZE, LOADER_SIZE), d['pose_input_rgbs'].reshape(-1, 3, LOADER_SIZE, LOADER_SIZE)])
            got = (flat(dd), dt['real_segm'][:, 0], dd['target_rgbs'][:, 0])
            want = (flat(hd), ht['real_segm'][:, 0], hd['target_rgbs'][:, 0])
            _, rows2, flagged = FP.pad(raw['buf'].numpy(), raw['table'].tolist())
            for i, r in enumerate(rows2):
                gates = tolerance(paths[s0 + i // per_sample])
                extra = extra_tolerance(r, flagged, LOADER_SIZE)
                for o, col in enumerate((FR.IMAGE_SLOT, FR.MASK_SLOT, FR.PRODUCT_SLOT)):
                    if r[col] < 0:
                        continue
                    err = (got[o][r[col]].cpu().double() - want[o][r[col]].double()).abs().numpy()
                    bound = gates[o] + (extra[o][None] if o == 1 else extra[o])
                    worst, widened = max(worst, float((err / bound).max())), widened + int((bound > gates[o]).sum())
                    assert (err <= bound).all(), (paths[s0 + i // per_sample], o, float(err.max()), gates[o])
            s0 += len(rows2) // per_sample
        print(f'[frames_pad] prepare with the flag, device vs prepare_host ({"fine-tuning" if "finetune" in flags else "meta-training"}): worst '
              f'difference / bound {worst:.2f}; outputs with a widened bound {widened}')


def test_one_training_iteration_with_blur_padded_bands(tree, tmp_path):
    """train.py on the tree with ``--blur_padded_bands``, at the geometry of tests/test_frames_gpu.py's iteration: finite losses"""
    from test_train_entry_gpu import COMMON
    common = list(COMMON)
    for flag in ('--dataloader', '--synthetic_dataset_len'):
        at = common.index(flag)
        del common[at:at + 2]
    cmd = [sys.executable, os.path.join(PKG, 'train.py')] + common + [
        '--dataloader', 'voxceleb2_segmentation_nolandmarks', '--data_root', str(tree), '--train_split_path', str(video_split(tree)),
        '--bboxes_dir', str(tree / 'bboxes.npy'), '--num_workers', '0', '--blur_padded_bands', '--experiments_dir', str(tmp_path),
        '--experiment_name', 'bands', '--log_frequency_loss', '1']
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'padded band carries' not in r.stdout + r.stderr                              # note_padding stays silent
    assert sorted(os.listdir(tmp_path / 'bands' / 'checkpoints')) == ['model_00000001.pth']
    line = [l for l in r.stdout.splitlines() if 'Epoch 0 (iteration' in l][-1]
    losses = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Loss_\w+) ([-+.\deE]+|nan|inf) \(avg', line)}
    print(f'[frames_pad] train.py with --blur_padded_bands, one iteration: {losses}')
    assert len(losses) >= 5 and all(math.isfinite(v) for v in losses.values()), losses
