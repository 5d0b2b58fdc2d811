"""lp_augment_triplet on the MI355X (``hipops.augment_triplet``: one launch for pose image, target and mask) against the fp64 restatement
(tests/augment_restatement.py), the bit-exact properties of the definition, the wrapper's refusals, the captured training step and train.py.

Case list: (H, W) in {(8, 8), (17, 17), (24, 40), (33, 19), (64, 64)} -- below one 16 x 16 tile, tile tails in both axes, W % 4 != 0 (the scalar
store path) -- x (B, C) in {1, 3} x {3, 1} x {contiguous 4-D inputs, ``[:, 0]`` views of [B, 2, C, H, W] tensors with a stride-0 ``expand``ed mask,
target and / or mask absent}; parameter rows: every group of columns ALONE (neutral; integer shifts (3, -2) and (-W - 1, H + 2); scale (0.8, 1.2);
scale + fractional shift; the four filters at their extreme parameters; mul 0.5 / 1.5; per-channel add; alpha 0.75 / 1.25; gain 3 / 11; sigma 0.05
with two seeds), all together, and 64 rows from ``ParametricAugmenter.sample``.

Gate: max-abs error <= (8 S + 8) 2^-23 Amp, S = max(H, W), Amp = sum|k| |mul| max(1, alpha, gain / 4) for the pose image, Amp = 1 for target and
mask.  Derivation: a source coordinate is three fp32 products and sums of magnitude <= 1.3 S, at most about 4 ulp(S) = 4 S 2^-23 per axis; that
error enters a bilinear weight which multiplies a pixel difference <= 1, on two axes: 8 S 2^-23.  The later steps are Lipschitz with the factors in
Amp (the filter sum|k|, the multiply |mul|, the contrasts alpha and gain / 4).  The + 8 covers their own roundings and the fp32 Box-Muller at
sigma <= 0.05.  No case needs masking: bilinear sampling, both border rules and every pixelwise step are continuous in the coordinate, so a
``floor`` that lands on the other side of an integer moves nothing.  The fp32 host implementation sits inside this gate (tests/test_augment_cpu.py:
worst error / gate 0.09 over the case list).

The train.py runs use 128 x 128 and batch 4, not 64 x 64 and batch 2: the default plugin family's identity encoder (the only family whose embedder
reads ``pose_input_rgbs``) takes frames of at least 128 x 128 and train-mode batches of at least 8 frames -- the geometry of
tests/test_train_entry_gpu.py.  The ``--hip_graph`` run makes five iterations instead of two: the first three run eagerly, so two iterations would
never replay the captured step."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import augment_restatement as AR          # noqa: E402
from test_augment_cpu import check_against_restatement, sampled_rows          # noqa: E402


def rows_tensor(rows, b):
    return torch.tensor(np.stack([rows[i % len(rows)] for i in range(b)]), dtype=torch.float32).cuda()


# ---- against the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', AR.SIZES)
def test_kernel_against_the_restatement(h, w):
    from latent_pose_reenactment_amd import hipops as ops
    worst = check_against_restatement(ops.augment_triplet, h, w, device='cuda')
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


# ---- bit-exact properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', AR.SIZES)
def test_neutral_row_returns_the_inputs_and_runs_repeat(h, w):
    from latent_pose_reenactment_amd import hipops as ops
    for b, c in AR.BATCH_CHANNELS:
        for layout in (AR.LAYOUTS if c == 3 else ('contiguous', 'pose_only')):
            pose, target, segm = AR.make_inputs(b, c, h, w, layout, seed=5, device='cuda')
            out = ops.augment_triplet(pose, rows_tensor([AR.neutral()], b), target, segm)
            for o, i in zip(out, (pose, target, segm)):
                assert (o is None) == (i is None)
                assert i is None or (torch.equal(o, i) and o.is_contiguous() and o.data_ptr() != i.data_ptr()), (b, c, layout)
            # 5-D in, 5-D out
            out5 = ops.augment_triplet(pose[:, None], rows_tensor([AR.neutral()], b), None if target is None else target[:, None])
            assert tuple(out5[0].shape) == (b, 1, c, h, w) and torch.equal(out5[0][:, 0], pose) and out5[2] is None
            # any row: two runs are identical
            for rows in AR.family_rows(h, w).values():
                par = rows_tensor(rows, b)
                first, second = ops.augment_triplet(pose, par, target, segm), ops.augment_triplet(pose, par, target, segm)
                assert all(a is None or torch.equal(a, b_) for a, b_ in zip(first, second))


def reflect_index(i, n):
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    m = torch.remainder(i, p)
    return torch.where(m < n, m, p - m)


@pytest.mark.parametrize('h,w', AR.SIZES)
def test_integer_shifts_are_index_gathers(h, w):
    from latent_pose_reenactment_amd import hipops as ops
    for b, c, layout in ((1, 3, 'contiguous'), (3, 3, 'views'), (3, 1, 'contiguous')):
        pose, target, segm = AR.make_inputs(b, c, h, w, layout, seed=8, device='cuda')
        for tx, ty in ((3, -2), (-w - 1, h + 2)):
            out = ops.augment_triplet(pose, rows_tensor([AR.affine_row(h, w, tx=tx, ty=ty)], b), target, segm)
            ys, xs = torch.arange(h, device='cuda') - ty, torch.arange(w, device='cuda') - tx          # source = destination - shift
            yr, xr = reflect_index(ys, h), reflect_index(xs, w)
            assert torch.equal(out[0], pose[:, :, yr][:, :, :, xr]), (b, c, layout, tx, ty)
            assert torch.equal(out[1], target[:, :, yr][:, :, :, xr])
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            want = segm[:, :, ys.clamp(0, h - 1)][:, :, :, xs.clamp(0, w - 1)] * inside
            assert torch.equal(out[2], want)
            assert (tx, ty) == (3, -2) or h < 3 or bool((out[2] == 0).all())          # shifted out of the frame: the mask is gone, the images are not
            assert bool((out[1] != 0).any())


def test_noise_depends_on_seed_row_and_column_only():
    from latent_pose_reenactment_amd import hipops as ops
    h, w = 33, 19
    pose = torch.full((3, 3, h, w), 0.5).cuda()
    a, b_ = AR.with_cols(sigma=0.05, seed=12345), AR.with_cols(sigma=0.05, seed=12346)
    one = ops.augment_triplet(pose[:1], rows_tensor([a], 1))[0]
    other = ops.augment_triplet(pose[:1], rows_tensor([b_], 1))[0]
    three = ops.augment_triplet(pose, rows_tensor([b_, AR.neutral(), a], 3))[0]
    assert not torch.equal(one, other)
    assert torch.equal(three[2], one[0]) and torch.equal(three[0], other[0]) and torch.equal(three[1], pose[1])
    assert torch.equal(one[0, 0], one[0, 1]) and torch.equal(one[0, 0], one[0, 2])          # one value per pixel, shared by the channels
    z = (one[0, 0].double().cpu().numpy() - 0.5) / float(np.float32(0.05))
    # (0.5 + sigma z rounds at 2^-24 of ~0.8, divided by sigma: 1e-6; logf, sqrtf, cosf: a few ulp of |z| <= 5.8)
    assert np.abs(z - AR.noise(12345, h, w)).max() <= 2e-5


# ---- the wrapper ------------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_malformed_inputs():
    from latent_pose_reenactment_amd import hipops as ops
    x, p = torch.zeros(2, 3, 8, 8).cuda(), torch.zeros(2, 32).cuda()
    assert tuple(ops.augment_triplet(x, p)[0].shape) == (2, 3, 8, 8)
    with pytest.raises(ValueError, match='pose must be fp32'):
        ops.augment_triplet(x.half(), p)
    with pytest.raises(ValueError, match='segm must be fp32'):
        ops.augment_triplet(x, p, None, x.double())
    with pytest.raises(ValueError, match='params must be fp32'):
        ops.augment_triplet(x, p.double())
    with pytest.raises(ValueError, match='target is on cpu'):
        ops.augment_triplet(x, p, x.cpu())
    with pytest.raises(ValueError, match='params is on cpu'):
        ops.augment_triplet(x, p.cpu())
    with pytest.raises(ValueError, match='pose is on cpu'):
        ops.augment_triplet(x.cpu(), p.cpu())
    with pytest.raises(ValueError, match='mismatch.*target'):
        ops.augment_triplet(x, p, torch.zeros(2, 3, 8, 9).cuda())
    with pytest.raises(ValueError, match='mismatch.*target'):
        ops.augment_triplet(x, p, torch.zeros(2, 1, 8, 8).cuda())
    with pytest.raises(ValueError, match='mismatch.*segm'):
        ops.augment_triplet(x, p, None, torch.zeros(2, 3, 9, 8).cuda())
    with pytest.raises(ValueError, match=r'params must be \[B, 32\]'):
        ops.augment_triplet(x, torch.zeros(3, 32).cuda())
    with pytest.raises(ValueError, match=r'params must be \[B, 32\]'):
        ops.augment_triplet(x, torch.zeros(2, 33).cuda())
    with pytest.raises(ValueError, match='4 channels'):
        ops.augment_triplet(torch.zeros(2, 5, 8, 8).cuda(), p)
    with pytest.raises(ValueError, match='4 channels'):
        ops.augment_triplet(x, p, None, torch.zeros(2, 5, 8, 8).cuda())
    with pytest.raises(ValueError, match=r'\[B, C, H, W\]'):
        ops.augment_triplet(torch.zeros(3, 8, 8).cuda(), p)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='mixed devices'):
            ops.augment_triplet(x, p.to('cuda:1'))


# ---- captured step ----------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_augments_with_the_new_batch_parameters(monkeypatch):
    """the parameter table is one more tensor of the batch: ``load_batch`` copies it into the captured step's static inputs and the replay augments
    the NEW batch with the NEW rows"""
    from latent_pose_reenactment_amd import hipops as ops
    import test_train_step as TS
    z = TS.load()
    tm, opt_G, opt_D, a, data, target, holycow = TS.build(z, 'RAdam', monkeypatch)
    b, s = data['pose_input_rgbs'].shape[0], data['pose_input_rgbs'].shape[-1]
    rows = sampled_rows(s, s, n=8, seed=3)
    rows = [r for r in rows if (r != AR.neutral()).any()]
    par1, par2 = rows_tensor(rows[:b], b), rows_tensor(rows[b:2 * b], b)
    assert not torch.equal(par1, par2)
    keys = ('pose_input_rgbs', 'target_rgbs', 'real_segm')
    data1 = dict(data, aug_params=par1)
    step = holycow.GraphedTrainStep(tm, opt_G, opt_D, a, data1, target, warmup_steps=3)
    step()
    torch.cuda.synchronize()
    assert 'aug_params' not in step.all_data
    first = {k: step.all_data[k].clone() for k in keys}
    want1 = ops.augment_triplet(data['pose_input_rgbs'], par1, data['target_rgbs'], target['real_segm'])
    assert all(torch.equal(first[k], w_) for k, w_ in zip(keys, want1))
    g = torch.Generator().manual_seed(1)
    data2 = {k: (torch.rand(v.shape, generator=g).cuda() if v.is_floating_point() else v) for k, v in data.items()}
    data2['aug_params'] = par2
    target2 = dict(target, real_segm=torch.rand(b, 1, 1, s, s, generator=g).cuda().expand(b, 1, 3, s, s))
    step.load_batch(data2, target2)
    step()
    torch.cuda.synchronize()
    want2 = ops.augment_triplet(data2['pose_input_rgbs'], par2, data2['target_rgbs'], target2['real_segm'])
    for k, w_ in zip(keys, want2):
        assert torch.equal(step.all_data[k], w_), k
        assert not torch.equal(step.all_data[k], first[k]), k
    assert all(torch.isfinite(v).all() for v in list(step.losses_G.values()) + list(step.losses_D.values()))


# ---- train.py ---------------------------------------------------------------------------------------------------------------------------------------
DRIVER = '''
import sys
sys.path.insert(0, {pkg!r})
import train
import runners.holycow as H
inner = H.train_step
def train_step(*args, **kw):
    out = inner(*args, **kw)
    print('ITERATION_LOSSES', {{k: float(v) for k, v in {{**out[1], **out[2]}}.items()}}, flush=True)
    return out
H.train_step = train_step
train.main()
'''


def run_train(tmp_path, name, loader, dataset_len, extra):
    from test_train_entry_gpu import COMMON
    args = list(COMMON)
    args[args.index('--dataloader') + 1] = loader
    args[args.index('--synthetic_dataset_len') + 1] = str(dataset_len)          # batch 4
    driver = tmp_path / 'drive_train.py'
    driver.write_text(DRIVER.format(pkg=PKG))
    cmd = [sys.executable, str(driver)] + args + ['--experiments_dir', str(tmp_path), '--experiment_name', name, '--log_frequency_loss', '1'] + extra
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if 'Epoch 0 (iteration' in l][-1]
    assert f'(iteration {dataset_len // 4})' in line, line
    last = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Loss_\w+) ([-+.\deEnaif]+) \(avg', line)}
    avg = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Loss_\w+) [-+.\deEnaif]+ \(avg ([-+.\deEnaif]+)\)', line)}
    eager = [eval(l.split('ITERATION_LOSSES', 1)[1]) for l in r.stdout.splitlines() if l.startswith('ITERATION_LOSSES')]
    return last, avg, eager


FLAGS = ['--use_affine_scale', '--use_affine_shift', '--use_pixelwise_augs']
RUNS = {'aug_eager': ('synthetic_voxceleb2_augmented', 8, FLAGS), 'aug_graph': ('synthetic_voxceleb2_augmented', 20, FLAGS + ['--hip_graph']),
        'aug_off': ('synthetic_voxceleb2_augmented', 8, []), 'base': ('synthetic_voxceleb2', 8, [])}


@pytest.fixture(scope='module')
def train_runs(tmp_path_factory):
    """name -> (last, avg, per-iteration losses) of a train.py run, each made once for the module"""
    done, tmp = {}, tmp_path_factory.mktemp('augment_train')

    def get(name):
        if name not in done:
            done[name] = run_train(tmp, name, *RUNS[name])
        return done[name]
    return get


def test_train_entry_with_augmentation_eager_and_graphed(train_runs):
    import math
    last, avg, eager = train_runs('aug_eager')
    assert len(last) >= 4 and len(eager) == 2, (last, eager)
    assert all(math.isfinite(v) for v in list(last.values()) + list(avg.values())), (last, avg)
    assert all(math.isfinite(v) for it in eager for v in it.values()), eager
    glast, gavg, geager = train_runs('aug_graph')
    assert set(glast) == set(last) and len(geager) == 3, (glast, geager)          # three eager iterations, then two replays of the captured step
    assert all(math.isfinite(v) for v in list(glast.values()) + list(gavg.values())), (glast, gavg)
    print(f'[augment] train.py with the three flags: eager last {last}; --hip_graph last (replayed) {glast}')


def test_train_entry_with_the_flags_off_is_the_base_loader(train_runs):
    off, base, on = train_runs('aug_off')[2], train_runs('base')[2], train_runs('aug_eager')[2]
    assert len(off) == len(base) == 2 and set(off[0]) == set(base[0]) and len(off[0]) >= 4
    print(f'[augment] first-iteration losses: flags off {off[0]}; base loader {base[0]}; flags on {on[0]}')
    assert off[0] == base[0], (off[0], base[0])
    assert on[0] != base[0]          # and with the flags on the step sees other pixels
