"""Host-side checks of the pose-input augmentation (no GPU):
  * ``ParametricAugmenter.sample``: ranges, probabilities, the shift shared by the pose map and the target map, nothing when empty / ``inference``;
  * ``augmentation.augment_triplet_host`` (fp32 torch ops) against the fp64 restatement (tests/augment_restatement.py) on the case list and inside the
    gate of tests/test_augment_gpu.py -- the fp32 host implementation must sit inside the gate before the GPU is asked to;
  * ``dataloaders/synthetic_voxceleb2_augmented.py``: the base loader's tensors bit for bit, ``aug_params`` only with a flag on, new rows per visit
    for 'train', the same rows for 'val';
  * ``TrainingModule.forward`` on CPU tensors: with ``aug_params`` every module sees the augmented tensors, without the key the three input tensors
    pass through as the same objects;
  * lp_augment_triplet refuses bad arguments before any device work."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import augment_restatement as AR          # noqa: E402
from latent_pose_reenactment_amd import augmentation as AUG          # noqa: E402


def aug_args(**kw):
    a = argparse.Namespace(image_size=64, n_frames_for_encoder=3, num_labels=7, synthetic_dataset_len=6, world_size=1, random_seed=5, finetune=False,
                           use_pixelwise_augs=False, use_affine_scale=False, use_affine_shift=False, inference=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


ALL_ON = dict(use_pixelwise_augs=True, use_affine_scale=True, use_affine_shift=True)


# ---- sample -----------------------------------------------------------------------------------------------------------------------------------------------
def test_sample_draws_inside_the_reference_ranges():
    from latent_pose_reenactment_amd import hipops as ops
    assert len(ops.AUG_COLUMNS) == 32 == AUG.NCOLS and len(set(ops.AUG_COLUMNS)) == 32
    col = {name: i for i, name in enumerate(ops.AUG_COLUMNS)}
    assert (col['pose_a00'], col['target_a00'], col['k00'], col['k11'], col['mul'], col['add_r'], col['alpha'], col['gain'], col['sigma'],
            col['seed']) == (0, 6, 12, 16, 21, 22, 25, 26, 27, 28)
    size = 64
    aug = AUG.ParametricAugmenter(aug_args(image_size=size, **ALL_ON))
    assert not aug.is_empty()
    g = torch.Generator().manual_seed(2024)
    rows = torch.stack([aug.sample(g) for _ in range(2000)])
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (2000, 32)
    r = rows.double().numpy()
    eps = 1e-6
    c = (size - 1) / 2.0
    # maps: no rotation / shear, scales in [1 / 1.2, 1 / 0.8], target map a pure shift of at most 5 % of the frame
    assert (r[:, [1, 3, 7, 9]] == 0).all() and (r[:, [6, 10]] == 1).all()
    assert (r[:, [0, 4]] >= 1 / 1.2 - eps).all() and (r[:, [0, 4]] <= 1 / 0.8 + eps).all()
    assert (np.abs(r[:, [8, 11]]) <= 0.05 * size + eps).all()
    scaled = (r[:, 0] != 1) | (r[:, 4] != 1)
    shifted = (r[:, 8] != 0) | (r[:, 11] != 0)
    assert 0.4 <= scaled.mean() <= 0.6 and 0.4 <= shifted.mean() <= 0.6, (scaled.mean(), shifted.mean())
    # both scales are drawn together
    assert ((r[:, 0] != 1) == (r[:, 4] != 1)).all()
    # the shift inside Ap is At's
    for a0, a2, t2 in ((0, 2, 8), (4, 5, 11)):
        tx_pose = (c - r[:, a2]) / r[:, a0] - c                 # forward map of xs = c is xd = c + tx; from xs = a0 xd + a2: xd = (c - a2) / a0
        assert np.abs(tx_pose - (-r[:, t2])).max() <= 1e-4, np.abs(tx_pose + r[:, t2]).max()
    assert (r[~scaled][:, [0, 2, 4, 5]] == r[~scaled][:, [6, 8, 10, 11]]).all()          # without a scale the pose row IS the target row
    # filter: one of the four kinds, inside the hull of their extreme parameters
    k = r[:, 12:21]
    has_filter = (k != np.array(AR.IDENT_K)).any(1)
    assert 0.2 <= has_filter.mean() <= 0.6          # 1/2 of the rows pick the slot on average, some kernels are the identity (box k = 1)
    assert (np.abs(k.sum(1) - 1) <= 1e-5)[k[:, 0] >= 0].all()          # blurs sum to 1
    assert (np.abs(k).sum(1) <= 8 + 9.5 + eps).all() and (k[:, 4] <= 9.5 + eps).all() and (k >= -1.5 - eps).all()
    # pixelwise columns
    assert (r[:, 21] >= 0.5 - eps).all() and (r[:, 21] <= 1.5 + eps).all()
    assert (np.abs(r[:, 22:25]) <= 10 / 255 + eps).all()
    assert (r[:, 25] >= 0.75 - eps).all() and (r[:, 25] <= 1.25 + eps).all()
    assert ((r[:, 26] == 0) | ((r[:, 26] >= 3 - eps) & (r[:, 26] <= 11 + eps))).all()
    assert ((r[:, 25] == 1) | (r[:, 26] == 0)).all()          # linear OR sigmoid contrast
    assert (r[:, 27] >= 0).all() and (r[:, 27] <= 0.05 + eps).all()
    assert (r[:, 28] >= 0).all() and (r[:, 28] < 2 ** 24).all() and (r[:, 28] == np.floor(r[:, 28])).all()
    assert (r[:, 28][r[:, 27] == 0] == 0).all() and (r[:, 29:] == 0).all()
    per_channel = (r[:, 22] != r[:, 23]) | (r[:, 23] != r[:, 24])
    added = (r[:, 22:25] != 0).any(1)
    assert 0.4 <= per_channel[added].mean() <= 0.6
    for on in (r[:, 21] != 1, added, (r[:, 25] != 1) | (r[:, 26] != 0), r[:, 27] != 0):
        assert 0.4 <= on.mean() <= 0.6, on.mean()          # k in U{0 .. 5} of five slots: each slot in half of the rows
    # one flag at a time touches its own columns only
    only_shift = torch.stack([AUG.ParametricAugmenter(aug_args(use_affine_shift=True)).sample(g) for _ in range(50)]).numpy()
    assert (only_shift[:, 12:] == AUG.neutral_row().numpy()[12:]).all() and (only_shift[:, [0, 4]] == 1).all() and (only_shift[:, 8] != 0).any()
    only_pix = torch.stack([AUG.ParametricAugmenter(aug_args(use_pixelwise_augs=True)).sample(g) for _ in range(50)]).numpy()
    assert (only_pix[:, :12] == AUG.neutral_row().numpy()[:12]).all() and (only_pix[:, 12:] != AUG.neutral_row().numpy()[12:]).any()


def test_empty_augmenter_and_inference_yield_no_parameters():
    assert AUG.ParametricAugmenter(aug_args()).is_empty()
    assert AUG.ParametricAugmenter(aug_args(inference=True, **ALL_ON)).is_empty()
    assert torch.equal(AUG.ParametricAugmenter(aug_args()).sample(torch.Generator().manual_seed(0)), AUG.neutral_row())
    assert np.array_equal(AUG.neutral_row().numpy(), AR.neutral().astype(np.float32))
    from utils.argparse_utils import MyArgumentParser
    parser = MyArgumentParser(conflict_handler='resolve')
    AUG.get_args(parser)
    a = parser.parse_args([])
    assert (a.use_pixelwise_augs, a.use_affine_scale, a.use_affine_shift) == (False, False, False)
    a = parser.parse_args(['--use_affine_scale', '--use_pixelwise_augs'])
    assert (a.use_pixelwise_augs, a.use_affine_scale, a.use_affine_shift) == (True, True, False)


# ---- the host implementation against the restatement ----------------------------------------------------------------------------------------------
def sampled_rows(h, w, n=64, seed=99):
    """``n`` rows from ``sample`` for an H x W frame (the augmenter is told both sides)"""
    aug = AUG.ParametricAugmenter(aug_args(image_size=w, **ALL_ON))
    aug.height = h
    g = torch.Generator().manual_seed(seed)
    return [aug.sample(g).double().numpy() for _ in range(n)]


def check_against_restatement(fn, h, w, device='cpu'):
    """every family of parameter rows x (B, C) x layout at one size through ``fn(pose, params, target, segm)``: max-abs error / gate per tensor and
    family, printed; -> the worst ratio"""
    worst = {}
    fams = AR.family_rows(h, w)
    fams['sampled'] = sampled_rows(h, w)
    case = 0
    for fam, rows in fams.items():
        for b, c in AR.BATCH_CHANNELS:
            if fam == 'sampled' and (b, c) != (3, 3) and (b, c) != (3, 1):
                continue          # (64 rows through the B = 3 launches: 22 launches per channel count)
            for params in AR.batches(rows, b):
                layout = AR.LAYOUTS[case % len(AR.LAYOUTS)] if c == 3 else ('contiguous', 'pose_only', 'no_target', 'no_segm')[case % 4]
                case += 1
                pose, target, segm = AR.make_inputs(b, c, h, w, layout, seed=case, device=device)
                host = (lambda t: None if t is None else t.cpu().numpy())
                want = AR.augment(host(pose), params, host(target), host(segm))
                par = torch.tensor(params, dtype=torch.float32)
                assert np.array_equal(par.double().numpy(), params)          # the rows are fp32 values: both sides see the same parameters
                got = fn(pose, par.to(device), target, segm)
                gp, gt = AR.gate(params, h, w)
                for name, g_, w_, bound, src in (('pose', got[0], want[0], gp, pose), ('target', got[1], want[1], gt, target),
                                                 ('segm', got[2], want[2], gt, segm)):
                    assert (g_ is None) == (src is None), (name, layout)
                    if src is None:
                        continue
                    assert tuple(g_.shape) == tuple(src.shape) and g_.dtype == torch.float32
                    err = np.abs(g_.double().cpu().numpy() - w_).reshape(b, -1).max(1)
                    ratio = float((err / bound).max())
                    worst[(name, fam)] = max(worst.get((name, fam), 0.0), ratio)
    for name in ('pose', 'target', 'segm'):
        print(f'[augment] {device} {h} x {w} {name}: worst error / gate per family',
              {fam: f'{v:.3f}' for (n_, fam), v in worst.items() if n_ == name})
    return worst


@pytest.mark.parametrize('h,w', AR.SIZES)
def test_host_implementation_sits_inside_the_gate(h, w):
    worst = check_against_restatement(AUG.augment_triplet_host, h, w)
    bad = {k: v for k, v in worst.items() if v > 1.0}
    assert not bad, bad


def test_host_neutral_row_and_integer_shift_are_exact():
    h, w = 17, 19
    pose, target, segm = AR.make_inputs(2, 3, h, w, 'views', seed=3)
    neutral = torch.tensor(np.stack([AR.neutral()] * 2), dtype=torch.float32)
    out = AUG.augment_triplet_host(pose, neutral, target, segm)
    assert all(torch.equal(o, i) for o, i in zip(out, (pose, target, segm)))
    # 5-D in, 5-D out
    out5 = AUG.augment_triplet_host(pose[:, None], neutral, target[:, None], segm[:, None])
    assert all(tuple(o.shape) == (2, 1, 3, h, w) for o in out5) and torch.equal(out5[0][:, 0], pose)
    shift = torch.tensor(np.stack([AR.affine_row(h, w, tx=-w - 1, ty=h + 2)] * 2), dtype=torch.float32)
    out = AUG.augment_triplet_host(pose, shift, target, segm)
    want = AR.augment(pose.numpy(), shift.numpy(), target.numpy(), segm.numpy())
    for o, w_ in zip(out, want):
        assert np.array_equal(o.double().numpy(), w_)
    # noise: a function of (seed, row, column) alone
    z1, z2 = AUG.noise_field(5, h, w), AUG.noise_field(6, h, w)
    assert not torch.equal(z1, z2) and torch.equal(z1, AUG.noise_field(5, h, w))
    assert np.abs(z1.double().numpy() - AR.noise(5, h, w)).max() <= 8 * 2.0 ** -23 * 6
    big = AR.noise(7, 200, 200)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1) < 0.02


# ---- loader -------------------------------------------------------------------------------------------------------------------------------------------
def test_loader_is_the_base_loader_plus_parameter_rows():
    import importlib
    base = importlib.import_module('dataloaders.synthetic_voxceleb2')
    mod = importlib.import_module('dataloaders.synthetic_voxceleb2_augmented')
    from utils.argparse_utils import MyArgumentParser
    parser = MyArgumentParser(conflict_handler='resolve')
    mod.Dataset.get_args(parser)
    a = parser.parse_args([])
    assert a.use_affine_shift is False and a.synthetic_dataset_len == 64
    for part in ('train', 'val'):
        plain = base.Dataset.get_dataset(aug_args(image_size=32), part)
        off = mod.Dataset.get_dataset(aug_args(image_size=32), part)
        on = mod.Dataset.get_dataset(aug_args(image_size=32, **ALL_ON), part)
        inference = mod.Dataset.get_dataset(aug_args(image_size=32, inference=True, **ALL_ON), part)
        assert len(on) == len(plain)
        first = {}
        for visit in range(3):
            for index in (0, 3):
                bdata, btarget = plain[index]
                for ds in (off, on, inference):
                    data, target = ds[index]
                    assert set(data) - {'aug_params'} == set(bdata) and set(target) == set(btarget)
                    for key in bdata:
                        assert torch.equal(data[key], bdata[key]), key
                    assert torch.equal(target['real_segm'], btarget['real_segm']) and target['label'] == btarget['label']
                    assert ('aug_params' in data) == (ds is on)
                    if ds is on:
                        row = data['aug_params']
                        assert tuple(row.shape) == (32,) and row.dtype == torch.float32
                        if visit == 0:
                            first[index] = row
                        elif part == 'train':
                            assert not torch.equal(row, first[index]), (index, visit)
                        else:
                            assert torch.equal(row, first[index]), (index, visit)
        assert not torch.equal(first[0], first[3])
    # one flag is enough, and the collated batch carries [B, 32]
    ds = mod.Dataset.get_dataset(aug_args(image_size=32, use_affine_shift=True), 'train')
    batch = torch.utils.data.default_collate([ds[0], ds[1]])
    assert tuple(batch[0]['aug_params'].shape) == (2, 32)
    # a second dataset object with the same seed serves the same rows in the same order
    again = mod.Dataset.get_dataset(aug_args(image_size=32, use_affine_shift=True), 'train')
    assert torch.equal(again[0][0]['aug_params'], batch[0]['aug_params'][0])


# ---- TrainingModule -----------------------------------------------------------------------------------------------------------------------------------
class _Embedder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.seen = None

    def forward(self, d):
        self.seen = d['pose_input_rgbs']
        d['pose_embedding'] = d['pose_input_rgbs'].mean((1, 2, 3, 4)) * self.w


class _Generator(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.saw_params = None

    def forward(self, d):
        self.saw_params = 'aug_params' in d
        d['fake_rgbs'] = d['target_rgbs'][:, 0] * self.w * d['pose_embedding'][:, None, None, None]


class _Critic(torch.nn.Module):
    def forward(self, d):
        d['score'] = (d['fake_rgbs'] * d['real_segm'][:, 0]).mean()


class _Criterion(torch.nn.Module):
    def forward(self, d):
        return {'l1': (d['fake_rgbs'] - d['target_rgbs'][:, 0]).abs().mean()}


def test_training_module_augments_at_the_top_of_the_forward():
    from runners import holycow
    b, s = 2, 16
    g = torch.Generator().manual_seed(0)
    data = {'enc_rgbs': torch.rand(b, 2, 3, s, s, generator=g), 'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g),
            'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g)}
    target = {'real_segm': torch.rand(b, 1, 1, s, s, generator=g).expand(b, 1, 3, s, s), 'label': torch.arange(b)}
    aug = AUG.ParametricAugmenter(aug_args(image_size=s, **ALL_ON))
    gp = torch.Generator().manual_seed(4)
    params = torch.stack([aug.sample(gp) for _ in range(b)])
    assert not torch.equal(params, torch.stack([AUG.neutral_row()] * b))
    E, G = _Embedder(), _Generator()
    tm = holycow.TrainingModule(E, G, _Critic(), [_Criterion()], [], running_averages=None)
    # without the key: the parent commit's path -- the three input tensors reach the modules and all_data as the same objects
    all_data, lg, ld = tm(dict(data), dict(target))
    assert all_data['pose_input_rgbs'] is data['pose_input_rgbs'] and all_data['target_rgbs'] is data['target_rgbs']
    assert all_data['real_segm'] is target['real_segm'] and E.seen is data['pose_input_rgbs'] and 'aug_params' not in all_data
    plain_loss = float(lg['l1'].detach())
    # with the key
    want = AUG.augment_triplet_host(data['pose_input_rgbs'], params, data['target_rgbs'], target['real_segm'])
    d_in, t_in = dict(data, aug_params=params), dict(target)
    all_data, lg, ld = tm(d_in, t_in)
    assert torch.equal(all_data['pose_input_rgbs'], want[0]) and torch.equal(all_data['target_rgbs'], want[1])
    assert torch.equal(all_data['real_segm'], want[2]) and tuple(all_data['real_segm'].shape) == (b, 1, 3, s, s)
    assert E.seen is all_data['pose_input_rgbs'] and not torch.equal(E.seen, data['pose_input_rgbs'])
    assert G.saw_params is False and 'aug_params' not in all_data          # consumed
    assert float(lg['l1'].detach()) != plain_loss
    # the caller's dicts are untouched
    assert d_in['pose_input_rgbs'] is data['pose_input_rgbs'] and 'aug_params' in d_in and t_in['real_segm'] is target['real_segm']
    # apply with a missing target or mask augments what is there
    d2, t2 = AUG.apply({'pose_input_rgbs': data['pose_input_rgbs'], 'aug_params': params}, {'label': target['label']})
    assert torch.equal(d2['pose_input_rgbs'], want[0]) and set(d2) == {'pose_input_rgbs'} and set(t2) == {'label'}
    d3, t3 = AUG.apply({'pose_input_rgbs': data['pose_input_rgbs'], 'aug_params': params}, {'real_segm': target['real_segm']})
    assert torch.equal(t3['real_segm'], want[2])


# ---- C entry point ------------------------------------------------------------------------------------------------------------------------------------
def test_c_entry_point_validates_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    st = (ctypes.c_longlong * 4)(768, 256, 16, 1)
    sp, fake = ctypes.addressof(st), 4096          # (never dereferenced: every call below is refused first)
    f = l.lp_augment_triplet
    assert f(None, sp, fake, sp, fake, sp, fake, 1, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, None, fake, sp, fake, sp, fake, 1, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, None, 1, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 3, 16, 16, None, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    # target / segm may be null only TOGETHER with their strides and outputs
    assert f(fake, sp, fake, None, fake, sp, fake, 1, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, None, None, fake, sp, fake, 1, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'target' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 3, 16, 16, fake, fake, None, None) == -1 and b'segm' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 0, 3, 3, 16, 16, fake, fake, fake, None) == -1 and b'B >= 1' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 0, 3, 16, 16, fake, fake, fake, None) == -1 and b'1 .. 4' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 5, 3, 16, 16, fake, fake, fake, None) == -1 and b'1 .. 4' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 5, 16, 16, fake, fake, fake, None) == -1 and b'Cs' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 0, 16, 16, fake, fake, fake, None) == -1 and b'Cs' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 3, 0, 16, fake, fake, fake, None) == -1 and b'H >= 1' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 1, 3, 3, 16, 0, fake, fake, fake, None) == -1 and b'W >= 1' in l.lp_last_error()
    assert f(fake, sp, fake, sp, fake, sp, fake, 30000, 3, 3, 16, 16, fake, fake, fake, None) == -2 and b'grid' in l.lp_last_error()


def test_wrapper_refuses_inputs_off_the_gpu_and_malformed_ones_first():
    from latent_pose_reenactment_amd import hipops as ops
    x, p = torch.zeros(2, 3, 8, 8), torch.zeros(2, 32)
    with pytest.raises(ValueError, match='CUDA'):
        ops.augment_triplet(x, p)
    with pytest.raises(ValueError, match='fp32'):
        ops.augment_triplet(x.double(), p)
    with pytest.raises(ValueError, match=r'params must be \[B, 32\]'):
        ops.augment_triplet(x, torch.zeros(2, 31))
    with pytest.raises(ValueError, match='mismatch.*target'):
        ops.augment_triplet(x, p, torch.zeros(2, 3, 8, 9))
    with pytest.raises(ValueError, match='mismatch.*segm'):
        ops.augment_triplet(x, p, None, torch.zeros(3, 1, 8, 8))
    with pytest.raises(ValueError, match='4 channels'):
        ops.augment_triplet(torch.zeros(2, 5, 8, 8), p)


def test_abi_tests_hold_with_the_new_symbol():
    import test_abi
    assert 'lp_augment_triplet' in test_abi.parse_header()
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_ctypes_signatures_match_header()
