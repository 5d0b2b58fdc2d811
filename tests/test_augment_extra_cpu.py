"""Host-side checks of the second augmentation stage (no GPU):
  * ``augmentation.augment_extra_host`` (fp32 torch ops) against the fp64 restatement (tests/augment_extra_restatement.py) on the case list and
    under the gates of tests/test_augment_extra_gpu.py, the 1 / 8 cap on blocks with a near-tie included -- the fp32 host implementation must sit
    inside them before the GPU is asked to;
  * the JPEG step alone against PIL's round trip (``subsampling=0``) at qualities 70 and 85: closer to PIL than PIL is to its input;
  * ``ParametricAugmenter.sample_extra``: a stream of its own (``aug_params`` bit-identical with the flag on and off), deterministic in
    (seed, index, visit), ranges over 10^4 draws, the neutral row under ``--inference``;
  * both loaders emit ``aug_params_extra`` only with the flag; ``apply`` on CPU tensors with either key alone and with both;
  * lp_augment_extra and ``hipops.augment_extra`` refuse bad arguments before any device work."""
import argparse
import ctypes
import io
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

import augment_extra_restatement as XR          # noqa: E402
from latent_pose_reenactment_amd import augmentation as AUG          # noqa: E402


def aug_args(**kw):
    a = argparse.Namespace(image_size=64, n_frames_for_encoder=3, num_labels=7, synthetic_dataset_len=6, world_size=1, random_seed=5, finetune=False,
                           use_pixelwise_augs=False, use_affine_scale=False, use_affine_shift=False, use_extra_pixelwise_augs=False, inference=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# ---- against the restatement ------------------------------------------------------------------------------------------------------------------------
CAP = 1.0 / 8.0


def saturation_image(b, h, w):
    """exact grey and black pixels, S on both sides of s0 = 20 / 255 (S = 0.05, 0.078, 0.08, 0.5, 1) and uniform noise elsewhere"""
    x = XR.noise_image(b, h, w, seed=77)
    special = [(0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.8, 0.76, 0.78), (0.8, 0.8 * (1 - 0.078), 0.79), (0.8, 0.8 * (1 - 0.08), 0.75),
               (0.2, 0.4, 0.3), (0.0, 0.6, 0.3), (0.25, 0.25, 0.25), (0.7, 0.7, 0.1)]
    flat = x.reshape(b, 3, h * w)
    for i, rgb in enumerate(special):
        flat[:, :, (3 * i + 1) % (h * w)] = np.array(rgb)[None]
    return np.float32(flat.reshape(b, 3, h, w)).astype(np.float64)


def median_image(b, h, w):
    """values from a set of five, so that every window holds repeated values"""
    return np.random.RandomState(5).choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0]), size=(b, 3, h, w))


def cases(h, w):
    """(name, x [B, 3, H, W] fp64, params [B, 16]) of one size: every step alone on its own inputs, B in {1, 3}"""
    out = []
    inputs = {'neutral': XR.noise_image, 'elastic': XR.noise_image, 'median': median_image, 'saturation': saturation_image, 'jpeg': XR.smooth_image}
    for step, rows in XR.step_rows().items():
        for b in XR.BATCHES:
            for k, par in enumerate(XR.batches(rows, b)):
                make = inputs[step]
                if step == 'jpeg':
                    x = XR.smooth_image(b, h, w, seed=100 * XR.JPEG_SEED[(h, w)] + 10 * b + k)
                else:
                    x = make(b, h, w) if make in (median_image, saturation_image) else make(b, h, w, seed=10 * h + k)
                out.append((f'{step}/B{b}/{k}', x, par))
    return out


def sampled_rows(n=32, seed=0):
    """``n`` rows from ``sample_extra`` (at most two steps each) behind one row with all four steps on.  A row with elastic AND JPEG flags every
    block of its sample (the elastic gate times 8 x 255 is far above a quantisation step), so the generator seed is one whose rows keep the case
    inside the 1 / 8 cap: this one draws elastic + JPEG once and saturation + JPEG twice"""
    aug = AUG.ParametricAugmenter(aug_args(use_extra_pixelwise_augs=True))
    g = torch.Generator().manual_seed(seed)
    return [XR.row(alpha=2.0, seed=4242, median=1, d=-12.0 / 255.0, quality=80)] + [aug.sample_extra(g).double().numpy() for _ in range(n)]


def run_case(fn, name, x, par, device, worst, flagged):
    got = fn(torch.tensor(x, dtype=torch.float32).to(device), torch.tensor(par, dtype=torch.float32).to(device))
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    res = XR.check(got.cpu().numpy(), x, par)
    step = name.split('/')[0]
    worst[step] = max(worst.get(step, 0.0), max(r['ratio'] for r in res))
    flagged[name] = float(np.mean([r['flagged'] for r in res]))


def check_against_restatement(fn, h, w, device='cpu'):
    """every case of one size through ``fn(pose, params_extra)`` -> ({step: worst error / gate}, {case: share of blocks with a near-tie}); printed"""
    worst, flagged = {}, {}
    for name, x, par in cases(h, w):
        run_case(fn, name, x, par, device, worst, flagged)
    print(f'[augment_extra] {device} {h} x {w}: worst error / gate per step', {k: f'{v:.4f}' for k, v in worst.items()},
          '; largest share of blocks with a near-tie', f'{max(flagged.values()):.3f}')
    return worst, flagged


def check_chain(fn, device='cpu'):
    """one row with all four steps and 32 sampled rows at 64 x 64, three per launch: ONE case for the cap"""
    rows = sampled_rows()
    worst, flagged = {}, {}
    for k, par in enumerate(XR.batches(rows, 3)):
        run_case(fn, f'chain/{k}', XR.smooth_image(3, 64, 64, seed=300 + k), par, device, worst, flagged)
    share = float(np.mean(list(flagged.values())))
    print(f'[augment_extra] {device} chain of {len(rows)} rows at 64 x 64: worst error / gate {worst["chain"]:.4f}; share of blocks with a near-tie '
          f'{share:.3f}')
    return worst['chain'], share


@pytest.mark.parametrize('h,w', XR.SIZES)
def test_host_implementation_sits_inside_the_gates(h, w):
    worst, flagged = check_against_restatement(AUG.augment_extra_host, h, w)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert worst['neutral'] == 0.0 and worst['median'] == 0.0          # selections and copies: exact
    assert all(v <= CAP for v in flagged.values()), {k: v for k, v in flagged.items() if v > CAP}


def test_host_chain_sits_inside_the_gates_and_the_cap():
    worst, share = check_chain(AUG.augment_extra_host)
    assert worst <= 1.0 and share <= CAP, (worst, share)
    rows = np.stack(sampled_rows())
    assert (rows[0, [0, 2, 3, 4]] != 0).all()
    for col in (0, 2, 3, 4):
        assert (rows[1:, col] != 0).any(), col          # the sampled rows exercise every step
    assert ((rows[1:, [0, 2, 3, 4]] != 0).sum(1) <= 2).all() and ((rows[1:, [0, 2, 3, 4]] != 0).sum(1) == 2).any()


def test_host_neutral_rows_views_and_pure_functions():
    x = torch.rand(2, 2, 3, 17, 19, generator=torch.Generator().manual_seed(0))
    view = x[:, 0]
    neutral = torch.zeros(2, 16)
    assert torch.equal(AUG.augment_extra_host(view, neutral), view)
    out5 = AUG.augment_extra_host(x[:, :1], neutral)
    assert tuple(out5.shape) == (2, 1, 3, 17, 19) and torch.equal(out5[:, 0], view)
    # values outside [0, 1] come back clamped
    assert torch.equal(AUG.augment_extra_host(view * 3 - 1, neutral), (view * 3 - 1).clamp(0, 1))
    # each sample's result depends on its own row and image only
    par = torch.tensor(np.stack([XR.row(alpha=3.5, seed=9, median=1, d=0.05, quality=75), XR.row(d=-0.07)]), dtype=torch.float32)
    both = AUG.augment_extra_host(view, par)
    assert torch.equal(both[1], AUG.augment_extra_host(view[1:], par[1:])[0]) and torch.equal(both[0], AUG.augment_extra_host(view[:1], par[:1])[0])
    # displacement: exact in fp32, in [-1, 1), another field per seed, and not the noise step's field for the same seed
    u0, u1 = XR.displacement(5, 17, 19)
    assert u0.min() >= -1 and u0.max() < 1 and np.array_equal(np.float32(u0).astype(np.float64), u0) and not np.array_equal(u0, u1)
    assert not np.array_equal(u0, XR.displacement(6, 17, 19)[0])
    big = np.concatenate(XR.displacement(3, 200, 200))
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1 / np.sqrt(3)) < 0.01
    # a grey image stays grey under saturation, and the largest channel keeps its value
    grey = torch.full((1, 3, 8, 8), 0.4)
    assert torch.equal(AUG.augment_extra_host(grey, torch.tensor(XR.row(d=20 / 255)[None], dtype=torch.float32)), grey)
    sat = AUG.augment_extra_host(view, torch.tensor(np.stack([XR.row(d=20 / 255)] * 2), dtype=torch.float32))
    assert torch.equal(sat.max(1).values, view.max(1).values) and not torch.equal(sat, view)
    # quantisation tables: the IJG rule at its two branches and its clamps
    ql, qc = AUG.quant_tables(50)
    assert ql.flatten().tolist() == [float(v) for v in XR.K1] and qc.flatten().tolist() == [float(v) for v in XR.K2]
    assert AUG.quant_tables(100)[0].eq(1).all() and AUG.quant_tables(1)[1].eq(255).all() and AUG.quant_tables(75)[0][0, 0] == 8
    for quality in (1, 25, 49, 50, 70, 85, 95, 99, 100):
        for mine, theirs in zip(AUG.quant_tables(quality), XR.quant_tables(quality)):
            assert np.array_equal(mine.double().numpy(), theirs)


# ---- JPEG against PIL -------------------------------------------------------------------------------------------------------------------------------
def pil_inputs():
    """four 64 x 64 uint8 images as fp64 [3, 64, 64] in [0, 1]: smooth, smooth + 0.08 noise, a checker of the smooth image and its negative, noise"""
    rng = np.random.RandomState(3)
    smooth = XR.smooth_image(1, 64, 64, seed=42)[0]
    yy, xx = np.meshgrid(np.arange(64), np.arange(64), indexing='ij')
    checker = np.where(((yy // 4 + xx // 4) % 2 == 0)[None], smooth, 1.0 - smooth)
    imgs = {'smooth': smooth, 'smooth+noise': smooth + 0.08 * rng.standard_normal(smooth.shape), 'checker': checker,
            'noise': rng.uniform(0, 1, smooth.shape)}
    return {k: np.round(np.clip(v, 0, 1) * 255.0) / 255.0 for k, v in imgs.items()}


def pil_round_trip(img, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.round(img * 255.0).astype(np.uint8).transpose(1, 2, 0)).save(buf, format='JPEG', quality=quality, subsampling=0)
    return np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB')).transpose(2, 0, 1) / 255.0


def test_jpeg_step_models_pil_round_trip():
    """RMS(ours - PIL) < RMS(PIL - input) at qualities 70 and 85: the step models the compression and adds no distortion of its size.  Quality 99 is
    printed and not gated: PIL's uint8 output and integer DCT are then as large as the artefacts."""
    ratios = {}
    for name, img in pil_inputs().items():
        for quality in (70, 85, 99):
            pil = pil_round_trip(img, quality)
            par = torch.tensor(XR.row(quality=quality)[None], dtype=torch.float32)
            ours = AUG.augment_extra_host(torch.tensor(img[None], dtype=torch.float32), par)[0].double().numpy()
            rms = (lambda a: float(np.sqrt((a * a).mean())))
            ratios[(name, quality)] = rms(ours - pil) / rms(pil - img)
            assert np.abs(ours - XR.jpeg(img, quality).clip(0, 1)).max() < 1e-5
    print('[augment_extra] JPEG against PIL (subsampling=0), RMS(ours - PIL) / RMS(PIL - input):', {k: f'{v:.3f}' for k, v in ratios.items()})
    gated = {k: v for k, v in ratios.items() if k[1] in (70, 85)}
    print(f'[augment_extra] worst gated ratio {max(gated.values()):.3f}')
    assert all(v < 1.0 for v in gated.values()), gated


# ---- parameter stream -------------------------------------------------------------------------------------------------------------------------------
def test_sample_extra_ranges_stream_and_inference():
    from latent_pose_reenactment_amd import hipops as ops
    assert len(ops.AUG_EXTRA_COLUMNS) == 16 == AUG.NCOLS_EXTRA == XR.NCOLS and len(set(ops.AUG_EXTRA_COLUMNS)) == 16
    assert ops.AUG_EXTRA_COLUMNS[:5] == ('elastic_alpha', 'elastic_seed', 'median', 'saturation', 'jpeg_quality')
    aug = AUG.ParametricAugmenter(aug_args(use_extra_pixelwise_augs=True))
    assert not aug.is_empty() and aug.has_extra_stage() and not aug.has_first_stage()
    g = torch.Generator().manual_seed(2025)
    rows = torch.stack([aug.sample_extra(g) for _ in range(10000)])
    assert rows.dtype == torch.float32 and tuple(rows.shape) == (10000, 16)
    r = rows.double().numpy()
    eps = 1e-6
    on = r[:, [0, 2, 3, 4]] != 0
    assert (on.sum(1) <= 2).all() and (r[:, 5:] == 0).all()
    counts = np.bincount(on.sum(1), minlength=3) / len(r)
    # subset size uniform in {0, 1, 2}; a chosen elastic slot is on half of the time, so some subsets show one step fewer
    assert abs(counts[2] - (1 / 3) * (1 - 0.5 * 0.5)) < 0.03 and abs(counts[0] - (1 / 3 + (1 / 3) * 0.25 * 0.5)) < 0.03, counts
    share = on.mean(0)
    assert abs(share[0] - 0.125) < 0.02 and all(abs(s - 0.25) < 0.03 for s in share[1:]), share
    alpha = r[:, 0][on[:, 0]]
    assert (alpha >= 0.5 - eps).all() and (alpha <= 3.5 + eps).all() and alpha.min() < 0.6 and alpha.max() > 3.4
    assert (r[:, 1] >= 0).all() and (r[:, 1] < 2 ** 24).all() and (r[:, 1] == np.floor(r[:, 1])).all() and (r[:, 1][~on[:, 0]] == 0).all()
    assert set(np.unique(r[:, 2])) == {0.0, 1.0}
    d = r[:, 3][on[:, 2]]
    assert (np.abs(d) <= 20 / 255 + eps).all() and d.min() < -19 / 255 and d.max() > 19 / 255
    quality = r[:, 4][on[:, 3]]
    assert (quality == np.floor(quality)).all() and set(np.unique(quality)) == set(float(v) for v in range(70, 100))
    # flag off, or --inference: the neutral row, and nothing to emit
    for a in (aug_args(), aug_args(inference=True, use_extra_pixelwise_augs=True, use_pixelwise_augs=True)):
        off = AUG.ParametricAugmenter(a)
        assert off.is_empty() and not off.has_extra_stage()
        assert torch.equal(off.sample_extra(torch.Generator().manual_seed(1)), torch.zeros(16))
    assert torch.equal(AUG.neutral_row_extra(), torch.zeros(16)) and np.array_equal(XR.row(), np.zeros(16))
    # the flag: a store_bool, default off
    from utils.argparse_utils import MyArgumentParser
    parser = MyArgumentParser(conflict_handler='resolve')
    AUG.get_args(parser)
    assert parser.parse_args([]).use_extra_pixelwise_augs is False
    a = parser.parse_args(['--use_extra_pixelwise_augs'])
    assert a.use_extra_pixelwise_augs is True and a.use_pixelwise_augs is False
    # sample() does not look at the new flag
    first = AUG.ParametricAugmenter(aug_args(use_pixelwise_augs=True, use_affine_scale=True, use_extra_pixelwise_augs=True))
    plain = AUG.ParametricAugmenter(aug_args(use_pixelwise_augs=True, use_affine_scale=True))
    for seed in range(20):
        assert torch.equal(first.sample(torch.Generator().manual_seed(seed)), plain.sample(torch.Generator().manual_seed(seed)))
    assert AUG.extra_stream_seed(5, 3, 2) != (5 * 1000003 + 3) * 8191 + 2 + 700001


def test_synthetic_loader_emits_the_key_only_with_the_flag():
    import importlib
    mod = importlib.import_module('dataloaders.synthetic_voxceleb2_augmented')
    first_on = dict(use_pixelwise_augs=True, use_affine_scale=True, use_affine_shift=True)
    for part in ('train', 'val'):
        plain = mod.Dataset.get_dataset(aug_args(image_size=32, **first_on), part)
        both = mod.Dataset.get_dataset(aug_args(image_size=32, use_extra_pixelwise_augs=True, **first_on), part)
        alone = mod.Dataset.get_dataset(aug_args(image_size=32, use_extra_pixelwise_augs=True), part)
        again = mod.Dataset.get_dataset(aug_args(image_size=32, use_extra_pixelwise_augs=True), part)
        inference = mod.Dataset.get_dataset(aug_args(image_size=32, use_extra_pixelwise_augs=True, inference=True, **first_on), part)
        seen = {}
        for visit in range(3):
            for index in (0, 3, 4):
                p, b, a, g, i = plain[index][0], both[index][0], alone[index][0], again[index][0], inference[index][0]
                assert 'aug_params_extra' not in p and 'aug_params_extra' not in i and 'aug_params' not in i
                assert 'aug_params' not in a and set(b) == set(p) | {'aug_params_extra'} and set(a) == set(i) | {'aug_params_extra'}
                assert torch.equal(b['aug_params'], p['aug_params'])                    # bit-identical with the flag on and off
                row = b['aug_params_extra']
                assert tuple(row.shape) == (16,) and row.dtype == torch.float32
                assert torch.equal(row, a['aug_params_extra']) and torch.equal(row, g['aug_params_extra'])          # (seed, index, visit) decide
                want = AUG.ParametricAugmenter(aug_args(use_extra_pixelwise_augs=True)).sample_extra(
                    torch.Generator().manual_seed(AUG.extra_stream_seed(both.seed, index, visit if part == 'train' else 0)))
                assert torch.equal(row, want)
                seen.setdefault(index, []).append(row)
                for key in i:
                    assert torch.equal(b[key], i[key]), key                             # the images are the base loader's
        rows = torch.stack([r for v in seen.values() for r in v])
        assert (rows != 0).any()
        if part == 'val':
            assert all(torch.equal(v[0], v[1]) and torch.equal(v[0], v[2]) for v in seen.values())
        else:
            assert any(not torch.equal(v[0], v[1]) or not torch.equal(v[0], v[2]) for v in seen.values())
    batch = torch.utils.data.default_collate([both[0], both[1]])
    assert tuple(batch[0]['aug_params_extra'].shape) == (2, 16) and tuple(batch[0]['aug_params'].shape) == (2, 32)


def test_image_folder_loader_emits_the_key_only_with_the_flag(tmp_path):
    from pathlib import Path
    import test_voxceleb2_loader_cpu as V
    tree = V.build_tree(tmp_path / 'tree')
    person = Path('id00/vidA')
    common = dict(finetune=True, val_split_path=person, train_split_path=person)
    plain, _ = next(iter(V.loader_for(V.make_args(tree, use_pixelwise_augs=True, **common), 'val')))
    both, _ = next(iter(V.loader_for(V.make_args(tree, use_pixelwise_augs=True, use_extra_pixelwise_augs=True, **common), 'val')))
    alone, _ = next(iter(V.loader_for(V.make_args(tree, use_extra_pixelwise_augs=True, **common), 'val')))
    off, _ = next(iter(V.loader_for(V.make_args(tree, **common), 'val')))
    inference, _ = next(iter(V.loader_for(V.make_args(tree, use_extra_pixelwise_augs=True, inference=True, **common), 'val')))
    assert 'aug_params_extra' not in plain and 'aug_params_extra' not in off and 'aug_params' not in off
    assert 'aug_params_extra' not in inference and 'aug_params' not in inference
    assert 'aug_params' not in alone and tuple(alone['aug_params_extra'].shape) == (3, 16) and alone['aug_params_extra'].dtype == torch.float32
    assert torch.equal(both['aug_params'], plain['aug_params']) and torch.equal(both['aug_params_extra'], alone['aug_params_extra'])
    args = V.make_args(tree, use_extra_pixelwise_augs=True, **common)
    want = AUG.ParametricAugmenter(args).sample_extra(torch.Generator().manual_seed(AUG.extra_stream_seed(args.random_seed + 7919, 1, 0)))
    assert torch.equal(alone['aug_params_extra'][1], want)
    loader = V.loader_for(V.make_args(tree, batch_size=5, use_extra_pixelwise_augs=True, **common), 'train')
    first, second = next(iter(loader))[0]['aug_params_extra'], next(iter(loader))[0]['aug_params_extra']
    assert not torch.equal(first.sort(dim=0).values, second.sort(dim=0).values)          # 'train': every visit of a sample draws again


# ---- apply and TrainingModule ---------------------------------------------------------------------------------------------------------------------------
def test_apply_handles_either_key_alone_and_both():
    import test_augment_cpu as T
    from runners import holycow
    b, s = 2, 16
    g = torch.Generator().manual_seed(0)
    data = {'enc_rgbs': torch.rand(b, 2, 3, s, s, generator=g), 'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g),
            'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g)}
    target = {'real_segm': torch.rand(b, 1, 1, s, s, generator=g).expand(b, 1, 3, s, s), 'label': torch.arange(b)}
    aug = AUG.ParametricAugmenter(aug_args(image_size=s, use_pixelwise_augs=True, use_affine_scale=True, use_affine_shift=True))
    params = torch.stack([aug.sample(torch.Generator().manual_seed(4 + i)) for i in range(b)])
    extra = torch.tensor(np.stack([XR.row(alpha=2.5, seed=77, quality=80), XR.row(median=1, d=-0.06)]), dtype=torch.float32)
    first = AUG.augment_triplet_host(data['pose_input_rgbs'], params, data['target_rgbs'], target['real_segm'])
    # the new key alone: the pose image only, target and mask pass through as the same objects
    d1, t1 = AUG.apply(dict(data, aug_params_extra=extra), dict(target))
    assert torch.equal(d1['pose_input_rgbs'], AUG.augment_extra_host(data['pose_input_rgbs'], extra)) and 'aug_params_extra' not in d1
    assert tuple(d1['pose_input_rgbs'].shape) == (b, 1, 3, s, s) and not torch.equal(d1['pose_input_rgbs'], data['pose_input_rgbs'])
    assert d1['target_rgbs'] is data['target_rgbs'] and t1['real_segm'] is target['real_segm']
    # aug_params alone: what it was
    d2, t2 = AUG.apply(dict(data, aug_params=params), dict(target))
    assert torch.equal(d2['pose_input_rgbs'], first[0]) and torch.equal(d2['target_rgbs'], first[1]) and torch.equal(t2['real_segm'], first[2])
    # both: the second stage on the first stage's pose output
    d3, t3 = AUG.apply(dict(data, aug_params=params, aug_params_extra=extra), dict(target))
    assert torch.equal(d3['pose_input_rgbs'], AUG.augment_extra_host(first[0], extra)) and not torch.equal(d3['pose_input_rgbs'], first[0])
    assert torch.equal(d3['target_rgbs'], first[1]) and torch.equal(t3['real_segm'], first[2])
    assert 'aug_params' not in d3 and 'aug_params_extra' not in d3
    with pytest.raises(KeyError, match='pose_input_rgbs'):
        AUG.apply({'aug_params_extra': extra}, {})
    # TrainingModule.forward triggers on either key
    E, G = T._Embedder(), T._Generator()
    tm = holycow.TrainingModule(E, G, T._Critic(), [T._Criterion()], [], running_averages=None)
    all_data, lg, ld = tm(dict(data, aug_params_extra=extra), dict(target))
    assert torch.equal(E.seen, d1['pose_input_rgbs']) and 'aug_params_extra' not in all_data and all_data['target_rgbs'] is data['target_rgbs']
    all_data, lg, ld = tm(dict(data, aug_params=params, aug_params_extra=extra), dict(target))
    assert torch.equal(E.seen, d3['pose_input_rgbs']) and torch.equal(all_data['target_rgbs'], first[1])
    all_data, lg, ld = tm(dict(data), dict(target))
    assert E.seen is data['pose_input_rgbs']


# ---- refusals, without device work ------------------------------------------------------------------------------------------------------------------------
def test_c_entry_point_validates_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    st = (ctypes.c_longlong * 4)(768, 256, 16, 1)
    sp, fake = ctypes.addressof(st), 4096          # (never dereferenced: every call below is refused first)
    f = l.lp_augment_extra
    assert f(None, sp, fake, 1, 3, 16, 16, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, None, fake, 1, 3, 16, 16, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, None, 1, 3, 16, 16, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, fake, 1, 3, 16, 16, None, None) == -1 and b'null' in l.lp_last_error()
    assert f(fake, sp, fake, 0, 3, 16, 16, fake, None) == -1 and b'B >= 1' in l.lp_last_error()
    for c in (0, 1, 2, 4):
        assert f(fake, sp, fake, 1, c, 16, 16, fake, None) == -1 and b'C must be 3' in l.lp_last_error()
    assert f(fake, sp, fake, 1, 3, 0, 16, fake, None) == -1 and b'H >= 1' in l.lp_last_error()
    assert f(fake, sp, fake, 1, 3, 16, 0, fake, None) == -1 and b'W >= 1' in l.lp_last_error()
    assert f(fake, sp, fake, 70000, 3, 16, 16, fake, None) == -2 and b'grid' in l.lp_last_error()
    assert f(fake, sp, fake, 1, 3, 16 * 65536, 16, fake, None) == -2 and b'grid' in l.lp_last_error()


def test_wrapper_refuses_inputs_off_the_gpu_and_malformed_ones_first():
    from latent_pose_reenactment_amd import hipops as ops
    x, p = torch.zeros(2, 3, 8, 8), torch.zeros(2, 16)
    with pytest.raises(ValueError, match='CUDA'):
        ops.augment_extra(x, p)
    with pytest.raises(ValueError, match='pose must be fp32'):
        ops.augment_extra(x.double(), p)
    with pytest.raises(ValueError, match='params_extra must be fp32'):
        ops.augment_extra(x, p.half())
    for width in (15, 17, 32):
        with pytest.raises(ValueError, match=r'params_extra must be \[B, 16\]'):
            ops.augment_extra(x, torch.zeros(2, width))
    with pytest.raises(ValueError, match=r'params_extra must be \[B, 16\]'):
        ops.augment_extra(x, torch.zeros(3, 16))
    for c in (1, 4):
        with pytest.raises(ValueError, match='3 channels'):
            ops.augment_extra(torch.zeros(2, c, 8, 8), p)
        with pytest.raises(ValueError, match='3 channels'):
            AUG.augment_extra_host(torch.zeros(2, c, 8, 8), p)
    with pytest.raises(ValueError, match=r'\[B, 3, H, W\]'):
        ops.augment_extra(torch.zeros(3, 8, 8), p)
    with pytest.raises(ValueError, match='mismatch.*out'):
        ops.augment_extra(x, p, out=torch.zeros(2, 3, 8, 9))
    with pytest.raises(ValueError, match='out must be contiguous'):
        ops.augment_extra(x, p, out=torch.zeros(2, 3, 8, 16)[..., ::2])
    with pytest.raises(ValueError, match='launch grid'):
        ops.augment_extra(torch.zeros(1, 3, 16 * 65536, 1), torch.zeros(1, 16))
    with pytest.raises(ValueError, match='must be a tensor'):
        ops.augment_extra(x, [0.0] * 16)


def test_abi_tests_hold_with_the_new_symbol():
    import test_abi
    assert 'lp_augment_extra' in test_abi.parse_header()
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_ctypes_signatures_match_header()
