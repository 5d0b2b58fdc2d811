"""``train.py --visuals`` on the MI355X, toy geometry (the arguments of tests/test_train_entry_gpu.py):
  (e) the visual forward does not disturb training: runs with ``--visuals --log_frequency_images 1`` and without, from the same seed, end in the same
      ``state_dict`` of embedder, generator, discriminator and both running averages -- eager (3 iterations) and with ``--hip_graph`` (5 iterations:
      three eager warm-up steps, the capture, one replay).  The plain configuration runs twice first: the pair is held to the largest relative
      difference the two plain runs show, nothing beyond it (0, i.e. bit-identical, where the plain step is bit-reproducible);
  (f) the PNGs exist and decode to [Hc + n H, P W, 3] with the expected panels, for the latent-pose family and for ``--generator FSTH`` (no
      ``fake_segm``); the generator-output block of the last sheet is ``visual_sheet_host`` of the ``fake_rgbs`` the same running-average forward gives
      when run again; the other-person output of sample i is what driving with the pose input of sample i - 1 gives; with ``--finetune`` set, or
      one sample, the group is absent.
Each configuration is one train.py process, shared by the tests that read it.
Measured on one MI355X: plain against plain 0 and plain against --visuals 0 (every tensor bit-identical), eager and --hip_graph (``[visuals]`` lines)."""
import os
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

FSTH = ['--embedder', 'FSTH', '--generator', 'FSTH', '--discriminator', 'FSTH', '--criterions', 'adversarial, featmat, l1_rgb', '--runner', 'holycow',
        '--dataloader', 'synthetic_voxceleb2_stickmen', '--image_size', '64', '--num_channels', '8', '--max_num_channels', '32',
        '--embed_channels', '16', '--num_labels', '20', '--dis_num_blocks', '5', '--embed_num_blocks', '4', '--gen_num_downsample_blocks', '3',
        '--gen_num_residual_blocks', '1', '--batch_size', '2', '--synthetic_dataset_len', '4', '--n_frames_for_encoder', '2', '--num_epochs', '1',
        '--num_gpus', '1']

# train.py with the visual forward of the LAST logged iteration run again behind it: what it returns, the same drive done by hand with an explicit
# index instead of ``roll``, and the two cases without an other-person group
DRIVER = '''
import copy, os, sys
sys.path.insert(0, {pkg!r})
import torch
import train
import runners.holycow as H
from latent_pose_reenactment_amd.utils import visualize as V
inner = H.log_visuals
def log_visuals(tm, data, target, args):
    path = inner(tm, data, target, args)
    if args.iteration != {last}:
        return path
    again = H.visual_forward(tm, data, target, args)
    avg = tm.running_averages
    b = again['fake_rgbs'].shape[0]
    idx = [b - 1] + list(range(b - 1))
    d = dict(again)
    for k in H.CROSS_DRIVING_KEYS:
        if torch.is_tensor(d.get(k)):
            d[k] = d[k][idx]
    with torch.no_grad():
        avg['embedder'].get_pose_embedding(d)
        avg['generator'](d)
    ft = copy.copy(args)
    ft.finetune = True
    keys_ft = sorted(k for k in H.visual_forward(tm, data, target, ft) if k.endswith('_other_person'))
    keys_one, error_one = None, None
    if {one_sample}:
        try:
            one = H.visual_forward(tm, {{k: (v[:1] if torch.is_tensor(v) else v) for k, v in data.items()}},
                                   {{k: (v[:1] if torch.is_tensor(v) else v) for k, v in target.items()}}, args)
            keys_one = sorted(k for k in one if k.endswith('_other_person'))
        except Exception as e:
            error_one = repr(e)
    shown = dict(again)
    shown.pop('dec_stickmen', None)
    keep = ('fake_rgbs', 'fake_rgbs_other_person', 'pose_input_rgbs', 'pose_input_rgbs_other_person', 'fake_segm')
    torch.save({{'again': {{k: again[k].float().cpu() for k in keep if k in again}}, 'cross': d['fake_rgbs'].float().cpu(), 'keys': sorted(again),
                'captions': [c for c, _ in V.make_visual(shown, args.num_visuals_per_img)], 'keys_ft': keys_ft, 'keys_one': keys_one,
                'error_one': error_one, 'training': tm.training, 'toggles': (tm.use_running_averages, tm.compute_losses)}}, {dump!r})
    return path
H.log_visuals = log_visuals
train.main()
'''

RUNS = {}


def run(tmp, name, family_args, extra, driver_last=None, one_sample=False):
    """one train.py process per name -> (checkpoint, experiment directory, dump of the driver | None)"""
    if name in RUNS:
        return RUNS[name]
    script, dump = os.path.join(PKG, 'train.py'), None
    if driver_last is not None:
        dump = str(tmp / f'{name}_dump.pt')
        script = str(tmp / f'{name}_driver.py')
        with open(script, 'w') as f:
            f.write(DRIVER.format(pkg=PKG, last=driver_last, dump=dump, one_sample=one_sample))
    cmd = [sys.executable, script] + family_args + ['--experiments_dir', str(tmp), '--experiment_name', name, '--log_frequency_loss', '1'] + extra
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    ckpt_dir = os.path.join(str(tmp), name, 'checkpoints')
    ckpt = torch.load(os.path.join(ckpt_dir, sorted(os.listdir(ckpt_dir))[-1]), map_location='cpu', weights_only=False)
    RUNS[name] = (ckpt, tmp / name, None if dump is None else torch.load(dump))
    return RUNS[name]


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp('visuals')


def latent_args(iterations):
    from test_train_entry_gpu import COMMON
    args = list(COMMON)
    args[args.index('--synthetic_dataset_len') + 1] = str(4 * iterations)          # batch 4
    return args


def states(ckpt):
    out = {}
    for part in ('embedder', 'generator', 'discriminator'):
        out.update({f'{part}.{k}': v for k, v in ckpt[part].items() if torch.is_tensor(v)})
    for part, sd in ckpt['running_averages'].items():
        out.update({f'running_averages.{part}.{k}': v for k, v in sd.items() if torch.is_tensor(v)})
    return out


def largest_relative_difference(a, b):
    """max over the tensors of max |a - b| / max |a| (0 for two tensors that are bit-identical), and the tensor that gives it"""
    assert set(a) == set(b)
    worst, where = 0.0, None
    for k in a:
        if torch.equal(a[k], b[k]):
            continue
        x, y = a[k].double(), b[k].double()
        d = float((x - y).abs().max() / x.abs().max().clamp_min(1e-30))
        d = d if d == d else float('inf')
        if d >= worst:
            worst, where = d, k
    return worst, where


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['eager', 'hip_graph'])
def test_visuals_leave_the_training_trajectory_alone(tmp, mode):
    iterations = 3 if mode == 'eager' else 5
    extra = [] if mode == 'eager' else ['--hip_graph']
    plain = states(run(tmp, f'{mode}_plain', latent_args(iterations), extra)[0])
    plain2 = states(run(tmp, f'{mode}_plain2', latent_args(iterations), extra)[0])
    ckpt, exp, _ = run(tmp, f'{mode}_visuals', latent_args(iterations), extra + ['--visuals', '--log_frequency_images', '1'],
                       driver_last=iterations - 1 if mode == 'eager' else None)
    assert ckpt['args'].iteration == iterations and ckpt['args'].visuals is True
    assert len(plain) > 100 and any(k.startswith('running_averages.generator.') for k in plain)
    noise, noisy = largest_relative_difference(plain, plain2)
    got, where = largest_relative_difference(plain, states(ckpt))
    print(f'[visuals] {mode}, {iterations} iterations: plain vs plain {noise:.3e} ({noisy}); plain vs --visuals {got:.3e} ({where})')
    assert got <= noise, (mode, got, where, noise, noisy)
    assert sorted(os.listdir(exp / 'visuals')) == [f'train_{i:08}.png' for i in range(iterations)]


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------------------------------
def check_sheets(exp, dump, iterations, size, n_shown, captions):
    from PIL import Image
    from latent_pose_reenactment_amd import hipops as ops
    from latent_pose_reenactment_amd.utils import visualize as V
    assert dump['captions'] == captions and dump['training'] is True and dump['toggles'] == (False, True)
    hc, count = V.caption_height(size), len(captions)
    files = sorted(os.listdir(exp / 'visuals'))
    assert files == [f'train_{i:08}.png' for i in range(iterations)]
    sheets = [np.asarray(Image.open(exp / 'visuals' / f)) for f in files]
    for s in sheets:
        assert s.shape == (hc + n_shown * size, count * size, 3) and s.dtype == np.uint8
        assert np.array_equal(s[:hc, :, 0], V.caption_strip(captions, size, hc).numpy()) and np.array_equal(s[:hc, :, 0], s[:hc, :, 2])
    assert not np.array_equal(sheets[0][hc:], sheets[-1][hc:])
    last = sheets[-1][hc:]
    again = dump['again']

    def block(p):
        return last[:, p * size:(p + 1) * size]
    same = captions.index('Generator output')
    assert np.array_equal(block(same), ops.visual_sheet_host([again['fake_rgbs'][:n_shown]]).numpy())
    assert np.array_equal(block(captions.index('Pose input (same video)')), ops.visual_sheet_host([again['pose_input_rgbs'][:n_shown, 0]]).numpy())
    # the other-person group: sample i driven by the pose input of sample i - 1
    b = again['fake_rgbs'].shape[0]
    idx = [b - 1] + list(range(b - 1))
    assert captions[-2:] == ['Pose input (other person)', 'Generator output']
    assert torch.equal(again['pose_input_rgbs_other_person'], again['pose_input_rgbs'][idx])
    assert torch.equal(again['fake_rgbs_other_person'], dump['cross']) and not torch.equal(dump['cross'], again['fake_rgbs'])
    assert np.array_equal(block(count - 1), ops.visual_sheet_host([dump['cross'][:n_shown]]).numpy())
    assert np.array_equal(block(count - 2), ops.visual_sheet_host([again['pose_input_rgbs'][idx][:n_shown, 0]]).numpy())
    assert dump['keys_ft'] == []
    return last


def test_sheets_of_the_latent_pose_family(tmp):
    from latent_pose_reenactment_amd import hipops as ops
    _, exp, dump = run(tmp, 'eager_visuals', latent_args(3), ['--visuals', '--log_frequency_images', '1'], driver_last=2)
    captions = ['Identity src', 'Pose target (same video)', 'Pose input (same video)', 'Generator output', 'Predicted segmentation',
                'Pose input (other person)', 'Generator output']
    last = check_sheets(exp, dump, 3, 128, 2, captions)
    assert tuple(dump['again']['fake_segm'].shape) == (4, 1, 128, 128)
    assert np.array_equal(last[:, 4 * 128:5 * 128], ops.visual_sheet_host([dump['again']['fake_segm'][:2]]).numpy())
    assert dump['keys'].count('real_segm') == 0          # (the visual forward's only target is the label, as in the reference)


def test_sheets_of_the_fsth_family_and_of_one_sample(tmp):
    _, exp, dump = run(tmp, 'fsth_visuals', FSTH, ['--visuals', '--log_frequency_images', '1', '--num_visuals_per_img', '3'], driver_last=1,
                       one_sample=True)
    captions = ['Identity src', 'Pose target (same video)', 'Pose input (same video)', 'Generator output',
                'Pose src (other person)', 'Pose input (other person)', 'Generator output']
    assert 'fake_segm' not in dump['keys'] and 'dec_stickmen_other_person' in dump['keys']
    check_sheets(exp, dump, 2, 64, 2, captions)          # three samples asked for, the batch has two
    assert dump['error_one'] is None and dump['keys_one'] == [], dump['error_one']
