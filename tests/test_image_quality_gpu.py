"""GPU checks of the image-quality metric (csrc/image_quality.hip -> hipops.image_quality -> metrics/image_quality.py -> run_epoch):
  * the kernel against the fp64 restatement (tests/image_quality_restatement.py): one window (11 x 11), sizes below, at and above one 16 x 16 tile
    of windows, ragged last tiles in either direction, 256 x 256; B 1 and 3; C 3 and 1; six input pairs x four masks; contiguous tensors, the
    target as ``[:, 0]`` of a 5-D tensor, the image as a crop of a wider tensor, the mask as the stride-0 ``expand`` of a B x 1 x 1 x H x W tensor.
    Gates (set by the issue that introduced the metric):
        ssim, ssim_fg   abs error <= 5e-4   each second-moment term carries a few 2^-24 of absolute error against C2 = 9e-4: <= 2.6e-4 on exactly
                                            flat windows for the plain f(x^2) - mx^2 form, the gate is twice that
        psnr, psnr_fg   abs error <= 1e-3 dB   4.34 x the relative error of an fp32 sum of non-negative terms
        l1, l1_fg       rel error <= 1e-5      the gate of the l1_rgb criterion's test
    An identical pair gives exactly (1, 100, 0); two runs are bit-identical; an image whose mask is all zero has NaN in its _fg columns only.
  * the plugin on a batch shaped like the training step's, with and without ``--image_quality_foreground``;
  * two iterations of train.py with ``--metrics image_quality``: the epoch meter carries the six ``Metric_*`` keys, all finite, and ``Metric_ssim``
    equals the restatement on the last step's batch within the gate.
Every case prints its measured errors (``[image_quality]`` lines).  Measured on one MI355X: ssim / ssim_fg worst 2.3e-5 (27 x 27, the pair whose
upper half is black: black windows of a tile whose pivot is a bright pixel; <= 4.3e-7 on the other five input pairs), psnr / psnr_fg worst 5.5e-6 dB,
l1 / l1_fg worst 2.1e-7 relative; train.py's Metric_ssim 4.7e-8 from the restatement."""
import argparse
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'latent_pose_reenactment_amd')
for p in (PKG, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
pytestmark = pytest.mark.gpu

import image_quality_restatement as IQ          # noqa: E402

GATE_SSIM, GATE_PSNR, GATE_L1 = 5e-4, 1e-3, 1e-5
INPUTS = ('noise', 'smooth+noise', 'identical', 'flat', 'upper-half-black', 'out-of-range')
MASKS = ('none', 'ones', 'soft', 'soft+one-empty')


def make_pair(kind, b, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == 'noise':
        return torch.rand(b, c, h, w, generator=g), torch.rand(b, c, h, w, generator=g)
    if kind == 'smooth+noise':
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing='ij')
        ph = torch.rand(b, c, 1, 1, generator=g) * 6.0
        y = 0.5 + 0.4 * torch.sin(0.21 * xs + 0.13 * ys + ph)
        return y + 0.02 * torch.randn(b, c, h, w, generator=g), y
    if kind == 'identical':
        x = torch.rand(b, c, h, w, generator=g)
        return x, x.clone()
    if kind == 'flat':
        return torch.full((b, c, h, w), 0.7), torch.full((b, c, h, w), 0.701)
    if kind == 'upper-half-black':
        x, y = torch.rand(b, c, h, w, generator=g), torch.rand(b, c, h, w, generator=g)
        x[:, :, :h // 2] = 0.0
        y[:, :, :h // 2] = 0.0
        return x, y
    if kind == 'out-of-range':
        return torch.rand(b, c, h, w, generator=g) * 2 - 0.5, torch.rand(b, c, h, w, generator=g) * 2 - 0.5
    raise KeyError(kind)


def make_mask(kind, b, h, w):
    if kind == 'none':
        return None
    if kind == 'ones':
        return torch.ones(b, h, w)
    xs = torch.arange(w, dtype=torch.float32)[None, :].expand(h, w)
    ys = torch.arange(h, dtype=torch.float32)[:, None].expand(h, w)
    m = ((xs - 0.35 * ys) / (0.5 * w)).clamp(0.0, 1.0)[None].repeat(b, 1, 1)          # a soft half-plane in [0, 1]
    if kind == 'soft+one-empty':
        m[b - 1] = 0.0
    return m.contiguous()


def errors(got, want):
    """-> (ssim abs, psnr abs, l1 rel) maxima over the images and over both column triples; NaNs must sit in the same places"""
    got = got.detach().cpu().double()
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
    ok = ~torch.isnan(want)
    e = [0.0, 0.0, 0.0]
    for col in range(6):
        g, w_ = got[:, col][ok[:, col]], want[:, col][ok[:, col]]
        if g.numel() == 0:
            continue
        d = (g - w_).abs()
        if col % 3 == 2:
            d = torch.where(w_ == 0, torch.where(g == 0, torch.zeros_like(d), torch.full_like(d, math.inf)), d / w_.abs().clamp_min(1e-300))
        e[col % 3] = max(e[col % 3], d.max().item())
    return tuple(e)


def bits(t):
    return t.contiguous().view(torch.int32)


def check_case(kind, mkind, b, c, h, w, seed, layouts=True):
    from latent_pose_reenactment_amd import hipops as ops
    x, y = make_pair(kind, b, c, h, w, seed)
    m = make_mask(mkind, b, h, w)
    want = IQ.table(x, y, m)
    xd, yd, md = x.cuda(), y.cuda(), None if m is None else m.cuda()
    got = ops.image_quality(xd, yd, md)
    again = ops.image_quality(xd, yd, md)
    assert tuple(got.shape) == (b, 6) and got.dtype == torch.float32 and got.is_cuda
    assert torch.equal(bits(got), bits(again))          # run to run
    if layouts:
        y5 = torch.stack([yd, torch.rand_like(yd)], 1)                                        # B x 2 x C x H x W: frame 0 is the target
        wide = torch.full((b, c, h + 3, w + 5), 0.25, device='cuda')
        wide[:, :, 1:1 + h, 2:2 + w] = xd
        mv = None
        if md is not None:
            mv = md.reshape(b, 1, 1, h, w).expand(b, 1, 3, h, w)[:, 0, 1]                     # a channel of the stride-0 expand: no copy
            assert mv.data_ptr() == md.data_ptr() and tuple(mv.shape) == (b, h, w)
        strided = ops.image_quality(wide[:, :, 1:1 + h, 2:2 + w], y5, mv)
        assert torch.equal(bits(strided), bits(got))    # the layout changes nothing
    e = errors(got, want)
    print(f'[image_quality] {h}x{w} B {b} C {c} {kind} / mask {mkind}: ssim abs {e[0]:.2e} (gate {GATE_SSIM:.0e}), psnr abs {e[1]:.2e} dB '
          f'(gate {GATE_PSNR:.0e}), l1 rel {e[2]:.2e} (gate {GATE_L1:.0e})')
    assert e[0] <= GATE_SSIM and e[1] <= GATE_PSNR and e[2] <= GATE_L1, (kind, mkind, e, got, want)
    if mkind == 'none':
        assert bool(torch.isnan(got[:, 3:]).all()) and not bool(torch.isnan(got[:, :3]).any())
    if mkind == 'soft+one-empty':
        assert bool(torch.isnan(got[b - 1, 3:]).all()) and not bool(torch.isnan(got[b - 1, :3]).any())
        assert not bool(torch.isnan(got[:b - 1]).any())
    if kind == 'identical':
        assert got[:, :3].cpu().tolist() == [[1.0, 100.0, 0.0]] * b, got
        if mkind == 'ones':
            assert got[:, 3:].cpu().tolist() == [[1.0, 100.0, 0.0]] * b, got
    return e


# ---- kernel ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 3])
@pytest.mark.parametrize('h,w', [(11, 11), (12, 12), (16, 16), (27, 27), (43, 43), (13, 40), (64, 64)])
def test_kernel_vs_fp64_restatement(h, w, b):
    worst = [0.0, 0.0, 0.0]
    for i, kind in enumerate(INPUTS):
        for j, mkind in enumerate(MASKS):
            e = check_case(kind, mkind, b, 3, h, w, seed=1000 * h + 10 * w + b + 100 * i + j)
            worst = [max(a, v) for a, v in zip(worst, e)]
    print(f'[image_quality] {h}x{w} B {b}: worst ssim abs {worst[0]:.2e}, psnr abs {worst[1]:.2e} dB, l1 rel {worst[2]:.2e}')


def test_kernel_one_channel():
    for kind in INPUTS:
        check_case(kind, 'soft+one-empty', 3, 1, 27, 27, seed=5)
    check_case('noise', 'none', 3, 1, 27, 27, seed=6)


def test_kernel_256():
    check_case('smooth+noise', 'soft+one-empty', 3, 3, 256, 256, seed=7)
    check_case('flat', 'ones', 1, 3, 256, 256, seed=8, layouts=False)
    check_case('identical', 'none', 1, 3, 256, 256, seed=9, layouts=False)


# ---- plugin -------------------------------------------------------------------------------------------------------------------------------------------
def step_batch(b, s, seed):
    g = torch.Generator().manual_seed(seed)
    segm = make_mask('soft+one-empty', b, s, s).reshape(b, 1, 1, s, s)
    real = torch.rand(b, 1, 3, s, s, generator=g) * segm
    fake = (real[:, 0] + 0.1 * torch.randn(b, 3, s, s, generator=g))
    return {'fake_rgbs': fake.cuda(), 'target_rgbs': real.cuda(), 'real_segm': segm.cuda().expand(b, 1, 3, s, s)}


def test_plugin_on_a_step_batch():
    from utils.utils import load_wrappers_for_module_list
    from latent_pose_reenactment_amd import hipops as ops
    wrapper = load_wrappers_for_module_list('image_quality', 'metrics')[0]
    b, s = 3, 32
    batch = step_batch(b, s, 11)
    table = ops.image_quality(batch['fake_rgbs'], batch['target_rgbs'], batch['real_segm'][:, 0, 0]).cpu()
    net = wrapper.get_net(argparse.Namespace(image_quality_foreground=True, device='cuda'))
    values, counts = net(dict(batch, fake_rgbs=batch['fake_rgbs'].clone().requires_grad_(True)))          # (a live autograd leaf, as in the step)
    assert list(values) == list(ops.IMAGE_QUALITY_COLUMNS) == list(IQ.COLUMNS) and set(counts) == set(values)
    for k, name in enumerate(ops.IMAGE_QUALITY_COLUMNS):
        col = table[:, k]
        col = col[col == col]
        assert counts[name] == (b if k < 3 else b - 1) == col.numel(), (name, counts)
        assert values[name] == float(col.mean()) and isinstance(values[name], float), (name, values[name])
    want = IQ.table(batch['fake_rgbs'], batch['target_rgbs'], batch['real_segm'][:, 0, 0])
    e = errors(table, want)
    print(f'[image_quality] plugin batch {b} x 3 x {s} x {s}: ssim abs {e[0]:.2e}, psnr abs {e[1]:.2e} dB, l1 rel {e[2]:.2e}; values {values}')
    assert e[0] <= GATE_SSIM and e[1] <= GATE_PSNR and e[2] <= GATE_L1
    # the flag off, or a batch without real_segm: the whole-frame keys only
    plain = wrapper.get_net(argparse.Namespace(image_quality_foreground=False, device='cuda'))
    v2, c2 = plain(batch)
    assert list(v2) == ['ssim', 'psnr', 'l1'] and c2 == {'ssim': b, 'psnr': b, 'l1': b}
    assert all(v2[k] == values[k] for k in v2)
    v3, c3 = net({k: v for k, v in batch.items() if k != 'real_segm'})
    assert v3 == v2 and c3 == c2
    # every image without foreground: the _fg keys are there with count 0 (Meter.add skips them)
    v4, c4 = net(dict(batch, real_segm=torch.zeros_like(batch['real_segm'])))
    assert [c4[k] for k in ops.IMAGE_QUALITY_COLUMNS] == [b, b, b, 0, 0, 0] and all(math.isnan(v4[k]) for k in ('ssim_fg', 'psnr_fg', 'l1_fg'))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------------
DRIVER = '''
import os, sys
sys.path.insert(0, {pkg!r})
import torch
import train
import runners.holycow as H
inner = H.TrainingModule.compute_metrics
def compute_metrics(self, data_dict):
    torch.save({{k: data_dict[k].detach().float().cpu().clone() for k in ('fake_rgbs', 'target_rgbs', 'real_segm')}}, {dump!r})
    return inner(self, data_dict)
H.TrainingModule.compute_metrics = compute_metrics
train.main()
'''


def test_train_entry_reports_the_metrics(tmp_path):
    from test_train_entry_gpu import COMMON
    args = list(COMMON)
    args[args.index('--synthetic_dataset_len') + 1] = '8'          # batch 4: two iterations
    dump = str(tmp_path / 'last_all_data.pt')
    driver = tmp_path / 'drive_train.py'
    driver.write_text(DRIVER.format(pkg=PKG, dump=dump))
    cmd = [sys.executable, str(driver)] + args + ['--experiments_dir', str(tmp_path), '--experiment_name', 'iq', '--metrics', 'image_quality',
                                                   '--log_frequency_loss', '1']
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if 'Epoch 0 (iteration 2)' in l][-1]
    last = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Metric_\w+) ([-+.\deEnaif]+) \(avg', line)}
    avg = {m.group(1): float(m.group(2)) for m in re.finditer(r'(Metric_\w+) [-+.\deEnaif]+ \(avg ([-+.\deEnaif]+)\)', line)}
    assert set(last) == {f'Metric_{k}' for k in IQ.COLUMNS} == set(avg), line
    assert all(math.isfinite(v) for v in last.values()) and all(math.isfinite(v) for v in avg.values()), line
    d = torch.load(dump)
    assert tuple(d['fake_rgbs'].shape) == (4, 3, 128, 128) and tuple(d['real_segm'].shape) == (4, 1, 3, 128, 128)
    want = IQ.table(d['fake_rgbs'], d['target_rgbs'], d['real_segm'][:, 0, 0]).mean(0)          # (every synthetic image has foreground)
    err = {k: abs(last[f'Metric_{k}'] - want[i].item()) for i, k in enumerate(IQ.COLUMNS)}
    print(f'[image_quality] train.py, last of two iterations: {last}; abs error against the restatement {err}')
    # the log line prints six significant digits: half a unit of the sixth digit on top of the gate
    assert err['ssim'] <= GATE_SSIM + 5e-6 * abs(want[0].item()), (last, want)
    assert err['ssim_fg'] <= GATE_SSIM + 5e-6 * abs(want[3].item()), (last, want)
    assert err['psnr'] <= GATE_PSNR + 5e-6 * abs(want[1].item()) and err['psnr_fg'] <= GATE_PSNR + 5e-6 * abs(want[4].item()), (last, want)
    assert err['l1'] <= (GATE_L1 + 5e-6) * abs(want[2].item()) and err['l1_fg'] <= (GATE_L1 + 5e-6) * abs(want[5].item()), (last, want)
