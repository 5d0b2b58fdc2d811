"""lp_augment_extra on the MI355X (``hipops.augment_extra``: elastic, median, saturation and JPEG of the pose image in one launch) against the fp64
restatement (tests/augment_extra_restatement.py), the bit-exact properties of the definition, capture, the captured training step and train.py.

Case list (tests/test_augment_extra_cpu.py ``cases``): (H, W) in {8 x 8, 16 x 16, 20 x 24, 33 x 18, 64 x 64} -- below one tile, one tile, partial
JPEG blocks, tile tails in both axes, W % 4 != 0 (the scalar store path) -- x B in {1, 3} x {contiguous input, ``[:, 0]`` view of a
[B, 2, 3, H, W] tensor, ``out=`` a slice of a larger buffer}; every step ALONE on inputs made for it: elastic alpha 0.5 and 3.5 on noise (at 3.5 the
displacement leaves the frame at the border: checked below), the median on an image of five values (every window repeats some), saturation
d = +-20/255 and 7/255 on noise with exact grey, black and white pixels and S = 0.05, 0.078, 0.08 around s0 = 20/255 = 0.0784, JPEG at 70, 85, 95 on
smooth images; then one row with all four steps and 32 rows from ``sample_extra`` at 64 x 64.

Gates, u = 2^-24, U = 2^-23, S = max(H, W); all max-abs against the restatement of the SAME fp32 inputs and rows:
  elastic   (8 S + 8) U, the bilinear bound of tests/test_augment_gpu.py with Amp 1: the source coordinate x + alpha u(j) is one product (< 4, error
            <= U) and one sum of magnitude <= S + 4 (error <= S u), far inside the 4 ulp(S) allowed there; it enters a bilinear weight that multiplies
            a pixel difference <= 1, on two axes; + 8 U for the interpolation's own roundings.  Continuous in the coordinate: no masking.
  median    the gate of its input, Amp 1: a median is 1-Lipschitz in the sup norm (each order statistic is) and the selection network rounds nothing.
            Alone it is exact (gate 0): an fp32 selection of fp32 values.
  saturation  L e + 8 U, e = the gate of its input, L = 3 + s0.  With r = (M - c) / (M - m) in [0, 1]:
            S < s0: g = g0 = clamp01(s0 + d) / s0 in [0, 2] is constant, c' = (1 - g0) M + g0 c, sum of |partials| = |1 - g0| + g0 <= 3;
            S >= s0, unclamped: c' = c - d h, h = M (M - c) / (M - m); |dh/dc| = 1 / S, |dh/dm| = r / S, |dh/dM| = r + (1 - r) / S, sum <= 2 / S + 1, so
              the sum for c' is <= 1 + |d| (2 / S + 1) <= 1 + s0 (2 / s0 + 1) = 3 + s0 for |d| <= s0 (the column's range: the gate refuses others);
            clamped to 1 (S >= 1 - s0): c' = M - h, sum = 2 / S - 1 + r <= 2 / (1 - s0) < 3; clamped to 0: c' = M, sum 1.
            The map is continuous across the pieces (t = max(S, s0) and the clamp are; in S >= s0, 0 <= h <= M, so it is at M -> 0 too), so L holds
            globally.  Own roundings, exact inputs: S 2u (relative), t 2u, t + d (3 + |d| / t) u <= 4 u absolute, g 4u + 3u g <= 10 u,
            (M - c) g <= 14 u, the last subtraction u: 15 u < 8 U.  As (c1 S + c2) U Amp: c1 = 8 behind an elastic step and 0 otherwise, Amp = L.
  JPEG      rounds, so a coefficient within tau of a half-integer step may land on either side.  Error of a coefficient before the rounding, in
            255-units: delta = 8 x 255 e + 2^-9, e = the gate of the step's input.  8 = (sum_n |C[0][n]|)^2 = (2 sqrt 2)^2 is the largest sup-norm gain
            of the 2-D DCT (the other rows of C sum to 2.56 .. 2.61).  2^-9 for exact inputs: 255 v and the colour transform, 3 products with rounded
            constants, 2 sums <= 255 and the shift: 5.5 x 255 u per plane value, x 8 = 6.7e-4; the row pass, 8 products and sums and a rounded
            basis entry: 9 u sum|C||x| <= 9 u x 2.83 x 128 = 1.94e-4, x 2.83 through the column pass, + the column pass's own 9 u x 2.83 x 362 =
            5.5e-4: 1.1e-3; together 1.77e-3 < 2^-9 = 1.95e-3.  tau = delta / q.  WHICH coefficients sit within tau of a half-integer step is read
            from the fp64 restatement alone.  A block without one has the SAME quantised coefficients on both sides, exactly, so its error is the
            inverse transform's: values <= 1024 x 2.83 after the column pass, 9 u x 2896 x 2.83 + 9 u x 8192 = 2 x 9 x 8192 u, + 2048 u for the colour
            transform, / 255: 3.5e-5, whatever went before.  A block with flagged coefficients gets, on top, one step q of each times the basis
            amplitude (<= 1 / 4) times the plane's largest weight in an RGB channel (1, 1.772, 1.402), / 255: a wrong block cannot hide behind it.
            No case may flag more than 1 / 8 of its 8 x 8 pixel blocks (a block counts when ANY plane has a flagged coefficient); the inputs and
            the rows are chosen so (augment_extra_restatement.JPEG_SEED, test_augment_extra_cpu.sampled_rows) and the CPU test checks it.
The fp32 host implementation sits inside all of this (tests/test_augment_extra_cpu.py).  Measured on one MI355X, worst error / gate: elastic 0.044,
median 0, saturation 0.10, JPEG 0.005 with at most 10.9 % of a case's blocks flagged, the chain 0.087 with 7.2 % flagged (README, "Second stage").

The train.py runs use the geometry of tests/test_augment_gpu.py (128 x 128, batch 4; five iterations with ``--hip_graph``: three run eagerly, then
the capture and a replay)."""
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

import augment_extra_restatement as XR          # noqa: E402
import test_augment_extra_cpu as XC          # noqa: E402
from latent_pose_reenactment_amd import augmentation as AUG          # noqa: E402

GUARD = 7.0


def through_view(pose, par):
    """the input as the ``[:, 0]`` view of a [B, 2, 3, H, W] tensor (taken ON the device: a copy to it would materialise the view)"""
    from latent_pose_reenactment_amd import hipops as ops
    wide = torch.full((pose.shape[0], 2) + tuple(pose.shape[1:]), GUARD, device='cuda')
    wide[:, 0] = pose
    view = wide[:, 0]
    assert view.stride(0) == 2 * pose[0].numel() and view.data_ptr() == wide.data_ptr()
    return ops.augment_extra(view, par)


def into_slice(pose, par):
    """``out=`` the middle of a larger buffer, offset by ONE float (so never 16-byte aligned: the scalar stores), guard values around it"""
    from latent_pose_reenactment_amd import hipops as ops
    n = pose.numel()
    buf = torch.full((n + 2 * 5,), GUARD, device='cuda')
    out = buf[5:5 + n].view(pose.shape)
    assert out.data_ptr() % 16 != 0
    res = ops.augment_extra(pose, par, out=out)
    assert res is out and bool((buf[:5] == GUARD).all()) and bool((buf[5 + n:] == GUARD).all())
    return res


# ---- against the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('layout', ['contiguous', 'view', 'out_slice'])
@pytest.mark.parametrize('h,w', XR.SIZES)
def test_kernel_against_the_restatement(h, w, layout):
    from latent_pose_reenactment_amd import hipops as ops
    fn = {'contiguous': ops.augment_extra, 'view': through_view, 'out_slice': into_slice}[layout]
    worst, flagged = XC.check_against_restatement(fn, h, w, device='cuda')
    assert all(v <= 1.0 for v in worst.values()), worst
    assert worst['neutral'] == 0.0 and worst['median'] == 0.0
    assert all(v <= XC.CAP for v in flagged.values()), flagged


def test_all_steps_together_on_sampled_rows():
    from latent_pose_reenactment_amd import hipops as ops
    worst, share = XC.check_chain(ops.augment_extra, device='cuda')
    assert worst <= 1.0 and share <= XC.CAP, (worst, share)


def test_elastic_case_leaves_the_frame():
    """at alpha = 3.5 some source coordinates of the elastic cases lie outside the frame on every side, so the border rule is exercised"""
    big = XR.step_rows()['elastic'][1]
    for h, w in XR.SIZES:
        u0, u1 = XR.displacement(int(big[1]), h, w)
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        xs, ys = x + big[0] * u0, y + big[0] * u1
        assert xs.min() < 0 and xs.max() > w - 1 and ys.min() < 0 and ys.max() > h - 1, (h, w)


# ---- bit-exact properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', XR.SIZES)
def test_neutral_row_repeat_runs_and_independence_of_the_other_rows(h, w):
    from latent_pose_reenactment_amd import hipops as ops
    x = torch.rand(3, 2, 3, h, w, generator=torch.Generator().manual_seed(h * w)).cuda()
    pose = x[:, 0]
    neutral = torch.zeros(3, 16).cuda()
    for inp in (pose, pose.contiguous()):
        out = ops.augment_extra(inp, neutral)
        assert torch.equal(out, pose) and out.is_contiguous() and out.data_ptr() != inp.data_ptr()
    out5 = ops.augment_extra(x[:, :1], neutral)
    assert tuple(out5.shape) == (3, 1, 3, h, w) and torch.equal(out5[:, 0], pose)
    assert torch.equal(ops.augment_extra(pose * 3 - 1, neutral), (pose * 3 - 1).clamp(0, 1))          # the clamp always runs
    rows = [XR.row(alpha=3.5, seed=99, median=1, d=-0.07, quality=75), XR.row(alpha=1.0, seed=5, quality=90), XR.row(median=1, d=0.05)]
    par = torch.tensor(np.stack(rows), dtype=torch.float32).cuda()
    first, second = ops.augment_extra(pose, par), ops.augment_extra(pose, par)
    assert torch.equal(first, second) and not torch.equal(first, pose)
    for i in range(3):
        alone = ops.augment_extra(pose[i:i + 1], par[i:i + 1])
        assert torch.equal(alone[0], first[i]), i
    other = ops.augment_extra(pose, torch.stack([par[0], torch.zeros(16).cuda(), par[1]]))
    assert torch.equal(other[0], first[0]) and torch.equal(other[1], pose[1])
    # rows far outside the loader's ranges (a displacement of many reflection periods, quality 1 and 100): the result stays in [0, 1] and the
    # other samples are untouched
    far = torch.tensor([[1.0e6, 5.0, 1.0, 0.5, 100.0] + [0.0] * 11, [-300.0, 16777215.0, 0.0, -1.0, 1.0] + [0.0] * 11, [0.0] * 16]).cuda()
    out = ops.augment_extra(pose, far)
    assert torch.equal(out[2], pose[2]) and bool(((out >= 0) & (out <= 1)).all())


def test_wrapper_refuses_malformed_inputs():
    from latent_pose_reenactment_amd import hipops as ops
    x, p = torch.zeros(2, 3, 8, 8).cuda(), torch.zeros(2, 16).cuda()
    assert tuple(ops.augment_extra(x, p).shape) == (2, 3, 8, 8)
    with pytest.raises(ValueError, match='pose must be fp32'):
        ops.augment_extra(x.half(), p)
    with pytest.raises(ValueError, match='params_extra is on cpu'):
        ops.augment_extra(x, p.cpu())
    with pytest.raises(ValueError, match='pose is on cpu'):
        ops.augment_extra(x.cpu(), p)
    with pytest.raises(ValueError, match='out is on cpu'):
        ops.augment_extra(x, p, out=torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match='shares its storage'):
        ops.augment_extra(x, p, out=x)
    with pytest.raises(ValueError, match='3 channels'):
        ops.augment_extra(torch.zeros(2, 4, 8, 8).cuda(), p)
    with pytest.raises(ValueError, match=r'params_extra must be \[B, 16\]'):
        ops.augment_extra(x, torch.zeros(2, 32).cuda())


# ---- capture ------------------------------------------------------------------------------------------------------------------------------------------
def batch_rows(b, seed):
    aug = AUG.ParametricAugmenter(XC.aug_args(image_size=32, use_pixelwise_augs=True, use_affine_scale=True, use_affine_shift=True,
                                              use_extra_pixelwise_augs=True))
    g = torch.Generator().manual_seed(seed)
    first = torch.stack([aug.sample(g) for _ in range(b)])
    extra = [r for r in (aug.sample_extra(g) for _ in range(40)) if (r != 0).any()][:b]
    return first.cuda(), torch.stack(extra).cuda()


def test_apply_with_both_keys_is_capturable_and_replays_with_new_rows():
    b, s = 3, 32
    g = torch.Generator().manual_seed(2)
    data = {'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g).cuda(), 'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g).cuda()}
    target = {'real_segm': torch.rand(b, 1, 1, s, s, generator=g).cuda().expand(b, 1, 3, s, s)}
    par1, extra1 = batch_rows(b, 1)
    par2, extra2 = batch_rows(b, 2)
    assert not torch.equal(par1, par2) and not torch.equal(extra1, extra2)
    static = dict(data, aug_params=par1.clone(), aug_params_extra=extra1.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        AUG.apply(static, target)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        d, t = AUG.apply(static, target)
    keys = (('pose_input_rgbs', d), ('target_rgbs', d), ('real_segm', t))
    for par, extra in ((par1, extra1), (par2, extra2)):
        static['aug_params'].copy_(par)
        static['aug_params_extra'].copy_(extra)
        graph.replay()
        torch.cuda.synchronize()
        de, te = AUG.apply(dict(data, aug_params=par, aug_params_extra=extra), target)
        for key, where in keys:
            assert torch.equal(where[key], (de if where is d else te)[key]), key
    assert 'aug_params' not in d and 'aug_params_extra' not in d


def test_graph_replay_augments_with_the_new_rows_of_both_stages(monkeypatch):
    """both parameter tables are tensors of the batch: ``load_batch`` copies them into the captured step's static inputs and the replay augments the
    NEW batch with the NEW rows, first stage then second"""
    from latent_pose_reenactment_amd import hipops as ops
    import test_train_step as TS
    z = TS.load()
    tm, opt_G, opt_D, a, data, target, holycow = TS.build(z, 'RAdam', monkeypatch)
    b, s = data['pose_input_rgbs'].shape[0], data['pose_input_rgbs'].shape[-1]
    (par1, extra1), (par2, extra2) = batch_rows(b, 11), batch_rows(b, 12)

    def want(dd, tt, par, extra):
        first = ops.augment_triplet(dd['pose_input_rgbs'], par, dd['target_rgbs'], tt['real_segm'])
        return ops.augment_extra(first[0], extra), first[1], first[2]
    keys = ('pose_input_rgbs', 'target_rgbs', 'real_segm')
    step = holycow.GraphedTrainStep(tm, opt_G, opt_D, a, dict(data, aug_params=par1, aug_params_extra=extra1), target, warmup_steps=3)
    step()
    torch.cuda.synchronize()
    assert 'aug_params' not in step.all_data and 'aug_params_extra' not in step.all_data
    first = {k: step.all_data[k].clone() for k in keys}
    assert all(torch.equal(first[k], w_) for k, w_ in zip(keys, want(data, target, par1, extra1)))
    g = torch.Generator().manual_seed(1)
    data2 = {k: (torch.rand(v.shape, generator=g).cuda() if v.is_floating_point() else v) for k, v in data.items()}
    data2.update(aug_params=par2, aug_params_extra=extra2)
    target2 = dict(target, real_segm=torch.rand(b, 1, 1, s, s, generator=g).cuda().expand(b, 1, 3, s, s))
    step.load_batch(data2, target2)
    step()
    torch.cuda.synchronize()
    for k, w_ in zip(keys, want(data2, target2, par2, extra2)):
        assert torch.equal(step.all_data[k], w_), k
        assert not torch.equal(step.all_data[k], first[k]), k
    # the second stage did something: the pose image is not the first stage's output
    assert not torch.equal(step.all_data['pose_input_rgbs'], ops.augment_triplet(data2['pose_input_rgbs'], par2)[0])
    assert all(torch.isfinite(v).all() for v in list(step.losses_G.values()) + list(step.losses_D.values()))


# ---- train.py -----------------------------------------------------------------------------------------------------------------------------------------
# train.py with (check) the pose image every module saw compared with apply's output and with the two launches done by hand, and / or (parent) the
# PARENT commit's code path put back: its ``apply`` (one key, one launch) and its ``is_empty``, written out from that commit
DRIVER = '''
import sys
sys.path.insert(0, {pkg!r})
import torch
import train
import runners.holycow as H
from latent_pose_reenactment_amd import augmentation as A, hipops
inner = H.train_step
def train_step(*args, **kw):
    out = inner(*args, **kw)
    print('ITERATION_LOSSES', {{k: float(v) for k, v in {{**out[1], **out[2]}}.items()}}, flush=True)
    return out
H.train_step = train_step
if {check}:
    applied = []
    inner_apply = A.apply
    def apply(d, t):
        out = inner_apply(d, t)
        applied.append(out[0]['pose_input_rgbs'])
        return out
    A.apply = apply
    inner_forward = H.TrainingModule.forward
    def forward(self, d, t):
        out = inner_forward(self, d, t)
        if 'aug_params_extra' in d:
            first = hipops.augment_triplet(d['pose_input_rgbs'], d['aug_params'], d['target_rgbs'], t['real_segm'])
            want = hipops.augment_extra(first[0], d['aug_params_extra'])
            seen = out[0]['pose_input_rgbs']
            print('POSE_SEEN', seen is applied[-1], bool(torch.equal(seen, want)), bool(torch.equal(seen, first[0])),
                  bool(torch.equal(out[0]['target_rgbs'], first[1])), flush=True)
        return out
    H.TrainingModule.forward = forward
if {parent}:
    def parent_apply(data_dict, target_dict):
        data_dict = dict(data_dict)
        target_dict = dict(target_dict) if isinstance(target_dict, dict) else target_dict
        params = data_dict.pop('aug_params')
        dicts = [data_dict] + ([target_dict] if isinstance(target_dict, dict) else [])
        def find(key):
            for d in dicts:
                if torch.is_tensor(d.get(key)):
                    return d
            return None
        where = {{key: find(key) for key in ('pose_input_rgbs', 'target_rgbs', 'real_segm')}}
        pose = where['pose_input_rgbs']['pose_input_rgbs']
        target = None if where['target_rgbs'] is None else where['target_rgbs']['target_rgbs']
        segm = None if where['real_segm'] is None else where['real_segm']['real_segm']
        outs = hipops.augment_triplet(pose, params, target, segm)
        for key, out in zip(('pose_input_rgbs', 'target_rgbs', 'real_segm'), outs):
            if out is not None:
                where[key][key] = out
        return data_dict, target_dict
    A.apply = parent_apply
    A.ParametricAugmenter.is_empty = lambda self: not (self.pixelwise or self.scale or self.shift)
    A.ParametricAugmenter.has_first_stage = lambda self: not self.is_empty()
    A.ParametricAugmenter.has_extra_stage = lambda self: False
train.main()
'''

RUNS = {}
FIRST = ['--use_pixelwise_augs']
BOTH = FIRST + ['--use_extra_pixelwise_augs']


def run_train(tmp, name, iterations, extra, check=False, parent=False):
    """one train.py process per name -> (checkpoint, per-iteration losses, POSE_SEEN lines)"""
    if name in RUNS:
        return RUNS[name]
    from test_train_entry_gpu import COMMON
    args = list(COMMON)
    args[args.index('--dataloader') + 1] = 'synthetic_voxceleb2_augmented'
    args[args.index('--synthetic_dataset_len') + 1] = str(4 * iterations)          # batch 4
    driver = tmp / f'{name}_driver.py'
    driver.write_text(DRIVER.format(pkg=PKG, check=check, parent=parent))
    cmd = [sys.executable, str(driver)] + args + ['--experiments_dir', str(tmp), '--experiment_name', name, '--log_frequency_loss', '1'] + extra
    r = subprocess.run(cmd, cwd=PKG, env=dict(os.environ, LP_PREC='bf16x3'), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = [eval(l.split('ITERATION_LOSSES', 1)[1]) for l in r.stdout.splitlines() if l.startswith('ITERATION_LOSSES')]
    seen = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith('POSE_SEEN')]
    ckpt_dir = os.path.join(str(tmp), name, 'checkpoints')
    ckpt = torch.load(os.path.join(ckpt_dir, sorted(os.listdir(ckpt_dir))[-1]), map_location='cpu', weights_only=False)
    RUNS[name] = (ckpt, losses, seen)
    return RUNS[name]


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp('augment_extra_train')


def test_train_entry_with_both_stages_eager_and_graphed(tmp):
    import math
    ckpt, losses, seen = run_train(tmp, 'both_eager', 2, BOTH, check=True)
    assert ckpt['args'].use_extra_pixelwise_augs is True and ckpt['args'].iteration == 2
    assert len(losses) == 2 and len(losses[0]) >= 4 and all(math.isfinite(v) for it in losses for v in it.values()), losses
    # the pose image the encoder saw IS apply's output, equals the two launches done by hand, and (in at least one iteration) is not the first
    # stage's output; the target is the first stage's
    assert len(seen) >= 2 and all(s[0] == 'True' and s[1] == 'True' and s[3] == 'True' for s in seen), seen
    assert any(s[2] == 'False' for s in seen), seen
    gckpt, glosses, _ = run_train(tmp, 'both_graph', 5, BOTH + ['--hip_graph'])
    assert gckpt['args'].iteration == 5 and len(glosses) == 3          # three eager iterations, then the capture and a replay
    assert all(math.isfinite(v) for it in glosses for v in it.values()), glosses
    import test_visuals_train_gpu as VT
    assert all(bool(torch.isfinite(v).all()) for v in VT.states(gckpt).values() if v.is_floating_point())
    print(f'[augment_extra] train.py with both stages: eager losses {losses[-1]}; --hip_graph last eager losses {glosses[-1]}')


def test_train_entry_without_the_flag_is_the_parent_code_path(tmp):
    """without --use_extra_pixelwise_augs the run ends in the ``state_dict``s of a run in which the parent commit's ``apply`` and ``is_empty`` are put
    back; two plain runs are themselves bit-identical (as established for the visuals), and the pair is held to what they show"""
    import test_visuals_train_gpu as VT
    plain = VT.states(run_train(tmp, 'plain', 2, FIRST)[0])
    plain2 = VT.states(run_train(tmp, 'plain2', 2, FIRST)[0])
    parent = VT.states(run_train(tmp, 'parent', 2, FIRST, parent=True)[0])
    assert len(plain) > 100
    noise, noisy = VT.largest_relative_difference(plain, plain2)
    got, where = VT.largest_relative_difference(plain, parent)
    print(f'[augment_extra] 2 iterations, --use_pixelwise_augs: plain vs plain {noise:.3e} ({noisy}); plain vs the parent code path {got:.3e} ({where})')
    assert got <= noise, (got, where, noise, noisy)
    both = VT.states(run_train(tmp, 'both_eager', 2, BOTH, check=True)[0])
    assert VT.largest_relative_difference(plain, both)[0] > 0          # and with the flag the step sees other pixels
