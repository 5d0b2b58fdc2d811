"""Host-side checks of the training visuals (csrc/visual_sheet.hip -> hipops.visual_sheet -> utils/visualize.py -> run_epoch --visuals, drive.py
--format png); no GPU:
  * the value rule: the closed forms, and for every k in 0 .. 255 the fp32 value nearest k / 255 with its two neighbours -- ``hipops.visual_sheet_host``
    against the numpy restatement (tests/visual_sheet_restatement.py), and drive_frames' torch chain against it on NaN-free input;
  * the layout: sample and panel order, the strip on top, a one-channel panel in all three channels, views read in place;
  * ``make_visual``: the reference's order and captions on batches with and without the optional keys, and no copies;
  * ``caption_strip``: a glyph pixel for pixel, a caption cut at its panel, a box for a character the font lacks, the cache;
  * ``hipops.visual_sheet`` and lp_visual_sheet refuse each bad argument before any device call;
  * ``run_epoch``: without --visuals it never touches utils.visualize; with it (a toy module on the CPU) it writes the sheets and leaves the weights
    exactly what they are without it;
  * drive.py's PNG writer gives files that decode to the frames."""
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

import visual_sheet_restatement as VR          # noqa: E402
from latent_pose_reenactment_amd import hipops as ops          # noqa: E402
from latent_pose_reenactment_amd.utils import visualize as V          # noqa: E402


def torch_chain(panels):
    """drive_frames' quantisation (drive.py: ``img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()``) laid out as a sheet"""
    cols = []
    for t in panels:
        n, c, h, w = t.shape
        cols.append(t.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte().expand(n, h, w, 3).reshape(n * h, w, 3))
    return torch.cat(cols, dim=1)


# ---- value rule -------------------------------------------------------------------------------------------------------------------------------------------
def test_closed_forms():
    assert np.array_equal(VR.quantise(VR.SPECIALS), VR.SPECIALS_Q)
    assert 0 < float(VR.DENORMAL) < np.finfo(np.float32).tiny
    x = torch.from_numpy(VR.SPECIALS.copy()).reshape(1, 1, 1, -1)
    got = ops.visual_sheet_host([x])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 8, 3)
    assert np.array_equal(got[0, :, 0].numpy(), VR.SPECIALS_Q) and torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])


def test_every_boundary_value_and_its_neighbours():
    b = VR.boundary_values()
    assert b.shape == (256, 3) and b.dtype == np.float32
    assert np.all(b[:, 0] < b[:, 1]) and np.all(b[:, 1] < b[:, 2]) and b[255, 1] == 1.0 and b[0, 1] == 0.0
    want = VR.quantise(b)
    # what the definition says about them without evaluating it: the value below k / 255 is in bin k - 1 (bin 0 for k = 0: it is negative), the value
    # above in bin k (k = 255: clamped), and the nearest fp32 value itself in one of the two
    ks = np.arange(256)
    assert np.array_equal(want[:, 0], np.maximum(ks - 1, 0)) and np.array_equal(want[:, 2], ks)
    assert np.all((want[:, 1] == ks) | (want[:, 1] == ks - 1)) and want[0, 1] == 0 and want[255, 1] == 255
    x = torch.from_numpy(b.copy()).reshape(1, 1, 256, 3)
    got = ops.visual_sheet_host([x])
    assert np.array_equal(got[..., 0].numpy(), want)
    assert np.array_equal(torch_chain([x])[..., 0].numpy(), want)


def test_host_version_and_torch_chain_equal_the_restatement():
    panels = [VR.salted_uniform((2, 3, 5, 7), 1), VR.salted_uniform((2, 1, 5, 7), 2), VR.salted_uniform((2, 3, 5, 7), 3)]
    strip = np.random.RandomState(4).randint(0, 256, size=(4, 21)).astype(np.uint8)
    want = VR.sheet(panels, strip)
    got = ops.visual_sheet([torch.from_numpy(p) for p in panels], caption=torch.from_numpy(strip))          # (CPU panels: the host version)
    assert got.is_contiguous() and np.array_equal(got.numpy(), want)
    clean = [np.where(np.isnan(p), np.float32(0.25), p) for p in panels]
    assert np.array_equal(torch_chain([torch.from_numpy(p) for p in clean]).numpy(), VR.sheet(clean))
    assert np.array_equal(ops.visual_sheet_host([torch.from_numpy(p) for p in clean]).numpy(), VR.sheet(clean))


# ---- layout -----------------------------------------------------------------------------------------------------------------------------------------------
def test_layout_sample_and_panel_order_strip_on_top_one_channel_replicated():
    n, h, w = 3, 2, 4
    # panel p, sample s, channel c -> the constant (40 p + 10 s + c) / 255 (+ half a step): every block of the sheet names where it came from
    def const(p, c_count):
        t = torch.zeros(n, c_count, h, w)
        for s in range(n):
            for c in range(c_count):
                t[s, c] = (40 * p + 10 * s + c + 0.5) / 255
        return t
    panels = [const(0, 3), const(1, 1), const(2, 3)]
    strip = torch.arange(5 * 3 * w, dtype=torch.uint8).reshape(5, 3 * w)
    for sheet in (ops.visual_sheet_host(panels, strip).numpy(), VR.sheet([p.numpy() for p in panels], strip.numpy())):
        assert sheet.shape == (5 + n * h, 3 * w, 3)
        assert all(np.array_equal(sheet[:5, :, c], strip.numpy()) for c in range(3))
        for p in range(3):
            for s in range(n):
                block = sheet[5 + s * h:5 + (s + 1) * h, p * w:(p + 1) * w]
                for c in range(3):
                    assert np.all(block[..., c] == 40 * p + 10 * s + (c if p != 1 else 0)), (p, s, c)
    assert ops.visual_sheet_host(panels).shape == (n * h, 3 * w, 3)
    out = torch.full((5 + n * h, 3 * w, 3), 7, dtype=torch.uint8)
    assert ops.visual_sheet(panels, strip, out=out) is out and torch.equal(out, ops.visual_sheet_host(panels, strip))


def test_views_are_read_in_place():
    g = torch.Generator().manual_seed(5)
    five = torch.rand(4, 2, 3, 6, 8, generator=g)
    mask = torch.rand(4, 1, 1, 6, 8, generator=g).expand(4, 1, 3, 6, 8)
    last = torch.rand(2, 6, 8, 3, generator=g).permute(0, 3, 1, 2)
    views = [five[:2, 0], mask[:2, 0], last, five[:2, 1, :, :, :][..., ::1]]
    want = VR.sheet([v.contiguous().numpy() for v in views])
    assert np.array_equal(ops.visual_sheet_host(views).numpy(), want)


# ---- make_visual ------------------------------------------------------------------------------------------------------------------------------------------
def batch(b=3, s=8, **extra):
    g = torch.Generator().manual_seed(6)
    d = {'enc_rgbs': torch.rand(b, 2, 3, s, s, generator=g), 'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g),
         'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g), 'fake_rgbs': torch.rand(b, 3, s, s, generator=g), 'label': torch.arange(b)}
    d.update(extra)
    return d, g


def same_view(view, base):
    return view.data_ptr() == base.data_ptr() and view.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()


def test_make_visual_order_captions_and_no_copies():
    d, g = batch()
    items = V.make_visual(d, 2)
    assert [c for c, _ in items] == ['Identity src', 'Pose target (same video)', 'Pose input (same video)', 'Generator output']
    for (_, view), key in zip(items, ('enc_rgbs', 'target_rgbs', 'pose_input_rgbs', 'fake_rgbs')):
        assert tuple(view.shape) == (2, 3, 8, 8) and same_view(view, d[key]), key
    assert torch.equal(items[0][1], d['enc_rgbs'][:2, 0]) and torch.equal(items[2][1], d['pose_input_rgbs'][:2, 0])
    # everything the reference shows
    d['real_segm'] = torch.rand(3, 1, 1, 8, 8, generator=g).expand(3, 1, 3, 8, 8)
    d['fake_segm'] = torch.rand(3, 1, 8, 8, generator=g)
    d['pose_input_rgbs_other_person'] = torch.rand(3, 1, 3, 8, 8, generator=g)
    d['fake_rgbs_other_person'] = torch.rand(3, 3, 8, 8, generator=g)
    items = V.make_visual(d, 2)
    assert [c for c, _ in items] == ['Identity src', 'Pose target (same video)', 'Pose input (same video)', 'Generator output', 'True segmentation',
                                     'Predicted segmentation', 'Pose input (other person)', 'Generator output']
    views = dict(zip(('enc', 'target', 'pose', 'fake', 'real_segm', 'fake_segm', 'pose_o', 'fake_o'), (v for _, v in items)))
    assert tuple(views['fake_segm'].shape) == (2, 1, 8, 8) and same_view(views['fake_segm'], d['fake_segm'])          # one channel, no cat
    assert tuple(views['real_segm'].shape) == (2, 3, 8, 8) and views['real_segm'].stride(1) == 0 and same_view(views['real_segm'], d['real_segm'])
    assert same_view(views['pose_o'], d['pose_input_rgbs_other_person']) and same_view(views['fake_o'], d['fake_rgbs_other_person'])
    # the other-video group sits between the segmentations and the other-person group; stickmen replace the pose target
    d['fake_rgbs_other_video'] = torch.rand(3, 3, 8, 8, generator=g)
    d['dec_stickmen'] = torch.rand(3, 1, 3, 8, 8, generator=g)
    d['dec_stickmen_other_person'] = torch.rand(3, 1, 3, 8, 8, generator=g)
    caps = [c for c, _ in V.make_visual(d, 5)]
    assert caps == ['Identity src', 'Pose src (same video)', 'Pose input (same video)', 'Generator output', 'True segmentation',
                    'Predicted segmentation', 'Generator output', 'Pose src (other person)', 'Pose input (other person)', 'Generator output']
    assert all(v.shape[0] == 3 for _, v in V.make_visual(d, 5))          # [:n_samples] of three samples
    assert V.make_visual({'label': d['label']}, 2) == []
    # the sheet of such a batch: the panels in that order
    del d['fake_rgbs_other_video'], d['dec_stickmen'], d['dec_stickmen_other_person']
    sheet = V.sheet(d, 2)
    items = V.make_visual(d, 2)
    hc = V.caption_height(8)
    assert tuple(sheet.shape) == (hc + 2 * 8, 8 * 8, 3)
    assert np.array_equal(sheet[hc:].numpy(), VR.sheet([v.contiguous().numpy() for _, v in items]))
    assert torch.equal(sheet[:hc, :, 1], V.caption_strip([c for c, _ in items], 8, hc))
    assert tuple(V.sheet(d, 2, captions=False).shape) == (2 * 8, 8 * 8, 3)


# ---- captions ---------------------------------------------------------------------------------------------------------------------------------------------
def ink(strip):
    return [''.join('#' if v == 0 else '.' for v in row.tolist()) for row in strip]


def test_caption_strip_glyphs_cut_and_box():
    assert set(''.join(c for c, _ in V.make_visual(batch()[0], 1)) + 'Pose src (other video) True Predicted segmentation person') <= set(V.FONT)
    assert all(len(rows.split()) == V.GLYPH_H and all(len(r) == V.GLYPH_W and set(r) <= {'#', '.'} for r in rows.split())
               for rows in list(V.FONT.values()) + [V.BOX])
    s = V.caption_strip(['P'], 10)
    assert s.dtype == torch.uint8 and tuple(s.shape) == (V.CAPTION_HEIGHT, 10) and set(s.unique().tolist()) == {0, 255}
    assert ink(s) == ['..........', '..........',
                      '.####.....', '.#...#....', '.#...#....', '.####.....', '.#........', '.#........', '.#........',
                      '..........', '..........']
    # a character the font lacks: the box; the second panel starts at its own column 0
    s = V.caption_strip(['', 'é'], 8)
    assert tuple(s.shape) == (V.CAPTION_HEIGHT, 16) and bool((s[:, :8] == 255).all())
    assert ink(s[2:9, 8:]) == ['.#####..', '.#...#..', '.#...#..', '.#...#..', '.#...#..', '.#...#..', '.#####..']
    # a caption wider than its panel is cut at the panel: nothing reaches the neighbour
    long, short = V.caption_strip(['Generator output', 'I'], 20), V.caption_strip(['Gen', 'I'], 20)
    assert torch.equal(long[:, 20:], short[:, 20:]) and torch.equal(long[:, :19], V.caption_strip(['Generator output'], 40)[:, :19])
    # characters start at columns 1, 7, 13, 19: the third is whole, of the fourth ('e') only the first column fits
    assert torch.equal(long[2:9, 13:18], 255 - 255 * V.glyph('n')) and torch.equal(long[2:9, 19], 255 - 255 * V.glyph('e')[:, 0])
    assert bool((long[2:9, 18] == 255).all())
    # twice the height budget: glyphs twice the size
    big = V.caption_strip(['P'], 16, 18)
    assert torch.equal(big[2:16, 1:11], V.caption_strip(['P'], 10)[2:9, 1:6].repeat_interleave(2, 0).repeat_interleave(2, 1))
    # a strip too low for the glyphs keeps what fits
    assert tuple(V.caption_strip(['P'], 10, 5).shape) == (5, 10) and ink(V.caption_strip(['P'], 10, 5))[2:] == ['.####.....', '.#...#....', '.#...#....']
    with pytest.raises(ValueError):
        V.caption_strip(['a'], 0)


def test_caption_strip_is_rasterised_once_per_caption_tuple(monkeypatch):
    calls = []
    inner = V.caption_strip
    monkeypatch.setattr(V, 'caption_strip', lambda *a, **k: calls.append(a) or inner(*a, **k))
    monkeypatch.setattr(V, '_STRIPS', {})
    d, _ = batch()
    a, b = V.sheet(d, 2), V.sheet(d, 1)
    assert len(calls) == 1 and torch.equal(a[:V.caption_height(8)], b[:V.caption_height(8)])
    d['fake_segm'] = torch.rand(3, 1, 8, 8)
    V.sheet(d, 2)
    assert len(calls) == 2


# ---- arguments --------------------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_bad_arguments_before_any_device_call(monkeypatch):
    from latent_pose_reenactment_amd import _lib
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was reached'))
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError, match='panel 1 must be fp32'):
        ops.visual_sheet([x, x.double()])
    with pytest.raises(ValueError, match='panel 0 must be 4-D'):
        ops.visual_sheet([x[0]])
    with pytest.raises(ValueError, match='panel 1 must have 1 or 3 channels'):
        ops.visual_sheet([x, torch.zeros(2, 2, 4, 4)])
    with pytest.raises(ValueError, match='shape mismatch between panel 0 .* and panel 2'):
        ops.visual_sheet([x, x, torch.zeros(2, 3, 4, 5)])
    with pytest.raises(ValueError, match='shape mismatch'):
        ops.visual_sheet([x, torch.zeros(3, 3, 4, 4)])
    with pytest.raises(ValueError, match='got 13 .*more than 12 panels'):
        ops.visual_sheet([x] * 13)
    with pytest.raises(ValueError, match='got 0'):
        ops.visual_sheet([])
    with pytest.raises(ValueError, match='sequence'):
        ops.visual_sheet(x)
    with pytest.raises(ValueError, match='panel 1 must be a tensor'):
        ops.visual_sheet([x, None])
    with pytest.raises(ValueError, match='not on the GPU|one device'):
        ops.visual_sheet([x.to('meta'), x])
    with pytest.raises(ValueError, match=r'caption strip must be uint8 \[Hc, P \* W\]'):
        ops.visual_sheet([x], caption=torch.zeros(3, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match='caption strip must be uint8'):
        ops.visual_sheet([x], caption=torch.zeros(3, 4))
    with pytest.raises(ValueError, match='out must be a contiguous uint8 tensor'):
        ops.visual_sheet([x], out=torch.zeros(8, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='empty'):
        ops.visual_sheet([torch.zeros(0, 3, 4, 4)])
    assert tuple(ops.visual_sheet([x] * 12).shape) == (8, 48, 3)          # twelve CPU panels: the host version, no library


def test_c_entry_point_validates_before_device_work():
    from latent_pose_reenactment_amd import _lib
    l = _lib.lib()
    assert l.lp_abi_version() == 12
    fake = 4096          # (never dereferenced: every call below is refused first)
    ptrs, st, ch = (ctypes.c_void_p * 13)(*[fake] * 13), (ctypes.c_longlong * 52)(*[48, 16, 4, 1] * 13), (ctypes.c_int * 13)(*[3] * 13)
    pp, sp, cp = ctypes.addressof(ptrs), ctypes.addressof(st), ctypes.addressof(ch)
    f = l.lp_visual_sheet
    assert f(None, sp, cp, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(pp, None, cp, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(pp, sp, None, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'null' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 1, 4, 4, None, 0, None, None) == -1 and b'null' in l.lp_last_error()
    assert f(pp, sp, cp, 0, 1, 4, 4, None, 0, fake, None) == -1 and b'1 .. 12' in l.lp_last_error()
    assert f(pp, sp, cp, 13, 1, 4, 4, None, 0, fake, None) == -1 and b'1 .. 12' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 0, 4, 4, None, 0, fake, None) == -1 and b'N >= 1' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 1, 0, 4, None, 0, fake, None) == -1 and b'H >= 1' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 1, 4, 0, None, 0, fake, None) == -1 and b'W >= 1' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 1, 4, 4, None, 5, fake, None) == -1 and b'caption' in l.lp_last_error()
    assert f(pp, sp, cp, 2, 1, 4, 4, fake, -1, fake, None) == -1 and b'Hc' in l.lp_last_error()
    for bad in (0, 2, 4):
        ch[1] = bad
        assert f(pp, sp, cp, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'C must be 1 or 3' in l.lp_last_error()
    ch[1] = 1
    ptrs[1] = None
    assert f(pp, sp, cp, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'null' in l.lp_last_error()
    ptrs[1] = fake
    st[6] = -4
    assert f(pp, sp, cp, 2, 1, 4, 4, None, 0, fake, None) == -1 and b'negative stride' in l.lp_last_error()
    st[6] = 4
    assert f(pp, sp, cp, 2, 1 << 30, 1 << 30, 4, None, 0, fake, None) == -2 and b'grid' in l.lp_last_error()


def test_abi_tests_hold_with_the_new_symbol():
    import test_abi
    assert 'lp_visual_sheet' in test_abi.parse_header()
    test_abi.test_library_exports_every_declared_symbol()
    test_abi.test_ctypes_signatures_match_header()


# ---- runner -----------------------------------------------------------------------------------------------------------------------------------------------
class _Embedder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.7]))

    def get_pose_embedding(self, d):
        d['pose_embedding'] = d['pose_input_rgbs'].mean((1, 2, 3, 4)) * self.w

    def forward(self, d):
        d['embeds'] = d['enc_rgbs'].mean((1, 2, 3, 4))
        self.get_pose_embedding(d)


class _Generator(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([1.3]))

    def forward(self, d):
        d['fake_rgbs'] = d['pose_input_rgbs'][:, 0] * (self.w * (d['pose_embedding'] + d['embeds']))[:, None, None, None]
        d['fake_segm'] = d['fake_rgbs'][:, :1] * 0.5


class _Critic(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor([0.2]))

    def forward(self, d):
        d['fake_score_G'] = (d['fake_rgbs'] * self.w).mean()
        d['fake_score_D'] = (d['fake_rgbs'].detach() * self.w).mean()


class _Criterion(torch.nn.Module):
    def forward(self, d):
        return {'l1': (d['fake_rgbs'] - d['target_rgbs'][:, 0]).abs().mean() - d['fake_score_G']}, {'d': d['fake_score_D'] ** 2}


def toy_run(tmp, visuals, b=3, s=8, iterations=3, finetune=False, holycow=None):
    torch.manual_seed(0)
    E, G, D = _Embedder(), _Generator(), _Critic()
    tm = holycow.TrainingModule(E, G, D, [_Criterion()], [], running_averages={})
    args = argparse.Namespace(device='cpu', num_gpus=1, finetune=finetune, detailed_metrics=True, iteration=0, log_frequency_loss=1,
                              log_frequency_images=1, num_visuals_per_img=2, visuals=visuals, logging=True, rank=0, set_eval_mode_in_test=True,
                              set_eval_mode_in_train=False, experiment_dir=tmp, hip_graph=False)
    g = torch.Generator().manual_seed(1)
    loader = []
    for _ in range(iterations):
        loader.append(({'enc_rgbs': torch.rand(b, 2, 3, s, s, generator=g), 'pose_input_rgbs': torch.rand(b, 1, 3, s, s, generator=g),
                        'target_rgbs': torch.rand(b, 1, 3, s, s, generator=g)},
                       {'label': torch.arange(b), 'real_segm': torch.rand(b, 1, 1, s, s, generator=g).expand(b, 1, 3, s, s)}))
    opt_G = torch.optim.SGD(list(E.parameters()) + list(G.parameters()), lr=0.1)
    opt_D = torch.optim.SGD(D.parameters(), lr=0.1)
    tm.train()
    holycow.run_epoch(loader, tm, opt_G, opt_D, 0, args, 'train')
    state = {f'{name}.{k}': v.clone() for name, m in (('E', E), ('G', G), ('D', D), ('avgE', tm.running_averages['embedder']),
                                                       ('avgG', tm.running_averages['generator'])) for k, v in m.state_dict().items()}
    return tm, args, loader, state


class _Forbidden:
    def __getattr__(self, name):
        raise AssertionError(f'utils.visualize.{name} was touched without --visuals')


def test_run_epoch_without_the_flag_never_touches_visualize(tmp_path, monkeypatch):
    from runners import holycow
    import latent_pose_reenactment_amd.utils as U
    monkeypatch.setitem(sys.modules, 'latent_pose_reenactment_amd.utils.visualize', _Forbidden())
    monkeypatch.setattr(U, 'visualize', _Forbidden(), raising=False)
    monkeypatch.setattr(holycow, 'log_visuals', lambda *a, **k: pytest.fail('log_visuals was called without --visuals'))
    monkeypatch.setattr(holycow, 'visual_forward', lambda *a, **k: pytest.fail('visual_forward was called without --visuals'))
    tm, args, _, _ = toy_run(tmp_path, False, holycow=holycow)
    assert args.iteration == 3 and tm.training and not (tmp_path / 'visuals').exists()
    # ... and the flag is what the parser knows: default off
    from utils.argparse_utils import MyArgumentParser
    parser = holycow.get_args(MyArgumentParser(conflict_handler='resolve'))
    assert parser.parse_args([]).visuals is False and parser.parse_args(['--visuals']).visuals is True


def test_run_epoch_with_the_flag_writes_the_sheets_and_leaves_training_alone(tmp_path):
    from PIL import Image
    from runners import holycow
    _, _, _, plain = toy_run(tmp_path / 'plain', False, holycow=holycow)
    tm, args, loader, with_visuals = toy_run(tmp_path / 'vis', True, holycow=holycow)
    assert set(plain) == set(with_visuals) and all(torch.equal(plain[k], with_visuals[k]) for k in plain)          # bit for bit
    assert tm.training and tm.use_running_averages is False and tm.compute_losses is True
    files = sorted(os.listdir(tmp_path / 'vis' / 'visuals'))
    assert files == ['train_00000000.png', 'train_00000001.png', 'train_00000002.png']
    # the last sheet was made AFTER the last update: the running averages as they are now give it again
    data, target = loader[-1]
    again = holycow.visual_forward(tm, data, target, args)
    caps = [c for c, _ in V.make_visual(again, 2)]
    assert caps == ['Identity src', 'Pose target (same video)', 'Pose input (same video)', 'Generator output', 'Predicted segmentation',
                    'Pose input (other person)', 'Generator output']          # (the visual forward's only target is the label: no true segmentation)
    png = np.asarray(Image.open(tmp_path / 'vis' / 'visuals' / files[-1]))
    hc, s = V.caption_height(8), 8
    assert png.shape == (hc + 2 * s, 7 * s, 3) and png.dtype == np.uint8
    assert np.array_equal(png, V.sheet(again, 2).numpy())
    assert np.array_equal(png[hc:, 3 * s:4 * s], ops.visual_sheet_host([again['fake_rgbs'][:2]]).numpy())
    # cross-driving: sample i is driven by the pose input of sample i - 1
    avgE, avgG = tm.running_averages['embedder'], tm.running_averages['generator']
    with torch.no_grad():
        d = {'enc_rgbs': data['enc_rgbs'], 'pose_input_rgbs': data['pose_input_rgbs'][[2, 0, 1]]}
        avgE(d)
        avgG(d)
    assert torch.equal(again['pose_input_rgbs_other_person'], data['pose_input_rgbs'][[2, 0, 1]])
    assert torch.equal(again['fake_rgbs_other_person'], d['fake_rgbs']) and not torch.equal(d['fake_rgbs'], again['fake_rgbs'])
    assert np.array_equal(png[hc:, 6 * s:], ops.visual_sheet_host([d['fake_rgbs'][:2]]).numpy())
    # one sample, or fine-tuning: no other-person group
    tm1, args1, loader1, _ = toy_run(tmp_path / 'one', True, b=1, iterations=1, holycow=holycow)
    assert not any(k.endswith('_other_person') for k in holycow.visual_forward(tm1, *loader1[0], args1))
    assert np.asarray(Image.open(tmp_path / 'one' / 'visuals' / 'train_00000000.png')).shape == (hc + s, 5 * s, 3)
    tm2, args2, loader2, _ = toy_run(tmp_path / 'ft', True, iterations=1, finetune=True, holycow=holycow)
    assert not any(k.endswith('_other_person') for k in holycow.visual_forward(tm2, *loader2[0], args2))
    # every --log_frequency_images iterations, counted from args.iteration
    args.log_frequency_images, args.iteration, args.experiment_dir = 2, 3, tmp_path / 'every2'
    holycow.run_epoch(loader, tm, torch.optim.SGD(tm.generator.parameters(), lr=0.0), torch.optim.SGD(tm.discriminator.parameters(), lr=0.0), 0, args, 'train')
    assert sorted(os.listdir(tmp_path / 'every2' / 'visuals')) == ['train_00000004.png']


# ---- drive.py ---------------------------------------------------------------------------------------------------------------------------------------------
def test_drive_png_writer_round_trips(tmp_path):
    from PIL import Image
    import drive
    video = np.random.RandomState(7).randint(0, 256, size=(3, 6, 10, 3)).astype(np.uint8)
    paths = drive.write_png_frames(tmp_path / 'seq' / 'driver', video[:, :, ::-1][:, :, ::-1])
    assert [p.name for p in paths] == ['000000.png', '000001.png', '000002.png'] and all(p.parent == tmp_path / 'seq' / 'driver' for p in paths)
    for t, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), video[t])
    # the frames drive_frames would hand over: its quantisation of a float image, through the file and back
    img = torch.from_numpy(VR.salted_uniform((1, 3, 6, 5), 8)).nan_to_num(nan=0.5)
    frame = img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte().numpy()
    (path,) = drive.write_png_frames(tmp_path / 'one', frame)
    assert np.array_equal(np.asarray(Image.open(path)), VR.sheet([img.numpy()]))
