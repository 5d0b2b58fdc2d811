"""The blur and fade of padded bands (csrc/frames_pad.hip's header comment) without a GPU: ``frames.pad_host`` (fp32 torch ops) against the fp64
restatement (tests/frames_pad_restatement.py) on the case list that tests/test_frames_pad_gpu.py runs through the kernel, ``frames.pad_plan`` against a
plan written out by hand, ``prepare_host`` with the flag end to end, the refusals, and the flag-off path against bytes the parent commit produced.

The rule of comparison.  Both sides end in ``clamp(rint(y))``, so the uint8 values are compared for EXACT equality, except where the fp64 value y before
the rounding lies within tau of a half-integer; there the two may differ by 1.  tau = (2 k + 32) 2^-24 255, from the definition alone:
  - each pass of the blur is an fp32 dot product of k taps with weights that sum to 1 and values <= 255: its error is at most k 2^-24 255, so 2 k for
    the two passes (the vertical pass's inputs carry the horizontal pass's error once, weights summing to 1);
  - the remaining 32 units of 2^-24 255 cover the taps rounded to fp32 after normalising in fp64 (1 per pass, 2), the two fp32 divisions of the
    weights, each scaled by 3 in a = clip(3 m + 1) and once more through f (2 x 3 + 2 = 8, each acting on a difference of at most 255), the product
    and sum of 3 m + 1 (2), and the two blends of three roundings each on values of at most 255 (2 x 3 x 2 = 12 with the doubled range of a
    difference): 24, rounded up to the next power of two.
A case may have at most 2 % of its values flagged (the restatement alone decides which): the case list was chosen so, and tiny even-n cases with pads
of 2, a third of whose values are exact half-integers, are deliberately not in it.
The shares, from the restatement alone on these seeds: worst 1.948 % (150 / 200 / 10 / -60 as a mask), 1.110 % (100 / 127 / -9 / -20 mask),
0.854 % (40 / 64 / -10 / -12 mask); every image case under 0.17 %, most cases under 0.1 %.
Measured on the host (``pad_host``): no mismatch outside the flagged values in any case; of the flagged values at most 70 of a case differ, by 1;
``prepare_host`` with the flag end to end: worst error 0.21 of the bound."""
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import frames_restatement as FR          # noqa: E402
import frames_pad_restatement as FP      # noqa: E402

# view H x H, n, t, l
CASES = [(1, 7, -3, -3), (3, 1, -1, 0), (5, 9, -3, -1), (7, 11, -3, -3), (3, 13, -5, -5), (12, 17, 0, -3), (12, 17, -5, 0), (12, 17, 0, 0),
         (20, 25, -3, 2), (30, 40, -7, -3), (30, 41, -7, -3), (50, 49, -3, 4), (60, 63, -1, -1), (61, 64, -1, -1), (40, 64, -10, -12),
         (100, 127, -9, -20), (150, 200, -30, -10), (150, 200, 10, -60), (250, 320, -40, -35), (300, 320, -1, -1)]
KINDS = ('image', 'mask')
SIZE = 64                       # the table's output size: only its checks and the mode read it here
CAP = 0.02
PREFIX = 5                      # (a frame need not start at a multiple of anything)


class Case:
    """one H x H x 3 image (smooth plus noise) and one H x H mask (a soft-edged disc that crosses the view's top and left edges), packed"""

    def __init__(self, h, n, t, l):
        self.h, self.n, self.t, self.l = h, n, t, l
        rng = np.random.default_rng([h, n, t + 1000, l + 1000])
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(h, dtype=np.float64), indexing='ij')
        smooth = np.stack([128 + 70 * np.sin(yy / 6.0 + c) * np.cos(xx / 4.5 - c) + 25 * np.cos((yy + xx) / 11.0 + 2 * c) for c in range(3)], axis=-1)
        self.image = np.clip(np.rint(smooth + rng.integers(-12, 13, (h, h, 3))), 0, 255).astype(np.uint8)
        d = np.sqrt((yy - 0.48 * h) ** 2 + (xx - 0.46 * h) ** 2)
        self.mask = np.rint(255 * np.clip(0.52 * h - d + 0.5, 0.0, 1.0)).astype(np.uint8)
        self.buf = np.concatenate([np.zeros(PREFIX, dtype=np.uint8), self.image.reshape(-1), self.mask.reshape(-1)])

    def view(self, kind, base=0):
        h, box = self.h, [self.t, self.l, self.t + self.n, self.l + self.n]
        if kind == 'image':
            return [base + PREFIX, h, h, 3 * h, 3] + box + [FR.mode_for(self.n, SIZE)]
        return [base + PREFIX + 3 * h * h, h, h, h, 1] + box

    def row(self, kind, slot=0, base=0):
        return FR.row(image=self.view(kind, base), image_slot=slot) if kind == 'image' else FR.row(mask=self.view(kind, base), mask_slot=slot)


_CASES, _WANT = {}, {}


def case(spec):
    if spec not in _CASES:
        _CASES[spec] = Case(*spec)
    return _CASES[spec]


def restated(spec, kind):
    """(uint8 [n, n, C], fp64 before the rounding), computed once"""
    if (spec, kind) not in _WANT:
        c = case(spec)
        _WANT[spec, kind] = FP.pad_view(c.buf, *c.view(kind)[:5], c.t, c.l, c.n, kind == 'mask')
    return _WANT[spec, kind]


def compare(got, spec, kind):
    """the rule of the module docstring -> (flagged share, flagged values that differ)"""
    want, y = restated(spec, kind)
    n = spec[1]
    assert got.shape == want.shape and got.dtype == np.uint8, (got.shape, want.shape)
    flags = FP.flagged(y, n)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share, off = float(flags.mean()), int((diff[flags] != 0).sum())
    print(f'[frames_pad] {spec} {kind}: k {FP.taps(n)[0]}, flagged {100 * share:.3f} %, of which differ {off}; mismatches elsewhere {int((diff[~flags] != 0).sum())}')
    assert share <= CAP, f'{spec} {kind}: {share:.4f} of the values are flagged'
    assert not (diff[~flags] != 0).any(), f'{spec} {kind}: {int((diff[~flags] != 0).sum())} values differ away from a half-integer (worst {diff[~flags].max()})'
    assert diff.max() <= 1, f'{spec} {kind}: a flagged value differs by {diff.max()}'
    return share, off


def workspace_of(buffer, nbytes, n, chans):
    ws = (nbytes + FP.ALIGN - 1) // FP.ALIGN * FP.ALIGN
    return np.asarray(buffer[ws:ws + n * n * chans]).reshape(n, n, chans)


def extra_tolerance(row, flags, size):
    """what one flagged byte may add to an output of ``FR.prepare`` on the rewritten ``row``: a flagged workspace byte may differ by 1 of 255, the
    resampling is linear in its source with the weights of ``FR.axis_matrix`` and the cubic clamp does not widen a difference, so an output may move by
    (1 / 255) x the sum of |w_y| |w_x| over the flagged source pixels it reads -> (image [3, S, S] | None, mask [S, S] | None, product [3, S, S] | None);
    product: |i' m' - i m| <= |i' - i| m' + i |m' - m| <= e_i (1 + e_m) + e_m for values in [0, 1]"""
    out = []
    for base, chans, mode in ((FR.IMG_OFF, 3, row[FR.IMG_MODE]), (FR.MSK_OFF, 1, FR.LINEAR)):
        off, h = row[base], row[base + 1]
        if h == 0:
            out.append(None)
            continue
        n = row[base + 7] - row[base + 5]
        f = flags[off:off + n * n * chans].reshape(n, n, chans).astype(np.float64) if off + n * n * chans <= flags.size and row[base + 3] == n * chans else None
        if f is None or not f.any():
            out.append(np.zeros((chans, size, size)))
            continue
        m = np.abs(FR.axis_matrix(mode, n, size))
        out.append(np.stack([m @ f[:, :, c] @ m.T for c in range(chans)]) / 255.0)
    e_img, e_msk = out[0], None if out[1] is None else out[1][0]
    e_prod = None if e_img is None or e_msk is None else e_img * (1.0 + e_msk[None]) + e_msk[None]
    return e_img, e_msk, e_prod


# ---- 1. pad_host against the restatement ------------------------------------------------------------------------------------------------------------
def test_the_integer_k_is_cv2s_rounding_and_the_taps_sum_to_one():
    for n in range(1, 1025):
        k, g = FP.taps(n)
        assert k == (int(np.floor(0.096 * n + 1.5)) | 1) and k % 2 == 1 and abs(g.sum() - 1.0) < 1e-14 and len(g) == k      # (no ties: floor(x + .5) is cvRound)
    assert FP.taps(1024)[0] == 99 and FP.taps(1)[0] == 1
    assert sorted({FP.taps(c[1])[0] for c in CASES}) == [1, 3, 5, 7, 13, 21, 33]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('spec', CASES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_pad_host_against_the_restatement(spec, kind):
    from latent_pose_reenactment_amd import frames
    c = case(spec)
    buf, table = frames.pad_host(torch.from_numpy(c.buf), torch.tensor([c.row(kind)], dtype=torch.int64), SIZE)
    chans = 3 if kind == 'image' else 1
    assert torch.equal(buf[:c.buf.size], torch.from_numpy(c.buf))
    compare(workspace_of(buf.numpy(), c.buf.size, c.n, chans), spec, kind)
    base = FR.IMG_OFF if kind == 'image' else FR.MSK_OFF
    ws = (c.buf.size + 15) // 16 * 16
    assert table[0, base:base + 9].tolist() == [ws, c.n, c.n, c.n * chans, chans, 0, 0, c.n, c.n] and buf.numel() == ws + c.n * c.n * chans


# ---- 2. the plan ------------------------------------------------------------------------------------------------------------------------------------
def test_pad_plan_against_a_plan_written_by_hand():
    from latent_pose_reenactment_amd import frames
    # a 10 x 10 x 3 frame at 0 and a 10 x 10 mask at 300: 400 bytes
    nbytes, size = 400, 8
    img = lambda t, l, n: [0, 10, 10, 30, 3, t, l, t + n, l + n, frames.mode_for(n, size)]
    msk = lambda t, l, n: [300, 10, 10, 10, 1, t, l, t + n, l + n]
    rows = [frames.make_row(img(-2, 1, 9), None, image_slot=0),                      # out at the top: 9 x 9 x 3 = 243 bytes at 400
            frames.make_row(img(1, 2, 8), msk(1, 2, 8), 1, 0, 0),                    # inside: untouched
            frames.make_row(img(0, 0, 10), msk(3, 3, 9), 2, 1, 1),                   # only the mask leaves: 81 bytes at 656 (643 rounded up)
            frames.make_row(img(-1, -1, 13), msk(-1, -1, 13), 3, 2, 2)]              # both: 507 bytes at 752 (737 rounded up), 169 at 1264 (1259)
    for r in rows:
        r[22], r[23] = 77, -5                                                        # the reserved columns are not read and travel as they are
    table = torch.tensor(rows, dtype=torch.int64)
    table2, plan, weights, total = frames.pad_plan(table, nbytes, size)
    assert frames.PLAN_COLUMNS == ('row', 'view', 'off', 'h', 'w', 'row_stride', 'pixel_stride', 't', 'l', 'n', 'pad_t', 'pad_l', 'pad_b', 'pad_r', 'k', 'ws_off')
    assert plan.tolist() == [[0, 0, 0, 10, 10, 30, 3, -2, 1, 9, 2, 0, 0, 0, 3, 400],
                             [2, 1, 300, 10, 10, 10, 1, 3, 3, 9, 0, 0, 2, 2, 3, 656],
                             [3, 0, 0, 10, 10, 30, 3, -1, -1, 13, 1, 1, 2, 2, 3, 752],
                             [3, 1, 300, 10, 10, 10, 1, -1, -1, 13, 1, 1, 2, 2, 3, 1264]]
    assert total == 1264 + 169 and all(p[15] % 16 == 0 for p in plan.tolist())
    want = [list(r) for r in rows]
    want[0][0:9] = [400, 9, 9, 27, 3, 0, 0, 9, 9]
    want[2][10:19] = [656, 9, 9, 9, 1, 0, 0, 9, 9]
    want[3][0:9] = [752, 13, 13, 39, 3, 0, 0, 13, 13]
    want[3][10:19] = [1264, 13, 13, 13, 1, 0, 0, 13, 13]
    assert table2.tolist() == want and torch.equal(table, torch.tensor(rows, dtype=torch.int64))          # (modes, slots and row 1 as they were)
    assert weights.dtype == torch.float32 and tuple(weights.shape) == (4, 100) and not weights[:, 3:].any()
    g = FP.taps(9)[1]
    assert torch.equal(weights[0, :3], torch.from_numpy(g).to(torch.float32)) and weights[0, 0] == weights[0, 2]
    frames.check_plan(plan, weights, nbytes, total)


def test_a_table_inside_its_views_is_left_alone():
    from latent_pose_reenactment_amd import frames
    c = case((30, 40, -7, -3))
    rows = [FR.row(image=[PREFIX, 30, 30, 90, 3, 2, 3, 22, 23, FR.mode_for(20, 16)], mask=[PREFIX + 2700, 30, 30, 30, 1, 0, 0, 30, 30], image_slot=0,
                   mask_slot=0, product_slot=0)]
    table, buf = torch.tensor(rows, dtype=torch.int64), torch.from_numpy(c.buf)
    table2, plan, weights, total = frames.pad_plan(table, buf.numel(), 16)
    assert torch.equal(table2, table) and tuple(plan.shape) == (0, 16) and tuple(weights.shape) == (0, 100) and total == buf.numel()
    buf2, table3 = frames.pad_host(buf, table, 16)
    assert torch.equal(buf2, buf) and torch.equal(table3, table)
    for a, b in zip(frames.prepare_host(buf, table, 16, blur_padded_bands=True), frames.prepare_host(buf, table, 16)):
        assert torch.equal(a, b)


# ---- 3. prepare_host with the flag, end to end -------------------------------------------------------------------------------------------------------
def mixed_table(size, specs=((12, 17, 0, -3), (30, 41, -7, -3), (20, 25, -3, 2), (5, 9, -3, -1))):
    """-> (buf, rows): image + mask + product rows of several cases in one buffer, and one row inside its views"""
    chunks, rows, base = [], [], 0
    for s, spec in enumerate(specs):
        c = case(spec)
        image = c.view('image', base)
        image[9] = FR.mode_for(c.n, size)
        rows.append(FR.row(image, c.view('mask', base), s, s, s))
        chunks.append(c.buf)
        base += c.buf.size
    c = case(specs[1])
    inside = [PREFIX + len(chunks[0]), c.h, c.h, 3 * c.h, 3, 2, 3, 22, 23, FR.mode_for(20, size)]
    rows.append(FR.row(inside, image_slot=len(specs)))
    return np.concatenate(chunks), rows


@pytest.mark.parametrize('size', [8, 16, 48])
def test_prepare_host_with_the_flag_end_to_end(size):
    """restatement-pad followed by ``frames_restatement.prepare``, under ``frames_restatement.gate`` plus ``extra_tolerance`` for flagged source
    bytes only"""
    from latent_pose_reenactment_amd import frames
    buf, rows = mixed_table(size)
    got = frames.prepare_host(torch.from_numpy(buf), torch.tensor(rows, dtype=torch.int64), size, blur_padded_bands=True)
    buf2, rows2, flags = FP.pad(buf, rows)
    want = FR.prepare(buf2, rows2, size)
    plain = frames.prepare_host(torch.from_numpy(buf), torch.tensor(rows, dtype=torch.int64), size)
    assert torch.equal(got[0][len(rows) - 1], plain[0][len(rows) - 1])                  # the row inside its view: untouched
    assert not torch.equal(got[0][0], plain[0][0]) and not torch.equal(got[1][0], plain[1][0])
    worst = 0.0
    for r in rows2:
        n_img, n_msk = r[FR.IMG_B] - r[FR.IMG_T], r[FR.MSK_B] - r[FR.MSK_T]
        gates = (FR.gate(n_img, size, r[FR.IMG_MODE]), FR.gate(n_msk, size, FR.LINEAR) if r[FR.MSK_H] else None,
                 FR.product_gate(n_img, r[FR.IMG_MODE], n_msk, size) if r[FR.MSK_H] else None)
        extra = extra_tolerance(r, flags, size)
        for o, col in enumerate((FR.IMAGE_SLOT, FR.MASK_SLOT, FR.PRODUCT_SLOT)):
            if r[col] < 0:
                continue
            err = np.abs(got[o][r[col]].double().numpy() - want[o][r[col]])
            bound = gates[o] + (extra[o][None] if o == 1 else extra[o])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (r[col], o, float((err - bound).max()))
    print(f'[frames_pad] prepare_host with the flag, S {size}: worst error / bound {worst:.2f}')


# ---- 4. the refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_cause():
    from latent_pose_reenactment_amd import frames
    buf = torch.zeros(4 * 4 * 3 + 16, dtype=torch.uint8)
    big = torch.tensor([FR.row([0, 4, 4, 12, 3, -1, 0, 1024, 1025, FR.AREA], image_slot=0)], dtype=torch.int64)
    with pytest.raises(ValueError, match=r'row 0.*image crop of 1025 is above 1024'):
        frames.pad_plan(big, buf.numel(), 256)
    with pytest.raises(ValueError, match=r'row 0.*above 1024'):
        frames.prepare_host(buf, big, 256, blur_padded_bands=True)
    assert frames.prepare_host(buf, big, 256)[0].shape == (1, 3, 256, 256)               # without the flag the crop is within the scale limit
    ok = torch.tensor([FR.row([0, 4, 4, 12, 3, -1, 0, 1023, 1024, FR.AREA], image_slot=0)], dtype=torch.int64)
    assert frames.pad_plan(ok, buf.numel(), 256)[1][0, 14] == 99
    with pytest.raises(ValueError, match='uint8'):
        frames.pad_host(buf.float(), ok, 256)
    with pytest.raises(ValueError, match='not square'):                                 # the table's own rules come first
        frames.pad_plan(torch.tensor([FR.row([0, 4, 4, 12, 3, -1, 0, 5, 7, FR.CUBIC], image_slot=0)], dtype=torch.int64), buf.numel(), 256)

    c = case((12, 17, 0, -3))
    _, plan, weights, total = frames.pad_plan(torch.tensor([c.row('image')], dtype=torch.int64), c.buf.size, SIZE)
    nbytes = c.buf.size

    def broken(col, value):
        p = plan.clone()
        p[0, col] = value
        return p
    for col, value, what in ((11, 2, 'pads'), (14, 5, r'k 5 is not'), (15, plan[0, 15] + 8, 'aligned'), (15, 0, 'behind the head'),
                             (15, plan[0, 15] + 16, 'does not fit'), (2, nbytes, 'outside the packed head'), (1, 2, 'neither 0'), (9, 0, 'side 0'),
                             (9, 2000, 'above 1024')):
        with pytest.raises(ValueError, match=rf'plan 0 \(row 0\).*{what}'):
            frames.check_plan(broken(col, value), weights, nbytes, total)
    with pytest.raises(ValueError, match='weights'):
        frames.check_plan(plan, weights[:, :99], nbytes, total)
    with pytest.raises(ValueError, match='packed head'):
        frames.check_plan(plan, weights, total + 1, total)


# ---- 5. flag off: the parent's bytes ------------------------------------------------------------------------------------------------------------------
def test_flag_off_gives_the_bytes_of_the_parent_commit(tmp_path, caplog):
    """``prepare`` without the flag on the loader tree of tests/test_voxceleb2_loader_cpu.py (the boxed, lossless video, fine-tuning form) against
    tests/golden/frames_pad_flag_off.npz, which the commit before this feature wrote from the same tree: bit-identical, the note logged as before;
    with the flag the same batch differs and the note stays silent"""
    from latent_pose_reenactment_amd import frames
    from test_voxceleb2_loader_cpu import build_tree, loader_for, make_args, SIZE as S
    tree = build_tree(tmp_path / 'tree')
    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames_pad_flag_off.npz'))
    flags = dict(finetune=True, val_split_path=Path('id02/vidA'), batch_size=2)
    frames._deviation_logged = False
    with caplog.at_level('WARNING', logger='frames'):
        data, target = next(iter(loader_for(make_args(tree, **flags), 'val')))
        assert len([r for r in caplog.records if 'padded band' in r.getMessage()]) == 1
        raw = next(iter(loader_for(make_args(tree, **flags), 'val').loader))
        explicit = frames.prepare(raw, S, 'cpu', blur_padded_bands=False)
        frames._deviation_logged = False
        caplog.clear()
        blurred, _ = next(iter(loader_for(make_args(tree, blur_padded_bands=True, **flags), 'val')))
        assert not [r for r in caplog.records if 'padded band' in r.getMessage()]
    for key, value in (('enc_rgbs', data['enc_rgbs']), ('target_rgbs', data['target_rgbs']), ('real_segm', target['real_segm'])):
        assert value.dtype == torch.float32 and np.array_equal(value.numpy().view(np.uint32), golden[key].view(np.uint32)), key
    assert torch.equal(explicit[0]['enc_rgbs'], data['enc_rgbs']) and torch.equal(explicit[1]['real_segm'], target['real_segm'])
    assert blurred['enc_rgbs'].shape == data['enc_rgbs'].shape and not torch.equal(blurred['enc_rgbs'], data['enc_rgbs'])
