"""The frame preparation (csrc/frames.hip's header comment) without a GPU: the fp64 restatement (tests/frames_restatement.py) against the only outside
opinions available here -- torch's CPU ``interpolate`` on the float64 crop -- and ``frames.prepare_host`` (fp32 torch ops) against the restatement on
the case list that tests/test_frames_gpu.py runs through the kernel, under the same gate.

Gate (frames_restatement.gate): per element (n_y + n_x + 8) 2^-24 W, n_y = n_x the taps per axis of the row (ceil(scale) + 1 | 4 | 2), W the product of
the per-axis sum |w| (1 for area and linear, <= 1.375^2 for cubic): the fp32 dot-product bound of the two separable passes plus the weight
arithmetic.  A product is held to the sum of its image's and its mask's gate plus one rounding.
``prepare_host`` measured on the host: worst error / gate 0.15 (area), 0.31 (cubic), 0.16 (linear), 0.10 (product)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frames_restatement as FR          # noqa: E402


# ---- 1. the restatement against torch.nn.functional.interpolate in float64 --------------------------------------------------------------------------
def _plane(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, n)).astype(np.float64)


@pytest.mark.parametrize('n,size', [(32, 16), (48, 16), (40, 20), (24, 8)])
def test_restatement_area_equals_torch_area_at_integer_ratios(n, size):
    p = _plane(n, n)
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None, None], size=(size, size), mode='area')[0, 0].numpy() / 255.0
    assert np.abs(FR.resample(p, size, FR.AREA) - want).max() <= 1e-12


@pytest.mark.parametrize('n,size', [(11, 16), (5, 8), (1, 8), (63, 64), (19, 20), (7, 64)])
def test_restatement_cubic_equals_torch_bicubic_before_the_clamp(n, size):
    p = _plane(n, 100 + n)
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None, None], size=(size, size), mode='bicubic', align_corners=False)[0, 0].numpy() / 255.0
    got = FR.resample(p, size, FR.CUBIC, clamp=False)
    assert np.abs(got - want).max() <= 1e-12
    if n > 2:          # blocks of 0 and 255 overshoot on both sides: the clamp has something to do
        blocks = 255.0 * ((np.arange(n)[:, None] // 2 + np.arange(n)[None, :] // 2) % 2)
        raw, clamped = FR.resample(blocks, size, FR.CUBIC, clamp=False), FR.resample(blocks, size, FR.CUBIC)
        assert raw.min() < 0.0 and raw.max() > 1.0 and np.array_equal(clamped, np.clip(raw, 0.0, 1.0))


@pytest.mark.parametrize('n,size', [(11, 16), (5, 8), (1, 8), (63, 64), (37, 16), (127, 16), (20, 20)])
def test_restatement_linear_equals_torch_bilinear(n, size):
    p = _plane(n, 200 + n)
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None, None], size=(size, size), mode='bilinear', align_corners=False)[0, 0].numpy() / 255.0
    assert np.abs(FR.resample(p, size, FR.LINEAR) - want).max() <= 1e-12


def test_restatement_border_rules():
    buf = np.arange(12, dtype=np.uint8) * 10          # a 3 x 4 one-channel view
    img = FR.crop_plane(buf, 0, 3, 4, 4, 1, 0, -5, -7, 14, False)
    rows, cols = [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0], [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0]          # reflect-101, several periods
    assert np.array_equal(img, buf.reshape(3, 4)[np.ix_(rows, cols)].astype(np.float64))
    msk = FR.crop_plane(buf, 0, 3, 4, 4, 1, 0, -2, -2, 8, True)
    assert np.all(msk[:2] == 0) and np.array_equal(msk[2:, :], buf.reshape(3, 4)[np.ix_([0, 1, 2, 2, 2, 2], [0, 0, 0, 1, 2, 3, 3, 3])])
    assert np.array_equal(FR.crop_plane(buf, 5, 1, 1, 4, 1, 0, -3, -3, 7, False), np.full((7, 7), 50.0))          # a 1-pixel axis maps to 0


# ---- the case list (shared with tests/test_frames_gpu.py) --------------------------------------------------------------------------------------------
class Frames:
    """four decoded frames packed back to back: A 142 x 142 x 3, M 142 x 142 x 3 (a segmentation PNG: channel 1 is the mask), B 30 x 30 x 3, T 5 x 5 x 3"""

    def __init__(self):
        rng = np.random.default_rng(7)
        self.shapes = {'A': (142, 142, 3), 'M': (142, 142, 3), 'B': (30, 30, 3), 'T': (5, 5, 3), 'N': (30, 30, 1)}
        self.offsets, chunks, at = {}, [], 3          # (a frame need not start at a multiple of anything)
        chunks.append(np.zeros(3, dtype=np.uint8))
        for name, shape in self.shapes.items():
            self.offsets[name] = at
            chunks.append(rng.integers(0, 256, int(np.prod(shape)), dtype=np.uint8))
            at += chunks[-1].size
        self.buf = np.concatenate(chunks)

    def view(self, name, channel=0, border=True):
        """(off, H, W, row stride, pixel stride): the frame without its one-pixel border (or whole)"""
        h, w, c = self.shapes[name]
        off = self.offsets[name] + channel
        return [off + (w * c + c if border else 0), h - 2 * border, w - 2 * border, w * c, c]

    def image(self, name, t, l, n, size, border=True):
        return self.view(name, 0, border) + [t, l, t + n, l + n, FR.mode_for(n, size)]

    def mask(self, name, t, l, n, border=True):
        return self.view(name, 0 if self.shapes[name][2] == 1 else 1, border) + [t, l, t + n, l + n]


FRAMES = Frames()
PAIRS = {16: [16, 32, 48, 37, 127, 11], 20: [20, 45], 8: [5, 1], 64: [63, 130]}


def call(size):
    """-> (size, rows): every n -> size pair of the issue inside the view, on each side, out on all four sides, the 3 x 3 view, the masks, all in ONE
    table (rows of different sizes and modes mixed)"""
    f, rows, slots = FRAMES, [], [0, 0, 0]

    def add(image=None, mask=None, product=False):
        r = FR.row(image, mask, slots[0] if image else -1, slots[1] if mask else -1, slots[2] if product else -1)
        slots[0] += image is not None; slots[1] += mask is not None; slots[2] += product
        rows.append(r)
    for n in PAIRS[size]:
        add(f.image('A', 3, 2, n, size))                                                 # inside the 140 x 140 view
        add(f.image('A', 0, 0, n, size, border=False), f.mask('M', 0, 0, n, border=False), True)          # whole-frame views, with mask and product
        add(mask=f.mask('M', 5, 1, n))                                                   # channel 1 of 3, border removed
    n = PAIRS[size][-1] if size != 64 else 63
    for t, l in ((-7, 4), (3, -9), (140 - n + 6, 2), (1, 140 - n + 5)):                  # out on each single side of A's view
        add(f.image('A', t, l, n, size), f.mask('M', t, l, n), True)
    add(f.image('B', -10, -11, 48, size) if 48 <= 8 * size else f.image('B', -10, -11, 40, size), f.mask('N', -9, -12, 52 if 52 <= 8 * size else 40), True)
    add(f.image('T', -5, -5, 13, size), f.mask('M', -6, 138 - 13, 13))                   # the 3 x 3 view, 5 pixels out: several reflection periods
    add(mask=f.mask('N', 25, -3, 9))                                                     # left and below the 28 x 28 view of a one-channel frame
    return size, rows


def row_gates(r, size):
    n_img, n_msk = r[FR.IMG_B] - r[FR.IMG_T], r[FR.MSK_B] - r[FR.MSK_T]
    return (FR.gate(n_img, size, r[FR.IMG_MODE]) if r[FR.IMG_H] else None, FR.gate(n_msk, size, FR.LINEAR) if r[FR.MSK_H] else None,
            FR.product_gate(n_img, r[FR.IMG_MODE], n_msk, size) if r[FR.IMG_H] and r[FR.MSK_H] else None)


_WANT = {}


def restated(size):
    """the fp64 result of ``call(size)``, computed once"""
    if size not in _WANT:
        _WANT[size] = FR.prepare(FRAMES.buf, call(size)[1], size)
    return _WANT[size]


def check_against_restatement(fn, size, device='cpu'):
    """fn(buf uint8 tensor on ``device``, table int64 CPU tensor, size) -> (image, mask, product); -> worst error / gate per kind"""
    _, rows = call(size)
    got = fn(torch.from_numpy(FRAMES.buf).to(device), torch.tensor(rows, dtype=torch.int64), size)
    want = restated(size)
    worst = {'area': 0.0, 'cubic': 0.0, 'linear': 0.0, 'product': 0.0}
    for i, r in enumerate(rows):
        gates = row_gates(r, size)
        for o, (col, kind) in enumerate(((FR.IMAGE_SLOT, 'area' if r[FR.IMG_MODE] == FR.AREA else 'cubic'), (FR.MASK_SLOT, 'linear'),
                                         (FR.PRODUCT_SLOT, 'product'))):
            if r[col] < 0:
                continue
            g = got[o][r[col]].double().cpu().numpy()
            assert g.shape == (3, size, size) and np.isfinite(g).all()
            err = np.abs(g - want[o][r[col]]).max()
            worst[kind] = max(worst[kind], err / gates[o])
            assert err <= gates[o], f'row {i} ({kind}, S {size}): error {err:.3e} > gate {gates[o]:.3e}'
    for o in range(3):
        assert (got[o] is None) == (want[o] is None) and (got[o] is None or (got[o].is_contiguous() and got[o].dtype == torch.float32))
    return worst


def check_exact_copy(fn, device='cpu'):
    """n == S is a copy: exactly v / 255, image, mask and product alike"""
    f = FRAMES
    for size in (16, 20):
        rows = [FR.row(f.image('A', 3, 2, size, size), f.mask('M', 5, 1, size), 0, 0, 0)]
        image, mask, product = fn(torch.from_numpy(f.buf).to(device), torch.tensor(rows, dtype=torch.int64), size)
        a = torch.from_numpy(f.buf[f.offsets['A']:][:142 * 142 * 3].reshape(142, 142, 3))[1 + 3:1 + 3 + size, 1 + 2:1 + 2 + size].permute(2, 0, 1)
        m = torch.from_numpy(f.buf[f.offsets['M']:][:142 * 142 * 3].reshape(142, 142, 3))[1 + 5:1 + 5 + size, 1 + 1:1 + 1 + size, 1]
        a, m = a.to(torch.float32) / 255, (m.to(torch.float32) / 255)[None].expand(3, size, size)
        assert torch.equal(image[0].cpu(), a) and torch.equal(mask[0].cpu(), m) and torch.equal(product[0].cpu(), a * m)


def check_refusals(fn, device='cpu'):
    f = FRAMES
    buf = torch.from_numpy(f.buf).to(device)
    table = lambda rows: torch.tensor(rows, dtype=torch.int64)
    with pytest.raises(ValueError, match=r'row 1.*scale above 8'):
        fn(buf, table([FR.row(f.image('A', 0, 0, 16, 16), image_slot=0), FR.row(f.image('A', 0, 0, 129, 16), image_slot=1)]), 16)
    with pytest.raises(ValueError, match=r'row 0.*mask.*scale above 8'):
        fn(buf, table([FR.row(mask=f.mask('M', 0, 0, 70), mask_slot=0)]), 8)
    outside = f.image('A', 0, 0, 16, 16)
    outside[0] = f.buf.size - 100
    with pytest.raises(ValueError, match=r'row 0.*outside the buffer'):
        fn(buf, table([FR.row(outside, image_slot=0)]), 16)
    negative = f.image('A', 0, 0, 16, 16)
    negative[0] = -1
    with pytest.raises(ValueError, match=r'outside the buffer'):
        fn(buf, table([FR.row(negative, image_slot=0)]), 16)
    oblong = f.image('A', 0, 0, 16, 16)
    oblong[8] += 1
    with pytest.raises(ValueError, match=r'row 0.*not square'):
        fn(buf, table([FR.row(oblong, image_slot=0)]), 16)
    with pytest.raises(ValueError, match=r'mode'):
        fn(buf, table([FR.row(f.image('A', 0, 0, 16, 16)[:9] + [FR.CUBIC], image_slot=0)]), 16)
    with pytest.raises(ValueError, match=r'no mask view'):
        fn(buf, table([FR.row(f.image('A', 0, 0, 16, 16), image_slot=0, product_slot=0)]), 16)
    with pytest.raises(ValueError, match=r'slots'):
        fn(buf, table([FR.row(f.image('A', 0, 0, 16, 16), image_slot=1)]), 16)


# ---- 2. prepare_host against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [8, 16, 20, 64])
def test_prepare_host_against_the_restatement(size):
    from latent_pose_reenactment_amd import frames
    worst = check_against_restatement(frames.prepare_host, size)
    print(f'[frames] prepare_host, S {size}: worst error / gate ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))


def test_prepare_host_copies_exactly_and_refuses_what_the_definition_does_not_cover():
    from latent_pose_reenactment_amd import frames
    check_exact_copy(frames.prepare_host)
    check_refusals(frames.prepare_host)


def test_product_is_image_times_mask_and_a_row_alone_gives_the_same_bits():
    from latent_pose_reenactment_amd import frames
    size, rows = call(16)
    buf = torch.from_numpy(FRAMES.buf)
    image, mask, product = frames.prepare_host(buf, torch.tensor(rows, dtype=torch.int64), size)
    for r in rows:
        if r[FR.PRODUCT_SLOT] >= 0:
            assert torch.equal(product[r[FR.PRODUCT_SLOT]], image[r[FR.IMAGE_SLOT]] * mask[r[FR.MASK_SLOT]])
            alone = FR.row(r[FR.IMG_OFF:FR.IMG_MODE + 1], r[FR.MSK_OFF:FR.MSK_R + 1], 0, 0, 0)
            one = frames.prepare_host(buf, torch.tensor([alone], dtype=torch.int64), size)
            assert torch.equal(one[0][0], image[r[FR.IMAGE_SLOT]]) and torch.equal(one[2][0], product[r[FR.PRODUCT_SLOT]])


def test_table_builder_restates_the_reference_arithmetic():
    from latent_pose_reenactment_amd import frames
    # no bounding box: the whole frame, which the reference's own arithmetic pads by 1 at the top and left and 2 at the bottom and right
    cols = frames.frame_rows(100, (40, 40, 3), (0.0, 0.0, 1.0, 1.0), 32)
    assert cols == [100 + 40 * 3 + 3, 38, 38, 120, 3, -1, -1, 40, 40, frames.MODE_AREA]
    assert frames.frame_rows(7, (40, 40, 3), (0.0, 0.0, 1.0, 1.0), 32, channel=1) == [7 + 120 + 3 + 1, 38, 38, 120, 3, -1, -1, 40, 40]
    assert frames.frame_rows(0, (40, 40, 3), (0.0, 0.0, 1.0, 1.0), 64)[-1] == frames.MODE_CUBIC
    assert frames.bbox_to_integer_coords(0.1, 0.26, 0.52, 0.7, 100, 100) == (10, 26, 55, 71)
    t, l, b, r = frames.scaled_square_box(0.25, 0.5, 0.75, 0.75)
    assert (t, l, b, r) == (0.625 - 0.45, 0.5 - 0.45, 0.625 + 0.45, 0.5 + 0.45)
    with pytest.raises(ValueError):
        frames.frame_rows(0, (2, 2, 3), (0.0, 0.0, 1.0, 1.0), 32)
