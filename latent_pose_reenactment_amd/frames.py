"""From decoded frames to the batch (reference: SampleLoader.load_sample, dataloaders/voxceleb2_segmentation_nolandmarks.py:89-175, and its
``crop_with_padding``, :283-367): the LOADER decodes uint8 frames and packs them back to back; the PIXELS -- crop to the bounding box through the
border rule, resize to the network's resolution, / 255, image x segmentation -- are made where the batch is consumed: one lp_frames_prepare launch
on the GPU (``hipops.frames_prepare``), or ``prepare_host`` -- the same definition in fp32 torch ops -- for CPU tensors.  The definition is the
header comment of csrc/frames.hip; tests/frames_restatement.py restates it in fp64.

What the reference does beyond that where a box leaves its frame -- the blur of the padded bands and their fade to the median colour
(``crop_with_padding``, :314-359) -- is opt-in (``blur_padded_bands``; the loader's ``--blur_padded_bands``) and defined by the header comment of
csrc/frames_pad.hip (fp64: tests/frames_pad_restatement.py).  ``pad_plan`` finds the affected views and gives each a dense uint8 n x n image in a
workspace behind the packed frames; ``hipops.frames_pad`` (lp_frames_pad) or ``pad_host`` fills those images; the preparation then runs unchanged
on the rewritten table, in which they are plain in-view boxes.  Without the flag padded bands carry the border rule's pixels as they are.

A table row (``COLUMNS``, int64) describes one output image: an image view with its box and mode, a mask view with its box, and the slot each of
the three outputs (image, mask, product) is written to (-1: not written).  A raw batch, as the loader's collate function makes it:
  buf     uint8 [bytes]      the decoded frames of the batch, packed
  table   int64 [R, 24]      offsets relative to ``buf``
  frames  K                  encoder frames per sample (slots b K + k of ``image``); 0: ``enc_rgbs`` and ``pose_input_rgbs`` are one image
  pose    bool               rows with the pose image follow at the slots B K + b
  label   int64 [B]          (+ aug_params [B, 32] / aug_params_extra [B, 16] when the loader augments)"""
import functools
import logging
import math

import torch

logger = logging.getLogger('frames')

COLUMNS = ('img_off', 'img_h', 'img_w', 'img_row_stride', 'img_pixel_stride', 'img_t', 'img_l', 'img_b', 'img_r', 'img_mode',
           'msk_off', 'msk_h', 'msk_w', 'msk_row_stride', 'msk_pixel_stride', 'msk_t', 'msk_l', 'msk_b', 'msk_r',
           'image_slot', 'mask_slot', 'product_slot', 'reserved0', 'reserved1')
NCOLS = len(COLUMNS)
MODE_AREA, MODE_CUBIC = 0, 1
MAX_SCALE = 8
MAX_SIZE = 4096
MAX_COORD = 1 << 30
CUBIC_A = -0.75
_IMG, _MSK, _SLOTS = 0, 10, 19
PLAN_COLUMNS = ('row', 'view', 'off', 'h', 'w', 'row_stride', 'pixel_stride', 't', 'l', 'n', 'pad_t', 'pad_l', 'pad_b', 'pad_r', 'k', 'ws_off')
NPLAN = len(PLAN_COLUMNS)
PAD_MAX_N = 1024                # k <= 99: the halo of a 16 x 16 tile, three channels, still fits LDS
PAD_WEIGHT_ROW = 100
PAD_ALIGN = 16


def bbox_to_integer_coords(t, l, b, r, image_h, image_w):
    """(t, l, b, r) of a box in the unit square -> integer pixel coordinates, b and r exclusive, exactly square -- the reference's function (:253-281),
    its use of the HEIGHT for both axes included (the frames are square)"""
    t, l, b, r = t * image_h, l * image_h, b * image_h, r * image_h
    l, t = math.floor(l), math.floor(t)
    r, b = math.ceil(r), math.ceil(b)
    b += (r - l) - (b - t)
    return t, l, b + 1, r + 1


def scaled_square_box(l, t, r, b, scale=1.8):
    """a detector's box in the unit square -> the square box around its centre, ``scale`` times its longer side (:103-112) -> (t, l, b, r)"""
    cx, cy = (l + r) * 0.5, (t + b) * 0.5
    half = max(b - t, r - l) / 2 * scale
    return cy - half, cx - half, cy + half, cx + half


def mode_for(n, size):
    """cv2.INTER_CUBIC if imsize > b - t else cv2.INTER_AREA (:135-136)"""
    return MODE_AREA if size <= n else MODE_CUBIC


def view_without_border(offset, h, w, channels, channel=0):
    """the view ``frame[1:-1, 1:-1, channel:]`` of an H x W x channels frame stored densely at ``offset`` (the reference drops the dataset's one-pixel
    grey border, :125 and :162) -> (off, H, W, row stride, pixel stride): arithmetic, no copy"""
    if h < 3 or w < 3:
        raise ValueError(f'a {h} x {w} frame has nothing inside its one-pixel border')
    return offset + w * channels + channels + channel, h - 2, w - 2, w * channels, channels


def frame_rows(offset, shape, box, size, channel=None):
    """the columns of one view and its box: ``shape`` (H, W, channels) of the decoded frame at ``offset``, ``box`` (t, l, b, r) in the unit square
    -> [off, H, W, row stride, pixel stride, t, l, b, r] (+ [mode] for an image, ``channel is None``)"""
    h, w, c = shape
    t, l, b, r = bbox_to_integer_coords(*box, h, w)
    off, vh, vw, rs, ps = view_without_border(offset, h, w, c, 0 if channel is None else channel)
    cols = [off, vh, vw, rs, ps, t - 1, l - 1, b - 1, r - 1]
    return cols + [mode_for(b - t, size)] if channel is None else cols


def make_row(image=None, mask=None, image_slot=-1, mask_slot=-1, product_slot=-1):
    row = [0] * NCOLS
    if image is not None:
        row[_IMG:_IMG + 10] = image
    if mask is not None:
        row[_MSK:_MSK + 9] = mask
    row[_SLOTS:_SLOTS + 3] = [image_slot, mask_slot, product_slot]
    return row


def check_table(table, nbytes, size):
    """-> (image, mask, product) slot counts; ValueError naming the row for anything the definition does not cover"""
    if not (torch.is_tensor(table) and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == NCOLS and table.shape[0] >= 1):
        raise ValueError(f'frames: the table must be an int64 tensor [rows >= 1, {NCOLS}]')
    if table.is_cuda:
        raise ValueError('frames: the table is a HOST tensor (it is checked before the launch)')
    if not 1 <= size <= MAX_SIZE:
        raise ValueError(f'frames: size must be in 1 .. {MAX_SIZE}, got {size}')
    rows = table.tolist()
    seen = ([], [], [])
    for i, r in enumerate(rows):
        has = [r[_IMG + 1] != 0, r[_MSK + 1] != 0]
        slots = r[_SLOTS:_SLOTS + 3]
        if any(s < -1 for s in slots) or all(s < 0 for s in slots):
            raise ValueError(f'frames: row {i} writes no output (slots {slots})')
        if (slots[0] >= 0 or slots[2] >= 0) and not has[0]:
            raise ValueError(f'frames: row {i} asks for an image output but has no image view')
        if (slots[1] >= 0 or slots[2] >= 0) and not has[1]:
            raise ValueError(f'frames: row {i} asks for a mask output but has no mask view')
        for what, base, chans, present in (('image', _IMG, 3, has[0]), ('mask', _MSK, 1, has[1])):
            if not present:
                continue
            off, h, w, rs, ps, t, l, b, rr = r[base:base + 9]
            n = b - t
            if n != rr - l or n < 1:
                raise ValueError(f'frames: row {i}: the {what} box t {t}, l {l}, b {b}, r {rr} is not square with side >= 1')
            if h < 1 or w < 1 or rs < 0 or ps < 0 or off < 0 or off + (h - 1) * rs + (w - 1) * ps + chans > nbytes:
                raise ValueError(f'frames: row {i}: the {what} view (offset {off}, {h} x {w}, strides {rs}, {ps}) lies outside the buffer of {nbytes} bytes')
            if max(abs(t), abs(l), h, w) >= MAX_COORD:
                raise ValueError(f'frames: row {i}: the {what} box or view exceeds 2^30')
            if n > MAX_SCALE * size:
                raise ValueError(f'frames: row {i}: the {what} crop {n} -> {size} is a scale above {MAX_SCALE}')
            if what == 'image' and r[base + 9] != mode_for(n, size):
                raise ValueError(f'frames: row {i}: mode {r[base + 9]} for {n} -> {size} (area = {MODE_AREA} when size <= n, else cubic = {MODE_CUBIC})')
        for k in range(3):
            if slots[k] >= 0:
                seen[k].append(slots[k])
    for k, name in enumerate(('image', 'mask', 'product')):
        if sorted(seen[k]) != list(range(len(seen[k]))):
            raise ValueError(f'frames: the {name} slots of the table are not 0 .. {len(seen[k]) - 1}, each once')
    return tuple(len(s) for s in seen)


# ---- the definition in fp32 torch ops (host) --------------------------------------------------------------------------------------------------------
def _reflect101(i, n):
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    m = torch.remainder(i, p)
    return torch.where(m < n, m, p - m)


def _crop(buf, off, h, w, rs, ps, chans, t, l, n, mask):
    ys, xs = t + torch.arange(n, dtype=torch.int64), l + torch.arange(n, dtype=torch.int64)
    if mask:
        above = ys < 0
        ys, xs = ys.clamp(0, h - 1), xs.clamp(0, w - 1)
    else:
        ys, xs = _reflect101(ys, h), _reflect101(xs, w)
    index = off + ys[:, None] * rs + xs[None, :] * ps
    crop = torch.stack([buf[index + c] for c in range(chans)]).to(torch.float32)
    if mask:
        crop[:, above, :] = 0.0
    return crop


def _axis_taps(mode, n, size):
    """-> (index [size, K] int64 clamped to the crop, weight [size, K] fp32; unused taps weigh 0), the weights formed in fp32 from exact integers"""
    d = torch.arange(size, dtype=torch.int64)
    if mode == MODE_AREA:
        first, end = (d * n) // size, ((d + 1) * n + size - 1) // size
        k = torch.arange(int((end - first).max()), dtype=torch.int64)
        j = first[:, None] + k[None, :]
        overlap = (torch.minimum((j + 1) * size, ((d + 1) * n)[:, None]) - torch.maximum(j * size, (d * n)[:, None])).clamp(min=0)
        return j.clamp(0, n - 1), overlap.to(torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    num, den = (2 * d + 1) * n - size, 2 * size
    q = torch.div(num, den, rounding_mode='floor')
    f = (num - q * den).to(torch.float32) / torch.tensor(float(den), dtype=torch.float32)
    if mode == 2:
        return (q[:, None] + torch.arange(2)[None, :]).clamp(0, n - 1), torch.stack([1.0 - f, f], dim=1)
    a = CUBIC_A
    g, e = f + 1.0, 1.0 - f
    w0 = ((a * g - 5.0 * a) * g + 8.0 * a) * g - 4.0 * a
    w1 = ((a + 2.0) * f - (a + 3.0)) * f * f + 1.0
    w2 = ((a + 2.0) * e - (a + 3.0)) * e * e + 1.0
    w3 = 1.0 - w0 - w1 - w2
    return (q[:, None] - 1 + torch.arange(4)[None, :]).clamp(0, n - 1), torch.stack([w0, w1, w2, w3], dim=1)


def _resample(crop, size, mode):
    """[C, n, n] raw values -> [C, size, size] in [0, 1]: horizontal pass, vertical pass (taps added up in order from 0), clamp (cubic), / 255"""
    n = crop.shape[-1]
    index, weight = _axis_taps(mode, n, size)
    mid = torch.zeros(crop.shape[0], n, size, dtype=torch.float32)
    for k in range(index.shape[1]):
        mid = mid + crop[:, :, index[:, k]] * weight[None, None, :, k]
    out = torch.zeros(crop.shape[0], size, size, dtype=torch.float32)
    for k in range(index.shape[1]):
        out = out + mid[:, index[:, k], :] * weight[None, :, k, None]
    if mode == MODE_CUBIC:
        out = out.clamp(0.0, 255.0)
    return out / 255.0


# ---- the padded bands (csrc/frames_pad.hip) ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def blur_taps(n):
    """-> the k Gaussian taps g[-R .. R] of a crop of side n, in fp64: k = cvRound(6 sigma + 1) | 1 with sigma = 0.016 n, in integers (no ties)"""
    k = ((96 * n + 1500) // 1000) | 1
    radius, sigma = (k - 1) // 2, 0.016 * n
    g = [math.exp(-(a * a) / (2.0 * sigma * sigma)) for a in range(-radius, radius + 1)]
    total = sum(g)
    return tuple(v / total for v in g)


def pad_plan(table, nbytes, size):
    """the views of ``table`` whose box leaves them -> (rewritten table, plan int64 [P, 16] (``PLAN_COLUMNS``), weights fp32 [P, 100], total bytes).
    Each such view gets a dense uint8 [n, n, C] image at ``ws_off`` (16-byte aligned) behind the ``nbytes`` packed bytes, and in the rewritten table it
    is that image with the box 0, 0, n, n and the same mode; a row whose boxes lie inside their views is not touched and takes no workspace.  Pure
    integer arithmetic on the host (the reserved columns are not read); ValueError naming the row for a padded crop above ``PAD_MAX_N``."""
    check_table(table, nbytes, size)
    rows = table.tolist()
    plan, weights, end = [], [], nbytes
    for i, r in enumerate(rows):
        for view, (what, base, chans) in enumerate((('image', _IMG, 3), ('mask', _MSK, 1))):
            if not r[base + 1]:
                continue
            off, h, w, rs, ps, t, l, b, rr = r[base:base + 9]
            n = b - t
            pads = [max(0, -t), max(0, -l), max(0, b - h), max(0, rr - w)]
            if not any(pads):
                continue
            if n > PAD_MAX_N:
                raise ValueError(f'frames: row {i}: the padded {what} crop of {n} is above {PAD_MAX_N} (the blur of the padded bands supports k <= 99)')
            g = blur_taps(n)
            ws = (end + PAD_ALIGN - 1) // PAD_ALIGN * PAD_ALIGN
            end = ws + n * n * chans
            plan.append([i, view, off, h, w, rs, ps, t, l, n] + pads + [len(g), ws])
            weights.append(list(g) + [0.0] * (PAD_WEIGHT_ROW - len(g)))
            r[base:base + 9] = [ws, n, n, n * chans, chans, 0, 0, n, n]
    return (torch.tensor(rows, dtype=torch.int64), torch.tensor(plan, dtype=torch.int64).reshape(-1, NPLAN),
            torch.tensor(weights, dtype=torch.float64).to(torch.float32).reshape(-1, PAD_WEIGHT_ROW), end)


def check_plan(plan, weights, head_bytes, buf_bytes):
    """ValueError naming the plan row for anything lp_frames_pad would refuse (the same rules, before any device work)"""
    if not (torch.is_tensor(plan) and plan.dtype == torch.int64 and plan.dim() == 2 and plan.shape[1] == NPLAN and plan.shape[0] >= 1 and not plan.is_cuda):
        raise ValueError(f'frames: the plan must be an int64 HOST tensor [plans >= 1, {NPLAN}]')
    if not (torch.is_tensor(weights) and weights.dtype == torch.float32 and tuple(weights.shape) == (plan.shape[0], PAD_WEIGHT_ROW) and not weights.is_cuda):
        raise ValueError(f'frames: the weights must be an fp32 HOST tensor [{plan.shape[0]}, {PAD_WEIGHT_ROW}]')
    if not 0 <= head_bytes <= buf_bytes:
        raise ValueError(f'frames: the packed head of {head_bytes} bytes must lie inside the buffer of {buf_bytes} bytes')
    end = head_bytes
    for i, (row, view, off, h, w, rs, ps, t, l, n, pt, pl, pb, pr, k, ws) in enumerate(plan.tolist()):
        if view not in (0, 1):
            raise ValueError(f'frames: plan {i} (row {row}): view {view} is neither 0 (image) nor 1 (mask)')
        chans = 1 if view else 3
        if n < 1:
            raise ValueError(f'frames: plan {i} (row {row}): the crop has side {n} < 1')
        if n > PAD_MAX_N:
            raise ValueError(f'frames: plan {i} (row {row}): the padded crop of {n} is above {PAD_MAX_N}')
        if h < 1 or w < 1 or rs < 0 or ps < 0 or off < 0 or max(abs(t), abs(l), h, w, rs, ps) >= MAX_COORD or off + (h - 1) * rs + (w - 1) * ps + chans > head_bytes:
            raise ValueError(f'frames: plan {i} (row {row}): the view (offset {off}, {h} x {w}, strides {rs}, {ps}) lies outside the packed head of '
                             f'{head_bytes} bytes')
        pads = [max(0, -t), max(0, -l), max(0, t + n - h), max(0, l + n - w)]
        if pads != [pt, pl, pb, pr] or not any(pads):
            raise ValueError(f'frames: plan {i} (row {row}): the pads {[pt, pl, pb, pr]} are not those of a box that leaves its view ({pads})')
        if k != ((96 * n + 1500) // 1000) | 1:
            raise ValueError(f'frames: plan {i} (row {row}): k {k} is not ((96 n + 1500) // 1000) | 1 for n {n}')
        if ws < end or ws % PAD_ALIGN or ws + n * n * chans > buf_bytes:
            raise ValueError(f'frames: plan {i} (row {row}): the workspace image at {ws} ({PAD_ALIGN}-byte aligned, behind the head and the images '
                             f'before it) does not fit the buffer of {buf_bytes} bytes')
        end = ws + n * n * chans


def _blend(x, y, w):
    """x + (y - x) w; a weight of exactly 0 returns x, of exactly 1 returns y"""
    return torch.where(w <= 0, x, torch.where(w >= 1, y, x + (y - x) * w))


def _side(n, p0, p1):
    """1 - min(i / p0, (n - 1 - i) / p1) for i = 0 .. n - 1 in fp32; a term whose pad is 0 is +inf"""
    i = torch.arange(n, dtype=torch.float32)
    inf = torch.full((n,), float('inf'), dtype=torch.float32)
    u = i / torch.tensor(float(p0), dtype=torch.float32) if p0 else inf
    v = (n - 1 - i) / torch.tensor(float(p1), dtype=torch.float32) if p1 else inf
    return 1.0 - torch.minimum(u, v)


def _pad_view(buf, p, g):
    """one plan row -> uint8 [n, n, C]: the definition of csrc/frames_pad.hip in fp32 torch ops"""
    _, view, off, h, w, rs, ps, t, l, n, pt, pl, pb, pr, k, _ = p
    chans, mask = (1, True) if view else (3, False)
    crop = _crop(buf, off, h, w, rs, ps, chans, t, l, n, mask)
    radius = (k - 1) // 2
    index = _reflect101(torch.arange(-radius, n + radius, dtype=torch.int64), n)
    ext = crop[:, :, index]
    mid = torch.zeros_like(crop)
    for q in range(k):
        mid = mid + ext[:, :, q:q + n] * g[q]
    ext = mid[:, index, :]
    blur = torch.zeros_like(crop)
    for q in range(k):
        blur = blur + ext[:, q:q + n, :] * g[q]
    mh, mv = _side(n, pl, pr)[None, :], _side(n, pt, pb)[:, None]
    m = torch.maximum(mh, mv)
    a = (3.0 * m + 1.0).clamp(0.0, 1.0)
    f = (mh.expand(n, n) if mask else m).clamp(0.0, 1.0)
    if mask:
        fade = torch.zeros(1, 1, 1, dtype=torch.float32)
    else:
        v = crop.reshape(chans, -1).sort(dim=1).values
        fade = ((v[:, (n * n - 1) // 2] + v[:, (n * n) // 2]) / 2.0)[:, None, None]
    y = _blend(_blend(crop, blur, a[None]), fade.expand_as(crop), f[None])
    return y.round().clamp(0.0, 255.0).to(torch.uint8).permute(1, 2, 0).contiguous()


def pad_host(buf, table, size):
    """``pad_plan`` and ``hipops.frames_pad`` for CPU tensors -> (buffer of the plan's total size: ``buf``, then the workspace images; rewritten table)"""
    if not (torch.is_tensor(buf) and buf.dtype == torch.uint8 and buf.dim() == 1 and not buf.is_cuda):
        raise ValueError('frames.pad_host: buf must be a 1-D uint8 CPU tensor')
    table2, plan, weights, total = pad_plan(table, buf.numel(), size)
    out = torch.zeros(total, dtype=torch.uint8)
    out[:buf.numel()] = buf
    for p, g in zip(plan.tolist(), weights):
        n, chans, ws = p[9], 1 if p[1] else 3, p[15]
        out[ws:ws + n * n * chans] = _pad_view(buf, p, g).reshape(-1)
    return out, table2


def prepare_host(buf, table, size, blur_padded_bands=False):
    """``hipops.frames_prepare`` for CPU tensors: (image, mask, product), fp32 [slots, 3, size, size] each, None where no row asks;
    ``blur_padded_bands``: through ``pad_host`` first"""
    if not (torch.is_tensor(buf) and buf.dtype == torch.uint8 and buf.dim() == 1 and not buf.is_cuda):
        raise ValueError('frames.prepare_host: buf must be a 1-D uint8 CPU tensor')
    if blur_padded_bands:
        buf, table = pad_host(buf, table, size)
    counts = check_table(table, buf.numel(), size)
    outs = [torch.empty(c, 3, size, size, dtype=torch.float32) if c else None for c in counts]
    for r in table.tolist():
        img = msk = None
        if r[_IMG + 1]:
            img = _resample(_crop(buf, *r[_IMG:_IMG + 5], 3, r[_IMG + 5], r[_IMG + 6], r[_IMG + 7] - r[_IMG + 5], False), size, r[_IMG + 9])
        if r[_MSK + 1]:
            msk = _resample(_crop(buf, *r[_MSK:_MSK + 5], 1, r[_MSK + 5], r[_MSK + 6], r[_MSK + 7] - r[_MSK + 5], True), size, 2)
        s_img, s_msk, s_prod = r[_SLOTS:_SLOTS + 3]
        if s_img >= 0:
            outs[0][s_img] = img
        if s_msk >= 0:
            outs[1][s_msk] = msk.expand(3, size, size)
        if s_prod >= 0:
            outs[2][s_prod] = img * msk
    return tuple(outs)


_deviation_logged = False


def note_padding(table):
    """logs the deviation from the reference once, the first time a box leaves its view by more than 2 pixels"""
    global _deviation_logged
    if _deviation_logged:
        return
    for base in (_IMG, _MSK):
        h, w, t, l, b, r = (table[:, base + c] for c in (1, 2, 5, 6, 7, 8))
        out = torch.stack([-t, -l, b - h, r - w]).amax(dim=0)
        if bool(((h > 0) & (out > 2)).any()):
            _deviation_logged = True
            logger.warning('a bounding box leaves its frame by more than 2 pixels: the padded band carries the border rule\'s pixels as they are '
                           '(reflected image, replicated mask); the reference also blurs the band and fades it to the median colour '
                           '(crop_with_padding): pass --blur_padded_bands for that')
            return


STATUS_WORDS = {1: 'no Huffman code of <= 16 bits matches', 2: 'a run of zeros leaves its block', 3: 'a segment ends inside a code'}


def check_decoded(pending):
    """the decode status words ``_prepare_decoding`` sent on their way to pinned memory: waits for each copy's event, empties the list and raises
    ValueError naming the first file whose stream did not decode"""
    while pending:
        status, event, files = pending.pop(0)
        if event is not None:
            event.synchronize()
        bad = torch.nonzero(status).reshape(-1).tolist()
        if bad:
            pending.clear()
            code = int(status[bad[0]])
            raise ValueError(f'{files[bad[0]]}: the JPEG stream does not decode ({STATUS_WORDS.get(code, code)}; status {code}); '
                             f'{len(bad)} of the {len(files)} JPEG frames of the batch are affected')


def _prepare_decoding(raw_batch, size, device, blur_padded_bands, pending):
    """``prepare`` for a raw batch of ``--decode_jpeg_on_gpu``: 'buf' holds only the regions the workers decoded (masks, fallback frames), 'regions'
    int64 [n, 3] = (offset in the decoded layout, offset in 'buf', length), 'nbytes' the size of the decoded layout -- which the table describes,
    identical to the PIL route's -- and 'jpeg' the packed segments of the other frames (``utils.jpeg_parse.merge``), 'files' their paths.
    -> (image, mask, product).  On a GPU, in this order: ONE device buffer at the decoded size (the pad plan's total with ``blur_padded_bands``), the
    regions copied into it from pinned memory, the decode launches (``hipops.jpeg_decode``) into the rest, then the existing launches; no host
    synchronisation anywhere: the per-frame status goes to pinned memory with a non-blocking copy and is appended, with its event, to ``pending``
    (``check_decoded``).  CPU: the same through ``hipops.jpeg_decode_host`` and ``prepare_host``, the status checked at once."""
    from latent_pose_reenactment_amd import hipops
    buf, table, nbytes, jpeg = raw_batch['buf'], raw_batch['table'], int(raw_batch['nbytes']), raw_batch['jpeg']
    regions = []
    for d, s, n in raw_batch['regions'].tolist():          # neighbours in both layouts (a mask behind its fallback frame, ...) travel as one copy
        if regions and regions[-1][0] + regions[-1][2] == d and regions[-1][1] + regions[-1][2] == s:
            regions[-1][2] += n
        else:
            regions.append([d, s, n])
    if any(d < 0 or s < 0 or n < 0 or d + n > nbytes or s + n > buf.numel() for d, s, n in regions):
        raise ValueError(f'frames: a region of the raw batch lies outside the decoded layout of {nbytes} bytes or the {buf.numel()} bytes held')
    if device.type != 'cuda':
        full = torch.zeros(nbytes, dtype=torch.uint8)
        for d, s, n in regions:
            full[d:d + n] = buf[s:s + n]
        if jpeg is not None:
            check_decoded([(hipops.jpeg_decode_host(jpeg, out=full).status, None, raw_batch['files'])])
        return prepare_host(full, table, size, blur_padded_bands)
    if not buf.is_pinned():
        buf = buf.pin_memory()
    plan = pad_plan(table, nbytes, size) if blur_padded_bands else None
    padded = plan is not None and plan[1].shape[0]
    dev = torch.empty(plan[3] if padded else nbytes, dtype=torch.uint8, device=device)
    for d, s, n in regions:
        dev[d:d + n].copy_(buf[s:s + n], non_blocking=True)
    if jpeg is not None:
        status = hipops.jpeg_decode(jpeg, out=dev).status
        host = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        if pending is None:
            check_decoded([(host, event, raw_batch['files'])])
        else:
            pending.append((host, event, raw_batch['files']))
    if padded:
        return hipops.frames_prepare(hipops.frames_pad(dev, nbytes, plan[1], plan[2]), plan[0], size)
    return hipops.frames_prepare(dev, table, size)


def prepare(raw_batch, size, device, blur_padded_bands=False, pending=None):
    """a raw batch (module docstring) -> the standard (data_dict, target_dict), fp32 on ``device``: ``enc_rgbs`` B x K x 3 x S x S,
    ``pose_input_rgbs``, ``target_rgbs`` B x 1 x 3 x S x S, ``real_segm`` B x 1 x 3 x S x S, ``label`` -- whichever the rows of the table write.
    On a GPU: one pinned host-to-device copy of the packed bytes, then one launch on the current stream.  ``blur_padded_bands``: a batch with a box
    that leaves its view gets ONE device buffer of the plan's total size, the pinned bytes copied into its head, the pad launches
    (``hipops.frames_pad``) and then the same one launch on the rewritten table.  A batch of ``--decode_jpeg_on_gpu`` (it has 'jpeg'): see
    ``_prepare_decoding``; ``pending`` is the caller's list for the status words (without one they are waited for and checked here)."""
    buf, table, label = raw_batch['buf'], raw_batch['table'], raw_batch['label']
    device = torch.device(device)
    if not blur_padded_bands:
        note_padding(table)
    if 'jpeg' in raw_batch:
        image, mask, product = _prepare_decoding(raw_batch, size, device, blur_padded_bands, pending)
    elif device.type == 'cuda':
        from latent_pose_reenactment_amd import hipops
        if not buf.is_pinned():
            buf = buf.pin_memory()
        plan = pad_plan(table, buf.numel(), size) if blur_padded_bands else None
        if plan is not None and plan[1].shape[0]:
            table, rows, weights, total = plan
            dev = torch.empty(total, dtype=torch.uint8, device=device)
            dev[:buf.numel()].copy_(buf, non_blocking=True)
            image, mask, product = hipops.frames_prepare(hipops.frames_pad(dev, buf.numel(), rows, weights), table, size)
        else:
            image, mask, product = hipops.frames_prepare(buf.to(device, non_blocking=True), table, size)
    else:
        image, mask, product = prepare_host(buf, table, size, blur_padded_bands)
    b, k = label.shape[0], int(raw_batch['frames'])
    data_dict, target_dict = {}, {}
    if k == 0:                  # fine-tuning: the one image is encoder input and pose input alike (:200-202)
        data_dict['enc_rgbs'] = data_dict['pose_input_rgbs'] = image.view(b, 1, 3, size, size)
    else:
        data_dict['enc_rgbs'] = image[:b * k].view(b, k, 3, size, size)
        if raw_batch['pose']:
            data_dict['pose_input_rgbs'] = image[b * k:].view(b, 1, 3, size, size)
    if product is not None:
        data_dict['target_rgbs'] = product.view(b, 1, 3, size, size)
    if mask is not None:
        target_dict['real_segm'] = mask.view(b, 1, 3, size, size)
    if 'aug_params' in raw_batch:
        data_dict['aug_params'] = raw_batch['aug_params'].to(device, non_blocking=True)
    if 'aug_params_extra' in raw_batch:
        data_dict['aug_params_extra'] = raw_batch['aug_params_extra'].to(device, non_blocking=True)
    target_dict['label'] = label.to(device, non_blocking=True)
    return data_dict, target_dict
