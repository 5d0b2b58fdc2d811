"""From decoded frames to the batch (reference: SampleLoader.load_sample, dataloaders/voxceleb2_segmentation_nolandmarks.py:89-175, and its
``crop_with_padding``, :283-367): the LOADER decodes uint8 frames and packs them back to back; the PIXELS -- crop to the bounding box through the
border rule, resize to the network's resolution, / 255, image x segmentation -- are made where the batch is consumed: one lp_frames_prepare launch
on the GPU (``hipops.frames_prepare``), or ``prepare_host`` -- the same definition in fp32 torch ops -- for CPU tensors.  The definition, and what
it leaves out of the reference (the blur and fade of the padded bands), is the header comment of csrc/frames.hip; tests/frames_restatement.py
restates it in fp64.

A table row (``COLUMNS``, int64) describes one output image: an image view with its box and mode, a mask view with its box, and the slot each of
the three outputs (image, mask, product) is written to (-1: not written).  A raw batch, as the loader's collate function makes it:
  buf     uint8 [bytes]      the decoded frames of the batch, packed
  table   int64 [R, 24]      offsets relative to ``buf``
  frames  K                  encoder frames per sample (slots b K + k of ``image``); 0: ``enc_rgbs`` and ``pose_input_rgbs`` are one image
  pose    bool               rows with the pose image follow at the slots B K + b
  label   int64 [B]          (+ aug_params [B, 32] / aug_params_extra [B, 16] when the loader augments)"""
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


def prepare_host(buf, table, size):
    """``hipops.frames_prepare`` for CPU tensors: (image, mask, product), fp32 [slots, 3, size, size] each, None where no row asks"""
    if not (torch.is_tensor(buf) and buf.dtype == torch.uint8 and buf.dim() == 1 and not buf.is_cuda):
        raise ValueError('frames.prepare_host: buf must be a 1-D uint8 CPU tensor')
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
                           '(crop_with_padding), which is not provided')
            return


def prepare(raw_batch, size, device):
    """a raw batch (module docstring) -> the standard (data_dict, target_dict), fp32 on ``device``: ``enc_rgbs`` B x K x 3 x S x S,
    ``pose_input_rgbs``, ``target_rgbs`` B x 1 x 3 x S x S, ``real_segm`` B x 1 x 3 x S x S, ``label`` -- whichever the rows of the table write.
    On a GPU: one pinned host-to-device copy of the packed bytes, then one launch on the current stream."""
    buf, table, label = raw_batch['buf'], raw_batch['table'], raw_batch['label']
    device = torch.device(device)
    note_padding(table)
    if device.type == 'cuda':
        from latent_pose_reenactment_amd import hipops
        if not buf.is_pinned():
            buf = buf.pin_memory()
        image, mask, product = hipops.frames_prepare(buf.to(device, non_blocking=True), table, size)
    else:
        image, mask, product = prepare_host(buf, table, size)
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
