"""Training visuals (reference: utils/visualize.py ``make_visual`` + the TensorBoard branch of runners/holycow.py:324-342): the panels of a batch --
identity source, pose target / pose input, generator output, segmentations, then the same for other drivers -- side by side with captions, one row
per sample, written as a PNG.  The panels are VIEWS of the batch tensors; the sheet is composed and quantised on the device in one launch
(hipops.visual_sheet: csrc/visual_sheet.hip holds the value rule) and crosses to the host once, as uint8.

Captions are rasterised on the host from the 5 x 7 bitmap font below (no PIL font: its rendering may differ between versions; cv2 is absent), once
per caption tuple, and uploaded once."""
import torch

from latent_pose_reenactment_amd import hipops as ops

DRIVERS = (('', 'same video'), ('_other_video', 'other video'), ('_other_person', 'other person'))


def _frame0(t, n_samples):
    """[:n_samples] of a batch tensor, frame 0 of a 5-D one: a view"""
    t = t[:n_samples]
    return t[:, 0] if t.dim() > 4 else t


def make_visual(data, n_samples=2):
    """the panels of ``data`` (the dict a visual forward returned) as a list of (caption, view [n, C, H, W]) in the reference's order and with its
    captions.  Nothing is copied: ``fake_segm`` stays one channel (the sheet kernel writes it to all three), ``real_segm`` stays its expanded view."""
    out = []
    if 'enc_rgbs' in data:
        out.append(('Identity src', _frame0(data['enc_rgbs'], n_samples)))

    def driver(suffix, note):
        for key, title in (('dec_stickmen', 'Pose src'), ('pose_input_rgbs_cropped_voxceleb1', 'Pose src'), ('target_rgbs', 'Pose target')):
            if key + suffix in data:          # (the first of the three that the batch carries)
                out.append((f'{title} ({note})', _frame0(data[key + suffix], n_samples)))
                break
        if 'pose_input_rgbs' + suffix in data:
            out.append((f'Pose input ({note})', _frame0(data['pose_input_rgbs' + suffix], n_samples)))
        if 'fake_rgbs' + suffix in data:
            out.append(('Generator output', _frame0(data['fake_rgbs' + suffix], n_samples)))

    driver(*DRIVERS[0])
    if 'real_segm' in data:
        out.append(('True segmentation', _frame0(data['real_segm'], n_samples)))
    if 'fake_segm' in data:
        out.append(('Predicted segmentation', _frame0(data['fake_segm'], n_samples)))
    driver(*DRIVERS[1])
    driver(*DRIVERS[2])
    return out


# ---- captions ---------------------------------------------------------------------------------------------------------------------------------------------
GLYPH_W, GLYPH_H = 5, 7          # a character cell is GLYPH_W + 1 columns wide
CAPTION_HEIGHT = 11              # default strip: 2 rows above the glyphs, 2 below
BOX = '##### #...# #...# #...# #...# #...# #####'          # a character the font does not have
FONT = {
    ' ': '..... ..... ..... ..... ..... ..... .....',
    '(': '...#. ..#.. .#... .#... .#... ..#.. ...#.',
    ')': '.#... ..#.. ...#. ...#. ...#. ..#.. .#...',
    '/': '....# ....# ...#. ..#.. .#... #.... #....',
    '-': '..... ..... ..... ##### ..... ..... .....',
    '_': '..... ..... ..... ..... ..... ..... #####',
    '.': '..... ..... ..... ..... ..... .##.. .##..',
    ',': '..... ..... ..... ..... .##.. ..#.. .#...',
    ':': '..... .##.. .##.. ..... .##.. .##.. .....',
    '0': '.###. #...# #..## #.#.# ##..# #...# .###.',
    '1': '..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.',
    '2': '.###. #...# ....# ...#. ..#.. .#... #####',
    '3': '##### ...#. ..#.. ...#. ....# #...# .###.',
    '4': '...#. ..##. .#.#. #..#. ##### ...#. ...#.',
    '5': '##### #.... ####. ....# ....# #...# .###.',
    '6': '..##. .#... #.... ####. #...# #...# .###.',
    '7': '##### ....# ...#. ..#.. .#... .#... .#...',
    '8': '.###. #...# #...# .###. #...# #...# .###.',
    '9': '.###. #...# #...# .#### ....# ...#. .##..',
    'A': '.###. #...# #...# ##### #...# #...# #...#',
    'B': '####. #...# #...# ####. #...# #...# ####.',
    'C': '.###. #...# #.... #.... #.... #...# .###.',
    'D': '###.. #..#. #...# #...# #...# #..#. ###..',
    'E': '##### #.... #.... ####. #.... #.... #####',
    'F': '##### #.... #.... ####. #.... #.... #....',
    'G': '.###. #...# #.... #.### #...# #...# .####',
    'H': '#...# #...# #...# ##### #...# #...# #...#',
    'I': '.###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.',
    'J': '..### ...#. ...#. ...#. ...#. #..#. .##..',
    'K': '#...# #..#. #.#.. ##... #.#.. #..#. #...#',
    'L': '#.... #.... #.... #.... #.... #.... #####',
    'M': '#...# ##.## #.#.# #.#.# #...# #...# #...#',
    'N': '#...# #...# ##..# #.#.# #..## #...# #...#',
    'O': '.###. #...# #...# #...# #...# #...# .###.',
    'P': '####. #...# #...# ####. #.... #.... #....',
    'Q': '.###. #...# #...# #...# #.#.# #..#. .##.#',
    'R': '####. #...# #...# ####. #.#.. #..#. #...#',
    'S': '.#### #.... #.... .###. ....# ....# ####.',
    'T': '##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..',
    'U': '#...# #...# #...# #...# #...# #...# .###.',
    'V': '#...# #...# #...# #...# #...# .#.#. ..#..',
    'W': '#...# #...# #...# #.#.# #.#.# #.#.# .#.#.',
    'X': '#...# #...# .#.#. ..#.. .#.#. #...# #...#',
    'Y': '#...# #...# #...# .#.#. ..#.. ..#.. ..#..',
    'Z': '##### ....# ...#. ..#.. .#... #.... #####',
    'a': '..... ..... .###. ....# .#### #...# .####',
    'b': '#.... #.... #.##. ##..# #...# #...# ####.',
    'c': '..... ..... .###. #.... #.... #...# .###.',
    'd': '....# ....# .##.# #..## #...# #...# .####',
    'e': '..... ..... .###. #...# ##### #.... .###.',
    'f': '..##. .#..# .#... ###.. .#... .#... .#...',
    'g': '..... .#### #...# #...# .#### ....# .###.',
    'h': '#.... #.... #.##. ##..# #...# #...# #...#',
    'i': '..#.. ..... .##.. ..#.. ..#.. ..#.. .###.',
    'j': '...#. ..... ..##. ...#. ...#. #..#. .##..',
    'k': '#.... #.... #..#. #.#.. ##... #.#.. #..#.',
    'l': '.##.. ..#.. ..#.. ..#.. ..#.. ..#.. .###.',
    'm': '..... ..... ##.#. #.#.# #.#.# #...# #...#',
    'n': '..... ..... #.##. ##..# #...# #...# #...#',
    'o': '..... ..... .###. #...# #...# #...# .###.',
    'p': '..... ####. #...# #...# ####. #.... #....',
    'q': '..... .#### #...# #...# .#### ....# ....#',
    'r': '..... ..... #.##. ##..# #.... #.... #....',
    's': '..... ..... .###. #.... .###. ....# ####.',
    't': '.#... .#... ###.. .#... .#... .#..# ..##.',
    'u': '..... ..... #...# #...# #...# #..## .##.#',
    'v': '..... ..... #...# #...# #...# .#.#. ..#..',
    'w': '..... ..... #...# #...# #.#.# #.#.# .#.#.',
    'x': '..... ..... #...# .#.#. ..#.. .#.#. #...#',
    'y': '..... #...# #...# #...# .#### ....# .###.',
    'z': '..... ..... ##### ...#. ..#.. .#... #####',
}


def glyph(ch):
    """uint8 [7, 5], 1 where the character has ink; a character outside ``FONT`` draws a box"""
    rows = FONT.get(ch, BOX).split()
    return torch.tensor([[1 if c == '#' else 0 for c in row] for row in rows], dtype=torch.uint8)


def caption_strip(captions, width, height=CAPTION_HEIGHT):
    """uint8 [height, len(captions) * width] on the host, black (0) on white (255): caption p starts one column inside panel p, two rows from the top;
    the glyphs are enlarged by the whole factor max(1, (height - 4) // 7); what does not fit the panel's width or the strip's height is cut"""
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise ValueError(f'caption_strip: width and height must be >= 1, got {width} x {height}')
    scale = max(1, (height - 4) // GLYPH_H)
    strip = torch.full((height, len(captions) * width), 255, dtype=torch.uint8)
    for p, text in enumerate(captions):
        cell = torch.full((height, width), 255, dtype=torch.uint8)          # the panel's own part: nothing spills into the neighbour
        for i, ch in enumerate(str(text)):
            x0 = 1 + i * (GLYPH_W + 1) * scale
            if x0 >= width:
                break
            ink = glyph(ch).repeat_interleave(scale, 0).repeat_interleave(scale, 1)
            gh, gw = min(ink.shape[0], height - 2), min(ink.shape[1], width - x0)
            if gh > 0:
                cell[2:2 + gh, x0:x0 + gw][ink[:gh, :gw] == 1] = 0
        strip[:, p * width:(p + 1) * width] = cell
    return strip


_STRIPS = {}


def _strip_on(device, captions, width, height):
    """the strip of a caption tuple on ``device``: rasterised and uploaded once"""
    key = (tuple(captions), int(width), int(height), str(device))
    if key not in _STRIPS:
        _STRIPS[key] = caption_strip(captions, width, height).to(device)
    return _STRIPS[key]


def caption_height(width):
    """strip height ``sheet`` uses for panels ``width`` wide: the longest reference caption (26 characters) fits a 256-pixel panel at scale 1"""
    return CAPTION_HEIGHT if width < 320 else 2 * GLYPH_H + 4


def sheet(data, n_samples=2, captions=True):
    """the captioned panel sheet of ``data`` as a uint8 tensor [Hc + n H, P W, 3] on the panels' device (one launch there)"""
    items = make_visual(data, n_samples)
    if not items:
        raise ValueError('visualize.sheet: the batch carries none of the tensors make_visual shows')
    panels = [t for _, t in items]
    width = panels[0].shape[-1]
    strip = _strip_on(panels[0].device, [c for c, _ in items], width, caption_height(width)) if captions else None
    return ops.visual_sheet(panels, caption=strip)


def save_png(path, sheet_u8, encoder='pil'):
    """one device-to-host copy of the uint8 HWC sheet, then PIL writes the PNG (lossless: the file decodes to the same bytes).  ``encoder='gpu'``:
    the sheet is encoded where it is (``hipops.png_encode``, csrc/png.hip) and only the file's bytes are copied; it decodes to the same bytes too"""
    import os
    from PIL import Image
    if not (isinstance(sheet_u8, torch.Tensor) and sheet_u8.dtype == torch.uint8 and sheet_u8.dim() == 3 and sheet_u8.shape[2] == 3):
        raise ValueError('save_png: expected a uint8 tensor [H, W, 3]')
    if encoder not in ('pil', 'gpu'):
        raise ValueError(f"save_png: encoder must be 'pil' or 'gpu', got {encoder!r}")
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    if encoder == 'gpu':
        data, _ = ops.png_encode(sheet_u8[None])
        with open(str(path), 'wb') as f:
            f.write(data.cpu().numpy().tobytes())
        return path
    Image.fromarray(sheet_u8.cpu().numpy()).save(str(path))
    return path
