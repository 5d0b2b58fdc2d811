"""A VoxCeleb2-layout tree with landmark files, written with PIL and numpy from a seeded generator, for the tests of the keypoint loaders
(``dataloaders/voxceleb2.py``, ``dataloaders/voxceleb2_FSTH_crop.py``) on the CPU and on the GPU, and what the loaders must make of it, worked out
here independently of them: the frames a deterministic loader samples, the boxes, the normalised keypoints in float64."""
import os
import random
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):          # (plugins resolve as dataloaders.<name>)
    if _p not in sys.path:
        sys.path.insert(0, _p)

SIZE, K = 24, 2
NAMES = tuple(f'{i:05d}' for i in range(4))
# video -> (H, W, columns of its landmark files)
VIDEOS = {'id00/vidA': (20, 20, 2), 'id00/vidB': (32, 32, 3), 'id01/vidA': (32, 32, 2), 'id01/vidB': (20, 20, 3), 'id02/vidA': (24, 32, 2)}
SQUARE = tuple(v for v, (h, w, _) in VIDEOS.items() if h == w)
PLUGINS = ('voxceleb2', 'voxceleb2_FSTH_crop')


def build_tree(root):
    """-> the data root: Img/<video>/<frame>.jpg, landmarks/<video>/<frame>.npy, square.csv (the square videos), all.csv, and a second root
    ``short`` whose only video has a 60-row landmark file"""
    import pandas
    from PIL import Image
    rng = np.random.default_rng(23)
    root = Path(root)

    def write(base, video, h, w, cols, rows=68):
        (base / 'Img' / video).mkdir(parents=True)
        (base / 'landmarks' / video).mkdir(parents=True)
        for name in NAMES:
            smooth = np.add.outer(np.arange(h) * 5, np.arange(w) * 3)[:, :, None] + rng.integers(0, 80, (h, w, 3))
            Image.fromarray(np.clip(smooth, 0, 255).astype(np.uint8)).save(base / 'Img' / video / (name + '.jpg'), quality=92)
            kp = np.concatenate([rng.uniform(0.1 * w, 0.9 * w, (rows, 1)), rng.uniform(0.25 * h, 0.95 * h, (rows, 1)), rng.normal(size=(rows, 1))], 1)
            np.save(base / 'landmarks' / video / (name + '.npy'), kp[:, :cols])
    for video, (h, w, cols) in VIDEOS.items():
        write(root, video, h, w, cols)
    write(root / 'short', 'id09/vidA', 20, 20, 2, rows=60)
    pandas.DataFrame({'path': ['id09/vidA']}).to_csv(root / 'short' / 'short.csv', index=False)
    pandas.DataFrame({'path': list(SQUARE)}).to_csv(root / 'square.csv', index=False)
    pandas.DataFrame({'path': list(VIDEOS)}).to_csv(root / 'all.csv', index=False)
    return root


def make_args(root, split='square.csv', **over):
    root = Path(root)
    args = SimpleNamespace(data_root=root, img_dir=Path('Img'), kp_dir=Path('landmarks'), draw_oval=True, stickman_thickness=2,
                           n_frames_for_encoder=K, image_size=SIZE, train_split_path=root / split, val_split_path=root / split, finetune=False,
                           inference=False, checkpoint_path='', num_labels=98000, world_size=1, rank=0, batch_size=2, num_gpus=1, num_workers=0,
                           random_seed=123, device='cpu', use_pixelwise_augs=False, use_affine_scale=False, use_affine_shift=False,
                           use_extra_pixelwise_augs=False)
    for k, v in over.items():
        setattr(args, k, v)
    return args


def loader_for(plugin, args, part='val'):
    from latent_pose_reenactment_amd.dataloaders.dataloader import Dataloader
    return Dataloader(plugin).get_dataloader(args, part=part, phase=part)


def sampled(root, video, k=K + 1):
    """the frames a deterministic loader takes from a video: Random(666)'s sample of the sorted folder"""
    files = sorted((Path(root) / 'Img' / video).iterdir())
    return [f.stem for f in random.Random(666).sample(files, k=k)]


def box(plugin, h, w):
    """-> (t, l, n), from the issue's text"""
    if plugin == 'voxceleb2':
        assert h == w
        return 0, 0, h
    cut_t = min(h - 1, round(0.2 * h))
    n = max(cut_t + 1, round(h)) - cut_t
    return cut_t, (w - n) // 2, n


def reference_cut_width(w):
    """cut_r - cut_l of the reference's SmallCropSampleLoader, its floats as it forms them"""
    cut_t, cut_b = 0.2, 1.0
    cut_l = (1.0 - (cut_b - cut_t)) / 2
    cut_r = 1.0 - cut_l
    cut_l = min(w - 1, round(cut_l * w))
    cut_r = max(cut_l + 1, round(cut_r * w))
    return cut_r - cut_l


def decode(root, video, name):
    from PIL import Image
    with Image.open(Path(root) / 'Img' / video / (name + '.jpg')) as im:
        return np.array(im.convert('RGB'), dtype=np.uint8)


def keypoints64(root, plugin, video, name):
    """the normalised keypoints in float64, [136]"""
    h, w, _ = VIDEOS[video]
    t, l, n = box(plugin, h, w)
    kp = np.load(Path(root) / 'landmarks' / video / (name + '.npy'))[:, :2].astype(np.float64)
    if plugin == 'voxceleb2':
        return (kp / w).reshape(-1)
    return ((kp - np.array([[l, t]], dtype=np.float64)) / n).reshape(-1)


def host_image(root, plugin, video, name, size=SIZE):
    """``frames.prepare_host`` on the frame's own bytes with the stated box -> fp32 [3, S, S]"""
    from latent_pose_reenactment_amd import frames
    rgb = decode(root, video, name)
    h, w = rgb.shape[:2]
    t, l, n = box(plugin, h, w)
    row = frames.make_row([0, h, w, 3 * w, 3, t, l, t + n, l + n, frames.mode_for(n, size)], image_slot=0)
    return frames.prepare_host(torch.from_numpy(rgb).reshape(-1), torch.tensor([row], dtype=torch.int64), size)[0][0]
