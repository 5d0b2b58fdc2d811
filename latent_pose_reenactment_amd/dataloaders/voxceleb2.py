"""The reference's keypoint dataset plugin of the FSTH family (dataloaders/voxceleb2.py, dataloaders/common/voxceleb.py:119-299): image folders
with one landmark file per frame,
  <data_root>/<img_dir>/<identity>/<video>/<frame>.jpg         <data_root>/<kp_dir>/<identity>/<video>/<frame>.npy  (>= 68 rows of x, y[, z] in pixels)
with the reference's flags and its ways of naming the identities (``get_part_data`` of ``voxceleb2_segmentation_nolandmarks``).  The work is split
as in that plugin: the dataset (in ``--num_workers`` worker processes, which never touch the GPU) DECODES frames with PIL and returns them as raw
uint8 bytes with the rows of the table that describe them, and the frame's keypoints normalised to the unit square of its box (fp32, 136 per
frame); the collate function packs a batch; the loader returned by ``get_dataloader`` makes the batch where it is consumed (``prepare``): one pinned
copy of the bytes, one lp_frames_prepare launch, one pinned copy of the keypoints, one lp_stickman_render_hard launch for all B (K + 1) stickmen
(``hipops.stickman_render_hard``: the reference's cv2.polylines drawing restated exactly in integers, csrc/stickman_hard.hip).  It yields the
reference's contract, fp32 on the device:
  data_dict:   enc_rgbs B x K x 3 x S x S, enc_stickmen B x K x 3 x S x S, target_rgbs = pose_input_rgbs B x 1 x 3 x S x S (one image),
               dec_stickmen B x 1 x 3 x S x S, dec_keypoints B x 1 x 136
  target_dict: label int64 B
and with ``--finetune`` the one image of a sample and its stickman under both the ``enc_`` and the ``dec_`` names (K = 1), label 0.  ``--inference``
changes nothing but the augmentation flags, which it switches off; one that is on is refused ("Keypoints augmentation is NYI", as in the reference).
This plugin takes the whole frame, which must be square (the reference squashes another frame anisotropically; the table of lp_frames_prepare holds
square boxes only); ``voxceleb2_FSTH_crop`` cuts the reference's crop.  Not offered here: ``--blur_padded_bands``, ``--decode_jpeg_on_gpu``."""
import logging
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader

from latent_pose_reenactment_amd import augmentation, frames
from latent_pose_reenactment_amd.dataloaders import voxceleb2_segmentation_nolandmarks as _folders
from latent_pose_reenactment_amd.dataloaders.synthetic_voxceleb2_stickmen import REFERENCE_PARTS, REFERENCE_PARTS_NO_OVAL

logger = logging.getLogger('dataloader')

NUM_KEYPOINTS = 68
AUGMENTATION_FLAGS = ('use_pixelwise_augs', 'use_affine_scale', 'use_affine_shift', 'use_extra_pixelwise_augs')


def whole_frame_box(h, w, file):
    """-> (t, l, n): the whole frame (voxceleb.py:275-286 resizes it to imsize x imsize); ValueError naming the file for a frame that is not square"""
    if h != w:
        raise ValueError(f"{file}: the frame is {h} x {w}; dataloader 'voxceleb2' takes the whole frame, which must be square "
                         "(`--dataloader voxceleb2_FSTH_crop` cuts a square crop from any frame)")
    return 0, 0, h


class SampleLoader(_folders.SampleLoader):
    """decoding only: ``load_rgb`` / ``list_ids`` of the image-folder plugin and the landmark files (voxceleb.SampleLoader.load_keypoints)"""
    box = staticmethod(whole_frame_box)

    def __init__(self, data_root, img_dir, kp_dir, deterministic):
        self.data_root, self.img_dir, self.kp_dir = Path(data_root), Path(img_dir), Path(kp_dir)
        self.deterministic = deterministic
        self.decode_jpeg_on_gpu = False

    def load_keypoints(self, path, i):
        """-> float64 [68, 2] (x, y) in pixels of the decoded frame; ValueError naming the file if it holds fewer than 68 rows"""
        kp_path = self.data_root / self.kp_dir / path / (i + '.npy')
        keypoints = np.load(kp_path)
        if keypoints.ndim != 2 or keypoints.shape[0] < NUM_KEYPOINTS or keypoints.shape[1] < 2:
            raise ValueError(f'{kp_path}: keypoints of shape {keypoints.shape}; at least {NUM_KEYPOINTS} rows of (x, y) are required')
        return keypoints[:NUM_KEYPOINTS, :2].astype(np.float64)

    def load_frame(self, path, i, size):
        """-> (H x W x 3 uint8, image columns of its table row but for the offset, fp32 [136] keypoints in the unit square of the box)"""
        rgb = self.load_rgb(path, i)
        h, w = rgb.shape[:2]
        t, l, n = self.box(h, w, self.data_root / self.img_dir / path / i)
        keypoints = (self.load_keypoints(path, i) - np.array([[l, t]], dtype=np.float64)) / float(n)
        columns = [h, w, w * 3, 3, t, l, t + n, l + n, frames.mode_for(n, size)]          # the view is the whole decoded frame
        return rgb, columns, keypoints.astype(np.float32).reshape(-1)


class Dataset(torch.utils.data.Dataset):
    SAMPLE_LOADER = SampleLoader

    @staticmethod
    def get_args(parser):
        parser.add('--data_root', default='', type=Path)
        parser.add('--img_dir', default='Img', type=Path)
        parser.add('--kp_dir', default='landmarks', type=Path)
        parser.add('--draw_oval', default=True, action="store_bool")
        parser.add('--n_frames_for_encoder', default=8, type=int)
        parser.add('--num_labels', type=int, default=98000, help='identities in the training split; set from the split when training from scratch')
        parser.add('--stickman_thickness', type=int, default=2, help='line thickness of the stickmen in pixels, 1 .. 8 (the reference draws 2)')
        return augmentation.get_args(parser)

    @classmethod
    def get_dataset(cls, args, part):
        return cls(args, part)

    @classmethod
    def get_dataloader(cls, args, part):
        return get_dataloader(cls, args, part)

    def __init__(self, args, part):
        if not getattr(args, 'inference', False):          # (under --inference the reference switches the flags off: augmentation.py:107-109)
            for flag in AUGMENTATION_FLAGS:
                if getattr(args, flag, False):
                    raise NotImplementedError(f'Keypoints augmentation is NYI (`--{flag}` is on)')
        self.thickness = int(getattr(args, 'stickman_thickness', 2))
        if not 1 <= self.thickness <= 8:
            raise ValueError(f'`--stickman_thickness` must be in 1 .. 8, got {self.thickness}')
        self.parts = REFERENCE_PARTS if getattr(args, 'draw_oval', True) else REFERENCE_PARTS_NO_OVAL
        self.dirlist = _folders.get_part_data(args, part)
        self.loader = self.SAMPLE_LOADER(args.data_root, args.img_dir, args.kp_dir, deterministic=part != 'train')
        self.frames = args.n_frames_for_encoder
        self.size = args.image_size
        self.finetuning = 'file' in self.dirlist

    def __len__(self):
        return self.dirlist.shape[0]

    def __getitem__(self, index):
        """-> {'bytes': the decoded frames of this sample, packed; 'rows': their table rows, offsets relative to 'bytes' and slots relative to the
        sample (image slot k < K: encoder frame k, K: the target frame); 'keypoints': fp32 [frames, 136] in the order of the rows; 'label'; 'index'}"""
        row = self.dirlist.iloc[index]
        path = row['path']
        if self.finetuning:                  # `dirlist` enumerates the images of the one identity (voxceleb2.py:43-65)
            ids, label = [row['file']], 0
        else:                                # "one sample" is one video: K encoder frames and the target frame (:66-97)
            ids, label = self.loader.list_ids(path, self.frames + 1), int(self.dirlist.index[index])
        chunks, rows, keypoints, offset = [], [], [], 0
        for k, i in enumerate(ids):
            rgb, columns, kp = self.loader.load_frame(path, i, self.size)
            rows.append(frames.make_row([offset] + columns, image_slot=k))
            chunks.append(torch.from_numpy(rgb).reshape(-1))
            keypoints.append(torch.from_numpy(kp))
            offset += rgb.size
        return {'bytes': torch.cat(chunks), 'rows': torch.tensor(rows, dtype=torch.int64), 'keypoints': torch.stack(keypoints), 'label': label,
                'index': int(index)}


class Collate(_folders.Collate):
    """the image-folder plugin's collate function (bytes packed, offsets rebased, slots made global) + the keypoints in the order of the image
    slots: fp32 [B K + B, 136], the encoder frames of all samples first, then the target frames"""

    def __init__(self, num_frames, finetuning):
        super().__init__(num_frames, finetuning, inference=False)

    def __call__(self, samples):
        raw = super().__call__(samples)
        k = self.frames
        kp = [sample['keypoints'] for sample in samples]
        raw['keypoints'] = torch.cat([p[:k] for p in kp] + [p[k:] for p in kp])
        return raw


def prepare(raw_batch, size, device, thickness=2, parts=REFERENCE_PARTS):
    """a raw batch of ``Collate`` -> (data_dict, target_dict) of the module docstring, fp32 on ``device``.  On a GPU: one pinned host-to-device copy
    of the packed bytes, one lp_frames_prepare launch, one pinned copy of the keypoint block and one lp_stickman_render_hard launch into ONE buffer,
    of which ``enc_stickmen`` and ``dec_stickmen`` are views; all on the current stream, nothing waited for.  CPU tensors: ``frames.prepare_host`` and
    ``hipops.stickman_render_hard_host``, the same definitions."""
    from latent_pose_reenactment_amd import hipops
    buf, table, label, keypoints = raw_batch['buf'], raw_batch['table'], raw_batch['label'], raw_batch['keypoints']
    device = torch.device(device)
    if device.type == 'cuda':
        if not buf.is_pinned():
            buf = buf.pin_memory()
        if not keypoints.is_pinned():
            keypoints = keypoints.pin_memory()
        image = hipops.frames_prepare(buf.to(device, non_blocking=True), table, size)[0]
        keypoints = keypoints.to(device, non_blocking=True)
        stickmen = hipops.stickman_render_hard(keypoints, size, thickness, parts=parts)
    else:
        image = frames.prepare_host(buf, table, size)[0]
        stickmen = hipops.stickman_render_hard_host(keypoints, size, thickness, parts=parts)
    b, k = label.shape[0], int(raw_batch['frames'])
    data_dict = {}
    if k == 0:                  # fine-tuning: the one image and its stickman under both names (voxceleb2.py:57-63)
        data_dict['enc_rgbs'] = data_dict['target_rgbs'] = data_dict['pose_input_rgbs'] = image.view(b, 1, 3, size, size)
        data_dict['enc_stickmen'] = data_dict['dec_stickmen'] = stickmen.view(b, 1, 3, size, size)
        data_dict['dec_keypoints'] = keypoints.view(b, 1, 2 * NUM_KEYPOINTS)
    else:
        data_dict['enc_rgbs'] = image[:b * k].view(b, k, 3, size, size)
        data_dict['enc_stickmen'] = stickmen[:b * k].view(b, k, 3, size, size)
        data_dict['target_rgbs'] = data_dict['pose_input_rgbs'] = image[b * k:].view(b, 1, 3, size, size)
        data_dict['dec_stickmen'] = stickmen[b * k:].view(b, 1, 3, size, size)
        data_dict['dec_keypoints'] = keypoints[b * k:].view(b, 1, 2 * NUM_KEYPOINTS)
    return data_dict, {'label': label.to(device, non_blocking=True)}


class KeypointLoader:
    """iterable of (data_dict, target_dict) over a torch DataLoader of raw batches (``prepare`` per batch, on the current stream)"""

    def __init__(self, loader, dataset, args):
        self.loader, self.dataset = loader, loader.dataset
        self.size, self.thickness, self.parts = args.image_size, dataset.thickness, dataset.parts
        device = str(getattr(args, 'device', 'cuda'))
        self.device = device if device.startswith('cuda') and torch.cuda.is_available() else 'cpu'
        self.batch_size = loader.batch_size

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for raw in self.loader:
            yield prepare(raw, self.size, self.device, self.thickness, self.parts)


def get_dataloader(cls, args, part):
    """the hook ``Dataloader.get_dataloader`` honours: rank-strided, shuffled for 'train', as the image-folder plugin builds its loader"""
    dataset = cls(args, part)
    assert len(dataset) % args.world_size == 0, "the dataset was expected to be equally divisible by `args.world_size`"
    subset = torch.utils.data.Subset(dataset, range(args.rank, len(dataset), args.world_size))
    logger.info(f"This process will receive a dataset with {len(subset)} samples")
    if len(subset) < args.batch_size:
        logger.warning(f"Dataset length is smaller than batch size ({len(subset)} < {args.batch_size}), reducing the latter")
        args.batch_size = len(subset)
    workers = max(0, min(int(getattr(args, 'num_workers', 0)), _folders.MAX_WORKERS))
    loader = DataLoader(subset, batch_size=max(1, args.batch_size // args.num_gpus), num_workers=workers, pin_memory=torch.cuda.is_available(),
                        drop_last=(part == 'train'), shuffle=(part == 'train'), collate_fn=Collate(dataset.frames, dataset.finetuning))
    return KeypointLoader(loader, dataset, args)
