"""The reference's VoxCeleb2 dataset plugin (dataloaders/voxceleb2_segmentation_nolandmarks.py, dataloaders/common/voxceleb.py:14-173): image folders
  <data_root>/<img_dir>/<identity>/<video>/<frame>.jpg         <data_root>/<segm_dir>/<identity>/<video>/<frame>.png  (or .png.npy)
with the reference's flags and its ways of naming the identities (one identity folder, a CSV, a folder of identities, the fine-tuning image list).
The work is split where the data changes hands: the dataset (in ``--num_workers`` worker processes, which never touch the GPU) DECODES frames with
PIL and returns them as raw uint8 bytes with the rows of the table that describe them -- never a resized image; the collate function packs a batch's
bytes and rebases the offsets; the loader returned by ``get_dataloader`` copies the packed bytes to the device once and makes the batch there
(``frames.prepare``: crop to the scaled bounding box, resize, / 255, image x segmentation in one lp_frames_prepare launch).  What it yields is
``synthetic_voxceleb2``'s contract:
  data_dict:   enc_rgbs B x K x 3 x S x S, pose_input_rgbs B x 1 x 3 x S x S, target_rgbs B x 1 x 3 x S x S (+ aug_params B x 32 / aug_params_extra B x 16 when augmenting)
  target_dict: real_segm B x 1 x 3 x S x S, label int64 B
and under ``--inference`` only what the reference loads then (fine-tuning form: enc_rgbs = pose_input_rgbs and the label; otherwise the encoder
frames and the label).  Keypoints and stickmen (the FSTH family) are not read.  ``--blur_padded_bands`` (off by default) blurs the padded bands
of a box that leaves its frame and fades them to the median colour, as the reference's ``crop_with_padding`` does (csrc/frames_pad.hip); without
it they carry the border rule's pixels as they are (csrc/frames.hip).  ``--decode_jpeg_on_gpu`` (off by default) moves the JPEG decode to the device
as well: the workers read the file bytes and parse the headers only (``utils.jpeg_parse``), the compressed scan crosses PCIe and is decoded into the
same packed buffer (csrc/jpeg_decode.hip); a file outside the supported set, or a .png frame, is decoded with PIL in the worker as before; the
masks stay with PIL."""
import logging
import random
from itertools import chain
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader

from latent_pose_reenactment_amd import augmentation, frames

logger = logging.getLogger('dataloader')

SCALE = 1.8
MAX_WORKERS = 8


def get_part_data(args, part):
    """the identities of a split as a pandas dataframe with the column 'path' (or, when fine-tuning, the images of the one identity: 'path', 'file')
    -- dataloaders/common/voxceleb.py:14-117"""
    import pandas
    assert part in ('train', 'val'), "`.get_part_data()`'s `part` argument must be 'train' or 'val'"
    split_path = Path(args.train_split_path if part == 'train' else args.val_split_path)
    data_root, img_dir = Path(args.data_root), Path(args.img_dir)
    hint = "pass `--dataloader synthetic_voxceleb2` for batches with the same data_dict/target_dict contract without a dataset"
    if str(args.data_root) == '' or not data_root.is_dir():
        raise FileNotFoundError(f"dataloader 'voxceleb2_segmentation_nolandmarks' reads VoxCeleb2-layout image folders, and `--data_root` "
                                f"'{args.data_root}' is not a directory; {hint}")
    identity_list = None
    if (data_root / img_dir / split_path).is_dir():
        logger.info(f"'{data_root / img_dir / split_path}' is a directory; the only {part} identity will be '{split_path}'")
        identity_list = pandas.DataFrame({'path': [str(split_path)]})
    elif split_path.is_file():
        logger.info(f"'{split_path}' is a file; reading the {part} identity list from it")
        identity_list = pandas.read_csv(split_path)
    elif (data_root / img_dir).is_dir():
        identity_list = pandas.DataFrame({'path': sorted(str(x.relative_to(data_root / img_dir)) for x in (data_root / img_dir).iterdir() if x.is_dir())})
        logger.info(f"'{data_root / img_dir}' is a directory; found {len(identity_list)} {part} identities in it")
    if identity_list is None:
        raise FileNotFoundError(f"Could not determine input data source, check `args.data_root`, `args.img_dir` and `args.{part}_split_path` "
                                f"(none of '{data_root / img_dir / split_path}', '{split_path}', '{data_root / img_dir}' exists); {hint}")

    if args.finetune:
        if len(identity_list) > 1:
            raise NotImplementedError("Sorry, fine-tuning to multiple identities is not yet available")
        image_list = sorted(chain(*((data_root / img_dir / x).iterdir() for x in identity_list['path'])))
        logger.info(f"This dataset has {len(image_list)} images")
        args.num_labels = 1
        logger.info("Setting `args.num_labels` to 1 because we are fine-tuning or the model has been fine-tuned")
        return pandas.DataFrame({'path': [str(path.parent.relative_to(data_root / img_dir)) for path in image_list],
                                 'file': [path.stem for path in image_list]})
    if getattr(args, 'checkpoint_path', '') != "":
        logger.info(f"Truncating the identity list as in the checkpoint, to {args.num_labels} samples")
        identity_list = identity_list.iloc[:args.num_labels]
    elif part == 'train':
        args.num_labels = len(identity_list)
        logger.info(f"Setting `args.num_labels` to {args.num_labels}")
    num_samples_to_add = (args.world_size - len(identity_list) % args.world_size) % args.world_size
    logger.info(f"Making dataset length divisible by world size: was {len(identity_list)}, became {len(identity_list) + num_samples_to_add}")
    return pandas.concat([identity_list, identity_list.iloc[:num_samples_to_add]])


class SampleLoader:
    """decoding only (voxceleb.SampleLoader.load_rgb / list_ids and this plugin's load_segm / bounding boxes in the reference)"""

    def __init__(self, data_root, img_dir, segm_dir, bboxes_dir, deterministic, decode_jpeg_on_gpu=False):
        self.data_root, self.img_dir, self.segm_dir = Path(data_root), Path(img_dir), Path(segm_dir)
        self.deterministic = deterministic
        self.decode_jpeg_on_gpu = decode_jpeg_on_gpu
        try:
            self.bboxes = np.load(bboxes_dir, allow_pickle=True).item()
        except (FileNotFoundError, IsADirectoryError):
            self.bboxes = {}
            logger.warning("Could not find the '.npy' file with bboxes, will assume the images are already cropped")

    def list_ids(self, path, k):
        """k frame names of a video: a random sample, Random(666)'s for a deterministic loader (voxceleb.py:156-173; the folder is read in sorted
        order, so that the same seed names the same frames on every file system)"""
        full_path = self.data_root / self.img_dir / path
        id_list = sorted(full_path.iterdir())
        generator = random.Random(666) if self.deterministic else random
        while k > len(id_list):
            id_list += sorted(full_path.iterdir())
        return [i.stem for i in generator.sample(id_list, k=k)]

    def box(self, path, i):
        """(t, l, b, r) in the space where the frame is the unit square: the detector's box made square and scaled by 1.8, or the whole frame"""
        try:
            identity, sequence = path.split('/')
            l, t, r, b = (np.asarray(self.bboxes[identity][sequence][int(i)], dtype=np.float64) / 256.0).tolist()
        except Exception:                   # no such box: this image is taken to be cropped already (:113-115)
            return 0.0, 0.0, 1.0, 1.0
        return frames.scaled_square_box(l, t, r, b, SCALE)

    def load_rgb(self, path, i):
        """-> H x W x 3 uint8; with ``decode_jpeg_on_gpu`` a ``jpeg_parse.Descriptor`` for a .jpg file of the supported set (its pixels are made on
        the device) -- ValueError naming the file for a malformed one"""
        from PIL import Image
        img_path = self.data_root / self.img_dir / path / (i + '.jpg')
        if not img_path.exists():           # (lossless frames: what the tests write)
            img_path = img_path.with_suffix('.png')
        if self.decode_jpeg_on_gpu and img_path.suffix == '.jpg':
            from latent_pose_reenactment_amd.utils import jpeg_parse
            data = img_path.read_bytes()
            try:
                descriptor = jpeg_parse.parse(data)
            except ValueError as e:
                raise ValueError(f'{img_path}: {e}') from e
            if descriptor is not None:
                return descriptor, str(img_path)
        with Image.open(img_path) as im:
            return np.array(im.convert('RGB'), dtype=np.uint8)          # (a copy: PIL's buffer is read-only)

    def load_segm(self, path, i):
        """-> (H x W x C uint8, the channel to take): the second channel of the PNG (with PGN it denotes head + body; with Graphonomy all three are
        identical), the first of the .png.npy form"""
        from PIL import Image
        segm_path = self.data_root / self.segm_dir / path / (i + '.png')
        segm_path_np = self.data_root / self.segm_dir / path / (i + '.png.npy')
        if segm_path.exists():
            with Image.open(segm_path) as im:
                segm = np.array(im if im.mode in ('L', 'RGB') else im.convert('RGB'), dtype=np.uint8)
            channel = 1
        elif segm_path_np.exists():
            segm, channel = np.load(str(segm_path_np)).astype(np.uint8), 0
        else:
            raise FileNotFoundError(f'Sample {segm_path} not found')
        if segm.ndim == 2:
            segm, channel = segm[:, :, None], 0
        return np.ascontiguousarray(segm), channel


class Dataset(torch.utils.data.Dataset):
    @staticmethod
    def get_args(parser):
        parser.add('--data_root', default='', type=Path)
        parser.add('--img_dir', default='Img', type=Path)
        parser.add('--kp_dir', default='landmarks', type=Path)
        parser.add('--segm_dir', default='segm', type=Path)
        parser.add('--bboxes_dir', default="/non/existent/VoxCeleb2.1_bounding-boxes-SingleBBox.npy", type=Path)
        parser.add('--draw_oval', default=True, action="store_bool")
        parser.add('--n_frames_for_encoder', default=8, type=int)
        parser.add('--num_labels', type=int, default=98000, help='identities in the training split; set from the split when training from scratch')
        parser.add('--blur_padded_bands', default=False, action="store_bool",
                   help='blur the padded bands of a box that leaves its frame and fade them to the median colour (crop_with_padding)')
        parser.add('--decode_jpeg_on_gpu', default=False, action="store_bool",
                   help='decode the JPEG frames on the GPU: the workers parse the headers only and the compressed bytes cross PCIe (csrc/jpeg_decode.hip). '
                        'Measured SLOWER per batch than the PIL decode on files without restart markers (README): it frees the workers, not time')
        return augmentation.get_args(parser)

    @staticmethod
    def get_dataset(args, part):
        return Dataset(args, part)

    @staticmethod
    def get_dataloader(args, part):
        return get_dataloader(args, part)

    def __init__(self, args, part):
        self.dirlist = get_part_data(args, part)
        self.decode_jpeg_on_gpu = bool(getattr(args, 'decode_jpeg_on_gpu', False))
        self.loader = SampleLoader(args.data_root, args.img_dir, args.segm_dir, args.bboxes_dir, deterministic=part != 'train',
                                   decode_jpeg_on_gpu=self.decode_jpeg_on_gpu)
        self.inference = bool(getattr(args, 'inference', False))
        self.frames = args.n_frames_for_encoder
        self.size = args.image_size
        self.finetuning = 'file' in self.dirlist

    def __len__(self):
        return self.dirlist.shape[0]

    def __getitem__(self, index):
        """-> {'bytes': the decoded frames of this sample, packed; 'rows': their table rows, offsets relative to 'bytes' and slots relative to the
        sample (image slot k < K: encoder frame k, K: the pose image); 'label'; 'index'}.  With ``--decode_jpeg_on_gpu`` the offsets of the rows
        still describe the DECODED layout ('size' bytes), identical to the PIL route's, while 'bytes' holds only what was decoded here -- masks and
        fallback frames, 'regions' int64 [n, 3] = (offset in the decoded layout, offset in 'bytes', length) -- and 'jpeg' the packed descriptors
        of the other frames (``jpeg_parse.pack``, destination offsets in the decoded layout) with their 'files'"""
        row = self.dirlist.iloc[index]
        path = row['path']
        chunks, rows, offset = [], [], 0
        regions, descriptors, destinations, files, held = [], [], [], [], 0

        def add(array):
            nonlocal offset, held
            start = offset
            chunks.append(torch.from_numpy(array).reshape(-1))
            regions.append([start, held, array.size])
            offset += array.size
            held += array.size
            return start

        def image_columns(i):
            nonlocal offset
            rgb = self.loader.load_rgb(path, i)
            if isinstance(rgb, tuple):       # a descriptor: the pixels are decoded on the device into [offset, offset + H W 3)
                descriptor, name = rgb
                start, shape = offset, (descriptor.h, descriptor.w, 3)
                descriptors.append(descriptor)
                destinations.append(start)
                files.append(name)
                offset += descriptor.h * descriptor.w * 3
                return frames.frame_rows(start, shape, self.loader.box(path, i), self.size)
            return frames.frame_rows(add(rgb), rgb.shape, self.loader.box(path, i), self.size)

        def mask_columns(i):
            segm, channel = self.loader.load_segm(path, i)
            return frames.frame_rows(add(segm), segm.shape, self.loader.box(path, i), self.size, channel=channel)

        if self.finetuning:                  # `dirlist` enumerates the images of the one identity (:188-209)
            i = row['file']
            if self.inference:
                rows.append(frames.make_row(image_columns(i), image_slot=0))
            else:
                rows.append(frames.make_row(image_columns(i), mask_columns(i), image_slot=0, mask_slot=0, product_slot=0))
            label = 0
        else:                                # "one sample" is one video (:210-241)
            ids = self.loader.list_ids(path, self.frames + 1)
            for k, i in enumerate(ids[:-1]):
                rows.append(frames.make_row(image_columns(i), image_slot=k))
            if not self.inference:
                i = ids[-1]
                rows.append(frames.make_row(image_columns(i), mask_columns(i), image_slot=self.frames, mask_slot=0, product_slot=0))
            label = int(self.dirlist.index[index])
        sample = {'bytes': torch.cat(chunks) if chunks else torch.zeros(0, dtype=torch.uint8), 'rows': torch.tensor(rows, dtype=torch.int64),
                  'label': label, 'index': int(index)}
        if self.decode_jpeg_on_gpu:
            from latent_pose_reenactment_amd.utils import jpeg_parse
            sample.update(size=offset, regions=torch.tensor(regions, dtype=torch.int64).reshape(-1, 3), files=files,
                          jpeg=jpeg_parse.pack(descriptors, destinations) if descriptors else None)
        return sample


_OFFSETS = [c for c, name in enumerate(frames.COLUMNS) if name.endswith('_off')]
_H = [c for c, name in enumerate(frames.COLUMNS) if name in ('img_h', 'msk_h')]
_IMAGE_SLOT, _MASK_SLOT, _PRODUCT_SLOT = (frames.COLUMNS.index(n) for n in ('image_slot', 'mask_slot', 'product_slot'))


class Collate:
    """samples -> a raw batch (frames.py): the bytes packed into one buffer, the offsets rebased, the slots made global"""

    def __init__(self, num_frames, finetuning, inference):
        self.frames = 0 if finetuning else num_frames
        self.pose = not finetuning and not inference

    def __call__(self, samples):
        b, k = len(samples), self.frames
        tables, base = [], 0
        for s, sample in enumerate(samples):
            rows = sample['rows'].clone()
            for off, h in zip(_OFFSETS, _H):
                rows[:, off] += base * (rows[:, h] > 0)
            local = rows[:, _IMAGE_SLOT]
            rows[:, _IMAGE_SLOT] = torch.where(local < max(k, 1), s * max(k, 1) + local, b * k + s)
            for col in (_MASK_SLOT, _PRODUCT_SLOT):
                rows[:, col] = torch.where(rows[:, col] >= 0, torch.full_like(local, s), rows[:, col])
            tables.append(rows)
            base += sample['size'] if 'size' in sample else sample['bytes'].numel()
        raw = {'buf': torch.cat([sample['bytes'] for sample in samples]), 'table': torch.cat(tables), 'frames': k, 'pose': self.pose,
               'label': torch.tensor([sample['label'] for sample in samples], dtype=torch.int64),
               'index': torch.tensor([sample['index'] for sample in samples], dtype=torch.int64)}
        if 'size' in samples[0]:             # --decode_jpeg_on_gpu: 'buf' holds the regions decoded in the worker, 'jpeg' the segments of the rest
            from latent_pose_reenactment_amd.utils import jpeg_parse
            regions, packs, bases, files, base, held = [], [], [], [], 0, 0
            for sample in samples:
                regions.append(sample['regions'] + torch.tensor([base, held, 0], dtype=torch.int64))
                if sample['jpeg'] is not None:
                    packs.append(sample['jpeg'])
                    bases.append(base)
                    files += sample['files']
                base += sample['size']
                held += sample['bytes'].numel()
            jpeg = None
            if packs:
                jpeg = {key: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for key, v in jpeg_parse.merge(packs, bases).items()}
            raw.update(nbytes=base, regions=torch.cat(regions), jpeg=jpeg, files=files)
        return raw


class FrameLoader:
    """iterable of (data_dict, target_dict) over a torch DataLoader of raw batches: per batch one pinned host-to-device copy of the packed bytes and
    one launch on the current stream (``frames.prepare``; with ``--blur_padded_bands`` the pad launches before it).  The augmentation parameters are drawn HERE, in the iterating process, so that they do not
    depend on the number of workers: seeded as ``synthetic_voxceleb2_augmented`` seeds them, from (seed, index, visit) for ``part == 'train'`` and from
    (seed, index) alone otherwise."""

    def __init__(self, loader, args, part):
        self.loader, self.dataset = loader, loader.dataset
        self.size, self.part = args.image_size, part
        self.blur_padded_bands = bool(getattr(args, 'blur_padded_bands', False))
        self.pending = []                # decode status words on their way to the host (frames.prepare), checked before the next batch is asked for
        device = str(getattr(args, 'device', 'cuda'))
        self.device = device if device.startswith('cuda') and torch.cuda.is_available() else 'cpu'
        self.augmenter = augmentation.ParametricAugmenter(args)
        self.seed = (getattr(args, 'random_seed', 0) or 0) + (0 if part == 'train' else 7919)
        self.visits = {}
        self.batch_size = loader.batch_size

    def __len__(self):
        return len(self.loader)

    def _aug_params(self, indices):
        """-> {'aug_params': [B, 32]} and / or {'aug_params_extra': [B, 16]}, whichever the flags ask for; the two rows of a sample come from two
        generator streams, so ``aug_params`` is the same with and without the second stage"""
        rows, extra = [], []
        for index in indices:
            visit = 0
            if self.part == 'train':
                visit = self.visits.get(index, 0)
                self.visits[index] = visit + 1
            if self.augmenter.has_first_stage():
                g = torch.Generator().manual_seed((self.seed * 1000003 + index) * 8191 + visit + 700001)
                rows.append(self.augmenter.sample(g))
            if self.augmenter.has_extra_stage():
                g = torch.Generator().manual_seed(augmentation.extra_stream_seed(self.seed, index, visit))
                extra.append(self.augmenter.sample_extra(g))
        out = {}
        if rows:
            out['aug_params'] = torch.stack(rows)
        if extra:
            out['aug_params_extra'] = torch.stack(extra)
        return out

    def __iter__(self):
        batches = iter(self.loader)
        while True:
            frames.check_decoded(self.pending)          # the batch before this one: a stream that did not decode raises, naming its file
            raw = next(batches, None)
            if raw is None:
                return
            if not self.augmenter.is_empty():
                raw = dict(raw, **self._aug_params(raw['index'].tolist()))
            yield frames.prepare(raw, self.size, self.device, self.blur_padded_bands, pending=self.pending)


def get_dataloader(args, part):
    """the hook ``Dataloader.get_dataloader`` honours: rank-strided, shuffled for 'train', as the front-end builds its loader"""
    dataset = Dataset(args, part)
    assert len(dataset) % args.world_size == 0, "the dataset was expected to be equally divisible by `args.world_size`"
    subset = torch.utils.data.Subset(dataset, range(args.rank, len(dataset), args.world_size))
    logger.info(f"This process will receive a dataset with {len(subset)} samples")
    if len(subset) < args.batch_size:
        logger.warning(f"Dataset length is smaller than batch size ({len(subset)} < {args.batch_size}), reducing the latter")
        args.batch_size = len(subset)
    workers = max(0, min(int(getattr(args, 'num_workers', 0)), MAX_WORKERS))
    loader = DataLoader(subset, batch_size=max(1, args.batch_size // args.num_gpus), num_workers=workers, pin_memory=torch.cuda.is_available(),
                        drop_last=(part == 'train'), shuffle=(part == 'train'), collate_fn=Collate(dataset.frames, dataset.finetuning, dataset.inference))
    return FrameLoader(loader, args, part)
