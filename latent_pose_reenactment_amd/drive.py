#!/usr/bin/env python3
"""Reenactment ("driving") entry point with the reference's CLI (drive.py:19-98): load a fine-tuned checkpoint, take the
EMA weights, and for every driving frame run ``embedder.get_pose_embedding`` + ``generator`` (HIP kernels, eval mode: the
spectral norms are constant so the packed bf16 weights are reused).  The reference writes an .mp4 through cv2 (absent here,
out of scope): frames are written as one .npy uint8 array [T, H, 2W, 3] (driver | result) per driving sequence instead, with
``--format png`` as one PNG per frame, <destination>/<driver>/<frame:06>.png (PIL, or ``--png_encoder gpu``: ``hipops.png_encode``), or with ``--format avi`` as a playable Motion-JPEG video
<destination>/<driver>.avi whose frames are JPEG-encoded on the GPU (``hipops.jpeg_encode``): only the compressed bytes cross PCIe."""
import argparse
import copy
import logging
import os
import sys
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_grad_enabled(False)

from utils import utils  # noqa: E402


def string_to_valid_filename(x):
    return str(x).replace('/', '_')


def load_for_inference(checkpoint_path, data_root, device):
    checkpoint_object = utils.torch_load(checkpoint_path)
    saved_args = copy.copy(checkpoint_object['args'])
    saved_args.finetune = True
    saved_args.inference = True
    saved_args.data_root = data_root
    saved_args.world_size = 1
    saved_args.num_workers = 1
    saved_args.batch_size = 1
    saved_args.device = device
    saved_args.bboxes_dir = Path("/non/existent/file")
    saved_args.prefetch_size = 4
    embedder, generator, _, running_averages, _, _, _ = utils.load_model_from_checkpoint(checkpoint_object, saved_args)
    if 'embedder' in running_averages:
        embedder.load_state_dict(running_averages['embedder'])
    if 'generator' in running_averages:
        generator.load_state_dict(running_averages['generator'])
    embedder.train(not saved_args.set_eval_mode_in_test)
    generator.train(not saved_args.set_eval_mode_in_test)
    return embedder, generator, saved_args


def drive_frames(embedder, generator, data_dict):
    """one iteration of the hot loop (drive.py:84-88) on a batch of B >= 1 driving frames -> uint8 [B, H, 2W, 3] frame grids
    (driver | result), left ON THE DEVICE: the caller gathers a whole sequence and crosses PCIe once (no per-frame host sync).
    A batch without ``pose_input_rgbs`` is driven by a pose alone (generators/FSTH.py on ``dec_stickmen``, or on a ``dec_keypoints`` track B x 1 x 136
    that is rendered on the device): its left panel is the ``dec`` stickman"""
    embedder.get_pose_embedding(data_dict)
    generator(data_dict)
    to_u8 = lambda img: img.permute(0, 2, 3, 1).clamp(0, 1).mul(255).byte()
    driver = data_dict.get('pose_input_rgbs')
    if driver is None:
        from latent_pose_reenactment_amd import fsth
        driver = fsth.stickmen(data_dict, 'dec', data_dict['fake_rgbs'].shape[-1])
    if driver.dim() > 4:
        driver = driver[:, 0]
    return torch.cat((to_u8(driver), to_u8(data_dict['fake_rgbs'])), dim=2)


def drive_frame(embedder, generator, data_dict):
    """single-frame form (B = 1) -> uint8 HWC frame grid"""
    return drive_frames(embedder, generator, data_dict)[0]


def write_png_frames(directory, video):
    """``video``: uint8 [T, H, W, 3] on the host -> <directory>/<frame:06>.png, one lossless file per frame; returns the paths"""
    from PIL import Image
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    paths = []
    for t, frame in enumerate(video):
        paths.append(directory / f'{t:06}.png')
        Image.fromarray(np.ascontiguousarray(frame)).save(paths[-1])
    return paths


AVI_CHUNK = 64          # frames per hipops.jpeg_encode / hipops.png_encode call


def write_avi(path, video, fps=25, quality=90, chunk=AVI_CHUNK):
    """``video``: uint8 [T, H, W, 3] frame grids, on the device as ``drive_frames`` leaves them -> a Motion-JPEG AVI at ``path``.  The frames are
    encoded where they are, ``chunk`` at a time (csrc/jpeg.hip; one read-back of one integer per chunk), and only the compressed bytes are copied to
    the host, where utils/mjpeg.AviWriter puts them into the container.  Returns the number of bytes written"""
    from latent_pose_reenactment_amd import hipops
    from latent_pose_reenactment_amd.utils.mjpeg import AviWriter
    if not (isinstance(video, torch.Tensor) and video.dtype == torch.uint8 and video.dim() == 4 and video.shape[3] == 3 and video.shape[0] >= 1):
        raise ValueError(f'write_avi: video must be a uint8 tensor [T, H, W, 3] with T >= 1, got '
                         f'{(video.dtype, tuple(video.shape)) if isinstance(video, torch.Tensor) else type(video).__name__}')
    chunk = max(1, int(chunk))
    with AviWriter(path, video.shape[1], video.shape[2], fps) as avi:
        for t in range(0, video.shape[0], chunk):
            avi.add(*hipops.jpeg_encode(video[t:t + chunk], quality))
    return os.path.getsize(path)


def write_png_frames_gpu(directory, video, chunk=AVI_CHUNK):
    """``video``: uint8 [T, H, W, 3] frame grids, on the device as ``drive_frames`` leaves them -> <directory>/<frame:06>.png, the files
    ``write_png_frames`` names, each decoding to the same pixels.  The frames are encoded where they are, ``chunk`` at a time (csrc/png.hip; one
    read-back of one integer per chunk); the compressed bytes of a chunk are copied once and sliced by its offsets table.  Returns the paths"""
    from latent_pose_reenactment_amd import hipops
    if not (isinstance(video, torch.Tensor) and video.dtype == torch.uint8 and video.dim() == 4 and video.shape[3] == 3 and video.shape[0] >= 1):
        raise ValueError(f'write_png_frames_gpu: video must be a uint8 tensor [T, H, W, 3] with T >= 1, got '
                         f'{(video.dtype, tuple(video.shape)) if isinstance(video, torch.Tensor) else type(video).__name__}')
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    chunk = max(1, int(chunk))
    paths = []
    for t in range(0, video.shape[0], chunk):
        data, offsets = hipops.png_encode(video[t:t + chunk])
        data, offsets = data.cpu().numpy(), offsets.tolist()
        for i, (a, b) in enumerate(zip(offsets, offsets[1:])):
            paths.append(directory / f'{t + i:06}.png')
            with open(paths[-1], 'wb') as f:
                f.write(data[a:b].tobytes())
    return paths


def main():
    logging.basicConfig(level=logging.INFO, stream=sys.stdout, format="%(asctime)s - %(levelname)s - %(message)s")
    logger = logging.getLogger('drive')
    ap = argparse.ArgumentParser(description="Render 'puppeteering' frames, given a fine-tuned model and driving images.",
                                 formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument('checkpoint_path', type=Path)
    ap.add_argument('data_root', type=Path)
    ap.add_argument('--images_paths', type=Path, nargs='+')
    ap.add_argument('--destination', type=Path, required=True)
    ap.add_argument('--batch_size', type=int, default=1, help='driving frames per generator call (the reference drives one frame at a time)')
    ap.add_argument('--format', choices=('npy', 'png', 'avi'), default='npy',
                    help='npy: one uint8 array [T, H, 2W, 3] per driving sequence; png: the same frames as <destination>/<driver>/<frame:06>.png;\n'
                         'avi: the same frames as a Motion-JPEG video <destination>/<driver>.avi, encoded on the GPU')
    ap.add_argument('--png_encoder', choices=('pil', 'gpu'), default='pil',
                    help='with --format png: pil = copy the raw frames to the host and let PIL compress them one by one; gpu = encode them on the\n'
                         'device (csrc/png.hip) and copy the compressed bytes.  Measured on one MI355X, 64 frames of 256 x 512: gpu 1.07 ms\n'
                         'against pil 898 ms (839 x faster); the drive loop writes 443 against 102 frames/s at B = 1 and 2580 against 131 at B = 8.\n'
                         'Both routes keep every pixel; the files differ in size by a few per cent (README)')
    ap.add_argument('--fps', type=float, default=25, help='frame rate written into the .avi')
    ap.add_argument('--jpeg_quality', type=int, default=90, help='JPEG quality of the .avi frames, 1 .. 100 (the IJG scale)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('drive.py needs the MI355X: the generator has no CPU fallback')
    device = 'cuda:0'
    embedder, generator, saved_args = load_for_inference(args.checkpoint_path, args.data_root, device)
    saved_args.batch_size = max(1, args.batch_size)
    from dataloaders.dataloader import Dataloader
    for driver in args.images_paths:
        saved_args.val_split_path = driver
        loader = Dataloader(saved_args.dataloader).get_dataloader(saved_args, part='val', phase='val')
        out = (args.destination / string_to_valid_filename(driver)).with_suffix('.npy')
        out.parent.mkdir(parents=True, exist_ok=True)
        frames = []
        for data_dict, _ in loader:
            utils.dict_to_device(data_dict, device)
            frames.append(drive_frames(embedder, generator, data_dict))       # uint8 on the device: nothing waits for the GPU here
        if args.format == 'avi':
            out = out.with_suffix('.avi')
            nbytes = write_avi(out, torch.cat(frames), args.fps, args.jpeg_quality)       # the frames stay on the device
            logger.info(f'wrote {sum(len(f) for f in frames)} frames ({nbytes} bytes) to {out}')
            continue
        if args.format == 'png' and args.png_encoder == 'gpu':
            out = out.with_suffix('')
            paths = write_png_frames_gpu(out, torch.cat(frames))                         # the frames stay on the device
            logger.info(f'wrote {len(paths)} frames to {out}')
            continue
        video = torch.cat(frames).cpu().numpy()                             # one device-to-host transfer (and sync) per sequence
        if args.format == 'png':
            out = out.with_suffix('')
            write_png_frames(out, video)
        else:
            np.save(out, video)
        logger.info(f'wrote {len(video)} frames to {out}')


if __name__ == '__main__':
    main()
