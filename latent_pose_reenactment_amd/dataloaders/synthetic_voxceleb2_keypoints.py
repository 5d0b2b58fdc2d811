"""The samples of dataloaders/synthetic_voxceleb2_stickmen.py with the poses left as keypoints: the contract of dataloaders/synthetic_voxceleb2.py plus
  data_dict:   ... + enc_keypoints K x 136, dec_keypoints 1 x 136 ((x, y) pairs in [0, 1], fp32)
Same seed stream, so the keypoints are bit-identical to the ones synthetic_voxceleb2_stickmen draws; nothing is drawn here.  The nets of the FSTH family
render the stickmen they need from the keypoints on the device (fsth.stickmen -> hipops.stickman_render): 136 floats per frame cross to the GPU
instead of 3 x S x S, and the host renders nothing."""
from latent_pose_reenactment_amd.dataloaders import synthetic_voxceleb2 as _base
from latent_pose_reenactment_amd.dataloaders.synthetic_voxceleb2_stickmen import sample_keypoints


def make_sample(index, image_size, num_frames, num_labels, finetune, seed):
    data, target = _base.make_sample(index, image_size, num_frames, num_labels, finetune, seed)
    enc_pts, dec_pts = sample_keypoints(index, num_frames, seed)
    data['enc_keypoints'] = enc_pts.reshape(num_frames, 136)
    data['dec_keypoints'] = dec_pts.reshape(1, 136)
    return data, target


class Dataset(_base.Dataset):
    @staticmethod
    def get_dataset(args, part):
        return Dataset(args, part)

    def __getitem__(self, index):
        return make_sample(index, self.size, self.frames, self.num_labels, self.finetune, self.seed)
