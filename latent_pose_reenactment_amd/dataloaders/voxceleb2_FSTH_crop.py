"""The reference's cropped keypoint dataset plugin (dataloaders/voxceleb2_FSTH_crop.py): ``dataloaders/voxceleb2.py`` on the lower 80 % of every
frame.  The reference cuts rows [cut_t, cut_b) and columns [cut_l, cut_r) with
  cut_t = min(H - 1, round(0.2 H)), cut_b = max(cut_t + 1, round(H)), cut_l = min(W - 1, round(0.1 W)), cut_r = max(cut_l + 1, round(0.9 W))
(Python's round, floats as it forms them) and resizes the two axes by their own factors.  Here the box is SQUARE: n = cut_b - cut_t rows, and
n columns from l = (W - n) // 2 -- the reference's cut_r - cut_l differs from n by one pixel at most common sizes (204 against 205 at 256 x 256), a
deliberate deviation of at most one pixel that keeps the table of lp_frames_prepare to square boxes.  Keypoints are (kp - [l, cut_t]) / n.  A box
that leaves a frame which is not square goes through the border rule of csrc/frames.hip."""
from latent_pose_reenactment_amd.dataloaders import voxceleb2 as _base


def crop_box(h, w, file=None):
    """-> (t, l, n) of the square box"""
    cut_t = min(h - 1, round(0.2 * h))
    cut_b = max(cut_t + 1, round(1.0 * h))
    n = cut_b - cut_t
    return cut_t, (w - n) // 2, n


class SampleLoader(_base.SampleLoader):
    box = staticmethod(crop_box)


class Dataset(_base.Dataset):
    SAMPLE_LOADER = SampleLoader
