"""The keypoint sets and tables that tests/test_stickman_hard_cpu.py holds the host twin to and tests/test_stickman_hard_gpu.py the kernel: built
once, shared, never changed.  Every set is fp32 [n, 68, 2] in units of the image side (a point at pixel p of an S-pixel image is p / S)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'latent_pose_reenactment_amd'), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from latent_pose_reenactment_amd.dataloaders.synthetic_voxceleb2_stickmen import REFERENCE_PARTS, REFERENCE_PARTS_NO_OVAL, face_keypoints  # noqa: E402

SIZES = (1, 5, 8, 22, 64)
THICKNESSES = (1, 2, 3, 8)
# two parts that cross: a white horizontal bar drawn first, a red vertical bar drawn over it -- the crossing is red by painter's order alone
CROSSING_PARTS = ((0, 1, False, (1.0, 1.0, 1.0)), (2, 3, False, (1.0, 0.0, 0.0)))


def faces(n, seed=40):
    return torch.stack([face_keypoints(torch.Generator().manual_seed(seed + i)) for i in range(n)])


def keypoint_sets(n, size):
    """name -> fp32 [n, 68, 2]"""
    base = faces(n)
    s = float(size)
    sets = {'faces': base, 'all-equal': torch.full((n, 68, 2), 0.5)}
    zero = base.clone()
    zero[:, 18] = zero[:, 17]; zero[:, 37] = zero[:, 36]; zero[:, 48:60] = zero[:, 48:49]          # zero-length segments, a whole part in one point
    sets['zero-length'] = zero
    # every point on a half-integer pixel position: x * S = k + 0.5 exactly (S a power of two) or to fp32 rounding, so the rounding rule decides
    ties = ((base * s).floor() + 0.5) / s
    sets['rounding-ties'] = ties
    outside = base.clone()
    outside[:, 0] = torch.tensor([-0.3, 0.5]); outside[:, 8] = torch.tensor([0.5, 1.4]); outside[:, 16] = torch.tensor([1.3, 0.4])          # left, below, right
    outside[:, 19] = torch.tensor([0.4, -0.25]); outside[:, 33] = torch.tensor([1.0, 1.0]); outside[:, 27] = torch.tensor([-1.0 / s, 0.0])          # above; corner; one pixel out
    sets['outside'] = outside
    far = base.clone()
    far[:, 3] = torch.tensor([1.0e6, 0.5]); far[:, 24] = torch.tensor([-3.0e38, 3.0e38]); far[:, 50] = torch.tensor([float('inf'), float('-inf')])          # the clamp
    sets['far-outside'] = far
    nan = base.clone()
    nan[:, 40, 0] = float('nan')          # one NaN coordinate: the lower clamp bound
    sets['one-nan'] = nan
    return sets


N_MAX = 3
_SETS, _WANT = {}, {}


def points(size, name):
    """the set ``name`` for ``size``, [N_MAX, 68, 2] (built once)"""
    if size not in _SETS:
        _SETS[size] = keypoint_sets(N_MAX, size)
    return _SETS[size][name]


SET_NAMES = tuple(keypoint_sets(1, 8))


def want(size, thickness, oval, name):
    """the restatement's image of ``points(size, name)``, [N_MAX, 3, S, S] (computed once per case and shared; callers must not write into it)"""
    import stickman_hard_restatement as HR
    key = (size, thickness, oval, name)
    if key not in _WANT:
        _WANT[key] = HR.render(points(size, name), size, REFERENCE_PARTS if oval else REFERENCE_PARTS_NO_OVAL, thickness)
    return _WANT[key]


def crossing_points(size):
    """[1, 68, 2]: points 0-1 a horizontal bar, 2-3 a vertical bar through its middle (``CROSSING_PARTS``)"""
    pts = torch.zeros(1, 68, 2)
    m = (size // 2) / float(size)
    pts[0, 0] = torch.tensor([0.0, m]); pts[0, 1] = torch.tensor([1.0, m])
    pts[0, 2] = torch.tensor([m, 0.0]); pts[0, 3] = torch.tensor([m, 1.0])
    return pts


def boundary_case(size, thickness):
    """an axis-aligned segment from (1, c) to (size - 2, c), even ``thickness``: for a pixel (u, c +- T / 2) beside its body, cross = L (T / 2) and
    4 cross^2 = T^2 L2 EXACTLY -- the boundary of the body's test, which must count as covered -> ([1, 68, 2] points, parts, c)"""
    assert thickness % 2 == 0 and size >= 2 * thickness + 4
    c = size // 2
    pts = torch.zeros(1, 68, 2)
    pts[0, 0] = torch.tensor([1.0 / size, c / float(size)]); pts[0, 1] = torch.tensor([(size - 2.0) / size, c / float(size)])
    return pts, ((0, 1, False, (0.0, 1.0, 0.0)),), c
