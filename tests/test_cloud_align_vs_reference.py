"""tripled_amd.cloud_align's closed-form solve against the reference's ``umeyama_alignment`` (mono/tools/geometry.py), loaded
stand-alone from the reference's checkout where there is one (TD_REFERENCE, default /root/reference); skipped where there is none.
Nothing of the reference is copied: its function and its ground-truth poses of sequence 09 are read in place.

The case: the 1 591 camera centres of mono/datasets/gt_pose/09.txt against a copy that is rotated, scaled by 1/36 (one unit of a
stereo-trained model is about 36 m) and noised.  Both of this project's routes to (c, R, t) -- similarity_from_poses, centred like the
reference's function, and solve_from_moments over moments_numpy, which is not centred but taken about an origin -- agree with it within
the project's RTOL = 1e-9 (tests/odom_util.py), relative to the largest entry of each quantity."""
import importlib.util
import os

import numpy as np
import pytest

import tripled_amd  # noqa: F401
from tripled_amd import cloud_align, odometry
from tests import cloud_align_util as U
from tests.odom_util import RTOL

REFERENCE = os.environ.get("TD_REFERENCE", "/root/reference")
GEOMETRY = os.path.join(REFERENCE, "mono", "tools", "geometry.py")
POSES = os.path.join(REFERENCE, "mono", "datasets", "gt_pose", "09.txt")
pytestmark = pytest.mark.skipif(not (os.path.isfile(GEOMETRY) and os.path.isfile(POSES)), reason="the reference checkout is not present")


@pytest.fixture(scope="module")
def case():
    spec = importlib.util.spec_from_file_location("_reference_geometry", GEOMETRY)
    geometry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(geometry)
    gt = odometry.load_kitti_poses(POSES)
    assert gt.shape == (1591, 3, 4)
    rng = np.random.default_rng(9)
    R = U.rotation([0.2, 1.0, -0.4], 37.0)
    own = gt.copy()
    own[:, :, 3] = (gt[:, :, 3].dot(R.T) + [3.0, -1.0, 2.0]) / 36.0 + rng.normal(0, 0.01, (len(gt), 3))
    want = {ws: geometry.umeyama_alignment(own[:, :, 3].T.copy(), gt[:, :, 3].T.copy(), ws) for ws in (True, False)}      # -> r, t, c
    return own, gt, want


def _close(got, want, label):
    (c, R, t), (wR, wt, wc) = got, want
    errs = (abs(c - wc) / abs(wc), np.abs(R - wR).max(), np.abs(t - wt).max() / np.abs(wt).max())
    print("%s: relative error of c %.3g, R %.3g, t %.3g" % ((label,) + errs))
    assert max(errs) <= RTOL, errs


@pytest.mark.parametrize("with_scale", [True, False])
def test_similarity_from_poses_is_the_reference_closed_form(case, with_scale):
    own, gt, want = case
    assert 30.0 < want[True][2] < 40.0                                 # the planted 1/36 is what is being undone
    _close(cloud_align.similarity_from_poses(own, gt, with_scale), want[with_scale], "similarity_from_poses")


@pytest.mark.parametrize("with_scale", [True, False])
def test_solve_from_moments_is_the_reference_closed_form(case, with_scale):
    own, gt, want = case
    x, y = np.ascontiguousarray(own[:, :, 3]), np.ascontiguousarray(gt[:, :, 3])
    origin = 0.5 * (y.min(0) + y.max(0))                               # CloudAligner's: the centre of the reference's bounding box
    m, n, bad = cloud_align.moments_numpy(x, y, np.arange(len(x)), np.zeros(len(x)), 0.0, origin)
    assert (n, bad) == (len(x), 0)
    c, R, t = cloud_align.solve_from_moments(n, m, with_scale)         # about the origin: q - o = c R (p - o) + t
    _close((c, R, c * R.dot(-origin) + t + origin), want[with_scale], "solve_from_moments")
