"""tests/golden/velodyne.npz and the numpy statement against the reference's checkout, where there is one (TD_REFERENCE, default
/root/reference): the golden is regenerated with the reference's generate_depth_map and compared with the committed file, and one
scan of KITTI size goes through the reference and the statement.  Skipped without the checkout."""
import os
import sys

import numpy as np
import pytest

import tripled_amd  # noqa: F401
from tests import velo_util
from tests.test_velodyne_cpu import GOLDEN, check_against_reference
from tripled_amd import velodyne

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("TD_REFERENCE", "/root/reference")
pytestmark = pytest.mark.skipif(not os.path.isfile(os.path.join(REFERENCE, "mono", "datasets", "kitti_utils.py")),
                                reason="no reference checkout at %s" % REFERENCE)


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_golden_velo
    finally:
        sys.path.pop(0)
    return gen_golden_velo


def test_golden_is_what_the_reference_computes():
    fresh = _generator().record(REFERENCE)
    with np.load(GOLDEN) as committed:
        assert sorted(committed.files) == sorted(fresh)
        for k in committed.files:
            if "_depth_" not in k:                              # the points and the calibration numbers
                assert committed[k].dtype == fresh[k].dtype and np.array_equal(committed[k], fresh[k], equal_nan=True), k
            else:                                               # another BLAS may round the reference's np.dot differently
                check_against_reference(committed[k], fresh[k], k.endswith("vel1"), k)
    assert not hasattr(np, "int")                               # the alias the reference needs does not outlive the generator


@pytest.mark.parametrize("cam", [2, 3])
def test_kitti_size_scan(cam):
    gen = _generator()
    kitti_utils = gen.load_reference(REFERENCE)
    H, W, n = 375, 1242, 120000
    calib = velo_util.synthetic_calibration(H, W, 21)
    points = velo_util.synthetic_scan(calib, n, 22)
    maps, read = gen.reference_scene(kitti_utils, calib, points, cams=(cam,))
    P = velo_util.projection(read, cam)
    for vd in (False, True):
        m, stats = velodyne.depth_map_numpy(points, P, H, W, vd)
        check_against_reference(m, maps[(cam, vd)], vd, "375 x 1242 cam %d vel_depth %d" % (cam, vd))
    # the fixture exercises what it claims
    mixed, dups = velo_util.false_collisions(points, P, H, W)
    stats = dict(zip(velodyne.STATS, velodyne.depth_map_numpy(points, P, H, W)[1]))
    print("duplicate groups %d, joining two pixels %d, stats %s" % (dups, mixed, stats))
    assert dups > 1000 and mixed >= 1 and stats["pixels_clamped"] >= 1 and stats["behind"] >= 1 and stats["outside"] >= 1
