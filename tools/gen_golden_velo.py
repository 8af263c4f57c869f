#!/usr/bin/env python3
"""Records tests/golden/velodyne.npz: two small synthetic calibrations with a scan each, and what the REFERENCE's generate_depth_map
(mono/datasets/kitti_utils.py:50-102) makes of them, so that the tests of tripled_amd.velodyne (CPU and GPU) have the reference's
maps where its checkout is not present.

  python tools/gen_golden_velo.py [--reference /path/to/reference] [--out tests/golden/velodyne.npz]

The reference defaults to $TD_REFERENCE.  Its kitti_utils.py is loaded stand-alone from its file; it spells an integer cast
``np.int``, which numpy 2 no longer has, so the name is aliased to ``int`` in this process while the function runs and removed
again afterwards.  The reference's files are not touched.  Recorded per scene s in (a: 9 x 14, 400 points; b: 12 x 33, 3000
points), data only:
  s_points [n,4] float32             the scan as its file holds it (tests/velo_util.synthetic_scan)
  s_S_rect_02, s_P_rect_02, s_P_rect_03, s_R_rect_00, s_R, s_T      the calibration files' numbers, as read_calib_file returns them
  s_depth_cam{2,3}_vel{0,1} [H,W] float64      generate_depth_map(calib_dir, scan, cam, vel_depth)
The conditions the tests rely on are checked here: every scene has duplicate groups, a group that joins two pixels, and a pixel
clamped from a negative depth.
"""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from tests import velo_util  # noqa: E402
from tripled_amd import velodyne  # noqa: E402


def load_reference(reference_root):
    """The reference's mono/datasets/kitti_utils.py as a module, without importing its package."""
    path = os.path.join(reference_root, "mono", "datasets", "kitti_utils.py")
    bytecode = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location("_reference_kitti_utils", path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module
    finally:
        sys.dont_write_bytecode = bytecode


def reference_depth_map(kitti_utils, calib_dir, scan_path, cam, vel_depth):
    """generate_depth_map with ``np.int`` present for the duration of the call."""
    had = hasattr(np, "int")
    if not had:
        np.int = int
    try:
        with np.errstate(all="ignore"):
            return kitti_utils.generate_depth_map(calib_dir, scan_path, cam, vel_depth)
    finally:
        if not had:
            del np.int


def reference_scene(kitti_utils, calib, points, cams=(2, 3), vel_depths=(False, True)):
    """{(cam, vel_depth): map} and the calibration numbers as the reference reads them back from the files."""
    with tempfile.TemporaryDirectory() as tmp:
        velo_util.write_calib(tmp, calib)
        scan_path = velo_util.write_scan(tmp, "drive", 0, points)
        maps = {(cam, bool(vd)): reference_depth_map(kitti_utils, tmp, scan_path, cam, vd) for cam in cams for vd in vel_depths}
        cam2cam = kitti_utils.read_calib_file(os.path.join(tmp, "calib_cam_to_cam.txt"))
        velo2cam = kitti_utils.read_calib_file(os.path.join(tmp, "calib_velo_to_cam.txt"))
    read = {k: np.asarray((velo2cam if k in ("R", "T") else cam2cam)[k], dtype=np.float64) for k in velo_util.CALIB_KEYS}
    return maps, read


def check_conditions(name, calib, points):
    H, W = velo_util.size_of(calib)
    P = velo_util.projection(calib, 2)
    mixed, dups = velo_util.false_collisions(points, P, H, W)
    stats = velodyne.depth_map_numpy(points, P, H, W)[1]
    if not (dups > 0 and mixed > 0 and stats[5] > 0 and stats[1] > 0 and stats[2] > 0):
        raise ValueError("scene %s does not exercise what it claims: %d duplicate groups, %d joining two pixels, stats %s"
                         % (name, dups, mixed, stats.tolist()))
    return mixed, dups, stats


def record(reference_root):
    kitti_utils = load_reference(reference_root)
    out = {}
    for name, H, W, n, seed in velo_util.GOLDEN_SCENES:
        calib = velo_util.synthetic_calibration(H, W, seed)
        points = velo_util.synthetic_scan(calib, n, seed)
        maps, read = reference_scene(kitti_utils, calib, points)
        out[name + "_points"] = points
        for k in velo_util.CALIB_KEYS:
            out["%s_%s" % (name, k)] = read[k]
        for (cam, vd), m in maps.items():
            out["%s_depth_cam%d_vel%d" % (name, cam, int(vd))] = np.asarray(m, dtype=np.float64)
        mixed, dups, stats = check_conditions(name, read, points)
        print("scene %s (%d x %d, %d points): %d duplicate groups, %d joining two pixels, stats %s"
              % (name, H, W, n, dups, mixed, dict(zip(velodyne.STATS, stats.tolist()))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TD_REFERENCE"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "velodyne.npz"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or TD_REFERENCE): the reference's checkout")
    data = record(args.reference)
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
