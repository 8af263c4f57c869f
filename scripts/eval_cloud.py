#!/usr/bin/env python3
"""A fused cloud scored against the lidar: the velodyne scans of a KITTI odometry sequence are fused, under given poses, into a
reference cloud in the same world frame, and the predicted cloud is compared with it by nearest neighbours within a radius.  The
reference has no such program.

  python scripts/eval_cloud.py --cloud cloud.ply (--data_path ROOT --sequence 9 --poses FILE [--frames A:B] | --ref ref.ply) \
         [--config CFG | --K fx fy cx cy] [--height H --width W] [--ref_voxel V] [--min_depth Z] [--max_range R] [--tau T] \
         [--thresholds T1 T2 ...] [--pred_scale S] [--batch_size 12] [--save_ref ref.ply] [--save_error error.ply] [--device cpu]

Scans: <data_path>/sequences/NN/velodyne/%06d.bin (float32 x y z reflectance), velodyne to camera from the "Tr:" line of
<data_path>/sequences/NN/calib.txt.  --poses: camera-to-world poses in KITTI pose text, one per scan of the sequence, typically the
ground truth the cloud was fused with (reconstruct.py --poses gt.txt --depth_scale S); --frames A:B takes the scans A ... B-1.  With a
camera (--config: the datasets' KITTI intrinsics at the config's size or at --height x --width; or --K with --height and --width) only
lidar points inside the camera's image are fused: without it the lidar's 360 degrees count against the recall of a forward-looking
camera.  --ref takes a reference cloud that was saved earlier (--save_ref) instead of the scans.  --ref_voxel, --min_depth, --max_range
and --tau are in the poses' units (metres for the ground truth); --pred_scale multiplies the predicted cloud and is the only alignment
there is.  The defaults of --tau (three voxels of cloud.py's default) and --thresholds (tau/4, tau/2, tau) are UNTUNED.
Prints the scan statistics, one line per cause; both clouds' sizes, dropped points and largest cell; one line per threshold with
precision, recall and F-score; accuracy and completeness (the mean distance to the nearest neighbour, capped at tau).
--save_error writes the predicted cloud coloured by min(distance, tau) / tau through the magma table, pure green (0, 255, 0) where
nothing lies within tau; --save_ref writes the lidar cloud (grey by reflectance).  The work is tripled_amd.cloud_eval (csrc/td_scan.hip
and csrc/td_nn.hip on a HIP device); with --device cpu everything runs through the numpy statements.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from tripled_amd import cloud, cloud_eval, odometry, velodyne  # noqa: E402


def _host(t):
    return np.asarray(t.cpu() if torch.is_tensor(t) else t)


def _load_xyz(path):
    points = cloud.load_ply(path)
    return np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float32), points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cloud", required=True, help="the predicted cloud (PLY of reconstruct.py)")
    ap.add_argument("--data_path", default=None, help="KITTI odometry root (sequences/)")
    ap.add_argument("--sequence", type=int, default=9)
    ap.add_argument("--poses", default=None, help="camera-to-world poses in KITTI pose text, one per scan")
    ap.add_argument("--frames", default=None, help="A:B, the scans A ... B-1 (default: all poses)")
    ap.add_argument("--ref", default=None, help="a saved reference cloud instead of the scans")
    ap.add_argument("--config", default=None)
    ap.add_argument("--K", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"), help="pixels at --height x --width")
    ap.add_argument("--height", type=int, default=None, help="default: the config's")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--ref_voxel", type=float, default=cloud.DEFAULT_VOXEL)
    ap.add_argument("--min_depth", type=float, default=cloud.DEFAULT_MIN_DEPTH)
    ap.add_argument("--max_range", type=float, default=cloud.DEFAULT_MAX_RANGE)
    ap.add_argument("--tau", type=float, default=cloud_eval.DEFAULT_TAU, help="search radius (untuned)")
    ap.add_argument("--thresholds", type=float, nargs="+", default=None, help="ascending, at most tau (default: tau/4 tau/2 tau, untuned)")
    ap.add_argument("--pred_scale", type=float, default=1.0)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--save_ref", default=None)
    ap.add_argument("--save_error", default=None)
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    args = ap.parse_args()
    if (args.ref is None) == (args.data_path is None):
        ap.error("one of --data_path (with --poses) and --ref")
    if args.data_path and not args.poses:
        ap.error("--data_path needs --poses")
    if args.config and args.K:
        ap.error("at most one of --config and --K")
    pred_xyz, pred = _load_xyz(args.cloud)
    if args.ref:
        ref_xyz, _ = _load_xyz(args.ref)
        print("-> Reference cloud %s: %d points" % (args.ref, len(ref_xyz)))
    else:
        K, height, width = None, 0, 0
        if args.config:
            from mmcv import Config
            from mono.datasets.kitti_dataset import KITTIDataset
            cfg = Config.fromfile(args.config)
            height, width = args.height or cfg.model["height"], args.width or cfg.model["width"]
            K = KITTIDataset.K.copy()                # normalised; the datasets scale it like this (float32)
            K[0, :] *= width
            K[1, :] *= height
            K = K[:3, :3].astype(np.float64)
        elif args.K:
            if not (args.height and args.width):
                ap.error("--K needs --height and --width")
            height, width = args.height, args.width
            fx, fy, cx, cy = args.K
            K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        seq = os.path.join(args.data_path, "sequences", "%02d" % args.sequence)
        Tr = velodyne.read_calib_file(os.path.join(seq, "calib.txt"))["Tr"].reshape(3, 4)
        poses = odometry.load_kitti_poses(args.poses)
        a, _, b = (args.frames or ":").partition(":")
        numbers = list(range(int(a or 0), min(int(b or len(poses)), len(poses))))
        if not numbers:
            ap.error("--frames %s of %d poses: nothing to fuse" % (args.frames, len(poses)))
        scans = [np.fromfile(os.path.join(seq, "velodyne", "%06d.bin" % n), dtype=np.float32).reshape(-1, 4) for n in numbers]
        print("-> Fusing %d scans of sequence %02d (%s view test)" % (len(scans), args.sequence, "%d x %d" % (height, width) if K is not None else "no"))
        fuser = cloud_eval.ScanFuser(args.device, args.ref_voxel, Tr, K=K, height=height, width=width, min_depth=args.min_depth,
                                     max_range=args.max_range, batch_size=args.batch_size)
        ref = fuser.fuse(scans, poses[numbers])
        for name, value in ref.stats.items():
            print("scans %s %d" % (name, value))
        ref_xyz = ref.xyz
        if args.save_ref:
            os.makedirs(os.path.dirname(os.path.abspath(args.save_ref)), exist_ok=True)
            cloud.save_ply(args.save_ref, ref.xyz, ref.rgb, ref.count)
            print("saved %d reference points to %s" % (len(ref.keys), args.save_ref))
    result = cloud_eval.CloudComparer(args.device, args.tau, args.thresholds).compare(pred_xyz, ref_xyz, args.pred_scale)
    for name, n, grid in (("predicted", "n_pred", "pred_grid"), ("reference", "n_ref", "ref_grid")):
        print("%s cloud: %d points, dropped %d, cells %d, max_cell %d" % (
            name, result.stats[n], result.stats[grid]["dropped"], result.stats[grid]["cells"], result.stats[grid]["max_cell"]))
    for t, p, r, f in zip(result.thresholds, result.precision, result.recall, result.fscore):
        print("threshold %.6g: precision %.4f recall %.4f fscore %.4f" % (t, p, r, f))
    print("accuracy %.6g completeness %.6g (tau %.6g)" % (result.accuracy, result.completeness, args.tau))
    if args.save_error:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_error)), exist_ok=True)
        colors = cloud_eval.error_colors(_host(result.pred.d2), _host(result.pred.index), args.tau)
        cloud.save_ply(args.save_error, pred_xyz, colors, pred["count"])
        print("saved %d error-coloured points to %s" % (len(pred_xyz), args.save_error))


if __name__ == "__main__":
    main()
