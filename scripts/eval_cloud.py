#!/usr/bin/env python3
"""A fused cloud scored against the lidar: the velodyne scans of a KITTI odometry sequence are fused, under given poses, into a
reference cloud in the same world frame, and the predicted cloud is compared with it by nearest neighbours within a radius.  The
reference has no such program.

  python scripts/eval_cloud.py --cloud cloud.ply (--data_path ROOT --sequence 9 --poses FILE [--frames A:B] | --ref ref.ply) \
         [--config CFG | --K fx fy cx cy] [--height H --width W] [--ref_voxel V] [--min_depth Z] [--max_range R] [--tau T] \
         [--thresholds T1 T2 ...] [--pred_scale S] [--batch_size 12] [--save_ref ref.ply] [--save_error error.ply] [--device cpu] \
         [--align {none,rigid,similarity} [--align_tau T] [--align_iters 30] [--align_trim D] [--align_stride 1] [--init_poses FILE] \
          [--align_criterion {point,plane}] [--save_transform T.txt] [--save_aligned aligned.ply]] \
         [--align_normal_radius R] [--align_min_neighbours 6] [--align_max_curvature 0.01] [--align_rcond 1e-3] [--save_ref_normals FILE]

Scans: <data_path>/sequences/NN/velodyne/%06d.bin (float32 x y z reflectance), velodyne to camera from the "Tr:" line of
<data_path>/sequences/NN/calib.txt.  --poses: camera-to-world poses in KITTI pose text, one per scan of the sequence, typically the
ground truth the cloud was fused with (reconstruct.py --poses gt.txt --depth_scale S); --frames A:B takes the scans A ... B-1.  With a
camera (--config: the datasets' KITTI intrinsics at the config's size or at --height x --width; or --K with --height and --width) only
lidar points inside the camera's image are fused: without it the lidar's 360 degrees count against the recall of a forward-looking
camera.  --ref takes a reference cloud that was saved earlier (--save_ref) instead of the scans.  --ref_voxel, --min_depth, --max_range
and --tau are in the poses' units (metres for the ground truth); --pred_scale multiplies the predicted cloud and, without --align, is
the only alignment there is.  The defaults of --tau (three voxels of cloud.py's default) and --thresholds (tau/4, tau/2, tau) are UNTUNED.
--align rigid | similarity first registers the predicted cloud to the reference by iterated closest points (tripled_amd.cloud_align:
x' = c R x + t, point to point, predicted into reference) and scores the ALIGNED cloud.  The initial guess is --pred_scale, or, with
--init_poses (the poses the cloud was fused with, reconstruct.py --save_poses; one per pose of --poses), the closed-form similarity
between the two trajectories' camera centres: ICP cannot start from the identity when the scale is off by 36.  --align_tau is the
radius of the correspondence search (default 2 tau), --align_trim leaves out correspondences farther apart (default: none),
--align_stride uses every n-th point, --align_iters bounds the passes; all UNTUNED.  Prints the initial guess, one line per pass
(matched, rms), the final scale, R, t and whether it converged; the score lines are then prefixed "aligned".  --save_transform writes
the 4x4 [[c R, t], [0, 1]] as text, --save_aligned the aligned cloud with its colours.
--align_criterion plane minimises the distance along the REFERENCE'S NORMALS instead (point to plane: two clouds that sample the same
surfaces at different points; tripled_amd.cloud_normals, csrc/td_normals.hip): the normals are estimated once from the neighbours within
--align_normal_radius (default and at most --align_tau), a point with fewer than --align_min_neighbours of them or a patch rougher than
--align_max_curvature (lambda_min / trace) has none and is not matched; a direction whose eigenvalue is below --align_rcond of the
largest is dropped from the step and reported (the translation along a corridor); all UNTUNED.  It prints the normal counters once and
per pass additionally the rms along the normals and the rank.  --save_ref_normals writes the reference cloud with these normals as
nx ny nz (all zero: none), with or without --align; a --ref file without colours or counts gets black and 1.  With --orient_normals
the written normals are first turned towards the nearest camera of --poses (the poses the scans were fused under; with --ref give the
--poses the reference was fused under; cloud_normals.orient_*, csrc/td_surfel.hip) and the counters of that are printed; the alignment
itself keeps the unoriented normals (the plane criterion is sign-free, and an alignment must not change).
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
from tripled_amd import cloud, cloud_align, cloud_eval, cloud_normals, odometry, velodyne  # noqa: E402


def _host(t):
    return np.asarray(t.cpu() if torch.is_tensor(t) else t)


def _load_xyz(path):
    points = cloud.load_ply(path)
    return np.stack([points["x"], points["y"], points["z"]], 1).astype(np.float32), points


def _align(args, pred_xyz, ref_xyz):
    """--align: the initial guess, the passes and the result are printed; -> the aligned cloud, float64 [n,3] on the host."""
    with_scale = args.align == "similarity"
    init = (args.pred_scale, np.eye(3), np.zeros(3))
    if args.init_poses:
        gt, own = odometry.load_kitti_poses(args.poses), odometry.load_kitti_poses(args.init_poses)
        if len(own) != len(gt):
            raise SystemExit("--init_poses: %d poses, --poses has %d" % (len(own), len(gt)))
        a, _, b = (args.frames or ":").partition(":")
        rows = slice(int(a or 0), int(b or len(gt)))
        if not with_scale:
            own[:, :, 3] *= args.pred_scale              # rigid: the scale stays --pred_scale, so the centres are aligned at it
        c, R, t = cloud_align.similarity_from_poses(own[rows], gt[rows], with_scale)
        init = (c if with_scale else args.pred_scale, R, t)
    align_tau = 2.0 * args.tau if args.align_tau is None else args.align_tau
    print("-> Aligning (%s, tau %.6g, at most %d passes, stride %d)" % (args.align, align_tau, args.align_iters, args.align_stride))
    print("initial scale %.9g R %s t %s" % (init[0], " ".join("%.9g" % v for v in np.reshape(init[1], -1)), " ".join("%.9g" % v for v in init[2])))
    aligner = cloud_align.CloudAligner(args.device, align_tau, args.align, args.align_iters, args.align_trim, args.align_stride,
                                       criterion=args.align_criterion, normal_radius=args.align_normal_radius,
                                       min_neighbours=args.align_min_neighbours, max_curvature=args.align_max_curvature, rcond=args.align_rcond)
    result = aligner.align(pred_xyz, ref_xyz, init)
    if args.align_criterion == "plane":
        print("reference normals: " + " ".join("%s %d" % item for item in aligner.normal_stats.items()))
    for n, (matched, rms) in enumerate(result.history):
        line = "pass %d: matched %d rms %.6g" % (n, matched, rms)
        if args.align_criterion == "plane":
            plane_rms, rank, dropped = aligner.plane_history[n]
            line += " plane rms %.6g rank %d" % (plane_rms, rank)
            if dropped is not None:
                line += " dropped " + "; ".join(" ".join("%.3f" % v for v in row) for row in dropped)
        print(line)
    print("scale %.9g R %s t %s" % (result.scale, " ".join("%.9g" % v for v in result.R.reshape(-1)), " ".join("%.9g" % v for v in result.t)))
    print("converged %s after %d passes" % (result.converged, result.iterations))
    if args.save_transform:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_transform)), exist_ok=True)
        np.savetxt(args.save_transform, cloud_align.matrix(result.scale, result.R, result.t), fmt="%.17g")
        print("saved the transform to %s" % args.save_transform)
    if aligner.on_hip:
        moved = cloud_align.transform_hip(torch.as_tensor(pred_xyz).to(aligner.device, torch.float64).contiguous(), result.scale, result.R, result.t)
        return moved.cpu().numpy()
    return cloud_align.transform_numpy(pred_xyz, result.scale, result.R, result.t)


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
    ap.add_argument("--align", choices=("none", "rigid", "similarity"), default="none", help="register the cloud to the reference first")
    ap.add_argument("--align_tau", type=float, default=None, help="radius of the correspondence search (default: 2 tau, untuned)")
    ap.add_argument("--align_iters", type=int, default=30)
    ap.add_argument("--align_trim", type=float, default=None, help="leave out correspondences farther apart (default: align_tau)")
    ap.add_argument("--align_stride", type=int, default=1, help="align on every n-th predicted point")
    ap.add_argument("--init_poses", default=None, help="the poses the cloud was fused with; aligned to --poses for the initial guess")
    ap.add_argument("--save_transform", default=None, help="the 4x4 [[c R, t], [0, 1]] as text")
    ap.add_argument("--save_aligned", default=None, help="the aligned cloud (PLY)")
    ap.add_argument("--align_criterion", choices=cloud_align.CRITERIA, default="point", help="plane: the distance along the reference's normals")
    ap.add_argument("--align_normal_radius", type=float, default=None, help="neighbourhood of a normal (default: align_tau, untuned)")
    ap.add_argument("--align_min_neighbours", type=int, default=6, help="fewer neighbours: no normal (untuned)")
    ap.add_argument("--align_max_curvature", type=float, default=0.01, help="a rougher patch (lambda_min / trace): no normal (untuned)")
    ap.add_argument("--align_rcond", type=float, default=1e-3, help="eigenvalues below this fraction of the largest are dropped (untuned)")
    ap.add_argument("--save_ref_normals", default=None, help="the reference cloud with nx ny nz (PLY)")
    ap.add_argument("--orient_normals", action="store_true", help="turn the saved normals towards the nearest camera of --poses")
    args = ap.parse_args()
    if args.align == "none" and (args.init_poses or args.save_transform or args.save_aligned):
        ap.error("--init_poses, --save_transform and --save_aligned need --align rigid or similarity")
    if args.align == "none" and args.align_criterion != "point":
        ap.error("--align_criterion needs --align rigid or similarity")
    if args.orient_normals and not (args.save_ref_normals and args.poses):
        ap.error("--orient_normals needs --save_ref_normals and --poses")
    if args.init_poses and not args.poses:
        ap.error("--init_poses needs --poses, the trajectory it is aligned to")
    if (args.ref is None) == (args.data_path is None):
        ap.error("one of --data_path (with --poses) and --ref")
    if args.data_path and not args.poses:
        ap.error("--data_path needs --poses")
    if args.config and args.K:
        ap.error("at most one of --config and --K")
    pred_xyz, pred = _load_xyz(args.cloud)
    if args.ref:
        ref_xyz, saved = _load_xyz(args.ref)
        ref_rgb = ref_count = None                   # read from ``saved`` where they are needed, if it has them
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
        ref_xyz, ref_rgb, ref_count = ref.xyz, ref.rgb, ref.count
        if args.save_ref:
            os.makedirs(os.path.dirname(os.path.abspath(args.save_ref)), exist_ok=True)
            cloud.save_ply(args.save_ref, ref.xyz, ref.rgb, ref.count)
            print("saved %d reference points to %s" % (len(ref.keys), args.save_ref))
    if args.save_ref_normals:
        align_tau = 2.0 * args.tau if args.align_tau is None else args.align_tau
        estimator = cloud_normals.CloudNormals(args.device, align_tau, args.align_normal_radius, args.align_min_neighbours, args.align_max_curvature)
        if args.orient_normals:
            view_poses = odometry.load_kitti_poses(args.poses)
            a, _, b = (args.frames or ":").partition(":")
            found = estimator.estimate(ref_xyz, poses=view_poses[int(a or 0):int(b or len(view_poses))])
        else:
            found = estimator.estimate(ref_xyz)
        if ref_rgb is None:                          # a reference PLY may hold x y z alone: black, and one sample per point
            names, n = saved.dtype.names, len(saved)
            has_rgb = all(c in names for c in ("red", "green", "blue"))
            ref_rgb = np.stack([saved["red"], saved["green"], saved["blue"]], 1) if has_rgb else np.zeros((n, 3), np.uint8)
            ref_count = saved["count"] if "count" in names else np.ones(n, np.int32)
        os.makedirs(os.path.dirname(os.path.abspath(args.save_ref_normals)), exist_ok=True)
        cloud.save_ply(args.save_ref_normals, ref_xyz, ref_rgb, ref_count, normals=_host(found.normal))
        print("saved %d reference points with normals to %s: %s" % (len(_host(ref_xyz)), args.save_ref_normals,
                                                                    " ".join("%s %d" % item for item in found.stats.items())))
    label, pred_scale = "", args.pred_scale
    if args.align != "none":
        pred_xyz = _align(args, pred_xyz, ref_xyz)
        label, pred_scale = "aligned ", 1.0
        if args.save_aligned:
            os.makedirs(os.path.dirname(os.path.abspath(args.save_aligned)), exist_ok=True)
            cloud.save_ply(args.save_aligned, pred_xyz, np.stack([pred["red"], pred["green"], pred["blue"]], 1), pred["count"])
            print("saved %d aligned points to %s" % (len(pred_xyz), args.save_aligned))
    result = cloud_eval.CloudComparer(args.device, args.tau, args.thresholds).compare(pred_xyz, ref_xyz, pred_scale)
    for name, n, grid in (("predicted", "n_pred", "pred_grid"), ("reference", "n_ref", "ref_grid")):
        print("%s%s cloud: %d points, dropped %d, cells %d, max_cell %d" % (
            label if name == "predicted" else "", name, result.stats[n], result.stats[grid]["dropped"], result.stats[grid]["cells"], result.stats[grid]["max_cell"]))
    for t, p, r, f in zip(result.thresholds, result.precision, result.recall, result.fscore):
        print("%sthreshold %.6g: precision %.4f recall %.4f fscore %.4f" % (label, t, p, r, f))
    print("%saccuracy %.6g completeness %.6g (tau %.6g)" % (label, result.accuracy, result.completeness, args.tau))
    if args.save_error:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_error)), exist_ok=True)
        colors = cloud_eval.error_colors(_host(result.pred.d2), _host(result.pred.index), args.tau)
        cloud.save_ply(args.save_error, pred_xyz, colors, pred["count"])
        print("saved %d error-coloured points to %s" % (len(pred_xyz), args.save_error))


if __name__ == "__main__":
    main()
