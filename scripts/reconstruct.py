#!/usr/bin/env python3
"""Scene reconstruction from a checkpoint: the predicted depth maps and camera poses of a KITTI odometry sequence fused into one
voxel-averaged coloured point cloud (binary PLY: x y z float, red green blue uchar, count int).  The reference has no such program.

  python scripts/reconstruct.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth --data_path /data/kitti_odom \
         --sequence 9 [--frames A:B] [--poses FILE] [--voxel V] [--stride S] [--border P] [--max_range R] [--edge E] [--min_count N] \
         [--min_views M] [--view_radius R] [--view_tol T] [--depth_scale S] [--pose_scale S] [--batch_size 12] [--precision bf16] \
         [--post_process] [--device cpu] [--save_poses FILE] [--tsdf [--trunc_voxels 3] [--min_weight 2] [--save_map map.npz]] \
         --out cloud.ply

Frames: <data_path>/sequences/NN/image_0/%06d.png; the frame count is the line count of <data_path>/poses/NN.txt (or of --poses).
Without --poses the model's own poses are used (depth and pose share the model's scale); --poses FILE takes camera-to-world poses
in KITTI pose text (the ground truth: give --depth_scale, the model's unit in metres, ~36 for a stereo-trained checkpoint).
--voxel, --max_range and --edge are in the model's units; their defaults are untuned starting values.  --min_views M (default 0: off)
keeps a pixel only if at least M of the 2 R frames around its own (--view_radius R) see a depth within --view_tol of its own where
the pixel's point projects into them; the defaults of R and T are untuned as well.  With it the statistics gain invalid_views, and
the last line is the consistency rate, the kept pixels over the tested ones: a figure of a checkpoint that needs no ground truth.
The work is tripled_amd.cloud.SceneFuser (csrc/td_cloud.hip and csrc/td_views.hip on a HIP device); without --min_views the last
line printed is the statistics.  --save_poses FILE writes the camera-to-world poses that were fused (the model's own, or --poses')
in KITTI pose text: what scripts/render_cloud.py needs to look at the cloud from where the frames were taken.
--tsdf fuses truncated signed distances instead of averaging points per voxel (tripled_amd.tsdf.TsdfFuser, csrc/td_tsdf.hip): every
pixel adds its signed distance to the voxels its ray meets within --trunc_voxels voxels of its surface, and the PLY holds one point
per voxel edge on which the averaged distance changes sign, between voxels of at least --min_weight samples (both untuned starting
values), with nx ny nz after count: unit normals that face where the surface was seen from, so render_cloud.py --surfels and
eval_cloud.py use them as they are.  count holds the edge's weight.  --min_count does not apply; --min_views composes through the
per-pixel mask.  Without --tsdf nothing of this runs and the output is what it always was.  --save_map FILE (with --tsdf) also writes
the fused voxel map itself (tripled_amd.tsdf.save_map: one .npz of keys, integer rows, voxel and band), which
scripts/render_cloud.py --map ray-casts into depth, normal and colour images.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from mmcv import Config  # noqa: E402
from mono.datasets.kitti_dataset import KITTIOdomDataset, odom_sequence_files  # noqa: E402
from mono.model import MONO  # noqa: E402
from tripled_amd import cloud, odometry, tsdf  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data_path", required=True, help="KITTI odometry root (sequences/, poses/)")
    ap.add_argument("--sequence", type=int, default=9)
    ap.add_argument("--frames", default=None, help="A:B, the frames A ... B-1 of the sequence (default: all)")
    ap.add_argument("--poses", default=None, help="camera-to-world poses in KITTI pose text instead of the model's own")
    ap.add_argument("--height", type=int, default=None, help="default: the config's")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--img_ext", default=".png")
    ap.add_argument("--voxel", type=float, default=cloud.DEFAULT_VOXEL)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--border", type=int, default=0)
    ap.add_argument("--min_depth", type=float, default=cloud.DEFAULT_MIN_DEPTH)
    ap.add_argument("--max_range", type=float, default=cloud.DEFAULT_MAX_RANGE)
    ap.add_argument("--edge", type=float, default=cloud.DEFAULT_EDGE)
    ap.add_argument("--min_count", type=int, default=1)
    ap.add_argument("--min_views", type=int, default=0, help="multi-view filter: neighbouring frames that must confirm a pixel (0: off)")
    ap.add_argument("--view_radius", type=int, default=cloud.DEFAULT_VIEW_RADIUS, help="frames on either side that are asked (untuned)")
    ap.add_argument("--view_tol", type=float, default=cloud.DEFAULT_VIEW_TOL, help="relative depth difference that still agrees (untuned)")
    ap.add_argument("--depth_scale", type=float, default=1.0)
    ap.add_argument("--pose_scale", type=float, default=1.0)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--post_process", action="store_true")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--save_poses", default=None, help="write the poses that were fused, in KITTI pose text")
    ap.add_argument("--tsdf", action="store_true", help="fuse truncated signed distances: surface points with oriented normals")
    ap.add_argument("--trunc_voxels", type=int, default=tsdf.DEFAULT_TRUNC_VOXELS, help="the band on either side of a surface, in voxels (untuned)")
    ap.add_argument("--min_weight", type=int, default=tsdf.DEFAULT_MIN_WEIGHT, help="samples a voxel needs to take part in the surface (untuned)")
    ap.add_argument("--save_map", default=None, help="with --tsdf: write the fused voxel map (.npz) for render_cloud.py --map")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.save_map and not args.tsdf:
        ap.error("--save_map writes the map of --tsdf")
    cfg = Config.fromfile(args.config)
    cfg.model["imgs_per_gpu"] = 1
    height, width = args.height or cfg.model["height"], args.width or cfg.model["width"]
    model = MONO.module_dict[cfg.model["name"]](cfg.model)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)      # executes nothing from the file
    model.load_state_dict(ckpt["state_dict"], strict=True)
    model.eval().to(args.device)
    poses = odometry.load_kitti_poses(args.poses) if args.poses else None
    n_frames = len(poses) if poses is not None else len(odometry.load_kitti_poses(
        os.path.join(args.data_path, "poses", "%02d.txt" % args.sequence)))
    frames = None
    if args.frames:
        a, _, b = args.frames.partition(":")
        frames = (int(a or 0), int(b or n_frames))
    dataset = KITTIOdomDataset(args.data_path, odom_sequence_files(args.sequence, n_frames), height, width, [0, 1], is_train=False,
                               img_ext=args.img_ext)
    shared = dict(voxel=args.voxel, batch_size=args.batch_size, precision=args.precision, stride=args.stride, border=args.border,
                  min_depth=args.min_depth, max_range=args.max_range, edge=args.edge, depth_scale=args.depth_scale,
                  pose_scale=args.pose_scale, post_process=args.post_process, min_views=args.min_views, view_radius=args.view_radius,
                  view_tol=args.view_tol)
    if args.tsdf:
        fuser = tsdf.TsdfFuser(model, height, width, args.device, trunc_voxels=args.trunc_voxels, min_weight=args.min_weight, **shared)
    else:
        fuser = cloud.SceneFuser(model, height, width, args.device, min_count=args.min_count, **shared)
    print("-> Fusing sequence %02d: frames %s of %d" % (args.sequence, "%d:%d" % frames if frames else "0:%d" % n_frames, n_frames))
    result = fuser.fuse(dataset, poses=poses, frames=frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.tsdf:
        cloud.save_ply(args.out, result.xyz, result.rgb, result.weight, normals=result.normal)
    else:
        cloud.save_ply(args.out, result.xyz, result.rgb, result.count)
    print("saved %d points to %s" % (len(result.xyz), args.out))
    if args.save_poses:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_poses)), exist_ok=True)
        odometry.save_kitti_poses(args.save_poses, fuser.poses)
        print("saved %d poses to %s" % (len(fuser.poses), args.save_poses))
    if args.save_map:
        os.makedirs(os.path.dirname(os.path.abspath(args.save_map)), exist_ok=True)
        tsdf.save_map(args.save_map, *fuser.map, args.voxel, args.trunc_voxels)
        print("saved %d voxels to %s" % (len(fuser.map[0]), args.save_map))
    print(" ".join("%s %d" % (k, v) for k, v in result.stats.items()))
    if args.min_views and not args.tsdf:
        kept, tested = result.stats["valid"], result.stats["valid"] + result.stats["invalid_views"]
        print("consistency rate %.4f (%d of %d tested pixels have %d views or more)" % (kept / max(tested, 1), kept, tested, args.min_views))


if __name__ == "__main__":
    main()
