#!/usr/bin/env python3
"""Offline KITTI odometry evaluation (reference: scripts/eval_pose.py, scripts/draw_odometry.py and
mono/tools/kitti_evaluation_toolkit.py): load a checkpoint, predict the relative pose of every consecutive frame pair of a
sequence, and print the 5-frame snippet ATE and the KITTI translational / rotational errors over 100 ... 800 m segments.

  python scripts/eval_pose.py --config config/cfg_kitti_tripleD.py --checkpoint work/epoch_20.pth --data_path /data/kitti_odom \
         [--sequences 9 10] [--height 192 --width 640] [--batch_size 12] [--precision bf16] [--device cpu] [--result_dir DIR]

Frames: <data_path>/sequences/NN/image_0/%06d.png; ground truth: <data_path>/poses/NN.txt (or --gt_dir/NN.txt), whose line count
is the sequence's frame count.  --split_file lists the frame pairs explicitly ("<seq> <i> l" per line) for a single sequence.
With --result_dir: NN_pred.txt (KITTI pose text, %1.8e), NN_eval/NN_error.txt (first_frame r_err t_err len speed) and
NN_eval/NN_stats.txt, and NN_relative.npy: the float32 [n,4,4] relative transforms, which OdometryEvaluator.evaluate(relative=...)
scores again without running the network.  No plots.  The work is tripled_amd.odometry.OdometryEvaluator (csrc/td_odom.hip on a HIP device).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tripled_amd  # noqa: F401,E402
from mmcv import Config  # noqa: E402
from mono.datasets.kitti_dataset import KITTIOdomDataset, odom_sequence_files  # noqa: E402
from mono.model import MONO  # noqa: E402
from tripled_amd import odometry  # noqa: E402


def write_results(result_dir, seq, result):
    os.makedirs(os.path.join(result_dir, "%02d_eval" % seq), exist_ok=True)
    odometry.save_kitti_poses(os.path.join(result_dir, "%02d_pred.txt" % seq), result.poses)
    np.save(os.path.join(result_dir, "%02d_relative.npy" % seq), result.relative.cpu().numpy())
    with open(os.path.join(result_dir, "%02d_eval" % seq, "%02d_error.txt" % seq), "w") as f:
        for first, r_err, t_err, length, speed in result.segments:
            f.write("%d %s %s %d %s\n" % (int(first), repr(float(r_err)), repr(float(t_err)), int(length), repr(float(speed))))
    with open(os.path.join(result_dir, "%02d_eval" % seq, "%02d_stats.txt" % seq), "w") as f:
        f.write("Average sequence translation RMSE (%):    {0:.4f}\n".format(result.t_err * 100))
        f.write("Average sequence rotation error (deg/m):  {0:.4f}".format(result.r_err / np.pi * 180))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data_path", required=True, help="KITTI odometry root (sequences/, poses/)")
    ap.add_argument("--gt_dir", default=None, help="directory of NN.txt ground-truth poses (default: <data_path>/poses)")
    ap.add_argument("--sequences", type=int, nargs="+", default=[9, 10])
    ap.add_argument("--split_file", default=None, help="frame-pair lines of ONE sequence instead of all its consecutive pairs")
    ap.add_argument("--height", type=int, default=None, help="default: the config's")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--img_ext", default=".png")
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--result_dir", default=None)
    args = ap.parse_args()
    if args.split_file and len(args.sequences) != 1:
        ap.error("--split_file names the pairs of one sequence: give exactly one --sequences id")
    cfg = Config.fromfile(args.config)
    cfg.model["imgs_per_gpu"] = 1
    height, width = args.height or cfg.model["height"], args.width or cfg.model["width"]
    model = MONO.module_dict[cfg.model["name"]](cfg.model)
    ckpt = torch.load(args.checkpoint, map_location="cpu", weights_only=True)      # executes nothing from the file
    model.load_state_dict(ckpt["state_dict"], strict=True)
    model.eval().to(args.device)
    evaluator = odometry.OdometryEvaluator(model, args.device, batch_size=args.batch_size, precision=args.precision)
    for seq in args.sequences:
        gt = odometry.load_kitti_poses(os.path.join(args.gt_dir or os.path.join(args.data_path, "poses"), "%02d.txt" % seq))
        if args.split_file:
            with open(args.split_file) as f:
                files = f.read().splitlines()
        else:
            files = odom_sequence_files(seq, len(gt))
        dataset = KITTIOdomDataset(args.data_path, files, height, width, [0, 1], is_train=False, img_ext=args.img_ext)
        print("-> Computing pose predictions: sequence %02d, %d frame pairs" % (seq, len(dataset)))
        result = evaluator.evaluate(dataset, gt[:len(dataset) + 1])
        print("\n  odom_{} Trajectory error: {:0.3f}, std: {:0.3f}\n".format(seq, result.ate_mean, result.ate_std))
        print("Sequence: %02d" % seq)
        print("Distance (m): %d" % result.distance)
        print("Scale of the alignment: {0:.6f}".format(result.scale))
        print("Average sequence translational RMSE (%):   {0:.4f}".format(result.t_err * 100))
        print("Average sequence rotational error (deg/m): {0:.4f}\n".format(result.r_err / np.pi * 180))
        if args.result_dir:
            write_results(args.result_dir, seq, result)
            print("saving into ", args.result_dir)


if __name__ == "__main__":
    main()
