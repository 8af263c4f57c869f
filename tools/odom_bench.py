#!/usr/bin/env python3
"""Timing of the KITTI odometry evaluation (tripled_amd.odometry) on one GPU.

A synthetic sequence of ``--frames`` frames (default 1 591, sequence 09's count) at 192 x 640 is scored two ways with the same
model (cfg_kitti_fm, random weights) on the same device:
  1. OdometryEvaluator.evaluate: every frame uploaded once as uint8, pairs by td_pose_pairs_u8, batches of ``--batch_size``,
     td_pose_fwd, the three metric kernels, one copy to the host;
  2. the followed project's procedure on the same classes: batch 1, both frames of every pair converted and uploaded per sample,
     one 4x4 copied to the host per pair, then the numpy statements (np.linalg.inv / np.dot loops) for the trajectory, the snippet
     ATEs and the segment errors.
Frames are held decoded in memory on both sides (PNG decoding is the same work for both and is left out).  Wall clock around the
whole call, median over ``--rounds`` rounds after a warm-up round; the parts of (2) are reported separately.

  python tools/odom_bench.py [--frames 1591] [--batch_size 12] [--rounds 3] [--json profiles/odom/odom_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import odometry  # noqa: E402

H, W = 192, 640


class Frames:
    """n_frames decoded frames; len() = n_frames - 1 pairs; frame_u8 as mono.datasets.KITTIOdomDataset."""

    def __init__(self, n_frames, seed=0):
        g = torch.Generator().manual_seed(seed)
        base = torch.randint(0, 256, (3, H, W + 2 * n_frames), generator=g, dtype=torch.uint8)
        self.frames = [base[:, :, 2 * i:2 * i + W].contiguous() for i in range(n_frames)]

    def __len__(self):
        return len(self.frames) - 1

    def frame_u8(self, index, offset=0):
        return self.frames[index + offset]


def ground_truth(n_frames, seed=1):
    g = np.random.default_rng(seed)
    rel = np.tile(np.eye(4), (n_frames - 1, 1, 1))
    yaw = 0.01 * np.sin(np.arange(n_frames - 1) / 40.0) + g.normal(0, 1e-3, n_frames - 1)
    rel[:, 0, 0], rel[:, 0, 2], rel[:, 2, 0], rel[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
    rel[:, :3, 3] = np.array([0.0, 0.0, -1.07]) + g.normal(0, 0.02, (n_frames - 1, 3))
    return odometry.trajectory_numpy(rel)


def reference_way(model, dataset, gt, device):
    """(seconds in the network loop, seconds in the numpy metrics, result tuple)."""
    t0 = time.perf_counter()
    rel = []
    with torch.no_grad():
        for i in range(len(dataset)):
            a = (dataset.frame_u8(i, 0).float() / 255.0).unsqueeze(0).to(device)
            b = (dataset.frame_u8(i, 1).float() / 255.0).unsqueeze(0).to(device)
            axisangle, translation = model.PoseDecoder(model.PoseEncoder(torch.cat([a, b], 1)))
            rel.append(model.transformation_from_parameters(axisangle[:, 0], translation[:, 0]).cpu().numpy())
    rel = np.concatenate(rel)
    t1 = time.perf_counter()
    poses = odometry.trajectory_numpy(rel)
    ates = odometry.snippet_ates_numpy(rel, gt)
    rows, scale, _ = odometry.sequence_errors_numpy(gt, poses)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, (float(np.mean(ates)), odometry.overall_errors(rows), scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1591)
    ap.add_argument("--batch_size", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from mmcv import Config
    from mono.model import MONO
    cfg = Config.fromfile(os.path.join(ROOT, "config", "cfg_kitti_fm.py"))
    cfg.model.update(imgs_per_gpu=1)
    torch.manual_seed(0)
    device = torch.device("cuda", 0)
    model = MONO.module_dict[cfg.model["name"]](cfg.model).to(device).eval()
    dataset, gt = Frames(args.frames), ground_truth(args.frames)
    out = {"frames": args.frames, "height": H, "width": W, "batch_size": args.batch_size, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0)}
    for precision in ("fp32", "bf16"):
        ev = odometry.OdometryEvaluator(model, device, batch_size=args.batch_size, precision=precision)
        times = []
        for r in range(args.rounds + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = ev.evaluate(dataset, gt)
            times.append(time.perf_counter() - t0)
        out["evaluator_%s_s" % precision] = statistics.median(times[1:])
        out["evaluator_%s_ate_mean" % precision] = res.ate_mean
        rel = res.relative
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate(dataset, gt, relative=rel)
        out["metrics_on_device_%s_s" % precision] = time.perf_counter() - t0      # three launches + the one copy
    net, host = [], []
    for r in range(max(1, args.rounds // 2) + 1):
        a, b, _ = reference_way(model, dataset, gt, device)
        net.append(a)
        host.append(b)
    out["reference_way_network_loop_s"] = statistics.median(net[1:])
    out["reference_way_numpy_metrics_s"] = statistics.median(host[1:])
    out["reference_way_s"] = out["reference_way_network_loop_s"] + out["reference_way_numpy_metrics_s"]
    out["speedup_fp32"] = out["reference_way_s"] / out["evaluator_fp32_s"]
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
