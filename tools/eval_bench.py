#!/usr/bin/env python3
"""Timing of the KITTI depth evaluation (tripled_amd.evaluate) on one GPU.

  1. images/s of scripts/eval_depth.evaluate (one frame at a time, scored on the host in numpy): the yardstick;
  2. images/s of DepthEvaluator.evaluate over the same frames at batch 1 and 12, fp32 and bf16, with and without flip
     post-processing; wall clock around the whole call (its one copy to the host included), median over rounds;
  3. the scoring call alone (evaluate_disparity_hip: the 10 launches of td_eval_depth) in microseconds per batch, HIP events
     around ``--inner`` back-to-back calls, median over ``--rounds`` rounds, after a warm-up.
Model: cfg_kitti_tripleD (ResNet50 depth encoder), random weights, network 192 x 640.  Frames: synthetic, with sparse (about 5 %)
ground truth of the four KITTI sizes.  Nothing is tuned per side: both run what the product runs.

  python tools/eval_bench.py [--frames 48] [--rounds 20] [--inner 20] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import evaluate  # noqa: E402

H, W = 192, 640
SIZES = [(375, 1242), (370, 1226), (374, 1238), (376, 1241)]


class Frames(torch.utils.data.Dataset):
    """Validation samples as the KITTI dataset returns them: the frame at network size, float32, and 'gt_depth'."""

    def __init__(self, n, seed=0, density=0.05):
        g = np.random.default_rng(seed)
        y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        self.samples = []
        for i in range(n):
            img = np.stack([0.5 + 0.4 * np.sin(6.28 * (g.uniform(1, 4) * y + g.uniform(1, 4) * x)) + g.uniform(-0.1, 0.1, (H, W))
                            for _ in range(3)], 0)
            img = torch.from_numpy(np.clip(img, 0, 1).astype(np.float32))
            gh, gw = SIZES[i % len(SIZES)]
            gt = (1.0 + 78.0 * g.random((gh, gw))).astype(np.float32)
            gt[g.random((gh, gw)) >= density] = 0.0
            self.samples.append({("color", 0, 0): img, ("color_aug", 0, 0): img.clone(), "gt_depth": gt})

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return dict(self.samples[i])


def wall_s(fn, rounds):
    fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    return statistics.median(samples), min(samples)


def event_us(fn, rounds, inner):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / inner * 1e3)
    return statistics.median(samples), min(samples)


def path_rows(data, rounds):
    import eval_depth
    from mmcv import Config
    from mono.model import MONO
    dev = torch.device("cuda", 0)
    cfg = Config.fromfile(os.path.join(ROOT, "config", "cfg_kitti_tripleD.py"))
    cfg.model["imgs_per_gpu"] = 1
    torch.manual_seed(0)
    model = MONO.module_dict[cfg.model["name"]](cfg.model).to(dev).eval()
    n = len(data)
    rows = []
    s = wall_s(lambda: eval_depth.evaluate(model, data, False, dev), max(3, rounds // 4))
    rows.append(dict(path="eval_depth.evaluate loop (fp32, one frame at a time, numpy)", B=1, imgs_per_s=n / s[0], best_imgs_per_s=n / s[1]))
    for precision in ("fp32", "bf16"):
        for post in (False, True):
            for B in (1, 12):
                ev = evaluate.DepthEvaluator(model, dev, batch_size=B, precision=precision, post_process=post)
                s = wall_s(lambda: ev.evaluate(data), max(3, rounds // 4))
                rows.append(dict(path="DepthEvaluator %s%s" % (precision, " + flip post-processing" if post else ""), B=B,
                                 imgs_per_s=n / s[0], best_imgs_per_s=n / s[1]))
    return rows


def score_rows(data, rounds, inner):
    dev = torch.device("cuda", 0)
    rows = []
    for B in (1, 12):
        gt, sizes, crops = evaluate.pad_ground_truth([data[i]["gt_depth"] for i in range(B)], dev)
        ws = evaluate.eval_workspace(B, gt.shape[1], gt.shape[2], dev)
        for dtype in (torch.float32, torch.bfloat16):
            disp = torch.rand(B, H, W, device=dev).to(dtype)
            us = event_us(lambda: evaluate.evaluate_disparity_hip(disp, gt, sizes, crops, workspace=ws), rounds, inner)
            rows.append(dict(B=B, dtype=str(dtype).replace("torch.", ""), us_per_batch=us[0], min_us_per_batch=us[1]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--score-only", action="store_true")
    args = ap.parse_args()
    data = Frames(args.frames)
    scores = score_rows(data, args.rounds, args.inner)
    print("%-28s %3s %10s %14s" % ("scoring call (td_eval_depth)", "B", "disparity", "us per batch"))
    for r in scores:
        print("%-28s %3d %10s %14.1f" % ("", r["B"], r["dtype"], r["us_per_batch"]))
    paths = [] if args.score_only else path_rows(data, args.rounds)
    if paths:
        print("\n%-62s %3s %10s" % ("path (%d frames)" % args.frames, "B", "imgs/s"))
        for r in paths:
            print("%-62s %3d %10.1f" % (r["path"], r["B"], r["imgs_per_s"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(score=scores, paths=paths, frames=args.frames, rounds=args.rounds, inner=args.inner), f, indent=1)


if __name__ == "__main__":
    main()
