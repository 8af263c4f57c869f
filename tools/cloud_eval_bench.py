#!/usr/bin/env python3
"""Timing of the cloud evaluation (tripled_amd.cloud_eval, csrc/td_scan.hip, csrc/td_nn.hip) on one GPU.

Two SYNTHETIC clouds of about 3 M points each, laid out like voxel-averaged clouds of a street: a ground strip of ``--length`` x 40
units and two walls of ``--length`` x 10 units, one point per 0.2 x 0.2 patch (the voxel), jittered by up to a quarter voxel.  The
predicted cloud is the same street sampled half a voxel over, with 0.1 units of noise along the surface normals.  tau = 0.6 (three
voxels), thresholds tau/4, tau/2, tau.  Both clouds are in key order along the street, as a fused cloud is.  The scans: 12 scans of
120 000 points around the sensor, fused with a view test at 192 x 640.
Timed separately, with device events, median of ``--repeats`` after ``--warmup`` runs of the same shapes:
  scan_keys      td_scan_keys on the 12 scans (reads 16 bytes and writes 16 per point)
  grid_ref       grid_hip of the reference: product, floor, torch.sort, td_cloud_heads, nonzero / cumsum plumbing, two gathers; host
                 clock around a synchronise, because it synchronises once itself
  query_pred     td_nn_query, the predicted points into the reference's grid
  query_ref      td_nn_query, the reference points into the predicted cloud's grid
  query_shuffled query_pred with the queries in random order: what the coherence of neighbouring threads' walks is worth
  compare        CloudComparer.compare end to end (two grids, two queries, two means), host clock
Alongside: nearest_numpy on a stated random subsample of the predicted points against the whole reference (the full statement is
too slow to time in whole), its time per query, and ``device_equals_numpy`` on that subsample (the bits of d2, the indices);
scan_keys_numpy's time for the same scans and whether the device's pairs equal it.

  python tools/cloud_eval_bench.py [--repeats 20] [--warmup 3] [--length 2000] [--subsample 20000] [--json profiles/cloud_eval/cloud_eval_bench.json]
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
from tripled_amd import cloud_eval  # noqa: E402

VOXEL, TAU = 0.2, 0.6
SCANS, SCAN_POINTS, H, W = 12, 120000, 192, 640
TR = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]])
K = np.array([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]])


def street(length, seed, shift, noise):
    """float64 [n,3]: x along the street (the key's major axis), the ground at y = 0, walls at z = -20 and z = 20."""
    rng = np.random.default_rng(seed)
    nx = int(round(length / VOXEL))
    parts = []
    for width, fixed_axis, fixed in ((40.0, 1, 0.0), (10.0, 2, -20.0), (10.0, 2, 20.0)):
        a, b = np.meshgrid(np.arange(nx) * VOXEL + shift, np.arange(int(round(width / VOXEL))) * VOXEL + shift, indexing="ij")
        p = np.zeros((a.size, 3))
        p[:, 0] = a.reshape(-1)
        p[:, 3 - fixed_axis] = b.reshape(-1) - (20.0 if fixed_axis == 1 else 0.0)      # the ground spans z = -20 ... 20, a wall y = 0 ... 10
        p += rng.uniform(-0.25 * VOXEL, 0.25 * VOXEL, p.shape)
        p[:, fixed_axis] = fixed + (rng.normal(0, noise, a.size) if noise else 0.0)
        parts.append(p)
    p = np.concatenate(parts)
    return p[np.argsort(np.floor(p[:, 0] / VOXEL), kind="stable")]                         # key order along the street


def scans(seed):
    rng = np.random.default_rng(seed)
    pts = np.empty((SCANS * SCAN_POINTS, 4), np.float32)
    pts[:, 0], pts[:, 1] = rng.uniform(-60, 60, len(pts)), rng.uniform(-30, 30, len(pts))
    pts[:, 2], pts[:, 3] = rng.uniform(-2, 2, len(pts)), rng.uniform(0, 1, len(pts))
    poses = np.zeros((SCANS, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[:, 2, 3] = 0.8 * np.arange(SCANS)
    return pts, np.arange(SCANS + 1, dtype=np.int64) * SCAN_POINTS, poses


def timed(fn, warmup, repeats):
    """Median, minimum and maximum of ``repeats`` device-event timings of fn(), in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def wall_clock(fn, warmup, repeats):
    """Median, minimum and maximum of the host clock around fn() and a synchronise, in microseconds."""
    for _ in range(warmup):
        fn()
    wall = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": statistics.median(wall), "min_us": min(wall), "max_us": max(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--length", type=float, default=2000.0)
    ap.add_argument("--subsample", type=int, default=20000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "voxel": VOXEL, "tau": TAU, "repeats": args.repeats, "warmup": args.warmup,
           "length": args.length}
    # scans
    pts, offsets, poses = scans(0)
    camera = dict(K=K, height=H, width=W, min_depth=1.0, max_range=60.0, inv_voxel=1.0 / VOXEL)
    pts_d, off_d, poses_d = (torch.from_numpy(a).to(device) for a in (pts, offsets, poses))
    stats = torch.zeros(5, dtype=torch.int64, device=device)
    key, payload = cloud_eval.scan_keys_hip(pts_d, off_d, TR, poses_d, stats=stats, **camera)
    out["scan_points"], out["scan_counts"] = len(pts), dict(zip(cloud_eval.SCAN_CAUSES, (int(v) for v in stats.cpu())))
    out["scan_keys"] = timed(lambda: cloud_eval.scan_keys_hip(pts_d, off_d, TR, poses_d, **camera), args.warmup, args.repeats)
    out["scan_keys_bytes_per_s"] = 32.0 * len(pts) / (out["scan_keys"]["median_us"] * 1e-6)
    t0 = time.perf_counter()
    hkey, hpayload, hcounts = cloud_eval.scan_keys_numpy(pts, offsets, TR, poses, **camera)
    out["numpy_scan_keys_s"] = time.perf_counter() - t0
    out["scan_keys_equal_numpy"] = bool(np.array_equal(key.cpu().numpy(), hkey) and np.array_equal(stats.cpu().numpy(), hcounts) and
                                        np.array_equal(payload.cpu().numpy().view(np.uint64), hpayload))
    # clouds
    ref, pred = street(args.length, 1, 0.0, 0.0), street(args.length, 2, 0.5 * VOXEL, 0.1)
    ref_d, pred_d = torch.from_numpy(ref).to(device), torch.from_numpy(pred).to(device)
    ref_grid, pred_grid = cloud_eval.grid_hip(ref_d, TAU), cloud_eval.grid_hip(pred_d, TAU)
    out["ref"], out["pred"] = ref_grid.stats, pred_grid.stats
    shuffled = pred_d[torch.randperm(len(pred_d), device=device)].contiguous()
    out["grid_ref"] = wall_clock(lambda: cloud_eval.grid_hip(ref_d, TAU), args.warmup, args.repeats)
    out["query_pred"] = timed(lambda: cloud_eval.nearest_hip(pred_d, ref_grid, TAU), args.warmup, args.repeats)
    out["query_ref"] = timed(lambda: cloud_eval.nearest_hip(ref_d, pred_grid, TAU), args.warmup, args.repeats)
    out["query_shuffled"] = timed(lambda: cloud_eval.nearest_hip(shuffled, ref_grid, TAU), args.warmup, args.repeats)
    comparer = cloud_eval.CloudComparer(device, TAU)
    out["compare"] = wall_clock(lambda: comparer.compare(pred_d, ref_d), args.warmup, args.repeats)
    result = comparer.compare(pred_d, ref_d)
    out["scores"] = {"thresholds": result.thresholds, "precision": result.precision, "recall": result.recall, "fscore": result.fscore,
                     "accuracy": result.accuracy, "completeness": result.completeness}
    # the statement on a subsample of the queries, against the whole reference
    pick = np.sort(np.random.default_rng(3).choice(len(pred), min(args.subsample, len(pred)), replace=False))
    t0 = time.perf_counter()
    host_grid = cloud_eval.grid_numpy(ref, TAU)
    t1 = time.perf_counter()
    want = cloud_eval.nearest_numpy(pred[pick], host_grid, TAU)
    t2 = time.perf_counter()
    got = cloud_eval.nearest_hip(pred_d[torch.from_numpy(pick).to(device)].contiguous(), ref_grid, TAU)
    out["subsample"], out["numpy_grid_s"], out["numpy_nearest_subsample_s"] = len(pick), t1 - t0, t2 - t1
    out["numpy_nearest_us_per_query"] = (t2 - t1) * 1e6 / len(pick)
    out["device_equals_numpy"] = bool(np.array_equal(got.d2.cpu().numpy().view(np.uint64), want.d2.view(np.uint64)) and
                                      np.array_equal(got.index.cpu().numpy(), want.index) and
                                      np.array_equal(got.counts.cpu().numpy(), want.counts))
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
