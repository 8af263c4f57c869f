#!/usr/bin/env python3
"""Timing of the velodyne ground truth (tripled_amd.velodyne, csrc/td_velo.hip) on one GPU.

One batch is B = 12 SYNTHETIC scans of KITTI size: about 120 000 points each, projected into 375 x 1242 maps through a synthetic
calibration (tests/velo_util.py).  No real scan has been run: a real scan's points follow the sensor's 64 rings, these are drawn per
pixel, so the number of duplicates and the locality of the scatter differ.  Timed:
  chain       depth_maps_hip: the launch chain of td_velo_depth (two fills, scatter, resolve) with the points already on the
              device, device events, median of ``--repeats`` after ``--warmup`` calls, in microseconds per batch; and the bytes it
              must move (the points once, the tables cleared, written and read, the maps written) over that time
  batch       batch_ground_truth: concatenate on the host, ONE upload, the chain; host clock around a synchronise
  numpy       depth_map_numpy over the same 12 scans, seconds
  bruteforce  depth_map_bruteforce over ``--bruteforce_frames`` of them (default 1), seconds per frame
Alongside: the host synchronisations of one chain call and of one batch call, counted as Tensor.item / .tolist / .cpu calls, and
whether the device maps equal the statement's bit for bit.  Per-kernel times come from a kernel trace of a run with --chain_only
(a profiler slows the host: the figures above are taken without it).

  python tools/velo_bench.py [--repeats 200] [--warmup 20] [--json profiles/velo/velo_bench.json] [--chain_only]
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
from tests import velo_util  # noqa: E402
from tripled_amd import velodyne  # noqa: E402

B, H, W, POINTS = 12, 375, 1242, 120000
HBM_SPEC = 8.0e12


def make_batch():
    calib = velo_util.synthetic_calibration(H, W, 21)
    scans = [velo_util.synthetic_scan(calib, POINTS + 997 * (i % 3), 100 + i) for i in range(B)]
    Ps = [velo_util.projection(calib, 2 + i % 2) for i in range(B)]
    return scans, Ps, [(H, W)] * B


def timed(fn, warmup, repeats):
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


def count_syncs(fn):
    """Calls of Tensor.item / .tolist / .cpu during fn(): each waits for the device."""
    calls = [0]
    saved = {name: getattr(torch.Tensor, name) for name in ("item", "tolist", "cpu")}

    def counting(name):
        def wrapper(self, *a, **k):
            calls[0] += 1
            return saved[name](self, *a, **k)
        return wrapper

    for name in saved:
        setattr(torch.Tensor, name, counting(name))
    try:
        fn()
    finally:
        for name, f in saved.items():
            setattr(torch.Tensor, name, f)
    return calls[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bruteforce_frames", type=int, default=1)
    ap.add_argument("--chain_only", action="store_true", help="only the chain, for a kernel trace")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    scans, Ps, sizes = make_batch()
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum([len(s) for s in scans], out=offsets[1:])
    points_d = torch.from_numpy(np.concatenate(scans, 0)).to(device)
    offsets_d, P_d = torch.from_numpy(offsets).to(device), torch.from_numpy(np.stack(Ps, 0)).to(device)
    sizes_d = torch.tensor(sizes, dtype=torch.int32, device=device)
    workspace = velodyne.velo_workspace(B, H, W, device)

    def chain():
        return velodyne.depth_maps_hip(points_d, offsets_d, P_d, sizes_d, workspace=workspace, max_size=(H, W))

    out = {"device": torch.cuda.get_device_name(0), "batch": B, "height": H, "width": W, "points": int(offsets[-1]),
           "synthetic_scans": True, "repeats": args.repeats, "warmup": args.warmup, "workspace_bytes": int(workspace.numel())}
    out["chain"] = timed(chain, args.warmup, args.repeats)
    if not args.chain_only:
        # bytes the chain cannot avoid: the points read once, the tables filled and read once, the maps written; the atomics'
        # read-modify-write traffic (four 8-byte entries per valid point) is counted once as well
        gt, stats = chain()
        stats = stats.cpu().numpy()
        valid = int(stats[:, 3].sum())
        moved = 16 * int(offsets[-1]) + 2 * int(workspace.numel()) + 4 * B * H * W + 4 * 8 * valid
        out["chain_bytes"] = moved
        out["chain_bytes_per_s"] = moved / (out["chain"]["median_us"] * 1e-6)
        out["chain_fraction_of_hbm_spec"] = out["chain_bytes_per_s"] / HBM_SPEC
        out["stats_total"] = dict(zip(velodyne.STATS, (int(v) for v in stats.sum(0))))
        out["host_syncs_chain"] = count_syncs(chain)

        def batch():
            return velodyne.batch_ground_truth(scans, Ps, sizes, device, workspace=workspace)

        for _ in range(3):
            batch()
        wall = []
        for _ in range(max(5, args.repeats // 10)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
        out["batch"] = {"median_us": statistics.median(wall), "min_us": min(wall), "max_us": max(wall)}
        out["host_syncs_batch"] = count_syncs(batch)
        t0 = time.perf_counter()
        host = [velodyne.depth_map_numpy(s, p, H, W)[0] for s, p in zip(scans, Ps)]
        out["numpy_s"] = time.perf_counter() - t0
        gt = gt.cpu().numpy()
        out["device_equals_numpy"] = bool(all(np.array_equal(gt[i].view(np.uint32), host[i].astype(np.float32).view(np.uint32)) for i in range(B)))
        t0 = time.perf_counter()
        for i in range(args.bruteforce_frames):
            brute = velodyne.depth_map_bruteforce(scans[i], Ps[i], H, W)[0]
            out["bruteforce_equals_numpy"] = bool(np.array_equal(brute, host[i]))
        out["bruteforce_s_per_frame"] = (time.perf_counter() - t0) / max(args.bruteforce_frames, 1)
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
