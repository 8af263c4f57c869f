#!/usr/bin/env python3
"""Timing of the point renderer (tripled_amd.render, csrc/td_render.hip) on one GPU.

The cloud is SYNTHETIC: about 3 million points on the voxel lattice of a corridor (a ground plane 1.2 wide and two walls 0.4 high,
37.5 long, in the model's units; voxel 0.005), coloured at random, in random order.  No real cloud has been rendered: a fused
sequence has holes, clutter and a voxel order (ascending keys) that this one does not.  Twelve cameras stand along the corridor and
look down it with the KITTI intrinsics of the datasets; near 0.1, far 4.0.  Cases: 192 x 640 and 320 x 1024, splat 0 (one pixel per
point) and splat = the voxel size.  Timed per case:
  chain     render_hip: the launch chain of td_cloud_render (two fills, scatter, resolve) with the cloud already on the device,
            device events, median of ``--repeats`` after ``--warmup`` calls, in microseconds per batch of 12 views
  numpy     render_numpy on the same input, seconds, once (``--numpy_cameras N`` cuts the input down to the first N cameras, and the
            output says so; 0 skips the statement)
Alongside: whether the device maps equal the statement's bit for bit, the stats summed over the views, the share
of pixels hit, and the host synchronisations of one chain call counted as Tensor.item / .tolist / .cpu calls.

  python tools/render_bench.py [--repeats 50] [--warmup 5] [--json profiles/render/render_bench_v1.json] [--txt ....txt]
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
from tripled_amd import render  # noqa: E402

VOXEL, NEAR, FAR, CAMERAS = 0.005, 0.1, 4.0, 12
LENGTH, HALF_WIDTH, WALL, CAMERA_HEIGHT = 37.5, 0.6, 0.4, 0.045
SIZES = ((192, 640), (320, 1024))


def make_cloud(seed=0):
    """The corridor's voxel centres: x right, y down (the ground at y = CAMERA_HEIGHT below the cameras), z forward."""
    g = np.random.default_rng(seed)
    zs = (np.arange(int(LENGTH / VOXEL)) + 0.5) * VOXEL
    xs = (np.arange(int(2 * HALF_WIDTH / VOXEL)) + 0.5) * VOXEL - HALF_WIDTH
    ys = CAMERA_HEIGHT - (np.arange(int(WALL / VOXEL)) + 0.5) * VOXEL
    ground = np.stack(np.broadcast_arrays(xs[None, :], CAMERA_HEIGHT, zs[:, None]), -1).reshape(-1, 3)
    walls = [np.stack(np.broadcast_arrays(side * HALF_WIDTH, ys[None, :], zs[:, None]), -1).reshape(-1, 3) for side in (-1.0, 1.0)]
    xyz = np.concatenate([ground] + walls, 0).astype(np.float32)
    xyz = xyz[g.permutation(len(xyz))]
    return xyz, g.integers(0, 256, (len(xyz), 3)).astype(np.uint8)


def make_cameras():
    poses = np.zeros((CAMERAS, 3, 4))
    for c in range(CAMERAS):
        a = 0.05 * (c % 3 - 1)
        poses[c, :, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        poses[c, :, 3] = [0.1 * (c % 2) - 0.05, 0.0, (LENGTH - FAR) * c / CAMERAS]
    return poses


def kitti_K(H, W):
    return np.array([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]])


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
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy_cameras", type=int, default=CAMERAS, help="cameras the numpy statement draws (fewer: a cut-down input; 0: skip it)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "render", "render_bench_v1.json"))
    ap.add_argument("--txt", default=None, help="default: --json with .txt")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    xyz, rgb = make_cloud()
    poses = make_cameras()
    xyz_d, rgb_d, poses_d = (torch.from_numpy(a).to(device) for a in (xyz, rgb, poses))
    out = {"device": torch.cuda.get_device_name(0), "points": len(xyz), "cameras": CAMERAS, "synthetic_cloud": True, "voxel": VOXEL,
           "near": NEAR, "far": FAR, "repeats": args.repeats, "warmup": args.warmup, "numpy_cameras": args.numpy_cameras, "cases": []}
    lines = ["%s, %d points (synthetic corridor), %d cameras, median of %d runs after %d" % (
        out["device"], len(xyz), CAMERAS, args.repeats, args.warmup)]
    for H, W in SIZES:
        K = kitti_K(H, W)
        workspace = render.render_workspace(CAMERAS, H, W, device)
        for splat in (0.0, VOXEL):
            def chain():
                return render.render_hip(xyz_d, rgb_d, poses_d, K, H, W, near=NEAR, far=FAR, splat=splat, workspace=workspace)

            case = {"height": H, "width": W, "splat": splat, "workspace_bytes": int(workspace.numel())}
            case["chain"] = timed(chain, args.warmup, args.repeats)
            got = chain()
            stats = got.stats.cpu().numpy()
            case["stats_total"] = dict(zip(render.STATS, (int(v) for v in stats.sum(0))))
            case["share_hit"] = float(stats[:, 4].sum()) / (CAMERAS * H * W)
            case["projections_per_s"] = CAMERAS * len(xyz) / (case["chain"]["median_us"] * 1e-6)
            case["host_syncs_chain"] = count_syncs(chain)
            n = min(args.numpy_cameras, CAMERAS)
            if n:
                t0 = time.perf_counter()
                want = render.render_numpy(xyz, rgb, poses[:n], K, H, W, near=NEAR, far=FAR, splat=splat)
                case["numpy_s"] = time.perf_counter() - t0
                case["numpy_input"] = "the same input" if n >= CAMERAS else "cut down: the first %d of %d cameras" % (n, CAMERAS)
                case["device_equals_numpy"] = bool(all(
                    np.array_equal(a[:n].cpu().numpy().view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(got, want)))
            out["cases"].append(case)
            lines.append("%4d x %4d splat %-6g chain %9.1f us (min %.1f, max %.1f)  %.2e projections/s  hit %.3f  syncs %d%s" % (
                H, W, splat, case["chain"]["median_us"], case["chain"]["min_us"], case["chain"]["max_us"], case["projections_per_s"],
                case["share_hit"], case["host_syncs_chain"],
                "  numpy (%d cameras) %.2f s  equal %s" % (n, case["numpy_s"], case["device_equals_numpy"]) if n else ""))
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")
    with open(args.txt or os.path.splitext(args.json)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
