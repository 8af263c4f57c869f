#!/usr/bin/env python3
"""Timing of the point-cloud fusion (tripled_amd.cloud, csrc/td_cloud.hip) on one GPU.

One chunk is a batch of B = 12 frames, at 192 x 640 and at 320 x 1024.  The depth maps are synthetic (a smooth field of 3 ... 33
units), the camera moves forward 0.8 units per frame with a slight yaw, the voxel is 0.2 units: a few points to a few hundred per
voxel.  Timed separately, with device events, median of ``--repeats`` after ``--warmup`` runs of the same shapes:
  keys        td_cloud_keys (reads 7 bytes and writes 16 per pixel; its fraction of the HBM bandwidth is bytes / time over 8.0 TB/s,
              the specification, and over 6.29 TB/s, a measured float4 copy)
  sort        torch.sort of the int64 keys
  table       td_cloud_heads, torch.cumsum, td_cloud_reduce_packed, with the voxel count known (no synchronisation inside)
  merge       merge_hip of the chunk's voxels into a running map built from ``--map_chunks`` earlier chunks of the same drive
  chunk       everything a chunk costs after the depth network: keys, table_hip, merge_hip, host clock around a synchronise
The multi-view filter (csrc/td_views.hip; ``--view_radius``, ``--view_tol``, ``--min_views``, which must be > 0 here), with the chunk's
own 12 frames as the window (every frame a centre, every frame a possible neighbour):
  views          td_cloud_views without keys: every pixel is tested and the votes are written (its upper bound)
  views_on_keys  td_cloud_views on the pairs td_cloud_keys wrote (fresh copies per run, made outside the timed window): pixels that
                 are invalid already are skipped, the others are tested, pixels with fewer than min_views votes lose their key
  chunk_views    the chunk with the filter on: keys, views on those keys, table_hip, merge_hip; ``chunk`` is the filter off, the
                 launches of a build without the filter
Alongside: the numpy statement's time for the same batch (keys_numpy + voxel_table_numpy, once), and the number of host
synchronisations per chunk, counted as the Tensor.item() calls of one chunk.  The network, the frame upload and the per-batch
permuted copy of the frames that DepthPredictor wants are not part of this benchmark.

  python tools/cloud_bench.py [--repeats 20] [--warmup 3] [--map_chunks 8] [--min_views 2] [--view_radius 2] [--view_tol 0.05]
                              [--json profiles/cloud/cloud_bench.json]
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
from tripled_amd import cloud  # noqa: E402

B = 12
VOXEL = 0.2
PARAMS = dict(depth_scale=1.0, pose_scale=1.0, inv_voxel=1.0 / VOXEL, stride=1, border=0, min_depth=0.5, max_range=40.0, edge=0.1)
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def chunk_inputs(index, H, W, device):
    """(depth, color, poses) of chunk ``index`` of the synthetic drive, on the device."""
    g = torch.Generator().manual_seed(index)
    coarse = 3.0 + 30.0 * torch.rand(B, 1, 6, 20, generator=g)
    depth = torch.nn.functional.interpolate(coarse, (H, W), mode="bilinear", align_corners=False)[:, 0].contiguous()
    color = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
    poses = np.zeros((B, 3, 4))
    for b in range(B):
        k = index * B + b
        yaw = 0.3 * np.sin(k / 40.0)
        poses[b, :, :3] = [[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]]
        poses[b, :, 3] = [2.0 * np.sin(k / 40.0), 0.0, 0.8 * k]
    return depth.to(device), color.to(device), torch.from_numpy(poses).to(device)


def intrinsics(H, W):
    return np.array([[0.58 * W, 0, 0.5 * W], [0, 1.92 * H, 0.5 * H], [0, 0, 1]], dtype=np.float64)


def inv_K(H, W):
    return np.linalg.inv(intrinsics(H, W))


def timed(fn, warmup, repeats, setup=None):
    """Median, minimum and maximum of ``repeats`` device-event timings of fn(*setup()), in microseconds; ``setup`` runs outside the
    timed window."""
    for _ in range(warmup):
        fn(*(setup() if setup else ()))
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        given = setup() if setup else ()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*given)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def count_items(fn):
    calls = [0]
    item = torch.Tensor.item

    def counting(self):
        calls[0] += 1
        return item(self)

    torch.Tensor.item = counting
    try:
        fn()
    finally:
        torch.Tensor.item = item
    return calls[0]


def wall_clock(fn, args):
    """Median, minimum and maximum of the host clock around fn() and a synchronise, in microseconds."""
    for _ in range(args.warmup):
        fn()
    wall = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": statistics.median(wall), "min_us": min(wall), "max_us": max(wall)}


def bench_size(H, W, device, args):
    ik = inv_K(H, W)
    vmap_keys = torch.zeros(0, dtype=torch.int64, device=device)
    vmap_sums = torch.zeros(0, 7, dtype=torch.int64, device=device)
    for index in range(args.map_chunks):
        key, payload = cloud.keys_hip(*chunk_inputs(index, H, W, device), ik, **PARAMS)
        vmap_keys, vmap_sums = cloud.merge_hip(vmap_keys, vmap_sums, *cloud.table_hip(key, payload))
    depth, color, poses = chunk_inputs(args.map_chunks, H, W, device)
    key, payload = cloud.keys_hip(depth, color, poses, ik, **PARAMS)
    sorted_keys, perm = torch.sort(key)
    seg = torch.cumsum(cloud.heads_hip(sorted_keys), 0)
    V = int(seg[-1].item())
    ckeys, csums = cloud.reduce_hip(sorted_keys, seg, perm, payload, V)
    n = B * H * W
    out = {"height": H, "width": W, "batch": B, "points": n, "valid_points": int((key != cloud.INVALID_KEY).sum().item()),
           "chunk_voxels": V, "map_voxels": int(vmap_keys.shape[0]), "map_chunks": args.map_chunks}

    def table():
        s = torch.cumsum(cloud.heads_hip(sorted_keys), 0)
        cloud.reduce_hip(sorted_keys, s, perm, payload, V)

    def chunk():
        k, p = cloud.keys_hip(depth, color, poses, ik, **PARAMS)
        cloud.merge_hip(vmap_keys, vmap_sums, *cloud.table_hip(k, p))

    K = intrinsics(H, W)
    view = dict(radius=args.view_radius, tol=args.view_tol, depth_scale=PARAMS["depth_scale"], pose_scale=PARAMS["pose_scale"],
                min_depth=PARAMS["min_depth"], max_range=PARAMS["max_range"])

    def views_on_keys(k, p):
        cloud.views_hip(depth, poses, ik, K, key=k, payload=p, min_views=args.min_views, votes=False, **view)

    def chunk_views():
        k, p = cloud.keys_hip(depth, color, poses, ik, **PARAMS)
        views_on_keys(k, p)
        cloud.merge_hip(vmap_keys, vmap_sums, *cloud.table_hip(k, p))

    out["keys"] = timed(lambda: cloud.keys_hip(depth, color, poses, ik, **PARAMS), args.warmup, args.repeats)
    out["views"] = timed(lambda: cloud.views_hip(depth, poses, ik, K, **view), args.warmup, args.repeats)
    out["views_on_keys"] = timed(views_on_keys, args.warmup, args.repeats, setup=lambda: (key.clone(), payload.clone()))
    counts = torch.zeros(2, dtype=torch.int64, device=device)
    cloud.views_hip(depth, poses, ik, K, key=key.clone(), payload=payload.clone(), min_views=args.min_views, stats=counts, votes=False, **view)
    out["views_tested"], out["views_dropped"] = (int(v) for v in counts.cpu())
    out["sort"] = timed(lambda: torch.sort(key), args.warmup, args.repeats)
    out["table"] = timed(table, args.warmup, args.repeats)
    out["merge"] = timed(lambda: cloud.merge_hip(vmap_keys, vmap_sums, ckeys, csums), args.warmup, args.repeats)
    out["chunk"] = wall_clock(chunk, args)
    out["host_syncs_per_chunk"] = count_items(chunk)
    out["chunk_views"] = wall_clock(chunk_views, args)
    out["host_syncs_per_chunk_views"] = count_items(chunk_views)
    rate = 23.0 * n / (out["keys"]["median_us"] * 1e-6)
    out["keys_bytes_per_s"] = rate
    out["keys_fraction_of_hbm_spec"], out["keys_fraction_of_measured_copy"] = rate / HBM_SPEC, rate / HBM_COPY
    d, c, p = depth.cpu().numpy(), color.cpu().numpy(), poses.cpu().numpy()
    t0 = time.perf_counter()
    hkey, hpayload, _ = cloud.keys_numpy(d, c, p, ik, **PARAMS)
    t1 = time.perf_counter()
    hkeys, hsums = cloud.voxel_table_numpy(hkey, hpayload)
    t2 = time.perf_counter()
    out["numpy_keys_s"], out["numpy_table_s"] = t1 - t0, t2 - t1
    out["device_equals_numpy"] = bool(np.array_equal(ckeys.cpu().numpy(), hkeys) and np.array_equal(csums.cpu().numpy(), hsums))
    t0 = time.perf_counter()
    hvotes = cloud.views_numpy(d, p, ik, K, **view)
    out["numpy_views_s"] = time.perf_counter() - t0
    out["views_equal_numpy"] = bool(np.array_equal(cloud.views_hip(depth, poses, ik, K, **view).cpu().numpy(), hvotes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--map_chunks", type=int, default=8)
    ap.add_argument("--min_views", type=int, default=2)
    ap.add_argument("--view_radius", type=int, default=cloud.DEFAULT_VIEW_RADIUS)
    ap.add_argument("--view_tol", type=float, default=cloud.DEFAULT_VIEW_TOL)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.min_views < 1:
        ap.error("--min_views: at least 1 (the chunk without the filter is timed as well)")
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "voxel": VOXEL, "repeats": args.repeats, "warmup": args.warmup,
           "min_views": args.min_views, "view_radius": args.view_radius, "view_tol": args.view_tol,
           "sizes": [bench_size(H, W, device, args) for H, W in ((192, 640), (320, 1024))]}
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
