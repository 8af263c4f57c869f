#!/usr/bin/env python3
"""Timing of the truncated signed distance fusion (tripled_amd.tsdf, csrc/td_tsdf.hip) on one GPU, beside the voxel-averaging chain
(tripled_amd.cloud) in the same run.

The chunk, the synthetic drive, the voxel and the single-frame filters are those of tools/cloud_bench.py: B = 12 frames at 192 x 640 and
at 320 x 1024, voxel 0.2; the band is T = 3 voxels, so a chunk makes 13 pairs per pixel.  Timed separately, with device events, median
of ``--repeats`` after ``--warmup`` runs of the same shapes:
  samples     td_tsdf_samples (reads 7 bytes and writes 16 (4T+1) per pixel; its fraction of the HBM bandwidth as in cloud_bench.py)
  sort        torch.sort of the int64 keys of all (4T+1) B H W pairs
  table       td_cloud_heads, torch.cumsum, td_cloud_reduce_packed, with the voxel count known (no synchronisation inside)
  merge       merge_hip of the chunk's voxels into a running map built from ``--map_chunks`` earlier chunks of the same drive
  surface     td_tsdf_surface on the merged map (the boolean select that compacts its slots is not part of it)
  chunk       everything a chunk costs after the depth network: samples, table_hip, merge_hip, host clock around a synchronise
and the same stages of the voxel average (keys, sort, table, merge, chunk) under "average".  Alongside: the numpy statements' time for
the same batch (samples_numpy + voxel_table_numpy, and surface_numpy on the chunk's own map, once each) and ``device_equals_numpy``:
the chunk's voxel rows and its surface slots, bit for bit.  The network and the frame upload are not part of this benchmark.

  python tools/tsdf_bench.py [--repeats 20] [--warmup 3] [--map_chunks 8] [--json profiles/tsdf/tsdf_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import cloud, tsdf  # noqa: E402
from cloud_bench import B, HBM_COPY, HBM_SPEC, PARAMS, VOXEL, chunk_inputs, count_items, inv_K, timed, wall_clock  # noqa: E402

T = 3
MIN_WEIGHT = tsdf.DEFAULT_MIN_WEIGHT
SAMPLE_PARAMS = {k: v for k, v in PARAMS.items() if k != "inv_voxel"}


def bench_size(H, W, device, args):
    ik = inv_K(H, W)
    ik_d = tsdf.inv_K_device(ik, device)
    sample = lambda d, c, p: tsdf.samples_hip(d, c, p, ik_d, T, VOXEL, **SAMPLE_PARAMS)
    empty = lambda: (torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, 7, dtype=torch.int64, device=device))
    (tkeys, tsums), (akeys, asums) = empty(), empty()
    for index in range(args.map_chunks):
        inputs = chunk_inputs(index, H, W, device)
        tkeys, tsums = cloud.merge_hip(tkeys, tsums, *cloud.table_hip(*sample(*inputs)))
        akeys, asums = cloud.merge_hip(akeys, asums, *cloud.table_hip(*cloud.keys_hip(*inputs, ik, **PARAMS)))
    depth, color, poses = chunk_inputs(args.map_chunks, H, W, device)
    n = B * H * W
    out = {"height": H, "width": W, "batch": B, "points": n, "pairs": (4 * T + 1) * n, "map_chunks": args.map_chunks}

    def stages(make_pairs, map_keys, map_sums):
        key, payload = make_pairs()
        sorted_keys, perm = torch.sort(key)
        seg = torch.cumsum(cloud.heads_hip(sorted_keys), 0)
        V = int(seg[-1].item())
        ckeys, csums = cloud.reduce_hip(sorted_keys, seg, perm, payload, V)

        def table():
            s = torch.cumsum(cloud.heads_hip(sorted_keys), 0)
            cloud.reduce_hip(sorted_keys, s, perm, payload, V)

        def chunk():
            k, p = make_pairs()
            cloud.merge_hip(map_keys, map_sums, *cloud.table_hip(k, p))

        res = {"valid_pairs": int((key != cloud.INVALID_KEY).sum().item()), "chunk_voxels": V, "map_voxels": int(map_keys.shape[0]),
               "pairs": timed(make_pairs, args.warmup, args.repeats), "sort": timed(lambda: torch.sort(key), args.warmup, args.repeats),
               "table": timed(table, args.warmup, args.repeats),
               "merge": timed(lambda: cloud.merge_hip(map_keys, map_sums, ckeys, csums), args.warmup, args.repeats),
               "chunk": wall_clock(chunk, args), "host_syncs_per_chunk": count_items(chunk)}
        return res, ckeys, csums

    res, ckeys, csums = stages(lambda: sample(depth, color, poses), tkeys, tsums)
    res["samples"] = res.pop("pairs")
    out.update(res)
    out["average"], _, _ = stages(lambda: cloud.keys_hip(depth, color, poses, ik, **PARAMS), akeys, asums)
    out["average"]["keys"] = out["average"].pop("pairs")
    mkeys, msums = cloud.merge_hip(tkeys, tsums, ckeys, csums)
    out["surface"] = timed(lambda: tsdf.surface_hip(mkeys, msums, VOXEL, MIN_WEIGHT), args.warmup, args.repeats)
    counts = torch.zeros(len(tsdf.SURFACE_STATS), dtype=torch.int64, device=device)
    tsdf.surface_hip(mkeys, msums, VOXEL, MIN_WEIGHT, stats=counts)
    out["surface_map_voxels"] = int(mkeys.shape[0])
    out["surface_stats"] = dict(zip(tsdf.SURFACE_STATS, (int(v) for v in counts.cpu())))
    rate = (7.0 + 16.0 * (4 * T + 1)) * n / (out["samples"]["median_us"] * 1e-6)
    out["samples_bytes_per_s"] = rate
    out["samples_fraction_of_hbm_spec"], out["samples_fraction_of_measured_copy"] = rate / HBM_SPEC, rate / HBM_COPY
    d, c, p = depth.cpu().numpy(), color.cpu().numpy(), poses.cpu().numpy()
    t0 = time.perf_counter()
    hkey, hpayload, _ = tsdf.samples_numpy(d, c, p, ik, T, VOXEL, **SAMPLE_PARAMS)
    t1 = time.perf_counter()
    hkeys, hsums = cloud.voxel_table_numpy(hkey, hpayload)
    t2 = time.perf_counter()
    want = tsdf.surface_numpy(hkeys, hsums, VOXEL, MIN_WEIGHT)
    t3 = time.perf_counter()
    out["numpy_samples_s"], out["numpy_table_s"], out["numpy_surface_s"] = t1 - t0, t2 - t1, t3 - t2
    got = [t.cpu().numpy() for t in tsdf.surface_hip(ckeys, csums, VOXEL, MIN_WEIGHT)]
    hit = want[4]
    same = np.array_equal(ckeys.cpu().numpy(), hkeys) and np.array_equal(csums.cpu().numpy(), hsums) and np.array_equal(got[4], hit)
    same = same and all(np.array_equal(a[hit].view(np.uint32), b[hit].view(np.uint32)) for a, b in zip(got[:2], want[:2]))
    out["device_equals_numpy"] = bool(same and all(np.array_equal(a[hit], b[hit]) for a, b in zip(got[2:4], want[2:4])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--map_chunks", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "voxel": VOXEL, "trunc_voxels": T, "min_weight": MIN_WEIGHT, "repeats": args.repeats,
           "warmup": args.warmup, "sizes": [bench_size(H, W, device, args) for H, W in ((192, 640), (320, 1024))]}
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
