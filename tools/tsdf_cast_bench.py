#!/usr/bin/env python3
"""Timing of the TSDF ray cast (tripled_amd.tsdf.raycast_hip, csrc/td_tsdf_cast.hip) on one GPU, and of the surfel renderer on the
surface points of the same map in the same run.

The map is the one tools/tsdf_bench.py times: ``--map_chunks`` + 1 chunks of tools/cloud_bench.py's synthetic drive (12 frames each, at
192 x 640 and at 320 x 1024, voxel 0.2, band T = 3) fused by samples_hip and cloud's table / merge chain.  Cast: the 12 poses of the
last chunk, near 0.5, far 40, steps of half a voxel (396 samples per ray), min_weight 2.  Timed with device events, median of
``--repeats`` after ``--warmup`` runs; every timing is taken in ``--passes`` separate passes that alternate between the timed calls, and
the spread between a call's pass medians is its run-to-run spread:
  cast        td_tsdf_cast: four lower bounds in the key table per sample
  surfels     td_cloud_render_surfels on the map's surface points (td_tsdf_surface, compacted) with their normals, radius = the voxel
and the share of pixels hit by the cast and by the surfels.  ``device_equals_numpy``: 2 of the views at 24 x 80 (the same camera with
its principal point moved, so the small view looks at the middle of the large one) against raycast_numpy, bit for bit.
profiles/tsdf/tsdf_cast_bench_v1.* was written by an earlier form of this tool, when the kernel also had a two-level form (a sorted
table of occupied 8 x 8 x 8 blocks asked first): it lost to this one at both sizes and was dropped.  Those two files
are the record of that comparison and this tool cannot make them again: it refuses to write over them; its own output is
profiles/tsdf/tsdf_cast_bench_v2.{txt,json}.

  python tools/tsdf_cast_bench.py [--repeats 20] [--warmup 3] [--passes 3] [--map_chunks 8] [--json profiles/tsdf/tsdf_cast_bench_v2.json]
         [--txt profiles/tsdf/tsdf_cast_bench_v2.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import cloud, render, tsdf  # noqa: E402
from cloud_bench import B, PARAMS, VOXEL, chunk_inputs, intrinsics, inv_K, timed  # noqa: E402

T = 3
MIN_WEIGHT = tsdf.DEFAULT_MIN_WEIGHT
SAMPLE_PARAMS = {k: v for k, v in PARAMS.items() if k != "inv_voxel"}
CAST = dict(min_weight=MIN_WEIGHT, near=0.5, far=40.0, step_voxels=tsdf.DEFAULT_STEP_VOXELS)


def fused_map(H, W, device, chunks):
    ik_d = tsdf.inv_K_device(inv_K(H, W), device)
    keys, sums = torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, 7, dtype=torch.int64, device=device)
    for index in range(chunks):
        depth, color, poses = chunk_inputs(index, H, W, device)
        keys, sums = cloud.merge_hip(keys, sums, *cloud.table_hip(*tsdf.samples_hip(depth, color, poses, ik_d, T, VOXEL, **SAMPLE_PARAMS)))
    return keys, sums, poses


def same_bits(got, want):
    host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else t
    return all(np.array_equal(host(a).view(np.uint32) if host(a).dtype == np.float32 else host(a),
                              b.view(np.uint32) if b.dtype == np.float32 else b) for a, b in zip(got, want))


def bench_size(H, W, device, args):
    keys, sums, poses = fused_map(H, W, device, args.map_chunks + 1)
    ik, K = tsdf.inv_K_device(inv_K(H, W), device), intrinsics(H, W)      # on the device once: no upload inside a timed call
    cast = lambda: tsdf.raycast_hip(keys, sums, poses, ik, H, W, VOXEL, **CAST)
    stats = cast().stats.cpu().numpy()
    out = {"height": H, "width": W, "views": B, "map_voxels": int(keys.shape[0]),
           "n_steps": tsdf._check_cast(H, W, VOXEL, MIN_WEIGHT, CAST["near"], CAST["far"], CAST["step_voxels"])[1],
           "cast_stats": dict(zip(tsdf.CAST_STATS, (int(v) for v in stats.sum(0)))),
           "cast_share_hit": float(stats[:, 1].sum() / stats[:, 0].sum())}
    # the surface points of the same map through the surfel renderer
    xyz, normal, rgb, _, hit = tsdf.surface_hip(keys, sums, VOXEL, MIN_WEIGHT)
    xyz, normal, rgb = xyz[hit].contiguous(), normal[hit].contiguous(), rgb[hit].contiguous()
    workspace = render.render_workspace(B, H, W, device)
    surfels = lambda: render.render_surfels_hip(xyz, rgb, normal, poses, K, H, W, VOXEL, near=CAST["near"], far=CAST["far"], workspace=workspace)
    drawn = surfels().stats.cpu().numpy()
    out["surface_points"], out["surfel_radius"] = int(xyz.shape[0]), VOXEL
    out["surfel_share_hit"] = float(drawn[:, 7].sum() / (B * H * W))
    timings = dict(cast=cast, surfels=surfels)
    passes = {name: [] for name in timings}
    for _ in range(args.passes):                                    # alternate: a drift of the clocks meets both alike
        for name, fn in timings.items():
            passes[name].append(timed(fn, args.warmup, args.repeats))
    for name, runs in passes.items():
        medians = [r["median_us"] for r in runs]
        out[name] = {"median_us": statistics.median(medians), "pass_medians_us": medians, "min_us": min(r["min_us"] for r in runs),
                     "max_us": max(r["max_us"] for r in runs), "runs": args.passes * args.repeats}
        out[name]["pass_spread_us"] = max(medians) - min(medians)
    # a subsample against the statement: the same cameras, a 24 x 80 window in the middle of the image
    h, w = 24, 80
    k_small = K.copy()
    k_small[0, 2] -= (W - w) // 2
    k_small[1, 2] -= (H - h) // 2
    ik_small = np.linalg.inv(k_small)                                   # (a host array: uploaded by the checking call)
    host_keys, host_sums, views = keys.cpu().numpy(), sums.cpu().numpy(), poses[:2].cpu().numpy()
    want = tsdf.raycast_numpy(host_keys, host_sums, views, ik_small, h, w, VOXEL, **CAST)
    out["subsample_hits"] = int(want.stats[:, 1].sum())
    out["device_equals_numpy"] = bool(same_bits(tsdf.raycast_hip(keys, sums, poses[:2], ik_small, h, w, VOXEL, **CAST), want))
    return out


def report(out):
    lines = ["TSDF ray cast on %s: %d views per launch, voxel %g, band %d, min_weight %d, near %g, far %g, step %g voxels"
             % (out["device"], B, VOXEL, T, MIN_WEIGHT, CAST["near"], CAST["far"], CAST["step_voxels"]),
             "medians of %d passes x %d runs (after %d warm-up runs each), device events, microseconds" % (out["passes"], out["repeats"], out["warmup"])]
    for s in out["sizes"]:
        lines.append("")
        lines.append("%d x %d: map %d voxels, %d samples per ray" % (s["height"], s["width"], s["map_voxels"], s["n_steps"]))
        for name in ("cast", "surfels"):
            r = s[name]
            lines.append("  %-10s median %10.1f   pass medians %s (spread %.1f)   min %.1f max %.1f   (%d runs)" % (
                name, r["median_us"], " ".join("%.1f" % v for v in r["pass_medians_us"]), r["pass_spread_us"], r["min_us"], r["max_us"], r["runs"]))
        lines.append("  share of pixels hit: cast %.4f (%s), surfels of radius %g on %d surface points %.4f" % (
            s["cast_share_hit"], " ".join("%s %d" % kv for kv in s["cast_stats"].items()), s["surfel_radius"], s["surface_points"],
            s["surfel_share_hit"]))
        lines.append("  device equals raycast_numpy on 2 views of 24 x 80 (%d hits): %s" % (s["subsample_hits"], s["device_equals_numpy"]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--map_chunks", type=int, default=8)
    ap.add_argument("--json", default=None)
    ap.add_argument("--txt", default=None)
    args = ap.parse_args()
    for path in (args.json, args.txt):
        if path and os.path.basename(path).startswith("tsdf_cast_bench_v1."):
            ap.error("%s is the record of the two-form comparison, which this tool no longer runs: write to a v2 name" % path)
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "voxel": VOXEL, "trunc_voxels": T, "cast": CAST, "repeats": args.repeats,
           "warmup": args.warmup, "passes": args.passes, "sizes": [bench_size(H, W, device, args) for H, W in ((192, 640), (320, 1024))]}
    line = json.dumps(out)
    print(line)
    for path, text in ((args.json, line + "\n"), (args.txt, report(out))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
