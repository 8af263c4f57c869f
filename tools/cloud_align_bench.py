#!/usr/bin/env python3
"""Timing of the cloud alignment (tripled_amd.cloud_align, csrc/td_align.hip) on one GPU.

The SYNTHETIC street of tools/cloud_eval_bench.py: a reference of about 3 M points (a ground strip of ``--length`` x 40 units, two
walls of ``--length`` x 10, one point per 0.2 x 0.2 patch) and a predicted cloud that is the same street sampled half a voxel over
with 0.1 units of noise along the normals, carried through the INVERSE of a planted similarity transform about the street's centre
(0.01 degrees about a tilted axis, scale 1.0002, 0.1 units of translation: up to 0.4 units at the street's ends, inside tau = 0.6).
Timed, median of ``--repeats`` after ``--warmup`` runs of the same shapes:
  transform        td_cloud_transform on the predicted cloud, device events (reads 24 bytes and writes 24 per point)
  moments          td_icp_moments as called (the clear of 152 bytes and both stages), device events
  moments_rows / moments_finish   the two stages on their own, from torch.profiler's kernel records of the same calls (device time of
                   each kernel); "stages_error" says why when the profiler gave none
  query            td_nn_query of the transformed cloud into the reference's grid, K = 0 thresholds, device events
  iteration        one pass of CloudAligner: transform, query, moments, the copy of 19 numbers, the host solve; host clock
  align            CloudAligner.align end to end (grid_hip, the origin, all passes), host clock
Alongside: the passes it took, the recovered transform's distance from the planted one, and ``device_equals_numpy``: on a stated random
subsample of the predicted points against the whole reference, the bits of the transformed points and, after nearest_numpy, of the 17
sums and the counters.
With ``--criterion plane`` additionally (the point-to-point figures stay, for the comparison):
  normals          td_cloud_normals (csrc/td_normals.hip) of the whole reference against its own grid, device events, and its counters
  plane_moments    td_icp_plane_moments as called, with its ratio to ``moments`` and its bytes per row (64 + 24 for the gathered normal)
  plane_iteration  one pass of CloudAligner(criterion="plane"): transform, query, plane moments, the copy of 40 numbers, the host solve
  plane_align      CloudAligner(criterion="plane").align end to end (grid, origin, normals, all passes), host clock
  plane_result     its passes, ranks, dropped directions (the weight of every unknown: w (3), tau (3), sigma), its distance from the
                   planted transform and the largest displacement of a predicted point from its planted position, beside ``result``'s
  plane_device_equals_numpy   on the subsample: the bits of the normals (subsampled queries, whole grid), of the 37 sums and the counters
Every figure is of ONE run of this tool (``runs``: 1) on a SYNTHETIC scene (``scene``).

  python tools/cloud_align_bench.py [--repeats 20] [--warmup 3] [--length 2000] [--subsample 20000] [--criterion plane] [--json profiles/cloud_eval/cloud_align_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import cloud_align, cloud_eval, cloud_normals  # noqa: E402
from cloud_eval_bench import TAU, VOXEL, street, timed, wall_clock  # noqa: E402

DEGREES, SCALE, SHIFT = 0.01, 1.0002, 0.1
ROW_BYTES = 64          # per row of the moments: 24 (cur) + 8 (index) + 8 (d2) read in order, 24 gathered from the reference
PLANE_ROW_BYTES = 88    # the plane moments gather the neighbour's normal as well: 24 more


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K.dot(K)


def stage_times(fn, repeats):
    """Device time per kernel name over ``repeats`` calls of fn(), from torch.profiler -> {name: median_us}."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(repeats):
            fn()
        torch.cuda.synchronize()
    seen = {}
    for ev in prof.events():
        for stage in ("icp_moments_rows_kernel", "icp_moments_finish_kernel"):
            if stage in ev.name:
                seen.setdefault(stage, []).append(float(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0)))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "records": len(v)} for k, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--length", type=float, default=2000.0)
    ap.add_argument("--subsample", type=int, default=20000)
    ap.add_argument("--criterion", choices=cloud_align.CRITERIA, default="point")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "voxel": VOXEL, "tau": TAU, "repeats": args.repeats, "warmup": args.warmup,
           "length": args.length, "planted": {"degrees": DEGREES, "scale": SCALE, "shift": SHIFT}, "runs": 1,
           "scene": "SYNTHETIC street (tools/cloud_eval_bench.py)", "criterion": args.criterion}
    ref, moved = street(args.length, 1, 0.0, 0.0), street(args.length, 2, 0.5 * VOXEL, 0.1)
    centre = np.array([0.5 * args.length, 0.0, 0.0])
    R = rotation([0.3, 1.0, 0.2], DEGREES)
    t = SHIFT * np.array([0.6, -0.3, 0.74]) / np.linalg.norm([0.6, -0.3, 0.74])
    t = centre - SCALE * R.dot(centre) + t                               # x' = c R (x - centre) + centre + shift
    pred = (moved - t).dot(R) / SCALE
    ref_d, pred_d = torch.from_numpy(ref).to(device), torch.from_numpy(pred).to(device)
    out["n_ref"], out["n_pred"] = len(ref), len(pred)
    eye, zero = np.eye(3), np.zeros(3)
    grid = cloud_eval.grid_hip(ref_d, TAU)
    origin = 0.5 * (ref.min(0) + ref.max(0))
    trim2 = TAU * TAU
    cur = cloud_align.transform_hip(pred_d, 1.0, eye, zero)
    nb = cloud_eval.nearest_hip(cur, grid, TAU, ())
    out["transform"] = timed(lambda: cloud_align.transform_hip(pred_d, SCALE, R, t, out=cur), args.warmup, args.repeats)
    out["transform_bytes_per_s"] = 48.0 * len(pred) / (out["transform"]["median_us"] * 1e-6)
    cur = cloud_align.transform_hip(pred_d, 1.0, eye, zero)               # the first pass's cloud again
    sums = torch.empty(19, dtype=torch.float64, device=device)
    moments = lambda: cloud_align.moments_hip(cur, ref_d, nb.index, nb.d2, trim2, origin, out=sums)
    out["moments"] = timed(moments, args.warmup, args.repeats)
    try:
        out.update({"moments_rows": None, "moments_finish": None})
        stages = stage_times(moments, args.repeats)
        out["moments_rows"], out["moments_finish"] = stages.get("icp_moments_rows_kernel"), stages.get("icp_moments_finish_kernel")
        if out["moments_rows"]:
            out["moments_rows_bytes_per_s"] = ROW_BYTES * len(pred) / (out["moments_rows"]["median_us"] * 1e-6)
    except Exception as e:                                                # the split is extra: the entry point's time stands without it
        out["stages_error"] = "%s: %s" % (type(e).__name__, e)
    out["moments_bytes_per_s"] = ROW_BYTES * len(pred) / (out["moments"]["median_us"] * 1e-6)
    out["matched_first_pass"] = cloud_align.moments_to_host(sums)[1]
    out["query"] = timed(lambda: cloud_eval.nearest_hip(cur, grid, TAU, ()), args.warmup, args.repeats)
    aligner = cloud_align.CloudAligner(device, TAU)

    def one_pass():
        m, matched, _ = aligner._pass(pred_d, ref_d, grid, origin, 1.0, eye, zero, trim2)
        return cloud_align.solve_from_moments(matched, m)

    out["iteration"] = wall_clock(one_pass, args.warmup, args.repeats)
    out["align"] = wall_clock(lambda: aligner.align(pred_d, ref_d), args.warmup, args.repeats)
    result = aligner.align(pred_d, ref_d)
    out["result"] = {"iterations": result.iterations, "converged": result.converged, "matched": [h[0] for h in result.history],
                     "rms": [h[1] for h in result.history], "scale_error": abs(result.scale - SCALE) / SCALE,
                     "R_error": float(np.abs(result.R - R).max()), "t_error": float(np.abs(result.t - t).max())}
    # the statements on a subsample of the predicted points, against the whole reference
    pick = np.sort(np.random.default_rng(3).choice(len(pred), min(args.subsample, len(pred)), replace=False))
    sub_d = pred_d[torch.from_numpy(pick).to(device)].contiguous()
    t0 = time.perf_counter()
    want_cur = cloud_align.transform_numpy(pred[pick], SCALE, R, t)
    host_grid = cloud_eval.grid_numpy(ref, TAU)
    want_nb = cloud_eval.nearest_numpy(want_cur, host_grid, TAU, ())
    want = cloud_align.moments_numpy(want_cur, ref, want_nb.index, want_nb.d2, trim2, origin)
    out["subsample"], out["numpy_pass_subsample_s"] = len(pick), time.perf_counter() - t0
    got_cur = cloud_align.transform_hip(sub_d, SCALE, R, t)
    got_nb = cloud_eval.nearest_hip(got_cur, grid, TAU, ())
    got = cloud_align.moments_to_host(cloud_align.moments_hip(got_cur, ref_d, got_nb.index, got_nb.d2, trim2, origin))
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    out["device_equals_numpy"] = bool(np.array_equal(bits(got_cur.cpu().numpy()), bits(want_cur)) and
                                      np.array_equal(bits(got[0]), bits(want[0])) and got[1:] == want[1:])
    if args.criterion == "plane":
        displacement = lambda res: float(np.sqrt((((res.scale * pred[pick].dot(res.R.T) + res.t) - (SCALE * pred[pick].dot(R.T) + t)) ** 2).sum(1)).max())
        out["result"]["max_displacement_subsample"] = displacement(result)
        counters = torch.zeros(5, dtype=torch.int64, device=device)
        found = cloud_normals.normals_hip(ref_d, grid, stats=counters)
        out["normals"] = timed(lambda: cloud_normals.normals_hip(ref_d, grid), args.warmup, args.repeats)
        out["normal_counters"] = dict(zip(cloud_normals.CAUSES, (int(v) for v in counters.cpu().numpy())))
        out["normals_max_cell"] = grid.stats["max_cell"]
        plane_sums = torch.empty(40, dtype=torch.float64, device=device)
        plane = lambda: cloud_align.plane_moments_hip(cur, ref_d, found.normal, nb.index, nb.d2, trim2, origin, out=plane_sums)
        out["plane_moments"] = timed(plane, args.warmup, args.repeats)
        out["plane_moments_over_moments"] = out["plane_moments"]["median_us"] / out["moments"]["median_us"]
        out["plane_moments_bytes_per_row"] = PLANE_ROW_BYTES
        out["plane_moments_bytes_per_s"] = PLANE_ROW_BYTES * len(pred) / (out["plane_moments"]["median_us"] * 1e-6)
        first = cloud_align.plane_moments_to_host(plane_sums)
        out["plane_matched_first_pass"], out["plane_no_normal_first_pass"] = first[1], first[3]
        planar = cloud_align.CloudAligner(device, TAU, criterion="plane")
        length = float((0.5 * (ref.max(0) - ref.min(0))).max())

        def one_plane_pass():
            m, matched, _, _ = planar._pass(pred_d, ref_d, grid, origin, 1.0, eye, zero, trim2, found.normal)
            return cloud_align.solve_plane_step(matched, m, True, length, planar.rcond)

        out["plane_iteration"] = wall_clock(one_plane_pass, args.warmup, args.repeats)
        out["plane_align"] = wall_clock(lambda: planar.align(pred_d, ref_d), args.warmup, args.repeats)
        res = planar.align(pred_d, ref_d)
        out["plane_result"] = {"iterations": res.iterations, "converged": res.converged, "matched": [h[0] for h in res.history],
                               "rms": [h[1] for h in res.history], "plane_rms": [h[0] for h in planar.plane_history],
                               "ranks": [h[1] for h in planar.plane_history],
                               "dropped_weights": [None if h[2] is None else (h[2] ** 2).tolist() for h in planar.plane_history],
                               "unknowns": ["w_x", "w_y", "w_z", "tau_x", "tau_y", "tau_z", "sigma"],
                               "scale_error": abs(res.scale - SCALE) / SCALE, "R_error": float(np.abs(res.R - R).max()),
                               "t_error": float(np.abs(res.t - t).max()), "t_error_xyz": np.abs(res.t - t).tolist(),
                               "max_displacement_subsample": displacement(res)}
        want_normals = cloud_normals.normals_numpy(ref[pick], host_grid)
        got_normals = cloud_normals.normals_hip(ref_d[torch.from_numpy(pick).to(device)].contiguous(), grid)
        host_normals = found.normal.cpu().numpy()
        want_plane = cloud_align.plane_moments_numpy(want_cur, ref, host_normals, want_nb.index, want_nb.d2, trim2, origin)
        got_plane = cloud_align.plane_moments_to_host(cloud_align.plane_moments_hip(got_cur, ref_d, found.normal, got_nb.index, got_nb.d2, trim2, origin))
        out["plane_device_equals_numpy"] = bool(
            np.array_equal(bits(got_normals.normal.cpu().numpy()), bits(want_normals.normal)) and
            np.array_equal(bits(got_normals.curvature.cpu().numpy()), bits(want_normals.curvature)) and
            np.array_equal(got_normals.count.cpu().numpy(), want_normals.count) and
            np.array_equal(bits(got_plane[0]), bits(want_plane[0])) and got_plane[1:] == want_plane[1:])
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
