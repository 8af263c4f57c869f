#!/usr/bin/env python3
"""Timing of the surfel renderer and of the orientation of normals (tripled_amd.render, tripled_amd.cloud_normals, csrc/td_surfel.hip)
on one GPU, beside the square-splat renderer of the same library in the same run.

The cloud is tools/render_bench.py's SYNTHETIC corridor (about 3 million points on a voxel lattice, voxel 0.005, random colours, random
order), with the normals of its planes in cloud_normals' sign convention (largest component positive); no real cloud has been
rendered.  Twelve cameras, near 0.1, far 4.0, 192 x 640 and 320 x 1024.  Timed, device events, median of ``--repeats`` after
``--warmup`` calls, microseconds per call:
  orient    orient_hip against the 12 cameras, and against a trajectory of 1 600 cameras along the corridor
  surfels   render_surfels_hip (two fills, scatter, resolve) in both work distributions: "thread" (one thread per surfel) and
            "cooperative" (boxes of more than 4 pixels through the LDS queue); radius = half the voxel, ambient 0.5, no culling
  squares   render_hip with splat = the voxel, which covers a comparable area
Alongside: the share of pixels hit by each, the surfel stats summed over the views, whether the two forms return the same bits, and
whether the device equals the numpy statement on a subsample (every ``--subsample``-th point, the first 2 cameras).

  python tools/surfel_bench.py [--repeats 50] [--warmup 5] [--json profiles/render/surfel_bench_v1.json] [--txt ....txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tripled_amd  # noqa: F401,E402
from tripled_amd import cloud_normals, render  # noqa: E402
import render_bench as RB  # noqa: E402

RADIUS, AMBIENT, TRAJECTORY = 0.5 * RB.VOXEL, 0.5, 1600


def make_normals(xyz):
    """The corridor's planes: the ground has y = CAMERA_HEIGHT exactly (in float32), everything else is a wall."""
    ground = xyz[:, 1] == np.float32(RB.CAMERA_HEIGHT)
    n = np.zeros_like(xyz)
    n[ground, 1], n[~ground, 0] = 1.0, 1.0
    return n


def make_trajectory(n):
    poses = np.zeros((n, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[:, 2, 3] = RB.LENGTH * np.arange(n) / n
    return poses


def equal_bits(a, b):
    return bool(all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)) for x, y in zip(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--subsample", type=int, default=30, help="every n-th point goes through the numpy statement (0: skip it)")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "render", "surfel_bench_v1.json"))
    ap.add_argument("--txt", default=None, help="default: --json with .txt")
    args = ap.parse_args()
    device = torch.device("cuda", 0)
    xyz, rgb = RB.make_cloud()
    raw = make_normals(xyz)
    poses = RB.make_cameras()
    xyz_d, rgb_d, raw_d, poses_d = (torch.from_numpy(a).to(device) for a in (xyz, rgb, raw, poses))
    out = {"device": torch.cuda.get_device_name(0), "points": len(xyz), "cameras": RB.CAMERAS, "synthetic_cloud": True, "voxel": RB.VOXEL,
           "radius": RADIUS, "ambient": AMBIENT, "near": RB.NEAR, "far": RB.FAR, "repeats": args.repeats, "warmup": args.warmup,
           "subsample": args.subsample, "orient": [], "cases": []}
    lines = ["%s, %d points (synthetic corridor), %d cameras, median of %d runs after %d" % (
        out["device"], len(xyz), RB.CAMERAS, args.repeats, args.warmup)]
    for name, cams in (("the %d cameras" % RB.CAMERAS, poses_d), ("a trajectory of %d" % TRAJECTORY, torch.from_numpy(make_trajectory(TRAJECTORY)).to(device))):
        t = RB.timed(lambda: cloud_normals.orient_hip(xyz_d, raw_d, cams), args.warmup, args.repeats)
        turned = cloud_normals.orient_hip(xyz_d, raw_d, cams)
        stats = dict(zip(cloud_normals.ORIENT_STATS, (int(v) for v in turned.stats.cpu())))
        out["orient"].append({"cameras": int(cams.shape[0]), "time": t, "stats": stats})
        lines.append("orient against %-22s %9.1f us (min %.1f, max %.1f)  %s" % (
            name, t["median_us"], t["min_us"], t["max_us"], " ".join("%s %d" % kv for kv in stats.items())))
    normals_d = cloud_normals.orient_hip(xyz_d, raw_d, poses_d).normal
    normals = normals_d.cpu().numpy()
    for H, W in RB.SIZES:
        K = RB.kitti_K(H, W)
        workspace = render.render_workspace(RB.CAMERAS, H, W, device)
        case = {"height": H, "width": W}

        def surfels(form):
            return render.render_surfels_hip(xyz_d, rgb_d, normals_d, poses_d, K, H, W, RADIUS, near=RB.NEAR, far=RB.FAR, ambient=AMBIENT,
                                             workspace=workspace, form=form)

        def squares():
            return render.render_hip(xyz_d, rgb_d, poses_d, K, H, W, near=RB.NEAR, far=RB.FAR, splat=RB.VOXEL, workspace=workspace)

        # alternate the three, so that all of them see the same machine state
        case["squares"] = RB.timed(squares, args.warmup, args.repeats)
        case["thread"] = RB.timed(lambda: surfels("thread"), args.warmup, args.repeats)
        case["cooperative"] = RB.timed(lambda: surfels("cooperative"), args.warmup, args.repeats)
        case["squares_again"] = RB.timed(squares, args.warmup, args.repeats)
        got = {form: [t.cpu().numpy() for t in surfels(form)] for form in ("thread", "cooperative")}
        case["forms_equal"] = equal_bits(got["thread"], got["cooperative"])
        stats = got["thread"][4]
        case["stats_total"] = dict(zip(render.SURFEL_STATS, (int(v) for v in stats.sum(0))))
        case["share_hit_surfels"] = float(stats[:, 7].sum()) / (RB.CAMERAS * H * W)
        case["share_hit_squares"] = float(squares().stats[:, 4].sum().cpu()) / (RB.CAMERAS * H * W)
        if args.subsample:
            sub = slice(None, None, args.subsample)
            xs, cs, ns = (np.ascontiguousarray(a[sub]) for a in (xyz, rgb, normals))
            want = render.render_surfels_numpy(xs, cs, ns, poses[:2], K, H, W, RADIUS, near=RB.NEAR, far=RB.FAR, ambient=AMBIENT)
            dev = render.render_surfels_hip(*(torch.from_numpy(a).to(device) for a in (xs, cs, ns)), poses_d[:2].contiguous(), K, H, W, RADIUS,
                                            near=RB.NEAR, far=RB.FAR, ambient=AMBIENT)
            case["device_equals_numpy"] = equal_bits([t.cpu().numpy() for t in dev], want)
            case["subsample_points"] = len(xs)
        out["cases"].append(case)
        lines.append("%4d x %4d  squares (splat %g) %9.1f us  surfels (radius %g) thread %9.1f us  cooperative %9.1f us  squares again %9.1f us" % (
            H, W, RB.VOXEL, case["squares"]["median_us"], RADIUS, case["thread"]["median_us"], case["cooperative"]["median_us"],
            case["squares_again"]["median_us"]))
        lines.append("             hit: squares %.3f surfels %.3f  forms equal %s  %s%s" % (
            case["share_hit_squares"], case["share_hit_surfels"], case["forms_equal"],
            " ".join("%s %d" % kv for kv in case["stats_total"].items()),
            "  device equals numpy on %d points x 2 cameras: %s" % (case["subsample_points"], case["device_equals_numpy"]) if args.subsample else ""))
    line = json.dumps(out)
    print("\n".join(lines))
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")
    with open(args.txt or os.path.splitext(args.json)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
