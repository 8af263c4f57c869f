#!/usr/bin/env python3
"""Records tests/golden/odometry.npz: a short ground-truth trajectory, a drifting prediction, and what the REFERENCE's pose
evaluation programs make of them, so that the tests of tripled_amd.odometry (CPU and GPU) have the reference's numbers where its
checkout is not present.

  python tools/gen_golden_pose.py --reference /path/to/reference [--out tests/golden/odometry.npz]

The reference's mono/datasets/utils.py (dump_xyz, compute_ate) and mono/tools/kitti_evaluation_toolkit.py (with trajectory.py,
geometry.py, ...) are loaded stand-alone (``load_reference``): while they load, ``mono`` names the reference's directories and
cv2 / matplotlib are stub modules; afterwards sys.modules is as it was.  Recorded (data only):
  gt [300,3,4]      the first 300 poses of the reference's mono/datasets/gt_pose/09.txt
  rel [299,4,4]     float32 relative transforms (frame k+1 -> frame k) of a prediction derived from gt by a seeded drift
                    (rotation bias + noise, translation noise) and a scale of 0.03
  traj [300,3,4]    the loop of scripts/draw_odometry.py:62-74 over ``rel`` widened to float64
  ates [299]        scripts/eval_pose.py:66-80 with the reference's dump_xyz and compute_ate
  seq_err [k,5]     kittiOdomEval.calcSequenceErrors (object made without __init__, lengths = [100, 200]) of gt against traj after
                    align_trajectory(correct_only_scale=True); scale: that alignment's scale; distance: the object's
  overall [2]       computeOverallErr (t_err, r_err);  segment [2,3]: computeSegmentErr rows (len, t_err, r_err)
The conditions the tests rely on are checked here: every segment's rotation error is above 1e-3 rad (arccos is ill-conditioned at
0) and no cumulative distance lies within 1e-6 m of a dist[first] + len threshold.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POSES = 300
LENGTHS = [100, 200]
SCALE = 0.03


def load_reference(reference_root):
    """(mono.datasets.utils, mono.tools.kitti_evaluation_toolkit, mono.tools.trajectory) of the reference as modules."""
    mono_dir = os.path.join(reference_root, "mono")
    saved = {k: v for k, v in sys.modules.items() if k == "mono" or k.startswith("mono.") or k == "cv2" or k.startswith("matplotlib")}
    for k in saved:
        del sys.modules[k]
    bytecode = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        for name, path in (("mono", mono_dir), ("mono.tools", os.path.join(mono_dir, "tools")),
                           ("mono.datasets", os.path.join(mono_dir, "datasets"))):
            pkg = types.ModuleType(name)
            pkg.__path__ = [path]
            sys.modules[name] = pkg
        sys.modules["cv2"] = types.ModuleType("cv2")
        for name in ("matplotlib", "matplotlib.pyplot", "matplotlib.backends", "matplotlib.backends.backend_pdf"):
            sys.modules[name] = types.ModuleType(name)
        sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
        sys.modules["matplotlib"].backends = sys.modules["matplotlib.backends"]
        sys.modules["matplotlib.backends"].backend_pdf = sys.modules["matplotlib.backends.backend_pdf"]
        sys.modules["matplotlib.pyplot"].switch_backend = lambda name: None
        return (importlib.import_module("mono.datasets.utils"), importlib.import_module("mono.tools.kitti_evaluation_toolkit"),
                importlib.import_module("mono.tools.trajectory"))
    finally:
        sys.dont_write_bytecode = bytecode
        for k in [k for k in sys.modules if k == "mono" or k.startswith("mono.") or k == "cv2" or k.startswith("matplotlib")]:
            del sys.modules[k]
        sys.modules.update(saved)


def to_4x4(p):
    out = np.zeros((len(p), 4, 4))
    out[:, :3] = p
    out[:, 3, 3] = 1.0
    return out


def rodrigues(v):
    angle = np.linalg.norm(v)
    if angle == 0:
        return np.eye(3)
    k = v / angle
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def drifting_prediction(gt, seed=0):
    """float32 [n,4,4]: M_k = inv(D'_k), D'_k = the ground truth's step inv(G_k) G_{k+1} with a rotation drift (a constant bias of
    2e-3 rad per frame about y plus noise), translation noise, and the translation scaled by 0.03 (a monocular network's unit)."""
    g = np.random.default_rng(seed)
    G = to_4x4(gt)
    rel = []
    for k in range(len(G) - 1):
        D = np.linalg.inv(G[k]) @ G[k + 1]
        D[:3, :3] = D[:3, :3] @ rodrigues(np.array([0.0, 2e-3, 0.0]) + g.normal(0, 5e-4, 3))
        D[:3, 3] = SCALE * (D[:3, 3] * (1 + g.normal(0, 0.03)) + g.normal(0, 0.01, 3))
        rel.append(np.linalg.inv(D))
    return np.stack(rel).astype(np.float32)


def draw_odometry_loop(rel):
    """scripts/draw_odometry.py:62-74 on whatever dtype ``rel`` has: [n,4,4] -> [n+1,3,4]."""
    global_pose = np.identity(4)
    poses = [global_pose[0:3, :].reshape(1, 12)]
    for backward_transform in rel:
        global_pose = global_pose @ np.linalg.inv(backward_transform)
        poses.append(global_pose[0:3, :].reshape(1, 12))
    return np.concatenate(poses, axis=0).reshape(-1, 3, 4)


def eval_pose_ates(utils, rel, gt):
    """scripts/eval_pose.py:66-80."""
    G = to_4x4(gt)
    gt_local = [np.linalg.inv(np.dot(np.linalg.inv(G[i - 1]), G[i])) for i in range(1, len(G))]
    ates, track_length = [], 5
    for i in range(0, len(G) - 1):
        local_xyzs = np.array(utils.dump_xyz(rel[i:i + track_length - 1]))
        gt_local_xyzs = np.array(utils.dump_xyz(gt_local[i:i + track_length - 1]))
        ates.append(utils.compute_ate(gt_local_xyzs, local_xyzs))
    return np.array(ates, dtype=np.float64)


def toolkit_eval(toolkit, trajectory, gt, traj, lengths=LENGTHS):
    """kittiOdomEval.eval's core (kitti_evaluation_toolkit.py:571-621) on in-memory poses."""
    ev = toolkit.kittiOdomEval.__new__(toolkit.kittiOdomEval)
    ev.lengths, ev.num_lengths = list(lengths), len(lengths)
    tra_pred = trajectory.PosePath3D(poses_se3=list(to_4x4(traj)))
    tra_gt = trajectory.PosePath3D(poses_se3=list(to_4x4(gt)))
    corrected, _, _, scale = trajectory.align_trajectory(tra_pred, tra_gt, correct_only_scale=True, return_parameters=True)
    poses_result, poses_gt = ev.loadPoseSe3(corrected), ev.loadPoseSe3(tra_gt)
    seq_err = ev.calcSequenceErrors(poses_gt, poses_result)
    t_err, r_err = ev.computeOverallErr(seq_err)
    seg = ev.computeSegmentErr(seq_err)
    segment = np.array([[k, seg[k][0], seg[k][1]] for k in lengths if seg[k] != []], dtype=np.float64).reshape(-1, 3)
    dist = np.array(ev.trajectoryDistances(poses_gt), dtype=np.float64)
    return dict(seq_err=np.array(seq_err, dtype=np.float64).reshape(-1, 5), scale=np.float64(scale), distance=np.float64(ev.distance),
                overall=np.array([t_err, r_err], dtype=np.float64), segment=segment), dist


def check_conditions(seq_err, dist, lengths, step=10):
    """(smallest segment rotation error in rad, smallest |dist[i] - (dist[first] + len)| in m); raises if a test could be
    ill-conditioned on them."""
    r_min = float((seq_err[:, 1] * seq_err[:, 3]).min()) if len(seq_err) else float("inf")
    gap = min(float(np.abs(dist - (dist[first] + length)).min()) for first in range(0, len(dist), step) for length in lengths)
    if not r_min > 1e-3:
        raise ValueError("a segment's rotation error is %.3e rad: arccos is ill-conditioned there" % r_min)
    if not gap > 1e-6:
        raise ValueError("a cumulative distance lies %.3e m from a segment threshold" % gap)
    return r_min, gap


def record(reference_root):
    utils, toolkit, trajectory = load_reference(reference_root)
    gt = np.loadtxt(os.path.join(reference_root, "mono", "datasets", "gt_pose", "09.txt"))[:N_POSES].reshape(-1, 3, 4)
    out = {"gt": gt, "rel": drifting_prediction(gt)}
    out["traj"] = draw_odometry_loop(out["rel"].astype(np.float64))
    out["ates"] = eval_pose_ates(utils, out["rel"], gt)
    scored, dist = toolkit_eval(toolkit, trajectory, gt, out["traj"])
    out.update(scored)
    out["lengths"] = np.array(LENGTHS, dtype=np.int64)
    r_min, gap = check_conditions(out["seq_err"], dist, LENGTHS)
    print("conditions: smallest segment rotation error %.3e rad, nearest threshold %.3e m, %d segments" % (r_min, gap,
                                                                                                         len(out["seq_err"])))
    return out


def deviations(reference_root, data):
    """What the two stated deviations from the reference amount to on the golden trajectory (figures for DESIGN.md section 16, no
    bounds): the float32 np.linalg.inv of draw_odometry.py against the widened inverse, and scoring the %1.8e text of the
    prediction against scoring the in-memory poses."""
    import io
    _, toolkit, trajectory = load_reference(reference_root)
    f32 = draw_odometry_loop(data["rel"])                      # np.linalg.inv of a float32 array stays in float32
    d_traj = float(np.abs(f32 - data["traj"]).max())
    buf = io.StringIO()
    np.savetxt(buf, data["traj"].reshape(-1, 12), delimiter=" ", fmt="%1.8e")
    text = np.loadtxt(io.StringIO(buf.getvalue())).reshape(-1, 3, 4)
    out = {"float32_inverse_max_abs_m": d_traj, "trajectory_extent_m": float(np.abs(data["traj"][:, :, 3]).max())}
    for name, traj in (("float32_inverse", f32), ("text_1.8e", text)):
        scored, _ = toolkit_eval(toolkit, trajectory, data["gt"], traj, [int(v) for v in data["lengths"]])
        out[name + "_t_err_rel"] = float(abs(scored["overall"][0] - data["overall"][0]) / data["overall"][0])
        out[name + "_r_err_rel"] = float(abs(scored["overall"][1] - data["overall"][1]) / data["overall"][1])
        out[name + "_scale_rel"] = float(abs(scored["scale"] - data["scale"]) / data["scale"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "odometry.npz"))
    args = ap.parse_args()
    data = record(args.reference)
    np.savez_compressed(args.out, **data)
    print("%s: %d arrays, %d bytes" % (args.out, len(data), os.path.getsize(args.out)))
    for k, v in deviations(args.reference, data).items():
        print("deviation %-32s %.3e" % (k, v))


if __name__ == "__main__":
    main()
