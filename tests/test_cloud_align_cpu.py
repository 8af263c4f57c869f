"""The host side of tripled_amd.cloud_align, pinned: moments_numpy (reshapes and halving slices) by a literal per-row loop over the same
two-stage tree, on the bits; transform_numpy by a per-point loop; the closed-form solve on a reflection and on every degenerate cause;
the whole loop on a small street with an exactly planted similarity transform; scripts/eval_cloud.py --align end to end on a synthetic
odometry tree, and its output without --align.  The C entry points refuse bad arguments before any launch, which a CPU host can check.
No GPU.

Bounds.  The planted transform is recovered within the project's RTOL = 1e-9 (tests/odom_util.py).  The floor is float64 rounding
through an SVD of a 3x3 (a few 1e-16, times the scene's extent of 20 for t) and depends on the BLAS behind numpy: the bound sits five
orders above it and three below what a float32 slip would show."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, cloud_align, cloud_eval, native, odometry
from tests import cloud_align_util as U
from tests import cloud_eval_util as E
from tests.odom_util import RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N", U.MOMENT_SIZES)
def test_moments_are_the_per_row_loop_over_the_tree(N):
    args = U.correspondences(N)
    cur, ref, index, d2, trim2, origin = args
    m, matched, bad = cloud_align.moments_numpy(*args)
    want_m, want_matched, want_bad = U.moments_loop(*args)
    assert U.same_bits(m, want_m) and (matched, bad) == (want_matched, want_bad)
    if N >= 255:                                                       # the inputs exercise every kind of row
        assert 0 < matched < N and bad == 3 and (index == -1).any() and (d2 > trim2).any() and np.isnan(d2).any()
        assert np.isnan(cur).any() and (index == len(ref) - 1).any() and (d2 == trim2).any() and np.isfinite(m).all() and m[16] > 0
    none = cloud_align.moments_numpy(*U.correspondences(N, kind="unmatched"))
    assert U.same_bits(none[0], np.zeros(17)) and none[1:] == (0, 0)
    every = U.correspondences(N, kind="matched")
    assert cloud_align.moments_numpy(*every)[1:] == (N, 0) and U.same_bits(cloud_align.moments_numpy(*every)[0], U.moments_loop(*every)[0])


def test_moments_of_nothing_and_bad_inputs():
    cur, ref, index, d2, trim2, origin = U.correspondences(5)
    m, matched, bad = cloud_align.moments_numpy(cur[:0], ref, index[:0], d2[:0], trim2, origin)
    assert U.same_bits(m, np.zeros(17)) and (matched, bad) == (0, 0)
    m, matched, bad = cloud_align.moments_numpy(cur, ref[:0], index, d2, trim2, origin)      # no reference: every index but -1 is bad
    assert U.same_bits(m, np.zeros(17)) and matched == 0 and bad == np.count_nonzero(index != -1) == 5
    for wrong in (dict(d2=d2[:4]), dict(index=index[:4]), dict(trim2=-1.0), dict(trim2=np.nan), dict(origin=[0, np.nan, 0])):
        kw = dict(cur=cur, ref=ref, index=index, d2=d2, trim2=trim2, origin=origin)
        kw.update(wrong)
        with pytest.raises(ValueError):
            cloud_align.moments_numpy(**kw)


@pytest.mark.parametrize("N", [0, 1, 65, 1000])
def test_transform_is_the_per_point_loop(N):
    src = U.points_with_poison(N)
    c, R, t = U.planted("large")
    got = cloud_align.transform_numpy(src, c, R, t)
    want = U.transform_loop(src, c, R, t)
    finite = np.isfinite(src).all(1)
    assert got.shape == (N, 3) and U.same_bits(got[finite], want[finite]) and np.array_equal(got, want, equal_nan=True)
    assert not np.isfinite(got[~finite]).all(1).any()                  # a row that is not finite stays not finite
    if N == 1000:
        assert (~finite).sum() == 3


def _moments_of_pairs(p, q, origin=(0.0, 0.0, 0.0)):
    n = len(p)
    return cloud_align.moments_numpy(p, q, np.arange(n), np.zeros(n), 1.0, origin)


def test_solve_recovers_a_similarity_and_handles_a_reflection():
    rng = np.random.default_rng(4)
    p = rng.normal(0, 3, (50, 3)) + [5.0, -2.0, 9.0]
    c, R, t = 1.7, U.rotation([1, 2, 3], 25.0), np.array([0.5, -4.0, 2.0])
    q = c * p.dot(R.T) + t
    m, n, _ = _moments_of_pairs(p, q)
    gc, gR, gt = cloud_align.solve_from_moments(n, m)
    assert abs(gc - c) <= RTOL * c and np.abs(gR - R).max() <= RTOL and np.abs(gt - t).max() <= RTOL * np.abs(t).max()
    rc, rR, rt = cloud_align.solve_from_moments(n, m, with_scale=False)
    assert rc == 1.0 and np.abs(rR - R).max() <= RTOL
    # a mirrored cloud: the least-squares orthogonal matrix has det -1, Umeyama's S flips the smallest singular direction instead
    mirrored = q * np.array([1.0, 1.0, -1.0])
    m, n, _ = _moments_of_pairs(p, mirrored)
    mean_p, mean_q = m[0:3] / n, m[3:6] / n
    u, d, v = np.linalg.svd(m[6:15].reshape(3, 3) / n - np.outer(mean_q, mean_p))
    assert np.linalg.det(u) * np.linalg.det(v) < 0                     # the case is the reflection case
    fc, fR, ft = cloud_align.solve_from_moments(n, m)
    assert np.linalg.det(fR) > 0 and np.abs(fR.dot(fR.T) - np.eye(3)).max() < 1e-12 and 0 < fc < c
    assert abs(fc - (d[0] + d[1] - d[2]) / (m[15] / n - mean_p.dot(mean_p))) <= RTOL * fc


def test_solve_is_degenerate_for_every_listed_cause():
    rng = np.random.default_rng(5)
    p = rng.normal(0, 1, (10, 3))
    m, n, _ = _moments_of_pairs(p, p)
    assert cloud_align.solve_from_moments(n, m) is not None
    assert cloud_align.solve_from_moments(2, m) is None and cloud_align.solve_from_moments(0, np.zeros(17)) is None      # n < 3
    same = np.tile([[1.0, 2.0, 3.0]], (10, 1))
    m, n, _ = _moments_of_pairs(same, p)                               # all p in one point: sigma = 0 (or below, by rounding)
    assert cloud_align.solve_from_moments(n, m) is None
    for slot, value in ((0, np.nan), (7, np.inf), (15, -np.inf), (16, np.nan)):
        broken = _moments_of_pairs(p, p)[0]
        broken[slot] = value
        assert cloud_align.solve_from_moments(10, broken) is None
    with pytest.raises(ValueError):
        cloud_align.solve_from_moments(10, np.zeros(16))


def test_similarity_from_poses_recovers_the_planted_transform():
    c, R, t = U.planted("large")
    gt = U.trajectory()
    own = U.carried(gt, c, R, t)
    gc, gR, gt_t = cloud_align.similarity_from_poses(own, gt)
    assert abs(gc - c) <= RTOL * c and np.abs(gR - R).max() <= RTOL and np.abs(gt_t - t).max() <= RTOL * max(1.0, np.abs(t).max())
    assert cloud_align.similarity_from_poses(own, gt, with_scale=False)[0] == 1.0
    four = np.tile(np.eye(4), (len(gt), 1, 1))
    four[:, :3] = own
    assert np.array_equal(cloud_align.similarity_from_poses(four, gt)[1], gR)      # [m,4,4] is read like [m,3,4]
    with pytest.raises(ValueError):
        cloud_align.similarity_from_poses(own[:2], gt[:2])
    with pytest.raises(ValueError):
        cloud_align.similarity_from_poses(np.zeros_like(own), gt)      # every centre in one point


def _recovered(result, planted):
    c, R, t = planted
    return abs(result.scale - c) <= RTOL * c and np.abs(result.R - R).max() <= RTOL and np.abs(result.t - t).max() <= RTOL * max(1.0, np.abs(t).max())


def test_street_similarity_is_recovered():
    pred, ref, planted = U.street_pair("small")
    assert ref.shape == (9200, 3) and len(pred) == 6134
    tau = U.STREET_TAU
    result = cloud_align.align_numpy(pred, ref, tau)
    print("passes %d, scale err %.3g, R err %.3g, t err %.3g" % (result.iterations, abs(result.scale - planted[0]) / planted[0],
                                                                  np.abs(result.R - planted[1]).max(), np.abs(result.t - planted[2]).max()))
    assert result.converged and result.iterations == len(result.history) <= 30
    assert _recovered(result, planted)
    assert result.history[-1][0] == len(pred) and result.history[0][0] < len(pred) and result.history[-1][1] < 1e-9 < result.history[0][1]
    before = cloud_eval.compare_numpy(pred, ref, tau)
    after = cloud_eval.compare_numpy(cloud_align.transform_numpy(pred, result.scale, result.R, result.t), ref, tau)
    assert after.thresholds[0] == tau / 4 and after.precision[0] == 1.0 and before.precision[0] < 0.5
    # the class on the host is the function, and two runs are one
    again = cloud_align.CloudAligner("cpu", tau).align(pred, ref)
    assert again.scale == result.scale and np.array_equal(again.R, result.R) and np.array_equal(again.t, result.t) and again.history == result.history


def test_street_passes_run_out_and_stride_and_trim():
    pred, ref, planted = U.street_pair("large")
    tau = U.STREET_TAU
    full = cloud_align.align_numpy(pred, ref, tau)
    assert full.converged and 10 < full.iterations <= 30 and _recovered(full, planted)
    short = cloud_align.align_numpy(pred, ref, tau, iters=10)
    assert not short.converged and short.iterations == 10 and short.history == full.history[:10]
    assert np.isfinite(short.scale) and np.isfinite(short.R).all() and np.isfinite(short.t).all() and not _recovered(short, planted)
    none = cloud_align.align_numpy(pred, ref, tau, iters=0)
    assert none.iterations == 0 and not none.converged and none.scale == 1.0 and np.array_equal(none.R, np.eye(3))
    strided = cloud_align.align_numpy(pred, ref, tau, stride=3)
    assert strided.converged and strided.history[-1][0] == len(pred[::3]) and _recovered(strided, planted)
    trimmed = cloud_align.align_numpy(pred, ref, tau, trim=tau / 2)
    assert trimmed.history[0][0] < full.history[0][0] and trimmed.history[0][1] < full.history[0][1]
    # a good initial guess is a fixed point: one pass, and the step is the identity
    at_once = cloud_align.align_numpy(pred, ref, tau, init=planted)
    assert at_once.converged and at_once.iterations == 1 and _recovered(at_once, planted)
    for bad in (dict(mode="affine"), dict(stride=0), dict(iters=-1), dict(trim=-1.0), dict(tol=-1.0)):
        with pytest.raises(ValueError):
            cloud_align.align_numpy(pred, ref, tau, **bad)
    with pytest.raises(ValueError):
        cloud_align.align_numpy(pred, ref, tau, init=(0.0, np.eye(3), np.zeros(3)))


def test_rigid_mode_keeps_the_scale_at_exactly_one():
    _, ref, (_, R, t) = U.street_pair("small")
    moved = (ref[::2] - t).dot(R)                                      # a rigidly moved copy of half the reference
    result = cloud_align.align_numpy(moved, ref, U.STREET_TAU, mode="rigid")
    assert result.scale == 1.0 and result.converged and _recovered(result, (1.0, R, t))


def test_a_degenerate_pass_keeps_the_last_good_transform():
    ref = U.street()
    far = ref[:50] + 100.0                                             # nothing within tau: no row is matched
    result = cloud_align.align_numpy(far, ref, U.STREET_TAU, init=(1.0, np.eye(3), np.array([0.0, 0.5, 0.0])))
    assert not result.converged and result.iterations == 1 and result.history == ((0, 0.0),)
    assert result.scale == 1.0 and np.array_equal(result.R, np.eye(3)) and np.array_equal(result.t, [0.0, 0.5, 0.0])
    empty = cloud_align.align_numpy(np.zeros((0, 3)), ref, U.STREET_TAU)
    assert not empty.converged and empty.history == ((0, 0.0),)


# ---- the script ----------------------------------------------------------------------------------------------------------------------

def _street_tree(tmp_path):
    """A KITTI odometry tree whose four scans carry the street between them, the predicted cloud (the planted transform's inverse
    image of part of it, as a PLY in float32) and the poses it would have been fused with."""
    ref, (c, R, t) = U.street(), U.planted("small")
    poses = np.zeros((4, 3, 4))
    for s in range(4):
        poses[s, :, :3] = np.eye(3)
        poses[s, :, 3] = [1.5 + 2.0 * (s % 2), 1.0 + 0.5 * (s // 2), -30.0 + 1.5 * s]
    scans = []
    for s in range(4):
        cam = ref[s::4] - poses[s, :, 3]
        velo = (cam - E.TR[:, 3]).dot(E.TR[:, :3])                      # the inverse of TR: its 3x3 is orthonormal
        scans.append(np.concatenate([velo, np.full((len(velo), 1), 0.5)], 1).astype(np.float32))
    root = str(tmp_path / "odom")
    poses_file = E.write_odometry_tree(root, scans, poses)
    pred = ((ref[np.arange(len(ref)) % 3 != 2] - t).dot(R) / c).astype(np.float32)
    cloud_ply = str(tmp_path / "cloud.ply")
    cloud.save_ply(cloud_ply, pred, np.full((len(pred), 3), 7, np.uint8), np.ones(len(pred), np.int32))
    own_file = str(tmp_path / "own_poses.txt")
    odometry.save_kitti_poses(own_file, U.carried(poses, c, R, t))
    return root, scans, poses_file, own_file, cloud_ply, pred


def test_script_aligns_on_a_synthetic_odometry_tree(tmp_path):
    root, scans, poses_file, own_file, cloud_ply, pred = _street_tree(tmp_path)
    tau = 0.3
    transform_txt, aligned_ply = str(tmp_path / "out/T.txt"), str(tmp_path / "out/aligned.ply")
    common = [sys.executable, os.path.join(ROOT, "scripts", "eval_cloud.py"), "--cloud", cloud_ply, "--tau", str(tau), "--device", "cpu",
              "--data_path", root, "--sequence", "9", "--poses", poses_file, "--ref_voxel", "0.1", "--min_depth", "1", "--max_range", "80"]
    flags = ["--align", "similarity", "--init_poses", own_file, "--save_transform", transform_txt, "--save_aligned", aligned_ply]
    run = subprocess.run(common + flags, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    gt = odometry.load_kitti_poses(poses_file)
    ref = cloud_eval.ScanFuser("cpu", 0.1, E.TR, min_depth=1.0, max_range=80.0).fuse(scans, gt)
    assert ref.stats["valid"] == 9200
    init = cloud_align.similarity_from_poses(odometry.load_kitti_poses(own_file), gt)
    want = cloud_align.align_numpy(pred, ref.xyz, 2 * tau, init=init)                       # --align_tau defaults to 2 tau
    assert want.converged and abs(want.scale - 1.02) < 1e-3 and abs(init[0] - 1.02) < 1e-3   # float32 clouds, %1.8e poses, voxel means
    fmt = lambda v: " ".join("%.9g" % x for x in np.reshape(v, -1))
    assert "initial scale %.9g R %s t %s" % (init[0], fmt(init[1]), fmt(init[2])) in lines
    for n, (matched, rms) in enumerate(want.history):
        assert "pass %d: matched %d rms %.6g" % (n, matched, rms) in lines
    assert "scale %.9g R %s t %s" % (want.scale, fmt(want.R), fmt(want.t)) in lines
    assert "converged True after %d passes" % want.iterations in lines
    aligned = cloud_align.transform_numpy(pred, want.scale, want.R, want.t)
    scores = cloud_eval.compare_numpy(aligned, ref.xyz, tau)
    for th, p, r, f in zip(scores.thresholds, scores.precision, scores.recall, scores.fscore):
        assert "aligned threshold %.6g: precision %.4f recall %.4f fscore %.4f" % (th, p, r, f) in lines
    assert "aligned accuracy %.6g completeness %.6g (tau %.6g)" % (scores.accuracy, scores.completeness, tau) in lines
    assert scores.precision[-1] == 1.0 and cloud_eval.compare_numpy(pred, ref.xyz, tau).precision[-1] < 0.95
    assert not [l for l in lines if l.startswith(("threshold", "accuracy"))]               # nothing unlabelled
    assert np.array_equal(np.loadtxt(transform_txt), cloud_align.matrix(want.scale, want.R, want.t))
    saved = cloud.load_ply(aligned_ply)
    assert np.array_equal(np.stack([saved["x"], saved["y"], saved["z"]], 1), aligned.astype(np.float32)) and (saved["red"] == 7).all()
    # rigid: the scale stays --pred_scale, and the trajectories are aligned at that scale
    rigid = subprocess.run(common + ["--align", "rigid", "--init_poses", own_file, "--pred_scale", "1.02"], env=dict(os.environ, PYTHONPATH=ROOT),
                           capture_output=True, text=True, timeout=600)
    assert rigid.returncode == 0, rigid.stdout + rigid.stderr
    own = odometry.load_kitti_poses(own_file)
    own[:, :, 3] *= 1.02
    _, R0, t0 = cloud_align.similarity_from_poses(own, gt, with_scale=False)
    want = cloud_align.align_numpy(pred, ref.xyz, 2 * tau, mode="rigid", init=(1.02, R0, t0))
    assert want.converged and want.scale == 1.02
    assert "scale %.9g R %s t %s" % (want.scale, fmt(want.R), fmt(want.t)) in rigid.stdout.splitlines()
    assert "aligned threshold %.6g: precision 1.0000 recall" % tau in rigid.stdout
    # the flags that depend on --align are refused without it
    lone = subprocess.run(common + ["--save_transform", transform_txt], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                          timeout=600)
    assert lone.returncode == 2 and "--align" in lone.stderr


def test_script_without_align_prints_what_it_printed_before(tmp_path):
    """The whole of stdout, rebuilt here from the statements with the format strings the script has had since it was added."""
    pred, ref, _ = U.street_pair("small")
    cloud_ply, ref_ply = str(tmp_path / "cloud.ply"), str(tmp_path / "ref.ply")
    for path, xyz in ((cloud_ply, pred), (ref_ply, ref)):
        cloud.save_ply(path, xyz.astype(np.float32), np.zeros((len(xyz), 3), np.uint8), np.ones(len(xyz), np.int32))
    tau = U.STREET_TAU
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "eval_cloud.py"), "--cloud", cloud_ply, "--ref", ref_ply, "--tau", str(tau),
                          "--pred_scale", "1.02", "--device", "cpu"], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want = cloud_eval.compare_numpy(pred.astype(np.float32), ref.astype(np.float32), tau, pred_scale=1.02)
    text = "-> Reference cloud %s: %d points\n" % (ref_ply, len(ref))
    for name, n, grid in (("predicted", "n_pred", "pred_grid"), ("reference", "n_ref", "ref_grid")):
        text += "%s cloud: %d points, dropped %d, cells %d, max_cell %d\n" % (
            name, want.stats[n], want.stats[grid]["dropped"], want.stats[grid]["cells"], want.stats[grid]["max_cell"])
    for t, p, r, f in zip(want.thresholds, want.precision, want.recall, want.fscore):
        text += "threshold %.6g: precision %.4f recall %.4f fscore %.4f\n" % (t, p, r, f)
    text += "accuracy %.6g completeness %.6g (tau %.6g)\n" % (want.accuracy, want.completeness, tau)
    assert run.stdout == text


# ---- the C entry points ----------------------------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    f64, i64 = (ctypes.c_double * 64)(), (ctypes.c_longlong * 8)()
    eye = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    move = lambda **kw: lib.td_cloud_transform(*[kw.get(k, d) for k, d in (
        ("src", p(f64)), ("N", 2), ("c", 1.0), ("R", eye), ("t", (ctypes.c_double * 3)()), ("out", p(f64)), ("stream", None))])
    for bad in (dict(src=None), dict(R=None), dict(t=None), dict(out=None), dict(N=-1), dict(c=nan), dict(c=inf),
                dict(R=(ctypes.c_double * 9)(1, 0, 0, 0, nan, 0, 0, 0, 1)), dict(t=(ctypes.c_double * 3)(0, 0, inf))):
        assert move(**bad) == -1, bad
    assert move(N=0) == 0                                              # a successful no-op: nothing is launched
    assert [lib.td_icp_moments_workspace(n) for n in (-1, 0, 1, 256, 257, 65537)] == [0, 0, 136, 136, 272, 257 * 136]
    sums = lambda **kw: lib.td_icp_moments(*[kw.get(k, d) for k, d in (
        ("cur", p(f64)), ("N", 2), ("ref", p(f64)), ("M", 2), ("index", p(i64)), ("d2", p(f64)), ("trim2", 0.25),
        ("origin", (ctypes.c_double * 3)()), ("workspace", p(f64)), ("workspace_bytes", 136), ("out", p(f64)), ("stream", None))])
    for bad in (dict(cur=None), dict(ref=None), dict(index=None), dict(d2=None), dict(origin=None), dict(workspace=None), dict(out=None),
                dict(N=-1), dict(M=-1), dict(trim2=-1.0), dict(trim2=nan), dict(origin=(ctypes.c_double * 3)(0, nan, 0)),
                dict(origin=(ctypes.c_double * 3)(inf, 0, 0)), dict(workspace_bytes=-1),
                dict(out=ctypes.c_void_p(ctypes.addressof(f64) + 4)), dict(workspace=ctypes.c_void_p(ctypes.addressof(f64) + 4))):
        assert sums(**bad) == -1, bad
    assert sums(workspace_bytes=135) == -4 and sums(N=257, workspace_bytes=271) == -4      # TD_ERR_WORKSPACE, before any launch
    # N = 0 is accepted with nothing but origin and out, but it is no no-op: it clears out, so it succeeds where there is a device
    # and reports the runtime's error (TD_ERR_LAUNCH, "no ROCm-capable device") where there is none -- never a bad argument
    # (with a device the call would clear ``out``, which is host memory here: tests/test_hip_cloud_align.py makes it on device memory)
    if not torch.cuda.is_available():
        assert sums(N=0, cur=None, index=None, d2=None, workspace=None, workspace_bytes=0, ref=None, M=0) == -3
        assert b"td_icp_moments (clear)" in lib.td_last_hip_error()
    with pytest.raises(native.NativeLibraryError):
        cloud_align.transform_hip(torch.zeros(4, 3, dtype=torch.float64), 1.0, np.eye(3), np.zeros(3))
    with pytest.raises(native.NativeLibraryError):
        cloud_align.moments_hip(torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, dtype=torch.int64),
                                torch.zeros(4, dtype=torch.float64), 0.25, np.zeros(3))
