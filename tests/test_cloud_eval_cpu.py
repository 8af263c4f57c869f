"""The host statements of tripled_amd.cloud_eval, pinned: nearest_numpy (the sorted grid) by the all-pairs nearest_bruteforce on the bits
of d2 and on the indices, scan_keys_numpy by a literal per-point loop, the scores by an analytic wall, scripts/eval_cloud.py end to end
on a tiny synthetic odometry tree.  The C entry points refuse bad arguments before any launch, which a CPU host can check.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import tripled_amd  # noqa: F401
from tripled_amd import cloud, cloud_eval, native, odometry
from tests import cloud_eval_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    assert np.array_equal(a.d2.view(np.uint64), b.d2.view(np.uint64))
    assert np.array_equal(a.index, b.index)
    assert np.array_equal(a.counts, b.counts)


@pytest.mark.parametrize("tau", U.TAUS)
def test_grid_search_is_the_all_pairs_search(tau):
    query, ref = U.nn_scene(tau)
    assert ref.shape == (4097, 3) and query.shape == (1000, 3)
    thresholds = (tau / 4, tau / 2, tau)
    want = cloud_eval.nearest_bruteforce(query, ref, tau, thresholds)
    got = cloud_eval.nearest_numpy(query, ref, tau, thresholds)
    _same(got, want)
    # the inputs exercise the outcomes
    found = want.index >= 0
    assert found.any() and (~found).any() and want.counts[3] == found.sum() and want.counts[4] == 4
    assert np.isinf(want.d2[~found]).all() and (want.d2[found] == 0).any()
    assert 0 < want.counts[0] < want.counts[1] < want.counts[2] == want.counts[3]
    corners, centres = U.lattice(tau)
    assert found[:len(centres)].all()                                  # every cube centre has its eight corners at equal distance
    assert U.ties_broken_by_index(query[:len(centres)], ref, tau) == len(centres)
    for q, j in zip(centres[:8], want.index[:8]):                      # ... and the lowest index of the eight wins
        e = ref - q
        d2 = ((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2])
        assert j == np.nonzero(d2 == d2.min())[0][0] and np.count_nonzero(d2 == d2.min()) == 8
    # the copies moved by tau along an axis: the neighbour is one cell over, at the radius, found or not by the rounded d2 alone
    sparse = slice(len(centres) + len(corners[::7]), len(centres) + len(corners[::7]) + 96)
    assert found[sparse].any()
    # a pre-built grid gives the same answer, and its statistics add up
    grid = cloud_eval.grid_numpy(ref, tau)
    _same(cloud_eval.nearest_numpy(query, grid, tau, thresholds), want)
    assert grid.stats["points"] == 4097 and grid.stats["dropped"] == 0 and grid.stats["cells"] == len(grid.cell_key)
    assert grid.stats["max_cell"] == np.diff(grid.cell_start).max() and grid.cell_start[-1] == 4097
    assert np.array_equal(np.sort(grid.order), np.arange(4097))


def test_grid_drops_what_has_no_cell_and_thresholds_are_checked():
    tau = 0.25
    ref = np.array([[0.0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [2.0 ** 21, 0, 0], [0.1, 0, 0]])
    grid = cloud_eval.grid_numpy(ref, tau)
    assert grid.stats == {"points": 5, "dropped": 3, "cells": 1, "max_cell": 2} and np.array_equal(grid.order, [0, 4])
    nb = cloud_eval.nearest_numpy(np.array([[0.06, 0, 0]]), grid, tau, (tau,))
    assert nb.index[0] == 4 and np.array_equal(nb.counts, [1, 1, 0])
    empty = cloud_eval.nearest_numpy(np.zeros((2, 3)), np.zeros((0, 3)), tau)
    assert np.isinf(empty.d2).all() and (empty.index == -1).all() and np.array_equal(empty.counts, [0, 0, 0, 0, 0])
    assert cloud_eval.nearest_numpy(np.zeros((0, 3)), ref, tau).d2.shape == (0,)
    for bad in ((0.3,), (0.2, 0.1), (-0.1,), tuple([0.1] * 17)):
        with pytest.raises(ValueError):
            cloud_eval.nearest_numpy(ref, ref, tau, bad)
    with pytest.raises(ValueError):
        cloud_eval.nearest_numpy(ref, grid, 0.5)                       # a grid built for another radius
    with pytest.raises(ValueError):
        cloud_eval.grid_numpy(ref, 0.0)


@pytest.mark.parametrize("view", [False, True])
def test_scan_keys_are_the_per_point_loop(view):
    points, offsets, poses = U.scan_batch()
    camera = dict(K=U.scan_K(), height=U.SCAN_H, width=U.SCAN_W) if view else {}
    want = U.scan_keys_loop(points, offsets, U.TR, poses, **camera, **U.SCAN_PARAMS)
    got = cloud_eval.scan_keys_numpy(points, offsets, U.TR, poses, **camera, **U.SCAN_PARAMS)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    counts = got[2]
    assert counts.sum() == len(points) == 1066 and offsets[0] == offsets[1] == 0          # one empty scan in the batch
    assert counts[0] > 0 and counts[1] == 6 and counts[2] > 0 and (counts[3] > 0) == view and counts[4] > 0
    # reflectance: NaN and negative -> 0, above 1 and inf -> 255, 0.5 -> 128
    at = int(offsets[2])                                               # the scan of 65 points: its planted points stay in key range
    grey = [(int(got[1][at + i]) >> 30) & 255 for i in (9, 11, 13, 15, 17)]
    assert grey == [0, 0, 255, 255, 128] and all(got[0][at + i] != cloud.INVALID_KEY for i in (9, 11, 13, 15, 17))
    with pytest.raises(ValueError):
        cloud_eval.scan_keys_numpy(points, offsets[::-1].copy(), U.TR, poses, **U.SCAN_PARAMS)
    with pytest.raises(ValueError):
        cloud_eval.scan_keys_numpy(points, offsets, U.TR, poses, height=4, width=4, **U.SCAN_PARAMS)      # a view test without K


def test_scan_fuser_on_the_host_is_the_statement_chain():
    points, offsets, poses = U.scan_batch()
    scans = [points[offsets[s]:offsets[s + 1]] for s in range(4)]
    fuser = cloud_eval.ScanFuser("cpu", U.SCAN_VOXEL, U.TR, K=U.scan_K(), height=U.SCAN_H, width=U.SCAN_W, min_depth=1.0, max_range=45.0,
                                 batch_size=2)
    got = fuser.fuse(scans, poses)
    key, payload, counts = cloud_eval.scan_keys_numpy(points, offsets, U.TR, poses, K=U.scan_K(), height=U.SCAN_H, width=U.SCAN_W,
                                                      **U.SCAN_PARAMS)
    keys, sums = cloud.voxel_table_numpy(key, payload)
    xyz, rgb, count, _ = cloud.finish_numpy(keys, sums, U.SCAN_VOXEL)
    assert np.array_equal(got.keys, keys) and np.array_equal(got.xyz.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(got.rgb, rgb) and np.array_equal(got.count, count) and (rgb[:, 0] == rgb[:, 2]).all()
    assert got.stats == dict(points=1066, voxels=len(keys), **{n: int(c) for n, c in zip(cloud_eval.SCAN_CAUSES, counts)})


def test_wall_scores_one_and_a_shifted_wall_scores_zero():
    scans, poses = U.wall_scans()
    ref = cloud_eval.ScanFuser("cpu", U.WALL_VOXEL, U.TR, min_depth=1.0, max_range=20.0).fuse(scans, poses)
    assert ref.stats["valid"] == ref.stats["points"] == sum(len(s) for s in scans)
    assert np.abs(ref.xyz[:, 2] - U.WALL_Z).max() < 1e-3 and ref.xyz[:, 0].min() < -3.9 and ref.xyz[:, 0].max() > 3.9
    pred = U.wall_prediction()
    comparer = cloud_eval.CloudComparer("cpu", U.WALL_TAU)
    same = comparer.compare(pred, ref.xyz)
    assert same.thresholds == (U.WALL_TAU / 4, U.WALL_TAU / 2, U.WALL_TAU)
    assert same.precision[-1] == 1.0 and same.recall[-1] == 1.0 and same.fscore[-1] == 1.0
    assert same.pred.counts[3] == len(pred) and same.ref.counts[3] == len(ref.xyz) and same.pred.counts[4] == 0
    assert 0 < same.accuracy < U.WALL_VOXEL and 0 < same.completeness < U.WALL_VOXEL
    assert same.precision[0] <= same.precision[1] <= 1.0
    shifted = pred + np.array([0, 0, 2 * U.WALL_TAU], np.float32)
    apart = comparer.compare(shifted, ref.xyz)
    assert apart.precision == (0.0, 0.0, 0.0) and apart.recall == (0.0, 0.0, 0.0) and apart.fscore == (0.0, 0.0, 0.0)
    assert apart.accuracy == U.WALL_TAU and apart.completeness == U.WALL_TAU
    assert (apart.pred.index == -1).all() and np.isinf(apart.ref.d2).all()
    # pred_scale is the only alignment: the wall at half its size, scaled back
    _same(comparer.compare(pred * np.float32(0.5), ref.xyz, pred_scale=2.0).pred, same.pred)
    colors = cloud_eval.error_colors(apart.pred.d2, apart.pred.index, U.WALL_TAU)
    assert (colors == cloud_eval.NOT_FOUND_RGB).all()
    assert not (cloud_eval.error_colors(same.pred.d2, same.pred.index, U.WALL_TAU) == cloud_eval.NOT_FOUND_RGB).all(1).any()


def test_script_on_a_synthetic_odometry_tree(tmp_path):
    scans, poses = U.wall_scans()
    root = str(tmp_path / "odom")
    poses_file = U.write_odometry_tree(root, scans, poses)
    pred = U.wall_prediction()
    cloud_ply, ref_ply, err_ply = (str(tmp_path / n) for n in ("cloud.ply", "out/ref.ply", "out/error.ply"))
    cloud.save_ply(cloud_ply, pred, np.full((len(pred), 3), 7, np.uint8), np.ones(len(pred), np.int32))
    common = [sys.executable, os.path.join(ROOT, "scripts", "eval_cloud.py"), "--cloud", cloud_ply, "--tau", str(U.WALL_TAU), "--device", "cpu"]
    lidar = ["--data_path", root, "--sequence", "9", "--poses", poses_file, "--ref_voxel", str(U.WALL_VOXEL), "--min_depth", "1",
             "--max_range", "20", "--batch_size", "2", "--save_ref", ref_ply, "--save_error", err_ply]
    run = subprocess.run(common + lidar, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want_ref = cloud_eval.ScanFuser("cpu", U.WALL_VOXEL, U.TR, min_depth=1.0, max_range=20.0).fuse(scans, odometry.load_kitti_poses(poses_file))
    want = cloud_eval.compare_numpy(pred, want_ref.xyz, U.WALL_TAU)
    lines = run.stdout.splitlines()
    for cause in ("points",) + cloud_eval.SCAN_CAUSES + ("voxels",):
        assert "scans %s %d" % (cause, want_ref.stats[cause]) in lines
    assert "predicted cloud: %d points, dropped 0, cells %d, max_cell %d" % (
        len(pred), want.stats["pred_grid"]["cells"], want.stats["pred_grid"]["max_cell"]) in lines
    assert "threshold %.6g: precision 1.0000 recall 1.0000 fscore 1.0000" % U.WALL_TAU in lines
    assert "accuracy %.6g completeness %.6g (tau %.6g)" % (want.accuracy, want.completeness, U.WALL_TAU) in lines
    saved = cloud.load_ply(ref_ply)
    assert np.array_equal(saved["x"], want_ref.xyz[:, 0]) and np.array_equal(saved["count"], want_ref.count)
    err = cloud.load_ply(err_ply)
    colors = cloud_eval.error_colors(want.pred.d2, want.pred.index, U.WALL_TAU)
    assert np.array_equal(err["x"], pred[:, 0]) and np.array_equal(np.stack([err["red"], err["green"], err["blue"]], 1), colors)
    # the same scores from the saved reference
    again = subprocess.run(common + ["--ref", ref_ply], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert again.returncode == 0, again.stdout + again.stderr
    assert [l for l in again.stdout.splitlines() if l.startswith(("threshold", "accuracy"))] == \
        [l for l in lines if l.startswith(("threshold", "accuracy"))]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    f32, f64, i64 = (ctypes.c_float * 8)(), (ctypes.c_double * 36)(), (ctypes.c_longlong * 20)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    scan = lambda **kw: lib.td_scan_keys(*[kw.get(k, d) for k, d in (
        ("points", p(f32)), ("n", 2), ("offsets", p(i64)), ("S", 1), ("Tr", f64), ("poses", p(f64)), ("K", f64), ("H", 4), ("W", 4),
        ("min_depth", 0.1), ("max_range", 1.0), ("inv_voxel", 10.0), ("key", p(i64)), ("payload", p(i64)), ("stats", None), ("stream", None))])
    for bad in (dict(points=None), dict(offsets=None), dict(Tr=None), dict(poses=None), dict(K=None), dict(key=None), dict(payload=None),
                dict(n=-1), dict(S=0), dict(H=-1), dict(W=-1), dict(W=0), dict(inv_voxel=0.0), dict(inv_voxel=float("nan")),
                dict(min_depth=2.0)):
        assert scan(**bad) == -1, bad
    assert scan(n=0) == 0 and scan(n=0, K=None, H=0, W=0) == 0                  # a successful no-op: nothing is launched
    nn = lambda **kw: lib.td_nn_query(*[kw.get(k, d) for k, d in (
        ("query", p(f64)), ("N", 2), ("points", p(f64)), ("order", p(i64)), ("M", 2), ("cell_key", p(i64)), ("cell_start", p(i64)), ("C", 1),
        ("tau", 0.5), ("thr2", f64), ("K", 3), ("d2", p(f64)), ("index", p(i64)), ("counts", p(i64)), ("stream", None))])
    for bad in (dict(query=None), dict(points=None), dict(order=None), dict(cell_key=None), dict(cell_start=None), dict(thr2=None),
                dict(d2=None), dict(index=None), dict(counts=None), dict(N=-1), dict(M=-1), dict(C=-1), dict(C=3), dict(K=17), dict(K=-1),
                dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf"))):
        assert nn(**bad) == -1, bad
    assert nn(N=0) == 0 and nn(N=0, M=0, C=0, points=None, order=None, cell_key=None, K=0, thr2=None) == 0
    import torch
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.grid_hip(torch.zeros(4, 3, dtype=torch.float64), 0.5)
    with pytest.raises(native.NativeLibraryError):
        cloud_eval.scan_keys_hip(torch.zeros(2, 4), torch.tensor([0, 2]), U.TR, torch.zeros(1, 3, 4, dtype=torch.float64))
