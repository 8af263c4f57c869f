"""The TSDF ray cast without a GPU (tripled_amd.tsdf: raycast_numpy, raycast_bruteforce, TsdfCaster, save_map / load_map): the numpy
statement against the literal brute force (plain Python floats and a dict), every branch of the walk reached and asserted through
the counters, a noise-free plane against the analytic ray-plane depth within a derived bound, the caster's independence of its
batches, the map on disk, TsdfFuser.map, the argument checks of td_tsdf_cast and the two programs on a tiny tree.  Everything but the
plane's bound is exact."""
import ctypes
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, native, render, tsdf
from tests import odom_util
from tests import tsdf_cast_util as C
from tests import tsdf_util as U
from tests.infer_util import build_model, ROOT

VOXEL = C.VOXEL


def both(keys, sums, poses, H, W, ik=None, **over):
    """raycast_numpy, checked against raycast_bruteforce bit for bit."""
    args = dict(C.CAST, **over)
    ik = C.inv_K(H, W) if ik is None else ik
    got = tsdf.raycast_numpy(keys, sums, poses, ik, H, W, VOXEL, **args)
    want = tsdf.raycast_bruteforce(U.table_of_rows(keys, sums), poses, ik, H, W, VOXEL, **args)
    C.assert_casts_equal(got, want)
    C.assert_stats_consistent(got, H, W)
    assert got.depth.dtype == np.float32 and got.normal.shape == (len(poses), 3, H, W) and got.color.dtype == np.uint8
    assert got.weight.dtype == np.int32 and got.stats.dtype == np.int64 and got.stats.shape == (len(poses), len(tsdf.CAST_STATS))
    return got


# ---- 1. the statement against the brute force -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cameras", [1, 3])
def test_slab_is_the_brute_force(n_cameras):
    keys, sums = C.slab(6, 5, 8)
    got = both(keys, sums, C.cameras_in_front(keys, n_cameras), 9, 13)
    assert got.stats[:, 1].min() > 0 and got.stats[:, 3].min() > 0          # every camera hits and misses
    lengths = np.linalg.norm(got.normal.astype(np.float64), axis=1)
    assert np.all((np.abs(lengths - 1.0) < 1e-6) | (lengths == 0.0))
    assert np.all(got.normal[:, 2][got.depth > 0] <= 0)                     # the slab's distance falls along +z, the cameras look along +z


@pytest.mark.parametrize("V,n_cameras", [(1, 1), (7, 3), (60, 1), (400, 3)])
def test_sparse_maps_are_the_brute_force(V, n_cameras):
    keys, sums = C.sparse_map(V, seed=V)
    got = both(keys, sums, C.cameras_in_front(keys, n_cameras, seed=V, back=3.0), 7, 11, far=30.0)
    assert got.stats[:, 0].sum() == n_cameras * 77      # (at 30 % fill a full corner set is rare: these maps are mostly unknown space)


def test_slab_with_holes_breaks_pairs():
    keys, sums = C.holed_slab()
    full_keys, full_sums = C.slab(7, 6, 8, seed=1)
    poses = C.cameras_in_front(full_keys, 3, seed=2)
    got = both(keys, sums, poses, 9, 13)
    full = tsdf.raycast_numpy(full_keys, full_sums, poses, C.inv_K(9, 13), 9, 13, VOXEL, **C.CAST)
    # a missing voxel makes the samples around it unknown: rays that hit the full slab lose their pair and run on
    assert 0 < got.stats[:, 1].sum() < full.stats[:, 1].sum() and got.stats[:, 3].sum() > full.stats[:, 3].sum()


def test_field_ends_are_the_brute_force():
    keys, sums = C.field_ends_map(63)
    got = both(keys, sums, C.field_end_cameras(), 5, 7, far=24.0)
    assert got.stats[:, 0].sum() == 3 * 35
    # the first camera's central ray walks the column x = y = -2^20 up to z = 2^20 - 1 and on: the sample whose +z corner would be the
    # NEXT column's first voxel (its key is the last voxel's key + 1, and it is in the map) is unknown
    ix = iy = -cloud.HALF
    last, first_of_next = cloud.pack_key(ix, iy, cloud.HALF - 1), cloud.pack_key(ix, iy + 1, -cloud.HALF)
    assert first_of_next == last + 1 and last in keys and first_of_next in keys
    qualifies = np.ones(len(keys), bool)
    g = [np.array([ix + 0.7]), np.array([iy + 0.7]), np.array([cloud.HALF - 0.3])]
    assert not tsdf._corners_numpy(keys, qualifies, g)[0][0]
    g[2] = np.array([cloud.HALF - 1.3])
    assert tsdf._corners_numpy(keys, qualifies, g)[0][0]
    # the corner set that contains the sentinel voxel is unknown although the other seven voxels exist
    g = [np.array([cloud.HALF - 1.3])] * 3
    assert not tsdf._corners_numpy(keys, qualifies, g)[0][0]


@pytest.mark.parametrize("n_cameras", [1, 3])
def test_fused_scene_is_the_brute_force(n_cameras):
    keys, sums, poses, _ = C.fused_map()
    assert len(keys) > 100
    got = both(keys, sums, poses[:n_cameras], 8, 12, far=20.0)
    assert got.stats[0, 1] > 0
    if n_cameras == 3:
        assert got.stats[2, 3] == 96                                        # the last frame stands beyond +-2^20 voxels: nothing is known


# ---- 2. each branch, asserted through the counters --------------------------------------------------------------------------------------

def flat_band(nz=6, z0=4, n=4, w=2, sign=1):
    """n x n columns of nz voxels whose distance falls (sign = 1) or rises along z, zero between voxels z0 + nz/2 - 1 and z0 + nz/2."""
    cells = {}
    for x in range(-n, n):
        for y in range(-n, n):
            for z in range(nz):
                d = sign * (nz / 2.0 - z - 0.5) / nz
                cells[(x, y, z0 + z)] = (w, int(round(d * U.ONE)) * w, 10 * w, 20 * w, 30 * w)
    return cells


def centre_ray(keys, sums, eye, R=C.FORWARD, **over):
    """One pixel whose ray is the camera's axis (inv_K = 1)."""
    return both(keys, sums, C.pose(eye, R)[None], 1, 1, ik=np.eye(3), **over)


def test_hit_backface_and_miss():
    keys, sums = U.hand_map(flat_band())
    hit = centre_ray(keys, sums, [0.0, 0.0, 0.0])
    assert list(hit.stats[0]) == [1, 1, 0, 0, 0]
    # the zero lies between the centres of voxels 6 and 7, at z = 7 voxels; the field is linear in z: the depth is exact
    assert hit.depth[0, 0, 0] == np.float32(7.0 * VOXEL) and list(hit.normal[0, :, 0, 0]) == [0.0, 0.0, -1.0]
    assert list(hit.color[0, :, 0, 0]) == [10, 20, 30] and hit.weight[0, 0, 0] == 2
    behind = centre_ray(keys, sums, [0.0, 0.0, 14.0], C.BACKWARD)           # the camera behind the slab looks back at it
    assert list(behind.stats[0]) == [1, 0, 1, 0, 0] and behind.depth[0, 0, 0] == 0 and behind.weight[0, 0, 0] == 0
    away = centre_ray(keys, sums, [0.0, 0.0, 0.0], C.BACKWARD, background=(7, 8, 9))
    assert list(away.stats[0]) == [1, 0, 0, 1, 0] and list(away.color[0, :, 0, 0]) == [7, 8, 9]


def test_camera_inside_the_band_and_the_last_sample():
    keys, sums = U.hand_map(flat_band())
    # the eye stands behind the zero: the first known sample is negative, nothing follows but negative values and the band's end
    inside = centre_ray(keys, sums, [0.0, 0.0, 7.5])
    assert list(inside.stats[0]) == [1, 0, 0, 1, 0]
    # far chosen so that the last sample is the first negative one: samples at 1, 2, ... (voxel 2, step 1); the zero is at 14
    for far, hits in ((14.5, 1), (13.5, 0)):
        got = centre_ray(keys, sums, [0.0, 0.0, 0.0], near=1.25, far=far)
        assert got.stats[0, 1] == hits, (far, got.stats)
    assert tsdf._check_cast(1, 1, VOXEL, 1, 1.25, 14.5, 0.5)[1] == 14        # 1.25 + 13 = 14.25: the last sample, just behind the zero


def test_one_sample_empty_map_and_nan_pose():
    keys, sums = U.hand_map(flat_band())
    one = centre_ray(keys, sums, [0.0, 0.0, 0.0], near=13.0, far=13.0)
    assert tsdf._check_cast(1, 1, VOXEL, 1, 13.0, 13.0, 0.5)[1] == 1 and list(one.stats[0]) == [1, 0, 0, 1, 0]
    empty = both(np.zeros(0, np.int64), np.zeros((0, 7), np.int64), C.cameras_in_front(keys, 3), 3, 4)
    assert np.array_equal(empty.stats, [[12, 0, 0, 12, 0]] * 3) and not empty.depth.any() and not empty.normal.any()
    poses = C.cameras_in_front(keys, 3)
    poses[1, 0, 1] = np.nan
    got = both(keys, sums, poses, 5, 6)
    assert list(got.stats[1]) == [30, 0, 0, 30, 0] and got.stats[0, 1] > 0 and got.stats[2, 1] > 0


def test_hit_without_normal_and_min_weight():
    # A hit's corner set is neither sample's when the ray passes a voxel-centre plane of x between sample s-1 and the hit, and one of
    # z between the hit and sample s: a tilted ray that drifts towards +x.  A voxel that only the hit's set needs can then be taken
    # away (or left with too few samples) without touching the hit: the normal goes, the colour and weight come from sample s.
    cells = flat_band(nz=4, z0=4, n=2)
    keys, sums = U.hand_map(cells)
    R = C.tilt(0.0, 0.5)                                                    # the ray moves towards +x as it goes
    eye = [-1.65, 0.2, 2.2]
    got = centre_ray(keys, sums, eye, R, near=1.0, far=30.0, step_voxels=1.0)
    assert list(got.stats[0]) == [1, 1, 0, 0, 0]                            # the full band: a hit with a normal
    # every voxel that the hit's corner set needs and neither sample's set does, removed in turn, leaves the hit and takes the normal
    table, found = dict(cells), 0
    for cell in sorted(cells):
        less = {k: v for k, v in table.items() if k != cell}
        k2, s2 = U.hand_map(less)
        cast = tsdf.raycast_numpy(k2, s2, C.pose(eye, R)[None], np.eye(3), 1, 1, VOXEL, min_weight=1, near=1.0, far=30.0, step_voxels=1.0)
        if list(cast.stats[0]) == [1, 1, 0, 0, 1]:
            found += 1
            again = centre_ray(k2, s2, eye, R, near=1.0, far=30.0, step_voxels=1.0)
            assert not again.normal.any() and again.depth[0, 0, 0] == got.depth[0, 0, 0] and again.weight[0, 0, 0] == 2
            # the same through min_weight: the voxel stays in the map with one sample, and two are asked
            light = dict(cells)
            light[cell] = (1,) + tuple(v // 2 for v in cells[cell][1:])
            k3, s3 = U.hand_map(light)
            weighed = centre_ray(k3, s3, eye, R, near=1.0, far=30.0, step_voxels=1.0, min_weight=2)
            C.assert_casts_equal(weighed, again)
            assert list(centre_ray(k3, s3, eye, R, near=1.0, far=30.0, step_voxels=1.0, min_weight=1).stats[0]) == [1, 1, 0, 0, 0]
    assert found > 0


def test_parameters_are_checked():
    keys, sums = C.slab(2, 2, 2)
    poses, ik = C.cameras_in_front(keys, 1), C.inv_K(4, 4)
    for bad in (dict(near=0.0), dict(near=5.0, far=4.0), dict(far=math.inf), dict(step_voxels=0.0), dict(step_voxels=math.nan),
                dict(min_weight=0), dict(far=1.0 + 0.5 * VOXEL * tsdf.CAST_MAX_STEPS), dict(background=(0, 0, 256))):
        with pytest.raises(ValueError):
            tsdf.raycast_numpy(keys, sums, poses, ik, 4, 4, VOXEL, **dict(C.CAST, **bad))
    assert tsdf._check_cast(4, 4, VOXEL, 1, 1.0, 1.0 + 0.5 * VOXEL * (tsdf.CAST_MAX_STEPS - 1), 0.5)[1] == tsdf.CAST_MAX_STEPS
    with pytest.raises(ValueError):
        tsdf.raycast_numpy(keys[::-1], sums, poses, ik, 4, 4, VOXEL, **C.CAST)
    with pytest.raises(ValueError):
        tsdf.raycast_numpy(keys, sums, poses[:, :2], ik, 4, 4, VOXEL, **C.CAST)


# ---- 3. the analytic plane ------------------------------------------------------------------------------------------------------------------

def test_noise_free_plane_is_the_analytic_plane():
    """A fronto-parallel plane at the dyadic depth z0 = 6, fused without noise by cameras with R = I and t_z = 0: a sample's distance is
    z0 - (i_z + 0.5) voxel whatever camera and pixel it came from, so a voxel's D is that value rounded to the distance quantum
    q = trunc 2^-20: D = L + e with L linear in z and |e| <= q / 2 =: delta.  Trilinear interpolation reproduces L and is a convex
    combination of the e, so the interpolated value along a ray is lambda(z) = sigma (zc0 - z) + e(z), |e| <= delta, with z the depth
    along the camera's axis, zc0 the analytic depth and sigma = (R_2 . ray) / ray_z the world-z advance per unit of camera depth (the
    ray's obliquity).  The cast interpolates between samples a = z_(s-1) and a + step:
        z_hit - zc0 = ((a - zc0) (e1 - e2) + step e1) / (sigma step + e1 - e2),   |a - zc0| <= step
        |z_hit - zc0| <= 3 delta step / (sigma step - 2 delta)
    Float64 rounding of the fewer than 2^10 operations on values below 2^5 adds less than 2^-38; the float32 output adds half an ulp,
    at most zc0 2^-24.  The normal: a difference of two D has an error of at most 2 delta, the gradient's components are convex
    combinations of such differences, the true gradient is (0, 0, -voxel) per voxel: G = (e0, e1, -voxel + e2) with |e_k| <= 2 delta,
    so each component of G / |G| is within 2 delta / (voxel - 2 delta) of (0, 0, -1) (the third by less: it is second order), the
    rotation into the camera adds the three up, and the float32 output adds 2^-24."""
    B, H, W, z0, voxel, T = 8, 24, 48, 6.0, 0.25, 3
    depth, color, poses, ik = U.plane(3, B, H, W, z=z0, noise=0.0)
    assert np.all(depth == np.float32(z0))
    debug = {}
    surface = tsdf.fuse_tsdf_numpy(depth, color, poses, ik, voxel, T, 2, min_depth=0.5, max_range=40.0, debug=debug)
    keys, sums = debug["keys"], debug["sums"]
    turned = np.zeros((1, 3, 4))
    turned[0, :, :3] = C.tilt(0.06, -0.1)
    turned[0, :, 3] = (0.1, -0.05, 0.5)
    views = np.concatenate([poses, turned])
    step_voxels = 0.5
    cast = tsdf.raycast_numpy(keys, sums, views, ik, H, W, voxel, min_weight=2, near=0.5, far=12.0, step_voxels=step_voxels)
    delta, step = 0.5 * T * voxel * 2.0 ** -20, step_voxels * voxel
    # the part of the plane that every fusing camera saw, a voxel and a half in from its edge: the corner voxels of a sample within a
    # step of the zero have their centres within a voxel of it, and a voxel inside the footprint is met by rays (they are denser than voxels)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = [ik[k, 0] * u + ik[k, 1] * v + ik[k, 2] for k in range(3)]
    lo = [max(poses[b, k, 3] + z0 * ray[k].min() for b in range(B)) + 1.5 * voxel for k in range(2)]
    hi = [min(poses[b, k, 3] + z0 * ray[k].max() for b in range(B)) - 1.5 * voxel for k in range(2)]
    seen = 0
    for c, P in enumerate(views):
        R, t = P[:, :3], P[:, 3]
        world_z = R[2, 0] * ray[0] + R[2, 1] * ray[1] + R[2, 2] * ray[2]
        sigma = world_z / ray[2]
        zc0 = (z0 - t[2]) / sigma
        point = [t[k] + zc0 * (R[k, 0] * ray[0] + R[k, 1] * ray[1] + R[k, 2] * ray[2]) / ray[2] for k in range(2)]
        interior = (point[0] >= lo[0]) & (point[0] <= hi[0]) & (point[1] >= lo[1]) & (point[1] <= hi[1])
        assert interior.sum() > 0.5 * H * W
        seen += int(interior.sum())
        assert np.all(cast.depth[c][interior] > 0)                          # every interior pixel hits
        bound = 3.0 * delta * step / (sigma * step - 2.0 * delta) + 2.0 ** -38 + zc0 * 2.0 ** -24
        error = np.abs(cast.depth[c].astype(np.float64) - zc0)
        assert np.all(error[interior] <= bound[interior]), (c, float(error[interior].max()), float(bound[interior].min()))
        want = R.T @ np.array([0.0, 0.0, -1.0])
        nbound = 3.0 * 2.0 * delta / (voxel - 2.0 * delta) + 2.0 ** -24 + 2.0 ** -38
        for k in range(3):
            assert np.all(np.abs(cast.normal[c, k].astype(np.float64) - want[k])[interior] <= nbound), (c, k)
    # the same rays through the surfel renderer at ITS default radius (render.DEFAULT_SPLAT, a model-unit constant that knows nothing of
    # this map's voxel) miss pixels the cast hits: the field needs no radius
    K = np.linalg.inv(ik)
    drawn = render.CloudRenderer("cpu", H, W, K, near=0.5, far=12.0).render_surfels(surface.xyz, surface.rgb, surface.normal, views)
    assert int((drawn.depth > 0).sum()) < seen <= int((cast.depth > 0).sum())


# ---- 4. the caster, the map on disk, the fuser's map ---------------------------------------------------------------------------------------

def test_caster_does_not_depend_on_its_batches():
    keys, sums = C.slab(6, 5, 8)
    poses = C.cameras_in_front(keys, 5)
    K = np.linalg.inv(C.inv_K(6, 9))
    params = dict(min_weight=1, near=1.0, far=40.0)
    whole = tsdf.TsdfCaster("cpu", 6, 9, K, VOXEL, batch_size=12, **params).cast(keys, sums, poses)
    C.assert_casts_equal(whole, tsdf.raycast_numpy(keys, sums, poses, np.linalg.inv(K), 6, 9, VOXEL, step_voxels=tsdf.DEFAULT_STEP_VOXELS, **params))
    for batch_size in (1, 2, 5):
        C.assert_casts_equal(tsdf.TsdfCaster("cpu", 6, 9, K, VOXEL, batch_size=batch_size, **params).cast(keys, sums, poses), whole)
    halves = [tsdf.TsdfCaster("cpu", 6, 9, K, VOXEL, **params).cast(keys, sums, part) for part in (poses[:2], poses[2:])]
    C.assert_casts_equal(tsdf.Cast(*(np.concatenate(pair) for pair in zip(*halves))), whole)
    with pytest.raises(ValueError):
        tsdf.TsdfCaster("cpu", 6, 9, K, VOXEL, batch_size=0)
    for none in (poses[:0], np.zeros((0, 4, 4))):                          # no view: a clear refusal, not an empty concatenation
        with pytest.raises(ValueError, match="C >= 1"):
            tsdf.TsdfCaster("cpu", 6, 9, K, VOXEL, **params).cast(keys, sums, none)
        with pytest.raises(ValueError, match="C >= 1"):
            tsdf.raycast_numpy(keys, sums, none, np.linalg.inv(K), 6, 9, VOXEL, **params)
    assert tsdf.DEFAULT_STEP_VOXELS == 0.5


def test_map_round_trip(tmp_path):
    keys, sums = C.sparse_map(60)
    first, second = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    tsdf.save_map(first, keys, sums, 0.25, 3)
    k, s, voxel, T = tsdf.load_map(first)
    assert np.array_equal(k, keys) and np.array_equal(s, sums) and k.dtype == s.dtype == np.int64 and (voxel, T) == (0.25, 3)
    tsdf.save_map(second, torch.from_numpy(k), torch.from_numpy(s), voxel, T)
    with open(first, "rb") as f, open(second, "rb") as g:
        assert f.read() == g.read()
    empty = str(tmp_path / "empty.npz")
    tsdf.save_map(empty, keys[:0], sums[:0], 0.25, 3)
    assert len(tsdf.load_map(empty)[0]) == 0
    with pytest.raises(ValueError):
        tsdf.save_map(first, keys[::-1], sums, 0.25, 3)
    with pytest.raises(ValueError):
        tsdf.save_map(first, keys, sums, 0.25, 0)


class _Marker:
    def __reduce__(self):
        return (os.system, ("true",))


def test_map_refuses_a_pickle(tmp_path):
    bad = str(tmp_path / "bad.npz")
    keys, sums = C.sparse_map(5)
    np.savez(bad, keys=np.array([_Marker()], dtype=object), sums=sums, voxel=0.25, trunc_voxels=3)
    with pytest.raises(ValueError):
        tsdf.load_map(bad)
    with open(str(tmp_path / "bad.pkl"), "wb") as f:
        pickle.dump({"keys": keys}, f)
    with pytest.raises((ValueError, OSError, pickle.UnpicklingError)):
        tsdf.load_map(str(tmp_path / "bad.pkl"))
    np.savez(bad, keys=keys, sums=sums)
    with pytest.raises(ValueError):
        tsdf.load_map(bad)


def _tree(tmp_path, n_frames=4):
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, n_frames, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, n_frames), 64, 96, [0, 1], is_train=False, img_ext=".png")
    return gt, ds


FUSER = dict(voxel=0.5, batch_size=3, stride=2, border=1, min_depth=0.1, max_range=50.0, edge=0.5)
CLI = ["--voxel", "0.5", "--stride", "2", "--border", "1", "--max_range", "50", "--edge", "0.5", "--batch_size", "3"]


def test_fuser_keeps_its_map(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    fuser = tsdf.TsdfFuser(model, 64, 96, "cpu", trunc_voxels=2, min_weight=1, **FUSER)
    assert fuser.map is None
    debug = {}
    got = fuser.fuse(ds, poses=gt, debug=debug)
    kept = {}
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    want = tsdf.fuse_tsdf_numpy(debug["depth"].numpy(), cloud.odometry.dataset_frames_u8(ds).numpy(), debug["poses"], cloud.dataset_inv_K(ds),
                                0.5, 2, 1, debug=kept, **params)
    U.assert_surfaces_equal(got, want)                                      # fuse's return value is what it was
    assert np.array_equal(fuser.map[0], kept["keys"]) and np.array_equal(fuser.map[1], kept["sums"]) and len(fuser.map[0]) > 0


# ---- 5. the C entry point -----------------------------------------------------------------------------------------------------------------

def test_entry_point_rejects_bad_arguments_without_a_gpu():
    lib = native.load()
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the checks come first
    #     keys sums V  poses inv_K C  H  W  voxel inv  mw near far  step ps   bg        depth normal color weight stats stream
    ok = [one, one, 4, one, one, 0, 8, 8, 0.25, 4.0, 2, 0.1, 4.0, 0.5, 1.0, 0, 0, 0, one, one, one, one, one, None]
    sig = native.SIGNATURES["td_tsdf_cast"][1]
    scalars = (native._P, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong)
    assert len(sig) == len(ok) and all(a in scalars for a in sig)              # no TD_HOST parameter: inv_K is a device array
    assert lib.td_tsdf_cast(*ok) == 0                                          # C = 0: a no-op, nothing is launched
    for pos in (0, 1, 3, 4, 18, 19, 20, 21, 22):
        args = list(ok)
        args[pos] = None
        assert lib.td_tsdf_cast(*args) == -1, pos
    nan, inf = float("nan"), float("inf")
    for pos, bad in ((2, -1), (5, -1), (6, 0), (7, 0), (8, 0.0), (8, nan), (8, inf), (9, 0.0), (9, nan), (10, 0), (10, -2),
                     (11, 0.0), (11, -1.0), (11, nan), (12, inf), (12, nan), (12, 0.05), (13, 0.0), (13, -0.5), (13, nan), (13, inf), (14, nan),
                     (15, -1), (16, 256), (17, 300)):
        args = list(ok)
        args[pos] = bad
        assert lib.td_tsdf_cast(*args) == -1, (pos, bad)
    # n_steps over the cap, and the cap itself (0.1 + 65535 * 0.125 has 65536 samples): both before anything is launched (C = 0)
    step = 0.5 * 0.25
    cap = native.CONSTANTS["TD_TSDF_CAST_MAX_STEPS"]
    assert cap == tsdf.CAST_MAX_STEPS == 65536
    for far, code in ((0.1 + step * (cap - 1) + 0.01, 0), (0.1 + step * cap + 0.01, -2)):
        args = list(ok)
        args[12] = far
        assert lib.td_tsdf_cast(*args) == code, far
    args = list(ok)
    args[5] = 65536                                                            # more views than a grid's y holds
    assert lib.td_tsdf_cast(*args) == -2
    assert lib.td_tsdf_cast(*(ok[:2] + [0] + ok[3:])) == 0                     # V = 0 with C = 0


def test_device_entry_point_refuses_host_tensors():
    keys, sums = C.slab(2, 2, 2)
    poses = torch.from_numpy(C.cameras_in_front(keys, 1))
    with pytest.raises(native.NativeLibraryError):
        tsdf.raycast_hip(torch.from_numpy(keys), torch.from_numpy(sums), poses, C.inv_K(4, 4), 4, 4, VOXEL)


# ---- 6. the programs --------------------------------------------------------------------------------------------------------------------

def test_programs_on_the_host(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    ckpt = str(tmp_path / "model.pth")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "scripts", "reconstruct.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
            "--checkpoint", ckpt, "--data_path", str(tmp_path), "--sequence", "9", "--height", "64", "--width", "96", "--device", "cpu",
            "--tsdf", "--trunc_voxels", "2", "--min_weight", "1"] + CLI
    pose_file, map_file = str(tmp_path / "fused_poses.txt"), str(tmp_path / "map.npz")
    with_map = subprocess.run(base + ["--save_poses", pose_file, "--save_map", map_file, "--out", str(tmp_path / "a.ply")], env=env,
                              capture_output=True, text=True, timeout=600)
    assert with_map.returncode == 0, with_map.stdout + with_map.stderr
    without = subprocess.run(base + ["--save_poses", pose_file, "--out", str(tmp_path / "b.ply")], env=env, capture_output=True, text=True,
                             timeout=600)
    assert without.returncode == 0, without.stdout + without.stderr
    # without the new flag the program prints and writes what it did; with it one line more, and the same PLY
    with open(str(tmp_path / "a.ply"), "rb") as f, open(str(tmp_path / "b.ply"), "rb") as g:
        assert f.read() == g.read()
    lines = [l for l in with_map.stdout.replace("a.ply", "b.ply").splitlines() if not l.startswith("saved") or "voxels" not in l]
    assert lines == without.stdout.splitlines() and "voxels to" not in without.stdout
    fuser = tsdf.TsdfFuser(model, 64, 96, "cpu", trunc_voxels=2, min_weight=1, **FUSER)
    fuser.fuse(ds)
    keys, sums, voxel, T = tsdf.load_map(map_file)
    assert np.array_equal(keys, fuser.map[0]) and np.array_equal(sums, fuser.map[1]) and (voxel, T) == (0.5, 2)
    assert "saved %d voxels to %s" % (len(keys), map_file) in with_map.stdout
    # the map, cast from the poses it was fused with
    views = str(tmp_path / "views")
    common = ["--poses", pose_file, "--K", "55.68", "122.88", "48", "32", "--height", "64", "--width", "96", "--near", "0.05", "--far", "30",
              "--device", "cpu"]
    program = [sys.executable, os.path.join(ROOT, "scripts", "render_cloud.py")]
    run = subprocess.run(program + ["--map", map_file, "--frames", "1:3", "--min_weight", "1", "--step_voxels", "0.5", "--save_depth",
                                    "--save_normals", "--out", views] + common, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    K = np.array([[55.68, 0, 48], [0, 122.88, 32], [0, 0, 1.0]])
    want = tsdf.TsdfCaster("cpu", 64, 96, K, 0.5, min_weight=1, near=0.05, far=30.0, step_voxels=0.5).cast(
        keys, sums, cloud.odometry.load_kitti_poses(pose_file)[1:3])                # the poses as the text file holds them
    assert want.stats[:, 1].sum() > 0
    for j, n in enumerate((1, 2)):
        stem = os.path.join(views, "view_%06d" % n)
        assert all(os.path.exists(stem + tail) for tail in ("_color.png", "_depth.png", "_normal.png"))
        assert np.array_equal(np.load(stem + "_depth.npy").view(np.uint32), want.depth[j].view(np.uint32))
        assert np.array_equal(np.load(stem + "_normal.npy").view(np.uint32), want.normal[j].view(np.uint32))
        assert "view %06d %s" % (n, " ".join("%s %d" % (k, v) for k, v in zip(tsdf.CAST_STATS, want.stats[j]))) in run.stdout
    assert "total over 2 views " + " ".join("%s %d" % (k, v) for k, v in zip(tsdf.CAST_STATS, want.stats.sum(0))) in run.stdout
    assert not os.path.exists(os.path.join(views, "view_000000_color.png"))
    # --map excludes --cloud, --top and --surfels, with a message
    for extra, word in ((["--cloud", str(tmp_path / "a.ply")], "--cloud and --map"), (["--top"], "perspective only"), (["--surfels"], "discs")):
        bad = subprocess.run(program + ["--map", map_file, "--out", views] + extra + common, env=env, capture_output=True, text=True, timeout=600)
        assert bad.returncode == 2 and word in bad.stderr, bad.stderr
    # without --map the program draws the cloud as before: the same bytes as CloudRenderer gives
    plain = str(tmp_path / "plain")
    run = subprocess.run(program + ["--cloud", str(tmp_path / "a.ply"), "--splat", "0.5", "--save_depth", "--out", plain] + common, env=env,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    points = cloud.load_ply(str(tmp_path / "a.ply"))
    xyz = np.stack([points["x"], points["y"], points["z"]], 1)
    rgb = np.stack([points["red"], points["green"], points["blue"]], 1)
    drawn = render.CloudRenderer("cpu", 64, 96, K, near=0.05, far=30.0, splat=0.5).render(xyz, rgb, fuser.poses)
    for n in range(len(fuser.poses)):
        assert np.array_equal(np.load(os.path.join(plain, "view_%06d_depth.npy" % n)).view(np.uint32), drawn.depth[n].view(np.uint32))
    assert "rays" not in run.stdout and "Casting" not in run.stdout
