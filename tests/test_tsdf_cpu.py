"""tripled_amd.tsdf without a GPU: the numpy statements against the literal brute forces (plain Python floats and a dict), the sampling
rules one at a time, the recovery of the summed distance from the payload's three field sums, the surface on hand-built maps, the
prototype's noisy plane against the voxel-averaging fuser, TsdfFuser(device='cpu') and scripts/reconstruct.py --tsdf on a tiny tree,
and the argument checks of the two C entry points.  Everything but the plane's rms comparison is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, native, tsdf
from tests import odom_util
from tests import tsdf_util as U
from tests.infer_util import build_model, ROOT

ONE = U.ONE


# ---- 1. the statements against the brute forces -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed,B,H,W,T,masked,over", [
    (0, 3, 7, 13, 3, False, {}),
    (1, 2, 9, 12, 1, True, dict(stride=3, border=2)),
    (2, 3, 6, 11, 8, True, dict(edge=0.15, border=1)),
    (3, 2, 5, 17, 3, True, dict(edge=0.3, depth_scale=1.7, pose_scale=0.5)),
    (4, 2, 8, 12, 2, False, dict(edge=0.3, stride=2)),
])
def test_statements_are_the_brute_forces(seed, B, H, W, T, masked, over):
    depth, color, poses, inv_K = U.scene(seed, B, H, W)
    mask = U.pixel_mask(seed, depth.shape) if masked else None
    params = dict(U.PARAMS, **over)
    key, payload, counts = tsdf.samples_numpy(depth, color, poses, inv_K, T, U.VOXEL, mask, **params)
    n = B * H * W
    assert key.shape == payload.shape == ((4 * T + 1) * n,) and key.dtype == np.int64 and payload.dtype == np.uint64
    assert not payload[key == cloud.INVALID_KEY].any()
    table, want_counts = tsdf.samples_bruteforce(depth, color, poses, inv_K, T, U.VOXEL, mask, **params)
    assert list(counts) == want_counts, (counts, want_counts)
    assert counts[:6].sum() == n and counts[6:].sum() == (4 * T + 1) * counts[0] and counts[6] == (key != cloud.INVALID_KEY).sum()
    keys, sums = cloud.voxel_table_numpy(key, payload)
    want_keys, want_sums = U.rows_of_table(table)
    assert np.array_equal(keys, want_keys)
    assert np.array_equal(sums[:, 0], want_sums[:, 0]) and np.array_equal(sums[:, 4:], want_sums[:, 4:])
    assert np.array_equal(tsdf.row_sdf_sum(sums), tsdf.row_sdf_sum(want_sums))
    # the scene does exercise the rules: bad depths, the far frame (beyond the key range unless pose_scale halves its translation),
    # negative coordinates, and each way of skipping a slot
    if not over.get("stride"):
        assert counts[0] > 0 and counts[3] > 0 and counts[7] > 0 and counts[8] > 0 and (counts[9] > 0) == (params["pose_scale"] == 1.0)
        assert (counts[4] > 0) == (params["edge"] > 0) and (counts[5] > 0) == masked
        assert min(int(c.min()) for c in cloud.unpack_key(keys)) < 0
    for min_weight in (1, 2):
        U.assert_surface_is_bruteforce(keys, sums, U.VOXEL, min_weight)


def test_fuse_is_the_chain_of_the_statements():
    depth, color, poses, inv_K = U.scene(5, 3, 8, 12)
    params = dict(U.PARAMS, edge=0.3)
    debug = {}
    got = tsdf.fuse_tsdf_numpy(depth, color, poses, inv_K, U.VOXEL, 2, 1, debug=debug, **params)
    key, payload, counts = tsdf.samples_numpy(depth, color, poses, inv_K, 2, U.VOXEL, **params)
    keys, sums = cloud.voxel_table_numpy(key, payload)
    assert np.array_equal(debug["keys"], keys) and np.array_equal(debug["sums"], sums)
    xyz, normal, rgb, weight, hit, scounts = tsdf.surface_numpy(keys, sums, U.VOXEL, 1)
    assert len(got.xyz) == hit.sum() > 0 and np.array_equal(got.xyz, xyz[hit]) and np.array_equal(got.normal, normal[hit])
    assert np.array_equal(got.rgb, rgb[hit]) and np.array_equal(got.weight, weight[hit])
    assert got.stats["points"] == depth.size and got.stats["samples"] == counts[6] and got.stats["voxels"] == len(keys)
    assert got.stats["surface_points"] == sum(got.stats["crossings_" + a] for a in "xyz") == len(got.xyz)
    # the multi-view filter composes through the mask: the same as handing the votes over as a mask
    inv = np.linalg.inv(inv_K)
    votes = cloud.views_numpy(depth, poses, inv_K, inv, 1, 0.2, min_depth=params["min_depth"], max_range=params["max_range"])
    filtered = tsdf.fuse_tsdf_numpy(depth, color, poses, inv_K, U.VOXEL, 2, 1, min_views=1, view_radius=1, view_tol=0.2, K=inv, **params)
    U.assert_surfaces_equal(filtered, tsdf.fuse_tsdf_numpy(depth, color, poses, inv_K, U.VOXEL, 2, 1, mask=votes >= 1, **params))
    assert filtered.stats["invalid_mask"] > 0


# ---- 2. the sampling rules ---------------------------------------------------------------------------------------------------------

def _one_pixel(ray, d, T, voxel=1.0, depth_scale=1.0):
    inv_K = np.array([[0.0, 0.0, ray[0]], [0.0, 0.0, ray[1]], [0.0, 0.0, ray[2]]])
    depth = np.full((1, 1, 1), d, np.float32)
    color = np.array([7, 8, 9], np.uint8).reshape(1, 3, 1, 1)
    poses = np.eye(4)[None, :3]
    args = (depth, color, poses, inv_K, T, voxel)
    params = dict(U.PARAMS, depth_scale=depth_scale)
    key, payload, counts = tsdf.samples_numpy(*args, **params)
    table, want = tsdf.samples_bruteforce(*args, **params)
    assert list(counts) == want
    return key, payload, counts, table


def test_a_diagonal_ray_emits_every_voxel_once():
    """Along (1, 1, 1) at voxel 1 a half-voxel step of depth moves every coordinate by 0.5: consecutive slots share a voxel."""
    T = 3
    key, payload, counts, table = _one_pixel((1.0, 1.0, 1.0), 5.0, T)
    # 13 slots at 2, 2.5, ... 8 meet the voxels 2 ... 8, all but the last twice; voxel 8's centre is 3.5 behind the surface: outside the band
    assert counts[0] == 1 and counts[6] == 6 and counts[7] == 6 and counts[8] == 1 and counts[9] == 0
    kept = key[key != cloud.INVALID_KEY]
    assert len(np.unique(kept)) == len(kept) == 6
    assert sorted(table) == [(i, i, i) for i in range(2, 8)] and all(row[0] == 1 for row in table.values())
    # slot 0 (s = -2T) is kept, slot 1 repeats its voxel: the first of two equal slots wins
    assert key[0] != cloud.INVALID_KEY and key[1] == cloud.INVALID_KEY and payload[1] == 0
    # sdf = 5 - (i + 0.5), q = sdf 2^20 / 3
    assert [table[(i, i, i)][1] - ONE for i in range(2, 8)] == [int(round((4.5 - i) * (1048576.0 / 3.0))) for i in range(2, 8)]


def test_the_band_keeps_its_edge_and_drops_the_next_value():
    """|sdf| == trunc is kept; the next representable float64 above it is dropped.  Ray (0, 0, 1), voxel 1, T = 1: depth 5.5 samples the
    voxels 4, 5, 6 with sdf 1, 0, -1; depth 5.5 (1 + 2^-52) = nextafter(5.5) gives voxel 4 the sdf 1 + 2^-50."""
    key, payload, counts, table = _one_pixel((0.0, 0.0, 1.0), 5.5, 1)
    assert counts[6] == 3 and counts[7] == 2 and counts[8] == 0
    assert {c: row[1] - ONE for c, row in table.items()} == {(0, 0, 4): ONE, (0, 0, 5): 0, (0, 0, 6): -ONE}
    above = np.nextafter(1.0, 2.0)
    assert 5.5 * above == np.nextafter(5.5, 6.0) and 5.5 * above - 4.5 == 1.0 + 2.0 ** -50
    key, payload, counts, table = _one_pixel((0.0, 0.0, 1.0), 5.5, 1, depth_scale=above)
    assert counts[6] == 2 and counts[7] == 2 and counts[8] == 1
    assert sorted(table) == [(0, 0, 5), (0, 0, 6)] and table[(0, 0, 6)][1] - ONE == -ONE


@pytest.mark.parametrize("T", [1, 8])
def test_narrowest_and_widest_band(T):
    key, payload, counts, table = _one_pixel((0.25, -0.5, 1.0), 9.3, T, voxel=0.5)
    assert len(key) == 4 * T + 1 and counts[6] + counts[7] + counts[8] == 4 * T + 1 and counts[6] >= 2 * T
    assert all(abs(row[1] - ONE * row[0]) <= ONE * row[0] for row in table.values())
    for bad in (0, 9, -1):
        with pytest.raises(ValueError):
            tsdf.samples_numpy(np.ones((1, 1, 1), np.float32), np.zeros((1, 3, 1, 1), np.uint8), np.eye(4)[None, :3], np.eye(3), bad, 1.0)


# ---- 3. the payload carries the distance through the unchanged reduction -------------------------------------------------------------

def test_summed_distance_is_recovered_from_the_field_sums():
    g = np.random.default_rng(0)
    v = np.concatenate([g.integers(0, 2 * ONE + 1, 500), [0, 2 * ONE, ONE, 1023, 1024, ONE - 1]]).astype(np.int64)
    colour = g.integers(0, 256, (len(v), 3)).astype(np.uint64)
    payload = v.astype(np.uint64) | (colour[:, 0] << np.uint64(30)) | (colour[:, 1] << np.uint64(38)) | (colour[:, 2] << np.uint64(46))
    rows = cloud.unpack_payload(payload)
    assert np.array_equal(rows[:, 1] + 1024 * rows[:, 2] + ONE * rows[:, 3], v) and np.array_equal(rows[:, 4:], colour.astype(np.int64))
    key = g.integers(0, 5, len(v)).astype(np.int64)
    keys, sums = cloud.voxel_table_numpy(key, payload)
    for k, row, S in zip(keys, sums, tsdf.row_sdf_sum(sums)):
        assert int(S) == int(v[key == k].sum()) - ONE * int((key == k).sum()) and row[0] == (key == k).sum()
    # rows with counts of 2^31: the three sums stay exact in int64, against Python's integers
    for q in (0, 2 * ONE, ONE + 12345, 987654):
        n = 2 ** 31
        row = np.array([[n, n * (q & 1023), n * ((q >> 10) & 1023), n * (q >> 20), 0, 0, 0]], np.int64)
        assert int(tsdf.row_sdf_sum(row)[0]) == n * q - n * ONE


# ---- 4. the surface on hand-built maps ---------------------------------------------------------------------------------------------

def _surface(cells, min_weight=1, voxel=0.5):
    keys, sums = U.hand_map(cells)
    out = U.assert_surface_is_bruteforce(keys, sums, voxel, min_weight)
    return keys, out


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_crossing_on_one_axis(axis):
    a = (3, -4, 5)
    b = tuple(a[k] + (k == axis) for k in range(3))
    keys, (xyz, normal, rgb, weight, hit, counts) = _surface({a: (2, 2 * 300000, 20, 40, 60), b: (3, -3 * 100000, 300, 330, 360)})
    ia = int(np.searchsorted(keys, cloud.pack_key(*a)))
    assert hit.sum() == 1 and hit[ia, axis] and list(counts) == [0] + [int(k == axis) for k in range(3)] + [0]
    t = 300000.0 / (300000.0 - -100000.0)
    want = [(a[k] + 0.5 + (t if k == axis else 0.0)) * 0.5 for k in range(3)]
    assert np.array_equal(xyz[ia, axis], np.array(want, np.float32))
    # D falls along the axis: the gradient is one-sided on both voxels and points down it, towards the positive side
    assert np.array_equal(normal[ia, axis], np.array([-1.0 * (k == axis) for k in range(3)], np.float32))
    assert list(rgb[ia, axis]) == [100, 110, 120] and weight[ia, axis] == 2          # t = 0.75: b's colour; min(2, 3)


def test_zero_counts_as_positive_and_missing_or_light_neighbours_do_not_cross():
    # S = 0 on one side: a crossing at the zero voxel's centre (t = 0) or at b's (t = 1)
    keys, (xyz, normal, rgb, weight, hit, counts) = _surface({(0, 0, 0): (1, 0, 1, 2, 3), (0, 0, 1): (1, -5000, 4, 5, 6)})
    assert hit.sum() == 1 and np.array_equal(xyz[0, 2], np.array([0.25, 0.25, 0.25], np.float32)) and list(rgb[0, 2]) == [1, 2, 3]
    keys, (xyz, normal, rgb, weight, hit, counts) = _surface({(0, 0, 0): (1, -5000, 1, 2, 3), (0, 0, 1): (1, 0, 4, 5, 6)})
    assert hit.sum() == 1 and np.array_equal(xyz[0, 2], np.array([0.25, 0.25, 0.75], np.float32)) and list(rgb[0, 2]) == [4, 5, 6]
    # both zero, or zero against positive: no crossing
    assert _surface({(0, 0, 0): (1, 0, 0, 0, 0), (0, 0, 1): (1, 0, 0, 0, 0), (0, 1, 0): (1, 77, 0, 0, 0)})[1][4].sum() == 0
    # a neighbour missing: the voxels are two apart
    assert _surface({(0, 0, 0): (1, 9000, 0, 0, 0), (0, 0, 2): (1, -9000, 0, 0, 0), (2, 0, 0): (1, -9000, 0, 0, 0)})[1][4].sum() == 0
    # a neighbour under min_weight: counted, and no crossing
    cells = {(0, 0, 0): (3, 9000, 0, 0, 0), (0, 0, 1): (2, -9000, 0, 0, 0), (0, 1, 0): (3, -9000, 0, 0, 0)}
    out = _surface(cells, min_weight=3)[1]
    assert out[4].sum() == 1 and out[4][0, 1] and out[5][0] == 1
    assert _surface(cells, min_weight=2)[1][4].sum() == 2
    # ... nor does it enter a gradient: with the light voxel the z difference would tilt the normal
    assert np.array_equal(out[1][0, 1], np.array([0.0, -1.0, 0.0], np.float32))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_last_coordinate_has_no_neighbour_and_nothing_is_carried(axis):
    """Voxel a at 2^20 - 1 on ``axis``: a blind key + (1 << shift) would carry into the next field (or, on x, out of the key) and land on
    voxel ``trap``, which exists and has the other sign."""
    top, low = cloud.HALF - 1, -cloud.HALF
    a = [5, 6, 7]
    a[axis] = top
    trap = list(a)
    trap[axis] = low
    if axis > 0:
        trap[axis - 1] += 1
    cells = {tuple(a): (2, 50000, 0, 0, 0), tuple(trap): (2, -50000, 0, 0, 0)}
    if axis > 0:
        key_a, key_trap = (int(cloud.pack_key(*c)) for c in (a, trap))
        assert key_trap == key_a + (1 << (21 if axis == 1 else 0))          # the carry does land there
    keys, out = _surface(cells)
    assert out[4].sum() == 0 and list(out[5]) == [0, 0, 0, 0, 0]
    # and the first coordinate has no - neighbour for a gradient: b at -2^20 + 1 ... a at -2^20, crossing found, gradient one-sided
    a[axis] = low
    b = list(a)
    b[axis] = low + 1
    keys, out = _surface({tuple(a): (1, 7000, 0, 0, 0), tuple(b): (1, -7000, 0, 0, 0)})
    assert out[4].sum() == 1 and out[5][4] == 0


def test_a_crossing_without_a_gradient_has_no_normal_and_is_counted():
    """a = +d, b = -d on x, and beyond each the other's value again: both central differences are 0, and so is every other axis."""
    d = 40000
    cells = {(-1, 0, 0): (1, -d, 0, 0, 0), (0, 0, 0): (1, d, 9, 9, 9), (1, 0, 0): (1, -d, 0, 0, 0), (2, 0, 0): (1, d, 0, 0, 0)}
    keys, (xyz, normal, rgb, weight, hit, counts) = _surface(cells)
    assert hit.sum() == 3 and counts[1] == 3
    assert counts[4] == 1 and not normal[1, 0].any() and np.array_equal(xyz[1, 0], np.array([0.5, 0.25, 0.25], np.float32))
    assert normal[0, 0, 0] == 1.0 and normal[2, 0, 0] == 1.0          # the outer edges have one-sided gradients on one voxel


def test_surface_argument_errors_and_the_empty_map():
    out = tsdf.surface_numpy(np.zeros(0, np.int64), np.zeros((0, 7), np.int64), 0.5, 1)
    assert out[0].shape == (0, 3, 3) and out[4].shape == (0, 3) and not out[5].any()
    keys, sums = U.sparse_map(5)
    for bad in (dict(voxel=0.0), dict(min_weight=0)):
        with pytest.raises(ValueError):
            tsdf.surface_numpy(keys, sums, **dict(dict(voxel=0.5, min_weight=1), **bad))
    with pytest.raises(ValueError):
        tsdf.surface_numpy(keys[::-1], sums, 0.5, 1)
    with pytest.raises(ValueError):
        tsdf.fuse_tsdf_numpy(*U.scene(0, 2, 4, 6), voxel=0.25, trunc_voxels=9)


@pytest.mark.parametrize("maker", [U.sparse_map, U.field_ends_map])
def test_surface_on_seeded_maps(maker):
    for V in (1, 40, 63):
        keys, sums = maker(V, seed=V)
        for min_weight in (1, 3):
            U.assert_surface_is_bruteforce(keys, sums, 0.25, min_weight)
    keys, sums = U.slab(5, 4, 6)
    out = U.assert_surface_is_bruteforce(keys, sums, 0.25, 2)
    assert out[5][3] > 0


# ---- 5. the prototype's plane ----------------------------------------------------------------------------------------------------------

def test_noisy_plane_is_one_layer_with_normals_towards_the_camera(capsys):
    """A fronto-parallel plane at z = 6.1 in 8 frames of 24 x 48, uniform depth noise of +-0.3, voxel 0.25, T = 3, min_weight = 4.
    Measured with seed 0: rms z error 0.0367 (TSDF, z crossings) against 0.1760 (fuse_numpy's voxel averages): a ratio of 0.21."""
    depth, color, poses, inv_K = U.plane(0)
    params = dict(stride=1, border=0, min_depth=0.5, max_range=40.0, edge=0.0)
    debug = {}
    got = tsdf.fuse_tsdf_numpy(depth, color, poses, inv_K, 0.25, 3, 4, debug=debug, **params)
    averaged = cloud.fuse_numpy(depth, color, poses, inv_K, 0.25, **params)
    xyz, normal, rgb, weight, hit, counts = tsdf.surface_numpy(debug["keys"], debug["sums"], 0.25, 4)
    ix, iy, iz = cloud.unpack_key(debug["keys"])
    columns = np.stack([ix[hit[:, 2]], iy[hit[:, 2]]], 1)
    assert len(columns) > 400 and len(np.unique(columns, axis=0)) == len(columns)          # at most one z crossing per (x, y) column
    rms_tsdf = float(np.sqrt(np.mean((xyz[hit[:, 2], 2, 2].astype(np.float64) - 6.1) ** 2)))
    rms_mean = float(np.sqrt(np.mean((averaged.xyz[:, 2].astype(np.float64) - 6.1) ** 2)))
    with capsys.disabled():
        print("\nnoisy plane: rms z error tsdf %.4f, voxel average %.4f, ratio %.3f" % (rms_tsdf, rms_mean, rms_tsdf / rms_mean))
    assert rms_tsdf <= 0.5 * rms_mean
    assert len(got.normal) == hit.sum() and np.all(got.normal[:, 2] < 0)          # the cameras look along +z
    # the voxel average puts the plane into several layers per column
    ax, ay, az = cloud.unpack_key(averaged.keys)
    assert len(averaged.keys) / len(np.unique(np.stack([ax, ay], 1), axis=0)) > 2.0


# ---- 6. the fuser and the programs -------------------------------------------------------------------------------------------------

def _tree(tmp_path, n_frames=4):
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, n_frames, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, n_frames), 64, 96, [0, 1], is_train=False, img_ext=".png")
    return gt, ds


FUSER = dict(voxel=0.5, batch_size=3, stride=2, border=1, min_depth=0.1, max_range=50.0, edge=0.5)
CLI = ["--voxel", "0.5", "--stride", "2", "--border", "1", "--max_range", "50", "--edge", "0.5", "--batch_size", "3"]


def test_tsdf_fuser_on_the_host(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96).train()
    fuser = tsdf.TsdfFuser(model, 64, 96, "cpu", trunc_voxels=2, min_weight=1, **FUSER)
    debug = {}
    got = fuser.fuse(ds, debug=debug)
    assert model.training
    depth, poses = debug["depth"].numpy(), debug["poses"]
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    U.assert_surfaces_equal(got, tsdf.fuse_tsdf_numpy(depth, frames, poses, cloud.dataset_inv_K(ds), 0.5, 2, 1, **params))
    assert got.stats["points"] == 4 * 64 * 96 and got.stats["samples"] > 0 and np.array_equal(fuser.poses, poses)
    sub = fuser.fuse(ds, poses=gt, frames=(1, 3), debug=debug)
    U.assert_surfaces_equal(sub, tsdf.fuse_tsdf_numpy(debug["depth"].numpy(), frames[1:3], gt[1:3], cloud.dataset_inv_K(ds), 0.5, 2, 1, **params))
    # the multi-view filter composes through the mask
    seen = tsdf.TsdfFuser(model, 64, 96, "cpu", trunc_voxels=2, min_weight=1, min_views=1, view_radius=1, view_tol=0.5, **FUSER).fuse(ds, poses=gt)
    assert seen.stats["invalid_mask"] > 0 and seen.stats["valid"] + seen.stats["invalid_mask"] == fuser.fuse(ds, poses=gt).stats["valid"]
    for bad in (dict(trunc_voxels=0), dict(trunc_voxels=9), dict(min_weight=0), dict(voxel=0.0), dict(pair_chunk=0)):
        with pytest.raises(ValueError):
            tsdf.TsdfFuser(model, 64, 96, "cpu", **bad)
    with pytest.raises(ValueError):
        fuser.fuse(ds, frames=(2, 9))


def test_programs_on_the_host(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    ckpt = str(tmp_path / "model.pth")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    env = dict(os.environ, PYTHONPATH=ROOT)
    base = [sys.executable, os.path.join(ROOT, "scripts", "reconstruct.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
            "--checkpoint", ckpt, "--data_path", str(tmp_path), "--sequence", "9", "--height", "64", "--width", "96", "--device", "cpu"] + CLI
    out, pose_file = str(tmp_path / "surface.ply"), str(tmp_path / "fused_poses.txt")
    run = subprocess.run(base + ["--tsdf", "--trunc_voxels", "2", "--min_weight", "1", "--save_poses", pose_file, "--out", out],
                         env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want = tsdf.TsdfFuser(model, 64, 96, "cpu", trunc_voxels=2, min_weight=1, **FUSER).fuse(ds)
    back = cloud.load_ply(out)
    assert back.dtype.names == cloud.PLY_DTYPE.names + ("nx", "ny", "nz") and len(back) == len(want.xyz) > 0
    assert np.array_equal(np.stack([back["x"], back["y"], back["z"]], 1).view(np.uint32), want.xyz.view(np.uint32))
    assert np.array_equal(np.stack([back["nx"], back["ny"], back["nz"]], 1).view(np.uint32), want.normal.view(np.uint32))
    assert np.array_equal(np.stack([back["red"], back["green"], back["blue"]], 1), want.rgb) and np.array_equal(back["count"], want.weight)
    for name in ("samples", "skipped_duplicate", "voxels", "crossings_z", "crossings_without_normal", "surface_points"):
        assert "%s %d" % (name, want.stats[name]) in run.stdout, run.stdout
    lengths = np.linalg.norm(want.normal.astype(np.float64), axis=1)
    assert np.all((np.abs(lengths - 1.0) < 1e-6) | (lengths == 0.0))
    # the surfel renderer takes the PLY's normals as they are: nothing is estimated
    views = str(tmp_path / "views")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_cloud.py"), "--cloud", out, "--poses", pose_file, "--K", "55.68",
                          "122.88", "48", "32", "--height", "64", "--width", "96", "--near", "0.05", "--far", "100", "--surfels",
                          "--surfel_radius", "0.5", "--device", "cpu", "--out", views], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "normals: the cloud's own" in run.stdout and "estimated" not in run.stdout
    assert os.path.exists(os.path.join(views, "view_000000_normal.png"))
    # without --tsdf the program writes what the voxel-averaging statements give, byte for byte
    plain = str(tmp_path / "cloud.ply")
    run = subprocess.run(base + ["--out", plain], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    debug = {}
    cloud.SceneFuser(model, 64, 96, "cpu", **FUSER).fuse(ds, debug=debug)
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    direct = cloud.fuse_numpy(debug["depth"].numpy(), cloud.odometry.dataset_frames_u8(ds).numpy(), debug["poses"], cloud.dataset_inv_K(ds),
                              FUSER["voxel"], **params)
    direct_path = str(tmp_path / "direct.ply")
    cloud.save_ply(direct_path, direct.xyz, direct.rgb, direct.count)
    with open(plain, "rb") as f, open(direct_path, "rb") as g:
        assert f.read() == g.read()
    assert "samples" not in run.stdout and "crossings" not in run.stdout


# ---- 7. the C entry points ---------------------------------------------------------------------------------------------------------

def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = native.load()
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the checks come first
    #          depth color poses inv_K mask  B  H  W  T  dscale pscale voxel inv_voxel stride border min  max   edge key payload stats stream
    ok = [one, one, one, one, None, 1, 8, 8, 3, 1.0, 1.0, 0.25, 4.0, 1, 0, 0.1, 10.0, 0.0, one, one, None, None]
    assert len(native.SIGNATURES["td_tsdf_samples"][1]) == len(ok)
    scalars = (native._P, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong)
    assert all(a in scalars for a in native.SIGNATURES["td_tsdf_samples"][1] + native.SIGNATURES["td_tsdf_surface"][1])      # no TD_HOST
    for pos in (0, 1, 2, 3, 18, 19):
        args = list(ok)
        args[pos] = None
        assert lib.td_tsdf_samples(*args) == -1, pos
    for pos, bad in ((5, -1), (6, 0), (7, 0), (8, 0), (8, 9), (8, -1), (11, 0.0), (11, float("nan")), (12, 0.0), (13, 0), (14, -1), (17, -1.0),
                     (17, float("nan"))):
        args = list(ok)
        args[pos] = bad
        assert lib.td_tsdf_samples(*args) == -1, (pos, bad)
    assert lib.td_tsdf_samples(*(ok[:5] + [0] + ok[6:])) == 0                  # B = 0: a no-op, nothing is launched
    for T in (1, 8):
        assert lib.td_tsdf_samples(*(ok[:5] + [0, 8, 8, T] + ok[9:])) == 0
    #          keys sums V  voxel min_weight xyz normal rgb weight mask stats stream
    ok = [one, one, 4, 0.25, 2, one, one, one, one, one, None, None]
    assert len(native.SIGNATURES["td_tsdf_surface"][1]) == len(ok)
    for pos in (0, 1, 5, 6, 7, 8, 9):
        args = list(ok)
        args[pos] = None
        assert lib.td_tsdf_surface(*args) == -1, pos
    for pos, bad in ((2, -1), (3, 0.0), (3, float("nan")), (4, 0), (4, -3)):
        args = list(ok)
        args[pos] = bad
        assert lib.td_tsdf_surface(*args) == -1, (pos, bad)
    assert lib.td_tsdf_surface(*(ok[:2] + [0] + ok[3:])) == 0                  # V = 0


def test_device_entry_points_refuse_host_tensors():
    depth, color, poses, inv_K = (torch.from_numpy(a) for a in U.scene(0, 2, 4, 6))
    with pytest.raises(native.NativeLibraryError):
        tsdf.samples_hip(depth, color, poses, inv_K, 3, 0.25)
    with pytest.raises(native.NativeLibraryError):
        tsdf.surface_hip(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 7, dtype=torch.int64), 0.25)
    with pytest.raises(native.NativeLibraryError):
        tsdf.fuse_tsdf_hip(depth, color, poses, inv_K, 0.25)


# ---- the checks the two fusers share -------------------------------------------------------------------------------------------------

def test_shared_frame_and_row_checks(monkeypatch):
    depth, color, poses, inv_K = U.scene(0, 2, 4, 6)
    d, c, p = (torch.from_numpy(a) for a in (depth, color, poses))
    # the host variant converts what numpy can convert and refuses a wrong shape
    got = cloud._check_frames(depth.astype(np.float64), color.astype(np.int64), poses.astype(np.float32), device=False)
    assert [a.dtype for a in got] == [np.float32, np.uint8, np.float64] and all(a.flags.c_contiguous for a in got)
    for bad in ((depth[0], color, poses), (depth, color[:, :2], poses), (depth, color[:, :, :3], poses), (depth, color, poses[:1]),
                (depth, color, poses[:, :, :3])):
        with pytest.raises(ValueError):
            cloud._check_frames(*bad, device=False)
    # the device variant refuses a host tensor before it looks at anything else; the same for the rows
    keys, sums = torch.zeros(4, dtype=torch.int64), torch.zeros(4, 7, dtype=torch.int64)
    with pytest.raises(native.NativeLibraryError):
        cloud._check_frames(d, c, p, device=True)
    with pytest.raises(native.NativeLibraryError):
        cloud._check_rows(keys, sums)
    # every former copy raises through the one check: the call is seen, and its error is the caller's
    seen = []
    for name in ("_check_frames", "_check_rows"):
        real = getattr(cloud, name)
        monkeypatch.setattr(cloud, name, lambda *a, _real=real, _name=name, **k: (seen.append(_name), _real(*a, **k))[1])
    for site, error in ((lambda: cloud.keys_numpy(depth, color[:, :2], poses, inv_K), ValueError),
                        (lambda: tsdf.samples_numpy(depth, color[:, :2], poses, inv_K, 3, 0.25), ValueError),
                        (lambda: cloud.keys_hip(d, c, p, inv_K), native.NativeLibraryError),
                        (lambda: tsdf.samples_hip(d, c, p, inv_K, 3, 0.25), native.NativeLibraryError)):
        with pytest.raises(error):
            site()
    assert seen == ["_check_frames"] * 4
    for site in (lambda: cloud.finish_hip(keys, sums, 0.25), lambda: cloud.merge_hip(keys, sums, keys, sums),
                 lambda: tsdf.surface_hip(keys, sums, 0.25)):
        with pytest.raises(native.NativeLibraryError):
            site()
    assert seen[4:] == ["_check_rows"] * 3
    # with the device guard out of the way (there is no device here) the device variants refuse a wrong type and a wrong shape
    monkeypatch.setattr(native, "require_device", lambda *tensors: None)
    assert all(a is b for a, b in zip(cloud._check_frames(d, c, p, device=True), (d, c, p))) and cloud._check_rows(keys, sums) is keys
    for bad in ((d.double(), c, p), (d, c.to(torch.int8), p), (d, c, p.float()), (d[0], c, p), (d, c[:, :2], p), (d, c, p[:1])):
        with pytest.raises(ValueError):
            cloud._check_frames(*bad, device=True)
        with pytest.raises(ValueError):
            cloud.keys_hip(*bad, inv_K)
        with pytest.raises(ValueError):
            tsdf.samples_hip(*bad, inv_K, 3, 0.25)
    for bad in ((keys.int(), sums), (keys, sums.int()), (keys, sums[:3]), (keys, sums[:, :6]), (keys.reshape(2, 2), sums)):
        with pytest.raises(ValueError):
            cloud._check_rows(*bad)
        with pytest.raises(ValueError):
            cloud.finish_hip(*bad, 0.25)
        with pytest.raises(ValueError):
            cloud.merge_hip(keys, sums, *bad)
        with pytest.raises(ValueError):
            tsdf.surface_hip(*bad, 0.25)
