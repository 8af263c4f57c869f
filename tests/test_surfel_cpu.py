"""Surfel rendering and the orientation of normals without a GPU (tripled_amd.render.render_surfels_*, tripled_amd.cloud_normals.orient_*):
the numpy statements against their literal loops on scenes with every deciding point planted (tests/surfel_util.py), the conservative
pixel box, a plane that renders as a surface, shading, the refusals and the scripts.  Every comparison of rendered maps and normals is
exact: the outputs are comparisons and conversions of a fixed sequence of individually rounded float64 operations."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import tripled_amd  # noqa: F401
from tripled_amd import cloud, cloud_normals, native, odometry, render
from tests import render_util as U
from tests import surfel_util as S
from tests.infer_util import ROOT

C, H, W, V = 3, 9, 14, 700
_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        _CACHE["scene"] = S.scene(0, V, C, H, W)
    return _CACHE["scene"]


def _statement(mode):
    """render_surfels_numpy of the shared scene in one of the eight modes, computed once."""
    if mode not in _CACHE:
        s = _scene()
        _CACHE[mode] = render.render_surfels_numpy(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, **S.args(s, **S.modes()[mode]))
    return _CACHE[mode]


# ---------------------------------------------------------------------------------------------------------------------------
# A. the statement against the literal loop

@pytest.mark.parametrize("mode", sorted(S.modes()))
def test_statement_is_the_literal_loop(mode):
    s = _scene()
    want = render.render_surfels_bruteforce(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, box=True, **S.args(s, **S.modes()[mode]))
    S.assert_surfels_equal(_statement(mode), want)


@pytest.mark.parametrize("mode", sorted(S.modes()))
def test_the_planted_surfels_exercise_every_outcome(mode):
    s, got, kw, p = _scene(), _statement(mode), S.modes()[mode], _scene().planted
    assert [a.dtype for a in got] == [np.float32, np.uint8, np.int32, np.float32, np.int64]
    assert [a.shape for a in got] == [(C, H, W), (C, 3, H, W), (C, H, W), (C, 3, H, W), (C, 8)]
    st = dict(zip(render.SURFEL_STATS, got.stats.T))
    assert (st["points"] == V).all()
    assert np.array_equal(st["out_of_range"] + st["culled"] + st["outside"] + st["drawn"], st["points"])      # exactly one outcome each
    assert np.array_equal(st["pixels_hit"], (got.index >= 0).reshape(C, -1).sum(1)) and st["pixels_hit"].min() > 0
    assert (st["culled"] > 0).all() if kw["cull"] else not st["culled"].any()
    assert st["billboards"][0] >= 1 and (st["capped"] <= st["drawn"]).all()
    assert st["capped"][0] >= 1 if not kw["ortho"] else not st["capped"].any()        # orthographic: r = 3 for every disc
    geo = render.surfel_setup_numpy(s.xyz, s.normals, s.poses[0], s.K.reshape(-1), s.near, s.far, S.RADIUS, 1.0, kw["ortho"], kw["cull"], H, W)
    assert not geo["in_range"][[p["nan"], p["behind"], p["beyond"]]].any()
    assert geo["billboard"][p["bare"]] and (geo["m0"][p["bare"]], geo["m1"][p["bare"]], geo["m2"][p["bare"]]) == (0.0, 0.0, -1.0)
    assert geo["culled"][p["back"]] == kw["cull"] and not geo["culled"][p["facing"]] and not geo["culled"][p["bare"]]
    assert geo["visible"][p["edge_on"]] and not (got.index == p["edge_on"]).any()     # in its box, edge-on: nothing is drawn, anywhere
    if not kw["ortho"]:
        assert geo["capped"][p["capped"]] and geo["r"][p["capped"]] == render.MAX_SURFEL and geo["visible"][p["capped"]]
        fv, fu = p["facing_pixel"]                                                    # camera 0 sees the facing disc's centre there
        assert (int(geo["vi"][p["facing"]]), int(geo["ui"][p["facing"]])) == (fv, fu)
        covered, t, den, d0, d1 = render.surfel_pixel_numpy(s.K.reshape(-1), False, s.near, s.far, S.RADIUS,
                                                            *(geo[n][p["facing"]] for n in ("q0", "q1", "z", "m0", "m1", "m2")), fu, fv)
        assert covered and t == 1.0 and den == -1.0
        _, _, den, _, _ = render.surfel_pixel_numpy(s.K.reshape(-1), False, s.near, s.far, S.RADIUS,
                                                    *(geo[n][p["edge_on"]] for n in ("q0", "q1", "z", "m0", "m1", "m2")),
                                                    geo["ui"][p["edge_on"]], geo["vi"][p["edge_on"]])
        assert den == 0.0
    # the normal map: turned towards the viewer, +0.0 bits where nothing was drawn
    hit = got.index >= 0
    assert not got.normal.transpose(0, 2, 3, 1)[~hit].view(np.uint32).any() and np.array_equal(got.depth > 0, hit)
    if kw["ambient"] == 1.0:
        assert np.array_equal(got.color.transpose(0, 2, 3, 1)[hit], s.rgb[got.index[hit]])


# ---------------------------------------------------------------------------------------------------------------------------
# B. the box never removes a pixel the geometry covers

@pytest.mark.parametrize("ortho", [False, True])
def test_the_box_is_conservative(ortho):
    s = S.wide_scene(5, 400, 2, H, W)
    kw = S.args(s, radius=0.4, ortho=ortho)
    got = render.render_surfels_numpy(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, **kw)
    st = dict(zip(render.SURFEL_STATS, got.stats.T))
    assert not st["capped"].any() and (st["drawn"] > 0).all() and (st["outside"] > 0).all()
    geo = render.surfel_setup_numpy(s.xyz, s.normals, s.poses[0], s.K.reshape(-1), s.near, s.far, 0.4, 1.0, ortho, False, H, W)
    outside_image = (geo["ui"] < 0) | (geo["ui"] > W - 1) | (geo["vi"] < 0) | (geo["vi"] > H - 1)
    assert (geo["visible"] & outside_image).any()                                  # centres outside the image whose discs reach in
    want = render.render_surfels_bruteforce(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, box=False, **kw)
    S.assert_surfels_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------
# C. a surface is a surface

def test_a_sampled_plane_renders_as_a_surface():
    """Radius 0.36: no hole, the point behind the plane hidden, depth within 2^-21 of the analytic ray-plane depth (measured: 0 holes,
    largest relative error 1.24e-7).  The point renderer on the same input: 82 pixels of the plane, the far point visible.  Radius 0.3:
    8 pixels undrawn."""
    s, nrm, far_point = S.plane_scene()
    Hc, Wc = 9, 14
    got = render.render_surfels_numpy(s.xyz, s.rgb, s.normals, s.poses, s.K, Hc, Wc, 0.36, near=s.near, far=s.far)
    assert (got.index >= 0).all() and got.stats[0, 7] == Hc * Wc
    assert not (got.index == far_point).any()
    ys, xs = np.mgrid[0:Hc, 0:Wc]
    d0, d1 = (xs - s.K[0, 2]) / s.K[0, 0], (ys - s.K[1, 2]) / s.K[1, 1]
    analytic = (nrm @ np.array([0.0, 0.0, 3.0])) / (nrm[0] * d0 + nrm[1] * d1 + nrm[2])
    error = np.abs(got.depth[0].astype(np.float64) / analytic - 1.0).max()
    print("largest relative depth error %.3e" % error)
    assert error <= 2.0 ** -21
    old = render.render_numpy(s.xyz, s.rgb, s.poses, s.K, Hc, Wc, near=s.near, far=s.far, splat=0.0)
    assert np.count_nonzero((old.index >= 0) & (old.index != far_point)) == 82 and (old.index == far_point).sum() == 1
    assert old.index[0, 4, 7] == far_point                                        # (0.05, 0.03, 6) projects to (6.57, 4.04)
    thin = render.render_surfels_numpy(s.xyz, s.rgb, s.normals, s.poses, s.K, Hc, Wc, 0.3, near=s.near, far=s.far)
    print("undrawn at radius 0.3: %d" % np.count_nonzero(thin.index < 0))
    assert (thin.index < 0).any()


# ---------------------------------------------------------------------------------------------------------------------------
# D. orientation

def test_orient_numpy_is_the_per_point_loop():
    s = _scene()
    got, want = cloud_normals.orient_numpy(s.xyz, s.normals, s.poses), cloud_normals.orient_bruteforce(s.xyz, s.normals, s.poses)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert got.normal.dtype == np.float32 and got.camera.dtype == np.int32 and got.stats.dtype == np.int64
    assert got.stats.sum() == V and (got.stats > 0).all()                          # the NaN point is invalid, the bare one none
    assert set(got.camera.tolist()) == {-1, 0, 1, 2}
    half = cloud_normals.orient_numpy(s.xyz, s.normals, s.poses * np.array([1.0, 1.0, 1.0, 0.5]), pose_scale=2.0)      # the same centres
    assert np.array_equal(half.normal.view(np.uint32), got.normal.view(np.uint32)) and np.array_equal(half.camera, got.camera)


def test_orientation_rules():
    g = np.random.default_rng(11)
    centre = np.array([0.5, -1.0, 2.0])
    pose = np.concatenate([np.eye(3), centre[:, None]], 1)[None]
    d = g.normal(size=(300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    xyz = (centre + 3.0 * d).astype(np.float32)
    n = g.normal(size=(300, 3))
    normals = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    out = cloud_normals.orient_numpy(xyz, normals, pose)
    w = centre - xyz.astype(np.float64)
    s = ((out.normal[:, 0] * w[:, 0]) + (out.normal[:, 1] * w[:, 1])) + (out.normal[:, 2] * w[:, 2])
    assert (s >= 0).all() and out.stats[0] > 50 and out.stats[1] > 50 and out.stats[0] + out.stats[1] == 300 and (out.camera == 0).all()
    assert np.array_equal(np.abs(out.normal), np.abs(normals))                     # negation is exact
    again = cloud_normals.orient_numpy(xyz, out.normal, pose)                      # orienting twice changes nothing
    assert np.array_equal(again.normal.view(np.uint32), out.normal.view(np.uint32)) and again.stats.tolist() == [0, 300, 0, 0]
    # two cameras at the same distance: the lower index; s == 0 keeps; a zero normal stays +0.0 with its camera, counted as none; a NaN
    # point has no camera and is invalid
    poses = np.zeros((2, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[0, :, 3], poses[1, :, 3] = [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]
    xyz = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.0], [0.5, 0.0, 1.0], [np.nan, 0.0, 0.0], [-3.0, 0.0, 0.0]], np.float32)
    normals = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]], np.float32)
    for fn in (cloud_normals.orient_numpy, cloud_normals.orient_bruteforce):
        out = fn(xyz, normals, poses)
        assert out.camera.tolist() == [0, 0, 0, -1, 1]
        assert out.normal[0].tolist() == [0.0, 1.0, 0.0]                           # s = 0: kept
        assert out.normal[1].tolist() == [1.0, 0.0, 0.0]                           # towards camera 0 at (1, 0, 0): flipped
        assert not out.normal[2].view(np.uint32).any()                             # +0.0
        assert out.normal[3].tolist() == [0.0, 0.0, 1.0] and out.normal[4].tolist() == [1.0, 0.0, 0.0]
        assert dict(zip(cloud_normals.ORIENT_STATS, out.stats.tolist())) == dict(flipped=2, kept=1, none=1, invalid=1)
    with pytest.raises(ValueError):
        cloud_normals.orient_numpy(xyz, normals, poses[:0])
    with pytest.raises(ValueError):
        cloud_normals.orient_numpy(xyz, normals[:3], poses)


def test_estimate_orients_when_given_poses():
    g = np.random.default_rng(2)
    xy = g.uniform(-1.0, 1.0, (600, 2))
    xyz = np.stack([xy[:, 0], xy[:, 1], 0.001 * g.normal(size=600) + 2.0], 1)
    est = cloud_normals.CloudNormals("cpu", 0.5, min_neighbours=6, max_curvature=0.05)
    plain = est.estimate(xyz)
    assert plain.stats["valid"] > 300 and set(plain.stats) == set(cloud_normals.CAUSES)
    has = plain.normal.any(1)
    assert (plain.normal[has, 2] > 0.9).all()                                      # the sign convention: away from a camera at the origin
    pose = np.eye(4)[None]
    turned = est.estimate(xyz, poses=pose)
    assert np.array_equal(turned.normal[has], -plain.normal[has]) and not turned.normal[~has].any()      # float64, exactly negated
    assert turned.stats["orient_flipped"] == int(has.sum()) and turned.stats["orient_none"] == int((~has).sum())
    assert {k: v for k, v in turned.stats.items() if not k.startswith("orient_")} == plain.stats
    assert np.array_equal(turned.curvature, plain.curvature) and np.array_equal(turned.count, plain.count)


# ---------------------------------------------------------------------------------------------------------------------------
# E. shading

def test_shading():
    s = _scene()
    flat, lit = _statement("persp-all-flat"), _statement("persp-all-lit")
    hit = flat.index >= 0
    S.assert_surfels_equal(flat[:1] + flat[2:], lit[:1] + lit[2:])                  # ambient changes the colours only
    assert np.array_equal(flat.color.transpose(0, 2, 3, 1)[hit], s.rgb[flat.index[hit]])
    assert (lit.color.astype(int) <= flat.color.astype(int) + 1).all() and (lit.color != flat.color).any()
    length = np.sqrt((flat.normal.astype(np.float64) ** 2).sum(1))
    assert np.abs(length[hit] - 1.0).max() <= 1e-6 and not flat.normal.transpose(0, 2, 3, 1)[~hit].view(np.uint32).any()
    # a disc facing the camera on the optical axis: shade exactly 1 at the centre pixel, so any ambient leaves its colour alone
    K = np.array([[8.0, 0.0, 3.0], [0.0, 8.0, 2.0], [0.0, 0.0, 1.0]])
    xyz, rgb, n = np.array([[0.0, 0.0, 2.0]], np.float32), np.array([[200, 101, 7]], np.uint8), np.array([[0.0, 0.0, -1.0]], np.float32)
    for fn in (render.render_surfels_numpy, render.render_surfels_bruteforce):
        out = fn(xyz, rgb, n, np.eye(4)[None], K, 5, 7, 0.5, near=0.25, far=16.0, ambient=0.25)
        assert out.index[0, 2, 3] == 0 and out.color[0, :, 2, 3].tolist() == [200, 101, 7] and out.depth[0, 2, 3] == 2.0
        assert out.normal[0, :, 2, 3].tolist() == [0.0, 0.0, -1.0]
        assert out.index[0, 2, 5] == 0 and out.color[0, :, 2, 5].tolist() == [196, 99, 7]      # oblique ray: shade 1 / sqrt(1 + 1/16)
        dark = fn(xyz, rgb, n, np.eye(4)[None], K, 5, 7, 0.5, near=0.25, far=16.0, ambient=0.0)
        assert dark.color[0, :, 2, 3].tolist() == [200, 101, 7]
        back = fn(xyz, rgb, -n, np.eye(4)[None], K, 5, 7, 0.5, near=0.25, far=16.0, ambient=0.25)      # its back: the map is turned round
        assert back.normal[0, :, 2, 3].tolist() == [0.0, 0.0, -1.0] and back.color[0, :, 2, 3].tolist() == [200, 101, 7]
        assert (fn(xyz, rgb, -n, np.eye(4)[None], K, 5, 7, 0.5, near=0.25, far=16.0, cull=True).index == -1).all()


# ---------------------------------------------------------------------------------------------------------------------------
# F. refusals and scripts

def test_refusals():
    s = _scene()
    ok = dict(radius=0.3, near=0.25, far=16.0)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(ambient=-0.1), dict(ambient=1.5),
                dict(ambient=nan), dict(near=0.0), dict(far=inf), dict(far=0.1), dict(background=(0, 0, 256))):
        for fn in (render.render_surfels_numpy, render.render_surfels_bruteforce):
            with pytest.raises(ValueError):
                fn(s.xyz, s.rgb, s.normals, s.poses, s.K, H, W, **dict(ok, **bad))
    skew = s.K.copy()
    skew[1, 0] = 0.5
    flipped = s.K * np.array([[-1.0], [1.0], [1.0]])
    for args in ((s.xyz, s.rgb, s.normals[:5], s.poses, s.K, H, W), (s.xyz, s.rgb, s.normals[:, :2], s.poses, s.K, H, W),
                 (s.xyz, s.rgb, s.normals, s.poses[:0], s.K, H, W), (s.xyz, s.rgb, s.normals, s.poses, skew, H, W),
                 (s.xyz, s.rgb, s.normals, s.poses, flipped, H, W), (s.xyz, s.rgb, s.normals, s.poses, s.K, 0, W)):
        with pytest.raises(ValueError):
            render.render_surfels_numpy(*args, **ok)
    with pytest.raises(ValueError):
        render.CloudRenderer("cpu", H, W, s.K).render_surfels(s.xyz, s.rgb, s.normals, s.poses, radius=-1.0)


def test_the_hip_layers_refuse_host_tensors():
    s = _scene()
    xyz, rgb, normals, poses = (torch.from_numpy(a) for a in (s.xyz, s.rgb, s.normals, s.poses))
    with pytest.raises(native.NativeLibraryError):
        render.render_surfels_hip(xyz, rgb, normals, poses, s.K, H, W, 0.3, near=s.near, far=s.far)
    with pytest.raises(native.NativeLibraryError):
        cloud_normals.orient_hip(xyz, normals, poses)
    with pytest.raises(native.NativeLibraryError):
        native.call("td_normals_orient", xyz, normals, V, poses, C, 1.0, normals, xyz, xyz)
    with pytest.raises(native.NativeLibraryError):
        native.call("td_cloud_render_surfels", xyz, rgb, normals, V, poses, (ctypes.c_double * 9)(*s.K.reshape(-1)), C, H, W, 1.0, s.near,
                    s.far, 0.3, 0, 0, 1.0, 0, 0, 0, 0, xyz, 8, xyz, rgb, xyz, xyz, xyz)


def test_the_entry_points_reject_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    one = ctypes.c_void_p(64)          # a non-null, aligned pointer that is never dereferenced: the checks come first
    k = (ctypes.c_double * 9)(8.0, 0.0, 6.5, 0.0, 8.0, 4.0, 0.0, 0.0, 1.0)
    need = 3 * 9 * 14 * 8
    ok = [one, one, one, 700, one, k, 3, 9, 14, 1.0, 0.25, 16.0, 0.3, 0, 0, 1.0, 0, 0, 0, 0, one, need, one, one, one, one, one, None]
    for pos in (0, 1, 2, 4, 5, 20, 22, 23, 24, 25, 26):
        args = list(ok)
        args[pos] = None
        assert lib.td_cloud_render_surfels(*args) == -1, pos
    nan, inf = float("nan"), float("inf")
    skew = (ctypes.c_double * 9)(8.0, 0.0, 6.5, 0.25, 8.0, 4.0, 0.0, 0.0, 1.0)
    flat = (ctypes.c_double * 9)(8.0, 0.0, 6.5, 0.0, 0.0, 4.0, 0.0, 0.0, 1.0)
    for pos, bad in ((3, -1), (6, 0), (7, 0), (8, 0), (10, 0.0), (10, nan), (11, inf), (11, 0.125), (12, 0.0), (12, -1.0), (12, inf),
                     (12, nan), (15, -0.5), (15, 1.25), (15, nan), (16, 3), (16, -1), (17, 256), (18, -1), (21, need - 8),
                     (20, ctypes.c_void_p(68)), (5, skew), (5, flat)):
        args = list(ok)
        args[pos] = bad
        assert lib.td_cloud_render_surfels(*args) == -1, (pos, bad)
    for pos, bad in ((6, 65536), (3, 0x7fffffff)):
        args = list(ok)
        args[pos] = bad
        args[21] = 1 << 40
        assert lib.td_cloud_render_surfels(*args) == -2, (pos, bad)
    ok = [one, one, 700, one, 3, 1.0, one, one, one, None]
    for pos in (0, 1, 3, 6, 7, 8):
        args = list(ok)
        args[pos] = None
        assert lib.td_normals_orient(*args) == -1, pos
    for pos, bad in ((2, -1), (4, 0), (4, -3), (0, ctypes.c_void_p(66)), (8, ctypes.c_void_p(68))):
        args = list(ok)
        args[pos] = bad
        assert lib.td_normals_orient(*args) == -1, (pos, bad)


def _tiny_cloud(tmp_path, with_normals):
    s = S.scene(7, 300, 5, 13, 20)
    ply = str(tmp_path / ("cloud_n.ply" if with_normals else "cloud.ply"))
    keep = slice(1, None)                                                          # without the NaN: a top view needs a box
    cloud.save_ply(ply, s.xyz[keep], s.rgb[keep], np.ones(len(s.xyz) - 1, np.int32), normals=s.normals[keep] if with_normals else None)
    poses = str(tmp_path / "poses.txt")
    odometry.save_kitti_poses(poses, s.poses)
    return s, ply, poses


def _run_script(s, ply, poses_file, out, *more):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "render_cloud.py"), "--cloud", ply, "--poses", poses_file, "--frames", "1:5",
           "--every", "2", "--K", str(s.K[0, 0]), str(s.K[1, 1]), str(s.K[0, 2]), str(s.K[1, 2]), "--height", "13", "--width", "20",
           "--near", str(s.near), "--far", str(s.far), "--splat", str(U.mixed_splat(20)), "--top", "--save_depth", "--device", "cpu",
           "--out", out] + list(more)
    run = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_render_script_draws_surfels_from_a_ply_with_normals(tmp_path):
    s, ply, poses_file = _tiny_cloud(tmp_path, True)
    out = str(tmp_path / "views")
    text = _run_script(s, ply, poses_file, out, "--surfels", "--surfel_radius", "0.375", "--ambient", "0.5", "--cull", "--save_normals")
    poses = odometry.load_kitti_poses(poses_file)
    turned = cloud_normals.orient_numpy(s.xyz[1:], s.normals[1:], poses)
    want = render.render_surfels_numpy(s.xyz[1:], s.rgb[1:], turned.normal, poses[[1, 3]], s.K, 13, 20, 0.375, near=s.near, far=s.far,
                                       cull=True, ambient=0.5)
    assert want.stats[:, 7].min() > 0
    kinds = ("color.png", "depth.png", "normal.png", "depth.npy", "normal.npy")
    assert sorted(os.listdir(out)) == sorted(["top_color.png", "top_depth.png", "top_normal.png", "top_normal.npy"] +
                                             ["view_%06d_%s" % (n, kind) for n in (1, 3) for kind in kinds])
    assert "normals: the cloud's own" in text
    assert "orientation: " + " ".join("%s %d" % kv for kv in zip(cloud_normals.ORIENT_STATS, turned.stats)) in text
    for j, n in enumerate((1, 3)):
        depth = np.load(os.path.join(out, "view_%06d_depth.npy" % n))
        assert np.array_equal(depth.view(np.uint32), want.depth[j].view(np.uint32))
        normal = np.load(os.path.join(out, "view_%06d_normal.npy" % n))
        assert normal.dtype == np.float32 and np.array_equal(normal.view(np.uint32), want.normal[j].view(np.uint32))
        color = np.asarray(Image.open(os.path.join(out, "view_%06d_color.png" % n)))
        assert np.array_equal(color, want.color[j].transpose(1, 2, 0))
        picture = np.asarray(Image.open(os.path.join(out, "view_%06d_normal.png" % n)))
        hit = want.index[j] >= 0
        assert picture.shape == (13, 20, 3) and not picture[~hit].any() and picture[hit].any()
        assert np.abs(picture[hit].astype(np.float64) / 127.5 - 1.0 - want.normal[j].transpose(1, 2, 0)[hit]).max() <= 1.0 / 255 + 1e-6
        assert "view %06d " % n + " ".join("%s %d" % kv for kv in zip(render.SURFEL_STATS, want.stats[j])) in text
    assert np.asarray(Image.open(os.path.join(out, "top_normal.png"))).any()


def test_render_script_estimates_normals_and_is_unchanged_without_surfels(tmp_path):
    s, ply, poses_file = _tiny_cloud(tmp_path, False)
    out = str(tmp_path / "surfels")
    text = _run_script(s, ply, poses_file, out, "--surfels", "--normal_tau", "4.0", "--min_neighbours", "3", "--max_curvature", "0.3")
    assert "normals: estimated, valid " in text and "orientation: flipped " in text
    assert sorted(os.listdir(out)) == sorted(["top_color.png", "top_depth.png", "top_normal.png"] + [
        "view_%06d_%s" % (n, kind) for n in (1, 3) for kind in ("color.png", "depth.png", "normal.png", "depth.npy")])
    # without --surfels: the same bytes and the same text from two runs, and the text and files the point renderer always wrote
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    text_a, text_b = _run_script(s, ply, poses_file, a), _run_script(s, ply, poses_file, b)
    assert text_a == text_b and "culled" not in text_a and "orientation" not in text_a
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) == sorted(["top_color.png", "top_depth.png"] + [
        "view_%06d_%s" % (n, kind) for n in (1, 3) for kind in ("color.png", "depth.png", "depth.npy")])
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name
    poses = odometry.load_kitti_poses(poses_file)
    want = render.render_numpy(s.xyz[1:], s.rgb[1:], poses[[1, 3]], s.K, 13, 20, near=s.near, far=s.far, splat=U.mixed_splat(20))
    for j, n in enumerate((1, 3)):
        assert "view %06d points %d out_of_range %d outside %d drawn %d pixels_hit %d share_hit %.4f" % (
            (n,) + tuple(want.stats[j]) + (want.stats[j, 4] / 260,)) in text_a.splitlines()
        assert np.array_equal(np.load(os.path.join(a, "view_%06d_depth.npy" % n)).view(np.uint32), want.depth[j].view(np.uint32))


def test_eval_script_orients_the_saved_reference_normals(tmp_path):
    from tests import cloud_align_util as A
    from tests import cloud_plane_util as P
    pred, ref, _ = A.street_pair("small")
    cloud_ply, ref_ply, poses_file = str(tmp_path / "cloud.ply"), str(tmp_path / "ref.ply"), str(tmp_path / "poses.txt")
    P.save_xyz_ply(cloud_ply, pred)
    P.save_xyz_ply(ref_ply, ref)
    odometry.save_kitti_poses(poses_file, A.trajectory())
    tau = A.STREET_TAU
    common = [sys.executable, os.path.join(ROOT, "scripts", "eval_cloud.py"), "--cloud", cloud_ply, "--ref", ref_ply, "--tau", str(tau),
              "--pred_scale", "1.02", "--device", "cpu"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    plain_ply, turned_ply = str(tmp_path / "plain.ply"), str(tmp_path / "turned.ply")
    plain = subprocess.run(common + ["--save_ref_normals", plain_ply], env=env, capture_output=True, text=True, timeout=600)
    turned = subprocess.run(common + ["--save_ref_normals", turned_ply, "--orient_normals", "--poses", poses_file, "--frames", "5:30"],
                            env=env, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and turned.returncode == 0, plain.stdout + plain.stderr + turned.stdout + turned.stderr
    poses = odometry.load_kitti_poses(poses_file)[5:30]
    estimator = cloud_normals.CloudNormals("cpu", 2 * tau)
    want = estimator.estimate(ref.astype(np.float32), poses=poses)
    got, before = cloud.load_ply(turned_ply), cloud.load_ply(plain_ply)
    normal = lambda rec: np.stack([rec["nx"], rec["ny"], rec["nz"]], 1)
    assert np.array_equal(normal(got), want.normal.astype(np.float32))
    assert np.array_equal(normal(before), estimator.estimate(ref.astype(np.float32)).normal.astype(np.float32))      # unchanged without the flag
    assert np.array_equal(np.abs(normal(got)), np.abs(normal(before))) and want.stats["orient_flipped"] > 1000 and want.stats["orient_kept"] > 1000
    assert "orient_flipped %d orient_kept %d orient_none %d orient_invalid %d" % tuple(
        want.stats["orient_" + k] for k in cloud_normals.ORIENT_STATS) in turned.stdout and "orient_flipped" not in plain.stdout
    # everything but the line about the saved normals is what the run without the flag prints: the scores do not change
    strip = lambda text: [l for l in text.splitlines() if not l.startswith("saved ")]
    assert strip(turned.stdout) == strip(plain.stdout)
    lone = subprocess.run(common + ["--save_ref_normals", turned_ply, "--orient_normals"], env=env, capture_output=True, text=True, timeout=600)
    assert lone.returncode == 2 and "--orient_normals" in lone.stderr
