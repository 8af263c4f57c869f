"""tripled_amd.render without a GPU: the numpy statement against the literal per-pixel loop on a scene with every deciding point
planted (tests/render_util.py), an analytic case, the top view, the refusals, scripts/render_cloud.py on a tiny PLY and the poses that
scripts/reconstruct.py --save_poses writes.  Every comparison of rendered maps is exact: the outputs are comparisons and conversions of
a fixed sequence of individually rounded float64 operations."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import tripled_amd  # noqa: F401
from tripled_amd import cloud, infer, native, odometry, render
from tests import odom_util
from tests import render_util as U
from tests.infer_util import build_model, ROOT

C, H, W, V = 3, 9, 14, 700
_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        _CACHE["scene"] = U.scene(0, V, C, H, W)
    return _CACHE["scene"]


def _statement(mode):
    """render_numpy of the shared scene in one of the four modes, computed once."""
    if mode not in _CACHE:
        s = _scene()
        _CACHE[mode] = render.render_numpy(s.xyz, s.rgb, s.poses, s.K, H, W, **U.render_args(s, **U.modes(W)[mode]))
    return _CACHE[mode]


@pytest.mark.parametrize("mode", ["none", "mixed", "saturated", "ortho"])
def test_render_numpy_is_the_per_pixel_loop(mode):
    s = _scene()
    want = render.render_bruteforce(s.xyz, s.rgb, s.poses, s.K, H, W, **U.render_args(s, **U.modes(W)[mode]))
    U.assert_rendered_equal(_statement(mode), want)


@pytest.mark.parametrize("mode", ["none", "mixed", "saturated", "ortho"])
def test_the_planted_points_exercise_every_outcome(mode):
    s, got = _scene(), _statement(mode)
    p, kw = s.planted, U.modes(W)[mode]
    assert got.depth.dtype == np.float32 and got.color.dtype == np.uint8 and got.index.dtype == np.int32 and got.stats.dtype == np.int64
    assert got.depth.shape == (C, H, W) and got.color.shape == (C, 3, H, W) and got.index.shape == (C, H, W) and got.stats.shape == (C, 5)
    assert (got.stats.sum(0) > 0).all() and (got.stats[:, 0] == V).all()          # every column counts something
    assert np.array_equal(got.stats[:, 1:4].sum(1), got.stats[:, 0])              # every point has exactly one outcome
    assert np.array_equal(got.stats[:, 4], (got.index >= 0).reshape(C, -1).sum(1))
    assert got.index.max() >= U.SPECIALS and got.index.max() < V                   # real indices, random points among them
    if mode == "saturated":                                                       # 17 x 17 squares leave nothing of 9 x 14 open
        assert got.index.min() >= 0
    else:
        assert got.index.min() == -1
    hit = got.index >= 0
    assert np.array_equal(got.depth > 0, hit) and not got.color.transpose(0, 2, 3, 1)[~hit].any()
    assert np.array_equal(got.color.transpose(0, 2, 3, 1)[hit], s.rgb[got.index[hit]])
    # camera 0: where the statement puts the planted points, and what that means in the maps
    ui, vi, r, zf, in_range, visible = render.project_numpy(s.xyz, s.poses[0], s.K.reshape(-1), s.near, s.far, kw["splat"], 1.0,
                                                            kw.get("ortho", False), H, W)
    assert not in_range[[p["nan"], p["behind"], p["beyond"]]].any() and in_range[list(p["tie"])].all()
    low, high = p["tie"]
    assert zf[low] == zf[high] == np.float32(s.near) and visible[low] and visible[high]
    tv, tu = int(vi[low]), int(ui[low])
    assert got.index[0, tv, tu] == low and got.depth[0, tv, tu] == np.float32(s.near)      # equal float32(z): the lower index wins
    assert np.array_equal(got.color[0, :, tv, tu], s.rgb[low])
    if mode != "ortho":
        assert (tv, tu) == p["tie_pixel"]
        for i, (v, u) in zip(p["half"], p["half_pixels"]):                        # k + 0.5 goes to the even neighbour
            assert (int(vi[i]), int(ui[i])) == (v, u), (i, vi[i], ui[i])
    if mode == "none":
        assert (r[in_range] == 0).all() and not visible[list(p["straddle"])].any()
    if mode == "mixed":
        assert r[p["near"]] == render.MAX_SPLAT and set(r[in_range]) >= {0.0, 1.0, 6.0, 8.0}
        assert visible[list(p["straddle"])].all()                                 # the centre is outside, the square reaches in
        for i, (v, u) in zip(p["straddle"], ((H // 2, 0), (H // 2, W - 1), (0, W // 2), (H - 1, W // 2))):
            assert not (0 <= ui[i] <= W - 1 and 0 <= vi[i] <= H - 1) and got.depth[0, v, u] <= zf[i]
    if mode == "saturated":
        assert (r[in_range] == render.MAX_SPLAT).all()


def test_every_scene_of_the_device_tests_can_be_built():
    for seed, (c, h, w, v) in enumerate(((1, 1, 1, 3), (3, 9, 14, 700), (2, 3, 300, 1000), (64, 5, 7, 20011), (2, 33, 65, 0))):
        s = U.scene(seed, v, c, h, w)
        assert s.xyz.shape == (v, 3) and s.poses.shape == (c, 3, 4) and bool(s.planted) == (v >= 2 * U.SPECIALS)
    got = render.render_numpy(*U.scene(0, 3, 1, 1, 1)[:4], 1, 1, near=U.NEAR, far=U.FAR)
    assert got.index[0, 0, 0] == 0 and got.depth[0, 0, 0] == 1.0
    empty = render.render_numpy(*U.scene(4, 0, 2, 33, 65)[:4], 33, 65, near=U.NEAR, far=U.FAR, background=(1, 2, 3))
    assert not empty.stats.any() and (empty.index == -1).all() and not empty.depth.any()
    assert (empty.color == np.array([1, 2, 3], np.uint8).reshape(1, 3, 1, 1)).all()


def test_one_point_straight_ahead():
    """A point at depth d on the optical axis lands on the principal point with depth float32(d), whatever the camera's pose."""
    K = np.array([[100.0, 0.0, 8.0], [0.0, 90.0, 5.0], [0.0, 0.0, 1.0]])
    a, d = 0.4, 3.3
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    t = np.array([1.0, -2.0, 0.5])
    pose = np.concatenate([R, t[:, None]], 1)[None]
    xyz = (t + d * R[:, 2])[None].astype(np.float32)
    rgb = np.array([[10, 20, 30]], np.uint8)
    for fn in (render.render_numpy, render.render_bruteforce):
        got = fn(xyz, rgb, pose, K, 11, 17, near=0.1, far=10.0, background=(9, 8, 7))
        assert got.stats.tolist() == [[1, 0, 0, 1, 1]] and np.argwhere(got.index == 0).tolist() == [[0, 5, 8]]
        assert abs(float(got.depth[0, 5, 8]) - d) <= 2.0 ** -22 * d             # float32 of the point, float32 of z: two roundings
        assert got.color[0, :, 5, 8].tolist() == [10, 20, 30] and got.color[0, :, 0, 0].tolist() == [9, 8, 7]
    ident = np.eye(4)[None, :3]
    got = render.render_numpy(np.array([[0.0, 0.0, d]], np.float32), rgb, ident, K, 11, 17, near=0.1, far=10.0)
    assert got.depth[0, 5, 8] == np.float32(d)                                  # the identity: exactly float32(d)
    # pose_scale multiplies the translation: half the translation with pose_scale 2 is the same camera
    half = pose.copy()
    half[0, :, 3] *= 0.5
    again = render.render_numpy(xyz, rgb, half, K, 11, 17, near=0.1, far=10.0, pose_scale=2.0)
    assert np.argwhere(again.index == 0).tolist() == [[0, 5, 8]]


def test_top_view():
    xyz = np.array([[-4.0, 1.0, 0.0], [6.0, -1.0, 20.0], [1.0, 0.5, 10.0], [np.nan, 0.0, 0.0]], np.float32)
    rgb = np.arange(12, dtype=np.uint8).reshape(4, 3)
    Ht, Wt, near = 41, 21, 0.5
    pose, K = render.top_view(xyz, Ht, Wt, margin=0.1, near=near)
    assert pose.shape == (3, 4) and K.shape == (3, 3)
    assert np.array_equal(pose[:, :3], [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]])      # x = +x, y = -z, z = +y
    assert np.allclose(pose[:, :3].T @ pose[:, :3], np.eye(3)) and np.isclose(np.linalg.det(pose[:, :3]), 1.0)
    # the box is 10 wide and 20 deep; 80 % of 20 x 40 pixel steps: 16 / 10 and 32 / 20 -> the scale is 1.6, the centre (1, ., 10)
    assert np.isclose(K[0, 0], 1.6) and K[0, 0] == K[1, 1] and (K[0, 2], K[1, 2]) == (10.0, 20.0)
    got = render.render_numpy(xyz, rgb, pose[None], K, Ht, Wt, near=near, far=3 * near + 2.0, ortho=True)
    assert got.stats[0].tolist() == [4, 1, 0, 3, 3]                             # the NaN is out of range, the others are drawn
    where = {int(i): (int(v), int(u)) for i, (v, u) in ((got.index[0, v, u], (v, u)) for v, u in np.argwhere(got.index[0] >= 0))}
    assert where[2] == (20, 10)                                                # the box's centre is the picture's
    assert where[0] == (36, 2) and where[1] == (4, 18)                          # forward (+z) is up, +x is right
    assert got.depth[0, 4, 18] == np.float32(2 * near) and got.depth[0, 36, 2] == np.float32(2 * near + 2.0)      # z >= near: y is down
    with pytest.raises(ValueError):
        render.top_view(xyz[3:], Ht, Wt)
    with pytest.raises(ValueError):
        render.top_view(xyz, Ht, Wt, margin=0.5)


def test_refusals():
    s = _scene()
    ok = dict(near=0.25, far=16.0, splat=0.0)
    for bad in (dict(near=0.0), dict(near=-1.0), dict(near=float("nan")), dict(far=float("inf")), dict(far=0.1), dict(far=float("nan")),
                dict(splat=-0.5), dict(splat=float("inf")), dict(splat=float("nan")), dict(background=(0, 0, 256)), dict(background=(0, 0))):
        for fn in (render.render_numpy, render.render_bruteforce):
            with pytest.raises(ValueError):
                fn(s.xyz, s.rgb, s.poses, s.K, H, W, **dict(ok, **bad))
    for args in ((s.xyz[:, :2], s.rgb, s.poses, s.K, H, W), (s.xyz, s.rgb[:5], s.poses, s.K, H, W), (s.xyz, s.rgb, s.poses[:0], s.K, H, W),
                 (s.xyz, s.rgb, s.poses, np.eye(2), H, W), (s.xyz, s.rgb, s.poses, s.K * np.nan, H, W), (s.xyz, s.rgb, s.poses, s.K, 0, W),
                 (s.xyz, s.rgb, s.poses, s.K, H, -1)):
        with pytest.raises(ValueError):
            render.render_numpy(*args, **ok)
    with pytest.raises(ValueError):
        render.CloudRenderer("cpu", H, W, s.K, near=0.0)
    with pytest.raises(ValueError):
        render.CloudRenderer("cpu", H, W, s.K, batch_size=0)


def test_render_hip_refuses_host_tensors():
    s = _scene()
    xyz, rgb, poses = (torch.from_numpy(a) for a in (s.xyz, s.rgb, s.poses))
    with pytest.raises(native.NativeLibraryError):
        render.render_hip(xyz, rgb, poses, s.K, H, W, near=s.near, far=s.far)
    with pytest.raises(native.NativeLibraryError):
        native.call("td_cloud_render", xyz, rgb, V, poses, (ctypes.c_double * 9)(*s.K.reshape(-1)), C, H, W, 1.0, s.near, s.far, 0.0, 0,
                    0, 0, 0, xyz, 8, xyz, rgb, xyz, xyz)


def test_the_entry_points_reject_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    assert lib.td_cloud_render_workspace_bytes(3, 9, 14) == 3 * 9 * 14 * 8
    assert lib.td_cloud_render_workspace_bytes(65535, 1, 1) == 65535 * 8 and lib.td_cloud_render_workspace_bytes(65536, 1, 1) == 0
    assert lib.td_cloud_render_workspace_bytes(0, 9, 14) == 0 and lib.td_cloud_render_workspace_bytes(1, 0, 14) == 0
    assert lib.td_cloud_render_workspace_bytes(1, 1 << 16, 1 << 15) == 0       # 2^31 pixels
    assert lib.td_cloud_render_workspace_bytes(1, 0x7fffffff, 1) == 0x7fffffff * 8
    one = ctypes.c_void_p(64)          # a non-null, aligned pointer that is never dereferenced: the checks come first
    k = (ctypes.c_double * 9)(8.0, 0.0, 6.5, 0.0, 8.0, 4.0, 0.0, 0.0, 1.0)
    need = 3 * 9 * 14 * 8
    ok = [one, one, 700, one, k, 3, 9, 14, 1.0, 0.25, 16.0, 0.0, 0, 0, 0, 0, one, need, one, one, one, one, None]
    for pos in (0, 1, 3, 4, 16, 18, 19, 20, 21):
        args = list(ok)
        args[pos] = None
        assert lib.td_cloud_render(*args) == -1, pos
    nan, inf = float("nan"), float("inf")
    for pos, bad in ((2, -1), (5, 0), (5, -2), (6, 0), (7, 0), (9, 0.0), (9, -1.0), (9, nan), (10, inf), (10, nan), (10, 0.125),
                     (11, -1.0), (11, inf), (11, nan), (13, 256), (14, -1), (15, 300), (17, need - 8), (16, ctypes.c_void_p(68))):
        args = list(ok)
        args[pos] = bad
        assert lib.td_cloud_render(*args) == -1, (pos, bad)
    for pos, bad in ((5, 65536), (2, 0x7fffffff)):
        args = list(ok)
        args[pos] = bad
        args[17] = 1 << 40
        assert lib.td_cloud_render(*args) == -2, (pos, bad)


def _tiny_cloud(tmp_path):
    s = U.scene(7, 300, 5, 12, 20)
    ply = str(tmp_path / "cloud.ply")
    cloud.save_ply(ply, s.xyz[1:], s.rgb[1:], np.ones(len(s.xyz) - 1, np.int32))      # without the NaN: a top view needs a box
    poses = str(tmp_path / "poses.txt")
    odometry.save_kitti_poses(poses, s.poses)
    return s, ply, poses


def test_render_script_on_the_host(tmp_path):
    s, ply, poses_file = _tiny_cloud(tmp_path)
    Hs, Ws = 12, 20
    out = str(tmp_path / "views")
    splat = U.mixed_splat(Ws)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "render_cloud.py"), "--cloud", ply, "--poses", poses_file, "--frames", "1:5",
           "--every", "2", "--K", str(s.K[0, 0]), str(s.K[1, 1]), str(s.K[0, 2]), str(s.K[1, 2]), "--height", str(Hs), "--width", str(Ws),
           "--near", str(s.near), "--far", str(s.far), "--splat", str(splat), "--top", "--save_depth", "--device", "cpu", "--out", out]
    run = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    poses = odometry.load_kitti_poses(poses_file)                              # as the script reads them: rounded to %1.8e
    want = render.render_numpy(s.xyz[1:], s.rgb[1:], poses[[1, 3]], s.K, Hs, Ws, near=s.near, far=s.far, splat=splat)
    assert want.stats[:, 4].min() > 0
    assert sorted(os.listdir(out)) == sorted(["top_color.png", "top_depth.png"] + [
        "view_%06d_%s" % (n, kind) for n in (1, 3) for kind in ("color.png", "depth.png", "depth.npy")])
    for j, n in enumerate((1, 3)):
        depth = np.load(os.path.join(out, "view_%06d_depth.npy" % n))
        assert depth.dtype == np.float32 and np.array_equal(depth.view(np.uint32), want.depth[j].view(np.uint32))
        color = np.asarray(Image.open(os.path.join(out, "view_%06d_color.png" % n)))
        assert color.shape == (Hs, Ws, 3) and np.array_equal(color, want.color[j].transpose(1, 2, 0))
        picture = np.asarray(Image.open(os.path.join(out, "view_%06d_depth.png" % n)))
        hit = want.depth[j] > 0
        magma = infer.colorize_numpy(want.depth[j], want.depth[j][hit].min(), want.depth[j][hit].max())
        assert picture.shape == (Hs, Ws, 3) and not picture[~hit].any() and np.array_equal(picture[hit], magma[hit])
        assert "view %06d points %d out_of_range %d outside %d drawn %d pixels_hit %d" % ((n,) + tuple(want.stats[j])) in run.stdout
    top = np.asarray(Image.open(os.path.join(out, "top_color.png")))
    assert top.shape == (Hs, Ws, 3) and top.any() and np.asarray(Image.open(os.path.join(out, "top_depth.png"))).shape == (Hs, Ws, 3)
    assert "mean share of pixels hit %.4f over 2 views" % (want.stats[:, 4].mean() / (Hs * Ws)) in run.stdout.splitlines()[-1]
    # CloudRenderer on the host is the statement, whatever the batch size
    got = render.CloudRenderer("cpu", Hs, Ws, s.K, near=s.near, far=s.far, splat=splat, batch_size=1).render(s.xyz[1:], s.rgb[1:], poses[[1, 3]])
    U.assert_rendered_equal(got, want)


def test_reconstruct_script_saves_the_poses_it_fused(tmp_path):
    """--save_poses writes SceneFuser.poses, the model's own here, and they come back through load_kitti_poses at the text's
    precision (%1.8e: relative 5e-9 per entry; the entries are at most a few units)."""
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    odom_util.make_sequence_tree(str(tmp_path), 9, 3, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, 3), 64, 96, [0, 1], is_train=False, img_ext=".png")
    model = build_model("cfg_kitti_fm", 64, 96)
    ckpt = str(tmp_path / "model.pth")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    out, saved = str(tmp_path / "cloud.ply"), str(tmp_path / "out" / "poses.txt")
    fuser_args = dict(voxel=0.5, batch_size=3, stride=2, border=1, min_depth=0.1, max_range=50.0, edge=0.5)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "reconstruct.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
           "--checkpoint", ckpt, "--data_path", str(tmp_path), "--sequence", "9", "--height", "64", "--width", "96", "--device", "cpu",
           "--voxel", "0.5", "--stride", "2", "--border", "1", "--max_range", "50", "--edge", "0.5", "--batch_size", "3", "--out", out,
           "--save_poses", saved]
    run = subprocess.run(cmd, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "saved 3 poses to %s" % saved in run.stdout
    fuser = cloud.SceneFuser(model, 64, 96, "cpu", **fuser_args)
    assert fuser.poses is None
    debug = {}
    fuser.fuse(ds, debug=debug)
    assert isinstance(fuser.poses, np.ndarray) and fuser.poses.dtype == np.float64 and fuser.poses.shape == (3, 3, 4)
    assert np.array_equal(fuser.poses, debug["poses"]) and np.array_equal(fuser.poses[0], np.eye(4)[:3])
    back = odometry.load_kitti_poses(saved)
    assert back.shape == (3, 3, 4) and np.abs(back[1:, :, 3]).max() > 0
    np.testing.assert_allclose(back, fuser.poses, rtol=1e-8, atol=1e-8 * np.abs(fuser.poses).max())
    # given poses are kept as they are, and a cloud fused with saved poses can be drawn from them
    gt = odometry.load_kitti_poses(os.path.join(str(tmp_path), "poses", "09.txt"))
    fuser.fuse(ds, poses=gt)
    assert np.array_equal(fuser.poses, gt)
    points = cloud.load_ply(out)
    xyz = np.stack([points["x"], points["y"], points["z"]], 1)
    rgb = np.stack([points["red"], points["green"], points["blue"]], 1)
    K = cloud.dataset_K(ds)
    seen = render.CloudRenderer("cpu", 64, 96, K, near=0.1, far=50.0, splat=0.5).render(xyz, rgb, back)
    assert seen.stats[:, 4].min() > 0
