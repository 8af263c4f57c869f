"""tripled_amd.cloud without a GPU: the numpy statements against a brute-force per-point fusion in plain Python (tests/cloud_util.py),
the camera points against the reference's Backproject (oracle.geometry.backproject), key packing, every cause of an invalid pixel,
the PLY round trip, SceneFuser(device='cpu') and scripts/reconstruct.py on a tiny tree, and the argument checks of the new C entry
points.  Everything but the float32 Backproject comparison is exact."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, native
from tests import cloud_util as U
from tests import odom_util
from tests.infer_util import build_model, ROOT


@pytest.mark.parametrize("seed,B,H,W,over", [
    (0, 3, 7, 13, {}),
    (1, 2, 9, 20, dict(stride=3, border=2)),
    (2, 3, 6, 11, dict(edge=0.15, border=1)),
    (3, 2, 5, 17, dict(edge=0.3, depth_scale=1.7, pose_scale=0.5, min_count=2)),
    (4, 2, 8, 12, dict(edge=0.3, stride=2)),
])
def test_fuse_numpy_is_the_per_point_fusion(seed, B, H, W, over):
    depth, color, poses, inv_K = U.scene(seed, B, H, W)
    params = dict(U.PARAMS, **over)
    min_count = params.pop("min_count", 1)
    got = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, min_count=min_count, **params)
    keys, sums, xyz, rgb, count, causes = U.brute_force(depth, color, poses, inv_K, U.VOXEL, min_count=min_count, **params)
    assert causes[0] >= len(keys) >= 1 and ("stride" in over or sums[:, 0].max() > 1)      # dense cases: voxels hold several points
    assert np.array_equal(got.keys, keys)
    assert np.array_equal(got.xyz.view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(got.rgb, rgb) and np.array_equal(got.count, count)
    assert [got.stats[name] for name in cloud.CAUSES] == causes and got.stats["points"] == B * H * W
    # the table on its own, and the rows form of it
    key, payload, _ = cloud.keys_numpy(depth, color, poses, inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    tkeys, tsums = cloud.voxel_table_numpy(key, payload)
    keep = tsums[:, 0] >= min_count
    assert np.array_equal(tkeys[keep], keys) and np.array_equal(tsums[keep], sums)
    again_keys, again_sums = cloud.voxel_table_numpy(np.concatenate([tkeys, tkeys[:3]]), np.concatenate([tsums, tsums[:3]]))
    assert np.array_equal(again_keys, tkeys) and np.array_equal(again_sums[:3], 2 * tsums[:3]) and np.array_equal(again_sums[3:], tsums[3:])


def test_camera_points_are_the_references_backproject():
    """oracle.geometry.backproject computes ray = m0 x + m1 y + m2 and depth * ray in float32: two products, two sums and one more
    product, five roundings of at most 2^-24 relative each, every one on a quantity no larger than the largest partial result M of the
    ray times the depth.  The float64 statement's own error (2^-53) is nothing next to it.  Bound: 5 x 2^-24 x max|depth| x M."""
    from oracle import geometry
    H, W = 12, 40
    K, inv_K = U.intrinsics(H, W)
    depth = U.scene(5, 2, H, W, special=False)[0]
    inv32 = torch.from_numpy(np.linalg.pinv(K)).unsqueeze(0).repeat(2, 1, 1)
    ref = geometry.backproject(torch.from_numpy(depth).unsqueeze(1), inv32)[:, :3].reshape(2, 3, H, W).numpy()
    m = inv32[0, :3, :3].numpy().astype(np.float64)                  # the same float32 entries, widened
    got = cloud.camera_points_numpy(depth, m)
    partial = max(np.abs(m[:, 0]).max() * (W - 1), np.abs(m[:, 1]).max() * (H - 1), np.abs(m[:, 2]).max())
    partial = max(partial, np.abs(got / depth[None].astype(np.float64)).max())
    bound = 5 * 2.0 ** -24 * float(np.abs(depth).max()) * partial
    err = float(np.abs(got.transpose(1, 0, 2, 3) - ref.astype(np.float64)).max())
    print("camera points vs float32 Backproject: max error %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    for k in range(3):                                                # pixel (u, v) at integer coordinates, no half-pixel offset:
        assert np.array_equal(got[k, :, 0, 0], depth[:, 0, 0].astype(np.float64) * m[k, 2])      # the ray of pixel (0, 0) is m's last column


def test_key_pack_and_unpack():
    edge = cloud.HALF
    ix = np.array([0, -1, 1, -edge, edge - 1, 5, -7, edge - 1])
    iy = np.array([0, -1, 1, edge - 1, -edge, -6, 8, edge - 1])
    iz = np.array([0, -1, 1, 0, 0, 7, -9, edge - 2])
    key = cloud.pack_key(ix, iy, iz)
    assert key.dtype == np.int64 and (key >= 0).all() and (key < cloud.INVALID_KEY).all()
    back = cloud.unpack_key(key)
    assert all(np.array_equal(a, b) for a, b in zip(back, (ix, iy, iz)))
    # key order is (x, y, z) lexicographic order, negative coordinates first
    cells = sorted(zip(ix.tolist(), iy.tolist(), iz.tolist()))
    assert [tuple(int(v[i]) for v in cloud.unpack_key(np.sort(key))) for i in range(len(key))] == cells
    assert int(cloud.pack_key(edge - 1, edge - 1, edge - 1)) == cloud.INVALID_KEY      # the sentinel's own voxel: keys_numpy refuses it
    for bad in (edge, -edge - 1):
        with pytest.raises(ValueError):
            cloud.pack_key(bad, 0, 0)
    rows = cloud.unpack_payload(np.array([1023 | (5 << 10) | (1 << 20) | (255 << 30) | (7 << 38) | (128 << 46)], np.uint64))
    assert rows.tolist() == [[1, 1023, 5, 1, 255, 7, 128]]


def test_every_cause_of_an_invalid_pixel_is_counted():
    H, W = 8, 10
    inv_K = U.intrinsics(H, W)[1]
    depth = np.full((2, H, W), 4.0, np.float32)
    depth[0, 3, 3] = np.nan          # depth; its four neighbours fall to the edge filter (a non-finite neighbour)
    depth[0, 5, 6] = 100.0           # beyond max_range; its neighbours differ from it by more than edge x min
    depth[0, 2, 7] = 0.1             # below min_depth; likewise
    color = np.zeros((2, 3, H, W), np.uint8)
    poses = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]), (2, 1, 1))
    poses[1, :, 3] = [1.0e6, 0.0, 0.0]                                # the whole second frame: out of the key range
    got = cloud.fuse_numpy(depth, color, poses, inv_K, 0.25, stride=1, border=1, min_depth=0.5, max_range=40.0, edge=0.2)
    inner = (H - 2) * (W - 2)
    want = {"points": 2 * H * W, "invalid_stride": 0, "invalid_border": 2 * (H * W - inner), "invalid_depth": 3, "invalid_edge": 12,
            "invalid_range": inner, "valid": inner - 3 - 12}
    assert {k: got.stats[k] for k in want} == want
    assert got.stats["voxels"] == len(got.keys) and got.stats["voxels_dropped"] == 0
    lattice = cloud.fuse_numpy(depth, color, poses, inv_K, 0.25, stride=3, border=0, min_depth=0.5, max_range=40.0, edge=0.0)
    on = len(range(0, H, 3)) * len(range(0, W, 3))
    assert lattice.stats["invalid_stride"] == 2 * (H * W - on) and lattice.stats["invalid_range"] == on
    dropped = cloud.fuse_numpy(depth, color, poses, inv_K, 0.25, stride=1, border=1, min_depth=0.5, max_range=40.0, edge=0.2, min_count=2)
    assert dropped.stats["voxels"] == got.stats["voxels"] and dropped.stats["voxels_dropped"] == int((got.count < 2).sum()) > 0
    assert len(dropped.keys) == dropped.stats["voxels"] - dropped.stats["voxels_dropped"]


def test_finish_rounds_colour_halves_up_and_saturates_the_count():
    keys = cloud.pack_key([0, -3, 2], [1, 0, -2], [0, 5, 9])
    sums = np.array([[2, 0, 1023, 1, 1, 3, 510],                      # means 0.5 -> 1, 1.5 -> 2, 255
                     [2 ** 31, 0, 0, 0, 2 ** 30, 2 ** 31, 255 * 2 ** 31],      # means 0.5 -> 1, 1, 255; count saturates
                     [4, 6, 6, 6, 5, 6, 7]], np.int64)                  # means 1.25 -> 1, 1.5 -> 2, 1.75 -> 2
    xyz, rgb, count, keep = cloud.finish_numpy(keys, sums, 0.5, min_count=3)
    assert rgb.tolist() == [[1, 2, 255], [1, 1, 255], [1, 2, 2]]
    assert count.tolist() == [2, 2 ** 31 - 1, 4] and keep.tolist() == [False, True, True]
    assert xyz[0].tolist() == [np.float32((0 + (0 / 2 + 0.5) / 1024.0) * 0.5), np.float32((1 + (1023 / 2 + 0.5) / 1024.0) * 0.5),
                               np.float32((0 + (1 / 2 + 0.5) / 1024.0) * 0.5)]
    assert xyz[2, 0] == np.float32((2 + (6 / 4 + 0.5) / 1024.0) * 0.5) and xyz[1, 0] < 0


def test_ply_round_trip(tmp_path):
    g = np.random.default_rng(0)
    xyz = g.standard_normal((37, 3)).astype(np.float32)
    rgb = g.integers(0, 256, (37, 3), dtype=np.uint8)
    count = g.integers(1, 2 ** 31 - 1, 37).astype(np.int32)
    path = str(tmp_path / "cloud.ply")
    cloud.save_ply(path, xyz, torch.from_numpy(rgb), count)
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode("ascii").splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 37"]
    assert head[3:] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                        "property uchar blue", "property int count"]
    assert len(raw) == raw.index(b"end_header\n") + len(b"end_header\n") + 37 * 19
    back = cloud.load_ply(path)
    assert back.dtype == cloud.PLY_DTYPE and len(back) == 37
    assert np.array_equal(np.stack([back["x"], back["y"], back["z"]], 1).view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(np.stack([back["red"], back["green"], back["blue"]], 1), rgb) and np.array_equal(back["count"], count)
    cloud.save_ply(path, xyz[:0], rgb[:0], count[:0])
    assert len(cloud.load_ply(path)) == 0
    with open(path, "wb") as f:
        f.write(b"not a ply\n")
    with pytest.raises(ValueError):
        cloud.load_ply(path)
    with pytest.raises(ValueError):
        cloud.save_ply(path, xyz, rgb[:5], count)


def _tree(tmp_path, n_frames=4):
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, n_frames, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, n_frames), 64, 96, [0, 1], is_train=False, img_ext=".png")
    return gt, ds


FUSER = dict(voxel=0.5, batch_size=3, stride=2, border=1, min_depth=0.1, max_range=50.0, edge=0.5)


def test_scene_fuser_on_the_host(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96).train()
    fuser = cloud.SceneFuser(model, 64, 96, "cpu", **FUSER)
    debug = {}
    got = fuser.fuse(ds, debug=debug)
    assert model.training and all(m.training for m in model.modules())
    depth, poses = debug["depth"].numpy(), debug["poses"]
    assert depth.shape == (4, 64, 96) and depth.dtype == np.float32 and poses.shape == (4, 3, 4) and poses.dtype == np.float64
    assert np.array_equal(poses[0], np.eye(4)[:3])
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    inv_K = cloud.dataset_inv_K(ds)
    assert np.allclose(inv_K @ np.asarray(ds[0]["K"], np.float64)[:3, :3], np.eye(3), atol=1e-12)
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    U.assert_clouds_equal(got, cloud.fuse_numpy(depth, frames, poses, inv_K, FUSER["voxel"], **params))
    assert got.stats["points"] == 4 * 64 * 96 and got.stats["valid"] > 0 and len(got.keys) == got.stats["voxels"] > 0
    assert np.all(np.diff(got.keys) > 0)
    # given poses (the ground truth) and a window of frames
    sub = fuser.fuse(ds, poses=gt, frames=(1, 3), debug=debug)
    assert np.array_equal(debug["poses"], gt) and debug["depth"].shape[0] == 2
    U.assert_clouds_equal(sub, cloud.fuse_numpy(debug["depth"].numpy(), frames[1:3], gt[1:3], inv_K, FUSER["voxel"], **params))
    with pytest.raises(ValueError):
        fuser.fuse(ds, poses=gt[:3])
    with pytest.raises(ValueError):
        fuser.fuse(ds, frames=(2, 9))


def test_argument_errors():
    depth, color, poses, inv_K = U.scene(0, 2, 4, 6)
    model = build_model("cfg_kitti_fm", 64, 96)
    for bad in (dict(voxel=0.0), dict(voxel=float("nan")), dict(stride=0), dict(border=-1), dict(edge=-0.1), dict(min_count=0),
                dict(min_depth=2.0, max_range=1.0)):
        with pytest.raises(ValueError):
            cloud.fuse_numpy(depth, color, poses, inv_K, **dict(dict(voxel=0.25), **bad))
        with pytest.raises(ValueError):
            cloud.SceneFuser(model, 64, 96, "cpu", **bad)
    with pytest.raises(ValueError):
        cloud.SceneFuser(model, 64, 96, "cpu", batch_size=0)
    with pytest.raises(ValueError):
        cloud.SceneFuser(model, 64, 96, "cpu", precision="bf16")      # the HIP device's path
    with pytest.raises(ValueError):
        cloud.keys_numpy(depth, color[:, :2], poses, inv_K)
    with pytest.raises(ValueError):
        cloud.keys_numpy(depth, color, poses[:1], inv_K)
    with pytest.raises(ValueError):
        cloud.keys_numpy(depth, color, poses, np.eye(2))
    with pytest.raises(ValueError):
        cloud.voxel_table_numpy(np.zeros(3, np.int64), np.zeros(2, np.uint64))


def test_device_entry_points_refuse_host_tensors():
    depth, color, poses, inv_K = (torch.from_numpy(a) for a in U.scene(0, 2, 4, 6))
    key = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(native.NativeLibraryError):
        cloud.keys_hip(depth, color, poses, inv_K)
    with pytest.raises(native.NativeLibraryError):
        cloud.heads_hip(key)
    with pytest.raises(native.NativeLibraryError):
        cloud.reduce_hip(key, key, None, key, 1)
    with pytest.raises(native.NativeLibraryError):
        cloud.finish_hip(key, torch.zeros(4, 7, dtype=torch.int64), 0.25)
    with pytest.raises(native.NativeLibraryError):
        cloud.merge_hip(key, torch.zeros(4, 7, dtype=torch.int64), key, torch.zeros(4, 7, dtype=torch.int64))
    with pytest.raises(native.NativeLibraryError):
        cloud.fuse_hip(depth, color, poses, inv_K, 0.25)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the checks come first
    ik = (ctypes.c_double * 9)(*([1.0] * 9))
    keys_ok = [one, one, one, ik, 1, 8, 8, 1.0, 1.0, 4.0, 1, 0, 0.1, 10.0, 0.0, one, one, None, None]
    assert lib.td_cloud_keys(None, None, None, None, 1, 8, 8, 1.0, 1.0, 4.0, 1, 0, 0.1, 10.0, 0.0, None, None, None, None) == -1
    for pos in (0, 1, 2, 3, 15, 16):
        args = list(keys_ok)
        args[pos] = None
        assert lib.td_cloud_keys(*args) == -1, pos
    for pos, bad in ((4, -1), (5, 0), (6, 0), (9, 0.0), (9, float("nan")), (10, 0), (11, -1), (14, -1.0)):
        args = list(keys_ok)
        args[pos] = bad
        assert lib.td_cloud_keys(*args) == -1, (pos, bad)
    assert lib.td_cloud_keys(*(keys_ok[:4] + [0] + keys_ok[5:])) == 0                  # B = 0: a no-op, nothing is launched
    assert lib.td_cloud_heads(None, 4, None, None) == -1 and lib.td_cloud_heads(one, -1, one, None) == -1
    assert lib.td_cloud_heads(one, 0, one, None) == 0
    for fn in (lib.td_cloud_reduce_packed, lib.td_cloud_reduce_rows):
        assert fn(None, None, None, None, 4, 4, 2, None, None, None) == -1
        for pos in (0, 1, 3, 7, 8):
            args = [one, one, None, one, 4, 4, 2, one, one, None]
            args[pos] = None
            assert fn(*args) == -1, pos
        assert fn(one, one, None, one, 4, -1, 2, one, one, None) == -1
        assert fn(one, one, None, one, 4, 4, 5, one, one, None) == -1                  # more rows than elements
        assert fn(one, one, None, one, -1, 4, 2, one, one, None) == -1
        assert fn(one, one, None, one, 4, 0, 0, one, one, None) == 0 and fn(one, one, None, one, 4, 4, 0, one, one, None) == 0
    assert lib.td_cloud_finish(None, None, 4, 0.25, 1, None, None, None, None, None) == -1
    for pos in (0, 1, 5, 6, 7, 8):
        args = [one, one, 4, 0.25, 1, one, one, one, one, None]
        args[pos] = None
        assert lib.td_cloud_finish(*args) == -1, pos
    assert lib.td_cloud_finish(one, one, 4, 0.0, 1, one, one, one, one, None) == -1
    assert lib.td_cloud_finish(one, one, -1, 0.25, 1, one, one, one, one, None) == -1
    assert lib.td_cloud_finish(one, one, 0, 0.25, 1, one, one, one, one, None) == 0


def test_reconstruct_script_on_the_host(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    ckpt = str(tmp_path / "model.pth")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    out = str(tmp_path / "out" / "cloud.ply")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "reconstruct.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
           "--checkpoint", ckpt, "--data_path", str(tmp_path), "--sequence", "9", "--height", "64", "--width", "96", "--device", "cpu",
           "--voxel", "0.5", "--stride", "2", "--border", "1", "--max_range", "50", "--edge", "0.5", "--batch_size", "3", "--out", out]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    back = cloud.load_ply(out)
    want = cloud.SceneFuser(model, 64, 96, "cpu", **FUSER).fuse(ds)
    assert back.dtype == cloud.PLY_DTYPE and len(back) == len(want.keys) > 0
    assert np.array_equal(np.stack([back["x"], back["y"], back["z"]], 1).view(np.uint32), want.xyz.view(np.uint32))
    assert np.array_equal(np.stack([back["red"], back["green"], back["blue"]], 1), want.rgb) and np.array_equal(back["count"], want.count)
    assert "points %d" % want.stats["points"] in run.stdout and "voxels %d" % want.stats["voxels"] in run.stdout
    # ground-truth poses from a file, a window of frames
    out2 = str(tmp_path / "gt.ply")
    run = subprocess.run(cmd[:-1] + [out2, "--poses", os.path.join(str(tmp_path), "poses", "09.txt"), "--frames", "1:3",
                                     "--depth_scale", "2.0"], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    want = cloud.SceneFuser(model, 64, 96, "cpu", depth_scale=2.0, **FUSER).fuse(ds, poses=gt, frames=(1, 3))
    assert len(cloud.load_ply(out2)) == len(want.keys)
