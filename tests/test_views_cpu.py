"""The multi-view filter of tripled_amd.cloud without a GPU: views_numpy against the vote count one pixel at a time in plain Python
(tests/views_util.py), against the analytic truth of a plane seen by a moving camera, fuse_numpy and SceneFuser(device='cpu') with
``min_views``, scripts/reconstruct.py --min_views, and the argument checks of td_cloud_views.  Every comparison is exact."""
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
from tests import views_util as V
from tests.infer_util import build_model, ROOT


# ---- 1. the statement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("N,H,W", [(3, 2, 2), (3, 5, 7), (5, 16, 24)])
def test_views_numpy_is_the_per_pixel_count(N, H, W, radius):
    depth, _, poses, inv_K, K = V.scene(N * H + radius, N, H, W)
    if N < 2 * radius + 1:          # three frames do not hold a window of five
        with pytest.raises(ValueError):
            cloud.views_numpy(depth, poses, inv_K, K, radius, 0.03, **V.RANGE)
        return
    got = cloud.views_numpy(depth, poses, inv_K, K, radius, 0.03, **V.RANGE)
    want = V.brute_force(depth, poses, inv_K, K, radius, 0.03, **V.RANGE)
    assert got.dtype == np.uint8 and got.shape == (N, H, W) and np.array_equal(got, want)
    if H * W > 4:          # the inputs exercise the outcomes: pixels nobody confirms, pixels every neighbour confirms, some in between
        assert got.min() == 0 and got.max() == 2 * radius and len(np.unique(got)) > 2
    # scales other than 1: the same statement on scaled quantities, again against the per-pixel count
    scales = dict(depth_scale=1.7, pose_scale=0.6, min_depth=1.0, max_range=17.0)
    assert np.array_equal(cloud.views_numpy(depth, poses, inv_K, K, radius, 0.05, **scales),
                          V.brute_force(depth, poses, inv_K, K, radius, 0.05, **scales))


def test_the_smallest_frame_has_votes():
    """2 x 2: all four taps are the whole frame.  A camera that only moves forward projects the pixel at the principal point, (1, 1),
    onto itself, the last column and the last row: x0 = min(1, W-2) = 0 with fx = 1."""
    depth, _, poses, inv_K, K = V.scene(1, 3, 2, 2, special=False, angle=0.0, jitter=0.0)
    got = cloud.views_numpy(depth, poses, inv_K, K, 1, 0.03, **V.RANGE)
    assert np.array_equal(got, V.brute_force(depth, poses, inv_K, K, 1, 0.03, **V.RANGE)) and got[:, 1, 1].max() >= 1 and got.max() == 2


@pytest.mark.parametrize("centres,bounds", [((2, 5), None), ((1, 4), (1, 6)), ((3, 3), (0, 7)), (None, (2, 7)), ((6, 7), (2, 7))])
def test_centre_sub_ranges_and_narrower_bounds(centres, bounds):
    depth, _, poses, inv_K, K = V.scene(21, 7, 6, 9)
    got = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.03, centres=centres, bounds=bounds, **V.RANGE)
    want = V.brute_force(depth, poses, inv_K, K, 2, 0.03, centres=centres, bounds=bounds, **V.RANGE)
    assert np.array_equal(got, want)
    if bounds is None:          # a sub-range of centres is a slice of the whole
        assert np.array_equal(got, cloud.views_numpy(depth, poses, inv_K, K, 2, 0.03, **V.RANGE)[centres[0]:centres[1]])
    elif centres is not None and centres[0] < centres[1]:          # narrower bounds are the same as cutting the sequence there
        lo, hi = bounds
        cut = cloud.views_numpy(depth[lo:hi], poses[lo:hi], inv_K, K, 2, 0.03, centres=(centres[0] - lo, centres[1] - lo), **V.RANGE)
        assert np.array_equal(got, cut)


@pytest.fixture(scope="module")
def plane():
    depth, poses, inv_K, K = V.plane_scene()
    votes = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.01, **V.RANGE)
    votes.setflags(write=False)
    return depth, poses, inv_K, K, votes


def test_a_plane_is_confirmed_by_every_neighbour(plane):
    depth, poses, inv_K, K, votes = plane
    assert depth.dtype == np.float32 and depth.shape == (11, 24, 40) and 5.0 < depth.min() and depth.max() < 20.0
    assert votes.shape == (11, 24, 40) and (votes[:, 4:-4, 6:-6] == 4).all()


def test_a_corrupted_patch_loses_its_votes_and_touches_only_the_frames_that_see_it(plane):
    depth, poses, inv_K, K, votes = plane
    bad = depth.copy()
    bad[5, 8:14, 10:20] *= np.float32(1.3)
    got = cloud.views_numpy(bad, poses, inv_K, K, 2, 0.01, **V.RANGE)
    assert (votes[5, 8:14, 10:20] == 4).all() and (got[5, 8:14, 10:20] == 0).all()
    for f in range(11):
        same = np.array_equal(got[f], votes[f])
        assert same == (f not in (3, 4, 5, 6, 7)), f          # the shifted windows of frames 0-2 and 8-10 do not contain frame 5


def test_votes_do_not_depend_on_the_unit(plane):
    depth, poses, inv_K, K, votes = plane
    twice = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.01, depth_scale=2.0, pose_scale=2.0, min_depth=1.0, max_range=80.0)
    assert np.array_equal(twice, votes)


# ---- 2. the fusion ---------------------------------------------------------------------------------------------------------------

def test_fuse_numpy_with_min_views_is_the_masking_by_hand():
    depth, color, poses, inv_K, K = V.scene(4, 6, 9, 14)
    params = dict(U.PARAMS, edge=0.3, border=1)
    plain = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, **params)
    debug = {}
    got = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, min_views=2, view_radius=2, view_tol=0.03, K=K, debug=debug, **params)
    key, payload, counts = cloud.keys_numpy(depth, color, poses, inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    votes = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.03, params["depth_scale"], params["pose_scale"], params["min_depth"],
                              params["max_range"]).reshape(-1)
    drop = (key != cloud.INVALID_KEY) & (votes < 2)
    assert 0 < drop.sum() < (key != cloud.INVALID_KEY).sum()
    key[drop], payload[drop] = cloud.INVALID_KEY, 0
    keys, sums = cloud.voxel_table_numpy(key, payload)
    xyz, rgb, count, keep = cloud.finish_numpy(keys, sums, U.VOXEL)
    assert np.array_equal(got.keys, keys[keep]) and np.array_equal(got.xyz.view(np.uint32), xyz[keep].view(np.uint32))
    assert np.array_equal(got.rgb, rgb[keep]) and np.array_equal(got.count, count[keep])
    assert got.stats["invalid_views"] == int(drop.sum()) and got.stats["valid"] == int(counts[0]) - int(drop.sum())
    assert sum(got.stats[name] for name in cloud.CAUSES) + got.stats["invalid_views"] == got.stats["points"] == depth.size
    assert {k: v for k, v in got.stats.items() if k in plain.stats and k not in ("valid", "voxels", "voxels_dropped")} == \
        {k: v for k, v in plain.stats.items() if k not in ("valid", "voxels", "voxels_dropped")}
    tested = cloud.keys_numpy(depth, color, poses, inv_K, inv_voxel=1.0 / U.VOXEL, **params)[0] != cloud.INVALID_KEY
    assert np.array_equal(debug["votes"].reshape(-1), np.where(tested, votes, 0))
    # K defaults to the inverse of inv_K's block
    again = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, min_views=2, view_radius=2, view_tol=0.03, K=np.linalg.inv(inv_K), **params)
    U.assert_clouds_equal(again, cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, min_views=2, view_radius=2, view_tol=0.03, **params))
    # off: today's cloud and today's stats keys
    off = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, min_views=0, view_radius=1, view_tol=0.5, **params)
    U.assert_clouds_equal(off, plain)
    assert list(off.stats) == ["points"] + list(cloud.CAUSES) + ["voxels", "voxels_dropped"]


# An untrained network's depth maps are nearly flat and its poses nearly the identity: at 1 % about half of the pixels find three
# neighbours that agree, so the filter both keeps and drops
FUSER = dict(voxel=0.5, stride=2, border=1, min_depth=0.1, max_range=50.0, edge=0.5, min_views=3, view_radius=2, view_tol=0.01)


def _tree(tmp_path, n_frames=6):
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, n_frames, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, n_frames), 64, 96, [0, 1], is_train=False, img_ext=".png")
    return gt, ds


def test_scene_fuser_on_the_host_with_min_views(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    inv_K, K = cloud.dataset_inv_K(ds), cloud.dataset_K(ds)
    assert K.shape == (3, 3) and K.dtype == np.float64 and np.array_equal(K, np.asarray(ds[0]["K"], np.float64)[:3, :3])
    params = {k: v for k, v in FUSER.items() if k != "voxel"}
    clouds, debug = [], {}
    for batch_size in (1, 4, 6):
        clouds.append(cloud.SceneFuser(model, 64, 96, "cpu", batch_size=batch_size, **FUSER).fuse(ds, debug=debug))
        if batch_size > 1:
            U.assert_clouds_equal(clouds[0], clouds[-1])
    got = clouds[-1]
    depth, poses = debug["depth"].numpy(), debug["poses"]
    assert depth.shape == (6, 64, 96) and debug["votes"].shape == (6, 64, 96) and debug["votes"].dtype == torch.uint8
    U.assert_clouds_equal(got, cloud.fuse_numpy(depth, frames, poses, inv_K, FUSER["voxel"], K=K, **params))
    assert got.stats["points"] == 6 * 64 * 96 and got.stats["valid"] > 0 and got.stats["invalid_views"] > 0
    assert sum(got.stats[name] for name in cloud.CAUSES) + got.stats["invalid_views"] == got.stats["points"]
    # given poses (the ground truth) and a window of frames: the neighbour bounds are the fused range
    # (the camera moves a unit per frame: depths of ~30 units change by 3.6 % per frame, the next frames agree at 5 %, the others not)
    over = dict(min_views=1, view_tol=0.05, depth_scale=150.0)
    fuser = cloud.SceneFuser(model, 64, 96, "cpu", batch_size=4, **dict(FUSER, **over))
    sub = fuser.fuse(ds, poses=gt, frames=(1, 6), debug=debug)
    assert np.array_equal(debug["poses"], gt) and debug["depth"].shape[0] == 5 and debug["votes"].shape[0] == 5
    assert sub.stats["valid"] > 0 and sub.stats["invalid_views"] > 0 and int(debug["votes"].max()) > 0
    U.assert_clouds_equal(sub, cloud.fuse_numpy(debug["depth"].numpy(), frames[1:6], gt[1:6], inv_K, FUSER["voxel"], K=K,
                                                **dict(params, **over)))
    with pytest.raises(ValueError):
        fuser.fuse(ds, frames=(1, 5))          # four frames: radius 2 needs five


# ---- 3. errors -------------------------------------------------------------------------------------------------------------------

def test_argument_errors():
    depth, color, poses, inv_K, K = V.scene(0, 5, 4, 6)
    ok = dict(radius=2, tol=0.05)
    cloud.views_numpy(depth, poses, inv_K, K, **ok)
    for bad in (dict(radius=0), dict(radius=9), dict(radius=3), dict(tol=-0.1), dict(tol=float("nan")), dict(bounds=(0, 4)),
                dict(bounds=(1, 6)), dict(centres=(0, 6)), dict(centres=(0, 2), bounds=(1, 5), radius=1), dict(centres=(3, 2))):
        with pytest.raises(ValueError):
            cloud.views_numpy(depth, poses, inv_K, K, **dict(ok, **bad))
    for d in (depth[:, :1], depth[:, :, :1]):
        with pytest.raises(ValueError):
            cloud.views_numpy(d, poses, inv_K, K, **ok)
    with pytest.raises(ValueError):
        cloud.views_numpy(depth, poses[:4], inv_K, K, **ok)
    with pytest.raises(ValueError):
        cloud.views_numpy(depth, poses, inv_K, np.eye(2), **ok)
    model = build_model("cfg_kitti_fm", 64, 96)
    for bad in (dict(min_views=5, view_radius=2), dict(min_views=-1), dict(view_radius=0), dict(view_radius=9), dict(view_tol=-1.0),
                dict(view_tol=float("nan"))):
        with pytest.raises(ValueError):
            cloud.fuse_numpy(depth, color, poses, inv_K, 0.25, **bad)
        with pytest.raises(ValueError):
            cloud.SceneFuser(model, 64, 96, "cpu", **bad)
    with pytest.raises(ValueError):
        cloud.fuse_numpy(depth[:4], color[:4], poses[:4], inv_K, 0.25, min_views=1)          # four frames: radius 2 needs five


def test_views_hip_refuses_host_tensors():
    depth, color, poses, inv_K, K = V.scene(0, 5, 4, 6)
    with pytest.raises(native.NativeLibraryError):
        cloud.views_hip(torch.from_numpy(depth), torch.from_numpy(poses), inv_K, K, 2, 0.05)
    with pytest.raises(native.NativeLibraryError):
        cloud.fuse_hip(torch.from_numpy(depth), torch.from_numpy(color), torch.from_numpy(poses), inv_K, 0.25, min_views=1)


def test_td_cloud_views_rejects_bad_arguments_without_a_gpu():
    lib = native.load()
    assert lib.td_abi_version() == 3
    one = ctypes.c_void_p(64)          # a non-null pointer that is never dereferenced: the checks come first
    k = (ctypes.c_double * 9)(*([1.0] * 9))
    #      depth poses K inv_K N  H  W  c0 c1 lo hi radius min_views tol depth_scale pose_scale min_depth max_range key payload votes stats
    good = [one, one, k, k, 5, 8, 8, 0, 5, 0, 5, 2, 1, 0.05, 1.0, 1.0, 0.1, 10.0, one, one, one, one, None]
    for pos in (0, 1, 2, 3, 18, 19):          # key without payload and payload without key included
        args = list(good)
        args[pos] = None
        assert lib.td_cloud_views(*args) == -1, pos
    neither = list(good)
    neither[18] = neither[19] = neither[20] = None          # neither keys nor votes: nothing to write
    assert lib.td_cloud_views(*neither) == -1
    for pos, bad in ((4, -1), (5, 1), (6, 1), (11, 0), (11, 9), (11, 3), (12, -1), (12, 5), (13, -0.01), (13, float("nan")), (9, -1),
                     (10, 6), (10, 4), (7, -1), (8, 6), (9, 1), (7, 6)):
        args = list(good)
        args[pos] = bad
        assert lib.td_cloud_views(*args) == -1, (pos, bad)
    shifted = list(good)
    shifted[7], shifted[8] = 3, 2          # c1 < c0
    assert lib.td_cloud_views(*shifted) == -1
    # the no-ops: no frames, no centres; nothing is launched (there is no GPU here)
    empty = list(good)
    empty[4] = empty[8] = empty[10] = 0
    assert lib.td_cloud_views(*empty) == 0
    none = list(good)
    none[7] = none[8] = 2
    assert lib.td_cloud_views(*none) == 0
    assert set(native.SIGNATURES) >= {"td_cloud_views"} and len(native.SIGNATURES["td_cloud_views"][1]) == len(good)


# ---- 4. the script ---------------------------------------------------------------------------------------------------------------

def test_reconstruct_script_with_min_views(tmp_path):
    gt, ds = _tree(tmp_path)
    model = build_model("cfg_kitti_fm", 64, 96)
    ckpt = str(tmp_path / "model.pth")
    torch.save({"state_dict": model.state_dict()}, ckpt)
    out = str(tmp_path / "out" / "cloud.ply")
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "reconstruct.py"), "--config", os.path.join(ROOT, "config", "cfg_kitti_fm.py"),
           "--checkpoint", ckpt, "--data_path", str(tmp_path), "--sequence", "9", "--height", "64", "--width", "96", "--device", "cpu",
           "--voxel", "0.5", "--stride", "2", "--border", "1", "--max_range", "50", "--edge", "0.5", "--batch_size", "4",
           "--min_views", "3", "--view_radius", "2", "--view_tol", "0.01", "--out", out]
    run = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    back = cloud.load_ply(out)
    want = cloud.SceneFuser(model, 64, 96, "cpu", batch_size=4, **FUSER).fuse(ds)
    assert back.dtype == cloud.PLY_DTYPE and len(back) == len(want.keys) > 0 and want.stats["invalid_views"] > 0
    assert np.array_equal(np.stack([back["x"], back["y"], back["z"]], 1).view(np.uint32), want.xyz.view(np.uint32))
    assert np.array_equal(np.stack([back["red"], back["green"], back["blue"]], 1), want.rgb) and np.array_equal(back["count"], want.count)
    assert "invalid_views %d" % want.stats["invalid_views"] in run.stdout and "valid %d" % want.stats["valid"] in run.stdout
    tested = want.stats["valid"] + want.stats["invalid_views"]
    assert "consistency rate %.4f (%d of %d" % (want.stats["valid"] / max(tested, 1), want.stats["valid"], tested) in run.stdout


# ---- 5. the sliding window's schedule and the driver's loop ----------------------------------------------------------------------

def _clamped(i, first, last, radius):
    return min(max(i - radius, first), last - 1 - 2 * radius)


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("batch_size", [1, 2, 3, 5, 12])
@pytest.mark.parametrize("first", [0, 2])
def test_window_schedule_over_all_small_cases(first, batch_size, radius):
    for n in range(2 * radius + 1, 13):
        last = first + n
        predicted, centres, w0 = [], [], first
        for at, end, ready, keep in cloud.window_schedule(first, last, batch_size, radius):
            predicted += list(range(at, end))
            assert 0 < end - at <= batch_size and end - w0 <= batch_size + 2 * radius          # what is held while the batch is fused
            for c0, c1 in ready:
                assert 0 < c1 - c0 <= batch_size
                for i in range(c0, c1):          # the centre's clamped window lies inside the held frames w0 ... end-1
                    a = _clamped(i, first, last, radius)
                    assert w0 <= a and a + 2 * radius < end, (n, i, w0, end)
                centres += list(range(c0, c1))
            assert w0 <= keep <= end and end - keep <= batch_size + 2 * radius          # what is held on to the next batch
            w0 = keep
        assert predicted == list(range(first, last)), n          # every frame once, in order
        assert centres == list(range(first, last)), n            # every centre once, ascending; none is left after the last batch


class _RecordingSink:
    def __init__(self, min_views, radius):
        self.min_views, self.radius, self.calls = min_views, radius, []

    def add(self, depth, color, poses, window=None):
        self.calls.append((depth, color, poses, window))


def _driver_inputs():
    """7 frames of 4 x 6 whose pixels are the frame's number; the predictor in the driver's place answers 1 + number / 8 everywhere."""
    color = torch.arange(7, dtype=torch.uint8).reshape(7, 1, 1, 1).expand(7, 3, 4, 6).contiguous()
    poses = torch.arange(7 * 12, dtype=torch.float64).reshape(7, 3, 4)
    predict = lambda c: 1.0 + c[:, 0].to(torch.float32) / 8.0
    return color, poses, predict


@pytest.mark.parametrize("first,last", [(0, 7), (2, 7)])
def test_driver_loop_without_the_filter_hands_on_the_batches(first, last):
    color, poses, predict = _driver_inputs()
    sink, depths = _RecordingSink(0, 1), []
    cloud.feed_frames(predict, sink, color, poses, first, last, 3, False, depths)
    starts = list(range(first, last, 3))
    assert len(sink.calls) == len(starts) == len(depths)
    for at, (d, c, p, window), kept in zip(starts, sink.calls, depths):
        end = min(at + 3, last)
        assert window is None and torch.equal(d, predict(color[at:end])) and d.shape == (end - at, 4, 6) and kept is d
        assert torch.equal(c, color[at:end]) and torch.equal(p, poses[at:end])


@pytest.mark.parametrize("first,last", [(0, 7), (2, 7)])
def test_driver_loop_with_the_filter_hands_on_centres_and_their_windows(first, last):
    color, poses, predict = _driver_inputs()
    radius, value = 1, lambda i: 1.0 + i / 8.0
    sink, depths = _RecordingSink(1, radius), []
    cloud.feed_frames(predict, sink, color, poses, first, last, 3, True, depths)
    assert torch.equal(torch.cat(depths), predict(color[first:last]))          # every frame predicted once, in order
    seen = []
    for d, c, p, (held, held_poses, (c0, c1), (lo, hi)) in sink.calls:
        frames = [int(round((float(v) - 1.0) * 8.0)) for v in held[:, 0, 0]]          # the frames the window holds, by their constants
        assert frames == list(range(frames[0], frames[0] + len(frames))) and (lo, hi) == (0, len(frames))
        assert torch.equal(held, torch.stack([torch.full((4, 6), value(i)) for i in frames]))
        assert torch.equal(held_poses, poses[frames[0]:frames[-1] + 1])
        centres = frames[c0:c1]
        assert 0 < len(centres) <= 3 and torch.equal(d, held[c0:c1])
        assert torch.equal(c, color[centres[0]:centres[-1] + 1]) and torch.equal(p, poses[centres[0]:centres[-1] + 1])
        for local, i in zip(range(c0, c1), centres):          # the kernel's clamp inside the bounds picks the centre's true neighbours
            assert frames[_clamped(local, lo, hi, radius)] == _clamped(i, first, last, radius)
        seen += centres
    assert seen == list(range(first, last))
