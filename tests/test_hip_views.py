"""csrc/td_views.hip on the device (through tripled_amd.cloud) against the numpy statement views_numpy, which tests/test_views_cpu.py
pins to a per-pixel count in plain Python and to an analytic scene.  Every comparison is exact (np.array_equal): a vote is a
comparison of a fixed sequence of individually rounded float64 operations.

Shapes: the smallest at which the kernel can go wrong.  A workgroup of 256 threads works on 256 consecutive pixels of one centre
frame: frames smaller than a wave (2 x 2, 5 x 7), a frame of one and a half workgroups whose rows are shorter than a wave (16 x 24),
a row that is no multiple of any vector width or of 64 (33 x 65), rows longer than a workgroup (3 x 300), and a frame of exactly 24
workgroups (64 x 96).  Offsets inside a frame are 32-bit by construction (a frame of more than 2^29 pixels is refused on the host)
and the frame bases are 64-bit, so no index beyond 2^31 (8.6 GB of depth) is run."""
import types

import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, dispatch, native
from tests import cloud_util as U
from tests import odom_util
from tests import views_util as V
from tests.infer_util import build_model, randomize_batchnorm

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


# ---- 1. the statement --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,H,W,radius,special,over", [
    (3, 2, 2, 1, True, {}),
    (3, 5, 7, 1, True, {}),
    (5, 16, 24, 2, True, {}),
    (5, 16, 24, 1, False, dict(depth_scale=1.7, pose_scale=0.6, min_depth=1.0, max_range=17.0)),
    (7, 33, 65, 3, True, {}),
    (7, 33, 65, 2, True, dict(depth_scale=0.5, pose_scale=0.5, min_depth=0.25, max_range=20.0)),
    (7, 3, 300, 2, True, {}),
    (4, 64, 96, 1, True, {}),
])
def test_votes_are_the_numpy_statement(N, H, W, radius, special, over):
    depth, _, poses, inv_K, K = V.scene(N * H + W, N, H, W, special=special)
    params = dict(V.RANGE, **over)
    want = cloud.views_numpy(depth, poses, inv_K, K, radius, 0.03, **params)
    got = cloud.views_hip(_d(depth), _d(poses), inv_K, K, radius, 0.03, **params)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, H, W)
    assert np.array_equal(_h(got), want)
    if H * W > 4:          # the inputs exercise the outcomes
        assert want.min() == 0 and want.max() == 2 * radius and len(np.unique(want)) > 2


def test_the_smallest_frame_has_votes():
    """2 x 2 under a camera that only moves forward: the pixel at the principal point projects onto the last row and column."""
    depth, _, poses, inv_K, K = V.scene(1, 3, 2, 2, special=False, angle=0.0, jitter=0.0)
    want = cloud.views_numpy(depth, poses, inv_K, K, 1, 0.03, **V.RANGE)
    assert want[:, 1, 1].max() >= 1 and want.max() == 2
    assert np.array_equal(_h(cloud.views_hip(_d(depth), _d(poses), inv_K, K, 1, 0.03, **V.RANGE)), want)


@pytest.mark.parametrize("centres,bounds", [((2, 5), None), ((1, 4), (1, 6)), ((3, 3), (0, 7)), (None, (2, 7)), ((6, 7), (2, 7)), ((0, 1), None)])
def test_centre_sub_ranges_and_narrower_bounds(centres, bounds):
    depth, _, poses, inv_K, K = V.scene(21, 7, 33, 65)
    want = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.03, centres=centres, bounds=bounds, **V.RANGE)
    got = cloud.views_hip(_d(depth), _d(poses), inv_K, K, 2, 0.03, centres=centres, bounds=bounds, **V.RANGE)
    assert tuple(got.shape) == want.shape and np.array_equal(_h(got), want)


def test_a_depth_tensor_that_is_a_slice_of_a_larger_one():
    depth, _, poses, inv_K, K = V.scene(5, 9, 16, 24)
    big_d, big_p = _d(depth), _d(poses)
    want = cloud.views_numpy(depth[2:8], poses[2:8], inv_K, K, 2, 0.03, **V.RANGE)
    got = cloud.views_hip(big_d[2:8], big_p[2:8], inv_K, K, 2, 0.03, **V.RANGE)
    assert big_d[2:8].data_ptr() != big_d.data_ptr() and np.array_equal(_h(got), want)


def test_the_plane_scene_on_the_device():
    depth, poses, inv_K, K = V.plane_scene()
    got = _h(cloud.views_hip(_d(depth), _d(poses), inv_K, K, 2, 0.01, **V.RANGE))
    assert np.array_equal(got, cloud.views_numpy(depth, poses, inv_K, K, 2, 0.01, **V.RANGE)) and (got[:, 4:-4, 6:-6] == 4).all()


# ---- 2. on the keys ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("centres", [(0, 6), (1, 4)])
@pytest.mark.parametrize("min_views", [0, 2, 4])
def test_key_masked_mode_is_the_numpy_masking(min_views, centres):
    N, H, W = 6, 33, 65
    depth, color, poses, inv_K, K = V.scene(9, N, H, W)
    c0, c1 = centres
    params = dict(U.PARAMS, edge=0.3, border=1)
    view = (params["depth_scale"], params["pose_scale"], params["min_depth"], params["max_range"])
    key, payload, _ = cloud.keys_numpy(depth[c0:c1], color[c0:c1], poses[c0:c1], inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    votes = cloud.views_numpy(depth, poses, inv_K, K, 2, 0.03, *view, centres=centres)
    want_key, want_payload, want_votes, want_counts = cloud.mask_views_numpy(key, payload, votes, min_views)
    assert (want_counts[1] > 0) == (min_views > 0) and want_counts[1] < want_counts[0] < key.size
    key_d, payload_d = cloud.keys_hip(_d(depth[c0:c1]), _d(color[c0:c1]), _d(poses[c0:c1]), inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    assert np.array_equal(_h(key_d), key)
    stats = torch.tensor([5, 7], dtype=torch.int64, device=_dev())          # incremented, not overwritten
    got = cloud.views_hip(_d(depth), _d(poses), inv_K, K, 2, 0.03, *view, centres=centres, key=key_d, payload=payload_d,
                          min_views=min_views, stats=stats)
    assert np.array_equal(_h(key_d), want_key) and np.array_equal(_h(payload_d).view(np.uint64), want_payload)
    assert np.array_equal(_h(got), want_votes) and np.array_equal(_h(stats), want_counts + [5, 7])
    # without the votes: the same keys
    key_d, payload_d = cloud.keys_hip(_d(depth[c0:c1]), _d(color[c0:c1]), _d(poses[c0:c1]), inv_K, inv_voxel=1.0 / U.VOXEL, **params)
    assert cloud.views_hip(_d(depth), _d(poses), inv_K, K, 2, 0.03, *view, centres=centres, key=key_d, payload=payload_d,
                           min_views=min_views, votes=False) is None
    assert np.array_equal(_h(key_d), want_key) and np.array_equal(_h(payload_d).view(np.uint64), want_payload)


# ---- 3. the fusion -----------------------------------------------------------------------------------------------------------------

def test_fuse_hip_with_min_views_is_fuse_numpy_whatever_the_batches():
    N, H, W = 7, 33, 65
    depth, color, poses, inv_K, K = V.scene(3, N, H, W)
    params = dict(U.PARAMS, edge=0.3, border=1, min_views=2, view_radius=2, view_tol=0.03, K=K)
    debug = {}
    want = cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, debug=debug, **params)
    assert 0 < want.stats["invalid_views"] and 0 < want.stats["valid"] and int(want.count.max()) > 1
    dev = (_d(depth), _d(color), _d(poses))
    dispatch.reset()
    whole = cloud.fuse_hip(*dev, inv_K, U.VOXEL, **params)
    assert dispatch.hip_calls["td_cloud_views"] == 1
    U.assert_clouds_equal(whole, want)
    U.assert_clouds_equal(whole, cloud.fuse_hip(*dev, inv_K, U.VOXEL, **params))          # two runs: the same bits
    for batch_size in (1, 2, 5):
        votes = {}
        U.assert_clouds_equal(cloud.fuse_hip(*dev, inv_K, U.VOXEL, batch_size=batch_size, debug=votes, **params), want)
        assert np.array_equal(_h(votes["votes"]), debug["votes"])


def test_fuse_hip_without_min_views_launches_no_views_kernel():
    depth, color, poses, inv_K, K = V.scene(3, 7, 33, 65)
    params = dict(U.PARAMS, edge=0.3, border=1)
    dev = (_d(depth), _d(color), _d(poses))
    dispatch.reset()
    plain = cloud.fuse_hip(*dev, inv_K, U.VOXEL, batch_size=2, **params)
    calls = dict(dispatch.hip_calls)
    dispatch.reset()
    off = cloud.fuse_hip(*dev, inv_K, U.VOXEL, batch_size=2, min_views=0, view_radius=1, view_tol=0.5, **params)
    assert dict(dispatch.hip_calls) == calls and "td_cloud_views" not in calls and calls["td_cloud_keys"] == 4
    U.assert_clouds_equal(off, plain)
    U.assert_clouds_equal(off, cloud.fuse_numpy(depth, color, poses, inv_K, U.VOXEL, **params))
    assert list(off.stats) == ["points"] + list(cloud.CAUSES) + ["voxels", "voxels_dropped"]


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------

# An untrained network's depth maps are nearly flat and its poses nearly the identity: at 1 % about a quarter of the pixels find three
# neighbours that agree, so the filter both keeps and drops
FUSER = dict(voxel=0.02, stride=1, border=2, min_depth=0.1, max_range=50.0, edge=0.5, min_views=3, view_radius=2, view_tol=0.01)


class _PixelwiseDepth:
    """In the place of a DepthPredictor: a depth of 0.18 ... 0.19 that is an element-wise function of the frame's own pixels, so that a
    frame gets the same bits whatever batch it arrives in."""

    def predict(self, images):
        x = images.to(torch.float32)
        return types.SimpleNamespace(depth=0.18 + (x[..., 0] + 2.0 * x[..., 1] + x[..., 2]) * (0.01 / 1020.0))


def test_scene_fuser_with_min_views_end_to_end(tmp_path):
    """The device cloud against fuse_numpy on the fuser's OWN depth maps and poses, read back: exact, as in test_hip_cloud.py, for
    batch sizes 4 and 1 (on six frames the centres become ready in a group, one at a time, and all at the end).

    Batch sizes 1, 2 and 4 agree: the fusion does not depend on the batch.  The NETWORK's output does: on an MI355X the depth maps
    of batch sizes 4 and 1 differ in their last bits (measured: not equal; the clouds then have the same voxels and statistics and
    differ in bits of xyz), and so do those of two fusers that both run the network one frame at a time (MIOpen does not promise
    the same convolution for every call).  So the agreement is asserted where the fusion gets the same depth maps and poses from
    every batch size: given poses, and _PixelwiseDepth in the place of the network."""
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, 6, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, 6), 64, 96, [0, 1], is_train=False, img_ext=".png")
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 64, 96, seed=3))
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    inv_K, K = cloud.dataset_inv_K(ds), cloud.dataset_K(ds)
    params = {k: v for k, v in FUSER.items() if k != "voxel"}
    clouds = []
    for batch_size in (4, 1):
        debug = {}
        got = cloud.SceneFuser(model, 64, 96, _dev(), batch_size=batch_size, **FUSER).fuse(ds, debug=debug)
        depth, poses, votes = debug["depth"], debug["poses"], debug["votes"]
        assert depth.is_cuda and depth.shape == (6, 64, 96) and votes.is_cuda and votes.shape == (6, 64, 96) and votes.dtype == torch.uint8
        host = {}
        want = cloud.fuse_numpy(_h(depth), frames, _h(poses), inv_K, FUSER["voxel"], K=K, debug=host, **params)
        U.assert_clouds_equal(got, want)
        assert np.array_equal(_h(votes), host["votes"])
        assert got.stats["points"] == 6 * 64 * 96 and got.stats["valid"] > 0 and got.stats["invalid_views"] > 0
        clouds.append(_h(depth))
    print("depth maps of batch sizes 4 and 1 equal: %s" % np.array_equal(clouds[0], clouds[1]))
    # ground-truth poses, a window of frames: the neighbour bounds are the fused range
    # (the camera moves a unit per frame: depths of ~28 units change by 3.6 % per frame, the next frames agree at 5 %, the others not)
    over = dict(min_views=1, view_tol=0.05, depth_scale=150.0)
    fuser = cloud.SceneFuser(model, 64, 96, _dev(), batch_size=2, **dict(FUSER, **over))
    debug = {}
    sub = fuser.fuse(ds, poses=gt, frames=(1, 6), debug=debug)
    assert debug["depth"].shape == (5, 64, 96) and debug["votes"].shape == (5, 64, 96)
    assert sub.stats["valid"] > 0 and sub.stats["invalid_views"] > 0
    U.assert_clouds_equal(sub, cloud.fuse_numpy(_h(debug["depth"]), frames[1:6], gt[1:6], inv_K, FUSER["voxel"], K=K, **dict(params, **over)))
    # the same depth maps for every batch size: batch sizes 2, 1 and 4 agree
    subs, maps = [], []
    for batch_size in (2, 1, 4):
        fuser = cloud.SceneFuser(model, 64, 96, _dev(), batch_size=batch_size, **dict(FUSER, **over))
        fuser.predictor = _PixelwiseDepth()
        debug = {}
        subs.append(fuser.fuse(ds, poses=gt, frames=(1, 6), debug=debug))
        maps.append(_h(debug["depth"]))
        assert np.array_equal(maps[-1], maps[0])
        U.assert_clouds_equal(subs[-1], subs[0])
    assert subs[0].stats["valid"] > 0 and subs[0].stats["invalid_views"] > 0 and int(debug["votes"].max()) == 4
    U.assert_clouds_equal(subs[0], cloud.fuse_numpy(maps[0], frames[1:6], gt[1:6], inv_K, FUSER["voxel"], K=K, **dict(params, **over)))


# ---- 5. the device-only contract ---------------------------------------------------------------------------------------------------

def test_host_tensors_and_bad_arguments_are_refused():
    depth, color, poses, inv_K, K = V.scene(0, 5, 4, 6)
    d, p = _d(depth), _d(poses)
    key = torch.zeros(5 * 4 * 6, dtype=torch.int64, device=_dev())
    with pytest.raises(native.NativeLibraryError):
        cloud.views_hip(d, torch.from_numpy(poses), inv_K, K, 2, 0.05)
    with pytest.raises(native.NativeLibraryError):
        cloud.views_hip(d, p, inv_K, K, 2, 0.05, key=key.cpu(), payload=key)
    with pytest.raises(native.NativeLibraryError):
        cloud.views_hip(d, p, inv_K, K, 2, 0.05, stats=torch.zeros(2, dtype=torch.int64))
    for bad in (dict(key=key), dict(key=key[:7], payload=key[:7]), dict(votes=False), dict(min_views=5), dict(bounds=(0, 4)),
                dict(key=torch.zeros(240, dtype=torch.int64, device=_dev())[::2], payload=key),          # changed in place: no copies
                dict(stats=torch.zeros(6, dtype=torch.int64, device=_dev()))):
        with pytest.raises(ValueError):
            cloud.views_hip(d, p, inv_K, K, 2, 0.05, **bad)
    with pytest.raises(ValueError):
        cloud.views_hip(d.double(), p, inv_K, K, 2, 0.05)
    assert tuple(cloud.views_hip(d, p, inv_K, K, 2, 0.05, centres=(2, 2)).shape) == (0, 4, 6)          # no centres: nothing is launched
