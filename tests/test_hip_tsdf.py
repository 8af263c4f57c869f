"""csrc/td_tsdf.hip on the device (through tripled_amd.tsdf) against the numpy statements, which tests/test_tsdf_cpu.py pins to literal
brute forces.  Every comparison is exact (np.array_equal on keys, payloads, sums, the bits of xyz and normal, rgb, weight and stats):
every quantity is an integer or a fixed sequence of individually rounded float64 operations.

Shapes: the smallest at which each kernel can go wrong.  Samples: td_cloud_keys' rows (13: shorter than a vector, width 1; 70: longer
than a wave, width 2; 257: longer than a workgroup's run, width 1; 264: the widest vector over several workgroups) and the same behind
an unaligned base pointer, crossed with the narrowest, the default and the widest band.  Surface: one voxel, one short of a wave, a
wave, one more, and more than a workgroup's 256 several times over (4 097)."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import cloud, native, tsdf
from tests import odom_util
from tests import tsdf_util as U
from tests.infer_util import build_model, randomize_batchnorm

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _h(t):
    return t.cpu().numpy()


# ---- 1. samples --------------------------------------------------------------------------------------------------------------------

def _check_samples(depth, color, poses, inv_K, T, mask, params, depth_d=None, color_d=None):
    want_key, want_payload, want_counts = tsdf.samples_numpy(depth, color, poses, inv_K, T, U.VOXEL, mask, **params)
    stats = torch.zeros(len(tsdf.SAMPLE_STATS), dtype=torch.int64, device=_dev())
    key, payload = tsdf.samples_hip(_d(depth) if depth_d is None else depth_d, _d(color) if color_d is None else color_d, _d(poses), inv_K,
                                    T, U.VOXEL, None if mask is None else _d(mask), stats=stats, **params)
    assert key.dtype == torch.int64 and payload.dtype == torch.int64 and key.shape == ((4 * T + 1) * depth.size,)
    assert np.array_equal(_h(key), want_key)
    assert np.array_equal(_h(payload).view(np.uint64), want_payload)
    assert np.array_equal(_h(stats), want_counts)
    return want_counts


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("edge", [0.0, 0.15])
@pytest.mark.parametrize("stride,border", [(1, 0), (1, 2), (3, 0), (3, 2)])
@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("H,W", [(7, 13), (9, 70), (5, 257), (6, 264)])
def test_samples_are_the_numpy_statement(H, W, T, stride, border, edge, masked):
    depth, color, poses, inv_K = U.scene(H * W + stride + T, 3, H, W)
    mask = U.pixel_mask(H * W + T, depth.shape) if masked else None
    counts = _check_samples(depth, color, poses, inv_K, T, mask, dict(U.PARAMS, stride=stride, border=border, edge=edge))
    if stride == 1 and border == 0:          # the inputs do exercise the rules
        assert counts[0] > 0 and counts[3] > 0 and (counts[4] > 0) == (edge > 0) and (counts[5] > 0) == masked
        assert counts[6] > 0 and counts[7] > 0 and counts[8] > 0 and counts[9] > 0


def test_samples_behind_an_unaligned_base_pointer():
    """A slice one element into a buffer: no vector width fits the base pointers, so the scalar path runs on a row length (264) that
    otherwise takes the widest one.  Scales other than 1 and a bool mask ride along."""
    B, H, W = 3, 6, 264
    depth, color, poses, inv_K = U.scene(11, B, H, W)
    dbuf = torch.zeros(B * H * W + 1, dtype=torch.float32, device=_dev())
    cbuf = torch.zeros(B * 3 * H * W + 1, dtype=torch.uint8, device=_dev())
    dbuf[1:].copy_(_d(depth).reshape(-1))
    cbuf[1:].copy_(_d(color).reshape(-1))
    depth_d, color_d = dbuf[1:].view(B, H, W), cbuf[1:].view(B, 3, H, W)
    assert depth_d.data_ptr() % 8 == 4 and color_d.data_ptr() % 2 == 1 and depth_d.is_contiguous()
    mask = U.pixel_mask(3, depth.shape).astype(bool)
    _check_samples(depth, color, poses, inv_K, 3, mask, dict(U.PARAMS, edge=0.2, border=1, depth_scale=1.3, pose_scale=0.7), depth_d, color_d)


def test_samples_of_no_frames():
    key, payload = tsdf.samples_hip(torch.zeros(0, 4, 6, device=_dev()), torch.zeros(0, 3, 4, 6, dtype=torch.uint8, device=_dev()),
                                    torch.zeros(0, 3, 4, dtype=torch.float64, device=_dev()), np.eye(3), 3, 0.5)
    assert key.shape == (0,) and payload.shape == (0,)


# ---- 2. surface --------------------------------------------------------------------------------------------------------------------

def _dense(V, seed):
    keys, sums = U.slab(17, 17, 15, seed) if V > 1000 else U.slab(3, 4, 6, seed)
    return keys[:V], sums[:V]


MAPS = {"slab": _dense, "sparse": lambda V, seed: U.sparse_map(V, seed), "field_ends": lambda V, seed: U.field_ends_map(V, seed)}


def _check_surface(keys, sums, voxel, min_weight):
    want = tsdf.surface_numpy(keys, sums, voxel, min_weight)
    stats = torch.zeros(len(tsdf.SURFACE_STATS), dtype=torch.int64, device=_dev())
    got = tsdf.surface_hip(_d(keys), _d(sums), voxel, min_weight, stats=stats)
    assert got[0].shape == (len(keys), 3, 3) and got[4].dtype == torch.bool
    U.assert_slots_equal(got, want)
    assert np.array_equal(_h(stats), want[5])
    return want


@pytest.mark.parametrize("V", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("kind", sorted(MAPS))
def test_surface_is_the_numpy_statement(kind, V):
    keys, sums = MAPS[kind](V, V)
    assert len(keys) == V
    for min_weight in (1, 3):
        want = _check_surface(keys, sums, 0.25, min_weight)
        if V >= 63 and min_weight == 1:
            assert want[4].any()
    if kind == "sparse":          # nothing above min_weight: every voxel is counted, nothing crosses
        want = _check_surface(keys, sums, 0.25, 100)
        assert not want[4].any() and list(want[5]) == [V, 0, 0, 0, 0]


def test_surface_of_an_empty_map():
    out = tsdf.surface_hip(torch.zeros(0, dtype=torch.int64, device=_dev()), torch.zeros(0, 7, dtype=torch.int64, device=_dev()), 0.5, 1)
    assert out[0].shape == (0, 3, 3) and out[4].shape == (0, 3)


# ---- 3. fusion ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("views", [0, 1])
def test_fusion_does_not_depend_on_batches_or_chunks(views):
    depth, color, poses, inv_K = U.scene(7, 4, 24, 48, far=False)
    if views:                                # frames that do see one another: small rotations and steps
        poses = poses.copy()
        poses[:, :, :3] = np.eye(3)
        poses[:, :, 3] = np.arange(4)[:, None] * np.array([0.05, 0.0, 0.1])
    params = dict(U.PARAMS, edge=0.3, border=1, min_views=views, view_radius=1, view_tol=0.2)
    want = tsdf.fuse_tsdf_numpy(depth, color, poses, inv_K, 0.5, 3, 2, **params)
    assert len(want.xyz) > 50 and want.stats["crossings_z"] > 0 and (want.stats["invalid_mask"] > 0) == bool(views)
    dev = [_d(depth), _d(color), _d(poses)]
    whole = tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=4, **params)
    assert whole.xyz.is_cuda and whole.xyz.dtype == torch.float32 and whole.normal.dtype == torch.float32
    assert whole.rgb.dtype == torch.uint8 and whole.weight.dtype == torch.int32
    others = [tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=4, **params),                    # the same input twice
              tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=2, **params),
              tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=1, **params),
              tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=4, pair_chunk=7001, **params),     # the pairs cut mid-slot
              tsdf.fuse_tsdf_hip(*dev, inv_K, 0.5, 3, 2, batch_size=3, pair_chunk=20000, **params)]
    for other in others + [want]:
        U.assert_surfaces_equal(whole, other)


FUSER = dict(voxel=0.02, batch_size=4, stride=1, border=2, min_depth=0.1, max_range=50.0, edge=0.5)


def test_tsdf_fuser_end_to_end(tmp_path):
    """The device surface against fuse_tsdf_numpy on the fuser's OWN depth maps and poses, read back: exact."""
    from mono.datasets import KITTIOdomDataset, odom_sequence_files
    gt = odom_util.make_sequence_tree(str(tmp_path), 9, 6, h=64, w=96)
    ds = KITTIOdomDataset(str(tmp_path), odom_sequence_files(9, 6), 64, 96, [0, 1], is_train=False, img_ext=".png")
    model = randomize_batchnorm(build_model("cfg_kitti_fm", 64, 96, seed=3))
    fuser = tsdf.TsdfFuser(model, 64, 96, _dev(), **FUSER)
    debug = {}
    got = fuser.fuse(ds, debug=debug)
    assert not next(model.parameters()).is_cuda
    depth, poses = debug["depth"], debug["poses"]
    assert depth.is_cuda and depth.shape == (6, 64, 96) and poses.is_cuda and poses.shape == (6, 3, 4)
    frames = cloud.odometry.dataset_frames_u8(ds).numpy()
    inv_K = cloud.dataset_inv_K(ds)
    params = {k: v for k, v in FUSER.items() if k not in ("voxel", "batch_size")}
    want = tsdf.fuse_tsdf_numpy(_h(depth), frames, _h(poses), inv_K, FUSER["voxel"], **params)
    assert got.xyz.is_cuda and got.stats["points"] == 6 * 64 * 96 and got.stats["samples"] > 0
    U.assert_surfaces_equal(got, want)
    # ground-truth poses, a window of frames, the multi-view filter through the mask, a small chunk
    fuser = tsdf.TsdfFuser(model, 64, 96, _dev(), trunc_voxels=2, min_weight=1, depth_scale=1.5, min_views=1, view_radius=1, view_tol=0.3,
                           pair_chunk=50000, **FUSER)
    sub = fuser.fuse(ds, poses=gt, frames=(1, 6), debug=debug)
    assert np.array_equal(_h(debug["poses"]), gt) and debug["depth"].shape == (5, 64, 96)
    U.assert_surfaces_equal(sub, tsdf.fuse_tsdf_numpy(_h(debug["depth"]), frames[1:6], gt[1:6], inv_K, FUSER["voxel"], 2, 1, depth_scale=1.5,
                                                      min_views=1, view_radius=1, view_tol=0.3, K=cloud.dataset_K(ds), **params))


# ---- 4. the device-only contract ---------------------------------------------------------------------------------------------------

def test_host_tensors_are_refused():
    depth, color, poses, inv_K = U.scene(0, 2, 4, 6)
    with pytest.raises(native.NativeLibraryError):
        tsdf.samples_hip(_d(depth), torch.from_numpy(color), _d(poses), inv_K, 3, 0.5)
    with pytest.raises(native.NativeLibraryError):
        tsdf.samples_hip(_d(depth), _d(color), _d(poses), inv_K, 3, 0.5, mask=torch.ones(2, 4, 6, dtype=torch.uint8))
    with pytest.raises(native.NativeLibraryError):
        tsdf.surface_hip(torch.zeros(4, dtype=torch.int64), torch.zeros(4, 7, dtype=torch.int64, device=_dev()), 0.5)
    with pytest.raises(native.NativeLibraryError):
        tsdf.fuse_tsdf_hip(torch.from_numpy(depth), _d(color), _d(poses), inv_K, 0.5)
    with pytest.raises(ValueError):
        tsdf.samples_hip(_d(depth), _d(color), _d(poses), inv_K, 9, 0.5)
