"""csrc/td_tsdf_cast.hip on the device (through tripled_amd.tsdf.raycast_hip) against the numpy statement raycast_numpy, which
tests/test_tsdf_cast_cpu.py pins to a literal brute force.  Every comparison is exact: depth and normal as uint32 bits, colour, weight
and stats as integers.

Shapes: a wave owns 8 x 8 pixels and a block 32 x 8, so W = 1, 63, 64, 65 and 130 (one column; one short of two blocks, two blocks, one
more, four full blocks and two columns) with H = 1 and 3 (tiles mostly outside the image) and one H = 9 (a second row of tiles); C = 1 and
3, and 5 views in batches of 2 through the caster.  The whole file takes seconds."""
import numpy as np
import pytest
import torch

import tripled_amd  # noqa: F401
from tripled_amd import native, tsdf
from tests import tsdf_cast_util as C
from tests import tsdf_util as U

pytestmark = pytest.mark.gpu

VOXEL = C.VOXEL


def _dev():
    return torch.device("cuda", 0)


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _check(keys, sums, poses, H, W, voxel=VOXEL, ik=None, **over):
    """The device against the statement -> the statement's Cast."""
    args = dict(C.CAST, **over)
    ik = C.inv_K(H, W) if ik is None else ik
    want = tsdf.raycast_numpy(keys, sums, poses, ik, H, W, voxel, **args)
    C.assert_casts_equal(tsdf.raycast_hip(_d(keys), _d(sums).reshape(-1, 7), _d(poses), ik, H, W, voxel, **args), want)
    return want


# ---- 1. the device against the statement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,n_cameras", [(1, 1, 1), (3, 63, 3), (1, 64, 3), (3, 65, 1), (3, 130, 3), (9, 33, 1)])
def test_slab_equals_the_statement(H, W, n_cameras):
    keys, sums = C.slab(6, 5, 8)
    want = _check(keys, sums, C.cameras_in_front(keys, n_cameras, seed=W), H, W)
    assert want.stats[:, 0].sum() == n_cameras * H * W and (W == 1 or want.stats[:, 1].sum() > 0)


@pytest.mark.parametrize("V,H,W,n_cameras", [(0, 3, 65, 3), (1, 1, 64, 1), (60, 3, 63, 1), (400, 3, 130, 3)])
def test_sparse_maps_equal_the_statement(V, H, W, n_cameras):
    keys, sums = C.sparse_map(V, seed=V) if V else (np.zeros(0, np.int64), np.zeros((0, 7), np.int64))
    _check(keys, sums, C.cameras_in_front(keys, n_cameras, seed=V, back=3.0), H, W, far=30.0)


def test_holes_fused_scene_and_a_nan_pose_equal_the_statement():
    keys, sums = C.holed_slab()
    poses = C.cameras_in_front(C.slab(7, 6, 8, seed=1)[0], 3, seed=2)
    want = _check(keys, sums, poses, 3, 65)
    assert want.stats[:, 1].sum() > 0 and want.stats[:, 3].sum() > 0
    poses[1, 0, 1] = np.nan
    assert _check(keys, sums, poses, 3, 63).stats[1, 3] == 3 * 63
    keys, sums, poses, ik = C.fused_map()
    want = _check(keys, sums, poses, 8, 12, ik=ik, far=20.0)
    assert want.stats[0, 1] > 0 and want.stats[2, 3] == 96
    # min_weight disqualifies voxels of one sample, a background is carried, pose_scale moves the cameras
    want = _check(keys, sums, poses, 8, 12, ik=ik, far=20.0, min_weight=2, background=(9, 80, 255), pose_scale=0.9)
    assert (want.color[:, 2][want.depth == 0] == 255).all()


# ---- 2. maps at the edges of the key fields -----------------------------------------------------------------------------------------------

def test_straddling_and_field_end_maps_equal_the_statement():
    keys, sums = C.straddling_map()                  # voxels on both sides of coordinate 0 on every axis, the surface at z = 0
    assert _check(keys, sums, C.cameras_in_front(keys, 3, seed=4), 9, 33).stats[:, 1].sum() > 0
    keys, sums = C.field_ends_map(63)
    assert _check(keys, sums, C.field_end_cameras(), 3, 65, far=24.0).stats[:, 0].sum() == 3 * 3 * 65


# ---- 3. the launch ----------------------------------------------------------------------------------------------------------------------

def _fenced(shape, dtype, marker):
    """A tensor of ``shape`` inside a larger buffer filled with ``marker`` -> (view, buffer, guard elements on either side)."""
    n, guard = int(np.prod(shape)), 256
    buf = torch.full((n + 2 * guard,), marker, dtype=dtype, device=_dev())
    return buf[guard:guard + n].view(shape), buf, guard


def test_two_runs_fences_and_zeroed_stats():
    keys, sums = C.slab(6, 5, 8)
    H, W, n = 3, 65, 3
    poses = C.cameras_in_front(keys, n, seed=7)
    want = tsdf.raycast_numpy(keys, sums, poses, C.inv_K(H, W), H, W, VOXEL, **C.CAST)
    shapes = (((n, H, W), torch.float32, -24576.0), ((n, 3, H, W), torch.float32, -24576.0), ((n, 3, H, W), torch.uint8, 171),
              ((n, H, W), torch.int32, -7), ((n, 5), torch.int64, 123456789))
    fenced = [_fenced(*s) for s in shapes]
    out = tsdf.Cast(*(f[0] for f in fenced))
    args = (_d(keys), _d(sums), _d(poses), C.inv_K(H, W), H, W, VOXEL)
    got = tsdf.raycast_hip(*args, out=out, **C.CAST)
    C.assert_casts_equal(got, want)                  # every element was written, the stats rows did not keep their 123456789
    for (view, buf, guard), (_, _, marker) in zip(fenced, shapes):
        edges = torch.cat([buf[:guard], buf[guard + view.numel():]])
        assert bool((edges == marker).all())
    first = [t.clone() for t in got]
    again = tsdf.raycast_hip(*args, out=out, **C.CAST)      # the same buffers: the stats are zeroed, not added to
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    fresh = tsdf.raycast_hip(*args, **C.CAST)
    C.assert_casts_equal(fresh, want)


def test_caster_on_the_device_is_the_caster_on_the_host():
    depth, color, poses, ik = U.scene(5, 3, 8, 12)
    debug = {}
    tsdf.fuse_tsdf_hip(_d(depth), _d(color), _d(poses), ik, U.VOXEL, 3, 1, batch_size=2, debug=debug, **dict(U.PARAMS))
    keys, sums = debug["keys"], debug["sums"]
    host_keys, host_sums, _, _ = C.fused_map()
    assert np.array_equal(keys.cpu().numpy(), host_keys) and np.array_equal(sums.cpu().numpy(), host_sums)
    views = np.concatenate([poses[:2], C.cameras_in_front(host_keys, 3, seed=1)])          # 5 views in batches of 2
    K = np.linalg.inv(C.inv_K(3, 65))
    params = dict(min_weight=1, near=1.0, far=20.0, step_voxels=0.5, pose_scale=1.0)
    want = tsdf.TsdfCaster("cpu", 3, 65, K, U.VOXEL, batch_size=12, **params).cast(host_keys, host_sums, views)
    got = tsdf.TsdfCaster("cuda:0", 3, 65, K, U.VOXEL, batch_size=2, **params).cast(keys, sums, views)
    C.assert_casts_equal(got, want)
    assert all(isinstance(a, np.ndarray) for a in got) and want.stats[:, 1].sum() > 0
    C.assert_casts_equal(tsdf.TsdfCaster("cuda:0", 3, 65, K, U.VOXEL, batch_size=3, **params).cast(host_keys, host_sums, views), want)


def test_host_tensors_and_bad_arguments_are_refused():
    keys, sums = C.slab(2, 2, 2)
    poses = C.cameras_in_front(keys, 1)
    ik = C.inv_K(4, 4)
    with pytest.raises(native.NativeLibraryError):
        tsdf.raycast_hip(torch.from_numpy(keys), _d(sums), _d(poses), ik, 4, 4, VOXEL)
    with pytest.raises(native.NativeLibraryError):
        tsdf.raycast_hip(_d(keys), _d(sums), torch.from_numpy(poses), ik, 4, 4, VOXEL)
    with pytest.raises(ValueError):
        tsdf.raycast_hip(_d(keys), _d(sums), _d(poses).float(), ik, 4, 4, VOXEL)
    with pytest.raises(ValueError, match="C >= 1"):                      # no view: the same clear refusal as on the host
        tsdf.raycast_hip(_d(keys), _d(sums), _d(poses)[:0], ik, 4, 4, VOXEL)
    with pytest.raises(ValueError, match="C >= 1"):
        tsdf.TsdfCaster("cuda:0", 4, 4, np.linalg.inv(ik), VOXEL).cast(keys, sums, poses[:0])
    with pytest.raises(ValueError):
        tsdf.raycast_hip(_d(keys), _d(sums), _d(poses), ik, 4, 4, VOXEL, near=1.0, far=1.0 + VOXEL * tsdf.CAST_MAX_STEPS)
    with pytest.raises(ValueError):
        tsdf.raycast_hip(_d(keys), _d(sums), _d(poses), ik, 4, 4, VOXEL, out=tsdf.Cast(*(torch.zeros(1, device=_dev()) for _ in range(5))))
