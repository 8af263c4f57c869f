"""Shared pieces of the TSDF ray-cast tests (test_tsdf_cast_cpu.py, test_hip_tsdf_cast.py): maps, cameras that look at them, and the
exact comparison of two Casts.  The maps are tsdf_util's; every case is small enough for the per-pixel, per-sample brute force."""
import functools

import numpy as np

import tripled_amd  # noqa: F401
from tripled_amd import cloud, tsdf

from tests import cloud_util
from tests import tsdf_util as U
from tests.tsdf_util import field_ends_map, hand_map, plane, slab, sparse_map, table_of_rows  # noqa: F401

VOXEL = U.VOXEL
HALF = cloud.HALF
# in the maps' units (VOXEL = 2.0): 40 samples one voxel apart would skip a 1-voxel band, half a voxel is the caster's default
CAST = dict(near=1.0, far=40.0, step_voxels=0.5, min_weight=1)

FORWARD = np.eye(3)                          # the camera looks along +z of the world
BACKWARD = np.diag([1.0, -1.0, -1.0])        # along -z (x kept, y and z turned: a rotation)


def inv_K(H, W):
    return cloud_util.intrinsics(H, W)[1]


def pose(eye_voxels, R=FORWARD, voxel=VOXEL):
    """Camera-to-world [3,4]: rotation R, the eye at ``eye_voxels`` (in voxels)."""
    out = np.zeros((3, 4))
    out[:, :3] = R
    out[:, 3] = np.asarray(eye_voxels, np.float64) * voxel
    return out


def tilt(ax, ay):
    """A small rotation about x, then y."""
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])


def cameras_in_front(keys, C, seed=0, back=6.0):
    """C poses [C,3,4] in front of the map's bounding box (on its -z side, ``back`` voxels away), looking along +z with a seeded
    tilt and offset."""
    g = np.random.default_rng(seed)
    cells = np.stack(cloud.unpack_key(keys), -1).astype(np.float64) if len(keys) else np.zeros((1, 3))
    lo, hi = cells.min(0), cells.max(0) + 1.0
    out = []
    for _ in range(C):
        eye = [0.5 * (lo[0] + hi[0]) + g.uniform(-0.7, 0.7), 0.5 * (lo[1] + hi[1]) + g.uniform(-0.7, 0.7), lo[2] - back + g.uniform(-0.5, 0.5)]
        out.append(pose(eye, tilt(*g.uniform(-0.08, 0.08, 2))))
    return np.stack(out)


def field_end_cameras():
    """Three cameras at +-2^20 voxels for field_ends_map: rays that walk up to and past the last coordinate of the z field at the low
    end of x and y (where the key after a column's last voxel IS the next column's first), down to the first coordinate at the high
    end of x and the low end of y, and into the corner whose corner set contains the sentinel voxel."""
    return np.stack([pose([-HALF + 1.0, -HALF + 1.1, HALF - 6.0]),
                     pose([HALF - 1.2, -HALF + 0.9, -HALF + 6.0], BACKWARD),
                     pose([HALF - 1.0, HALF - 1.0, HALF - 6.5], tilt(0.01, -0.02))])


def straddling_map():
    """A dense slab that lies across coordinate 0 on all three axes (x -4 ... 3, y -3 ... 3, z -4 ... 3), where the biased key fields
    pass 2^20 and an 8-aligned boundary of the coordinates: the surface, in the slab's middle, is at z = 0."""
    return slab(8, 7, 8, seed=3, origin=(-4, -3, -4))


def holed_slab(share=0.06, seed=1):
    """slab(7, 6, 8) with a seeded ``share`` of its voxels taken out: corner sets come and go along a ray."""
    keys, sums = slab(7, 6, 8, seed=seed)
    keep = np.random.default_rng(seed).random(len(keys)) >= share
    return keys[keep], sums[keep]


@functools.lru_cache(maxsize=None)
def fused_map(seed=5, B=3, H=8, W=12):
    """A map fused by fuse_tsdf_numpy from tsdf_util.scene (NaN, inf and out-of-range frames) -> (keys, sums, poses, inv_K)."""
    depth, color, poses, ik = U.scene(seed, B, H, W)
    debug = {}
    tsdf.fuse_tsdf_numpy(depth, color, poses, ik, U.VOXEL, 3, 1, debug=debug, **dict(U.PARAMS))
    return debug["keys"], debug["sums"], poses, ik


def bits(a):
    a = U.host(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_casts_equal(got, want):
    """Two Casts are the same bits: depth and normal as uint32, colour, weight and stats as integers."""
    for name, a, b in zip(tsdf.Cast._fields, got, want):
        a, b = bits(a), bits(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (name, int((a != b).sum()))


def assert_stats_consistent(cast, H, W):
    s = U.host(cast.stats)
    assert np.array_equal(s[:, 0], np.full(len(s), H * W)) and np.array_equal(s[:, 0], s[:, 1] + s[:, 2] + s[:, 3])
    depth, weight = U.host(cast.depth), U.host(cast.weight)
    assert np.array_equal((depth > 0).reshape(len(s), -1).sum(1), s[:, 1]) and np.array_equal((weight > 0), (depth > 0))
    none = (U.host(cast.normal) == 0).all(1) & (depth > 0)
    assert np.array_equal(none.reshape(len(s), -1).sum(1), s[:, 4])
