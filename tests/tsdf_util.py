"""Shared pieces of the TSDF tests (test_tsdf_cpu.py, test_hip_tsdf.py): scenes, hand-built voxel maps and the comparisons.

All comparisons are exact (np.array_equal on keys, payloads, sums, float bits and stats): every quantity is an integer or a fixed
sequence of individually rounded IEEE float64 operations (tsdf.py's docstring), and the brute forces take the same operations one
at a time in Python floats."""
import numpy as np

import tripled_amd  # noqa: F401
from tripled_amd import cloud, tsdf

from tests import cloud_util as U

VOXEL = U.VOXEL
PARAMS = dict(U.PARAMS)
ONE = 1 << 20


def scene(seed, B, H, W, **kw):
    """cloud_util.scene: NaN, +-inf, 0, negative, too-near and too-far depths, a step edge, rotated poses, negative coordinates and a
    last frame beyond +-2^20 voxels."""
    return U.scene(seed, B, H, W, **kw)


def pixel_mask(seed, shape, keep=0.8):
    return (np.random.default_rng(1000 + seed).random(shape) < keep).astype(np.uint8)


def plane(seed, B=8, H=24, W=48, z=6.1, noise=0.3):
    """A fronto-parallel plane at ``z`` seen by B cameras that look along +z from slightly different places, uniform depth noise."""
    g = np.random.default_rng(seed)
    depth = (z + g.uniform(-noise, noise, (B, H, W))).astype(np.float32)
    color = g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    poses = np.zeros((B, 3, 4))
    poses[:, :, :3] = np.eye(3)
    poses[:, :2, 3] = g.uniform(-0.2, 0.2, (B, 2))
    return depth, color, poses, U.intrinsics(H, W)[1]


def rows_of_table(table):
    """samples_bruteforce's dict -> (keys [V] ascending, sums [V,7] with the whole sum of v in the q_x column)."""
    cells = sorted(table)
    keys = cloud.pack_key(*np.array(cells, np.int64).reshape(-1, 3).T)
    sums = np.array([[table[c][0], table[c][1], 0, 0] + table[c][2:] for c in cells], np.int64).reshape(-1, 7)
    return keys, sums


def hand_map(cells):
    """{(ix, iy, iz): (w, S, r, g, b)} with S the summed signed distance -> (keys [V] ascending, sums [V,7]): sum v = S + 2^20 w, split
    over the three fields as the reduction leaves it (each field's sum below 1024 w)."""
    order = sorted(cells)
    keys = cloud.pack_key(*np.array(order, np.int64).reshape(-1, 3).T)
    sums = np.zeros((len(order), 7), np.int64)
    for j, c in enumerate(order):
        w, S = int(cells[c][0]), int(cells[c][1])
        total = S + ONE * w
        assert 0 <= total <= 2 * ONE * w
        z, rest = divmod(total, ONE)
        y, x = divmod(rest, 1024)
        sums[j] = [w, x, y, z] + [int(v) for v in cells[c][2:5]]
    return keys, sums


def table_of_rows(keys, sums):
    """(keys, sums) -> surface_bruteforce's dict."""
    S = tsdf.row_sdf_sum(sums)
    cells = np.stack(cloud.unpack_key(keys), -1)
    return {tuple(int(v) for v in c): (int(r[0]), int(s), int(r[4]), int(r[5]), int(r[6])) for c, r, s in zip(cells, np.asarray(sums), S)}


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def assert_slots_equal(got, want):
    """Two results of surface_numpy / surface_hip: the masks, and under the mask the bits."""
    hit = host(want[4]).astype(bool)
    assert np.array_equal(host(got[4]).astype(bool), hit)
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(host(a)[hit].view(np.uint32), host(b)[hit].view(np.uint32))
    for a, b in zip(got[2:4], want[2:4]):
        assert np.array_equal(host(a)[hit], host(b)[hit])


def assert_surface_is_bruteforce(keys, sums, voxel, min_weight):
    got = tsdf.surface_numpy(keys, sums, voxel, min_weight)
    want, counts = tsdf.surface_bruteforce(table_of_rows(keys, sums), voxel, min_weight)
    hit = got[4]
    assert list(got[5]) == counts, (got[5], counts)
    assert int(hit.sum()) == len(want)
    f32 = lambda rows: np.array(rows, np.float32).reshape(-1, 3).view(np.uint32)
    assert np.array_equal(got[0][hit].view(np.uint32), f32([p[0] for p in want]))
    assert np.array_equal(got[1][hit].view(np.uint32), f32([p[1] for p in want]))
    assert np.array_equal(got[2][hit], np.array([p[2] for p in want], np.uint8).reshape(-1, 3))
    assert np.array_equal(got[3][hit], np.array([p[3] for p in want], np.int32).reshape(-1))
    for a in got[:4]:
        assert not a[~hit].any()                     # a slot without a crossing is zero
    return got


def assert_surfaces_equal(a, b):
    """Two Surfaces (numpy arrays, or tensors brought to the host) are the same bits."""
    assert np.array_equal(host(a.xyz).view(np.uint32), host(b.xyz).view(np.uint32))
    assert np.array_equal(host(a.normal).view(np.uint32), host(b.normal).view(np.uint32))
    assert np.array_equal(host(a.rgb), host(b.rgb))
    assert np.array_equal(host(a.weight), host(b.weight))
    assert a.stats == b.stats, (a.stats, b.stats)


def slab(nx, ny, nz, seed=0, origin=(-3, -2, 4)):
    """A dense nx x ny x nz block of voxels whose distance falls from positive to negative along z, with seeded noise and weights."""
    g = np.random.default_rng(seed)
    cells = {}
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                w = int(g.integers(1, 9))
                d = (nz / 2.0 - z - 0.37 + 0.2 * np.sin(0.9 * x) + 0.15 * g.standard_normal()) / max(nz, 1)
                S = int(np.clip(np.rint(d * ONE), -ONE, ONE)) * w
                cells[(origin[0] + x, origin[1] + y, origin[2] + z)] = (w, S, *(int(v) * w for v in g.integers(0, 256, 3)))
    return hand_map(cells)


def sparse_map(V, seed=0):
    """V distinct voxels drawn from a box that they fill to about 30 %: neighbours exist or are missing by chance; signs, weights and
    colours are seeded."""
    g = np.random.default_rng(seed)
    extent = max(2, int(np.ceil((V / 0.3) ** (1.0 / 3.0) / 2.0)))
    cells = {}
    while len(cells) < V:
        c = tuple(int(v) for v in g.integers(-extent, extent, 3))
        w = int(g.integers(1, 6))
        cells[c] = (w, int(g.integers(-ONE, ONE + 1)) * w, *(int(v) * w for v in g.integers(0, 256, 3)))
    return hand_map(cells)


def field_ends_map(V, seed=0):
    """V voxels at both ends of every key field: coordinates from the first n and the last n of [-2^20, 2^20), n the smallest that holds
    V voxels (2 for V <= 63); never the sentinel voxel."""
    g = np.random.default_rng(seed)
    n = 2
    while (2 * n) ** 3 - 1 < V:
        n += 1
    ends = list(range(-cloud.HALF, -cloud.HALF + n)) + list(range(cloud.HALF - n, cloud.HALF))
    every = [(a, b, c) for a in ends for b in ends for c in ends if (a, b, c) != (cloud.HALF - 1,) * 3]
    cells = {}
    for j in g.permutation(len(every))[:V]:
        w = int(g.integers(1, 6))
        cells[every[j]] = (w, int(g.integers(-ONE, ONE + 1)) * w, *(int(v) * w for v in g.integers(0, 256, 3)))
    return hand_map(cells)
