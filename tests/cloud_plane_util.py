"""Seeded scenes and literal loops for the tests of tripled_amd.cloud_normals and of the point-to-plane half of tripled_amd.cloud_align:
a cloud with every kind of point planted, two exact-arithmetic corner cases of the neighbourhood, correspondences whose neighbours
partly have no normal, a per-row Python loop over the two-stage tree of the 37 sums, and street pairs whose two clouds sample the same
surfaces at DIFFERENT points (the case the plane criterion exists for)."""
import numpy as np

from tripled_amd import cloud, odometry
from tests import cloud_align_util as A
from tests import cloud_eval_util as E

NORMAL_SIZES = (1, 63, 64, 65, 257, 1000)
NORMAL_TAU = 0.5                      # a power of two: Q = 2^18 / radius is one too for radius = tau and tau / 2
FAR = 1.0e7                           # beyond the key range of every tau used here (2^20 cells of 0.5)


def poison_cloud(N, seed=0):
    """float64 [N,3]: a gently tilted, slightly noisy sheet at about 25 points per disc of radius 0.5, in shuffled order, with planted
    where N allows: a NaN row, a +inf and a -inf row, a row outside the key range, an isolated point, five collinear points, four
    duplicates (of one another), a blob of 30 points with no surface (N >= 257), 300 points inside one cell (a thin patch; N = 1000
    only).  Everything planted but the rows that are
    not finite lies far from the sheet and from each other."""
    rng = np.random.default_rng(seed + 7 * N)
    side = np.sqrt(max(N, 1) * np.pi * 0.25 / 25.0)
    p = np.zeros((N, 3))
    p[:, 0], p[:, 1] = rng.uniform(0, side, N) + 3.0, rng.uniform(0, side, N) - 2.0
    p[:, 2] = 0.2 * p[:, 0] - 0.1 * p[:, 1] + rng.normal(0, 0.002, N)
    at = 0

    def plant(rows):
        nonlocal at
        rows = np.atleast_2d(np.asarray(rows, np.float64))
        if at + len(rows) <= N - 40:                               # keep a sheet of at least 40 points
            p[at:at + len(rows)] = rows
            at += len(rows)

    plant([np.nan, 1.0, 2.0])
    plant([[0.5, np.inf, 0.0], [0.5, 0.0, -np.inf]])
    plant([FAR, 0.0, 0.0])
    plant([40.0, 40.0, 40.0])                                       # isolated: its own only neighbour
    plant(np.array([60.0, -60.0, 5.0]) + np.arange(5)[:, None] * np.array([0.03, 0.02, 0.01]))      # collinear
    plant(np.tile([-80.0, 10.0, 3.0], (4, 1)))                     # duplicates
    if N >= 257:
        plant(np.array([-30.0, -30.0, 7.0]) + rng.uniform(0, 0.3, (30, 3)))      # a blob: no surface, every patch is rough
    if N >= 1000:
        patch = np.array([100.2, 100.2, 100.2]) + np.concatenate([rng.uniform(0, 0.05, (300, 2)), rng.normal(0, 1e-4, (300, 1))], 1)
        plant(patch)                                                # one cell: floor(100.2 / 0.5) = floor(100.25 / 0.5)
    return p[rng.permutation(N)]


def lattice_sheet():
    """float64 [81,3]: a 9 x 9 lattice of step 0.25 in the plane z = 1, all coordinates exact.  With radius = 0.5 the neighbours two
    steps along an axis lie at EXACTLY the radius (d2 = 0.25 = radius^2, no rounding anywhere) and count: an interior point has 13."""
    g = np.arange(9) * 0.25
    x, y = np.meshgrid(g - 1.0, g + 2.0, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), np.ones(81)], 1)


def half_way_cloud(radius=0.5):
    """(cloud float64 [12,3], Q): around the point (1, 1, 1) eleven others whose offsets e have e_k Q exactly k + 1/2 in at least one
    component (Q = 2^18 / radius, a power of two, and the offsets are multiples of 1 / (2 Q) far below the points' own ulp budget): the
    quantisation must round them half to even."""
    Q = 2.0 ** 18 / radius
    rng = np.random.default_rng(11)
    halves = (rng.integers(-2000, 2000, (11, 3)) + 0.5) / Q
    halves[:, 2] = rng.integers(-3, 3, 11) / Q                     # a thin sheet: whole numbers across it
    cloud = np.concatenate([np.ones((1, 3)), 1.0 + halves])
    assert np.array_equal((cloud[1:] - 1.0) * Q, halves * Q)      # the offsets survive the addition exactly
    return cloud, Q


KEY_RANGE_TAU = 1.0
KEY_RANGE_STATS = [412, 3, 0, 0, 188]            # valid, few, degenerate, rough, invalid of key_range_scene at radius = tau, 3, 1.0


def key_range_scene():
    """(query float64 [603,3], ref float64 [6004,3]) for tau = 1: test_hip_cloud_eval.py's scene of cells at both ends of the key range
    (per axis a point sits near +2^20, near -2^20 or in the middle), denser, so that patches have neighbours.  The last cell on an
    axis starts at 2^20 - 2^-20, a neighbour cell beyond either end does not exist, a point beyond either is dropped from the grid
    and a query there is invalid.  ref ends in three points of the all-top corner cell, whose key is the sentinel (dropped), and one
    in the cell below it; query ends in two queries in the corner cell and one below it (valid: served from the cells around)."""
    edge = float(2 ** 20)
    rng = np.random.default_rng(9)

    def around(n):
        base = rng.uniform(-1.5, 1.5, (n, 3))
        side = rng.integers(0, 4, (n, 3))                              # per axis: the top edge, the bottom edge, or the middle
        return base + np.where(side == 0, edge, np.where(side == 1, -edge, 0.0)) + np.where(side == 1, -0.5, 0.0)

    ref = np.concatenate([around(6000), np.full((3, 3), edge + 0.25), [[edge + 0.25, edge + 0.25, edge - 0.5]]])
    query = np.concatenate([around(600), np.full((2, 3), edge + 0.3), [[edge + 0.3, edge + 0.3, edge - 0.3]]])
    return query, ref


def check_key_range_grid(grid, stats):
    """The grid of key_range_scene's ref reaches both ends of the key range, and the classes valid, few and invalid all occur."""
    ix = np.stack(cloud.unpack_key(np.asarray(grid.cell_key)), -1)
    assert ix.max() == cloud.HALF - 1 and ix.min() == -cloud.HALF
    assert grid.stats["dropped"] == 1965 and grid.stats["cells"] == 694
    assert np.asarray(stats).tolist() == KEY_RANGE_STATS and stats[0] > 0 and stats[1] > 0 and stats[4] > 0


# ---- plane moments -------------------------------------------------------------------------------------------------------------------

def plane_correspondences(N, M=97, seed=0, kind="mixed"):
    """cloud_align_util.correspondences plus normals [M,3]: unit vectors, every fifth row without one (all zero, one of them written
    with -0.0) unless kind is "matched".  -> (cur, ref, normals, index, d2, trim2, origin)."""
    cur, ref, index, d2, trim2, origin = A.correspondences(N, M, seed, kind)
    rng = np.random.default_rng(seed + 31 * N)
    normals = rng.normal(0, 1, (M, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    if kind != "matched":
        normals[::5] = 0.0
        normals[5] = [-0.0, 0.0, -0.0]
    return cur, ref, normals, index, d2, trim2, origin


def plane_moments_loop(cur, ref, normals, index, d2, trim2, origin):
    """cloud_align.plane_moments_numpy as a plain loop over the rows and over the tree, following the module's docstring literally."""
    N, M = len(cur), len(ref)
    matched = bad = flat = 0
    rows = []
    with np.errstate(invalid="ignore"):
        for i in range(N):
            v = np.zeros(37)
            j = int(index[i])
            if j >= M or j < -1:
                bad += 1
            elif j >= 0 and d2[i] <= trim2:
                n = [float(t) for t in normals[j]]
                if n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0:
                    flat += 1
                else:
                    matched += 1
                    p = [float(cur[i][k]) - float(origin[k]) for k in range(3)]
                    q = [float(ref[j][k]) - float(origin[k]) for k in range(3)]
                    g = [p[k] - q[k] for k in range(3)]
                    a = [p[1] * n[2] - p[2] * n[1], p[2] * n[0] - p[0] * n[2], p[0] * n[1] - p[1] * n[0], n[0], n[1], n[2],
                         (p[0] * n[0] + p[1] * n[1]) + p[2] * n[2]]
                    r = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]
                    v[:28] = [a[s] * a[t] for s in range(7) for t in range(s, 7)]
                    v[28:35] = [a[s] * r for s in range(7)]
                    v[35], v[36] = r * r, d2[i]
            rows.append(v)

        def tree(block):
            block = list(block)
            s = 128
            while s:
                for j in range(s):
                    block[j] = block[j] + block[j + s]
                s >>= 1
            return block[0]

        zero = np.zeros(37)
        partials = []
        for b in range(-(-N // 256)):
            block = rows[256 * b:256 * b + 256]
            partials.append(tree(block + [zero] * (256 - len(block))))
        threads = []
        for j in range(256):
            acc = np.zeros(37)
            for k in range(j, len(partials), 256):
                acc = acc + partials[k]
            threads.append(acc)
        return tree(threads), matched, bad, flat


# ---- street pairs with different samples -----------------------------------------------------------------------------------------------

def corridor(seed=0):
    """float64 [8000,3]: cloud_align_util.street without its three cross planes: ground and two walls.  Nothing constrains a
    translation along it (z)."""
    rng = np.random.default_rng(seed)
    g = np.zeros((5000, 3))
    g[:, 0], g[:, 2] = rng.uniform(-4, 4, 5000), rng.uniform(-20, 20, 5000)
    parts = [g]
    for x in (-4.0, 4.0):
        w = np.zeros((1500, 3))
        w[:, 0], w[:, 1], w[:, 2] = x, rng.uniform(0, 3, 1500), rng.uniform(-20, 20, 1500)
        parts.append(w)
    p = np.concatenate(parts) + np.array([1.5, -0.5, 3.0])
    return p[rng.permutation(len(p))]


def _carried_back(cloud, which):
    c, R, t = A.planted(which)
    return (cloud - t).dot(R) / c, (c, R, t)


def other_pair(which):
    """(pred, ref, (c, R, t)): the street sampled with ANOTHER seed carried through the inverse of the planted transform, and the
    street: no predicted point has its own image in the reference."""
    pred, planted = _carried_back(A.street(7), which)
    return pred, A.street(0), planted


def corridor_pair(which="small"):
    pred, planted = _carried_back(corridor(7), which)
    return pred, corridor(0), planted


def displacement(pred, result, planted):
    """The largest distance between where the result and where the planted transform put a predicted point."""
    c, R, t = planted
    got = result.scale * pred.dot(result.R.T) + result.t
    want = c * pred.dot(np.asarray(R).T) + t
    return float(np.sqrt(((got - want) ** 2).sum(1)).max())


# ---- files for the script ----------------------------------------------------------------------------------------------------------------

def street_tree(tmp_path):
    """A KITTI odometry tree whose four scans carry the street between them, the predicted cloud (the inverse image of two thirds of
    it under planted("small"), a PLY in float32) and the poses it would have been fused with -> (root, scans, poses_file, own_file,
    cloud_ply, pred)."""
    ref, (c, R, t) = A.street(), A.planted("small")
    poses = np.zeros((4, 3, 4))
    for s in range(4):
        poses[s, :, :3] = np.eye(3)
        poses[s, :, 3] = [1.5 + 2.0 * (s % 2), 1.0 + 0.5 * (s // 2), -30.0 + 1.5 * s]
    scans = []
    for s in range(4):
        velo = (ref[s::4] - poses[s, :, 3] - E.TR[:, 3]).dot(E.TR[:, :3])      # the inverse of TR: its 3x3 is orthonormal
        scans.append(np.concatenate([velo, np.full((len(velo), 1), 0.5)], 1).astype(np.float32))
    root = str(tmp_path / "odom")
    poses_file = E.write_odometry_tree(root, scans, poses)
    pred = ((ref[np.arange(len(ref)) % 3 != 2] - t).dot(R) / c).astype(np.float32)
    cloud_ply = str(tmp_path / "cloud.ply")
    cloud.save_ply(cloud_ply, pred, np.full((len(pred), 3), 7, np.uint8), np.ones(len(pred), np.int32))
    own_file = str(tmp_path / "own_poses.txt")
    odometry.save_kitti_poses(own_file, A.carried(poses, c, R, t))
    return root, scans, poses_file, own_file, cloud_ply, pred


def save_xyz_ply(path, xyz):
    """A binary PLY with x y z alone, as other tools export a lidar cloud: cloud.load_ply reads it."""
    rec = np.empty(len(xyz), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    rec["x"], rec["y"], rec["z"] = np.asarray(xyz, np.float32).T
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(xyz)
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + rec.tobytes())
