"""Seeded scenes and literal loops for the tests of tripled_amd.cloud_eval: nearest-neighbour scenes with the points planted that
decide whether a search is right (exact ties, neighbours at exactly the radius, duplicates, unusable queries), batches of velodyne
scans that exercise every cause, an analytic wall, and a tiny KITTI odometry tree."""
import math
import os

import numpy as np

from tripled_amd import cloud, cloud_eval, odometry

TAUS = (0.1, 0.25, 1.0)
HALF = cloud.HALF


# ---- nearest neighbour -----------------------------------------------------------------------------------------------------------

def lattice_step(tau):
    """The power of two at or below tau / 2: lattice coordinates and the midpoints between them are exact in float64."""
    return 2.0 ** math.floor(math.log2(tau / 2))


def lattice(tau, n=5, origin=(-3, 2, -1)):
    """n^3 lattice points (multiples of lattice_step) and the (n-1)^3 cube centres: a centre is equally far, in exact arithmetic and
    in float64, from its cube's eight corners."""
    h = lattice_step(tau)
    i = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)
    corners = i * h
    j = np.stack(np.meshgrid(*[np.arange(n - 1)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)
    return corners.astype(np.float64), (j + 0.5) * h


def nn_scene(tau, seed=0, n_ref=4097, n_query=1000):
    """(query float64 [n_query,3], ref float64 [n_ref,3]).  The reference, shuffled so that index order is not cell order: a lattice
    (ties), a dense random blob, a copy of the sparse queries moved by exactly tau along an axis (neighbours at the radius, one cell
    over), a handful of points twice (d2 = 0, two candidates).  The queries: the lattice's cube centres and corners, points in the
    blob, the sparse points, the duplicated points, NaN and inf rows, and one point farther than tau from everything."""
    rng = np.random.default_rng(seed)
    corners, centres = lattice(tau)
    sparse = rng.uniform(-60 * tau, -20 * tau, (96, 3))                       # ~1.5e-3 points per tau^3: alone but for their copies
    shifted = sparse.copy()
    shifted[np.arange(96), np.arange(96) % 3] += tau * np.where(np.arange(96) % 2 == 0, 1.0, -1.0)
    twice = rng.uniform(30 * tau, 34 * tau, (16, 3))
    n_blob = n_ref - len(corners) - len(shifted) - 2 * len(twice)
    side = tau * (4.19 * n_blob) ** (1.0 / 3.0)                               # about one point per ball of radius tau
    blob = rng.uniform(0, side, (n_blob, 3)) + np.array([0.0, 20 * tau, 0.0])
    ref = np.concatenate([corners, shifted, twice, twice, blob])
    ref = ref[rng.permutation(len(ref))]
    special = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e4 * tau, 0, 0], [0.0, 2.0 ** 21 * tau, 0.0]])
    planted = np.concatenate([centres, corners[::7], sparse, twice, special])
    n_blob_q = n_query - len(planted)
    assert n_blob > 0 and n_blob_q > 0
    near = blob[rng.integers(0, n_blob, n_blob_q // 2)] + rng.normal(0, 0.4 * tau, (n_blob_q // 2, 3))
    inside = rng.uniform(0, side, (n_blob_q - len(near), 3)) + np.array([0.0, 20 * tau, 0.0])
    return np.concatenate([planted, near, inside]), ref


def random_scene(N, M, tau, seed=0):
    """N queries and M reference points in one box with about one reference point per ball of radius tau; half of the queries sit
    near a reference point, every 16th ON one."""
    rng = np.random.default_rng(seed)
    side = tau * max(4.19 * M, 8.0) ** (1.0 / 3.0)
    ref = rng.uniform(-side / 2, side / 2, (M, 3))
    query = rng.uniform(-side / 2, side / 2, (N, 3))
    if M:
        pick = rng.integers(0, M, N)
        near = ref[pick] + rng.normal(0, 0.3 * tau, (N, 3))
        query = np.where((np.arange(N) % 2 == 0)[:, None], near, query)
        query = np.where((np.arange(N) % 16 == 0)[:, None], ref[pick], query)
    return query, ref


def ties_broken_by_index(query, ref, tau):
    """The number of queries whose winning d2 is reached by more than one reference point (all pairs)."""
    nb = cloud_eval.nearest_bruteforce(query, ref, tau)
    n = 0
    for q, d2 in zip(query[nb.index >= 0], nb.d2[nb.index >= 0]):
        e = ref - q
        n += np.count_nonzero(((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2]) == d2) > 1
    return n


# ---- scans -----------------------------------------------------------------------------------------------------------------------

TR = np.array([[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.07], [1.0, 0.0, 0.0, -0.27]])      # x forward, y left, z up -> right, down, forward
SCAN_H, SCAN_W = 32, 104
SCAN_VOXEL = 1e-4                                        # the key range ends at 104.86: world points beyond it exist
SCAN_PARAMS = dict(min_depth=1.0, max_range=45.0, inv_voxel=1.0 / SCAN_VOXEL)


def scan_K(H=SCAN_H, W=SCAN_W):
    return np.array([[0.58 * W, 0.0, 0.5 * W], [0.0, 1.92 * H, 0.5 * H], [0.0, 0.0, 1.0]])


def scan_poses(S):
    """Camera-to-world: a yaw of 0.05 s and translations that grow until, from the third scan on, far points leave the key range."""
    poses = np.zeros((S, 3, 4))
    for s in range(S):
        a = 0.05 * s
        poses[s, :, :3] = [[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]]
        poses[s, :, 3] = [0.5 * s, -0.1 * s, 35.0 * s]
    return poses


def scan_batch(lengths=(0, 1, 65, 1000), seed=0):
    """(points float32 [n,4], offsets int64 [S+1], poses float64 [S,3,4]): points all around the sensor (so the view test has work),
    behind and beyond the depth range, with planted NaN / inf coordinates and reflectances that are NaN, negative and above 1."""
    rng = np.random.default_rng(seed)
    scans = []
    for s, n in enumerate(lengths):
        p = np.empty((n, 4), np.float32)
        p[:, 0] = rng.uniform(-10, 60, n)
        p[:, 1] = rng.uniform(-12, 12, n)
        p[:, 2] = rng.uniform(-2.5, 1.5, n)
        p[:, 3] = rng.uniform(0, 1, n)
        ahead = rng.random(n) < 0.5                      # half of the points inside the camera's frustum, roughly
        p[ahead, 1] *= 0.02 * np.abs(p[ahead, 0])
        p[ahead, 2] *= 0.02 * np.abs(p[ahead, 0])
        if n >= 32:
            p[3, 0], p[5, 1], p[7, 2] = np.nan, np.inf, -np.inf
            p[9, 3], p[11, 3], p[13, 3], p[15, 3], p[17, 3] = np.nan, -0.5, 1.5, np.inf, 0.5
            p[[9, 11, 13, 15, 17], :3] = [[8.0 + s, 0.1, -0.2]] * 5          # in view, in range
        scans.append(p)
    offsets = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return np.concatenate(scans, 0), offsets, scan_poses(len(lengths))


def scan_keys_loop(points, offsets, Tr, poses, K=None, height=0, width=0, min_depth=0.0, max_range=1.0, inv_voxel=1.0):
    """cloud_eval.scan_keys_numpy as a plain loop over the points that follows the module's docstring literally."""
    Tr = np.asarray(Tr, np.float64).reshape(3, 4)
    key, payload, counts = [], [], [0] * 5
    f64 = np.float64
    with np.errstate(all="ignore"):
        for i, p in enumerate(np.asarray(points, np.float32)):
            owner = [s for s in range(len(offsets) - 1) if offsets[s] <= i < offsets[s + 1]]
            cause, k, pay = 0, cloud.INVALID_KEY, 0
            x, y, z = f64(p[0]), f64(p[1]), f64(p[2])
            if not owner or not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                cause = 1
            else:
                cam = [((Tr[r, 0] * x + Tr[r, 1] * y) + Tr[r, 2] * z) + Tr[r, 3] for r in range(3)]
                if not (min_depth <= cam[2] <= max_range):
                    cause = 2
                elif height > 0:
                    u = ((K[0][0] * cam[0] + K[0][1] * cam[1]) + K[0][2] * cam[2]) / cam[2]
                    v = ((K[1][0] * cam[0] + K[1][1] * cam[1]) + K[1][2] * cam[2]) / cam[2]
                    if not (0 <= u <= width - 1 and 0 <= v <= height - 1):
                        cause = 3
            if cause == 0:
                P = poses[owner[0]]
                g = [(((P[r, 0] * cam[0] + P[r, 1] * cam[1]) + P[r, 2] * cam[2]) + P[r, 3]) * f64(inv_voxel) for r in range(3)]
                fl = [np.floor(v) for v in g]
                if not all(-HALF <= v < HALF for v in fl):
                    cause = 4
                else:
                    k = int(cloud.pack_key(*[int(v) for v in fl]))
                    if k == cloud.INVALID_KEY:
                        cause = 4
                    else:
                        q = [min(1023, int(np.floor((a - b) * 1024.0))) for a, b in zip(g, fl)]
                        c = np.floor(f64(p[3]) * 255.0 + 0.5)
                        c = int(min(max(c, 0.0), 255.0)) if not np.isnan(c) else 0
                        pay = q[0] | q[1] << 10 | q[2] << 20 | c << 30 | c << 38 | c << 46
            key.append(k if cause == 0 else cloud.INVALID_KEY)
            payload.append(pay if cause == 0 else 0)
            counts[cause] += 1
    return np.array(key, np.int64).reshape(-1), np.array(payload, np.uint64).reshape(-1), np.array(counts, np.int64)


# ---- the analytic wall and the odometry tree ---------------------------------------------------------------------------------------

WALL_TAU, WALL_VOXEL, WALL_Z = 0.25, 0.1, 10.0           # tau a power of two: n copies of it sum exactly


def wall_scans(S=3, step=0.05):
    """S scans of the wall cam_z = WALL_Z, x in [-4, 4], y in [-1, 1] as seen from cameras that move sideways (identity rotations),
    in velodyne coordinates for Tr = TR.  Every voxel column of the wall is hit by every scan."""
    poses = np.zeros((S, 3, 4))
    scans = []
    xs, ys = np.meshgrid(np.arange(-4.0, 4.0 + 1e-9, step), np.arange(-1.0, 1.0 + 1e-9, step), indexing="ij")
    for s in range(S):
        poses[s, :, :3] = np.eye(3)
        poses[s, :, 3] = [0.25 * s, 0.0, 0.0]
        cam = np.stack([xs.reshape(-1) - poses[s, 0, 3], ys.reshape(-1), np.full(xs.size, WALL_Z)], 1)      # world -> camera s
        velo = np.stack([cam[:, 2] - TR[2, 3], -(cam[:, 0] - TR[0, 3]), -(cam[:, 1] - TR[1, 3])], 1)        # the inverse of TR
        scans.append(np.concatenate([velo, np.full((len(velo), 1), 0.5)], 1).astype(np.float32))
    return scans, poses


def wall_prediction(step=0.07, margin=0.05):
    """A predicted cloud on the same wall: another sampling, kept ``margin`` inside the lidar's extent."""
    xs, ys = np.meshgrid(np.arange(-4.0 + margin, 4.0 - margin, step), np.arange(-1.0 + margin, 1.0 - margin, step), indexing="ij")
    return np.stack([xs.reshape(-1), ys.reshape(-1), np.full(xs.size, WALL_Z)], 1).astype(np.float32)


def write_odometry_tree(root, scans, poses, sequence=9):
    """sequences/NN/velodyne/%06d.bin, sequences/NN/calib.txt (P0 ... P3 and Tr) and poses/NN.txt -> the pose file's path."""
    seq = os.path.join(root, "sequences", "%02d" % sequence)
    os.makedirs(os.path.join(seq, "velodyne"))
    os.makedirs(os.path.join(root, "poses"))
    for n, scan in enumerate(scans):
        np.asarray(scan, np.float32).tofile(os.path.join(seq, "velodyne", "%06d.bin" % n))
    with open(os.path.join(seq, "calib.txt"), "w") as f:
        for name in ("P0", "P1", "P2", "P3"):
            f.write("%s: %s\n" % (name, " ".join("%.12e" % v for v in np.eye(3, 4).reshape(-1))))
        f.write("Tr: %s\n" % " ".join("%.12e" % v for v in TR.reshape(-1)))
    path = os.path.join(root, "poses", "%02d.txt" % sequence)
    odometry.save_kitti_poses(path, poses)
    return path
