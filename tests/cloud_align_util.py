"""Seeded scenes and literal loops for the tests of tripled_amd.cloud_align: correspondences with every kind of row planted (matched,
unmatched, trimmed, NaN, an index of -1, -2, M and M - 1), a per-row Python loop over the two-stage tree, a per-point transform loop,
and a small street with an exactly planted similarity transform."""
import math

import numpy as np

from tripled_amd import cloud_align

MOMENT_SIZES = (1, 255, 256, 257, 65537)      # 65 537 rows are 257 partials: the smallest N at which a stage-2 thread adds two
STREET_TAU = 0.6
PLANTED = {"small": (1.0, 1.02, 0.1), "large": (2.0, 1.03, 0.2)}      # degrees about a tilted axis, scale, translation


# ---- moments -----------------------------------------------------------------------------------------------------------------------

def correspondences(N, M=97, seed=0, kind="mixed"):
    """(cur [N,3], ref [M,3], index [N], d2 [N], trim2, origin) as a nearest-neighbour query could have left them, with poison:
    ``mixed``: about two thirds matched; the others unmatched (-1, +inf), beyond trim2, a NaN d2, a NaN row of cur with index -1,
    an index of -2, of M and of 2^40 (all three must read nothing), and M - 1 (the last row that may be read); one d2 equal to trim2.
    ``matched``: every row matched;  ``unmatched``: none."""
    rng = np.random.default_rng(seed + 1000 * N)
    ref = rng.uniform(-30, 50, (M, 3))
    index = rng.integers(0, M, N).astype(np.int64)
    cur = ref[index] + rng.normal(0, 0.2, (N, 3))
    trim2 = 0.25
    d2 = rng.uniform(0, trim2, N)
    origin = np.array([9.5, 10.25, -3.0])
    if kind == "unmatched":
        index[:], d2[:] = -1, np.inf
    elif kind == "mixed":
        lot = rng.integers(0, 12, N)
        index[lot == 0], d2[lot == 0] = -1, np.inf
        d2[lot == 1] = np.nextafter(trim2, 1.0)
        d2[lot == 2] = np.nan
        cur[lot == 3], index[lot == 3], d2[lot == 3] = np.nan, -1, np.inf
        for at, (j, v) in enumerate(((M - 1, 0.1), (-2, 0.1), (M, 0.1), (2 ** 40, 0.1), (0, trim2))):      # planted where N allows
            if 3 * at < N:
                index[3 * at], d2[3 * at] = j, v
                cur[3 * at] = ref[min(max(j, 0), M - 1)] + 0.125
    return cur, ref, index, d2, trim2, origin


def moments_loop(cur, ref, index, d2, trim2, origin):
    """cloud_align.moments_numpy as a plain loop over the rows and over the tree, following the module's docstring literally (a row's
    17 slots are one numpy vector: the slots never mix)."""
    N, M = len(cur), len(ref)
    matched = bad = 0
    rows = []
    with np.errstate(invalid="ignore"):
        for i in range(N):
            v = np.zeros(17)
            j = int(index[i])
            if j >= M or j < -1:
                bad += 1
            elif j >= 0 and d2[i] <= trim2:
                matched += 1
                p, q = cur[i] - origin, ref[j] - origin
                v[0:3], v[3:6] = p, q
                v[6:15] = [q[r] * p[c] for r in range(3) for c in range(3)]
                v[15] = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
                v[16] = d2[i]
            rows.append(v)

        def tree(block):                                   # 256 vectors -> one
            block = list(block)
            s = 128
            while s:
                for j in range(s):
                    block[j] = block[j] + block[j + s]
                s >>= 1
            return block[0]

        zero = np.zeros(17)
        partials = []
        for b in range(-(-N // 256)):
            block = rows[256 * b:256 * b + 256]
            partials.append(tree(block + [zero] * (256 - len(block))))
        threads = []
        for j in range(256):
            acc = np.zeros(17)
            for k in range(j, len(partials), 256):
                acc = acc + partials[k]
            threads.append(acc)
        return tree(threads), matched, bad


def transform_loop(src, c, R, t):
    out = np.empty((len(src), 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, (x, y, z) in enumerate(np.asarray(src, np.float64)):
            for k in range(3):
                out[i, k] = c * ((R[k][0] * x + R[k][1] * y) + R[k][2] * z) + t[k]
    return out


def points_with_poison(N, seed=0):
    rng = np.random.default_rng(seed + N)
    p = rng.uniform(-50, 50, (N, 3))
    for at, v in ((0, np.nan), (5, np.inf), (7, -np.inf)):
        if N > 8:
            p[at, at % 3] = v
    return p


def rotation(axis, degrees):
    """Rodrigues' formula, float64."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K.dot(K)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


# ---- the street ----------------------------------------------------------------------------------------------------------------------

def street(seed=0):
    """float64 [9200,3]: a ground strip 8 x 40 (y = 0), two walls 3 high along it (x = -4 and x = 4) and three cross planes (z = -12,
    1 and 15), sampled uniformly at about one point per 0.25 x 0.25 patch, in shuffled order."""
    rng = np.random.default_rng(seed)
    parts = []
    g = np.zeros((5000, 3))
    g[:, 0], g[:, 2] = rng.uniform(-4, 4, 5000), rng.uniform(-20, 20, 5000)
    parts.append(g)
    for x in (-4.0, 4.0):
        w = np.zeros((1500, 3))
        w[:, 0], w[:, 1], w[:, 2] = x, rng.uniform(0, 3, 1500), rng.uniform(-20, 20, 1500)
        parts.append(w)
    for z in (-12.0, 1.0, 15.0):
        c = np.zeros((400, 3))
        c[:, 0], c[:, 1], c[:, 2] = rng.uniform(-4, 4, 400), rng.uniform(0, 3, 400), z
        parts.append(c)
    p = np.concatenate(parts) + np.array([1.5, -0.5, 3.0])
    return p[rng.permutation(len(p))]


def planted(which):
    """-> (c, R, t): the transform that maps the predicted cloud onto the reference."""
    degrees, scale, shift = PLANTED[which]
    R = rotation([0.3, 1.0, 0.2], degrees)
    t = shift * np.array([0.6, -0.3, 0.74])
    return scale, R, t / np.linalg.norm(t) * shift


def street_pair(which, seed=0):
    """(pred [6133,3], ref [9200,3], (c, R, t)): the predicted cloud is two thirds of the reference's points carried through the
    INVERSE of the planted transform, so that c R pred + t is the reference's point up to rounding."""
    ref = street(seed)
    c, R, t = planted(which)
    keep = np.nonzero(np.arange(len(ref)) % 3 != 2)[0]
    pred = (ref[keep] - t).dot(R) / c                          # R^T (x - t) / c
    return pred, ref, (c, R, t)


def trajectory(n=40):
    """[n,3,4] camera-to-world poses along the street, with a gentle turn."""
    poses = np.zeros((n, 3, 4))
    for i in range(n):
        poses[i, :, :3] = rotation([0, 1, 0], 0.5 * i)
        poses[i, :, 3] = [1.5 + 0.02 * i * i / n, 1.0 + 0.01 * i, -15.0 + 0.9 * i]
    return poses


def carried(poses, c, R, t):
    """The poses of a cloud that the planted transform maps onto the reference: centre = R^T (centre_gt - t) / c."""
    out = poses.copy()
    out[:, :, 3] = (poses[:, :, 3] - t).dot(R) / c
    out[:, :, :3] = np.einsum("ji,njk->nik", R, poses[:, :, :3])
    return out
