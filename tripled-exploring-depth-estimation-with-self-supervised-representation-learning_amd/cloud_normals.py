"""Surface normals of a cloud: per point the direction of least spread of its neighbours within a radius (the eigenvector of the
smallest eigenvalue of their covariance), with the surface variation lambda_min / trace as a measure of how flat the patch is.  What a
point-to-plane alignment (cloud_align.py, criterion="plane") needs per reference point, and what a PLY export carries as nx ny nz.
The reference has no such program.

Layers, as in cloud_eval.py:
  * host statements in numpy (``normals_numpy``, vectorised, and the all-pairs per-point loop ``normals_bruteforce`` that pins it): the
    host path (``device='cpu'``) and what the kernel is tested against, written in the kernel's operation order;
  * ``normals_hip`` (csrc/td_normals.hip): device tensors only, a CPU tensor is an error;
  * ``CloudNormals``: a cloud -> Normals in the cloud's own order.

Neighbours.  The query walks a cloud_eval.Grid built for ``tau`` the way td_nn_query does (9 lower bounds, at most three z-cells each).
For every grid point p with e = p - q and d2 = ((e_x e_x) + (e_y e_y)) + (e_z e_z) <= radius radius (a NaN fails; q itself counts when
it is in the grid; radius <= tau, so the 27 cells hold every such point):
    n += 1;   i_k = (int64) rint(e_k Q),  Q = 2^18 / radius (one division on the host), round half to even
    S1_k += i_k;   S2_kl += i_k i_l   for the six k <= l, in the order 00 01 02 11 12 22
All ten sums are 64-bit integers: the result depends neither on the order of the points inside a cell nor on the order the cells are
visited.  |i_k| <= 2^18 + 1, so below M = 2^26 grid points no sum can overflow; the entry point refuses more.

Per query with n >= min_neighbours, in float64, every operation rounded on its own:
    m_k = double(S1_k) / double(n);   C_kl = double(S2_kl) / double(n) - m_k m_l      (in units of 1 / Q^2)
The symmetric C (a_00 a_01 a_02 a_11 a_12 a_22) is diagonalised by cyclic Jacobi, V = I, SWEEPS sweeps over (p, q) = (0, 1), (0, 2),
(1, 2), never fewer.  A rotation whose a_pq is exactly 0 is skipped (nothing changes).  Otherwise, with r the third index:
    theta = (a_qq - a_pp) / (2 a_pq);   sign = -1 if theta < 0 else +1
    t = sign / (|theta| + sqrt(theta theta + 1));   c = 1 / sqrt(t t + 1);   s = t c
    h = t a_pq;   a_pp <- a_pp - h;   a_qq <- a_qq + h;   a_pq <- 0
    a_rp <- c a_rp - s a_rq;   a_rq <- s a_rp + c a_rq                        (both from the OLD a_rp, a_rq)
    v_kp <- c v_kp - s v_kq;   v_kq <- s v_kp + c v_kq   for k = 0, 1, 2      (likewise)
(a huge theta overflows theta theta to +inf, t becomes 0, c = 1, s = 0: no NaN arises from finite input).  Then l_k = a_kk,
    lo = the smallest l_k, lowest index among equal ones;   mid = max(min(l0, l1), min(max(l0, l1), l2));   trace = (l0 + l1) + l2
    normal = column lo of V divided by sqrt(((x x) + (y y)) + (z z)), its sign flipped so that the component of largest magnitude is
    positive (lowest index among equal magnitudes);   curvature = max(l_lo, 0) / trace
Every query ends in exactly one class, the first that holds: invalid (not finite or outside the key range, as in td_nn_query: count
0), few (n < min_neighbours), degenerate (not trace > 0, not mid > 0, or a normal or curvature that is not finite: the neighbours lie
in a point or on a line), rough (curvature > max_curvature: the curvature is written, the normal is not), valid.  Without a normal all
three components are +0.0; the curvature is +inf where it is undefined (invalid, few, degenerate).

SWEEPS = 4 is the smallest count at which the normals of the seeded test clouds agree with numpy.linalg.eigh's eigenvector within 1e-12
(sine of the angle) wherever (l1 - l0) / trace >= 1e-6 (tests/test_cloud_plane_cpu.py; DESIGN 25 has the figures).

Orientation (``orient_numpy``, ``orient_bruteforce``, ``orient_hip``: td_normals_orient in csrc/td_surfel.hip).  Given the poses the cloud
was fused under, every normal is turned towards the camera centre nearest to its point.  Per point p (float32, widened) and camera c,
float64, every operation rounded on its own:
    centre_c = pose_scale t_c;   w = centre_c - p;   d2_c = ((w_x w_x) + (w_y w_y)) + (w_z w_z)
    the viewpoint is the c of the smallest d2_c, the lowest c among equal ones; a NaN distance never wins (camera -1 when none did)
    s = ((n_x w_x) + (n_y w_y)) + (n_z w_z) with the winner's w;   the normal is negated (exactly) when s < 0, kept when s >= 0
Every point ends in exactly one class: none (no normal, all three components zero: it stays +0.0, its nearest camera is still
reported), invalid (no camera won, or s is a NaN: the normal stays as it is), flipped, kept.  Orienting twice changes nothing.
LIMIT of the viewpoint rule: the fused cloud keeps no record of which frame saw a voxel.  The nearest camera on the trajectory is on
the seen side of any surface the trajectory did not pass through; where the trajectory passes on both sides of a thin surface, or a
surface was seen from far away while the trajectory later came near its back, the sign can be wrong.

Limits: without poses the normal has no orientation beyond the sign convention; the covariance is of coordinates
quantised to radius 2^-18; a fixed radius, no k-nearest; the defaults min_neighbours = 6 and max_curvature = 0.01 are UNTUNED.
"""
import collections
import math

import numpy as np
import torch

from . import cloud, cloud_eval, native

SWEEPS = native.CONSTANTS["TD_NORMALS_SWEEPS"]
QUANT = 2.0 ** 18                     # csrc/td_normals.hip: the host passes Q = QUANT / radius
MAX_POINTS = 1 << 26                  # grid points: below it the integer sums cannot overflow
CAUSES = ("valid", "few", "degenerate", "rough", "invalid")
ORIENT_STATS = ("flipped", "kept", "none", "invalid")
ORIENT_CHUNK = 256                    # csrc/td_surfel.hip: camera centres staged through LDS at a time
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))

Normals = collections.namedtuple("Normals", "normal curvature count stats")
Normals.__doc__ = """normal float64 [N,3] (unit length, +0.0 in all three where the point has none), curvature float64 [N] (lambda_min /
trace, +inf where undefined), count int64 [N] (neighbours within the radius, the point itself included), stats: int64 [5] in the order
of CAUSES (a device tensor from normals_hip; CloudNormals turns it into a dict of Python ints)."""


def _params(grid, radius, min_neighbours, max_curvature):
    """-> (radius, r2, Q, min_neighbours, max_curvature), checked."""
    if not isinstance(grid, cloud_eval.Grid):
        raise ValueError("grid: a cloud_eval.Grid")
    cloud_eval.inv_cell(grid.tau)
    radius = grid.tau if radius is None else float(radius)
    if not (0 < radius <= grid.tau):
        raise ValueError("radius: inside (0, tau = %r], got %r" % (grid.tau, radius))
    if int(min_neighbours) != min_neighbours or int(min_neighbours) < 3:
        raise ValueError("min_neighbours: an integer, at least 3; got %r" % (min_neighbours,))
    max_curvature = float(max_curvature)
    if not max_curvature >= 0:
        raise ValueError("max_curvature: not negative, got %r" % (max_curvature,))
    if len(grid.points) >= MAX_POINTS:
        raise ValueError("at most 2^26 - 1 grid points, got %d" % len(grid.points))
    return radius, radius * radius, QUANT / radius, int(min_neighbours), max_curvature


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _jacobi_numpy(a):
    """a: dict (k, l) -> float64 [n] for k <= l.  -> (l [3] of [n], V [3][3] of [n]) after SWEEPS cyclic sweeps, np.where for the skip."""
    n = len(a[0, 0])
    a = dict(a)
    V = [[np.full(n, 1.0 if r == c else 0.0) for c in range(3)] for r in range(3)]
    key = lambda i, j: (i, j) if i <= j else (j, i)
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p, q in ((0, 1), (0, 2), (1, 2)):
                r = 3 - p - q
                apq = a[p, q]
                skip = apq == 0.0
                theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                sign = np.where(theta < 0.0, -1.0, 1.0)
                t = sign / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                h = t * apq
                keep = lambda old, new: np.where(skip, old, new)
                app, aqq = keep(a[p, p], a[p, p] - h), keep(a[q, q], a[q, q] + h)
                arp, arq = a[key(r, p)], a[key(r, q)]
                a[key(r, p)], a[key(r, q)] = keep(arp, c * arp - s * arq), keep(arq, s * arp + c * arq)
                a[p, p], a[q, q], a[p, q] = app, aqq, keep(apq, 0.0)
                for k in range(3):
                    vp, vq = V[k][p], V[k][q]
                    V[k][p], V[k][q] = keep(vp, c * vp - s * vq), keep(vq, s * vp + c * vq)
    return [a[0, 0], a[1, 1], a[2, 2]], V


def _finish_numpy(sums, valid, min_neighbours, max_curvature):
    """sums int64 [N,10] (n, S1 (3), S2 (6)), valid bool [N] -> Normals of numpy arrays."""
    N = len(sums)
    normal, curvature = np.zeros((N, 3)), np.full(N, np.inf)
    count = np.where(valid, sums[:, 0], 0).astype(np.int64)
    cause = np.full(N, 4, np.int8)                                  # invalid
    cause[valid] = 1                                                # few, until shown otherwise
    who = np.nonzero(valid & (count >= min_neighbours))[0]
    if len(who):
        with np.errstate(all="ignore"):
            n = sums[who, 0].astype(np.float64)
            m = [sums[who, 1 + k].astype(np.float64) / n for k in range(3)]
            a = {(k, l): sums[who, 4 + at].astype(np.float64) / n - m[k] * m[l] for at, (k, l) in enumerate(PAIRS)}
            l, V = _jacobi_numpy(a)
            lo = np.where(l[1] < l[0], 1, 0)
            lo = np.where(l[2] < np.where(lo == 1, l[1], l[0]), 2, lo)
            lmin = np.where(lo == 0, l[0], np.where(lo == 1, l[1], l[2]))
            mid = np.maximum(np.minimum(l[0], l[1]), np.minimum(np.maximum(l[0], l[1]), l[2]))
            trace = (l[0] + l[1]) + l[2]
            x, y, z = (np.where(lo == 0, V[k][0], np.where(lo == 1, V[k][1], V[k][2])) for k in range(3))
            norm = np.sqrt(((x * x) + (y * y)) + (z * z))
            x, y, z = x / norm, y / norm, z / norm
            big = np.where(np.abs(y) > np.abs(x), 1, 0)
            big = np.where(np.abs(z) > np.where(big == 1, np.abs(y), np.abs(x)), 2, big)
            lead = np.where(big == 0, x, np.where(big == 1, y, z))
            flip = lead < 0.0
            x, y, z = np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)
            curv = np.where(lmin > 0.0, lmin, 0.0) / trace
            fine = (trace > 0.0) & (mid > 0.0) & np.isfinite(l[0]) & np.isfinite(l[1]) & np.isfinite(l[2]) & np.isfinite(x) & \
                np.isfinite(y) & np.isfinite(z) & np.isfinite(curv)
            rough = fine & (curv > max_curvature)
            good = fine & ~rough
        cause[who] = np.where(good, 0, np.where(rough, 3, 2))
        curvature[who] = np.where(fine, curv, np.inf)
        for k, v in enumerate((x, y, z)):
            normal[who, k] = np.where(good, v, 0.0)
    return Normals(normal, curvature, count, np.bincount(cause, minlength=5).astype(np.int64))


def _sums_numpy(q, grid, r2, Q):
    """-> (sums int64 [N,10]: n, S1 (3), S2 (6);  valid bool [N]) over cloud_eval.walk_numpy's candidates."""
    key, valid = cloud_eval._cells_numpy(q, cloud_eval.inv_cell(grid.tau))
    N = len(q)
    sums = np.zeros((N, 10), np.int64)
    who = np.nonzero(valid)[0]
    if len(who) and len(grid.points):
        for act, p in cloud_eval.walk_numpy(grid, key[who]):
            qi = who[act]
            with np.errstate(invalid="ignore", over="ignore"):
                e = grid.points[p] - q[qi]
                d2 = ((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2])
                take = d2 <= r2                                 # a NaN fails
                i = np.rint(e[take] * Q).astype(np.int64)
            rows = qi[take]                                     # every query at most once per yield: no repeated index
            sums[rows, 0] += 1
            sums[rows, 1:4] += i
            for at, (k, l) in enumerate(PAIRS):
                sums[rows, 4 + at] += i[:, k] * i[:, l]
    return sums, valid


def normals_numpy(query, grid, radius=None, min_neighbours=6, max_curvature=0.01):
    """query float64 [N,3], grid: cloud_eval.grid_numpy's -> Normals of numpy arrays.  The statement td_cloud_normals is tested
    against."""
    q = cloud_eval._xyz64(query, "query")
    radius, r2, Q, min_neighbours, max_curvature = _params(grid, radius, min_neighbours, max_curvature)
    sums, valid = _sums_numpy(q, grid, r2, Q)
    return _finish_numpy(sums, valid, min_neighbours, max_curvature)


def covariances_numpy(query, grid, radius=None):
    """-> (C float64 [N,3,3], count int64 [N]): the covariance the Jacobi sweeps are given (module docstring, in units of 1 / Q^2;
    NaN where count is 0), for judging them against another eigen-solver."""
    q = cloud_eval._xyz64(query, "query")
    radius, r2, Q, _, _ = _params(grid, radius, 3, 0.0)
    sums, valid = _sums_numpy(q, grid, r2, Q)
    count = np.where(valid, sums[:, 0], 0).astype(np.int64)
    C = np.full((len(q), 3, 3), np.nan)
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)
        m = [sums[:, 1 + k].astype(np.float64) / n for k in range(3)]
        for at, (k, l) in enumerate(PAIRS):
            C[:, k, l] = C[:, l, k] = sums[:, 4 + at].astype(np.float64) / n - m[k] * m[l]
    return C, count


def _jacobi_scalar(a00, a01, a02, a11, a12, a22):
    """The module docstring's Jacobi on Python floats -> ([l0, l1, l2], V as three rows)."""
    a = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[p][q]
            if apq == 0.0:
                continue
            r = 3 - p - q
            theta = (a[q][q] - a[p][p]) / (2.0 * apq)
            sign = -1.0 if theta < 0.0 else 1.0
            sq = theta * theta                                      # may overflow to inf: t = 0
            t = sign / (abs(theta) + math.sqrt(sq + 1.0))
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            h = t * apq
            a[p][p], a[q][q] = a[p][p] - h, a[q][q] + h
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = c * arp - s * arq
            a[r][q] = a[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = V[k][p], V[k][q]
                V[k][p], V[k][q] = c * vp - s * vq, s * vp + c * vq
    return [a[0][0], a[1][1], a[2][2]], V


def normals_bruteforce(query, ref, tau, radius=None, min_neighbours=6, max_curvature=0.01):
    """normals_numpy over all pairs with no grid, one query at a time in plain Python with a scalar Jacobi: for the tests.  Reference
    points that are not finite or outside the key range are no candidates (the grid leaves them out)."""
    q, x = cloud_eval._xyz64(query, "query"), cloud_eval._xyz64(ref, "ref")
    tau = float(tau)
    ic = cloud_eval.inv_cell(tau)
    radius = tau if radius is None else float(radius)
    if not (0 < radius <= tau) or int(min_neighbours) < 3 or not float(max_curvature) >= 0:
        raise ValueError("0 < radius <= tau, min_neighbours >= 3, max_curvature >= 0; got %r, %r, %r" % (radius, min_neighbours, max_curvature))
    r2, Q = radius * radius, QUANT / radius
    key, usable = cloud_eval._cells_numpy(x, ic)
    x = x[usable & (key != cloud_eval.INVALID_KEY)]
    _, valid = cloud_eval._cells_numpy(q, ic)
    N = len(q)
    normal, curvature, count, stats = np.zeros((N, 3)), np.full(N, np.inf), np.zeros(N, np.int64), [0] * 5
    xs, qs = x.tolist(), q.tolist()                                  # Python floats: the same float64 operations, one at a time
    for i in range(N):
        if not valid[i]:
            stats[4] += 1
            continue
        n, S1, S2 = 0, [0, 0, 0], [0] * 6
        qx, qy, qz = qs[i]
        for px, py, pz in xs:
            ex, ey, ez = px - qx, py - qy, pz - qz
            if not ((ex * ex) + (ey * ey)) + (ez * ez) <= r2:
                continue
            v = [round(ex * Q), round(ey * Q), round(ez * Q)]      # Python's round: half to even, to an exact int
            n += 1
            for k in range(3):
                S1[k] += v[k]
            for at, (k, l) in enumerate(PAIRS):
                S2[at] += v[k] * v[l]
        count[i] = n
        if n < min_neighbours:
            stats[1] += 1
            continue
        m = [float(s) / float(n) for s in S1]
        c = [float(S2[at]) / float(n) - m[k] * m[l] for at, (k, l) in enumerate(PAIRS)]
        l, V = _jacobi_scalar(*c)
        lo = 1 if l[1] < l[0] else 0
        if l[2] < l[lo]:
            lo = 2
        mid = max(min(l[0], l[1]), min(max(l[0], l[1]), l[2]))
        trace = (l[0] + l[1]) + l[2]
        vx, vy, vz = V[0][lo], V[1][lo], V[2][lo]
        norm = math.sqrt(((vx * vx) + (vy * vy)) + (vz * vz))
        fine = trace > 0.0 and mid > 0.0 and all(math.isfinite(v) for v in l) and norm > 0.0 and math.isfinite(norm)
        if fine:
            v = [vx / norm, vy / norm, vz / norm]
            big = 1 if abs(v[1]) > abs(v[0]) else 0
            if abs(v[2]) > abs(v[big]):
                big = 2
            if v[big] < 0.0:
                v = [-v[0], -v[1], -v[2]]
            curv = (l[lo] if l[lo] > 0.0 else 0.0) / trace
            fine = all(math.isfinite(t) for t in v) and math.isfinite(curv)
        if not fine:
            stats[2] += 1
            continue
        curvature[i] = curv
        if curv > max_curvature:
            stats[3] += 1
            continue
        stats[0] += 1
        normal[i] = v
    return Normals(normal, curvature, count, np.array(stats, np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel

def normals_hip(query, grid, radius=None, min_neighbours=6, max_curvature=0.01, stats=None):
    """normals_numpy as one launch of td_cloud_normals -> Normals of device tensors.  ``grid``: cloud_eval.grid_hip's.  ``stats``: an
    int64 [5] device tensor that the launch increments (the order of CAUSES), or None for a fresh one.  No synchronisation."""
    q = cloud_eval._f64_points(query, "query")
    radius, _, Q, min_neighbours, max_curvature = _params(grid, radius, min_neighbours, max_curvature)
    if not all(torch.is_tensor(t) for t in (grid.points, grid.cell_key, grid.cell_start)):
        raise native.NativeLibraryError("libtripled_hip needs device tensors (got a host grid: cloud_eval.grid_hip builds the device's)")
    points = cloud_eval._f64_points(grid.points, "grid.points")
    M, N, dev = points.shape[0], q.shape[0], q.device
    cell_key = cloud._i64(grid.cell_key, "grid.cell_key")
    C = cell_key.shape[0]
    cell_start = cloud._i64(grid.cell_start, "grid.cell_start", C + 1)
    stats = torch.zeros(5, dtype=torch.int64, device=dev) if stats is None else cloud._i64(stats, "stats", 5)
    normal = torch.empty(N, 3, dtype=torch.float64, device=dev)
    curvature = torch.empty(N, dtype=torch.float64, device=dev)
    count = torch.empty(N, dtype=torch.int64, device=dev)
    if N == 0:                           # an empty tensor has no pointer to pass
        return Normals(normal, curvature, count, stats)
    native.call("td_cloud_normals", q, N, points if M else None, M, cell_key if C else None, cell_start, C, float(grid.tau), radius, Q,
                min_neighbours, max_curvature, normal, curvature, count, stats)
    return Normals(normal, curvature, count, stats)


# ---------------------------------------------------------------------------------------------------------------------------
# orientation towards the nearest camera

Oriented = collections.namedtuple("Oriented", "normal camera stats")
Oriented.__doc__ = """normal float32 [V,3], camera int32 [V] (the nearest camera, -1 where none won), stats int64 [4] in the order of
ORIENT_STATS: flipped, kept, none, invalid."""


def _orient_inputs(xyz, normal, poses):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim == 3 and poses.shape[1:] == (4, 4):
        poses = poses[:, :3]
    poses = np.ascontiguousarray(poses)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or normal.shape != xyz.shape or poses.ndim != 3 or poses.shape[1:] != (3, 4) or not len(poses):
        raise ValueError("xyz [V,3], normal [V,3], poses [C,3,4] with C >= 1; got %s, %s, %s" % (xyz.shape, normal.shape, poses.shape))
    return xyz, normal, poses


def orient_numpy(xyz, normal, poses, pose_scale=1.0):
    """xyz, normal float32 [V,3], poses float64 [C,3,4] camera-to-world -> Oriented of numpy arrays.  The statement td_normals_orient is
    tested against: one pass over the cameras in ascending order, vectorised over the points."""
    xyz, normal, poses = _orient_inputs(xyz, normal, poses)
    V, ps = len(xyz), np.float64(pose_scale)
    p = [xyz[:, k].astype(np.float64) for k in range(3)]
    camera = np.full(V, -1, np.int32)
    best, w = np.zeros(V), [np.zeros(V) for _ in range(3)]
    with np.errstate(all="ignore"):
        for c in range(len(poses)):
            d = [ps * poses[c, k, 3] - p[k] for k in range(3)]
            d2 = ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])
            win = (d2 == d2) & ((camera < 0) | (d2 < best))
            camera[win] = c
            best = np.where(win, d2, best)
            w = [np.where(win, d[k], w[k]) for k in range(3)]
        n = [normal[:, k].astype(np.float64) for k in range(3)]
        s = ((n[0] * w[0]) + (n[1] * w[1])) + (n[2] * w[2])
    none = (normal[:, 0] == 0) & (normal[:, 1] == 0) & (normal[:, 2] == 0)
    invalid = ~none & ((camera < 0) | (s != s))
    flipped = ~none & ~invalid & (s < 0.0)
    kept = ~none & ~invalid & ~flipped
    out = np.where(flipped[:, None], -normal, normal).astype(np.float32)
    stats = np.array([np.count_nonzero(m) for m in (flipped, kept, none, invalid)], np.int64)
    return Oriented(out, camera, stats)


def orient_bruteforce(xyz, normal, poses, pose_scale=1.0):
    """orient_numpy said a second time: one point at a time, Python floats, a plain loop over the cameras.  For the tests."""
    xyz, normal, poses = _orient_inputs(xyz, normal, poses)
    out, camera, stats = normal.copy(), np.full(len(xyz), -1, np.int32), [0, 0, 0, 0]
    centres = [[float(np.float64(pose_scale) * poses[c, k, 3]) for k in range(3)] for c in range(len(poses))]
    for i in range(len(xyz)):
        px, py, pz = (float(v) for v in xyz[i])
        cam, best, w = -1, 0.0, (0.0, 0.0, 0.0)
        for c, (cx, cy, cz) in enumerate(centres):
            dx, dy, dz = cx - px, cy - py, cz - pz
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            if d2 == d2 and (cam < 0 or d2 < best):
                cam, best, w = c, d2, (dx, dy, dz)
        camera[i] = cam
        nx, ny, nz = (float(v) for v in normal[i])
        if nx == 0.0 and ny == 0.0 and nz == 0.0:
            stats[2] += 1
            continue
        s = ((nx * w[0]) + (ny * w[1])) + (nz * w[2])
        if cam < 0 or s != s:
            stats[3] += 1
        elif s < 0.0:
            stats[0] += 1
            out[i] = -normal[i]
        else:
            stats[1] += 1
    return Oriented(out, camera, np.array(stats, np.int64))


def orient_hip(xyz, normal, poses, pose_scale=1.0):
    """orient_numpy as one launch of td_normals_orient -> Oriented of device tensors.  xyz, normal float32 [V,3], poses float64
    [C,3,4], all on one HIP device; a CPU tensor is an error.  No synchronisation."""
    native.load()
    native.require_device(xyz, normal, poses)
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or normal.dtype != torch.float32 or tuple(normal.shape) != tuple(xyz.shape) \
            or poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] < 1:
        raise ValueError("xyz float32 [V,3], normal float32 [V,3], poses float64 [C,3,4] with C >= 1; got %s %s, %s %s, %s %s" % (
            tuple(xyz.shape), xyz.dtype, tuple(normal.shape), normal.dtype, tuple(poses.shape), poses.dtype))
    V, dev = xyz.shape[0], poses.device
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    camera = torch.empty(V, dtype=torch.int32, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    if V == 0:                           # an empty tensor has no pointer to pass
        return Oriented(out, camera, stats)
    native.call("td_normals_orient", xyz.contiguous(), normal.contiguous(), V, poses.contiguous(), poses.shape[0], float(pose_scale), out,
                camera, stats)
    return Oriented(out, camera, stats)


# ---------------------------------------------------------------------------------------------------------------------------

class CloudNormals:
    """estimate(xyz) -> Normals in the cloud's own order: the grid is built from the cloud and every point is a query into it.

    device      'cuda[:i]': cloud_eval.grid_hip and normals_hip, the cloud may be a numpy array or a tensor anywhere and the Normals'
                arrays are device tensors; 'cpu': grid_numpy and normals_numpy.  The two paths agree on the bits.
    tau         the cell size of the grid;  radius: the neighbourhood, inside (0, tau], default tau
    min_neighbours, max_curvature   a point with fewer neighbours (itself included) or a rougher patch gets no normal; UNTUNED
    stats is a dict of Python ints under the names of CAUSES.

    estimate(xyz, poses=...) also orients the normals towards the nearest camera (module docstring): the points and the normals go
    through orient_numpy / orient_hip rounded to float32, which is what a PLY holds, and a normal that came back negated is negated in
    float64.  stats then also holds "orient_flipped", "orient_kept", "orient_none", "orient_invalid"."""

    def __init__(self, device, tau, radius=None, min_neighbours=6, max_curvature=0.01):
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        self.tau = float(tau)
        cloud_eval.inv_cell(self.tau)
        self.radius = self.tau if radius is None else float(radius)
        self.min_neighbours, self.max_curvature = min_neighbours, float(max_curvature)
        if not (0 < self.radius <= self.tau) or int(min_neighbours) != min_neighbours or min_neighbours < 3 or not self.max_curvature >= 0:
            raise ValueError("0 < radius <= tau, min_neighbours >= 3, max_curvature >= 0; got %r, %r, %r" % (radius, min_neighbours, max_curvature))

    def estimate(self, xyz, grid=None, poses=None, pose_scale=1.0):
        """``grid``: the cloud's Grid when the caller has built it already (for this tau, on this path).  ``poses``: [C,3,4] or
        [C,4,4] camera-to-world, None: the normals keep the sign convention."""
        if not self.on_hip:
            x = cloud_eval._xyz64(xyz, "xyz")
            grid = cloud_eval.grid_numpy(x, self.tau) if grid is None else grid
            out = normals_numpy(x, grid, self.radius, self.min_neighbours, self.max_curvature)
            counters = out.stats
        else:
            x = torch.as_tensor(xyz).to(self.device, torch.float64)
            if x.dim() != 2 or x.shape[1] != 3:
                raise ValueError("xyz: [n,3], got %s" % (tuple(x.shape),))
            x = x.contiguous()
            grid = cloud_eval.grid_hip(x, self.tau) if grid is None else grid
            out = normals_hip(x, grid, self.radius, self.min_neighbours, self.max_curvature)
            counters = out.stats.cpu().numpy()
        stats = {name: int(v) for name, v in zip(CAUSES, counters)}
        normal = out.normal
        if poses is not None:
            if not self.on_hip:
                n32 = normal.astype(np.float32)
                turned = orient_numpy(x.astype(np.float32), n32, poses, pose_scale)
                normal = np.where((turned.normal != n32).any(1)[:, None], -normal, normal)
                orient = turned.stats
            else:
                poses = _orient_inputs(np.zeros((0, 3)), np.zeros((0, 3)), poses.cpu().numpy() if torch.is_tensor(poses) else poses)[2]
                n32 = normal.to(torch.float32)
                turned = orient_hip(x.to(torch.float32), n32, torch.from_numpy(poses).to(self.device), pose_scale)
                normal = torch.where((turned.normal != n32).any(1)[:, None], -normal, normal)
                orient = turned.stats.cpu().numpy()
            stats.update({"orient_" + name: int(v) for name, v in zip(ORIENT_STATS, orient)})
        return Normals(normal, out.curvature, out.count, stats)
