"""A fused cloud scored against the lidar: the scans of a sequence fused into a reference cloud in the same world frame, a nearest-
neighbour query within a radius between two clouds of millions of points, and the standard reconstruction scores on top of it
(precision, recall and F-score at distance thresholds, mean accuracy and completeness).  The reference has no such program.

Three layers, as in cloud.py:
  * host statements in numpy (``scan_keys_numpy``, ``grid_numpy``, ``nearest_numpy``, ``compare_numpy`` and the all-pairs
    ``nearest_bruteforce`` that pins them): the host path (``device='cpu'``) and what the kernels are tested against, written
    element-wise in the kernels' operation order;
  * ``scan_keys_hip`` (csrc/td_scan.hip), ``grid_hip`` (torch.sort, td_cloud_heads, torch.cumsum: plumbing, no new kernel) and
    ``nearest_hip`` (csrc/td_nn.hip): device tensors only, a CPU tensor is an error;
  * ``ScanFuser`` (scans + poses -> cloud.Cloud) and ``CloudComparer`` (two clouds -> Comparison).

Scan keys (float64; every product, sum and quotient rounded on its own):
    cam_k   = ((Tr_k0 x + Tr_k1 y) + Tr_k2 z) + Tr_k3                       Tr: velodyne to camera, the odometry calib.txt's "Tr:"
    u = ((K00 cam_x + K01 cam_y) + K02 cam_z) / cam_z;  v likewise from row 1
    world_k = ((r_k0 cam_x + r_k1 cam_y) + r_k2 cam_z) + t_k                 [r | t]: the scan's camera-to-world pose
    key, q  = cloud.py's formula from world inv_voxel
    r = g = b = clamp(floor(float64(reflectance) 255.0 + 0.5), 0, 255), 0 for a NaN reflectance
A point is invalid by the first cause that holds: invalid_point (x, y or z not finite, or no scan owns the point), invalid_depth
(cam_z outside [min_depth, max_range]), invalid_view (a camera is given and not 0 <= u <= W-1 and 0 <= v <= H-1: without the view
test the lidar's 360 degrees count against the recall of a forward-looking camera), invalid_range (a voxel coordinate outside
[-2^20, 2^20), or the key is the sentinel).

Nearest neighbour within tau.  The reference is sorted into a uniform grid: cell = floor(x inv_cell) per axis, inv_cell = (1 - 2^-20) /
tau, packed with cloud.pack_key; points that are not finite or out of key range are left out and counted.  With that factor
|x - y| <= tau gives |fl(x c) - fl(y c)| < 1 for coordinates up to 2^20 cells, so two points within tau lie in cells at most one
apart on every axis and the 27 cells around a query hold every candidate: the search is exact.  Per candidate j:
    e = ref_j - query;  d2 = ((e_x e_x) + (e_y e_y)) + (e_z e_z);  candidate iff d2 <= tau2 = tau tau
The winner is the smallest d2, among equal d2 the lowest original reference index: it depends neither on the sort's order inside a
cell nor on the order the cells are visited.  A query that is not finite or out of range is invalid: d2 = +inf, index = -1.
"""
import collections
import ctypes

import numpy as np
import torch

from . import cloud, infer, native

HALF = cloud.HALF
INVALID_KEY = cloud.INVALID_KEY
SCAN_CAUSES = ("valid", "invalid_point", "invalid_depth", "invalid_view", "invalid_range")
MAX_THRESHOLDS = native.CONSTANTS["TD_NN_MAX_THRESHOLDS"]

# UNTUNED, like cloud.DEFAULT_VOXEL it is derived from: three voxels, in the clouds' units.  Nobody has scored a real cloud with it.
DEFAULT_TAU = 3 * cloud.DEFAULT_VOXEL
NOT_FOUND_RGB = (0, 255, 0)           # error_colors: a point with no neighbour within tau; pure green is not in the magma table

Grid = collections.namedtuple("Grid", "points order cell_key cell_start tau stats")
Grid.__doc__ = """A reference cloud sorted into cells: points float64 [M',3] in cell order, order int64 [M'] (the original index of every
sorted point), cell_key int64 [C] ascending, cell_start int64 [C+1], tau (the radius the cells were sized for), stats: dict of Python
ints: points (M), dropped (not finite or out of key range), cells (C), max_cell (the largest cell population: a query's work is at
most 27 max_cell candidates; for a voxel-averaged cloud about (tau / voxel + 1)^3)."""

Neighbours = collections.namedtuple("Neighbours", "d2 index counts")
Neighbours.__doc__ = """d2 float64 [N] (+inf: nothing within tau), index int64 [N] (-1 likewise), counts int64 [K+2]: queries with d2 <=
t_k^2 per threshold, queries that found a neighbour, invalid queries."""

Comparison = collections.namedtuple("Comparison", "thresholds precision recall fscore accuracy completeness pred ref stats")
Comparison.__doc__ = """thresholds, precision, recall, fscore: tuples of Python floats, one entry per threshold;  accuracy, completeness:
the mean of min(sqrt(d2), tau) over the predicted / the reference points (no neighbour counts as tau);  pred, ref: the Neighbours of
the predicted points in the reference and of the reference points in the predicted cloud;  stats: dict with n_pred, n_ref and the
two grids' statistics (pred_grid, ref_grid)."""


def inv_cell(tau):
    """(1 - 2^-20) / tau in float64: the two operations td_nn_query performs on the host."""
    tau = float(tau)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("tau: a positive radius, got %r" % (tau,))
    return (1.0 - 2.0 ** -20) / tau


def _thresholds(tau, thresholds):
    """-> (thresholds as floats, their squares): at most 16, ascending, inside [0, tau]; None: (tau/4, tau/2, tau)."""
    tau = float(tau)
    t = (tau / 4, tau / 2, tau) if thresholds is None else tuple(float(v) for v in thresholds)
    if len(t) > MAX_THRESHOLDS or any(not 0 <= v <= tau for v in t) or any(b < a for a, b in zip(t, t[1:])):
        raise ValueError("thresholds: at most %d ascending values in [0, tau = %r], got %r" % (MAX_THRESHOLDS, tau, t))
    return t, [v * v for v in t]


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _check_scans(Tr, K, height, width, inv_voxel, min_depth, max_range):
    Tr = np.ascontiguousarray(np.asarray(Tr, dtype=np.float64).reshape(-1))
    if Tr.shape != (12,):
        raise ValueError("Tr: 3x4 velodyne to camera, got %s" % (np.shape(Tr),))
    height, width = int(height), int(width)
    if height < 0 or width < 0 or (height > 0 and (K is None or width < 1)):
        raise ValueError("the view test needs K, height >= 1 and width >= 1; height = 0 turns it off; got %r x %r" % (height, width))
    K9 = cloud._inv_K9(K, "K") if height > 0 else None
    if not inv_voxel > 0 or not min_depth <= max_range:
        raise ValueError("inv_voxel > 0 and min_depth <= max_range; got %r, %r, %r" % (inv_voxel, min_depth, max_range))
    return Tr, K9, height, width


def scan_keys_numpy(points, offsets, Tr, poses, K=None, height=0, width=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                    max_range=cloud.DEFAULT_MAX_RANGE, inv_voxel=1.0 / cloud.DEFAULT_VOXEL):
    """points float32 [n,4], offsets int64 [S+1] (non-decreasing), Tr 3x4, poses float64 [S,3,4], K 3x3 or None -> (key int64 [n],
    payload uint64 [n], counts int64 [5] in the order of SCAN_CAUSES).  The statement td_scan_keys is tested against."""
    pts = np.ascontiguousarray(points, dtype=np.float32)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    P = np.ascontiguousarray(poses, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 4 or off.ndim != 1 or len(off) < 2 or P.shape != (len(off) - 1, 3, 4):
        raise ValueError("points [n,4], offsets [S+1] with S >= 1, poses [S,3,4]; got %s, %s, %s" % (pts.shape, off.shape, P.shape))
    if np.any(np.diff(off) < 0):
        raise ValueError("offsets run backwards")
    Tr, K9, H, W = _check_scans(Tr, K, height, width, inv_voxel, min_depth, max_range)
    n, S = len(pts), len(off) - 1
    i = np.arange(n, dtype=np.int64)
    s = np.searchsorted(off, i, side="right") - 1
    sc = np.clip(s, 0, S - 1)
    owned = (s >= 0) & (s < S) & (off[sc] <= i) & (i < off[sc + 1])
    cause = np.zeros(n, np.int8)

    def mark(mask, code):
        cause[(cause == 0) & mask] = code

    inv_voxel = np.float64(inv_voxel)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mark(~owned | ~np.isfinite(pts[:, 0]) | ~np.isfinite(pts[:, 1]) | ~np.isfinite(pts[:, 2]), 1)
        x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
        cx, cy, cz = (((Tr[4 * k] * x + Tr[4 * k + 1] * y) + Tr[4 * k + 2] * z) + Tr[4 * k + 3] for k in range(3))
        mark(~((cz >= np.float64(min_depth)) & (cz <= np.float64(max_range))), 2)
        if H > 0:
            u = ((K9[0] * cx + K9[1] * cy) + K9[2] * cz) / cz
            v = ((K9[3] * cx + K9[4] * cy) + K9[5] * cz) / cz
            mark(~((u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)), 3)                       # a NaN fails
        g = []
        for k in range(3):
            r0, r1, r2, t = (P[sc, k, j] for j in range(4))
            g.append((((r0 * cx + r1 * cy) + r2 * cz) + t) * inv_voxel)
        grey = np.floor(pts[:, 3].astype(np.float64) * 255.0 + 0.5)
        grey = np.where(grey >= 0, np.minimum(grey, 255.0), 0.0).astype(np.uint64)              # a NaN reflectance is 0
    key, _, payload = cloud.grid_keys_numpy(g)
    mark(key == INVALID_KEY, 4)
    ok = cause == 0
    payload = payload | (grey << np.uint64(30)) | (grey << np.uint64(38)) | (grey << np.uint64(46))
    key = np.where(ok, key, INVALID_KEY).astype(np.int64)
    payload = np.where(ok, payload, np.uint64(0)).astype(np.uint64)
    return key, payload, np.bincount(cause, minlength=5).astype(np.int64)


def _cells_numpy(x, ic):
    """float64 [M,3] -> (cell key int64 [M], ok bool [M]): cloud.grid_keys_numpy of x inv_cell.  ok: x is finite and in the key range
    (an inf times inv_cell stays an inf and fails the range test); the key is INVALID_KEY where not ok and in the corner cell."""
    with np.errstate(invalid="ignore", over="ignore"):
        key, ok, _ = cloud.grid_keys_numpy((x * np.float64(ic)).T)
    return key, ok


def _xyz64(a, name):
    a = np.ascontiguousarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: [n,3], got %s" % (name, a.shape))
    return a


def grid_numpy(ref, tau):
    """ref float64 [M,3] -> Grid of numpy arrays."""
    x = _xyz64(ref, "ref")
    key, _ = _cells_numpy(x, inv_cell(tau))
    kept = np.nonzero(key != INVALID_KEY)[0]                 # the one corner cell whose key is the sentinel holds nothing
    order = kept[np.argsort(key[kept], kind="stable")]
    cell_key, starts, sizes = np.unique(key[order], return_index=True, return_counts=True)
    cell_start = np.concatenate([starts, [len(order)]]).astype(np.int64)
    stats = {"points": len(x), "dropped": len(x) - len(order), "cells": len(cell_key), "max_cell": int(sizes.max()) if len(sizes) else 0}
    return Grid(np.ascontiguousarray(x[order]), order.astype(np.int64), cell_key.astype(np.int64), cell_start, float(tau), stats)


def _counts(d2, index, valid, thr2):
    return np.array([int(np.count_nonzero(d2 <= t)) for t in thr2] + [int(np.count_nonzero(index >= 0)), int(np.count_nonzero(~valid))],
                    np.int64)


def walk_numpy(grid, key):
    """The walk of td_nn_query and td_cloud_normals (over csrc/td_grid.h's pieces) for all queries at once.  key int64 [n]: the cells of the valid queries -> yields (queries, rows):
    indices into ``key`` and the rows of ``grid.points`` they visit, per (dx, dy) column (one lower and one upper bound over its at
    most three z-cells) and per rank inside the column; every query at most once per yield."""
    ix, iy, iz = cloud.unpack_key(key)
    z0, z1 = np.maximum(iz - 1, -HALF), np.minimum(iz + 1, HALF - 1)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            cx, cy = ix + dx, iy + dy
            inside = (cx >= -HALF) & (cx < HALF) & (cy >= -HALF) & (cy < HALF)
            cx, cy = np.where(inside, cx, 0), np.where(inside, cy, 0)
            p0 = grid.cell_start[np.searchsorted(grid.cell_key, cloud._pack(cx, cy, z0), side="left")]
            p1 = grid.cell_start[np.searchsorted(grid.cell_key, cloud._pack(cx, cy, z1), side="right")]
            p1 = np.where(inside, p1, p0)
            act, rank = np.nonzero(p1 > p0)[0], 0
            while len(act):
                yield act, p0[act] + rank
                rank += 1
                act = act[p0[act] + rank < p1[act]]


def nearest_numpy(query, ref, tau, thresholds=None):
    """query float64 [N,3], ref float64 [M,3] (or a Grid of grid_numpy at the same tau) -> Neighbours.  The statement td_nn_query is
    tested against: walk_numpy's candidates."""
    q = _xyz64(query, "query")
    grid = ref if isinstance(ref, Grid) else grid_numpy(ref, tau)
    if grid.tau != float(tau):
        raise ValueError("the grid was built for tau = %r, asked %r" % (grid.tau, tau))
    _, thr2 = _thresholds(tau, thresholds)
    tau2 = float(tau) * float(tau)
    key, valid = _cells_numpy(q, inv_cell(tau))
    N = len(q)
    best, best_index = np.full(N, np.inf), np.full(N, -1, np.int64)
    who = np.nonzero(valid)[0]
    if len(who) and len(grid.order):
        for act, p in walk_numpy(grid, key[who]):
            qi = who[act]
            e = grid.points[p] - q[qi]
            d2 = ((e[:, 0] * e[:, 0]) + (e[:, 1] * e[:, 1])) + (e[:, 2] * e[:, 2])
            j = grid.order[p]
            take = (d2 <= tau2) & ((d2 < best[qi]) | ((d2 == best[qi]) & (j < best_index[qi])))
            best[qi[take]], best_index[qi[take]] = d2[take], j[take]
    return Neighbours(best, best_index, _counts(best, best_index, valid, thr2))


def nearest_bruteforce(query, ref, tau, thresholds=None, chunk=256):
    """nearest_numpy over all pairs, with no grid: for the tests.  Reference points that are not finite are no candidates (points
    out of key range are not looked for: the tests keep the reference inside)."""
    q, x = _xyz64(query, "query"), _xyz64(ref, "ref")
    _, thr2 = _thresholds(tau, thresholds)
    tau2 = float(tau) * float(tau)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(q * np.float64(inv_cell(tau)))
        valid = np.isfinite(q).all(1) & ((f >= -float(HALF)) & (f < float(HALF))).all(1)
    best, best_index = np.full(len(q), np.inf), np.full(len(q), -1, np.int64)
    usable = np.isfinite(x).all(1)
    for at in range(0, len(q), chunk):
        rows = np.nonzero(valid[at:at + chunk])[0] + at
        if not len(rows) or not len(x):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            e = x[None, :, :] - q[rows, None, :]
            d2 = ((e[..., 0] * e[..., 0]) + (e[..., 1] * e[..., 1])) + (e[..., 2] * e[..., 2])
            d2 = np.where(usable[None, :] & (d2 <= tau2), d2, np.inf)
        j = np.argmin(d2, axis=1)                          # the first of equal minima: the lowest index
        found = np.isfinite(d2[np.arange(len(rows)), j])
        best[rows[found]], best_index[rows[found]] = d2[np.arange(len(rows)), j][found], j[found]
    return Neighbours(best, best_index, _counts(best, best_index, valid, thr2))


def _scores(tau, thresholds, pred, ref, n_pred, n_ref, accuracy, completeness, stats):
    K = len(thresholds)
    precision = tuple(int(pred.counts[k]) / n_pred if n_pred else 0.0 for k in range(K))
    recall = tuple(int(ref.counts[k]) / n_ref if n_ref else 0.0 for k in range(K))
    fscore = tuple(2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    return Comparison(tuple(thresholds), precision, recall, fscore, float(accuracy), float(completeness), pred, ref, stats)


def compare_numpy(pred_xyz, ref_xyz, tau=DEFAULT_TAU, thresholds=None, pred_scale=1.0):
    """The statement of CloudComparer.compare: both directions through nearest_numpy -> Comparison of numpy arrays."""
    thresholds, _ = _thresholds(tau, thresholds)
    p = _xyz64(pred_xyz, "pred_xyz") * np.float64(pred_scale)
    r = _xyz64(ref_xyz, "ref_xyz")
    pred_grid, ref_grid = grid_numpy(p, tau), grid_numpy(r, tau)
    pred, ref = nearest_numpy(p, ref_grid, tau, thresholds), nearest_numpy(r, pred_grid, tau, thresholds)
    mean = lambda d2: float(np.minimum(np.sqrt(d2), float(tau)).mean()) if len(d2) else 0.0
    stats = {"n_pred": len(p), "n_ref": len(r), "pred_grid": pred_grid.stats, "ref_grid": ref_grid.stats}
    return _scores(tau, thresholds, pred, ref, len(p), len(r), mean(pred.d2), mean(ref.d2), stats)


def error_colors(d2, index, tau, lut=None):
    """d2 float64 [N], index int64 [N] -> uint8 [N,3]: the magma table at round(255 min(sqrt(d2), tau) / tau); NOT_FOUND_RGB where
    index is -1 (nothing within tau)."""
    lut = infer.magma_lut() if lut is None else lut
    d2, index = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in (d2, index))
    with np.errstate(invalid="ignore"):
        t = np.minimum(np.sqrt(np.where(index >= 0, d2, 0.0)), float(tau)) / float(tau)
    rgb = lut[np.clip(np.floor(t * 255.0 + 0.5), 0, 255).astype(np.int64)].astype(np.uint8)
    rgb[index < 0] = NOT_FOUND_RGB
    return rgb


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def scan_keys_hip(points, offsets, Tr, poses, K=None, height=0, width=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                  max_range=cloud.DEFAULT_MAX_RANGE, inv_voxel=1.0 / cloud.DEFAULT_VOXEL, stats=None):
    """scan_keys_numpy as one launch of td_scan_keys -> (key int64 [n], payload int64 [n]: the uint64's bits).  points, offsets and
    poses on one HIP device; Tr and K are host arrays.  ``stats``: an int64 [5] device tensor that the launch increments (the order
    of SCAN_CAUSES), or None.  Nothing is read back: offsets that run backwards leave the points nobody owns invalid_point."""
    native.require_device(points, offsets, poses)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4 or offsets.dtype != torch.int64 or offsets.dim() != 1 \
            or offsets.shape[0] < 2 or poses.dtype != torch.float64 or tuple(poses.shape) != (offsets.shape[0] - 1, 3, 4):
        raise ValueError("points float32 [n,4], offsets int64 [S+1] with S >= 1, poses float64 [S,3,4]; got %s %s, %s %s, %s %s" % (
            tuple(points.shape), points.dtype, tuple(offsets.shape), offsets.dtype, tuple(poses.shape), poses.dtype))
    Tr, K9, H, W = _check_scans(Tr, K, height, width, inv_voxel, min_depth, max_range)
    if stats is not None:
        stats = cloud._i64(stats, "stats", 5)
    n = points.shape[0]
    key = torch.empty(n, dtype=torch.int64, device=points.device)
    payload = torch.empty(n, dtype=torch.int64, device=points.device)
    if n == 0:                           # an empty tensor has no pointer to pass
        return key, payload
    native.call("td_scan_keys", points.contiguous(), n, offsets.contiguous(), offsets.shape[0] - 1, (ctypes.c_double * 12)(*Tr),
                poses.contiguous(), None if K9 is None else (ctypes.c_double * 9)(*K9), H, W, float(min_depth), float(max_range),
                float(inv_voxel), key, payload, stats)
    return key, payload


def _f64_points(t, name):
    native.require_device(t)
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s: float64 [n,3], got %s %s" % (name, tuple(t.shape), t.dtype))
    return t.contiguous()


def grid_hip(ref, tau):
    """grid_numpy on the device -> Grid of device tensors: one elementwise product and floor, torch.sort on the keys, td_cloud_heads,
    torch.cumsum.  ONE host synchronisation (M', C and max_cell size the outputs and fill the statistics)."""
    x = _f64_points(ref, "ref")
    ic = inv_cell(tau)
    M, dev = x.shape[0], x.device
    if M == 0:
        empty = torch.zeros(0, dtype=torch.int64, device=dev)
        return Grid(x, empty, empty, torch.zeros(1, dtype=torch.int64, device=dev), float(tau),
                    {"points": 0, "dropped": 0, "cells": 0, "max_cell": 0})
    f = torch.floor(x * ic)
    ok = torch.isfinite(x).all(1) & ((f >= -float(HALF)) & (f < float(HALF))).all(1)
    c = torch.where(ok[:, None], f, torch.zeros_like(f)).to(torch.int64)
    key = cloud._pack(c[:, 0], c[:, 1], c[:, 2])
    key = torch.where(ok, key, torch.full_like(key, INVALID_KEY))         # the corner cell's key is the sentinel already
    sorted_keys, perm = torch.sort(key)
    heads = cloud.heads_hip(sorted_keys)
    starts = torch.nonzero(heads).reshape(-1)
    kept = (sorted_keys != INVALID_KEY).sum()
    cell_start = torch.cat([starts, kept.reshape(1)])
    sizes = cell_start[1:] - cell_start[:-1]
    largest = sizes.max() if starts.shape[0] else kept.new_zeros(())          # starts.shape: nonzero has synchronised already
    Mk, max_cell = (int(v) for v in torch.stack([kept, largest]).tolist())
    order = perm[:Mk].contiguous()
    stats = {"points": M, "dropped": M - Mk, "cells": int(starts.shape[0]), "max_cell": max_cell}
    return Grid(x[order].contiguous(), order, sorted_keys[starts].contiguous(), cell_start.contiguous(), float(tau), stats)


def nearest_hip(query, grid, tau, thresholds=None, counts=None):
    """nearest_numpy as one launch of td_nn_query -> Neighbours of device tensors.  ``grid``: grid_hip's, built for the same tau.
    ``counts``: an int64 [K+2] device tensor that the launch increments, or None for a fresh one.  No synchronisation."""
    q = _f64_points(query, "query")
    if not isinstance(grid, Grid) or grid.tau != float(tau):
        raise ValueError("grid: a Grid of grid_hip built for tau = %r" % (tau,))
    _, thr2 = _thresholds(tau, thresholds)
    K, N, dev = len(thr2), q.shape[0], q.device
    points = _f64_points(grid.points, "grid.points")
    M = points.shape[0]
    order, cell_key = cloud._i64(grid.order, "grid.order", M), cloud._i64(grid.cell_key, "grid.cell_key")
    C = cell_key.shape[0]
    cell_start = cloud._i64(grid.cell_start, "grid.cell_start", C + 1)
    counts = torch.zeros(K + 2, dtype=torch.int64, device=dev) if counts is None else cloud._i64(counts, "counts", K + 2)
    d2 = torch.empty(N, dtype=torch.float64, device=dev)
    index = torch.empty(N, dtype=torch.int64, device=dev)
    if N == 0:                           # an empty tensor has no pointer to pass
        return Neighbours(d2, index, counts)
    native.call("td_nn_query", q, N, points if M else None, order if M else None, M, cell_key if C else None, cell_start, C, float(tau),
                (ctypes.c_double * max(K, 1))(*thr2), K, d2, index, counts)
    return Neighbours(d2, index, counts)


# ---------------------------------------------------------------------------------------------------------------------------

class ScanFuser:
    """fuse(scans, poses) -> cloud.Cloud: the lidar scans of a sequence as one voxel-averaged cloud in the world frame of ``poses``,
    grey by reflectance.

    device      'cuda[:i]': per batch of ``batch_size`` scans one upload of the concatenated points, scan_keys_hip, then the unchanged
                cloud.table_hip / merge_hip into the running key-sorted map and finish_hip; 'cpu': the numpy statements.  The cloud
                does not depend on ``batch_size`` and equals the host path bit for bit.
    voxel, min_depth, max_range  in the scans' units (metres for KITTI); the defaults of the last two are cloud.py's, UNTUNED
    Tr          3x4 velodyne to camera (velodyne.read_calib_file(calib.txt)["Tr"])
    K, height, width  the camera whose view the points must lie in (K: the 3x3 block in pixels); height = 0: no view test
    The stats carry points, the SCAN_CAUSES and voxels."""

    def __init__(self, device, voxel, Tr, K=None, height=0, width=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                 max_range=cloud.DEFAULT_MAX_RANGE, batch_size=12):
        if not (np.isfinite(voxel) and voxel > 0) or int(batch_size) < 1:
            raise ValueError("voxel: a positive size, batch_size >= 1; got %r, %r" % (voxel, batch_size))
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        self.voxel, self.batch_size = float(voxel), int(batch_size)
        self.Tr, _, height, width = _check_scans(Tr, K, height, width, 1.0 / self.voxel, min_depth, max_range)
        self.params = dict(K=None if height == 0 else np.array(cloud._inv_K9(K, "K")).reshape(3, 3), height=height, width=width,
                           min_depth=float(min_depth), max_range=float(max_range), inv_voxel=1.0 / self.voxel)

    def fuse(self, scans, poses):
        scans = [np.ascontiguousarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1, 4) for s in scans]
        P = np.ascontiguousarray(np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, dtype=np.float64))
        if P.ndim != 3 or P.shape[0] != len(scans) or P.shape[1:] not in ((3, 4), (4, 4)) or not len(scans):
            raise ValueError("poses: [%d,3,4] camera-to-world, one per scan, at least one scan; got %s" % (len(scans), P.shape))
        P = np.ascontiguousarray(P[:, :3])

        def batch(at, size):
            part = scans[at:at + size]
            offsets = np.zeros(len(part) + 1, np.int64)
            np.cumsum([len(s) for s in part], out=offsets[1:])
            return np.concatenate(part, 0), offsets, np.ascontiguousarray(P[at:at + len(part)])

        if not self.on_hip:
            points, offsets, _ = batch(0, len(scans))          # all scans at once: the statement
            key, payload, counts = scan_keys_numpy(points, offsets, self.Tr, P, **self.params)
            keys, sums = cloud.voxel_table_numpy(key, payload)
            xyz, rgb, count, _ = cloud.finish_numpy(keys, sums, self.voxel)
            return cloud.Cloud(xyz, rgb, count, keys, self._stats(counts, len(keys)))
        vmap = cloud.VoxelMap(self.device, len(SCAN_CAUSES))
        for at in range(0, len(scans), self.batch_size):
            points, offsets, part = batch(at, self.batch_size)
            vmap.merge(*scan_keys_hip(torch.from_numpy(points).to(self.device), torch.from_numpy(offsets).to(self.device), self.Tr,
                                      torch.from_numpy(part).to(self.device), stats=vmap.counts, **self.params))
        xyz, rgb, count, _ = cloud.finish_hip(vmap.keys, vmap.sums, self.voxel)
        return cloud.Cloud(xyz, rgb, count, vmap.keys, self._stats(vmap.counts.cpu().numpy(), vmap.keys.shape[0]))

    @staticmethod
    def _stats(counts, voxels):
        out = {"points": int(np.sum(counts))}
        out.update({name: int(v) for name, v in zip(SCAN_CAUSES, counts)})
        out["voxels"] = int(voxels)
        return out


class CloudComparer:
    """compare(pred_xyz, ref_xyz, pred_scale=1.0) -> Comparison: the nearest-neighbour query in both directions (predicted points into
    the reference's grid, reference points into the predicted cloud's) and the scores on top of it.

    device      'cuda[:i]': grid_hip and nearest_hip; the clouds may be numpy arrays or tensors anywhere, they are converted to
                float64 on the device and the predicted one is multiplied by ``pred_scale`` there, the only alignment there is
                (no registration, no scale estimation); the Comparison's arrays are device tensors.  'cpu': compare_numpy.
    tau         the search radius and the cap of accuracy / completeness, in the clouds' units; DEFAULT_TAU is UNTUNED
    thresholds  at most 16 ascending distances inside [0, tau]; None: (tau/4, tau/2, tau), UNTUNED as well
    The counters are integers and equal the host path's exactly, hence the ratios; the two means are float64 sums in an order torch
    chooses and agree with numpy's to rounding."""

    def __init__(self, device, tau=DEFAULT_TAU, thresholds=None):
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        self.tau = float(tau)
        inv_cell(self.tau)
        self.thresholds, _ = _thresholds(self.tau, thresholds)

    def compare(self, pred_xyz, ref_xyz, pred_scale=1.0):
        if not self.on_hip:
            return compare_numpy(pred_xyz, ref_xyz, self.tau, self.thresholds, pred_scale)
        p = torch.as_tensor(pred_xyz).to(self.device, torch.float64) * float(pred_scale)
        r = torch.as_tensor(ref_xyz).to(self.device, torch.float64)
        pred_grid, ref_grid = grid_hip(p, self.tau), grid_hip(r, self.tau)
        pred = nearest_hip(p, ref_grid, self.tau, self.thresholds)
        ref = nearest_hip(r, pred_grid, self.tau, self.thresholds)
        mean = lambda d2: float(torch.clamp(torch.sqrt(d2), max=self.tau).mean().item()) if d2.shape[0] else 0.0
        stats = {"n_pred": p.shape[0], "n_ref": r.shape[0], "pred_grid": pred_grid.stats, "ref_grid": ref_grid.stats}
        host = lambda nb: Neighbours(nb.d2, nb.index, nb.counts.cpu().numpy())
        return _scores(self.tau, self.thresholds, host(pred), host(ref), p.shape[0], r.shape[0], mean(pred.d2), mean(ref.d2), stats)
