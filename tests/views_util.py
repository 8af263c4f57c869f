"""Shared pieces of the multi-view filter's tests (test_views_cpu.py, test_hip_views.py): sequences whose frames overlap, a scene
with an analytic truth (a plane seen by a moving camera), and the vote count one pixel at a time in plain Python floats, which is
what pins cloud.views_numpy.

All comparisons in those tests are exact (np.array_equal): a vote is a comparison of a fixed sequence of individually rounded IEEE
float64 operations, and Python's float arithmetic is the same IEEE arithmetic taken one operation at a time."""
import math

import numpy as np

from tests import cloud_util

RANGE = dict(min_depth=0.5, max_range=40.0)


def K_pair(h, w):
    """(K float64 [3,3], inv_K float64 [3,3]) of cloud_util.intrinsics."""
    K, inv_K = cloud_util.intrinsics(h, w)
    return K[:3, :3].astype(np.float64), inv_K


def poses_of(g, N, step, angle=0.02, jitter=0.05):
    """float64 [N,3,4] camera-to-world: ``step`` forward per frame, rotations of up to +-angle rad about every axis, lateral jitter."""
    poses = np.zeros((N, 3, 4))
    for b in range(N):
        poses[b, :, :3] = cloud_util._rotation(g.uniform(-angle, angle, 3))
        poses[b, :, 3] = [g.uniform(-jitter, jitter), g.uniform(-jitter, jitter), step * b]
    return poses


def scene(seed, N, H, W, special=True, angle=0.02, jitter=0.05):
    """(depth float32 [N,H,W], color uint8 [N,3,H,W], poses float64 [N,3,4], inv_K, K).  Every frame sees the same smooth surface of
    depth 7 ... 11 up to 1.5 % of noise and a 20 % step over a band of columns of every other frame, so that neighbours agree on some
    pixels and not on others; small rotations (up to ``angle``) and translations, so that the frames overlap (with no rotation and
    no jitter the pixel at the principal point projects onto itself: the way to a vote in a 2 x 2 frame); with ``special`` a
    sprinkle of NaN, inf, -inf, 0, negative, too-near and too-far depths, which make pixels and taps not ok."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = np.empty((N, H, W), np.float32)
    for b in range(N):
        f = (9.0 + 1.5 * np.sin(2.0 * x) + 0.5 * np.cos(3.0 * y)) * (1.0 + 0.015 * g.standard_normal((H, W)))
        if b % 2:
            f[:, W // 3:W // 2] *= 1.2
        depth[b] = f
    if special:
        flat = depth.reshape(-1)
        pick = g.choice(flat.size, size=max(7, flat.size // 12), replace=False)
        values = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0, 0.01, 1e6], np.float32)
        flat[pick] = values[np.arange(len(pick)) % len(values)]
    color = g.integers(0, 256, (N, 3, H, W), dtype=np.uint8)
    K, inv_K = K_pair(H, W)
    return depth, color, poses_of(g, N, 0.15, angle, jitter), inv_K, K


def plane_scene(N=11, H=24, W=40):
    """(depth float32 [N,H,W], poses, inv_K, K): the plane n.X = 12, n ~ (0.2, 0.1, 1), seen by a camera that moves 0.4 along z per
    frame with +-0.02 rad rotations and small lateral jitter.  The depth is the closed form d = (12 - n.t) / (n.(R ray)), cast to
    float32 (the ray's z component is 1, so the distance along the ray in units of it is the depth)."""
    g = np.random.default_rng(7)
    K, inv_K = K_pair(H, W)
    poses = poses_of(g, N, 0.4)
    n = np.array([0.2, 0.1, 1.0])
    n /= np.linalg.norm(n)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([inv_K[k, 0] * u + inv_K[k, 1] * v + inv_K[k, 2] for k in range(3)], -1)          # [H,W,3]
    depth = np.empty((N, H, W), np.float32)
    for b in range(N):
        depth[b] = (12.0 - n @ poses[b, :, 3]) / (rays @ (poses[b, :, :3].T @ n))
    return depth, poses, inv_K, K


def brute_force(depth, poses, inv_K, K, radius, tol, depth_scale=1.0, pose_scale=1.0, min_depth=0.5, max_range=40.0, centres=None,
                bounds=None):
    """The vote counts one pixel and one neighbour at a time: Python floats (IEEE float64, one rounding per operation) -> uint8
    [c1-c0,H,W].  Written from the statement in cloud.py's docstring, not from views_numpy."""
    N, H, W = depth.shape
    m = [float(t) for t in np.asarray(inv_K, np.float64).reshape(-1)]
    k = [float(t) for t in np.asarray(K, np.float64).reshape(-1)]
    depth_scale, pose_scale, tol = float(depth_scale), float(pose_scale), float(tol)
    lo, hi = (0, N) if bounds is None else bounds
    c0, c1 = (lo, hi) if centres is None else centres

    def scaled(f, y, x):
        """ds, or None where the depth is not ok"""
        d = float(depth[f, y, x])
        ds = d * depth_scale
        return ds if math.isfinite(d) and min_depth <= ds <= max_range else None

    votes = np.zeros((c1 - c0, H, W), np.uint8)
    for i in range(c0, c1):
        Pi = [[float(t) for t in row] for row in poses[i]]
        first = min(max(i - radius, lo), hi - 1 - 2 * radius)
        others = [j for j in range(first, first + 2 * radius + 1) if j != i]
        assert len(others) == 2 * radius and lo <= others[0] and others[-1] < hi
        for y in range(H):
            for x in range(W):
                ds = scaled(i, y, x)
                if ds is None:
                    continue
                u, v = float(x), float(y)
                p = [ds * ((m[3 * r] * u + m[3 * r + 1] * v) + m[3 * r + 2]) for r in range(3)]
                w = [((Pi[r][0] * p[0] + Pi[r][1] * p[1]) + Pi[r][2] * p[2]) + pose_scale * Pi[r][3] for r in range(3)]
                for j in others:
                    Pj = [[float(t) for t in row] for row in poses[j]]
                    e = [w[r] - pose_scale * Pj[r][3] for r in range(3)]
                    q = [(Pj[0][r] * e[0] + Pj[1][r] * e[1]) + Pj[2][r] * e[2] for r in range(3)]
                    z = q[2]
                    if not z > 0:
                        continue
                    uj = ((k[0] * q[0] + k[1] * q[1]) + k[2] * q[2]) / z
                    vj = ((k[3] * q[0] + k[4] * q[1]) + k[5] * q[2]) / z
                    if not (0 <= uj <= W - 1 and 0 <= vj <= H - 1):
                        continue
                    x0, y0 = min(math.floor(uj), W - 2), min(math.floor(vj), H - 2)
                    fx, fy = uj - float(x0), vj - float(y0)
                    taps = [scaled(j, y0, x0), scaled(j, y0, x0 + 1), scaled(j, y0 + 1, x0), scaled(j, y0 + 1, x0 + 1)]
                    if any(t is None for t in taps):
                        continue
                    top = taps[0] + fx * (taps[1] - taps[0])
                    bot = taps[2] + fx * (taps[3] - taps[2])
                    s = top + fy * (bot - top)
                    if abs(z - s) <= tol * min(z, s):
                        votes[i - c0, y, x] += 1
    return votes
