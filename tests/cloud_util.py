"""Shared pieces of the point-cloud tests (test_cloud_cpu.py, test_hip_cloud.py): synthetic scenes that exercise every way a pixel
can be invalid, and a brute-force per-point fusion in plain Python floats and a dict, which is what pins the numpy statements.

All comparisons in those tests are exact (np.array_equal): every quantity is an integer or a fixed sequence of individually rounded
IEEE float64 operations, and Python's float arithmetic is the same IEEE arithmetic taken one operation at a time."""
import math

import numpy as np

VOXEL = 2.0          # coarse against the pixel spacing of the tiny test images: voxels hold several points
PARAMS = dict(stride=1, border=0, min_depth=0.5, max_range=40.0, edge=0.0, depth_scale=1.0, pose_scale=1.0)


def intrinsics(h, w):
    """KITTI's normalised intrinsics at h x w -> (K float32 [4,4], inv_K float64 [3,3] of the widened 3x3 block)."""
    K = np.array([[0.58 * w, 0, 0.5 * w, 0], [0, 1.92 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    return K, np.linalg.inv(K[:3, :3].astype(np.float64))


def _rotation(v):
    angle = float(np.linalg.norm(v))
    k = v / max(angle, 1e-300)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def scene(seed, B, H, W, special=True, far=True):
    """(depth float32 [B,H,W], color uint8 [B,3,H,W], poses float64 [B,3,4], inv_K).  A smooth depth of 2 ... 12 with a step edge down
    the middle; with ``special`` a sprinkle of NaN, inf, -inf, 0, negative, too-near and too-far depths; rotated poses whose
    translations put points at negative coordinates and, with ``far``, the last frame beyond +-2^20 voxels of VOXEL."""
    g = np.random.default_rng(seed)
    y, x = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    depth = np.empty((B, H, W), np.float32)
    for b in range(B):
        f = 6.0 + 3.0 * np.sin(3.0 * x + b) + 2.0 * np.cos(2.0 * y - b) + 0.05 * g.standard_normal((H, W))
        f[:, W // 2:] += 4.0                                            # the step edge
        depth[b] = f
    if special:
        flat = depth.reshape(-1)
        pick = g.choice(flat.size, size=max(7, flat.size // 12), replace=False)
        values = np.array([np.nan, np.inf, -np.inf, 0.0, -3.0, 0.01, 1e6], np.float32)
        flat[pick] = values[np.arange(len(pick)) % len(values)]
    color = g.integers(0, 256, (B, 3, H, W), dtype=np.uint8)
    poses = np.zeros((B, 3, 4))
    for b in range(B):
        poses[b, :, :3] = _rotation(g.uniform(-0.6, 0.6, 3))
        poses[b, :, 3] = g.uniform(-6.0, 2.0, 3)
    if far and B > 1:
        poses[-1, :, 3] = [3.0e6, -3.0e6, 1.0]                          # 2^20 voxels of 2.0 = 2 097 152
    return depth, color, poses, intrinsics(H, W)[1]


def brute_force(depth, color, poses, inv_K, voxel, stride, border, min_depth, max_range, edge, depth_scale, pose_scale, min_count=1):
    """The fusion one point at a time: Python floats (IEEE float64, one rounding per operation), float32 only where the filter
    compares depths, a dict from (ix, iy, iz) to integer sums.  -> (keys, sums [V,7], xyz, rgb, count, counts-by-cause)."""
    B, H, W = depth.shape
    m = [float(v) for v in np.asarray(inv_K, np.float64).reshape(-1)]
    inv_voxel = 1.0 / float(voxel)
    table, causes = {}, [0] * 6
    half = 1 << 20
    for b in range(B):
        P = [[float(v) for v in row] for row in poses[b]]
        for y in range(H):
            for x in range(W):
                d32 = depth[b, y, x]
                ds = float(d32) * float(depth_scale)
                if x % stride or y % stride:
                    causes[1] += 1
                    continue
                if x < border or x >= W - border or y < border or y >= H - border:
                    causes[2] += 1
                    continue
                if not math.isfinite(float(d32)) or not (min_depth <= ds <= max_range):
                    causes[3] += 1
                    continue
                if edge > 0:
                    bad = False
                    for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                        if 0 <= yy < H and 0 <= xx < W:
                            nb = depth[b, yy, xx]
                            if not math.isfinite(float(nb)) or np.float32(abs(np.float32(d32 - nb))) > np.float32(edge) * min(d32, nb):
                                bad = True
                    if bad:
                        causes[4] += 1
                        continue
                u, v = float(x), float(y)
                ray = [(m[3 * k] * u + m[3 * k + 1] * v) + m[3 * k + 2] for k in range(3)]
                p = [ds * r for r in ray]
                world = [((P[k][0] * p[0] + P[k][1] * p[1]) + P[k][2] * p[2]) + float(pose_scale) * P[k][3] for k in range(3)]
                gg = [wv * inv_voxel for wv in world]
                if not all(math.isfinite(t) and -half <= math.floor(t) < half for t in gg):
                    causes[5] += 1
                    continue
                i = tuple(int(math.floor(t)) for t in gg)
                if i == (half - 1,) * 3:
                    causes[5] += 1
                    continue
                q = [min(1023, int(math.floor((t - float(c)) * 1024.0))) for t, c in zip(gg, i)]
                row = table.setdefault(i, [0] * 7)
                for j, t in enumerate([1] + q + [int(color[b, ch, y, x]) for ch in range(3)]):
                    row[j] += t
                causes[0] += 1
    cells = sorted(table)                                               # (ix, iy, iz) order = key order
    keys = np.array([((c[0] + half) << 42) | ((c[1] + half) << 21) | (c[2] + half) for c in cells], np.int64).reshape(-1)
    sums = np.array([table[c] for c in cells], np.int64).reshape(-1, 7)
    xyz = np.array([[np.float32((float(c[k]) + (float(table[c][1 + k]) / float(table[c][0]) + 0.5) / 1024.0) * float(voxel))
                     for k in range(3)] for c in cells], np.float32).reshape(-1, 3)
    rgb = np.array([[(2 * table[c][4 + k] + table[c][0]) // (2 * table[c][0]) for k in range(3)] for c in cells], np.uint8).reshape(-1, 3)
    count = sums[:, 0].astype(np.int32)
    keep = sums[:, 0] >= min_count
    return keys[keep], sums[keep], xyz[keep], rgb[keep], count[keep], causes


def assert_clouds_equal(a, b):
    """Two Clouds (numpy arrays, or tensors brought to the host) are the same bits."""
    def host(t):
        return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    assert np.array_equal(host(a.keys), host(b.keys))
    assert np.array_equal(host(a.xyz).view(np.uint32), host(b.xyz).view(np.uint32))
    assert np.array_equal(host(a.rgb), host(b.rgb))
    assert np.array_equal(host(a.count), host(b.count))
    assert a.stats == b.stats, (a.stats, b.stats)
