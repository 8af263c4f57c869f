"""Shared pieces of the odometry tests (test_odometry_cpu.py, test_odometry_vs_reference.py, test_hip_odometry.py).

Bounds.  Every float comparison of a kernel (or a host statement) against float64 numpy is within RTOL = 1e-9 relative (a trajectory:
relative to max(1, max |t|)).  Derived, not measured: float64 rounding over <= 4 540 compositions is n * 2^-53 ~ 5e-13 of the
largest entry, while a float32 slip anywhere (an inverse, a product or a sum taken in float32) shows at >= 1e-7.  arccos is
ill-conditioned at 0 and a segment end can flip when a cumulative distance sits on a threshold, so the inputs of the segment tests
must give every valid segment a rotation error above 1e-3 rad and keep every cumulative distance more than 1e-6 m away from every
dist[first] + len threshold: ``assert_conditions`` checks both on the host before anything is launched.
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-9


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "odometry.npz"))


def rel_err(a, b):
    """max |a - b| / |b| (0 where both are 0; NaN positions must coincide)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    if not ok.any():
        return 0.0
    d, s = np.abs(a[ok] - b[ok]), np.abs(b[ok])
    return float(np.max(np.where(d == 0, 0.0, d / np.where(s == 0, 1.0, s))))


def traj_err(a, b):
    """max |a - b| / max(1, max |t|) of two [m,3,4] trajectories."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b[:, :, 3]).max()))


def _rodrigues(v):
    angle = np.linalg.norm(v, axis=-1)[..., None, None]
    k = v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def smooth_relative(n, seed, speed=1.2, dtype=np.float32, bias=0.0, scale=1.0):
    """[n,4,4] smooth relative transforms: rotation <= 0.05 rad, translation <= 1.5.  ``bias`` adds a constant rotation about y per
    frame and ``scale`` scales the translation (a drifting monocular prediction of the same motion as bias = 0, scale = 1)."""
    g = np.random.default_rng(seed)
    k = np.arange(n)[:, None]
    f, ph = g.uniform(0.002, 0.02, (2, 3)), g.uniform(0, 6.28, (2, 3))
    v = 0.025 * np.sin(f[0] * k + ph[0]) * np.array([0.3, 1.0, 0.3]) + np.array([0.0, bias, 0.0])
    t = np.array([0.0, 0.0, -speed]) + 0.1 * np.sin(f[1] * k + ph[1])
    assert np.linalg.norm(v, axis=1).max() <= 0.05 + abs(bias) and np.abs(t).max() <= 1.5
    M = np.zeros((n, 4, 4))
    M[:, :3, :3], M[:, :3, 3], M[:, 3, 3] = _rodrigues(v), scale * t, 1.0
    return M.astype(dtype)


def assert_conditions(rows, dist, lengths, step):
    """See the module docstring.  rows: the host's valid rows [k,5]; dist: the host's cumulative distances."""
    if len(rows):
        r_min = float((rows[:, 1] * rows[:, 3]).min())
        assert r_min > 1e-3, "segment rotation error %.3e rad: arccos is ill-conditioned" % r_min
    gap = min(float(np.abs(dist - (dist[first] + length)).min()) for first in range(0, len(dist), step) for length in lengths)
    assert gap > 1e-6, "a cumulative distance lies %.3e m from a threshold" % gap


def make_sequence_tree(root, seq, n_frames, h=32, w=64, seed=0):
    """<root>/sequences/<seq>/image_0/%06d.png (smooth frames that shift a little from one to the next) and <root>/poses/<seq>.txt:
    1 m per frame with a 0.05 rad turn.  Returns the ground-truth poses [n_frames,3,4]."""
    from PIL import Image
    from tests.infer_util import smooth_image
    import tripled_amd  # noqa: F401
    from tripled_amd import odometry
    d = os.path.join(root, "sequences", "%02d" % seq, "image_0")
    os.makedirs(d)
    base = smooth_image(seed, h, w + 4 * n_frames)
    for i in range(n_frames):
        Image.fromarray(np.ascontiguousarray(base[:, 4 * i:4 * i + w])).save(os.path.join(d, "%06d.png" % i))
    gt = odometry.trajectory_numpy(smooth_relative(n_frames - 1, seed + 1, speed=1.0, dtype=np.float64, bias=0.05))
    os.makedirs(os.path.join(root, "poses"))
    np.savetxt(os.path.join(root, "poses", "%02d.txt" % seq), gt.reshape(-1, 12), fmt="%.12e")
    return odometry.load_kitti_poses(os.path.join(root, "poses", "%02d.txt" % seq))
