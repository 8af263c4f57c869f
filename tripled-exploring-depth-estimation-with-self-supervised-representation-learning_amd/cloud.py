"""Scene reconstruction: the predicted depth maps and camera poses of a sequence fused into one voxel-averaged coloured point cloud.

The model is a joint depth-and-pose network: its depth maps and its poses share one scale, so back-projecting every frame through
its own pose gives the scene's geometry.  A raw cloud grows with the number of frames (KITTI sequence 09 at 192 x 640 is 195 million
points); a voxel-fused one is bounded by the scene.  The reference has no such program (its only 3-D picture is draw_odometry.py's
bird's-eye trajectory).

The design is store, sort, then sum per destination (csrc/td_cloud.hip): a kernel stores a (voxel key, packed payload) pair per
pixel, torch.sort orders the keys, a kernel marks where a voxel's run starts, torch.cumsum numbers the runs and a segmented-sum
kernel adds every run into its voxel's row.  Everything that is accumulated is an integer (a count, 10-bit positions inside the
voxel, 8-bit colours), so the cloud is bit-identical from run to run, does not depend on how the sequence is cut into batches, and
equals the numpy statement below exactly.

Three layers, as in odometry.py:
  * host statements in numpy (``keys_numpy``, ``voxel_table_numpy``, ``finish_numpy``, ``fuse_numpy``, ``pack_key`` / ``unpack_key``,
    ``save_ply`` / ``load_ply``): the host path (``device='cpu'``) and what the kernels are tested against.  The arithmetic is written
    element-wise in the kernel's operation order: no ``@`` and no einsum, which BLAS may fuse;
  * ``keys_hip``, ``views_hip``, ``heads_hip``, ``reduce_hip``, ``finish_hip``, ``merge_hip`` (and ``table_hip`` / ``fuse_hip``, which
    chain them): device tensors only, a CPU tensor is an error; the kernels themselves never synchronise;
  * ``SequenceDriver`` (frames -> DepthPredictor + OdometryEvaluator.relative_poses / trajectory_hip -> a sink) and ``SceneFuser`` on it.

The exact arithmetic (float64; every product and sum rounded on its own; pixel (u, v) at integer coordinates like the reference's
Backproject, no half-pixel offset):
    ray_k   = (m_k0 u + m_k1 v) + m_k2                       m = the 3x3 block of inv_K
    p       = (depth depth_scale) ray
    world_k = ((r_k0 p_x + r_k1 p_y) + r_k2 p_z) + pose_scale t_k      [r | t] = the frame's camera-to-world pose
    g = world inv_voxel;  i = floor(g);  q = min(1023, int(floor((g - i) 1024.0)))
    key = ((i_x + 2^20) << 42) | ((i_y + 2^20) << 21) | (i_z + 2^20);  payload = q_x | q_y << 10 | q_z << 20 | r << 30 | g << 38 | b << 46
    voxel:  xyz = float32((i + (sum q / count + 0.5) / 1024.0) voxel);  rgb = (2 sum c + count) // (2 count)

The multi-view filter (``min_views`` > 0; ``views_numpy`` is its statement, csrc/td_views.hip its kernel) keeps a pixel only if enough
neighbouring frames, reprojected, see the same depth there: what single-frame filters cannot catch (moving objects, sky, scale drift
between frames, smeared boundaries) disagrees between views.  The neighbours of frame i are the 2 radius other frames of the window
a .. a + 2 radius, a = min(max(i - radius, lo), hi - 1 - 2 radius): shifted, not shortened, at the ends of the sequence.  Per pixel of
frame i and neighbour j, float64, every product, sum and quotient rounded on its own (R, t: a pose's rotation and translation; K's
3x3 block):
    ok_f   = isfinite(d_f) and min_depth <= ds_f <= max_range,   ds_f = float64(d_f) depth_scale
    p, w   = the camera point and the world point of the pixel, as above (p = ds_i ray, w = world)
    e_k    = w_k - pose_scale tj_k;   q_k = (Rj_0k e_0 + Rj_1k e_1) + Rj_2k e_2       (the transpose of Rj: the stated inverse)
    z = q_2;  X = (K00 q_0 + K01 q_1) + K02 q_2;  Y = (K10 q_0 + K11 q_1) + K12 q_2;  uj = X / z;  vj = Y / z
    inside = ok_i and z > 0 and 0 <= uj <= W-1 and 0 <= vj <= H-1                     (a NaN fails)
    x0 = min(floor(uj), W-2);  y0 = min(floor(vj), H-2);  fx = uj - x0;  fy = vj - y0
    t00, t01, t10, t11 = ds_j at (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1);  all four must be ok_j
    top = t00 + fx (t01 - t00);  bot = t10 + fx (t11 - t10);  s = top + fy (bot - top)
    vote   = inside and the taps are ok and |z - s| <= tol min(z, s)
"""
import collections
import ctypes

import numpy as np
import torch

from . import infer, native, odometry

HALF = 1 << 20                       # voxel coordinates lie in [-2^20, 2^20)
INVALID_KEY = (1 << 63) - 1          # csrc/td_grid.h: TD_KEY_INVALID; the sort puts it last
CAUSES = ("valid", "invalid_stride", "invalid_border", "invalid_depth", "invalid_edge", "invalid_range")

# Starting values in the MODEL's units: the stereo baseline (0.54 m) is 0.015 of them and the evaluation multiplies depths by 36, so
# one unit is about 36 m for a stereo-trained checkpoint.  UNTUNED: nobody has looked at a cloud of a trained checkpoint with them.
DEFAULT_VOXEL = 0.005        # ~0.18 m
DEFAULT_MIN_DEPTH = 0.1      # the depth network's own lower limit (disp_to_depth)
DEFAULT_MAX_RANGE = 1.0      # ~36 m: monocular depth degrades with range
DEFAULT_EDGE = 0.1           # 10 % depth step to a 4-neighbour
DEFAULT_VIEW_RADIUS = 2      # the multi-view filter (off by default: min_views = 0) asks the 2 frames before and the 2 after; UNTUNED
DEFAULT_VIEW_TOL = 0.05      # 5 % of the smaller of the two depths; UNTUNED like the rest
MAX_VIEW_RADIUS = native.CONSTANTS["TD_VIEWS_MAX_RADIUS"]

Cloud = collections.namedtuple("Cloud", "xyz rgb count keys stats")
Cloud.__doc__ = """xyz float32 [V,3], rgb uint8 [V,3], count int32 [V] (points fused into the voxel, saturating), keys int64 [V] (ascending:
the output order is defined), on the fuser's device (numpy arrays on the host path);  stats: dict of Python ints: points (pixels
seen), valid, invalid_stride / _border / _depth / _edge / _range (by the first cause that holds), with min_views > 0 invalid_views
(pixels valid by all of those that too few neighbouring frames confirm; ``valid`` is what is left), voxels (before min_count),
voxels_dropped (by min_count)."""

PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("count", "<i4")])
_PLY_TYPES = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _pack(ix, iy, iz):
    """pack_key without its check, on int64 numpy arrays or tensors."""
    return ((ix + HALF) << 42) | ((iy + HALF) << 21) | (iz + HALF)


def pack_key(ix, iy, iz):
    """Voxel coordinates in [-2^20, 2^20) -> int64 key (ascending key order = x major, then y, then z)."""
    ix, iy, iz = (np.asarray(v, dtype=np.int64) for v in (ix, iy, iz))
    for v in (ix, iy, iz):
        if v.size and (v.min() < -HALF or v.max() >= HALF):
            raise ValueError("voxel coordinates: [-2^20, 2^20)")
    return _pack(ix, iy, iz)


def grid_keys_numpy(g):
    """g: the three float64 arrays of grid coordinates (world inv_voxel, or a point times inv_cell) -> (key int64, ok bool, offset
    uint64), csrc/td_grid.h's voxel_key: i = floor(g), ok where every i lies in [-2^20, 2^20) (a NaN fails both
    comparisons), key = INVALID_KEY where not ok and for the one corner voxel whose key is the sentinel, offset = q_x | q_y << 10 |
    q_z << 20 with q = min(1023, int(floor((g - i) 1024.0))), 0 where the key is invalid."""
    with np.errstate(invalid="ignore", over="ignore"):
        f = [np.floor(v) for v in g]
        ok = np.ones(np.shape(f[0]), bool)
        for v in f:
            ok &= (v >= -float(HALF)) & (v < float(HALF))
        key = np.where(ok, _pack(*(np.where(ok, v, 0.0).astype(np.int64) for v in f)), INVALID_KEY).astype(np.int64)
        q = [np.minimum(1023, np.where(key != INVALID_KEY, np.floor((v - i) * 1024.0), 0.0).astype(np.int64)).astype(np.uint64)
             for v, i in zip(g, f)]
    return key, ok, q[0] | (q[1] << np.uint64(10)) | (q[2] << np.uint64(20))


def unpack_key(key):
    """int64 keys -> (ix, iy, iz) int64."""
    key = np.asarray(key, dtype=np.int64)
    mask = 2 * HALF - 1
    return ((key >> 42) & mask) - HALF, ((key >> 21) & mask) - HALF, (key & mask) - HALF


def unpack_payload(payload):
    """uint64 payloads [n] -> int64 rows [n,7]: 1, qx, qy, qz, r, g, b."""
    p = np.asarray(payload).astype(np.uint64)
    cols = [np.ones(p.shape, np.uint64), p & np.uint64(1023), (p >> np.uint64(10)) & np.uint64(1023), (p >> np.uint64(20)) & np.uint64(1023),
            (p >> np.uint64(30)) & np.uint64(255), (p >> np.uint64(38)) & np.uint64(255), (p >> np.uint64(46)) & np.uint64(255)]
    return np.stack(cols, -1).astype(np.int64).reshape(-1, 7)


def _check_params(voxel, stride, border, min_depth, max_range, edge, min_count=1):
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel: a positive size, got %r" % (voxel,))
    if int(stride) < 1 or int(border) < 0 or int(min_count) < 1:
        raise ValueError("stride >= 1, border >= 0, min_count >= 1; got %r, %r, %r" % (stride, border, min_count))
    if not (edge >= 0) or not (min_depth <= max_range):
        raise ValueError("edge >= 0 and min_depth <= max_range; got %r, %r, %r" % (edge, min_depth, max_range))


def _check_view_params(min_views, view_radius, view_tol):
    if not 1 <= int(view_radius) <= MAX_VIEW_RADIUS or not view_tol >= 0:
        raise ValueError("view_radius: 1 ... %d, view_tol >= 0; got %r, %r" % (MAX_VIEW_RADIUS, view_radius, view_tol))
    if not 0 <= int(min_views) <= 2 * int(view_radius):
        raise ValueError("min_views: 0 ... 2 view_radius = %d (a frame has that many neighbours), got %r" % (2 * int(view_radius), min_views))


def _check_frames(depth, color, poses, device):
    """depth float32 [B,H,W], color uint8 [B,3,H,W], poses float64 [B,3,4] -> the three, contiguous.  ``device``: tensors on a HIP device
    of exactly those types (a CPU tensor is native.require_device's error); else anything numpy converts to them."""
    kinds = (torch.float32, torch.uint8, torch.float64) if device else (np.float32, np.uint8, np.float64)
    if device:
        native.require_device(depth, color, poses)
        t = [x.contiguous() for x in (depth, color, poses)]
    else:
        t = [np.ascontiguousarray(x, dtype=kind) for x, kind in zip((depth, color, poses), kinds)]
    d, c, p = (tuple(x.shape) for x in t)
    if [x.dtype for x in t] != list(kinds) or len(d) != 3 or c != (d[0], 3) + d[1:] or p != (d[0], 3, 4):
        raise ValueError("depth float32 [B,H,W], color uint8 [B,3,H,W], poses float64 [B,3,4]; got " +
                         ", ".join("%s %s" % (tuple(x.shape), x.dtype) for x in t))
    return t


def _inv_K9(inv_K, name="inv_K"):
    m = np.asarray(inv_K, dtype=np.float64)
    if m.shape in ((3, 3), (4, 4)):
        m = m[:3, :3]
    m = np.ascontiguousarray(m).reshape(-1)
    if m.shape != (9,):
        raise ValueError("%s: 3x3 (or 4x4, whose 3x3 block is used), got %s" % (name, np.shape(inv_K)))
    return m


def _view_K9(K, inv_K):
    """The nine entries of K's 3x3 block; ``K`` None: the float64 inverse of inv_K's."""
    return _inv_K9(np.linalg.inv(_inv_K9(inv_K).reshape(3, 3)) if K is None else K, "K")


def _view_ranges(N, H, W, radius, tol, centres, bounds):
    """The checked (radius, c0, c1, lo, hi) of views_numpy / views_hip."""
    if H < 2 or W < 2:
        raise ValueError("frames of at least 2 x 2 pixels (the four taps), got %d x %d" % (H, W))
    if not 1 <= int(radius) <= MAX_VIEW_RADIUS or not tol >= 0:
        raise ValueError("radius: 1 ... %d, tol >= 0; got %r, %r" % (MAX_VIEW_RADIUS, radius, tol))
    lo, hi = (0, N) if bounds is None else (int(bounds[0]), int(bounds[1]))
    c0, c1 = (lo, hi) if centres is None else (int(centres[0]), int(centres[1]))
    if not 0 <= lo <= c0 <= c1 <= hi <= N:
        raise ValueError("0 <= lo <= c0 <= c1 <= hi <= %d; got centres %r, bounds %r" % (N, centres, bounds))
    if hi - lo < 2 * int(radius) + 1:
        raise ValueError("radius %d needs %d frames, the bounds hold %d" % (radius, 2 * int(radius) + 1, hi - lo))
    return int(radius), c0, c1, lo, hi


def camera_points_numpy(depth, inv_K, depth_scale=1.0):
    """depth float32 [B,H,W] -> float64 [3,B,H,W]: p = (depth depth_scale) ray, ray_k = (m_k0 u + m_k1 v) + m_k2 at integer pixel
    coordinates (the reference's Backproject, oracle/geometry.py:backproject, in float64)."""
    d = np.asarray(depth, dtype=np.float32)
    m = _inv_K9(inv_K)
    H, W = d.shape[1:]
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    with np.errstate(invalid="ignore", over="ignore"):
        ds = d.astype(np.float64) * np.float64(depth_scale)
        return np.stack([ds * ((m[3 * k] * u + m[3 * k + 1] * v) + m[3 * k + 2]) for k in range(3)], 0)


def pixel_causes_numpy(depth, depth_scale, stride, border, min_depth, max_range, edge):
    """depth float32 [B,H,W] -> int8 [B,H,W]: 0 for a pixel that is valid so far, else the first of td_cloud_keys' causes 1 ... 4 that
    holds (off the stride's lattice, in the border, depth not finite or out of range, a depth step to a 4-neighbour).  Shared by
    keys_numpy and tsdf.samples_numpy."""
    d = np.asarray(depth, dtype=np.float32)
    B, H, W = d.shape
    stride, border = int(stride), int(border)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ys, xs = np.broadcast_to(ys, d.shape), np.broadcast_to(xs, d.shape)
    cause = np.zeros(d.shape, np.int8)

    def mark(mask, code):
        cause[(cause == 0) & mask] = code

    with np.errstate(invalid="ignore", over="ignore"):
        ds = d.astype(np.float64) * np.float64(depth_scale)
        mark((xs % stride != 0) | (ys % stride != 0), 1)
        mark((xs < border) | (xs >= W - border) | (ys < border) | (ys >= H - border), 2)
        mark(~np.isfinite(d) | ~((ds >= np.float64(min_depth)) & (ds <= np.float64(max_range))), 3)
        if edge > 0:
            e = np.float32(edge)
            bad = np.zeros(d.shape, bool)
            for axis, shift in ((1, 1), (1, -1), (2, 1), (2, -1)):
                nb = np.roll(d, shift, axis=axis)
                inside = np.ones(d.shape, bool)
                edge_line = [slice(None)] * 3
                edge_line[axis] = 0 if shift == 1 else -1
                inside[tuple(edge_line)] = False           # the rolled-in line is no neighbour
                bad |= inside & (~np.isfinite(nb) | (np.abs(d - nb) > e * np.minimum(d, nb)))
            mark(bad, 4)
    return cause


def keys_numpy(depth, color, poses, inv_K, depth_scale=1.0, pose_scale=1.0, inv_voxel=1.0 / DEFAULT_VOXEL, stride=1, border=0,
               min_depth=DEFAULT_MIN_DEPTH, max_range=DEFAULT_MAX_RANGE, edge=0.0):
    """depth float32 [B,H,W], color uint8 [B,3,H,W], poses float64 [B,3,4] -> (key int64 [B H W], payload uint64 [B H W], counts
    int64 [6] in the order of CAUSES).  The statement td_cloud_keys is tested against, operation for operation."""
    d, c, P = _check_frames(depth, color, poses, device=False)
    m = _inv_K9(inv_K)
    B, H, W = d.shape
    stride, border = int(stride), int(border)
    depth_scale, pose_scale, inv_voxel = np.float64(depth_scale), np.float64(pose_scale), np.float64(inv_voxel)
    cause = pixel_causes_numpy(d, depth_scale, stride, border, min_depth, max_range, edge)

    def mark(mask, code):
        cause[(cause == 0) & mask] = code

    with np.errstate(invalid="ignore", over="ignore"):
        px, py, pz = camera_points_numpy(d, m, depth_scale)
        g = []
        for k in range(3):
            r0, r1, r2, t = (P[:, k, j].reshape(B, 1, 1) for j in range(4))
            world = ((r0 * px + r1 * py) + r2 * pz) + pose_scale * t
            g.append(world * inv_voxel)
    key, _, payload = grid_keys_numpy(g)
    mark(key == INVALID_KEY, 5)
    ok = cause == 0
    for ch, shift in ((0, 30), (1, 38), (2, 46)):
        payload = payload | (c[:, ch].astype(np.uint64) << np.uint64(shift))
    key = np.where(ok, key, INVALID_KEY).astype(np.int64).reshape(-1)
    payload = np.where(ok, payload, np.uint64(0)).astype(np.uint64).reshape(-1)
    return key, payload, np.bincount(cause.reshape(-1), minlength=6).astype(np.int64)


def views_numpy(depth, poses, inv_K, K, radius, tol, depth_scale=1.0, pose_scale=1.0, min_depth=DEFAULT_MIN_DEPTH,
                max_range=DEFAULT_MAX_RANGE, centres=None, bounds=None):
    """depth float32 [N,H,W], poses float64 [N,3,4] camera-to-world, K / inv_K: the 3x3 blocks -> votes uint8 [c1-c0,H,W]: for every
    pixel of the frames ``centres`` = (c0, c1) (default: the frames of ``bounds``) the number of its 2 radius neighbours inside
    ``bounds`` = (lo, hi) (default: (0, N)) that see the same depth there; 0 where the pixel's own depth is not ok.  The statement
    td_cloud_views is tested against, operation for operation (the module's docstring).

    A depth test alone is enough: the neighbour's surface is sampled where the pixel's point projects, so where z and s agree the
    point the neighbour sees there, sent back into frame i, lands within the same relative difference of the pixel it came from:
    the round-trip reprojection error is bounded by the difference that is tested, and a second criterion would add nothing."""
    d = np.ascontiguousarray(depth, dtype=np.float32)
    P = np.ascontiguousarray(poses, dtype=np.float64)
    if d.ndim != 3 or P.shape != (d.shape[0], 3, 4):
        raise ValueError("depth [N,H,W], poses [N,3,4]; got %s, %s" % (d.shape, P.shape))
    N, H, W = d.shape
    radius, c0, c1, lo, hi = _view_ranges(N, H, W, radius, tol, centres, bounds)
    m, k = _inv_K9(inv_K), _inv_K9(K, "K")
    depth_scale, pose_scale, tol = np.float64(depth_scale), np.float64(pose_scale), np.float64(tol)
    votes = np.zeros((c1 - c0, H, W), np.uint8)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ds = d.astype(np.float64) * depth_scale
        ok = np.isfinite(d) & (ds >= np.float64(min_depth)) & (ds <= np.float64(max_range))
        for i in range(c0, c1):
            p = camera_points_numpy(d[i:i + 1], m, depth_scale)[:, 0]
            w = [((P[i, r, 0] * p[0] + P[i, r, 1] * p[1]) + P[i, r, 2] * p[2]) + pose_scale * P[i, r, 3] for r in range(3)]
            first = min(max(i - radius, lo), hi - 1 - 2 * radius)
            for j in range(first, first + 2 * radius + 1):
                if j == i:
                    continue
                e = [w[r] - pose_scale * P[j, r, 3] for r in range(3)]
                q = [(P[j, 0, r] * e[0] + P[j, 1, r] * e[1]) + P[j, 2, r] * e[2] for r in range(3)]
                z = q[2]
                uj = ((k[0] * q[0] + k[1] * q[1]) + k[2] * q[2]) / z
                vj = ((k[3] * q[0] + k[4] * q[1]) + k[5] * q[2]) / z
                inside = ok[i] & (z > 0) & (uj >= 0) & (uj <= W - 1) & (vj >= 0) & (vj <= H - 1)          # a NaN fails
                x0 = np.minimum(np.floor(np.where(inside, uj, 0.0)), W - 2)
                y0 = np.minimum(np.floor(np.where(inside, vj, 0.0)), H - 2)
                fx, fy = uj - x0, vj - y0
                xi, yi = x0.astype(np.intp), y0.astype(np.intp)
                t00, t01, t10, t11 = ds[j][yi, xi], ds[j][yi, xi + 1], ds[j][yi + 1, xi], ds[j][yi + 1, xi + 1]
                taps = ok[j][yi, xi] & ok[j][yi, xi + 1] & ok[j][yi + 1, xi] & ok[j][yi + 1, xi + 1]
                top = t00 + fx * (t01 - t00)
                bot = t10 + fx * (t11 - t10)
                s = top + fy * (bot - top)
                votes[i - c0] += inside & taps & (np.abs(z - s) <= tol * np.minimum(z, s))
    return votes


def mask_views_numpy(key, payload, votes, min_views):
    """What td_cloud_views does to the pairs of keys_numpy: a pixel that is still valid and has fewer than ``min_views`` votes gets
    INVALID_KEY and payload 0 -> (key, payload, votes with 0 where the key was invalid already, int64 [2]: tested, dropped)."""
    key, payload = np.asarray(key, np.int64).reshape(-1), np.asarray(payload, np.uint64).reshape(-1)
    flat = np.asarray(votes, np.uint8).reshape(-1)
    tested = key != INVALID_KEY
    drop = tested & (flat < int(min_views))
    return (np.where(drop, INVALID_KEY, key).astype(np.int64), np.where(drop, np.uint64(0), payload).astype(np.uint64),
            np.where(tested, flat, 0).astype(np.uint8).reshape(np.shape(votes)), np.array([tested.sum(), drop.sum()], np.int64))


def voxel_table_numpy(key, rows):
    """Points (key int64 [n]; rows: uint64 payloads [n] or int64 rows [n,7]) -> (keys int64 [V] ascending, sums int64 [V,7]): sort,
    np.unique, np.add.reduceat.  Invalid keys are dropped."""
    key = np.asarray(key, dtype=np.int64).reshape(-1)
    rows = np.asarray(rows)
    rows = unpack_payload(rows) if rows.ndim == 1 else rows.astype(np.int64).reshape(-1, 7)
    if len(rows) != len(key):
        raise ValueError("one row per key: %d keys, %d rows" % (len(key), len(rows)))
    valid = key != INVALID_KEY
    key, rows = key[valid], rows[valid]
    if not len(key):
        return np.zeros(0, np.int64), np.zeros((0, 7), np.int64)
    order = np.argsort(key, kind="stable")
    key, rows = key[order], rows[order]
    ukeys, starts = np.unique(key, return_index=True)
    return ukeys, np.add.reduceat(rows, starts, axis=0)


def finish_numpy(keys, sums, voxel, min_count=1):
    """(keys [V], sums [V,7]) -> (xyz float32 [V,3], rgb uint8 [V,3], count int32 [V], keep bool [V])."""
    keys, sums = np.asarray(keys, np.int64), np.asarray(sums, np.int64).reshape(-1, 7)
    n = sums[:, 0]
    i = np.stack(unpack_key(keys), -1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        xyz = ((i + (sums[:, 1:4].astype(np.float64) / n.astype(np.float64)[:, None] + 0.5) / 1024.0) * np.float64(voxel)).astype(np.float32)
    rgb = ((2 * sums[:, 4:7] + n[:, None]) // np.maximum(2 * n[:, None], 1)).astype(np.uint8)
    count = np.minimum(n, 0x7fffffff).astype(np.int32)
    return xyz, rgb, count, n >= int(min_count)


def _stats(counts, voxels, kept, invalid_views=None):
    out = {"points": int(np.sum(counts))}
    out.update({name: int(v) for name, v in zip(CAUSES, counts)})
    if invalid_views is not None:          # the multi-view filter is on: it took these from the valid pixels
        out["valid"], out["invalid_views"] = out["valid"] - int(invalid_views), int(invalid_views)
    out["voxels"], out["voxels_dropped"] = int(voxels), int(voxels) - int(kept)
    return out


def fuse_numpy(depth, color, poses, inv_K, voxel=DEFAULT_VOXEL, stride=1, border=0, min_depth=DEFAULT_MIN_DEPTH,
               max_range=DEFAULT_MAX_RANGE, edge=0.0, min_count=1, depth_scale=1.0, pose_scale=1.0, min_views=0,
               view_radius=DEFAULT_VIEW_RADIUS, view_tol=DEFAULT_VIEW_TOL, K=None, debug=None):
    """All frames at once -> Cloud of numpy arrays: keys_numpy, with ``min_views`` > 0 views_numpy over all frames (every frame a
    centre, every frame a possible neighbour) and mask_views_numpy, then voxel_table_numpy, finish_numpy.  ``K``: the 3x3 block the
    filter projects with (default: the inverse of inv_K's);  ``debug``: a dict that receives the filter's "votes" [B,H,W]."""
    _check_params(voxel, stride, border, min_depth, max_range, edge, min_count)
    _check_view_params(min_views, view_radius, view_tol)
    key, payload, counts = keys_numpy(depth, color, poses, inv_K, depth_scale, pose_scale, 1.0 / float(voxel), stride, border, min_depth,
                                      max_range, edge)
    dropped = None
    if min_views > 0:
        votes = views_numpy(depth, poses, inv_K, _view_K9(K, inv_K), view_radius, view_tol, depth_scale, pose_scale, min_depth, max_range)
        key, payload, votes, (_, dropped) = mask_views_numpy(key, payload, votes, min_views)
        if debug is not None:
            debug["votes"] = votes
    keys, sums = voxel_table_numpy(key, payload)
    xyz, rgb, count, keep = finish_numpy(keys, sums, voxel, min_count)
    return Cloud(xyz[keep], rgb[keep], count[keep], keys[keep], _stats(counts, len(keys), int(keep.sum()), dropped))


def save_ply(path, xyz, rgb, count, normals=None):
    """binary_little_endian 1.0 PLY: x y z float, red green blue uchar, count int; one structured array, one write.  ``normals`` [n,3]
    (cloud_normals'; all zero: the point has none) adds nx ny nz float after count; without it the file is what it always was."""
    xyz, rgb, count = (np.asarray(t.cpu() if torch.is_tensor(t) else t) for t in (xyz, rgb, count))
    n = len(xyz)
    if xyz.shape != (n, 3) or rgb.shape != (n, 3) or count.shape != (n,):
        raise ValueError("xyz [n,3], rgb [n,3], count [n]; got %s, %s, %s" % (xyz.shape, rgb.shape, count.shape))
    dtype = PLY_DTYPE
    if normals is not None:
        normals = np.asarray(normals.cpu() if torch.is_tensor(normals) else normals)
        if normals.shape != (n, 3):
            raise ValueError("normals [n,3], got %s" % (normals.shape,))
        dtype = np.dtype(PLY_DTYPE.descr + [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])
    rec = np.empty(n, dtype)
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    rec["count"] = count
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n]
    header += ["property %s %s" % ({"<f4": "float", "u1": "uchar", "<i4": "int"}[dtype[name].str.replace("|", "")], name)
               for name in dtype.names]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def load_ply(path):
    """A binary_little_endian PLY with one vertex element of scalar properties -> structured array (save_ply's: PLY_DTYPE)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("%s: not a PLY file" % path)
        n, fields, fmt = None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            words = line.decode("ascii").split()
            if words[:1] == ["end_header"]:
                break
            if words[:1] == ["format"]:
                fmt = words[1]
            elif words[:2] == ["element", "vertex"]:
                n = int(words[2])
            elif words[:1] == ["element"]:
                raise ValueError("%s: only a vertex element is read" % path)
            elif words[:1] == ["property"]:
                if len(words) != 3 or words[1] not in _PLY_TYPES:
                    raise ValueError("%s: unsupported property %r" % (path, " ".join(words)))
                fields.append((words[2], _PLY_TYPES[words[1]]))
        if fmt != "binary_little_endian" or n is None:
            raise ValueError("%s: binary_little_endian with a vertex element expected" % path)
        dtype = np.dtype(fields)
        data = f.read()
    if len(data) != n * dtype.itemsize:
        raise ValueError("%s: %d bytes of vertices, expected %d" % (path, len(data), n * dtype.itemsize))
    return np.frombuffer(data, dtype=dtype, count=n).copy()


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def _i64(t, name, n=None):
    native.require_device(t)
    if t.dtype != torch.int64 or t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise ValueError("%s: int64 [%s], got %s %s" % (name, "n" if n is None else n, tuple(t.shape), t.dtype))
    return t.contiguous()


def _check_rows(keys, sums):
    """A voxel list on the device: keys int64 [V], sums int64 [V,7] -> the keys, contiguous."""
    keys = _i64(keys, "keys")
    native.require_device(sums)
    if sums.dtype != torch.int64 or tuple(sums.shape) != (keys.shape[0], 7):
        raise ValueError("sums: int64 [%d,7], got %s %s" % (keys.shape[0], tuple(sums.shape), sums.dtype))
    return keys


def keys_hip(depth, color, poses, inv_K, depth_scale=1.0, pose_scale=1.0, inv_voxel=1.0 / DEFAULT_VOXEL, stride=1, border=0,
             min_depth=DEFAULT_MIN_DEPTH, max_range=DEFAULT_MAX_RANGE, edge=0.0, stats=None):
    """keys_numpy as one launch of td_cloud_keys -> (key int64 [B H W], payload int64 [B H W]: the uint64's bits).  ``stats``: an int64
    [6] device tensor that the launch increments (the order of CAUSES), or None."""
    depth, color, poses = _check_frames(depth, color, poses, device=True)
    if int(stride) < 1 or int(border) < 0 or not inv_voxel > 0 or not edge >= 0:
        raise ValueError("stride >= 1, border >= 0, inv_voxel > 0, edge >= 0")
    if stats is not None:
        stats = _i64(stats, "stats", 6)
    m = _inv_K9(inv_K)
    B, H, W = depth.shape
    key = torch.empty(B * H * W, dtype=torch.int64, device=depth.device)
    payload = torch.empty(B * H * W, dtype=torch.int64, device=depth.device)
    if B * H * W == 0:                   # an empty tensor has no pointer to pass
        return key, payload
    native.call("td_cloud_keys", depth, color, poses, (ctypes.c_double * 9)(*m), B, H, W,
                float(depth_scale), float(pose_scale), float(inv_voxel), int(stride), int(border), float(min_depth), float(max_range),
                float(edge), key, payload, stats)
    return key, payload


def views_hip(depth, poses, inv_K, K, radius, tol, depth_scale=1.0, pose_scale=1.0, min_depth=DEFAULT_MIN_DEPTH,
              max_range=DEFAULT_MAX_RANGE, centres=None, bounds=None, key=None, payload=None, min_views=0, stats=None, votes=True):
    """views_numpy as one launch of td_cloud_views -> votes uint8 [c1-c0,H,W] (None with ``votes`` false).  ``depth`` and ``poses``
    are the whole window's.  ``key``, ``payload``: the int64 [(c1-c0) H W] pairs keys_hip wrote for the centre frames, changed in
    place as mask_views_numpy changes them (a pixel whose key is invalid already is skipped: 0 votes); without them every pixel is
    evaluated and only the votes are written.  ``stats``: an int64 [2] device tensor that the launch increments by the numbers of
    pixels tested and dropped, or None."""
    native.require_device(depth, poses)
    if depth.dtype != torch.float32 or depth.dim() != 3 or poses.dtype != torch.float64 or tuple(poses.shape) != (depth.shape[0], 3, 4):
        raise ValueError("depth float32 [N,H,W], poses float64 [N,3,4]; got %s %s, %s %s" % (
            tuple(depth.shape), depth.dtype, tuple(poses.shape), poses.dtype))
    N, H, W = depth.shape
    radius, c0, c1, lo, hi = _view_ranges(N, H, W, radius, tol, centres, bounds)
    if not 0 <= int(min_views) <= 2 * radius:
        raise ValueError("min_views: 0 ... 2 radius = %d, got %r" % (2 * radius, min_views))
    n = (c1 - c0) * H * W
    if (key is None) != (payload is None) or (key is None and not votes):
        raise ValueError("key and payload come together, and without them the votes are the only result")
    if key is not None:
        for t, name in ((key, "key"), (payload, "payload")):
            if _i64(t, name, n) is not t:          # changed in place: a copy would take the result away
                raise ValueError("%s: a contiguous tensor" % name)
    if stats is not None:
        stats = _i64(stats, "stats", 2)
    m, k = _inv_K9(inv_K), _inv_K9(K, "K")
    out = torch.empty(c1 - c0, H, W, dtype=torch.uint8, device=depth.device) if votes else None
    if n == 0:                           # an empty tensor has no pointer to pass
        return out
    native.call("td_cloud_views", depth.contiguous(), poses.contiguous(), (ctypes.c_double * 9)(*k), (ctypes.c_double * 9)(*m), N, H, W,
                c0, c1, lo, hi, radius, int(min_views), float(tol), float(depth_scale), float(pose_scale), float(min_depth),
                float(max_range), key, payload, out, stats)
    return out


def heads_hip(sorted_keys):
    """Sorted int64 keys [N] -> int32 [N]: 1 where a valid key differs from its predecessor (td_cloud_heads)."""
    keys = _i64(sorted_keys, "sorted_keys")
    flags = torch.empty(keys.shape[0], dtype=torch.int32, device=keys.device)
    if keys.shape[0] == 0:
        return flags
    native.call("td_cloud_heads", keys, keys.shape[0], flags)
    return flags


def reduce_hip(sorted_keys, seg, perm, src, V):
    """The segmented sum -> (keys int64 [V], sums int64 [V,7]).  ``seg``: torch.cumsum(heads_hip(sorted_keys), 0) (int64, inclusive);
    ``perm``: the sort's permutation or None;  ``src``: int64 [n] payloads as keys_hip wrote them (td_cloud_reduce_packed) or int64
    [n,7] already-summed rows (td_cloud_reduce_rows);  V = seg[-1], which the caller has read."""
    keys = _i64(sorted_keys, "sorted_keys")
    N, V = keys.shape[0], int(V)
    seg = _i64(seg, "seg", N)
    perm = None if perm is None else _i64(perm, "perm", N)
    native.require_device(src)
    packed = src.dim() == 1
    if src.dtype != torch.int64 or not (packed or (src.dim() == 2 and src.shape[1] == 7)):
        raise ValueError("src: int64 [n] payloads or int64 [n,7] rows, got %s %s" % (tuple(src.shape), src.dtype))
    if not 0 <= V <= N:
        raise ValueError("V: 0 ... %d, got %d" % (N, V))
    out_keys = torch.empty(V, dtype=torch.int64, device=keys.device)
    sums = torch.zeros(V, 7, dtype=torch.int64, device=keys.device)
    if V == 0:
        return out_keys, sums
    native.call("td_cloud_reduce_packed" if packed else "td_cloud_reduce_rows", keys, seg, perm, src.contiguous(), src.shape[0], N, V,
                out_keys, sums)
    return out_keys, sums


def finish_hip(keys, sums, voxel, min_count=1):
    """finish_numpy as td_cloud_finish -> (xyz float32 [V,3], rgb uint8 [V,3], count int32 [V], keep uint8 [V])."""
    keys = _check_rows(keys, sums)
    V = keys.shape[0]
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel: a positive size, got %r" % (voxel,))
    dev = keys.device
    xyz, rgb = torch.empty(V, 3, dtype=torch.float32, device=dev), torch.empty(V, 3, dtype=torch.uint8, device=dev)
    count, keep = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(V, dtype=torch.uint8, device=dev)
    if V == 0:
        return xyz, rgb, count, keep
    native.call("td_cloud_finish", keys, sums.contiguous(), V, float(voxel), int(min_count), xyz, rgb, count, keep)
    return xyz, rgb, count, keep


def table_hip(key, src):
    """voxel_table_numpy on the device: torch.sort, heads_hip, torch.cumsum, reduce_hip -> (keys [V] ascending, sums [V,7]).
    ONE host synchronisation: V = seg[-1] sizes the output."""
    key = _i64(key, "key")
    if key.shape[0] == 0:
        return key.new_zeros(0), key.new_zeros(0, 7)
    sorted_keys, perm = torch.sort(key)
    seg = torch.cumsum(heads_hip(sorted_keys), 0)
    V = int(seg[-1].item())
    return reduce_hip(sorted_keys, seg, perm, src, V)


def merge_hip(keys_a, sums_a, keys_b, sums_b):
    """Two voxel lists (unique keys, [.,7] rows) -> their union, rows of equal keys added: concatenate, table_hip."""
    keys_a, keys_b = _check_rows(keys_a, sums_a), _check_rows(keys_b, sums_b)
    if keys_a.shape[0] == 0:
        return keys_b, sums_b
    if keys_b.shape[0] == 0:
        return keys_a, sums_a
    return table_hip(torch.cat([keys_a, keys_b]), torch.cat([sums_a, sums_b]))


class VoxelMap:
    """The running voxel map on the device: ``keys`` int64 [V] sorted and unique, their rows ``sums`` int64 [V,7], and ``counts``, the
    int64 [n_counters] that the kernel which makes the map's pairs increments."""

    def __init__(self, device, n_counters):
        self.keys = torch.zeros(0, dtype=torch.int64, device=device)
        self.sums = torch.zeros(0, 7, dtype=torch.int64, device=device)
        self.counts = torch.zeros(n_counters, dtype=torch.int64, device=device)

    def merge(self, key, payload, pair_chunk=None):
        """A batch of pairs into the map, ``pair_chunk`` at a time (default: all at once); the sums are integers: the cut changes nothing."""
        step = max(key.shape[0], 1) if pair_chunk is None else pair_chunk
        for at in range(0, key.shape[0], step):
            self.keys, self.sums = merge_hip(self.keys, self.sums, *table_hip(key[at:at + step], payload[at:at + step]))


class FrameMap(VoxelMap):
    """A VoxelMap that frames are fused into, and what the sequence driver asks of a sink: ``add(depth, color, poses, window)`` for one
    batch of centre frames, ``min_views`` and ``radius``.  With the filter on, ``window`` = (depth [n,H,W], poses [n,3,4], centres,
    bounds): the frames the neighbours come from and where the batch and the sequence's ends lie in them; ``votes`` is views_hip on it."""

    def __init__(self, device, n_counters, inv_K, depth_scale, pose_scale, min_depth, max_range, min_views=0,
                 view_radius=DEFAULT_VIEW_RADIUS, view_tol=DEFAULT_VIEW_TOL, K=None):
        super().__init__(device, n_counters)
        _check_view_params(min_views, view_radius, view_tol)
        self.min_views, self.radius = int(min_views), int(view_radius)
        if self.min_views:
            self.view_args = (inv_K, _view_K9(K, inv_K), self.radius, float(view_tol), float(depth_scale), float(pose_scale), min_depth,
                              max_range)

    def votes(self, window, **kw):
        return views_hip(window[0], window[1], *self.view_args, centres=window[2], bounds=window[3], **kw)


class _DeviceMap(FrameMap):
    """The voxel-averaged cloud's map: keys_hip makes the pairs, the filter invalidates them in place.  ``want_votes``: keep the votes
    of every batch in ``self.kept_votes``."""

    def __init__(self, device, inv_K, voxel, stride, border, min_depth, max_range, edge, depth_scale, pose_scale, min_views=0,
                 view_radius=DEFAULT_VIEW_RADIUS, view_tol=DEFAULT_VIEW_TOL, K=None, want_votes=False):
        super().__init__(device, 6, inv_K, depth_scale, pose_scale, min_depth, max_range, min_views, view_radius, view_tol, K)
        self.args = (inv_K, float(depth_scale), float(pose_scale), 1.0 / float(voxel), stride, border, min_depth, max_range, edge)
        if self.min_views:
            self.view_counts = torch.zeros(2, dtype=torch.int64, device=device)
        self.want_votes, self.kept_votes = bool(want_votes), []

    def add(self, depth, color, poses, window=None):
        key, payload = keys_hip(depth, color, poses, *self.args, stats=self.counts)
        if self.min_views:
            votes = self.votes(window, key=key, payload=payload, min_views=self.min_views, stats=self.view_counts, votes=self.want_votes)
            if self.want_votes:
                self.kept_votes.append(votes)
        self.merge(key, payload)

    def cloud(self, voxel, min_count):
        xyz, rgb, count, keep = finish_hip(self.keys, self.sums, voxel, min_count)
        keep = keep.bool()
        out = (xyz[keep], rgb[keep], count[keep], self.keys[keep])
        dropped = int(self.view_counts[1].item()) if self.min_views else None
        return Cloud(*out, _stats(self.counts.cpu().numpy(), self.keys.shape[0], out[3].shape[0], dropped))


def frame_batches(first, last, batch_size):
    """The (at, end) of the batches of at most ``batch_size`` frames (None: one batch) that cover first ... last-1."""
    step = last - first if batch_size is None else int(batch_size)
    if step < 1 and last > first:
        raise ValueError("batch_size: at least 1, got %r" % (batch_size,))
    return [(at, min(at + step, last)) for at in range(first, last, max(step, 1))]


def fuse_hip(depth, color, poses, inv_K, voxel=DEFAULT_VOXEL, batch_size=None, stride=1, border=0, min_depth=DEFAULT_MIN_DEPTH,
             max_range=DEFAULT_MAX_RANGE, edge=0.0, min_count=1, depth_scale=1.0, pose_scale=1.0, min_views=0,
             view_radius=DEFAULT_VIEW_RADIUS, view_tol=DEFAULT_VIEW_TOL, K=None, debug=None):
    """fuse_numpy on the device, ``batch_size`` frames at a time (default: all at once) -> Cloud of device tensors.  With
    ``min_views`` > 0, per batch of centre frames: keys_hip, views_hip on those keys with all frames as the window, then the
    unchanged table and merge; with 0 no td_cloud_views is launched."""
    _check_params(voxel, stride, border, min_depth, max_range, edge, min_count)
    native.require_device(depth, color, poses)
    vmap = _DeviceMap(depth.device, inv_K, voxel, stride, border, min_depth, max_range, edge, depth_scale, pose_scale, min_views,
                      view_radius, view_tol, K, want_votes=debug is not None)
    for at, end in frame_batches(0, len(depth), batch_size):          # all frames are the filter's window
        vmap.add(depth[at:end], color[at:end], poses[at:end], (depth, poses, (at, end), (0, len(depth))) if vmap.min_views else None)
    if vmap.kept_votes:
        debug["votes"] = torch.cat(vmap.kept_votes)
    return vmap.cloud(voxel, min_count)


# ---------------------------------------------------------------------------------------------------------------------------

def dataset_K(dataset):
    """The float64 3x3 block of the dataset's inputs["K"] (pixels at the dataset's frame size)."""
    return np.ascontiguousarray(np.asarray(dataset[0]["K"], dtype=np.float64)[:3, :3])


def dataset_inv_K(dataset):
    """The float64 inverse of the 3x3 block of the dataset's inputs["K"] (pixels at the dataset's frame size)."""
    return np.linalg.inv(dataset_K(dataset))


def window_schedule(first, last, batch_size, radius):
    """The multi-view filter's sliding window over the frames first ... last-1 (at least 2 radius + 1), predicted ``batch_size`` at a
    time: yields (at, end, ready, keep) per batch.  The frames at ... end-1 join the held window; then the centres of ``ready``, a
    list of (c0, c1) ranges of at most batch_size frames, are fused: a centre is ready once the last frame of its clamped window
    (views_numpy's a ... a + 2 radius) is held; afterwards the window drops the frames before ``keep``, which no later centre needs.
    Every frame is predicted once, every centre fused once, in order; at most batch_size + 2 radius depth maps are ever held."""
    start = lambda i: min(max(i - radius, first), last - 1 - 2 * radius)          # the first frame of centre i's clamped window
    centre, keep = first, first
    for at, end in frame_batches(first, last, batch_size):
        done = centre
        while done < last and start(done) + 2 * radius < end:
            done += 1
        ready, centre = frame_batches(centre, done, batch_size), done
        if centre < last:
            keep = start(centre)
        yield at, end, ready, keep


def feed_frames(predict, sink, color, poses, first, last, batch_size, windowed, depths=None):
    """The sequence driver's loop.  ``predict``: uint8 frames [b,3,H,W] -> depth float32 [b,H,W];  ``color`` [n,3,H,W], ``poses``
    [n,3,4]: every frame's, of which first ... last-1 are fused;  ``depths``: a list that receives every batch's depth maps.
    ``windowed`` (the filter on the device path): window_schedule's batches; the depth maps of the frames w0 ... end-1 are held, and
    their ends stand in for the ends of the fused range: a centre that is ready has its whole clamped window inside."""
    if not windowed:
        for at, end in frame_batches(first, last, batch_size):
            depth = predict(color[at:end])
            sink.add(depth, color[at:end], poses[at:end])
            if depths is not None:
                depths.append(depth)
        return
    window, w0 = None, first
    for at, end, ready, keep in window_schedule(first, last, batch_size, sink.radius):
        depth = predict(color[at:end])
        if depths is not None:
            depths.append(depth)
        window = depth if window is None else torch.cat([window, depth])
        for c0, c1 in ready:                                                # at most a batch of points at a time
            sink.add(window[c0 - w0:c1 - w0], color[c0:c1], poses[c0:c1], (window, poses[w0:end], (c0 - w0, c1 - w0), (0, end - w0)))
        window, w0 = window[keep - w0:], keep


class HostFrames:
    """The host path's sink: it keeps the batches for the numpy chain, which takes all frames at once (``arrays``: depth [m,H,W],
    color [m,3,H,W], poses [m,3,4] of the fused frames)."""

    def __init__(self, min_views=0, view_radius=DEFAULT_VIEW_RADIUS):
        self.min_views, self.radius, self.batches = int(min_views), int(view_radius), []

    def add(self, depth, color, poses, window=None):
        self.batches.append((depth, color, poses))

    def arrays(self):
        return tuple(np.concatenate([np.asarray(b[k]) for b in self.batches]) for k in range(3))


class SequenceDriver:
    """What SceneFuser and tsdf.TsdfFuser share: frames of a dataset -> DepthPredictor (``predictor``) + the pose chain -> a sink.
    ``run`` uploads the frames once, checks the ranges and feeds the sink: sink.add(depth, color, poses, window) per batch (a
    FrameMap; HostFrames on the host path), sink.min_views and sink.radius for the multi-view filter, whose sliding window runs on
    the device path only.  ``poses``: float64 [n+1,3,4] on the host, the poses of the last run."""

    def __init__(self, model, height, width, device, batch_size=12, precision="fp32", post_process=False):
        self.device = infer.check_precision(device, precision, batch_size)
        self.on_hip = self.device.type == "cuda"
        self.model, self.batch_size, self.precision = model, int(batch_size), precision
        self.predictor = infer.DepthPredictor(model, height, width, self.device, precision=precision, post_process=post_process)
        self.poses = None

    def predict(self, color):
        return self.predictor.predict(color.permute(0, 2, 3, 1).contiguous()).depth.contiguous()

    def camera_poses(self, dataset, frames, poses):
        """float64 [n+1,3,4] camera-to-world, on the device (a numpy array on the host path)."""
        m = frames.shape[0]
        if poses is not None:
            p = np.ascontiguousarray(np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, dtype=np.float64))
            if p.ndim != 3 or p.shape[0] != m or p.shape[1:] not in ((3, 4), (4, 4)):
                raise ValueError("poses: [%d,3,4] camera-to-world for %d frames, got %s" % (m, m, p.shape))
            p = np.ascontiguousarray(p[:, :3])
            return torch.from_numpy(p).to(self.device) if self.on_hip else p
        rel = odometry.OdometryEvaluator(self.model, self.device, self.batch_size, self.precision).relative_poses(dataset, frames=frames)
        return odometry.trajectory_hip(rel) if self.on_hip else odometry.trajectory_numpy(rel.numpy())

    def run(self, dataset, sink, poses=None, frames=None, debug=None):
        """``poses``, ``frames``, ``debug``: SceneFuser.fuse's; the driver fills debug["depth"] and debug["poses"]."""
        host_frames = odometry.dataset_frames_u8(dataset)
        m = host_frames.shape[0]
        first, last = (0, m) if frames is None else (int(frames[0]), int(frames[1]))
        if not 0 <= first < last <= m:
            raise ValueError("frames: 0 <= first < last <= %d, got %r" % (m, frames))
        if sink.min_views and last - first < 2 * sink.radius + 1:
            raise ValueError("view_radius %d needs %d frames to fuse, got %d" % (sink.radius, 2 * sink.radius + 1, last - first))
        resident = host_frames.to(self.device)                                   # every frame: one upload, as bytes
        all_poses = self.camera_poses(dataset, resident, poses)
        self.poses = all_poses.cpu().numpy() if torch.is_tensor(all_poses) else np.array(all_poses)
        depths = None if debug is None else []
        with torch.no_grad():
            feed_frames(self.predict, sink, resident, all_poses, first, last, self.batch_size, self.on_hip and sink.min_views > 0, depths)
        if debug is not None:
            debug["depth"], debug["poses"] = torch.cat(depths), all_poses


class SceneFuser(SequenceDriver):
    """fuse(dataset, poses=None, frames=None) -> Cloud.

    model       a model of this build with a depth network and, for ``poses=None``, ``PoseEncoder`` / ``PoseDecoder``; it is never
                moved or changed (DepthPredictor and OdometryEvaluator work on their own copies where they must)
    height, width  the depth network's size; the depth maps come back at the dataset's frame size
    device      'cuda[:i]': the frames are uploaded once as uint8 (odometry.dataset_frames_u8); predicted poses go from
                OdometryEvaluator.relative_poses through trajectory_hip without visiting the host; per batch of ``batch_size`` frames:
                DepthPredictor (which wants HWC input: one permuted copy of the batch's frames), keys_hip, torch.sort, heads / cumsum
                / reduce, merge_hip into the running map, which stays sorted by key.  Memory: one batch of points plus the map.
                Two host synchronisations per batch (the voxel counts of the batch and of the merged map size their outputs).
                With ``min_views`` > 0 a sliding window of depth maps is held as well: every frame still goes through the depth
                network once, a frame is filtered and fused (keys_hip, views_hip on those keys, then the table and the merge as
                before) as soon as the last frame of its clamped window has been predicted, and at most batch_size + 2 view_radius
                depth maps are held from one batch to the next.  The cloud does not depend on ``batch_size``.
                'cpu': the host statements.
    voxel, min_depth, max_range  in the MODEL's units (the stereo baseline is 0.015 of them, x 36 gives metres); the defaults of these
                and of ``edge`` are UNTUNED starting values
    stride, border   use every stride-th pixel in x and y; drop ``border`` pixels at every image edge
    edge        flying-pixel filter: a pixel whose depth differs from a 4-neighbour's by more than edge x the smaller one is dropped
    min_count   drop voxels that fewer points fell into
    min_views, view_radius, view_tol   multi-view filter (0: off, and nothing of it runs): a pixel is kept only if at least min_views
                of its frame's 2 view_radius neighbouring frames (the window is shifted, not shortened, at the ends of the fused
                range ``frames``) see a depth within view_tol x the smaller of the two where the pixel's point projects into them;
                the defaults of view_radius and view_tol are UNTUNED.  Cloud.stats gains invalid_views; valid / (valid +
                invalid_views) is the share of pixels on which the frames agree, a figure of a checkpoint that needs no ground truth
    depth_scale, pose_scale  multiply the depths / the pose translations (ground-truth poses in metres: depth_scale = the model's
                unit in metres, ~36 for the reference's stereo-trained checkpoints)
    """

    def __init__(self, model, height, width, device, voxel=DEFAULT_VOXEL, batch_size=12, precision="fp32", stride=1, border=0,
                 min_depth=DEFAULT_MIN_DEPTH, max_range=DEFAULT_MAX_RANGE, edge=DEFAULT_EDGE, min_count=1, depth_scale=1.0,
                 pose_scale=1.0, post_process=False, min_views=0, view_radius=DEFAULT_VIEW_RADIUS, view_tol=DEFAULT_VIEW_TOL):
        _check_params(voxel, stride, border, min_depth, max_range, edge, min_count)
        _check_view_params(min_views, view_radius, view_tol)
        super().__init__(model, height, width, device, batch_size, precision, post_process)
        self.voxel, self.min_count = float(voxel), int(min_count)
        self.params = dict(stride=int(stride), border=int(border), min_depth=float(min_depth), max_range=float(max_range),
                           edge=float(edge), depth_scale=float(depth_scale), pose_scale=float(pose_scale))
        self.min_views = int(min_views)
        if self.min_views:                 # off: the parameters of the filter reach nothing
            self.params.update(min_views=self.min_views, view_radius=int(view_radius), view_tol=float(view_tol))

    def fuse(self, dataset, poses=None, frames=None, debug=None):
        """``poses``: any [n+1,3,4] camera-to-world array (KITTI ground truth with the user's depth_scale); None: the model's own.
        ``frames``: (first, last + 1) of the n+1 frames to fuse (poses are still computed from frame 0).  ``debug``: a dict that
        receives the "depth" maps [m,H,W] and the "poses" [n+1,3,4] that were fused and, with the multi-view filter on, the "votes"
        uint8 [m,H,W] of the pixels it tested (0 where a single-frame filter had dropped the pixel already).  The poses that were
        used stay in ``self.poses`` (float64 [n+1,3,4] on the host): what render.CloudRenderer needs to look at the cloud."""
        inv_K = dataset_inv_K(dataset)
        view_K = {"K": dataset_K(dataset)} if self.min_views else {}
        sink = _DeviceMap(self.device, inv_K, self.voxel, **self.params, **view_K, want_votes=debug is not None) if self.on_hip else \
            HostFrames(self.min_views, self.params.get("view_radius", DEFAULT_VIEW_RADIUS))
        self.run(dataset, sink, poses, frames, debug)
        if self.on_hip:
            if sink.kept_votes:
                debug["votes"] = torch.cat(sink.kept_votes)
            return sink.cloud(self.voxel, self.min_count)
        votes = {}
        cloud = fuse_numpy(*sink.arrays(), inv_K, self.voxel, min_count=self.min_count, debug=votes, **self.params, **view_K)
        if debug is not None and "votes" in votes:
            debug["votes"] = torch.from_numpy(votes["votes"])
        return cloud
