"""Truncated signed distance fusion: the depth maps and camera poses of a sequence fused into surface points with oriented normals.

cloud.py averages points per voxel: depth noise along the ray spreads one surface over several voxel layers, and the cloud keeps no
record of the side a surface was seen from.  Here every pixel adds a signed distance to the voxels its ray meets in a band around its
surface; the surface is where the averaged distance changes sign, and the gradient of that field is a normal that points at the
observer (Curless & Levoy 1996; KinectFusion).  The reference has no such program.

Scatter, not gather: a frame updates exactly the voxels its own rays sample, through the same store / sort / sum-per-destination chain
as cloud.py (td_cloud_heads, td_cloud_reduce_packed, merge_hip, all unchanged).  That chain's sums are linear in the payload's fields,
so a sample's distance rides in the 30 offset bits as an offset-binary integer v = q + 2^20, and sum v = sum q_x + 1024 sum q_y + 2^20
sum q_z.  Everything accumulated is an integer: the map is bit-identical from run to run and does not depend on how the sequence is
cut into batches or a batch's pairs into sub-chunks.

Three layers, as in cloud.py:
  * host statements in numpy (``samples_numpy``, ``surface_numpy``, ``fuse_tsdf_numpy``): the ``device='cpu'`` path and what the kernels
    are tested against, operation for operation; ``samples_bruteforce`` / ``surface_bruteforce`` (plain Python floats and a dict) pin them;
  * ``samples_hip``, ``surface_hip``, ``fuse_tsdf_hip`` (csrc/td_tsdf.hip): device tensors only, a CPU tensor is an error;
  * ``TsdfFuser``: frames of a dataset -> SceneFuser's depth and pose plumbing -> the surface;
  * the map ray-cast into camera views (``raycast_numpy``, pinned by ``raycast_bruteforce``; ``raycast_hip``: csrc/td_tsdf_cast.hip;
    ``TsdfCaster``), and the map on disk (``save_map`` / ``load_map``).

The exact arithmetic (float64; every operation rounded on its own).  A pixel is valid by td_cloud_keys' causes 1 ... 4 (cloud.py) and
then its mask.  ray, p: cloud.py's.  With half = voxel 0.5, trunc = float(T) voxel, scale = 1048576.0 / trunc, for s = -2T ... 2T:
    d_s = p_z + float(s) half;   f = d_s / ray_z;   sample_k = ray_k f
    world_k = ((r_k0 sample_x + r_k1 sample_y) + r_k2 sample_z) + pose_scale t_k;   g = world inv_voxel;   i = floor(g)
    skipped by the first rule that holds:  range: i outside [-2^20, 2^20) or the sentinel voxel;  duplicate: s > -2T and i is the
    voxel computed for slot s-1 (a ray meets a voxel in one interval, so equal voxels are consecutive);  band: not |sdf| <= trunc with
    e_k = (i_k + 0.5) voxel - pose_scale t_k;   z_c = (r_02 e_0 + r_12 e_1) + r_22 e_2;   sdf = p_z - z_c
    q = rint(sdf scale) clamped to [-2^20, 2^20];   payload = (q + 2^20) | r << 30 | g << 38 | b << 46
This is a defined sampling at half-voxel steps of depth along the ray, not a voxel traversal: a voxel whose corner the ray clips
between two samples is missed.  sdf is projective (along the camera's z), positive between the camera and the surface.
A voxel's row: w = count, S = (sum q_x + 1024 sum q_y + 2^20 sum q_z) - 2^20 w (exact), D = S / w in units of trunc / 2^20.  The
surface (``surface_numpy``'s docstring) lies on the +x / +y / +z edges between voxels of weight >= min_weight whose S differ in sign.

The ray cast (the other half of KinectFusion: a GATHER over the map; float64, every operation rounded on its own).  A voxel qualifies
when w >= min_weight; its value is D = float64(S) / float64(w), its colour (2 sum_c + w) // (2 w), as in ``surface_numpy``.  Per
camera [R|t] and pixel (x, y), with ray = cloud.py's, step = step_voxels voxel, n_steps = floor((far - near) / step) + 1 (refused
above CAST_MAX_STEPS), for s = 0 ... n_steps-1:
    z_s = near + float(s) step;   f = z_s / ray_z;   sample_k = ray_k f;   world = camera_to_world(sample) as above;   g = world inv_voxel
    corners(g):  h_k = g_k - 0.5;   i_k = floor(h_k);   f_k = h_k - i_k   (voxel centres sit at i + 0.5)
        known when every i_k lies in [-2^20, 2^20 - 1) (a NaN or an inf fails; the +1 neighbour of a field's last coordinate does not
        exist, nothing is carried into the next field) and all eight voxels i + {0,1}^3 are in the map, qualify and are not the
        sentinel voxel.  z is the low key field: the +z corner of a column is the next row.
    value:  along z  c_xy = D_xy0 + f_z (D_xy1 - D_xy0);   along y  c_x = c_x0 + f_y (c_x1 - c_x0);   along x  v = c_0 + f_x (c_1 - c_0)
    walking s upwards, prev = sample s-1 if it was known (an unknown sample breaks the pair):
        hit:        prev known, v_prev >= 0 and v < 0:   t = v_prev / (v_prev - v);   z_hit = z_(s-1) + t step;   the ray ends
        back face:  prev known, v_prev < 0 and v >= 0:   the ray ends without a hit (the surface is seen from behind)
        a ray that runs out of samples is a miss
At a hit depth = float32(z_hit); g_hit is computed from z_hit as a sample's g from z_s, and its corners are fetched again.  The
gradient of the trilinear interpolant, with e the differences of D along the gradient's own axis:
    d/dx:  e_yz = D_1yz - D_0yz;   along z  a_y = e_y0 + f_z (e_y1 - e_y0);   along y  G_0 = a_0 + f_y (a_1 - a_0)
    d/dy:  e_xz = D_x1z - D_x0z;   along z  a_x = e_x0 + f_z (e_x1 - e_x0);   along x  G_1 = a_0 + f_x (a_1 - a_0)
    d/dz:  e_xy = D_xy1 - D_xy0;   along y  a_x = e_x0 + f_y (e_x1 - e_x0);   along x  G_2 = a_0 + f_x (a_1 - a_0)
    |G| = sqrt((G_0 G_0 + G_1 G_1) + G_2 G_2);   n = G / |G|;   m_k = (R_0k n_0 + R_1k n_1) + R_2k n_2;   normal = float32(m)
D is positive on the observer's side: m faces where the surface was SEEN from and is not turned towards the viewer.  Where the
corners of g_hit are not all known, or |G| is not > 0, the normal is (0, 0, 0) and the pixel counts under hits_without_normal.  The
colour and the weight (w, saturating at int32) are those of the voxel floor(g_hit): corner c_k = 0 if floor(g_k) = i_k, else 1
(floor(g_k) is i_k or i_k + 1, because g_k - 0.5 is rounded monotonically and floor(g_k) +- 0.5 is exact).  Where the corners of
g_hit are not all known the corner set of sample s is used instead, by the same rule on g_s: sample s is known, lies at most one
step behind the surface, and so always names a voxel that exists (the choice between s-1 and s is arbitrary; s is the one on the
surface's far side, where the colours of a band were sampled as well).  No hit: depth 0, normal 0, the background colour, weight 0.
Per view: rays = hits + backface + misses, and hits_without_normal (CAST_STATS).  Limits: perspective only; the band is T voxels on
either side, so a camera that stands inside a band, or behind a surface, sees a back face or nothing; a ray that crosses the
interpolant's zero set twice inside one step sees neither crossing.
"""
import collections
import io
import math
import zipfile

import numpy as np
import torch

from . import cloud, native, render
from .cloud import HALF, INVALID_KEY

MAX_T = native.CONSTANTS["TD_TSDF_MAX_T"]
ONE = 1 << 20                          # trunc as an integer
SAMPLE_STATS = ("valid", "invalid_stride", "invalid_border", "invalid_depth", "invalid_edge", "invalid_mask", "samples",
                "skipped_duplicate", "skipped_band", "skipped_range")
SURFACE_STATS = ("voxels_under_min_weight", "crossings_x", "crossings_y", "crossings_z", "crossings_without_normal")
CAST_STATS = ("rays", "hits", "backface", "misses", "hits_without_normal")
CAST_MAX_STEPS = native.CONSTANTS["TD_TSDF_CAST_MAX_STEPS"]      # a guard against a runaway launch, not a tuning value
assert len(SAMPLE_STATS) == native.CONSTANTS["TD_TSDF_SAMPLE_STATS"] and len(SURFACE_STATS) == native.CONSTANTS["TD_TSDF_SURFACE_STATS"]
assert len(CAST_STATS) == native.CONSTANTS["TD_TSDF_CAST_STATS"]

# UNTUNED starting values: nobody has looked at a surface of a trained checkpoint with them.
DEFAULT_TRUNC_VOXELS = 3
DEFAULT_MIN_WEIGHT = 2
DEFAULT_PAIR_CHUNK = 1 << 25           # pairs sorted at a time (16 bytes each, and the sort's own buffers)
DEFAULT_STEP_VOXELS = 0.5              # the ray cast's step along the camera's z, in voxels.  UNTUNED like the rest

Surface = collections.namedtuple("Surface", "xyz normal rgb weight stats")
Cast = collections.namedtuple("Cast", "depth normal color weight stats")
Cast.__doc__ = """depth float32 [C,H,W] (float32(z_hit), 0 where the ray did not hit), normal float32 [C,3,H,W] (unit, in the camera's
frame, facing where the surface was seen from; (0, 0, 0): none), color uint8 [C,3,H,W] (the background where the ray did not hit),
weight int32 [C,H,W] (the hit voxel's sample count, saturating; 0: no hit), stats int64 [C,5] in the order of CAST_STATS."""

Surface.__doc__ = """xyz float32 [n,3], normal float32 [n,3] (unit, facing where the surface was seen from; (0, 0, 0): none), rgb uint8
[n,3], weight int32 [n] (the smaller sample count of the edge's two voxels, saturating), in (voxel, axis) order of the key-sorted map,
on the fuser's device (numpy arrays on the host path);  stats: dict of Python ints: points (pixels seen), SAMPLE_STATS, voxels,
SURFACE_STATS, surface_points."""


def _check(T, voxel, min_weight=1, pair_chunk=1):
    if not 1 <= int(T) <= MAX_T:
        raise ValueError("trunc_voxels: 1 ... %d, got %r" % (MAX_T, T))
    if not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel: a positive size, got %r" % (voxel,))
    if int(min_weight) < 1:
        raise ValueError("min_weight: at least 1, got %r" % (min_weight,))
    if int(pair_chunk) < 1:
        raise ValueError("pair_chunk: at least 1, got %r" % (pair_chunk,))


def row_sdf_sum(sums):
    """int64 rows [V,7] -> S int64 [V] = (sum q_x + 1024 sum q_y + 2^20 sum q_z) - 2^20 count, exact."""
    s = np.asarray(sums, np.int64).reshape(-1, 7)
    return (s[:, 1] + 1024 * s[:, 2] + ONE * s[:, 3]) - ONE * s[:, 0]


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def samples_numpy(depth, color, poses, inv_K, T, voxel, mask=None, depth_scale=1.0, pose_scale=1.0, stride=1, border=0,
                  min_depth=cloud.DEFAULT_MIN_DEPTH, max_range=cloud.DEFAULT_MAX_RANGE, edge=0.0):
    """depth float32 [B,H,W], color uint8 [B,3,H,W], poses float64 [B,3,4], mask [B,H,W] (0 drops the pixel) or None -> (key int64
    [(4T+1) B H W], payload uint64 [(4T+1) B H W], slot-major, counts int64 [10] in the order of SAMPLE_STATS).  The statement
    td_tsdf_samples is tested against, operation for operation (the module's docstring)."""
    d, c, P = cloud._check_frames(depth, color, poses, device=False)
    _check(T, voxel)
    T = int(T)
    m = cloud._inv_K9(inv_K)
    B, H, W = d.shape
    voxel, depth_scale, pose_scale = np.float64(voxel), np.float64(depth_scale), np.float64(pose_scale)
    inv_voxel = np.float64(1.0 / float(voxel))
    cause = cloud.pixel_causes_numpy(d, depth_scale, stride, border, min_depth, max_range, edge)
    if mask is not None:
        mk = np.asarray(mask)
        if mk.shape != d.shape:
            raise ValueError("mask: %s like the depth, got %s" % (d.shape, mk.shape))
        cause[(cause == 0) & (mk == 0)] = 5
    ok = cause == 0
    counts = np.zeros(len(SAMPLE_STATS), np.int64)
    counts[:6] = np.bincount(cause.reshape(-1), minlength=6)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = [(m[3 * k] * u + m[3 * k + 1] * v) + m[3 * k + 2] for k in range(3)]
    R = [[P[:, k, j].reshape(B, 1, 1) for j in range(4)] for k in range(3)]
    rgb = (c[:, 0].astype(np.uint64) << np.uint64(30)) | (c[:, 1].astype(np.uint64) << np.uint64(38)) | (c[:, 2].astype(np.uint64) << np.uint64(46))
    half = voxel * np.float64(0.5)
    trunc = np.float64(T) * voxel
    scale = np.float64(1048576.0) / trunc
    keys, payloads = [], []
    prev = np.full(d.shape, INVALID_KEY, np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pz = (d.astype(np.float64) * depth_scale) * ray[2]
        for s in range(-2 * T, 2 * T + 1):
            dz = pz + np.float64(s) * half
            f = dz / ray[2]
            sample = [ray[k] * f for k in range(3)]
            g = [(((R[k][0] * sample[0] + R[k][1] * sample[1]) + R[k][2] * sample[2]) + pose_scale * R[k][3]) * inv_voxel for k in range(3)]
            key = cloud.grid_keys_numpy(g)[0]
            out_of_range = ok & (key == INVALID_KEY)
            duplicate = ok & ~out_of_range & (key == prev) if s > -2 * T else np.zeros(d.shape, bool)
            rest = ok & ~out_of_range & ~duplicate
            e = [(np.floor(g[k]) + 0.5) * voxel - pose_scale * R[k][3] for k in range(3)]
            zc = (R[0][2] * e[0] + R[1][2] * e[1]) + R[2][2] * e[2]
            sdf = pz - zc
            inside = rest & (np.abs(sdf) <= trunc)
            q = np.clip(np.rint(np.where(inside, sdf * scale, 0.0)), -ONE, ONE).astype(np.int64)
            keys.append(np.where(inside, key, INVALID_KEY).astype(np.int64).reshape(-1))
            payloads.append(np.where(inside, (q + ONE).astype(np.uint64) | rgb, np.uint64(0)).astype(np.uint64).reshape(-1))
            counts[6] += inside.sum()
            counts[7] += duplicate.sum()
            counts[8] += (rest & ~inside).sum()
            counts[9] += out_of_range.sum()
            prev = np.where(ok, key, prev)
    return np.concatenate(keys), np.concatenate(payloads), counts


def _neighbour_numpy(keys, axis, direction):
    """The index of every voxel's neighbour one step along ``axis`` in ``direction`` = +-1 in the ascending unique ``keys``, -1 where
    there is none.  The coordinate field is tested first: nothing is carried into the next field."""
    shift = (42, 21, 0)[axis]
    mask = 2 * HALF - 1
    field = (keys >> shift) & mask
    edge = field == (mask if direction > 0 else 0)
    kb = np.where(edge, 0, keys + direction * (1 << shift))
    edge |= kb == INVALID_KEY
    at = np.searchsorted(keys, kb)
    found = ~edge & (at < len(keys))
    found &= keys[np.minimum(at, max(len(keys) - 1, 0))] == kb
    return np.where(found, at, -1)


def surface_numpy(keys, sums, voxel, min_weight=DEFAULT_MIN_WEIGHT):
    """keys int64 [V] ascending and unique, sums int64 [V,7] -> (xyz float32 [V,3,3], normal float32 [V,3,3], rgb uint8 [V,3,3], weight
    int32 [V,3], mask bool [V,3], counts int64 [5] in the order of SURFACE_STATS): slot (a, axis) holds the crossing on the edge from
    voxel a one step up the axis; where mask is False the slot is zero.  The statement td_tsdf_surface is tested against.

    D = float64(S) / float64(w).  A voxel qualifies when w >= min_weight.  The edge a -> b crosses when both exist and qualify and
    (S_a >= 0) != (S_b >= 0) (integers; zero counts as positive).  Then t = D_a / (D_a - D_b); the point is (i_a + 0.5) voxel, on the
    edge's axis ((i_a + 0.5) + t) voxel, as float32; the colour is the rounded mean colour of a if t < 0.5, else of b; the weight is
    min(w_a, w_b), saturating; the normal is g / |g| with g = (1.0 - t) g_a + t g_b, |g| = sqrt((g_0 g_0 + g_1 g_1) + g_2 g_2), and the
    gradient of D at a voxel is per axis (D_+ - D_-) / 2.0 where both neighbours qualify, D_+ - D or D - D_- where one does, else 0.
    D is positive on the camera's side, so the normal faces where the surface was seen from."""
    keys, sums = np.asarray(keys, np.int64).reshape(-1), np.asarray(sums, np.int64).reshape(-1, 7)
    _check(1, voxel, min_weight)
    V = len(keys)
    if len(sums) != V or (V > 1 and not np.all(np.diff(keys) > 0)):
        raise ValueError("keys [V] ascending and unique, sums [V,7]")
    voxel = np.float64(voxel)
    xyz, normal = np.zeros((V, 3, 3), np.float32), np.zeros((V, 3, 3), np.float32)
    rgb, weight, mask = np.zeros((V, 3, 3), np.uint8), np.zeros((V, 3), np.int32), np.zeros((V, 3), bool)
    counts = np.zeros(len(SURFACE_STATS), np.int64)
    if V == 0:
        return xyz, normal, rgb, weight, mask, counts
    w, S = sums[:, 0], row_sdf_sum(sums)
    qualifies = w >= int(min_weight)
    counts[0] = (~qualifies).sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        D = S.astype(np.float64) / w.astype(np.float64)
        G = np.zeros((V, 3))
        up = []
        for axis in range(3):
            p, m = _neighbour_numpy(keys, axis, 1), _neighbour_numpy(keys, axis, -1)
            up.append(p)
            hp, hm = (p >= 0) & qualifies[np.maximum(p, 0)], (m >= 0) & qualifies[np.maximum(m, 0)]
            Dp, Dm = D[np.maximum(p, 0)], D[np.maximum(m, 0)]
            G[:, axis] = np.where(hp & hm, (Dp - Dm) / 2.0, np.where(hp, Dp - D, np.where(hm, D - Dm, 0.0)))
        i = np.stack(cloud.unpack_key(keys), -1).astype(np.float64)
        colour = ((2 * sums[:, 4:7] + w[:, None]) // np.maximum(2 * w[:, None], 1)).astype(np.uint8)
        for axis in range(3):
            b = np.maximum(up[axis], 0)
            cross = (up[axis] >= 0) & qualifies & qualifies[b] & ((S >= 0) != (S[b] >= 0))
            t = np.where(cross, D / (D - D[b]), 0.0)
            g = [(1.0 - t) * G[:, k] + t * G[b, k] for k in range(3)]
            norm = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            has = cross & (norm > 0.0)
            for k in range(3):
                normal[:, axis, k] = np.where(has, g[k] / norm, 0.0).astype(np.float32)
                centre = i[:, k] + 0.5
                xyz[:, axis, k] = np.where(cross, ((centre + t) if k == axis else centre) * voxel, 0.0).astype(np.float32)
            rgb[:, axis] = np.where(cross[:, None], np.where((t < 0.5)[:, None], colour, colour[b]), 0)
            weight[:, axis] = np.where(cross, np.minimum(np.minimum(w, w[b]), 0x7fffffff), 0).astype(np.int32)
            mask[:, axis] = cross
            counts[1 + axis] = cross.sum()
            counts[4] += (cross & ~has).sum()
    return xyz, normal, rgb, weight, mask, counts


def _stats(sample_counts, voxels, surface_counts, n_points):
    out = {"points": int(np.sum(sample_counts[:6]))}
    out.update({name: int(v) for name, v in zip(SAMPLE_STATS, sample_counts)})
    out["voxels"] = int(voxels)
    out.update({name: int(v) for name, v in zip(SURFACE_STATS, surface_counts)})
    out["surface_points"] = int(n_points)
    return out


def _view_mask_numpy(depth, poses, inv_K, K, min_views, view_radius, view_tol, depth_scale, pose_scale, min_depth, max_range, mask):
    """The multi-view filter as a per-pixel mask: cloud.views_numpy's votes >= min_views, and the caller's mask."""
    votes = cloud.views_numpy(depth, poses, inv_K, cloud._view_K9(K, inv_K), view_radius, view_tol, depth_scale, pose_scale, min_depth,
                              max_range)
    keep = votes >= int(min_views)
    return keep if mask is None else keep & (np.asarray(mask) != 0)


def fuse_tsdf_numpy(depth, color, poses, inv_K, voxel=cloud.DEFAULT_VOXEL, trunc_voxels=DEFAULT_TRUNC_VOXELS,
                    min_weight=DEFAULT_MIN_WEIGHT, stride=1, border=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                    max_range=cloud.DEFAULT_MAX_RANGE, edge=0.0, depth_scale=1.0, pose_scale=1.0, mask=None, min_views=0,
                    view_radius=cloud.DEFAULT_VIEW_RADIUS, view_tol=cloud.DEFAULT_VIEW_TOL, K=None, debug=None):
    """All frames at once -> Surface of numpy arrays: samples_numpy (with ``min_views`` > 0 behind the mask votes >= min_views of
    cloud.views_numpy over all frames), cloud.voxel_table_numpy, surface_numpy, then a boolean select in (voxel, axis) order.
    ``debug``: a dict that receives the map's "keys" and "sums"."""
    cloud._check_params(voxel, stride, border, min_depth, max_range, edge)
    cloud._check_view_params(min_views, view_radius, view_tol)
    _check(trunc_voxels, voxel, min_weight)
    if min_views > 0:
        mask = _view_mask_numpy(depth, poses, inv_K, K, min_views, view_radius, view_tol, depth_scale, pose_scale, min_depth, max_range, mask)
    key, payload, counts = samples_numpy(depth, color, poses, inv_K, trunc_voxels, voxel, mask, depth_scale, pose_scale, stride, border,
                                         min_depth, max_range, edge)
    keys, sums = cloud.voxel_table_numpy(key, payload)
    if debug is not None:
        debug["keys"], debug["sums"] = keys, sums
    xyz, normal, rgb, weight, hit, scounts = surface_numpy(keys, sums, voxel, min_weight)
    return Surface(xyz[hit], normal[hit], rgb[hit], weight[hit], _stats(counts, len(keys), scounts, int(hit.sum())))


# ---------------------------------------------------------------------------------------------------------------------------
# the literal brute forces: plain Python floats (IEEE float64, one rounding per operation) and a dict

def samples_bruteforce(depth, color, poses, inv_K, T, voxel, mask=None, depth_scale=1.0, pose_scale=1.0, stride=1, border=0, min_depth=0.1,
                       max_range=1.0, edge=0.0):
    """One pixel and one slot at a time -> (table: dict (ix, iy, iz) -> [count, sum of v = q + 2^20, sum r, sum g, sum b], counts list
    [10] in the order of SAMPLE_STATS).  float32 only where the edge filter compares depths."""
    B, H, W = depth.shape
    m = [float(x) for x in np.asarray(inv_K, np.float64)[:3, :3].reshape(-1)]
    voxel, depth_scale, pose_scale = float(voxel), float(depth_scale), float(pose_scale)
    inv_voxel = 1.0 / voxel
    half, trunc = voxel * 0.5, float(T) * voxel
    scale = 1048576.0 / trunc
    table, counts = {}, [0] * len(SAMPLE_STATS)
    for b in range(B):
        P = [[float(x) for x in row] for row in poses[b]]
        for y in range(H):
            for x in range(W):
                d32 = depth[b, y, x]
                ds = float(d32) * depth_scale
                if x % stride or y % stride:
                    counts[1] += 1
                    continue
                if x < border or x >= W - border or y < border or y >= H - border:
                    counts[2] += 1
                    continue
                if not math.isfinite(float(d32)) or not (min_depth <= ds <= max_range):
                    counts[3] += 1
                    continue
                if edge > 0:
                    bad = False
                    for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                        if 0 <= yy < H and 0 <= xx < W:
                            nb = depth[b, yy, xx]
                            if not math.isfinite(float(nb)) or np.float32(abs(np.float32(d32 - nb))) > np.float32(edge) * min(d32, nb):
                                bad = True
                    if bad:
                        counts[4] += 1
                        continue
                if mask is not None and not mask[b, y, x]:
                    counts[5] += 1
                    continue
                counts[0] += 1
                u, v = float(x), float(y)
                ray = [(m[3 * k] * u + m[3 * k + 1] * v) + m[3 * k + 2] for k in range(3)]
                pz = ds * ray[2]
                prev = None
                for s in range(-2 * T, 2 * T + 1):
                    dz = pz + float(s) * half
                    try:
                        f = dz / ray[2]
                    except ZeroDivisionError:
                        f = math.nan
                    sample = [r * f for r in ray]
                    g = [(((P[k][0] * sample[0] + P[k][1] * sample[1]) + P[k][2] * sample[2]) + pose_scale * P[k][3]) * inv_voxel
                         for k in range(3)]
                    if not all(math.isfinite(t) and -HALF <= math.floor(t) < HALF for t in g):
                        counts[9] += 1
                        prev = None
                        continue
                    i = tuple(int(math.floor(t)) for t in g)
                    if i == (HALF - 1,) * 3:
                        counts[9] += 1
                        prev = None
                        continue
                    if i == prev:
                        counts[7] += 1
                        continue
                    prev = i
                    e = [(float(i[k]) + 0.5) * voxel - pose_scale * P[k][3] for k in range(3)]
                    zc = (P[0][2] * e[0] + P[1][2] * e[1]) + P[2][2] * e[2]
                    sdf = pz - zc
                    if not abs(sdf) <= trunc:
                        counts[8] += 1
                        continue
                    q = max(-ONE, min(ONE, int(round(sdf * scale))))          # round: half to even, as rint
                    row = table.setdefault(i, [0] * 5)
                    row[0] += 1
                    row[1] += q + ONE
                    for ch in range(3):
                        row[2 + ch] += int(color[b, ch, y, x])
                    counts[6] += 1
    return table, counts


def surface_bruteforce(table, voxel, min_weight):
    """table: dict (ix, iy, iz) -> (w, S, sum r, sum g, sum b) with S the exact summed distance -> a list, in (voxel, axis) order of the
    sorted voxels, of (xyz float32 x 3, normal float32 x 3, rgb x 3, weight), and the counts [5] in the order of SURFACE_STATS."""
    voxel = float(voxel)
    good = lambda c: c in table and table[c][0] >= min_weight
    D = lambda c: float(table[c][1]) / float(table[c][0])
    step = lambda c, axis, by: tuple(c[k] + (by if k == axis else 0) for k in range(3))

    def gradient(c):
        g = []
        for axis in range(3):
            p, m = step(c, axis, 1), step(c, axis, -1)
            if good(p) and good(m):
                g.append((D(p) - D(m)) / 2.0)
            elif good(p):
                g.append(D(p) - D(c))
            elif good(m):
                g.append(D(c) - D(m))
            else:
                g.append(0.0)
        return g

    out, counts = [], [0] * len(SURFACE_STATS)
    for a in sorted(table):
        if not good(a):
            counts[0] += 1
            continue
        for axis in range(3):
            b = step(a, axis, 1)
            if not good(b) or (table[a][1] >= 0) == (table[b][1] >= 0):
                continue
            t = D(a) / (D(a) - D(b))
            ga, gb = gradient(a), gradient(b)
            g = [(1.0 - t) * ga[k] + t * gb[k] for k in range(3)]
            norm = math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            n = [np.float32(g[k] / norm) if norm > 0.0 else np.float32(0.0) for k in range(3)]
            counts[4] += norm == 0.0
            p = [np.float32((((float(a[k]) + 0.5) + t) if k == axis else (float(a[k]) + 0.5)) * voxel) for k in range(3)]
            c = table[a] if t < 0.5 else table[b]
            rgb = [(2 * c[2 + k] + c[0]) // (2 * c[0]) for k in range(3)]
            out.append((p, n, rgb, min(table[a][0], table[b][0], 0x7fffffff)))
            counts[1 + axis] += 1
    return out, counts


# ---------------------------------------------------------------------------------------------------------------------------
# the ray cast: host statements

def _check_cast(height, width, voxel, min_weight, near, far, step_voxels, background=(0, 0, 0)):
    """-> (step, n_steps, background): step = step_voxels voxel, n_steps = floor((far - near) / step) + 1, float64."""
    bg = render._check_params(height, width, near, far, 0.0, background)
    _check(1, voxel, min_weight)
    if not (np.isfinite(step_voxels) and step_voxels > 0):
        raise ValueError("step_voxels: a positive step, got %r" % (step_voxels,))
    step = float(step_voxels) * float(voxel)
    steps = math.floor((float(far) - float(near)) / step) + 1.0 if step > 0 else math.inf
    if not steps <= CAST_MAX_STEPS:
        raise ValueError("near %r ... far %r in steps of %r: more than %d samples per ray" % (near, far, step, CAST_MAX_STEPS))
    return step, int(steps), bg


def _check_map(keys, sums):
    keys, sums = np.ascontiguousarray(keys, np.int64).reshape(-1), np.ascontiguousarray(sums, np.int64).reshape(-1, 7)
    if len(sums) != len(keys) or (len(keys) > 1 and not np.all(np.diff(keys) > 0)):
        raise ValueError("keys [V] ascending and unique, sums [V,7]")
    return keys, sums


def _cast_poses(poses):
    """float64 [C,3,4] (or [C,4,4], whose top rows are used) with C >= 1, contiguous; no view is a ValueError on every path."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim == 3 and poses.shape[1:] == (4, 4):
        poses = poses[:, :3]
    if poses.ndim != 3 or poses.shape[1:] != (3, 4) or not len(poses):
        raise ValueError("poses [C,3,4] camera-to-world with C >= 1, got %s" % (poses.shape,))
    return np.ascontiguousarray(poses)


def _corners_numpy(keys, qualifies, g):
    """g: three float64 arrays [n] -> (known bool [n], rows int64 [n,8] in (dx, dy, dz) order, f: three float64 [n], i: three float64
    [n]): the module docstring's corners(g).  Rows are meaningful where known."""
    V, n = len(keys), len(g[0])
    with np.errstate(invalid="ignore", over="ignore"):
        h = [v - 0.5 for v in g]
        i = [np.floor(v) for v in h]
        f = [a - b for a, b in zip(h, i)]
        known = np.ones(n, bool)
        for v in i:
            known &= (v >= -float(HALF)) & (v < float(HALF - 1))
    rows = np.zeros((n, 8), np.int64)
    if V == 0:
        return np.zeros(n, bool), rows, f, i
    ii = [np.where(known, v, 0.0).astype(np.int64) for v in i]
    for dx in (0, 1):
        for dy in (0, 1):
            kb = cloud._pack(ii[0] + dx, ii[1] + dy, ii[2])
            at = np.searchsorted(keys, kb)
            lo, up = np.minimum(at, V - 1), np.minimum(at + 1, V - 1)
            known &= (at < V) & (keys[lo] == kb) & qualifies[lo]
            known &= (at + 1 < V) & (keys[up] == kb + 1) & (kb + 1 != INVALID_KEY) & qualifies[up]
            rows[:, (dx * 2 + dy) * 2], rows[:, (dx * 2 + dy) * 2 + 1] = lo, up
    return known, rows, f, i


def _lerp(a, b, f):
    return a + f * (b - a)


def _trilinear(d, f):
    """d: the eight corner values in (dx, dy, dz) order, f = (f_x, f_y, f_z): along z, then y, then x."""
    c = [_lerp(d[2 * j], d[2 * j + 1], f[2]) for j in range(4)]
    return _lerp(_lerp(c[0], c[1], f[1]), _lerp(c[2], c[3], f[1]), f[0])


def _trilinear_gradient(d, f):
    """The gradient of _trilinear's interpolant, in the module docstring's order."""
    ex = [d[4 + j] - d[j] for j in range(4)]                                   # e_yz
    ey = [d[2] - d[0], d[3] - d[1], d[6] - d[4], d[7] - d[5]]                  # e_xz
    ez = [d[2 * j + 1] - d[2 * j] for j in range(4)]                           # e_xy
    return (_lerp(_lerp(ex[0], ex[1], f[2]), _lerp(ex[2], ex[3], f[2]), f[1]),
            _lerp(_lerp(ey[0], ey[1], f[2]), _lerp(ey[2], ey[3], f[2]), f[0]),
            _lerp(_lerp(ez[0], ez[1], f[1]), _lerp(ez[2], ez[3], f[1]), f[0]))


def raycast_numpy(keys, sums, poses, inv_K, height, width, voxel, min_weight=DEFAULT_MIN_WEIGHT, near=render.DEFAULT_NEAR,
                  far=render.DEFAULT_FAR, step_voxels=DEFAULT_STEP_VOXELS, pose_scale=1.0, background=(0, 0, 0)):
    """keys int64 [V] ascending and unique, sums int64 [V,7], poses float64 [C,3,4] camera-to-world, inv_K: the 3x3 block -> Cast of
    numpy arrays.  The statement td_tsdf_cast is tested against, operation for operation (the module's docstring): vectorised over a
    view's pixels, a loop over the samples that ends when every ray has ended."""
    H, W = int(height), int(width)
    step, n_steps, bg = _check_cast(H, W, voxel, min_weight, near, far, step_voxels, background)
    keys, sums = _check_map(keys, sums)
    P_all, m = _cast_poses(poses), cloud._inv_K9(inv_K)
    C, n = len(P_all), H * W
    near, step, ps = np.float64(near), np.float64(step), np.float64(pose_scale)
    inv_voxel = np.float64(1.0 / float(voxel))
    w, S = sums[:, 0], row_sdf_sum(sums)
    qualifies = w >= int(min_weight)
    with np.errstate(invalid="ignore", divide="ignore"):
        D = S.astype(np.float64) / w.astype(np.float64)
    colour = ((2 * sums[:, 4:7] + w[:, None]) // np.maximum(2 * w[:, None], 1)).astype(np.uint8)
    weight_of = np.minimum(w, 0x7fffffff).astype(np.int32)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = [((m[3 * k] * u + m[3 * k + 1] * v) + m[3 * k + 2]).reshape(-1) for k in range(3)]
    depth, normal = np.zeros((C, n), np.float32), np.zeros((C, 3, n), np.float32)
    color, weight = np.empty((C, 3, n), np.uint8), np.zeros((C, n), np.int32)
    color[:] = np.array(bg, np.uint8).reshape(1, 3, 1)
    stats = np.zeros((C, len(CAST_STATS)), np.int64)

    def grid(P, z, sel):
        with np.errstate(all="ignore"):
            f = z / ray[2][sel]
            sample = [ray[k][sel] * f for k in range(3)]
            return [(((P[k, 0] * sample[0] + P[k, 1] * sample[1]) + P[k, 2] * sample[2]) + ps * P[k, 3]) * inv_voxel for k in range(3)]

    def pick(g, i, rows):
        """The row of the voxel floor(g) among the corners."""
        with np.errstate(invalid="ignore"):
            c = [(np.floor(a) != b).astype(np.int64) for a, b in zip(g, i)]
        return rows[np.arange(len(rows)), (c[0] * 2 + c[1]) * 2 + c[2]]

    for c in range(C):
        P = P_all[c]
        alive = np.arange(n)
        prev_known, v_prev = np.zeros(n, bool), np.zeros(n)
        hit_s, z_hit = np.full(n, -1, np.int64), np.zeros(n)
        for s in range(n_steps):
            if not len(alive):
                break
            z = near + np.float64(s) * step
            known, rows, f, _ = _corners_numpy(keys, qualifies, grid(P, z, alive))
            val = _trilinear([D[rows[:, j]] for j in range(8)], f) if len(keys) else np.zeros(len(alive))
            pk, vp = prev_known[alive], v_prev[alive]
            hit = known & pk & (vp >= 0.0) & (val < 0.0)
            back = known & pk & (vp < 0.0) & (val >= 0.0)
            with np.errstate(all="ignore"):
                t = np.where(hit, vp / (vp - val), 0.0)
            z_hit[alive[hit]] = ((near + np.float64(s - 1) * step) + t * step)[hit]
            hit_s[alive[hit]] = s
            stats[c, 2] += back.sum()
            prev_known[alive], v_prev[alive] = known, np.where(known, val, 0.0)
            alive = alive[~(hit | back)]
        sel = np.nonzero(hit_s >= 0)[0]
        stats[c, 0], stats[c, 1] = n, len(sel)
        stats[c, 3] = n - stats[c, 1] - stats[c, 2]
        if not len(sel):
            continue
        g_hit = grid(P, z_hit[sel], sel)
        known, rows, f, i = _corners_numpy(keys, qualifies, g_hit)
        G = _trilinear_gradient([D[rows[:, j]] for j in range(8)], f)
        with np.errstate(all="ignore"):
            norm = np.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
            has = known & (norm > 0.0)
            unit = [np.where(has, a / norm, 0.0) for a in G]
            for k in range(3):
                normal[c, k, sel] = np.where(has, (P[0, k] * unit[0] + P[1, k] * unit[1]) + P[2, k] * unit[2], 0.0).astype(np.float32)
        stats[c, 4] = (~has).sum()
        g_s = grid(P, near + hit_s[sel].astype(np.float64) * step, sel)
        _, rows_s, _, i_s = _corners_numpy(keys, qualifies, g_s)                # known: the hit says so
        row = np.where(known, pick(g_hit, i, rows), pick(g_s, i_s, rows_s))
        depth[c, sel] = z_hit[sel].astype(np.float32)
        color[c][:, sel] = colour[row].T
        weight[c, sel] = weight_of[row]
    return Cast(depth.reshape(C, H, W), normal.reshape(C, 3, H, W), color.reshape(C, 3, H, W), weight.reshape(C, H, W), stats)


def raycast_bruteforce(table, poses, inv_K, height, width, voxel, min_weight=DEFAULT_MIN_WEIGHT, near=render.DEFAULT_NEAR,
                       far=render.DEFAULT_FAR, step_voxels=DEFAULT_STEP_VOXELS, pose_scale=1.0, background=(0, 0, 0)):
    """raycast_numpy said a second time, independently: ``table`` is surface_bruteforce's dict (ix, iy, iz) -> (w, S, sum r, sum g, sum b);
    one pixel and one sample at a time in plain Python floats -> Cast of numpy arrays.  It pins the statement."""
    H, W = int(height), int(width)
    step, n_steps, bg = _check_cast(H, W, voxel, min_weight, near, far, step_voxels, background)
    poses = _cast_poses(poses)
    m = [float(x) for x in cloud._inv_K9(inv_K)]
    near, ps, inv_voxel = float(near), float(pose_scale), 1.0 / float(voxel)
    sentinel = (HALF - 1,) * 3
    C = len(poses)
    depth, normal = np.zeros((C, H, W), np.float32), np.zeros((C, 3, H, W), np.float32)
    color, weight = np.empty((C, 3, H, W), np.uint8), np.zeros((C, H, W), np.int32)
    color[:] = np.array(bg, np.uint8).reshape(1, 3, 1, 1)
    stats = np.zeros((C, len(CAST_STATS)), np.int64)

    def good(cell):
        return all(-HALF <= v < HALF for v in cell) and cell != sentinel and cell in table and table[cell][0] >= min_weight

    def grid(P, ray, z):
        try:
            f = z / ray[2]
        except ZeroDivisionError:
            f = math.nan
        sample = [r * f for r in ray]
        return [(((P[k][0] * sample[0] + P[k][1] * sample[1]) + P[k][2] * sample[2]) + ps * P[k][3]) * inv_voxel for k in range(3)]

    def corners(g):
        """-> (cells in (dx, dy, dz) order, f) or None."""
        h = [v - 0.5 for v in g]
        if not all(math.isfinite(v) for v in h):
            return None
        i = [math.floor(v) for v in h]
        cells = [(i[0] + dx, i[1] + dy, i[2] + dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
        if not all(good(cell) for cell in cells):
            return None
        return cells, [a - float(b) for a, b in zip(h, i)]

    def value(cell):
        return float(table[cell][1]) / float(table[cell][0])

    def voxel_of(g, cells):
        cell = tuple(math.floor(v) for v in g)
        assert cell in cells
        return cell

    for c in range(C):
        P = [[float(x) for x in row] for row in poses[c]]
        for y in range(H):
            for x in range(W):
                ray = [(m[3 * k] * float(x) + m[3 * k + 1] * float(y)) + m[3 * k + 2] for k in range(3)]
                stats[c, 0] += 1
                prev, outcome = None, "miss"
                for s in range(n_steps):
                    z = near + float(s) * step
                    g = grid(P, ray, z)
                    got = corners(g)
                    if got is None:
                        prev = None
                        continue
                    val = _trilinear([value(cell) for cell in got[0]], got[1])
                    if prev is not None and prev >= 0.0 and val < 0.0:
                        outcome = "hit"
                        break
                    if prev is not None and prev < 0.0 and val >= 0.0:
                        outcome = "back"
                        break
                    prev = val
                if outcome != "hit":
                    stats[c, 2 if outcome == "back" else 3] += 1
                    continue
                stats[c, 1] += 1
                t = prev / (prev - val)
                z_hit = (near + float(s - 1) * step) + t * step
                g_hit = grid(P, ray, z_hit)
                at = corners(g_hit)
                unit = None
                if at is not None:
                    G = _trilinear_gradient([value(cell) for cell in at[0]], at[1])
                    norm = math.sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2])
                    if norm > 0.0:
                        unit = [a / norm for a in G]
                if unit is None:
                    stats[c, 4] += 1
                else:
                    normal[c, :, y, x] = [np.float32((P[0][k] * unit[0] + P[1][k] * unit[1]) + P[2][k] * unit[2]) for k in range(3)]
                row = table[voxel_of(g_hit, at[0]) if at is not None else voxel_of(g, got[0])]
                depth[c, y, x] = np.float32(z_hit)
                color[c, :, y, x] = [(2 * row[2 + k] + row[0]) // (2 * row[0]) for k in range(3)]
                weight[c, y, x] = min(row[0], 0x7fffffff)
    return Cast(depth, normal, color, weight, stats)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def inv_K_device(inv_K, device):
    """The nine float64 entries of inv_K's 3x3 block as a device tensor (td_tsdf_samples reads them from device memory)."""
    if torch.is_tensor(inv_K) and inv_K.is_cuda and inv_K.dtype == torch.float64 and tuple(inv_K.shape) == (9,):
        return inv_K.contiguous()
    return torch.from_numpy(cloud._inv_K9(inv_K.cpu().numpy() if torch.is_tensor(inv_K) else inv_K).copy()).to(device)


def samples_hip(depth, color, poses, inv_K, T, voxel, mask=None, depth_scale=1.0, pose_scale=1.0, stride=1, border=0,
                min_depth=cloud.DEFAULT_MIN_DEPTH, max_range=cloud.DEFAULT_MAX_RANGE, edge=0.0, stats=None):
    """samples_numpy as one launch of td_tsdf_samples -> (key int64 [(4T+1) B H W], payload int64 [(4T+1) B H W]: the uint64's bits).
    ``inv_K``: a float64 [9] device tensor (inv_K_device), or anything cloud accepts, which is uploaded;  ``mask``: a uint8 or bool
    [B,H,W] device tensor or None;  ``stats``: an int64 [10] device tensor that the launch increments (SAMPLE_STATS), or None."""
    depth, color, poses = cloud._check_frames(depth, color, poses, device=True)
    _check(T, voxel)
    if int(stride) < 1 or int(border) < 0 or not edge >= 0:
        raise ValueError("stride >= 1, border >= 0, edge >= 0")
    if mask is not None:
        native.require_device(mask)
        if mask.dtype not in (torch.uint8, torch.bool) or mask.shape != depth.shape:
            raise ValueError("mask: uint8 or bool %s, got %s %s" % (tuple(depth.shape), tuple(mask.shape), mask.dtype))
        mask = mask.contiguous().view(torch.uint8)
    if stats is not None:
        stats = cloud._i64(stats, "stats", len(SAMPLE_STATS))
    ik = inv_K_device(inv_K, depth.device)
    B, H, W = depth.shape
    n = (4 * int(T) + 1) * B * H * W
    key = torch.empty(n, dtype=torch.int64, device=depth.device)
    payload = torch.empty(n, dtype=torch.int64, device=depth.device)
    if n == 0:                           # an empty tensor has no pointer to pass
        return key, payload
    native.call("td_tsdf_samples", depth, color, poses, ik, mask, B, H, W, int(T),
                float(depth_scale), float(pose_scale), float(voxel), 1.0 / float(voxel), int(stride), int(border), float(min_depth),
                float(max_range), float(edge), key, payload, stats)
    return key, payload


def surface_hip(keys, sums, voxel, min_weight=DEFAULT_MIN_WEIGHT, stats=None):
    """surface_numpy as one launch of td_tsdf_surface -> (xyz float32 [V,3,3], normal float32 [V,3,3], rgb uint8 [V,3,3], weight int32
    [V,3], mask bool [V,3]); only where mask is set do the other four hold anything.  ``stats``: an int64 [5] device tensor that the
    launch increments (SURFACE_STATS), or None."""
    keys = cloud._check_rows(keys, sums)
    V = keys.shape[0]
    _check(1, voxel, min_weight)
    if stats is not None:
        stats = cloud._i64(stats, "stats", len(SURFACE_STATS))
    dev = keys.device
    xyz, normal = torch.empty(V, 3, 3, dtype=torch.float32, device=dev), torch.empty(V, 3, 3, dtype=torch.float32, device=dev)
    rgb, weight = torch.empty(V, 3, 3, dtype=torch.uint8, device=dev), torch.empty(V, 3, dtype=torch.int32, device=dev)
    mask = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    if V:
        native.call("td_tsdf_surface", keys, sums.contiguous(), V, float(voxel), int(min_weight), xyz, normal, rgb, weight, mask, stats)
    return xyz, normal, rgb, weight, mask.bool()


def raycast_hip(keys, sums, poses, inv_K, height, width, voxel, min_weight=DEFAULT_MIN_WEIGHT, near=render.DEFAULT_NEAR,
                far=render.DEFAULT_FAR, step_voxels=DEFAULT_STEP_VOXELS, pose_scale=1.0, background=(0, 0, 0), out=None):
    """raycast_numpy as one fill and one launch of td_tsdf_cast -> Cast of device tensors.  keys int64 [V], sums int64 [V,7], poses
    float64 [C,3,4], all on one HIP device; ``inv_K``: a float64 [9] device tensor (inv_K_device) or anything cloud accepts, which is
    uploaded.  ``out``: a Cast of tensors to write into (None: allocated here).  The
    call does not synchronise."""
    keys = cloud._check_rows(keys, sums)
    native.require_device(poses)
    H, W = int(height), int(width)
    _, _, bg = _check_cast(H, W, voxel, min_weight, near, far, step_voxels, background)
    if poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] < 1:
        raise ValueError("poses float64 [C,3,4] with C >= 1, got %s %s" % (tuple(poses.shape), poses.dtype))
    ik = inv_K_device(inv_K, poses.device)
    C, V, dev = poses.shape[0], keys.shape[0], poses.device
    shapes = (((C, H, W), torch.float32), ((C, 3, H, W), torch.float32), ((C, 3, H, W), torch.uint8), ((C, H, W), torch.int32),
              ((C, len(CAST_STATS)), torch.int64))
    if out is None:
        out = Cast(*(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in shapes))
    native.require_device(*out)
    if [(tuple(t.shape), t.dtype) for t in out] != list(shapes) or not all(t.is_contiguous() for t in out):
        raise ValueError("out: contiguous tensors %s" % (shapes,))
    depth, normal, color, weight, stats = out
    if V == 0:                                                              # an empty tensor has no address to pass
        keys, sums = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, 7, dtype=torch.int64, device=dev)
    native.call("td_tsdf_cast", keys, sums.contiguous(), V, poses.contiguous(),
                ik, C, H, W, float(voxel), 1.0 / float(voxel), int(min_weight), float(near), float(far),
                float(step_voxels), float(pose_scale), bg[0], bg[1], bg[2], depth, normal, color, weight, stats)
    return Cast(*out)


class _TsdfMap(cloud.FrameMap):
    """The voxel map of signed distances: samples_hip makes the pairs, the filter's votes become the batch's mask."""

    def __init__(self, device, inv_K, voxel, T, stride, border, min_depth, max_range, edge, depth_scale, pose_scale,
                 pair_chunk=DEFAULT_PAIR_CHUNK, min_views=0, view_radius=cloud.DEFAULT_VIEW_RADIUS, view_tol=cloud.DEFAULT_VIEW_TOL, K=None):
        _check(T, voxel, pair_chunk=pair_chunk)
        super().__init__(device, len(SAMPLE_STATS), inv_K, depth_scale, pose_scale, min_depth, max_range, min_views, view_radius, view_tol, K)
        self.ik = inv_K_device(inv_K, device)
        self.args = dict(T=int(T), voxel=float(voxel), depth_scale=float(depth_scale), pose_scale=float(pose_scale), stride=stride,
                         border=border, min_depth=min_depth, max_range=max_range, edge=edge)
        self.pair_chunk = int(pair_chunk)

    def add(self, depth, color, poses, window=None, mask=None):
        """One batch of centre frames: its pairs, ``pair_chunk`` at a time, into the map.  With the filter on the votes, compared with
        min_views, become the batch's mask (and ``mask``, if given, is and-ed in)."""
        if self.min_views:
            keep = self.votes(window) >= self.min_views
            mask = keep if mask is None else keep & (mask != 0)
        self.merge(*samples_hip(depth, color, poses, self.ik, mask=mask, stats=self.counts, **self.args), pair_chunk=self.pair_chunk)

    def surface(self, voxel, min_weight):
        counts = torch.zeros(len(SURFACE_STATS), dtype=torch.int64, device=self.keys.device)
        xyz, normal, rgb, weight, hit = surface_hip(self.keys, self.sums, voxel, min_weight, stats=counts)
        out = (xyz[hit], normal[hit], rgb[hit], weight[hit])
        return Surface(*out, _stats(self.counts.cpu().numpy(), self.keys.shape[0], counts.cpu().numpy(), out[0].shape[0]))


def fuse_tsdf_hip(depth, color, poses, inv_K, voxel=cloud.DEFAULT_VOXEL, trunc_voxels=DEFAULT_TRUNC_VOXELS,
                  min_weight=DEFAULT_MIN_WEIGHT, batch_size=None, stride=1, border=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                  max_range=cloud.DEFAULT_MAX_RANGE, edge=0.0, depth_scale=1.0, pose_scale=1.0, mask=None, min_views=0,
                  view_radius=cloud.DEFAULT_VIEW_RADIUS, view_tol=cloud.DEFAULT_VIEW_TOL, K=None, pair_chunk=DEFAULT_PAIR_CHUNK, debug=None):
    """fuse_tsdf_numpy on the device, ``batch_size`` frames at a time (default: all at once) and ``pair_chunk`` pairs of a batch at a
    time -> Surface of device tensors.  With ``min_views`` > 0 the votes of cloud.views_hip (all frames as the window; td_cloud_views
    is untouched) become the batch's mask."""
    cloud._check_params(voxel, stride, border, min_depth, max_range, edge)
    cloud._check_view_params(min_views, view_radius, view_tol)
    _check(trunc_voxels, voxel, min_weight)
    native.require_device(depth, color, poses)
    vmap = _TsdfMap(depth.device, inv_K, voxel, trunc_voxels, stride, border, min_depth, max_range, edge, depth_scale, pose_scale, pair_chunk,
                    min_views, view_radius, view_tol, K)
    for at, end in cloud.frame_batches(0, len(depth), batch_size):          # all frames are the filter's window
        vmap.add(depth[at:end], color[at:end], poses[at:end], (depth, poses, (at, end), (0, len(depth))) if vmap.min_views else None,
                 mask=None if mask is None else mask[at:end])
    if debug is not None:
        debug["keys"], debug["sums"] = vmap.keys, vmap.sums
    return vmap.surface(voxel, min_weight)


# ---------------------------------------------------------------------------------------------------------------------------
# the map on disk

def save_map(path, keys, sums, voxel, trunc_voxels):
    """The fused map as one .npz: keys int64 [V], sums int64 [V,7], voxel float64 [], trunc_voxels int64 [].  Written deterministically
    (stored, not compressed, with a fixed time stamp): the same map gives the same bytes."""
    host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    keys, sums = _check_map(host(keys), host(sums))
    _check(trunc_voxels, voxel)
    arrays = (("keys", keys), ("sums", sums), ("voxel", np.array(voxel, np.float64)), ("trunc_voxels", np.array(trunc_voxels, np.int64)))
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, version=(1, 0), allow_pickle=False)      # keys and sums are contiguous, the scalars 0-d
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def load_map(path):
    """save_map's file -> (keys int64 [V], sums int64 [V,7], voxel float, trunc_voxels int).  Nothing is unpickled."""
    with np.load(path, allow_pickle=False) as z:
        missing = [name for name in ("keys", "sums", "voxel", "trunc_voxels") if name not in z.files]
        if missing:
            raise ValueError("%s: not a TSDF map, no %s" % (path, ", ".join(missing)))
        keys, sums, voxel, T = z["keys"], z["sums"], float(z["voxel"][()]), int(z["trunc_voxels"][()])
    if keys.dtype != np.int64 or sums.dtype != np.int64:
        raise ValueError("%s: keys and sums are int64, got %s, %s" % (path, keys.dtype, sums.dtype))
    keys, sums = _check_map(keys, sums)
    _check(T, voxel)
    return keys, sums, voxel, T


# ---------------------------------------------------------------------------------------------------------------------------

class TsdfCaster:
    """cast(keys, sums, poses) -> Cast of host arrays for any number of poses: the fused map seen from camera-to-world ``poses``.

    device      'cuda[:i]': the map is uploaded once (device tensors are used as they are), ``batch_size`` cameras go through one td_tsdf_cast launch at a time, and each batch's maps are copied back
                before the next (the only synchronisation).  'cpu': raycast_numpy, the statement.
    K           the 3x3 block in pixels at ``height`` x ``width`` (the rays use its float64 inverse)
    voxel, min_weight   the fuser's;  near, far: in the map's units, along the camera's z
    step_voxels the step between samples in voxels; the default is an UNTUNED starting value, like min_weight, near and far
    pose_scale  multiplies the poses' translations, as in TsdfFuser
    The result does not depend on batch_size.
    """

    def __init__(self, device, height, width, K, voxel, min_weight=DEFAULT_MIN_WEIGHT, near=render.DEFAULT_NEAR, far=render.DEFAULT_FAR,
                 step_voxels=DEFAULT_STEP_VOXELS, pose_scale=1.0, batch_size=12):
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        if self.on_hip and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.height, self.width = int(height), int(width)
        _check_cast(self.height, self.width, voxel, min_weight, near, far, step_voxels)
        if int(batch_size) < 1:
            raise ValueError("batch_size: at least 1, got %r" % (batch_size,))
        self.inv_K = np.linalg.inv(render._K9(K).reshape(3, 3))
        self.params = dict(voxel=float(voxel), min_weight=int(min_weight), near=float(near), far=float(far), step_voxels=float(step_voxels),
                           pose_scale=float(pose_scale))
        self.batch_size = int(batch_size)

    def cast(self, keys, sums, poses, background=(0, 0, 0)):
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        poses = _cast_poses(host(poses))
        if not self.on_hip:
            return raycast_numpy(host(keys), host(sums), poses, self.inv_K, self.height, self.width, background=background, **self.params)
        on_device = all(torch.is_tensor(t) and t.device == self.device for t in (keys, sums))
        keys_d, sums_d = (keys, sums) if on_device else (torch.from_numpy(a).to(self.device) for a in _check_map(host(keys), host(sums)))
        poses_d, ik = torch.from_numpy(poses).to(self.device), inv_K_device(self.inv_K, self.device)
        parts = []
        for at in range(0, len(poses), self.batch_size):
            out = raycast_hip(keys_d, sums_d, poses_d[at:at + self.batch_size], ik, self.height, self.width, background=background,
                              **self.params)
            parts.append([t.cpu().numpy() for t in out])
        return Cast(*(np.concatenate([p[j] for p in parts], 0) for j in range(5)))


class TsdfFuser(cloud.SequenceDriver):
    """fuse(dataset, poses=None, frames=None) -> Surface.

    The depth maps and the poses come from cloud.SequenceDriver, as SceneFuser's do (its DepthPredictor, its pose chain, its frame
    upload): ``model``, ``height``, ``width``, ``device``, ``batch_size``, ``precision``, ``post_process``, ``voxel``, ``stride``, ``border``,
    ``min_depth``, ``max_range``, ``edge``, ``depth_scale``, ``pose_scale`` mean what they mean there.
    trunc_voxels   the band T on either side of a pixel's surface, in voxels (1 ... 8); UNTUNED starting value
    min_weight     a voxel takes part in the surface when at least this many samples fell into it; UNTUNED starting value
    min_views, view_radius, view_tol   SceneFuser's multi-view filter, composed through the per-pixel mask: a pixel with fewer than
                   min_views votes (cloud.views_numpy / views_hip) emits no sample.  On the device the frames go through
                   the driver's sliding window (cloud.window_schedule): at most batch_size + 2 view_radius depth maps are held.
    pair_chunk     a batch makes B H W (4 trunc_voxels + 1) pairs (19 M at 12 x 192 x 640, T = 3); they are sorted and summed this
                   many at a time.  The result does not depend on it, nor on batch_size.
    device 'cuda[:i]': per batch DepthPredictor, samples_hip, then cloud's unchanged sort / heads / cumsum / reduce / merge; one
    surface_hip at the end.  'cpu': the host statements.
    ``map``: (keys int64 [V], sums int64 [V,7]) of the last fuse, on the fuser's device (numpy arrays on the host path): what
    TsdfCaster.cast and save_map take.
    """

    def __init__(self, model, height, width, device, voxel=cloud.DEFAULT_VOXEL, trunc_voxels=DEFAULT_TRUNC_VOXELS,
                 min_weight=DEFAULT_MIN_WEIGHT, batch_size=12, precision="fp32", stride=1, border=0, min_depth=cloud.DEFAULT_MIN_DEPTH,
                 max_range=cloud.DEFAULT_MAX_RANGE, edge=cloud.DEFAULT_EDGE, depth_scale=1.0, pose_scale=1.0, post_process=False,
                 min_views=0, view_radius=cloud.DEFAULT_VIEW_RADIUS, view_tol=cloud.DEFAULT_VIEW_TOL, pair_chunk=DEFAULT_PAIR_CHUNK):
        _check(trunc_voxels, voxel, min_weight, pair_chunk)
        cloud._check_params(voxel, stride, border, min_depth, max_range, edge)
        cloud._check_view_params(min_views, view_radius, view_tol)
        super().__init__(model, height, width, device, batch_size, precision, post_process)
        self.voxel, self.T, self.min_weight, self.pair_chunk = float(voxel), int(trunc_voxels), int(min_weight), int(pair_chunk)
        self.params = dict(stride=int(stride), border=int(border), min_depth=float(min_depth), max_range=float(max_range),
                           edge=float(edge), depth_scale=float(depth_scale), pose_scale=float(pose_scale))
        self.views = dict(min_views=int(min_views), view_radius=int(view_radius), view_tol=float(view_tol))
        self.map = None

    def fuse(self, dataset, poses=None, frames=None, debug=None):
        """``poses``, ``frames``: as SceneFuser.fuse.  ``debug``: a dict that receives the "depth" maps [m,H,W] and the "poses"
        [n+1,3,4] that were fused."""
        inv_K, K = cloud.dataset_inv_K(dataset), cloud.dataset_K(dataset)
        sink = _TsdfMap(self.device, inv_K, self.voxel, self.T, pair_chunk=self.pair_chunk, K=K, **self.params, **self.views) if self.on_hip \
            else cloud.HostFrames(self.views["min_views"], self.views["view_radius"])
        self.run(dataset, sink, poses, frames, debug)
        if self.on_hip:
            self.map = (sink.keys, sink.sums)
            return sink.surface(self.voxel, self.min_weight)
        kept = {}
        out = fuse_tsdf_numpy(*sink.arrays(), inv_K, self.voxel, self.T, self.min_weight, K=K, debug=kept, **self.params, **self.views)
        self.map = (kept["keys"], kept["sums"])
        return out
