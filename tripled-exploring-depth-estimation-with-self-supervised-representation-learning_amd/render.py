"""A fused point cloud drawn back into camera views: per-camera depth, colour and point-index maps from a z-buffered point renderer.

cloud.py ends at a cloud; the rest of this build works with depth maps in a camera.  This module turns the one into the other: what a
camera at a given pose sees of the cloud, to look at a reconstruction, to compare it with the depth network's own output or with
velodyne.depth_maps_hip, and for any later occlusion-aware use of the cloud.  The reference has no such program (its only 3-D picture
is draw_odometry.py's bird's-eye trajectory; ``top_view`` is the cloud's counterpart of it).

Three layers, as in cloud.py:
  * host statements in numpy (``render_numpy`` and the literal per-pixel loop ``render_bruteforce``): the host path (``device='cpu'``)
    and what the kernel is tested against.  The projection is written element-wise in the kernel's operation order, with no ``@``;
  * ``render_hip`` / ``render_workspace``: td_cloud_render (csrc/td_render.hip).  Device tensors only; a CPU tensor is an error;
  * ``CloudRenderer``: a cloud and any number of poses -> host arrays, ``batch_size`` cameras per launch chain, one workspace.

What is computed per point i and camera c (float64; every product, sum and quotient rounded on its own; [R|t] = the camera-to-world
pose, k = K's 3x3 block in pixels, pixel centres at integer coordinates like the reference's Backproject):
    e_k = float64(xyz_k) - pose_scale t_k;   q_k = (R_0k e_0 + R_1k e_1) + R_2k e_2   (the transpose of R, as in cloud.views_numpy)
    z   = q_2
    perspective:   u = ((k00 q_0 + k01 q_1) + k02 q_2) / z;   v = ((k10 q_0 + k11 q_1) + k12 q_2) / z;   s = (splat k00) / z
    orthographic:  u = (k00 q_0 + k01 q_1) + k02;             v = (k10 q_0 + k11 q_1) + k12;             s = splat k00
    in_range = near <= z <= far  (a NaN fails);   ui = rint(u), vi = rint(v)  (half to even);   r = min(MAX_SPLAT, floor(0.5 s))
    visible  = in_range and ui + r >= 0 and ui - r <= W-1 and vi + r >= 0 and vi - r <= H-1      (in float64; a NaN fails)
    packed   = uint64(bits of float32(z)) << 32 | i
    every pixel of the square [ui-r, ui+r] x [vi-r, vi+r] inside the image keeps the minimum packed value it is offered
near > 0 makes float32(z) non-negative, so its bits order like its value: a pixel shows the nearest point that covers it, and among
equal float32(z) the one with the lowest index.  A pixel nothing covers has depth 0, the background colour and index -1.

Limits, stated plainly: a point is drawn as a SQUARE IN THE IMAGE of the size a ``splat``-wide object would have at its depth (at
most 17 x 17 pixels), not as a disc in space; where the squares of a surface leave gaps, the points behind it are drawn through them
(there is no hole filling); the defaults of ``splat``, ``near`` and ``far`` are UNTUNED starting values; no real cloud has been
rendered yet.

Surfels (``render_surfels_numpy``, the literal loop ``render_surfels_bruteforce``, ``render_surfels_hip``: td_cloud_render_surfels in
csrc/td_surfel.hip, ``CloudRenderer.render_surfels``) are the remedy for the first two limits: every point is an oriented DISC IN SPACE
of one ``radius``, with the normal n that cloud_normals estimates and orients.  Per point and camera, with e, q_0, q_1, z as above
(K must have k10 = 0 and positive k00, k11: the rays invert its upper triangle):
    m_k = (R_0k n_0 + R_1k n_1) + R_2k n_2;   a point without a normal (all three zero) gets m = (0, 0, -1): a billboard
    out of range unless near <= z <= far;   culled (``cull``) when ((m_0 q_0) + (m_1 q_1)) + (m_2 z) > 0, orthographic m_2 > 0
    perspective:   u = ((k00 q_0 + k01 q_1) + k02 z) / z;   v = (k11 q_1 + k12 z) / z;   tm = max(near, z - radius);   g = radius / tm
                   a_x = g (1 + |q_0| / z);   a_y = g (1 + |q_1| / z);   b_x = k00 a_x + |k01| a_y;   b_y = k11 a_y
    orthographic:  u = (k00 q_0 + k01 q_1) + k02;   v = k11 q_1 + k12;   b_x = (k00 + |k01|) radius;   b_y = k11 radius
    ui = rint(u), vi = rint(v);   r = floor(max(b_x, b_y) + SURFEL_SLACK);   capped when r > MAX_SURFEL, then r = MAX_SURFEL
    outside unless ui + r >= 0, ui - r <= W-1, vi + r >= 0, vi - r <= H-1;   else drawn
The box is conservative: a hit h on the disc has |h - q| <= radius and depth t >= tm, so |h_0 / t - q_0 / z| = |(h_0 - q_0) / t +
q_0 (z - t) / (t z)| <= (radius / tm) (1 + |q_0| / z) = a_x, likewise a_y, and the pixel of the hit is at most (b_x, b_y) from (u, v),
that is floor(b + 1/2) from (ui, vi); 2^-10 more absorbs the rounding of the bound and of the pixel test.  The bound grows off axis,
as the projection of a ball does.  Per pixel (x, y) of the box inside the image:
    d_1 = (y - k12) / k11;   d_0 = ((x - k02) - k01 d_1) / k00
    perspective:   den = ((m_0 d_0) + (m_1 d_1)) + m_2;   num = ((m_0 q_0) + (m_1 q_1)) + (m_2 z);   t = num / den;   hit = (t d_0, t d_1, t)
    orthographic:  den = m_2;   num = ((m_0 (q_0 - d_0)) + (m_1 (q_1 - d_1))) + (m_2 z);   t = num / den;   hit = (d_0, d_1, t)
    covered when den < 0 or den > 0 (edge-on draws nothing, a NaN fails), |hit - q|^2 <= radius radius, and near <= t <= far
    packed = uint64(bits of float32(t)) << 32 | i,   the pixel keeps the minimum
The resolve pass recomputes m and the ray from the winner's index: the depth float32(t), the index, the normal map float32(m), negated
when den > 0 (turned towards the viewer), and the colour: the point's own, untouched, when ambient = 1, else per channel
min(255, floor(c (ambient + (1 - ambient) shade) + 0.5)) with shade = |den| / sqrt(((d_0 d_0) + (d_1 d_1)) + 1) (orthographic: / sqrt(1)).
Limits: one radius for all discs; overlapping discs are not blended, the nearest wins; a box is capped at 33 x 33 pixels (counted as
capped, and drawn inside the capped box); a NaN normal draws nothing; the defaults of radius, ambient and MAX_SURFEL are UNTUNED; no
real cloud has been rendered.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import cloud, native

MAX_SPLAT = native.CONSTANTS["TD_RENDER_MAX_SPLAT"]
STATS = ("points", "out_of_range", "outside", "drawn", "pixels_hit")
_NONE = np.uint64(0xffffffffffffffff)

# In the MODEL's units, like cloud.py's.  UNTUNED: nobody has looked at a rendering of a trained checkpoint's cloud with them.
DEFAULT_NEAR = cloud.DEFAULT_MIN_DEPTH       # what the fuser does not back-project is not drawn either
DEFAULT_FAR = 4.0 * cloud.DEFAULT_MAX_RANGE  # a view sees farther than one frame contributed
DEFAULT_SPLAT = cloud.DEFAULT_VOXEL          # a point stands for its voxel

MAX_SURFEL = native.CONSTANTS["TD_SURFEL_MAX"]        # 16: the largest pixel box of a disc is 33 x 33.  UNTUNED
SURFEL_SLACK = native.CONSTANTS["TD_SURFEL_SLACK"]    # 0.5 + 2.0 ** -10
SURFEL_STATS = ("points", "out_of_range", "outside", "culled", "capped", "billboards", "drawn", "pixels_hit")
SURFEL_FORMS = {"auto": 0, "thread": 1, "cooperative": 2}      # td_cloud_render_surfels' work distribution; the bits do not depend on it

Rendered = collections.namedtuple("Rendered", "depth color index stats")
Rendered.__doc__ = """depth float32 [C,H,W] (float32(z) of the pixel's point, 0 where nothing was drawn), color uint8 [C,3,H,W] (the
background where nothing was drawn), index int32 [C,H,W] (the point's row in the cloud, -1 where nothing was drawn), stats int64 [C,5]
in the order of STATS: points, out of range, outside (in range but the square misses the image), drawn, pixels hit."""

SurfelRendered = collections.namedtuple("SurfelRendered", "depth color index normal stats")
SurfelRendered.__doc__ = """depth float32 [C,H,W] (float32(t) of the ray's hit on the pixel's disc, 0 where nothing was drawn), color uint8
[C,3,H,W] (shaded; the background where nothing was drawn), index int32 [C,H,W] (-1 where nothing was drawn), normal float32 [C,3,H,W]
(the disc's normal in the camera, turned towards the viewer; +0.0 where nothing was drawn), stats int64 [C,8] in the order of
SURFEL_STATS: points = out_of_range + culled + outside + drawn; capped and billboards count drawn surfels."""

# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _check_params(height, width, near, far, splat, background):
    if int(height) < 1 or int(width) < 1 or int(height) * int(width) > 0x7fffffff:
        raise ValueError("a view of at least 1 x 1 and at most 2^31 - 1 pixels, got %r x %r" % (height, width))
    if not near > 0 or not np.isfinite(far) or not far >= near:
        raise ValueError("0 < near <= far < inf, got %r, %r" % (near, far))
    if not splat >= 0 or not np.isfinite(splat):
        raise ValueError("splat: a finite size >= 0, got %r" % (splat,))
    bg = tuple(int(v) for v in background)
    if len(bg) != 3 or min(bg) < 0 or max(bg) > 255:
        raise ValueError("background: three values in 0 ... 255, got %r" % (background,))
    return bg


def _check_cloud(xyz, rgb, poses):
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim == 3 and poses.shape[1:] == (4, 4):
        poses = poses[:, :3]
    poses = np.ascontiguousarray(poses)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or rgb.shape != xyz.shape or poses.ndim != 3 or poses.shape[1:] != (3, 4) or not len(poses):
        raise ValueError("xyz [V,3], rgb [V,3], poses [C,3,4] with C >= 1; got %s, %s, %s" % (xyz.shape, rgb.shape, poses.shape))
    if len(xyz) >= 0x7fffffff:
        raise ValueError("at most 2^31 - 2 points, got %d" % len(xyz))
    return xyz, rgb, poses


def _K9(K):
    k = cloud._inv_K9(K, "K")
    if not np.isfinite(k).all():
        raise ValueError("K: finite entries, got %r" % (k,))
    return k


def project_numpy(xyz, pose, k, near, far, splat, pose_scale, ortho, height, width):
    """One camera: float32 [V,3] -> (ui, vi, r float64 [V], zf float32 [V], in_range, visible bool [V]), element-wise in the
    kernel's operation order."""
    ps, sk = np.float64(pose_scale), np.float64(splat) * k[0]
    with np.errstate(all="ignore"):
        e = [xyz[:, j].astype(np.float64) - ps * pose[j, 3] for j in range(3)]
        q = [(pose[0, j] * e[0] + pose[1, j] * e[1]) + pose[2, j] * e[2] for j in range(3)]
        z = q[2]
        in_range = (z >= np.float64(near)) & (z <= np.float64(far))
        if ortho:
            u = (k[0] * q[0] + k[1] * q[1]) + k[2]
            v = (k[3] * q[0] + k[4] * q[1]) + k[5]
            s = np.broadcast_to(sk, z.shape)
        else:
            u = ((k[0] * q[0] + k[1] * q[1]) + k[2] * z) / z
            v = ((k[3] * q[0] + k[4] * q[1]) + k[5] * z) / z
            s = sk / z
        ui, vi = np.rint(u), np.rint(v)
        r = np.floor(0.5 * s)
        r = np.where(r > float(MAX_SPLAT), float(MAX_SPLAT), r)             # a NaN stays one and fails below
        visible = in_range & (ui + r >= 0.0) & (ui - r <= float(width - 1)) & (vi + r >= 0.0) & (vi - r <= float(height - 1))
        zf = z.astype(np.float32)
    return ui, vi, r, zf, in_range, visible


def _resolve(buffer, rgb, background, shape):
    hit = buffer != _NONE
    index = np.where(hit, buffer & np.uint64(0xffffffff), np.uint64(0)).astype(np.int64)
    depth = np.where(hit, (buffer >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(0))
    color = np.empty((3,) + buffer.shape, np.uint8)
    for ch in range(3):
        color[ch] = np.where(hit, rgb[index, ch] if len(rgb) else 0, np.uint8(background[ch]))
    return (depth.astype(np.float32).reshape(shape), color.reshape((3,) + shape), np.where(hit, index, -1).astype(np.int32).reshape(shape),
            int(np.count_nonzero(hit)))


def render_numpy(xyz, rgb, poses, K, height, width, near=DEFAULT_NEAR, far=DEFAULT_FAR, splat=0.0, pose_scale=1.0, ortho=False,
                 background=(0, 0, 0)):
    """xyz float32 [V,3], rgb uint8 [V,3], poses float64 [C,3,4] camera-to-world, K: the 3x3 block in pixels -> Rendered of numpy
    arrays.  The statement td_cloud_render is tested against, operation for operation; the packed values are reduced with
    np.minimum.at, one pass per offset inside the largest square.  ``splat``: the world size of a point, 0: one pixel per point."""
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, splat, background)
    xyz, rgb, poses = _check_cloud(xyz, rgb, poses)
    k = _K9(K)
    C, V = len(poses), len(xyz)
    depth, color = np.empty((C, H, W), np.float32), np.empty((C, 3, H, W), np.uint8)
    index, stats = np.empty((C, H, W), np.int32), np.zeros((C, 5), np.int64)
    ids = np.arange(V, dtype=np.uint64)
    for c in range(C):
        ui, vi, r, zf, in_range, visible = project_numpy(xyz, poses[c], k, near, far, splat, pose_scale, ortho, H, W)
        buffer = np.full(H * W, _NONE, np.uint64)
        sel = np.nonzero(visible)[0]
        x, y, rr = ui[sel].astype(np.int64), vi[sel].astype(np.int64), r[sel].astype(np.int64)
        packed = (zf[sel].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[sel]
        reach = int(rr.max()) if len(sel) else -1
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                xx, yy = x + dx, y + dy
                m = (rr >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                np.minimum.at(buffer, (yy * W + xx)[m], packed[m])
        depth[c], color[c], index[c], hit = _resolve(buffer, rgb, bg, (H, W))
        n_in = int(np.count_nonzero(in_range))
        stats[c] = (V, V - n_in, n_in - len(sel), len(sel), hit)
    return Rendered(depth, color, index, stats)


def render_bruteforce(xyz, rgb, poses, K, height, width, near=DEFAULT_NEAR, far=DEFAULT_FAR, splat=0.0, pose_scale=1.0, ortho=False,
                      background=(0, 0, 0)):
    """render_numpy said a second time, independently: a plain loop over the points projects them with scalar float64 arithmetic, then
    a loop per camera and per pixel picks the minimum (float32(z), i) over the points whose square covers the pixel.  For the tests."""
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, splat, background)
    xyz, rgb, poses = _check_cloud(xyz, rgb, poses)
    k = [np.float64(v) for v in _K9(K)]
    C, V = len(poses), len(xyz)
    depth, color = np.zeros((C, H, W), np.float32), np.empty((C, 3, H, W), np.uint8)
    index, stats = np.full((C, H, W), -1, np.int32), np.zeros((C, 5), np.int64)
    color[:] = np.array(bg, np.uint8).reshape(1, 3, 1, 1)
    ps, near, far, splat = np.float64(pose_scale), np.float64(near), np.float64(far), np.float64(splat)
    with np.errstate(all="ignore"):
        for c in range(C):
            R, t = poses[c, :, :3], poses[c, :, 3]
            squares = []                                                    # (x, y, r, float32(z), i) of the visible points
            out_of_range = outside = 0
            for i in range(V):
                e = [np.float64(xyz[i, j]) - ps * t[j] for j in range(3)]
                q = [(R[0, j] * e[0] + R[1, j] * e[1]) + R[2, j] * e[2] for j in range(3)]
                z = q[2]
                if not near <= z <= far:
                    out_of_range += 1
                    continue
                if ortho:
                    u, v, s = (k[0] * q[0] + k[1] * q[1]) + k[2], (k[3] * q[0] + k[4] * q[1]) + k[5], splat * k[0]
                else:
                    u, v, s = ((k[0] * q[0] + k[1] * q[1]) + k[2] * z) / z, ((k[3] * q[0] + k[4] * q[1]) + k[5] * z) / z, (splat * k[0]) / z
                x, y, r = np.rint(u), np.rint(v), min(np.float64(MAX_SPLAT), np.floor(0.5 * s))
                if not (x + r >= 0 and x - r <= W - 1 and y + r >= 0 and y - r <= H - 1):
                    outside += 1
                    continue
                squares.append((int(x), int(y), int(r), np.float32(z), i))
            hit = 0
            for py in range(H):
                for px in range(W):
                    best = None
                    for x, y, r, zf, i in squares:
                        if abs(x - px) <= r and abs(y - py) <= r and (best is None or (zf, i) < best):
                            best = (zf, i)
                    if best is not None:
                        hit += 1
                        depth[c, py, px], index[c, py, px], color[c, :, py, px] = best[0], best[1], rgb[best[1]]
            stats[c] = (V, out_of_range, outside, len(squares), hit)
    return Rendered(depth, color, index, stats)


def top_view(xyz, height, width, margin=0.05, near=DEFAULT_NEAR):
    """An orthographic camera above the cloud's bounding box, looking along +y (KITTI's down) -> (pose float64 [3,4] camera-to-world,
    K float64 [3,3]) for ``ortho=True`` and ``pose_scale=1``.  The camera's axes in world coordinates: x = +x, y = -z, z = +y, so
    the sequence's forward direction is up in the picture.  One scale for both axes, the largest at which the box, centred, leaves
    ``margin`` of the width and of the height free on every side.  The camera stands 2 near above the highest point: every point has
    z >= near (the lowest has z = 2 near + the box's height, which ``far`` must reach).  Points that are not finite are ignored."""
    H, W = int(height), int(width)
    if H < 1 or W < 1 or not 0 <= margin < 0.5 or not near > 0:
        raise ValueError("a view of at least 1 x 1 pixels, 0 <= margin < 0.5, near > 0; got %r x %r, %r, %r" % (height, width, margin, near))
    p = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    if not len(p):
        raise ValueError("top_view: no finite point")
    lo, hi = p.min(0), p.max(0)
    free = 1.0 - 2.0 * float(margin)
    scales = [free * n / extent for n, extent in ((W - 1, hi[0] - lo[0]), (H - 1, hi[2] - lo[2])) if extent > 0 and n > 0]
    scale = min(scales) if scales else 1.0
    pose = np.array([[1.0, 0.0, 0.0, 0.5 * (lo[0] + hi[0])],
                     [0.0, 0.0, 1.0, lo[1] - 2.0 * float(near)],
                     [0.0, -1.0, 0.0, 0.5 * (lo[2] + hi[2])]])
    K = np.array([[scale, 0.0, 0.5 * (W - 1)], [0.0, scale, 0.5 * (H - 1)], [0.0, 0.0, 1.0]])
    return pose, K


# ---------------------------------------------------------------------------------------------------------------------------
# surfels: host statements

def _check_surfel_params(radius, ambient, k):
    if not radius > 0 or not np.isfinite(radius):
        raise ValueError("radius: a finite size > 0, got %r" % (radius,))
    if not (ambient >= 0 and ambient <= 1):
        raise ValueError("ambient: inside [0, 1], got %r" % (ambient,))
    if not (k[0] > 0 and k[4] > 0 and k[3] == 0):
        raise ValueError("surfels need K10 = 0 and positive K00, K11 (the rays invert K's upper triangle), got %r" % (k[:6],))


def _check_normals(normal, xyz):
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    if normal.shape != xyz.shape:
        raise ValueError("normals [V,3] like xyz, got %s for %s" % (normal.shape, xyz.shape))
    return normal


def surfel_setup_numpy(xyz, normal, pose, k, near, far, radius, pose_scale, ortho, cull, height, width):
    """One camera -> dict of per-point arrays in the kernel's operation order: q0, q1, z, m0, m1, m2 (float64), billboard, in_range,
    culled, visible, capped (bool; culled, visible and capped already exclude what an earlier test removed), ui, vi, r (float64)."""
    ps, rad = np.float64(pose_scale), np.float64(radius)
    with np.errstate(all="ignore"):
        e = [xyz[:, j].astype(np.float64) - ps * pose[j, 3] for j in range(3)]
        q0, q1, z = [(pose[0, j] * e[0] + pose[1, j] * e[1]) + pose[2, j] * e[2] for j in range(3)]
        n = [normal[:, j].astype(np.float64) for j in range(3)]
        billboard = (normal[:, 0] == 0) & (normal[:, 1] == 0) & (normal[:, 2] == 0)
        m = [(pose[0, j] * n[0] + pose[1, j] * n[1]) + pose[2, j] * n[2] for j in range(3)]
        m0, m1, m2 = np.where(billboard, 0.0, m[0]), np.where(billboard, 0.0, m[1]), np.where(billboard, -1.0, m[2])
        in_range = (z >= np.float64(near)) & (z <= np.float64(far))
        if ortho:
            back = m2 > 0.0
            u = (k[0] * q0 + k[1] * q1) + k[2]
            v = k[4] * q1 + k[5]
            bx = np.broadcast_to((k[0] + np.abs(k[1])) * rad, z.shape)
            by = np.broadcast_to(k[4] * rad, z.shape)
        else:
            back = ((m0 * q0) + (m1 * q1)) + (m2 * z) > 0.0
            u = ((k[0] * q0 + k[1] * q1) + k[2] * z) / z
            v = (k[4] * q1 + k[5] * z) / z
            tm = z - rad
            tm = np.where(tm < np.float64(near), np.float64(near), tm)
            g = rad / tm
            ax, ay = g * (1.0 + np.abs(q0) / z), g * (1.0 + np.abs(q1) / z)
            bx = k[0] * ax + np.abs(k[1]) * ay
            by = k[4] * ay
        culled = in_range & back if cull else np.zeros(len(z), bool)
        ui, vi = np.rint(u), np.rint(v)
        b = np.where(bx > by, bx, by)
        r = np.floor(b + SURFEL_SLACK)
        over = r > float(MAX_SURFEL)
        r = np.where(over, float(MAX_SURFEL), r)                              # a NaN stays one and fails below
        alive = in_range & ~culled
        visible = alive & (ui + r >= 0.0) & (ui - r <= float(width - 1)) & (vi + r >= 0.0) & (vi - r <= float(height - 1))
    return dict(q0=q0, q1=q1, z=z, m0=m0, m1=m1, m2=m2, billboard=billboard, in_range=in_range, culled=culled, visible=visible,
                capped=visible & over, ui=ui, vi=vi, r=r)


def surfel_pixel_numpy(k, ortho, near, far, radius, q0, q1, z, m0, m1, m2, x, y):
    """The ray of pixel (x, y) against the disc(s), element-wise in the kernel's operation order -> (covered, t, den, d0, d1)."""
    r2 = np.float64(radius) * np.float64(radius)
    with np.errstate(all="ignore"):
        d1 = (np.asarray(y, np.float64) - k[5]) / k[4]
        d0 = ((np.asarray(x, np.float64) - k[2]) - k[1] * d1) / k[0]
        if ortho:
            den = m2
            num = ((m0 * (q0 - d0)) + (m1 * (q1 - d1))) + (m2 * z)
        else:
            den = ((m0 * d0) + (m1 * d1)) + m2
            num = ((m0 * q0) + (m1 * q1)) + (m2 * z)
        t = num / den
        h0, h1 = (d0, d1) if ortho else (t * d0, t * d1)
        e0, e1, e2 = h0 - q0, h1 - q1, t - z
        dist2 = ((e0 * e0) + (e1 * e1)) + (e2 * e2)
        covered = ((den < 0.0) | (den > 0.0)) & (dist2 <= r2) & (t >= np.float64(near)) & (t <= np.float64(far))
    return covered, t, den, d0, d1


def _shade_numpy(c, f):
    """uint8 colours, float64 factor -> uint8: min(255, floor(c f + 0.5))."""
    with np.errstate(all="ignore"):
        val = np.floor(c.astype(np.float64) * f + 0.5)
    return np.where(val >= 255.0, 255.0, np.where(val > 0.0, val, 0.0)).astype(np.uint8)


def _resolve_surfels(buffer, s, rgb, k, ortho, near, far, radius, ambient, background, H, W):
    """The table of one camera -> (depth, color, index, normal map, pixels hit): the winner's disc is intersected again."""
    depth, color, index, hit_count = _resolve(buffer, rgb, background, (H, W))
    nmap = np.zeros((3, H, W), np.float32)
    ys, xs = np.nonzero(index >= 0)
    if len(ys):
        i = index[ys, xs].astype(np.int64)
        _, _, den, d0, d1 = surfel_pixel_numpy(k, ortho, near, far, radius, s["q0"][i], s["q1"][i], s["z"][i], s["m0"][i], s["m1"][i],
                                               s["m2"][i], xs, ys)
        away = den > 0.0
        for j, name in enumerate(("m0", "m1", "m2")):
            mf = s[name][i].astype(np.float32)
            nmap[j, ys, xs] = np.where(away, -mf, mf)
        if np.float64(ambient) != 1.0:
            with np.errstate(all="ignore"):
                dd = np.ones(len(i)) if ortho else ((d0 * d0) + (d1 * d1)) + 1.0
                shade = np.abs(den) / np.sqrt(dd)
                f = np.float64(ambient) + (1.0 - np.float64(ambient)) * shade
            for ch in range(3):
                color[ch, ys, xs] = _shade_numpy(rgb[i, ch], f)
    return depth, color, index, nmap, hit_count


def render_surfels_numpy(xyz, rgb, normals, poses, K, height, width, radius, near=DEFAULT_NEAR, far=DEFAULT_FAR, cull=False, ambient=1.0,
                         pose_scale=1.0, ortho=False, background=(0, 0, 0)):
    """xyz float32 [V,3], rgb uint8 [V,3], normals float32 [V,3] (all zero: none), poses float64 [C,3,4] -> SurfelRendered of numpy
    arrays.  The statement td_cloud_render_surfels is tested against, operation for operation (module docstring); the packed values
    are reduced with np.minimum.at, one pass per offset inside the largest box."""
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, 0.0, background)
    xyz, rgb, poses = _check_cloud(xyz, rgb, poses)
    normals = _check_normals(normals, xyz)
    k = _K9(K)
    _check_surfel_params(radius, ambient, k)
    C, V = len(poses), len(xyz)
    depth, color = np.empty((C, H, W), np.float32), np.empty((C, 3, H, W), np.uint8)
    index, nmap, stats = np.empty((C, H, W), np.int32), np.empty((C, 3, H, W), np.float32), np.zeros((C, 8), np.int64)
    ids = np.arange(V, dtype=np.uint64)
    for c in range(C):
        s = surfel_setup_numpy(xyz, normals, poses[c], k, near, far, radius, pose_scale, ortho, cull, H, W)
        buffer = np.full(H * W, _NONE, np.uint64)
        sel = np.nonzero(s["visible"])[0]
        x, y, rr = s["ui"][sel].astype(np.int64), s["vi"][sel].astype(np.int64), s["r"][sel].astype(np.int64)
        geo = [s[name][sel] for name in ("q0", "q1", "z", "m0", "m1", "m2")]
        reach = int(rr.max()) if len(sel) else -1
        for dy in range(-reach, reach + 1):
            for dx in range(-reach, reach + 1):
                xx, yy = x + dx, y + dy
                w = np.nonzero((rr >= max(abs(dx), abs(dy))) & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H))[0]
                if not len(w):
                    continue
                covered, t, _, _, _ = surfel_pixel_numpy(k, ortho, near, far, radius, *(g[w] for g in geo), xx[w], yy[w])
                w, t = w[covered], t[covered]
                packed = (t.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[sel[w]]
                np.minimum.at(buffer, (yy * W + xx)[w], packed)
        depth[c], color[c], index[c], nmap[c], hit = _resolve_surfels(buffer, s, rgb, k, ortho, near, far, radius, ambient, bg, H, W)
        n_in, n_cull = int(np.count_nonzero(s["in_range"])), int(np.count_nonzero(s["culled"]))
        stats[c] = (V, V - n_in, n_in - n_cull - len(sel), n_cull, int(np.count_nonzero(s["capped"])),
                    int(np.count_nonzero(s["billboard"][sel])), len(sel), hit)
    return SurfelRendered(depth, color, index, nmap, stats)


def render_surfels_bruteforce(xyz, rgb, normals, poses, K, height, width, radius, near=DEFAULT_NEAR, far=DEFAULT_FAR, cull=False,
                              ambient=1.0, pose_scale=1.0, ortho=False, background=(0, 0, 0), box=True):
    """render_surfels_numpy said a second time, independently: a literal loop over the cameras, the points and the pixels in Python
    floats (the same float64 operations, one at a time).  ``box=False`` tests EVERY pixel of the image for every surfel and ignores
    both the box and the cap (the stats are still counted as the box decides, the drawing does not depend on it): that the result is the same shows that the box removes no pixel the geometry covers.  For the tests."""
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, 0.0, background)
    xyz, rgb, poses = _check_cloud(xyz, rgb, poses)
    normals = _check_normals(normals, xyz)
    kk = _K9(K)
    _check_surfel_params(radius, ambient, kk)
    k00, k01, k02, _, k11, k12 = (float(v) for v in kk[:6])
    C, V = len(poses), len(xyz)
    depth, color = np.zeros((C, H, W), np.float32), np.empty((C, 3, H, W), np.uint8)
    index, nmap, stats = np.full((C, H, W), -1, np.int32), np.zeros((C, 3, H, W), np.float32), np.zeros((C, 8), np.int64)
    color[:] = np.array(bg, np.uint8).reshape(1, 3, 1, 1)
    ps, near, far, rad, amb = float(pose_scale), float(near), float(far), float(radius), float(ambient)
    r2 = rad * rad
    pts, nrm = xyz.astype(np.float64).tolist(), normals.astype(np.float64).tolist()

    def ray(px, py):
        d1 = (float(py) - k12) / k11
        return ((float(px) - k02) - k01 * d1) / k00, d1

    def test(q0, q1, z, m0, m1, m2, d0, d1):
        """-> (t, den) of a covered pixel, or None."""
        if ortho:
            den, num = m2, ((m0 * (q0 - d0)) + (m1 * (q1 - d1))) + (m2 * z)
        else:
            den, num = ((m0 * d0) + (m1 * d1)) + m2, ((m0 * q0) + (m1 * q1)) + (m2 * z)
        if not (den < 0.0 or den > 0.0):
            return None
        t = num / den
        h0, h1 = (d0, d1) if ortho else (t * d0, t * d1)
        e0, e1, e2 = h0 - q0, h1 - q1, t - z
        if ((e0 * e0) + (e1 * e1)) + (e2 * e2) <= r2 and near <= t <= far:
            return t, den
        return None

    for c in range(C):
        R, tr = poses[c, :, :3].tolist(), [ps * float(v) for v in poses[c, :, 3]]
        best = {}                                                             # (py, px) -> (float32(t), i)
        geo = {}
        counts = dict(out_of_range=0, outside=0, culled=0, capped=0, billboards=0, drawn=0)
        for i in range(V):
            e = [pts[i][j] - tr[j] for j in range(3)]
            q0, q1, z = [(R[0][j] * e[0] + R[1][j] * e[1]) + R[2][j] * e[2] for j in range(3)]
            n = nrm[i]
            bill = n[0] == 0.0 and n[1] == 0.0 and n[2] == 0.0
            m0, m1, m2 = (0.0, 0.0, -1.0) if bill else [(R[0][j] * n[0] + R[1][j] * n[1]) + R[2][j] * n[2] for j in range(3)]
            if not near <= z <= far:
                counts["out_of_range"] += 1
                continue
            if ortho:
                back = m2 > 0.0
                u, v = (k00 * q0 + k01 * q1) + k02, k11 * q1 + k12
                bx, by = (k00 + abs(k01)) * rad, k11 * rad
            else:
                back = ((m0 * q0) + (m1 * q1)) + (m2 * z) > 0.0
                u, v = ((k00 * q0 + k01 * q1) + k02 * z) / z, (k11 * q1 + k12 * z) / z
                tm = z - rad
                tm = near if tm < near else tm
                g = rad / tm
                ax, ay = g * (1.0 + abs(q0) / z), g * (1.0 + abs(q1) / z)
                bx, by = k00 * ax + abs(k01) * ay, k11 * ay
            if cull and back:
                counts["culled"] += 1
                continue
            b = bx if bx > by else by
            x = y = r = over = None
            if math.isfinite(u) and math.isfinite(v) and math.isfinite(b):        # else rint / floor fail every comparison: outside
                x, y, r = float(round(u)), float(round(v)), float(math.floor(b + SURFEL_SLACK))      # round: half to even
                over = r > MAX_SURFEL
                r = float(MAX_SURFEL) if over else r
                if not (x + r >= 0 and x - r <= W - 1 and y + r >= 0 and y - r <= H - 1):
                    x = None
            geo[i] = (q0, q1, z, m0, m1, m2)
            if x is None:
                counts["outside"] += 1
                if box:
                    continue
            else:
                counts["drawn"] += 1
                counts["capped"] += int(over)
                counts["billboards"] += int(bill)
            if box:
                x, y, r = int(x), int(y), int(r)
                pixels = [(py, px) for py in range(max(0, y - r), min(H - 1, y + r) + 1) for px in range(max(0, x - r), min(W - 1, x + r) + 1)]
            else:
                pixels = [(py, px) for py in range(H) for px in range(W)]
            for py, px in pixels:
                got = test(q0, q1, z, m0, m1, m2, *ray(px, py))
                if got is not None:
                    cand = (np.float32(got[0]), i)
                    if (py, px) not in best or cand < best[py, px]:
                        best[py, px] = cand
        for (py, px), (tf, i) in best.items():
            d0, d1 = ray(px, py)
            den = test(*geo[i], d0, d1)[1]
            depth[c, py, px], index[c, py, px] = tf, i
            m = np.array(geo[i][3:], np.float64).astype(np.float32)
            nmap[c, :, py, px] = -m if den > 0.0 else m
            if amb == 1.0:
                color[c, :, py, px] = rgb[i]
            else:
                dd = 1.0 if ortho else ((d0 * d0) + (d1 * d1)) + 1.0
                f = amb + (1.0 - amb) * (abs(den) / math.sqrt(dd))
                color[c, :, py, px] = [min(255, max(0, int(math.floor(float(ch) * f + 0.5)))) for ch in rgb[i]]
        stats[c] = (V, counts["out_of_range"], counts["outside"], counts["culled"], counts["capped"], counts["billboards"], counts["drawn"],
                    len(best))
    return SurfelRendered(depth, color, index, nmap, stats)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel

def render_workspace(C, height, width, device):
    """The scratch buffer of render_hip for up to C views of this size (uint8, td_cloud_render_workspace_bytes)."""
    n = native.load().td_cloud_render_workspace_bytes(int(C), int(height), int(width))
    if n <= 0:
        raise native.NativeLibraryError("td_cloud_render_workspace_bytes(%d, %d, %d): unsupported shape" % (C, height, width))
    return torch.empty(n, dtype=torch.uint8, device=device)


def render_hip(xyz, rgb, poses, K, height, width, near=DEFAULT_NEAR, far=DEFAULT_FAR, splat=0.0, pose_scale=1.0, ortho=False,
               background=(0, 0, 0), workspace=None):
    """render_numpy as the launch chain of td_cloud_render -> Rendered of device tensors.  xyz float32 [V,3], rgb uint8 [V,3], poses
    float64 [C,3,4], all on one HIP device; K on the host.  ``workspace``: render_workspace's (None: allocated here); a too-small
    one is an error.  The call does not synchronise."""
    lib = native.load()
    native.require_device(xyz, rgb, poses)
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, splat, background)
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.dtype != torch.uint8 or tuple(rgb.shape) != tuple(xyz.shape) \
            or poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] < 1:
        raise ValueError("xyz float32 [V,3], rgb uint8 [V,3], poses float64 [C,3,4] with C >= 1; got %s %s, %s %s, %s %s" % (
            tuple(xyz.shape), xyz.dtype, tuple(rgb.shape), rgb.dtype, tuple(poses.shape), poses.dtype))
    k = _K9(K)
    C, V = poses.shape[0], xyz.shape[0]
    need = lib.td_cloud_render_workspace_bytes(C, H, W)
    if need <= 0 or V >= 0x7fffffff:
        raise native.NativeLibraryError("td_cloud_render: unsupported shape (C %d, %d x %d, V %d)" % (C, H, W, V))
    if workspace is None:
        workspace = render_workspace(C, H, W, xyz.device)
    native.require_device(workspace)
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise native.NativeLibraryError("td_cloud_render: the workspace holds %d bytes, (%d, %d, %d) needs %d" % (have, C, H, W, need))
    if V == 0:                                                              # an empty tensor has no address to pass
        xyz, rgb = torch.zeros(1, 3, dtype=torch.float32, device=poses.device), torch.zeros(1, 3, dtype=torch.uint8, device=poses.device)
    dev = poses.device
    depth, color = torch.empty(C, H, W, dtype=torch.float32, device=dev), torch.empty(C, 3, H, W, dtype=torch.uint8, device=dev)
    index, stats = torch.empty(C, H, W, dtype=torch.int32, device=dev), torch.empty(C, 5, dtype=torch.int64, device=dev)
    native.call("td_cloud_render", xyz.contiguous(), rgb.contiguous(), V, poses.contiguous(), (ctypes.c_double * 9)(*k), C, H, W,
                float(pose_scale), float(near), float(far), float(splat), bool(ortho), bg[0], bg[1], bg[2], workspace, have, depth, color,
                index, stats)
    return Rendered(depth, color, index, stats)


def render_surfels_hip(xyz, rgb, normals, poses, K, height, width, radius, near=DEFAULT_NEAR, far=DEFAULT_FAR, cull=False, ambient=1.0,
                       pose_scale=1.0, ortho=False, background=(0, 0, 0), workspace=None, form="auto"):
    """render_surfels_numpy as the launch chain of td_cloud_render_surfels -> SurfelRendered of device tensors.  xyz float32 [V,3], rgb
    uint8 [V,3], normals float32 [V,3], poses float64 [C,3,4], all on one HIP device; K on the host.  ``workspace``: render_workspace's
    (None: allocated here); a too-small one is an error.  ``form``: a key of SURFEL_FORMS.  The call does not synchronise."""
    lib = native.load()
    native.require_device(xyz, rgb, normals, poses)
    H, W = int(height), int(width)
    bg = _check_params(H, W, near, far, 0.0, background)
    if xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or rgb.dtype != torch.uint8 or tuple(rgb.shape) != tuple(xyz.shape) \
            or normals.dtype != torch.float32 or tuple(normals.shape) != tuple(xyz.shape) \
            or poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4) or poses.shape[0] < 1:
        raise ValueError("xyz float32 [V,3], rgb uint8 [V,3], normals float32 [V,3], poses float64 [C,3,4] with C >= 1; got %s %s, %s %s, "
                         "%s %s, %s %s" % (tuple(xyz.shape), xyz.dtype, tuple(rgb.shape), rgb.dtype, tuple(normals.shape), normals.dtype,
                                           tuple(poses.shape), poses.dtype))
    k = _K9(K)
    _check_surfel_params(radius, ambient, k)
    if form not in SURFEL_FORMS:
        raise ValueError("form: one of %s, got %r" % (sorted(SURFEL_FORMS), form))
    C, V = poses.shape[0], xyz.shape[0]
    need = lib.td_cloud_render_workspace_bytes(C, H, W)
    if need <= 0 or V >= 0x7fffffff:
        raise native.NativeLibraryError("td_cloud_render_surfels: unsupported shape (C %d, %d x %d, V %d)" % (C, H, W, V))
    if workspace is None:
        workspace = render_workspace(C, H, W, xyz.device)
    native.require_device(workspace)
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise native.NativeLibraryError("td_cloud_render_surfels: the workspace holds %d bytes, (%d, %d, %d) needs %d" % (have, C, H, W, need))
    dev = poses.device
    if V == 0:                                                              # an empty tensor has no address to pass
        xyz, normals = torch.zeros(1, 3, dtype=torch.float32, device=dev), torch.zeros(1, 3, dtype=torch.float32, device=dev)
        rgb = torch.zeros(1, 3, dtype=torch.uint8, device=dev)
    depth, color = torch.empty(C, H, W, dtype=torch.float32, device=dev), torch.empty(C, 3, H, W, dtype=torch.uint8, device=dev)
    index, nmap = torch.empty(C, H, W, dtype=torch.int32, device=dev), torch.empty(C, 3, H, W, dtype=torch.float32, device=dev)
    stats = torch.empty(C, 8, dtype=torch.int64, device=dev)
    native.call("td_cloud_render_surfels", xyz.contiguous(), rgb.contiguous(), normals.contiguous(), V, poses.contiguous(),
                (ctypes.c_double * 9)(*k), C, H, W, float(pose_scale), float(near), float(far), float(radius), bool(ortho), bool(cull),
                float(ambient), SURFEL_FORMS[form], bg[0], bg[1], bg[2], workspace, have, depth, color, index, nmap, stats)
    return SurfelRendered(depth, color, index, nmap, stats)


# ---------------------------------------------------------------------------------------------------------------------------

class CloudRenderer:
    """render(xyz, rgb, poses) -> Rendered of host arrays for any number of poses.

    device      'cuda[:i]': the cloud is uploaded once, ``batch_size`` cameras go through one launch chain of td_cloud_render at a
                time, every batch into the same workspace, and each batch's maps are copied back before the next one is drawn
                (the only synchronisation).  'cpu': render_numpy.
    K           the 3x3 block in pixels at ``height`` x ``width``
    near, far, splat   in the cloud's units; splat = the world size a point is drawn with (the fuser's voxel), 0: one pixel per point
    pose_scale  multiplies the poses' translations, as in cloud.SceneFuser
    """

    def __init__(self, device, height, width, K, near=DEFAULT_NEAR, far=DEFAULT_FAR, splat=DEFAULT_SPLAT, pose_scale=1.0, batch_size=12):
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        if self.on_hip and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.height, self.width = int(height), int(width)
        _check_params(self.height, self.width, near, far, splat, (0, 0, 0))
        if int(batch_size) < 1:
            raise ValueError("batch_size: at least 1, got %r" % (batch_size,))
        self.K = _K9(K).reshape(3, 3)
        self.params = dict(near=float(near), far=float(far), splat=float(splat), pose_scale=float(pose_scale))
        self.batch_size = int(batch_size)
        self._workspace = None

    def upload(self, xyz, rgb):
        """The cloud where render() wants it: device tensors (host arrays on 'cpu').  For several render() calls on one cloud."""
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        xyz, rgb, _ = _check_cloud(host(xyz), host(rgb), np.zeros((1, 3, 4)))
        return (torch.from_numpy(xyz).to(self.device), torch.from_numpy(rgb).to(self.device)) if self.on_hip else (xyz, rgb)

    def render(self, xyz, rgb, poses, K=None, ortho=False, background=(0, 0, 0), **params):
        """``xyz``, ``rgb``: arrays or tensors anywhere (upload()'s are used as they are).  ``K``, ``ortho`` and any of near / far /
        splat / pose_scale override the renderer's for this call (a top view)."""
        uploaded = self.on_hip and all(torch.is_tensor(t) and t.device == self.device for t in (xyz, rgb))
        xyz_d, rgb_d = (xyz, rgb) if uploaded else self.upload(xyz, rgb)      # the one upload of the cloud
        poses = _check_cloud(np.zeros((0, 3)), np.zeros((0, 3)), poses.cpu().numpy() if torch.is_tensor(poses) else poses)[2]
        K = self.K if K is None else K
        args = dict(self.params, ortho=bool(ortho), background=background, **params)
        if not self.on_hip:
            return render_numpy(xyz_d, rgb_d, poses, K, self.height, self.width, **args)
        poses_d = torch.from_numpy(poses).to(self.device)
        if self._workspace is None:
            self._workspace = render_workspace(self.batch_size, self.height, self.width, self.device)
        parts = []
        for at in range(0, len(poses), self.batch_size):
            out = render_hip(xyz_d, rgb_d, poses_d[at:at + self.batch_size], K, self.height, self.width, workspace=self._workspace, **args)
            parts.append([t.cpu().numpy() for t in out])
        return Rendered(*(np.concatenate([p[j] for p in parts], 0) for j in range(4)))

    def render_surfels(self, xyz, rgb, normals, poses, radius=None, cull=False, ambient=1.0, K=None, ortho=False, background=(0, 0, 0),
                       **params):
        """render() with every point drawn as a disc in space -> SurfelRendered of host arrays.  ``normals`` [V,3]: float32 like a
        PLY's (a float64 array is rounded), all zero where a point has none; orient them first (cloud_normals) when ``cull`` or
        ``ambient`` < 1 is to mean anything.  ``radius``: the discs', in the cloud's units, None: DEFAULT_SPLAT (a disc as wide as
        two voxels: it covers its voxel's diagonal, UNTUNED).  near / far / pose_scale can be overridden as in render()."""
        host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        uploaded = self.on_hip and all(torch.is_tensor(t) and t.device == self.device for t in (xyz, rgb))
        xyz_d, rgb_d = (xyz, rgb) if uploaded else self.upload(xyz, rgb)
        poses = _check_cloud(np.zeros((0, 3)), np.zeros((0, 3)), host(poses))[2]
        K = self.K if K is None else K
        args = {name: v for name, v in self.params.items() if name != "splat"}
        args.update(cull=bool(cull), ambient=float(ambient), ortho=bool(ortho), background=background, **params)
        radius = DEFAULT_SPLAT if radius is None else float(radius)
        if not self.on_hip:
            return render_surfels_numpy(xyz_d, rgb_d, host(normals), poses, K, self.height, self.width, radius, **args)
        if torch.is_tensor(normals) and normals.device == self.device and normals.dtype == torch.float32:
            normals_d = normals
        else:
            normals_d = torch.from_numpy(np.ascontiguousarray(host(normals), dtype=np.float32)).to(self.device)
        poses_d = torch.from_numpy(poses).to(self.device)
        if self._workspace is None:
            self._workspace = render_workspace(self.batch_size, self.height, self.width, self.device)
        parts = []
        for at in range(0, len(poses), self.batch_size):
            out = render_surfels_hip(xyz_d, rgb_d, normals_d, poses_d[at:at + self.batch_size], K, self.height, self.width, radius,
                                     workspace=self._workspace, **args)
            parts.append([t.cpu().numpy() for t in out])
        return SurfelRendered(*(np.concatenate([p[j] for p in parts], 0) for j in range(5)))
