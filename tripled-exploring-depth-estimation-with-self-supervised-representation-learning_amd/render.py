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
"""
import collections
import ctypes

import numpy as np
import torch

from . import cloud, native

MAX_SPLAT = 8                        # csrc/td_render.hip: TD_RENDER_MAX_SPLAT
STATS = ("points", "out_of_range", "outside", "drawn", "pixels_hit")
_NONE = np.uint64(0xffffffffffffffff)

# In the MODEL's units, like cloud.py's.  UNTUNED: nobody has looked at a rendering of a trained checkpoint's cloud with them.
DEFAULT_NEAR = cloud.DEFAULT_MIN_DEPTH       # what the fuser does not back-project is not drawn either
DEFAULT_FAR = 4.0 * cloud.DEFAULT_MAX_RANGE  # a view sees farther than one frame contributed
DEFAULT_SPLAT = cloud.DEFAULT_VOXEL          # a point stands for its voxel

Rendered = collections.namedtuple("Rendered", "depth color index stats")
Rendered.__doc__ = """depth float32 [C,H,W] (float32(z) of the pixel's point, 0 where nothing was drawn), color uint8 [C,3,H,W] (the
background where nothing was drawn), index int32 [C,H,W] (the point's row in the cloud, -1 where nothing was drawn), stats int64 [C,5]
in the order of STATS: points, out of range, outside (in range but the square misses the image), drawn, pixels hit."""


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
