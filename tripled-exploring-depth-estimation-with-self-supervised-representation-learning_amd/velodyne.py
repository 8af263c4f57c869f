"""KITTI ground-truth depth maps from the raw velodyne scans: what every evaluation path of this build reads, made from the raw tree.

The reference makes its ground truth per frame with generate_depth_map (mono/datasets/kitti_utils.py:50-102, called by
KITTIRAWDataset.get_depth, mono/datasets/kitti_dataset.py:201-215): project the scan into the image, let the last point on a pixel
win, then resolve duplicates with a Counter and a Python loop.  Here a batch of scans becomes a batch of maps in one launch chain
(csrc/td_velo.hip), bit-identical from run to run and equal to the numpy statement below.

Three layers, as in cloud.py and odometry.py:
  * host statements in numpy (``read_calib_file``, ``velo_to_image``, ``load_velodyne_points``, ``depth_map_numpy`` and the literal
    per-point loop ``depth_map_bruteforce``): the host path (``device='cpu'``) and what the kernel is tested against.  The projection
    is written element-wise in the kernel's operation order, with no ``@``, which BLAS may round differently;
  * ``depth_maps_hip`` / ``velo_workspace``: td_velo_depth.  Device tensors only; a CPU tensor is an error;
  * ``VelodyneGroundTruth``: (folder, frame_index, side) lists -> (gt, sizes, crops) on the device, the arguments of
    evaluate.evaluate_disparity_hip; ``batch_ground_truth`` is the same for scans that are already in memory.

What is computed (float64, every product and sum rounded on its own):
  1. keep points with x >= 0 (a float32 compare: -0.0 passes, a NaN does not);
  2. r_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3;  u = rint(r_0 / r_2) - 1, v = rint(r_1 / r_2) - 1 (half to even, like np.round);
  3. valid when 0 <= u < W and 0 <= v < H: NaN and inf fail the compares, r_2 < 0 can pass them (a negative depth takes part);
  4. d = r_2, or float64(x) with vel_depth;
  5. a pixel takes the d of the LAST valid point on it, in file order;
  6. points are grouped by g = v (W-1) + u - 1, the reference's sub2ind, not by pixel: pixel (v, W-1) shares a group with pixel
     (v+1, 0), and g = -1 is pixel (0,0).  For a group of more than one point, the pixel of the group's FIRST point is overwritten
     with the minimum d of the whole group; the group's other pixel keeps its last-write value;
  7. values < 0 become 0, pixels nobody hit are 0.  The map is float64; the ground truth this build evaluates against is float32(map).

Deviations from the reference: get_depth's scipy.misc.imresize(depth, full_res_shape, "nearest") is not applied (the function no
longer exists, it byte-scaled the map, and the evaluation reads ground truth at native size); the minimum of a group is taken over an
order-preserving map of the doubles' bits, so -0.0 sorts below +0.0 where np.min returns whichever comes first (both compare equal and
neither is clamped); the reference's np.dot rounds the four-term products through BLAS, within 1.5e-14 absolute of these statements.
"""
import os

import numpy as np
import torch

from . import native

STATS = ("points", "behind", "outside", "valid", "pixels_hit", "pixels_clamped")
SIDE_CAM = {"2": 2, "3": 3, "l": 2, "r": 3}
_SIGN = np.uint64(1 << 63)


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def read_calib_file(path):
    """A KITTI calibration file -> {key: float64 array, or the text where a token is no number} (kitti_utils.py:21-40)."""
    data = {}
    with open(path, "r") as f:
        for line in f:
            if ":" not in line:
                continue
            key, value = line.split(":", 1)
            value = value.strip()
            try:
                data[key] = np.array([float(t) for t in value.split(" ")], dtype=np.float64)
            except ValueError:
                data[key] = value
    return data


def velo_to_image(calib_dir, cam=2):
    """(P float64 [3,4] = P_rect_0{cam} . R_rect_00 (4x4) . [R|T]_velo_to_cam (4x4), (H, W) = S_rect_02 reversed).  The size is read
    from S_rect_02 for camera 3 too, as the reference does (kitti_utils.py:54-66)."""
    cam2cam = read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
    velo2cam = read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
    return projection_matrix(cam2cam["P_rect_0%d" % int(cam)], cam2cam["R_rect_00"], velo2cam["R"], velo2cam["T"]), \
        image_size(cam2cam["S_rect_02"])


def projection_matrix(P_rect, R_rect_00, R, T):
    """The three small products of velo_to_image from the calibration files' numbers; np.dot on the host, as the reference."""
    velo2cam = np.vstack((np.hstack((np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 1))),
                          np.array([0, 0, 0, 1.0])))
    R_cam2rect = np.eye(4)
    R_cam2rect[:3, :3] = np.asarray(R_rect_00, np.float64).reshape(3, 3)
    return np.dot(np.dot(np.asarray(P_rect, np.float64).reshape(3, 4), R_cam2rect), velo2cam)


def image_size(S_rect):
    h, w = np.asarray(S_rect)[::-1].astype(np.int32)
    return int(h), int(w)


def load_velodyne_points(path):
    """A KITTI scan -> float32 [N,4] (x forward, y left, z up, 1): the reflectance column is overwritten, as the reference does."""
    points = np.fromfile(path, dtype=np.float32).reshape(-1, 4)
    points[:, 3] = 1.0
    return points


def ordered_bits(d):
    """float64 -> uint64 with the same order, negative values included (csrc/td_velo.hip: ordered_bits)."""
    b = np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)
    return np.where((b & _SIGN) != 0, ~b, b | _SIGN)


def from_ordered_bits(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k & _SIGN) != 0, k & ~_SIGN, ~k).astype(np.uint64).view(np.float64)


def _check_frame(points, P, H, W):
    pts = np.ascontiguousarray(points, dtype=np.float32)
    if pts.ndim != 2 or pts.shape[1] != 4:
        raise ValueError("points: float32 [N,4], got %s" % (pts.shape,))
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.shape != (3, 4):
        raise ValueError("P: float64 [3,4], got %s" % (P.shape,))
    H, W = int(H), int(W)
    if H < 1 or W < 2:
        raise ValueError("a map of at least 1 x 2 pixels (the group index needs W >= 2), got %d x %d" % (H, W))
    return pts, P, H, W


def depth_map_numpy(points, P, H, W, vel_depth=False):
    """One scan -> (depth float64 [H,W], stats int64 [6] in the order of STATS).  The statement td_velo_depth is tested against,
    operation for operation: every table is an order-independent reduction over the points."""
    pts, P, H, W = _check_frame(points, P, H, W)
    n = len(pts)
    xf = pts[:, 0]
    behind = int(np.count_nonzero(xf < np.float32(0)))
    idx = np.nonzero(xf >= np.float32(0))[0]                            # a NaN fails both compares: kept out, counted outside
    x, y, z = (pts[idx, k].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        r = [((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3)]
        u = np.rint(r[0] / r[2]) - 1.0
        v = np.rint(r[1] / r[2]) - 1.0
        valid = (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(H))
    idx = idx[valid]
    ui, vi = u[valid].astype(np.int64), v[valid].astype(np.int64)
    d = (x if vel_depth else r[2])[valid]
    pix = vi * W + ui
    g = vi * (W - 1) + ui                                               # the reference's index + 1: pixel (0,0) is entry 0
    n_groups = H * (W - 1) + 1
    last = np.full(H * W, -1, np.int64)
    np.maximum.at(last, pix, idx)
    first_of_group = np.full(n_groups, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first_of_group, g, idx)
    min_of_group = np.full(n_groups, np.iinfo(np.uint64).max, np.uint64)
    np.minimum.at(min_of_group, g, ordered_bits(d))
    members = np.bincount(g, minlength=n_groups)
    d_of = np.zeros(n, np.float64)
    d_of[idx] = d
    pix_of = np.zeros(n, np.int64)
    pix_of[idx] = pix
    depth = np.zeros(H * W, np.float64)
    hit = last >= 0
    depth[hit] = d_of[last[hit]]
    dup = np.nonzero(members > 1)[0]
    depth[pix_of[first_of_group[dup]]] = from_ordered_bits(min_of_group[dup])      # groups write to distinct pixels
    negative = depth < 0
    depth[negative] = 0
    stats = np.array([n, behind, n - behind - len(idx), len(idx), np.count_nonzero(hit), np.count_nonzero(negative)], np.int64)
    return depth.reshape(H, W), stats


def depth_map_bruteforce(points, P, H, W, vel_depth=False):
    """depth_map_numpy as a plain loop over the points that follows the seven steps literally.  For the tests and the benchmark."""
    pts, P, H, W = _check_frame(points, P, H, W)
    depth = np.zeros((H, W), np.float64)
    touched = np.zeros((H, W), bool)
    groups = {}                                                         # g -> [pixel of its first point, members, minimum d]
    behind = outside = n_valid = 0
    with np.errstate(all="ignore"):
        for p in pts:
            if p[0] < np.float32(0):
                behind += 1
                continue
            if not p[0] >= np.float32(0):
                outside += 1
                continue
            x, y, z = np.float64(p[0]), np.float64(p[1]), np.float64(p[2])
            r0, r1, r2 = (((P[k, 0] * x + P[k, 1] * y) + P[k, 2] * z) + P[k, 3] for k in range(3))
            u, v = np.rint(r0 / r2) - 1.0, np.rint(r1 / r2) - 1.0
            if not (0 <= u < W and 0 <= v < H):
                outside += 1
                continue
            n_valid += 1
            ui, vi = int(u), int(v)
            d = x if vel_depth else r2
            depth[vi, ui] = d                                           # the last one in file order stays
            touched[vi, ui] = True
            g = vi * (W - 1) + ui - 1
            if g not in groups:
                groups[g] = [(vi, ui), 1, d]
            else:
                groups[g][1] += 1
                if d < groups[g][2]:
                    groups[g][2] = d
    for (vi, ui), members, smallest in groups.values():
        if members > 1:
            depth[vi, ui] = smallest
    negative = depth < 0
    depth[negative] = 0
    return depth, np.array([len(pts), behind, outside, n_valid, np.count_nonzero(touched), np.count_nonzero(negative)], np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernel

def velo_workspace(B, Hmax, Wmax, device):
    """The scratch buffer of depth_maps_hip for batches up to this shape (uint8, td_velo_depth_workspace_bytes)."""
    n = native.load().td_velo_depth_workspace_bytes(int(B), int(Hmax), int(Wmax))
    if n <= 0:
        raise native.NativeLibraryError("td_velo_depth_workspace_bytes(%d, %d, %d): unsupported shape" % (B, Hmax, Wmax))
    return torch.empty(n, dtype=torch.uint8, device=device)


def depth_maps_hip(points, offsets, P, sizes, vel_depth=False, workspace=None, max_size=None):
    """B scans -> (gt float32 [B,Hmax,Wmax] zero-padded at the bottom and right, stats int64 [B,6]) as the launch chain of
    td_velo_depth.  points float32 [Ntot,4] (the scans concatenated), offsets int64 [B+1], P float64 [B,3,4], sizes int32 [B,2] =
    (H, W), all on one HIP device.  max_size = (Hmax, Wmax) from the caller's host copy of the sizes; without it the maximum is read
    back from ``sizes``, which is the call's only synchronisation.  A too-small ``workspace`` is an error."""
    lib = native.load()
    native.require_device(points, offsets, P, sizes)
    if points.dim() != 2 or points.shape[1] != 4 or points.dtype != torch.float32:
        raise ValueError("points: float32 [Ntot,4], got %s %s" % (tuple(points.shape), points.dtype))
    B = sizes.shape[0] if sizes.dim() == 2 else 0
    if B < 1 or tuple(sizes.shape) != (B, 2) or sizes.dtype != torch.int32:
        raise ValueError("sizes: int32 [B,2] with B >= 1, got %s %s" % (tuple(sizes.shape), sizes.dtype))
    if tuple(offsets.shape) != (B + 1,) or offsets.dtype != torch.int64:
        raise ValueError("offsets: int64 [%d], got %s %s" % (B + 1, tuple(offsets.shape), offsets.dtype))
    if tuple(P.shape) != (B, 3, 4) or P.dtype != torch.float64:
        raise ValueError("P: float64 [%d,3,4], got %s %s" % (B, tuple(P.shape), P.dtype))
    Hmax, Wmax = (int(v) for v in (max_size if max_size is not None else sizes.amax(0).tolist()))
    need = lib.td_velo_depth_workspace_bytes(B, Hmax, Wmax)
    if need <= 0:
        raise native.NativeLibraryError("td_velo_depth: unsupported batch shape (%d, %d, %d)" % (B, Hmax, Wmax))
    if workspace is None:
        workspace = velo_workspace(B, Hmax, Wmax, points.device)
    native.require_device(workspace)
    have = workspace.numel() * workspace.element_size()
    if have < need:
        raise native.NativeLibraryError("td_velo_depth: the workspace holds %d bytes, (%d, %d, %d) needs %d" % (have, B, Hmax, Wmax, need))
    if points.shape[0] == 0:                                            # an empty tensor has no address to pass
        points = torch.zeros(1, 4, dtype=torch.float32, device=points.device)
    gt = torch.empty(B, Hmax, Wmax, dtype=torch.float32, device=points.device)
    stats = torch.empty(B, 6, dtype=torch.int64, device=points.device)
    native.call("td_velo_depth", points, offsets, B, P, sizes, Hmax, Wmax, bool(vel_depth), workspace, have, gt, stats)
    return gt, stats


# ---------------------------------------------------------------------------------------------------------------------------
# batches

def batch_ground_truth(scans, Ps, sizes, device, vel_depth=False, workspace=None):
    """Scans in host memory -> the ground truth of a batch.  scans: float32 [N_i,4] arrays, Ps: [3,4] float64, sizes: (H, W).
    On a HIP device: (gt, sizes, crops) as evaluate.pad_ground_truth returns them, after ONE upload of the concatenated points and
    one launch chain.  On 'cpu': the statement's maps, float32, as a list."""
    from . import evaluate
    device = torch.device(device)
    scans = [np.ascontiguousarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1, 4) for s in scans]
    Ps = np.stack([np.asarray(p.cpu() if torch.is_tensor(p) else p, dtype=np.float64).reshape(3, 4) for p in Ps], 0)
    sizes = np.array([[int(v) for v in s] for s in sizes], dtype=np.int32).reshape(-1, 2)
    if not (len(scans) == len(Ps) == len(sizes)) or not len(scans):
        raise ValueError("one P and one size per scan, at least one scan")
    if sizes[:, 0].min() < 1 or sizes[:, 1].min() < 2:
        raise ValueError("maps of at least 1 x 2 pixels, got %s" % (sizes.tolist(),))
    if device.type != "cuda":
        return [depth_map_numpy(s, p, h, w, vel_depth)[0].astype(np.float32) for s, p, (h, w) in zip(scans, Ps, sizes)]
    offsets = np.zeros(len(scans) + 1, np.int64)
    np.cumsum([len(s) for s in scans], out=offsets[1:])
    points = torch.from_numpy(np.concatenate(scans, 0)).to(device)      # the one upload of the points
    crops = np.stack([evaluate.garg_crop(int(h), int(w)) for h, w in sizes], 0)
    sizes_d = torch.from_numpy(sizes).to(device)
    gt, _ = depth_maps_hip(points, torch.from_numpy(offsets).to(device), torch.from_numpy(Ps).to(device), sizes_d, vel_depth,
                           workspace, max_size=(int(sizes[:, 0].max()), int(sizes[:, 1].max())))
    return gt, sizes_d, torch.from_numpy(crops).to(device)


def sample_ground_truth(sample):
    """The float32 ground truth of one validation sample on the host: its "gt_depth", or the statement's map of its "velo" scan."""
    if "gt_depth" in sample:
        return np.asarray(torch.as_tensor(sample["gt_depth"]).cpu(), dtype=np.float32)
    h, w = (int(v) for v in sample["gt_size"])
    return depth_map_numpy(np.asarray(sample["velo"]), np.asarray(sample["velo_P"]), h, w)[0].astype(np.float32)


class VelodyneGroundTruth:
    """gt(items) with items = [(folder, frame_index, side), ...] as the split lists name them -> (gt, sizes, crops) on the device
    (a list of float32 maps on 'cpu').  Every scan is read once, P and the size are cached per (date, camera), and a batch's points
    travel in one upload."""

    def __init__(self, data_path, device, vel_depth=False):
        self.data_path = data_path
        self.device = torch.device(device)
        self.vel_depth = bool(vel_depth)
        self._calib = {}
        self._workspace = None

    def calibration(self, folder, side):
        key = (folder.split("/")[0], SIDE_CAM[str(side)])
        if key not in self._calib:
            self._calib[key] = velo_to_image(os.path.join(self.data_path, key[0]), key[1])
        return self._calib[key]

    def scan_path(self, folder, frame_index):
        return os.path.join(self.data_path, folder, "velodyne_points/data/{:010d}.bin".format(int(frame_index)))

    def __call__(self, items):
        items = list(items)
        calib = [self.calibration(folder, side) for folder, _, side in items]
        scans = [load_velodyne_points(self.scan_path(folder, frame_index)) for folder, frame_index, _ in items]
        sizes = [c[1] for c in calib]
        if self.device.type == "cuda":
            B, Hmax, Wmax = len(items), max(s[0] for s in sizes), max(s[1] for s in sizes)
            need = native.load().td_velo_depth_workspace_bytes(B, Hmax, Wmax)
            if self._workspace is None or self._workspace.numel() < need:
                self._workspace = velo_workspace(B, Hmax, Wmax, self.device)
        return batch_ground_truth(scans, [c[0] for c in calib], sizes, self.device, self.vel_depth, self._workspace)
