"""KITTI odometry evaluation: a pose checkpoint and a sequence in, the trajectory, the 5-frame snippet ATE and the KITTI
t_err / r_err over 100 ... 800 m segments out.

The protocol is the reference's scripts/eval_pose.py (snippet ATE with dump_xyz and compute_ate), scripts/draw_odometry.py (the
trajectory, written as KITTI pose text) and mono/tools/kitti_evaluation_toolkit.py (scale-only Umeyama alignment, segment errors).
The reference runs at batch 1, decodes and uploads every frame twice (sample i carries frames i and i+1), copies one 4x4 to the
host per frame and loops over np.linalg.inv / np.dot in Python.  Here every frame is decoded and uploaded once as uint8, the pairs
are formed on the device, the relative transforms stay there, and the trajectory, the snippet ATEs and the segment errors are
three launches whose results are copied to the host once.

Three layers, as in infer.py and evaluate.py:
  * host statements in numpy float64 (``trajectory_numpy``, ``snippet_ates_numpy``, ``sequence_errors_numpy``,
    ``umeyama_scale_numpy``, ``overall_errors``, ``segment_errors``, ``load_kitti_poses`` / ``save_kitti_poses``, ``pairs_torch``):
    the host path (``device='cpu'``) and what the kernels are tested against;
  * ``pairs_hip``, ``trajectory_hip``, ``snippet_ates_hip``, ``sequence_errors_hip``: csrc/td_odom.hip.  Device tensors only; a CPU
    tensor is an error.  No synchronisation;
  * ``OdometryEvaluator``: frames of a dataset -> pairs -> PoseEncoder / PoseDecoder -> td_pose_fwd -> the three metric kernels.

Deviations from the reference (DESIGN.md section 16 has the measured distances): a float32 relative transform is widened to float64
before it is inverted (np.linalg.inv of a float32 array stays in float32), and the in-memory poses are scored, not their %1.8e text.
"""
import collections
import ctypes

import numpy as np
import torch

from . import infer, native

LENGTHS = (100, 200, 300, 400, 500, 600, 700, 800)
STEP = 10
TRACK_LENGTH = 5
MAX_LENGTHS = native.CONSTANTS["TD_ODOM_MAX_LENGTHS"]
TRAJECTORY_THREADS = native.CONSTANTS["TD_ODOM_THREADS"]      # the workgroup of td_odom_trajectory (a thread owns ceil(n / 256) steps)

OdometryResult = collections.namedtuple(
    "OdometryResult", "ate_mean ate_std t_err r_err scale distance poses ates segments relative")
OdometryResult.__doc__ = """ate_mean, ate_std: np.mean / np.std of ``ates`` [n];  t_err, r_err: the means over ``segments``
(fractions and rad/m: x 100 and x 180 / pi for the toolkit's % and deg/m; NaN when no segment fits);  scale: the Umeyama scale
applied to the predicted translations;  distance: the ground truth's length in m;  poses [n+1,3,4] (unscaled);  segments [k,5]:
first_frame, r_err / len, t_err / len, len, speed;  relative: the [n,4,4] float32 relative transforms, on the evaluator's device."""


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def _as_4x4(poses):
    """[m,3,4] or [m,4,4] -> float64 [m,4,4]."""
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim != 3 or p.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("poses: [m,3,4] or [m,4,4], got %s" % (p.shape,))
    out = np.zeros((p.shape[0], 4, 4))
    out[:, :3] = p[:, :3]
    out[:, 3, 3] = 1.0
    return out


def load_kitti_poses(path):
    """KITTI pose text (12 numbers per line, the top three rows of the 4x4) -> float64 [m,3,4]."""
    return np.loadtxt(path, dtype=np.float64, ndmin=2).reshape(-1, 3, 4)


def save_kitti_poses(path, poses):
    """[m,3,4] (or [m,4,4]) -> KITTI pose text at %1.8e, the reference's np.savetxt(..., delimiter=' ', fmt='%1.8e')."""
    np.savetxt(path, _as_4x4(poses)[:, :3].reshape(-1, 12), delimiter=" ", fmt="%1.8e")


def pairs_torch(frames):
    """uint8 [n+1,3,H,W] -> float32 [n,6,H,W]: pair i = cat(ToTensor(frame i), ToTensor(frame i+1)), reference eval_pose.py:59."""
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 2:
        raise ValueError("frames: uint8 [n+1,3,H,W] with n >= 1, got %s %s" % (tuple(frames.shape), frames.dtype))
    x = frames.to(torch.float32) / 255.0
    return torch.cat([x[:-1], x[1:]], 1)


def trajectory_numpy(rel):
    """Relative transforms [n,4,4] (frame k+1 -> frame k) -> global poses float64 [n+1,3,4]: G_0 = I, G_{k+1} = G_k inv(M_k)
    (reference draw_odometry.py:62-74), every transform widened to float64 before it is inverted."""
    rel = np.asarray(rel, dtype=np.float64)
    g = np.identity(4)
    out = [g[:3].copy()]
    for m in rel:
        g = g @ np.linalg.inv(m)
        out.append(g[:3].copy())
    return np.stack(out, 0)


def _dump_xyz(transforms):
    cam_to_world = np.eye(4)
    xyzs = [cam_to_world[:3, 3]]
    for t in transforms:
        cam_to_world = np.dot(cam_to_world, t)
        xyzs.append(cam_to_world[:3, 3])
    return np.array(xyzs)


def _compute_ate(gt_xyz, pred_xyz):
    pred_xyz = pred_xyz + (gt_xyz[0] - pred_xyz[0])[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.sum(gt_xyz * pred_xyz) / np.sum(pred_xyz ** 2)
    err = pred_xyz * scale - gt_xyz
    return np.sqrt(np.sum(err ** 2)) / gt_xyz.shape[0]


def snippet_ates_numpy(rel, gt_poses, track_length=TRACK_LENGTH):
    """Predicted relative transforms [n,4,4] + ground-truth global poses [n+1,3,4] -> float64 [n]: reference eval_pose.py:66-80.
    The last track_length - 2 snippets are shorter; each divides by its own point count; 0 / 0 gives NaN."""
    rel = np.asarray(rel, dtype=np.float64)
    gt = _as_4x4(gt_poses)
    if rel.ndim != 3 or rel.shape[1:] != (4, 4) or gt.shape[0] != rel.shape[0] + 1:
        raise ValueError("rel: [n,4,4], gt_poses: [n+1,3,4]; got %s and %s" % (rel.shape, gt.shape))
    if not 2 <= int(track_length) <= 16:
        raise ValueError("track_length: 2 ... 16, got %r" % (track_length,))
    local = [np.linalg.inv(np.dot(np.linalg.inv(gt[i - 1]), gt[i])) for i in range(1, len(gt))]
    ates = [_compute_ate(_dump_xyz(local[i:i + track_length - 1]), _dump_xyz(rel[i:i + track_length - 1]))
            for i in range(len(rel))]
    return np.array(ates, dtype=np.float64)


def umeyama_scale_numpy(pred_xyz, gt_xyz):
    """The scale c of geometry.umeyama_alignment(pred.T, gt.T, with_scale=True): trace(diag(d) S) / sigma_x."""
    x, y = np.asarray(pred_xyz, np.float64).T, np.asarray(gt_xyz, np.float64).T
    n = x.shape[1]
    mean_x, mean_y = x.mean(axis=1), y.mean(axis=1)
    sigma_x = 1.0 / n * (np.linalg.norm(x - mean_x[:, None]) ** 2)
    cov = (y - mean_y[:, None]) @ (x - mean_x[:, None]).T / n
    u, d, v = np.linalg.svd(cov)
    s = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        s[2, 2] = -1
    return float(1 / sigma_x * np.trace(np.diag(d).dot(s)))


def trajectory_distances(gt_poses):
    """trajectoryDistances: cumulative distance, accumulated sequentially in index order (float64 [m])."""
    t = np.asarray(gt_poses, dtype=np.float64)[:, :3, 3]
    dist = [0.0]
    for i in range(len(t) - 1):
        dx, dy, dz = float(t[i, 0] - t[i + 1, 0]), float(t[i, 1] - t[i + 1, 1]), float(t[i, 2] - t[i + 1, 2])
        dist.append(dist[i] + np.sqrt(dx ** 2 + dy ** 2 + dz ** 2))
    return np.array(dist, dtype=np.float64)


def _last_frame(dist, first, length):
    """lastFrameFromSegmentLength: the first i >= first with dist[i] > dist[first] + length, or -1."""
    i = int(np.searchsorted(dist, dist[first] + length, side="right"))      # dist is non-decreasing
    return max(i, first) if i < len(dist) else -1


def sequence_errors_numpy(gt_poses, pred_poses, lengths=LENGTHS, step=STEP, align_scale=True):
    """The toolkit's eval core -> (rows float64 [k,5] in its order: first_frame major, length minor, segments that do not fit
    dropped; scale; total distance).  Row: first_frame, r_err / len, t_err / len, len, speed."""
    gt, pred = _as_4x4(gt_poses), _as_4x4(pred_poses)
    if gt.shape != pred.shape:
        raise ValueError("gt_poses and pred_poses: the same number of poses, got %d and %d" % (len(gt), len(pred)))
    scale = umeyama_scale_numpy(pred[:, :3, 3], gt[:, :3, 3]) if align_scale else 1.0
    pred = pred.copy()
    pred[:, :3, 3] = scale * pred[:, :3, 3]
    dist = trajectory_distances(gt)
    rows = []
    for first in range(0, len(gt), int(step)):
        for length in lengths:
            last = _last_frame(dist, first, length)
            if last == -1:
                continue
            delta_gt = np.dot(np.linalg.inv(gt[first]), gt[last])
            delta_pred = np.dot(np.linalg.inv(pred[first]), pred[last])
            err = np.dot(np.linalg.inv(delta_pred), delta_gt)
            d = 0.5 * (err[0, 0] + err[1, 1] + err[2, 2] - 1.0)
            r_err = np.arccos(max(min(d, 1.0), -1.0))
            t_err = np.sqrt(err[0, 3] ** 2 + err[1, 3] ** 2 + err[2, 3] ** 2)
            num_frames = last - first + 1.0
            rows.append([first, r_err / length, t_err / length, length, length / (0.1 * num_frames)])
    return np.array(rows, dtype=np.float64).reshape(-1, 5), scale, float(dist[-1])


def overall_errors(rows):
    """computeOverallErr: (mean t_err, mean r_err) over the rows; (NaN, NaN) when there is none."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    if not len(rows):
        return float("nan"), float("nan")
    return float(np.sum(rows[:, 2]) / len(rows)), float(np.sum(rows[:, 1]) / len(rows))


def segment_errors(rows, lengths=LENGTHS):
    """computeSegmentErr: {length: [mean t_err, mean r_err]} ([] for a length without rows)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    out = {}
    for length in lengths:
        sel = rows[rows[:, 3] == length]
        out[length] = [float(np.mean(sel[:, 2])), float(np.mean(sel[:, 1]))] if len(sel) else []
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def _rel(rel):
    native.require_device(rel)
    if rel.dim() != 3 or tuple(rel.shape[1:]) != (4, 4) or rel.shape[0] < 1 or rel.dtype not in (torch.float32, torch.float64):
        raise ValueError("rel: float32 / float64 [n,4,4] with n >= 1, got %s %s" % (tuple(rel.shape), rel.dtype))
    return rel.contiguous(), 1 if rel.dtype == torch.float64 else 0


def _poses(p, name, m=None):
    native.require_device(p)
    if p.dim() != 3 or tuple(p.shape[1:]) != (3, 4) or p.dtype != torch.float64 or (m is not None and p.shape[0] != m):
        raise ValueError("%s: float64 [%s,3,4], got %s %s" % (name, "m" if m is None else m, tuple(p.shape), p.dtype))
    return p.contiguous()


def _out(out, shape, dtype, device, name):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_cuda or not out.is_contiguous():
        raise ValueError("%s: contiguous %s %s on the device, got %s %s" % (name, dtype, tuple(shape), tuple(out.shape), out.dtype))
    return out


def pairs_hip(frames, dtype=torch.float32, first=0, count=None, out=None, out_first=None):
    """pairs_torch as td_pose_pairs_u8: pairs [first, first+count) of uint8 frames [n+1,3,H,W] as ``dtype`` (fp32 / bf16).
    Without ``out`` a new [count,6,H,W]; with ``out`` [.,6,H,W] the pairs go to its rows out_first ... (default: ``first``, a window
    of the full [n,6,H,W] array; 0 fills a batch buffer) and the other rows are left alone."""
    native.require_device(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 2:
        raise ValueError("frames: uint8 [n+1,3,H,W] with n >= 1, got %s %s" % (tuple(frames.shape), frames.dtype))
    if dtype not in native.DTYPE_CODES:
        raise ValueError("dtype: fp32 / bf16, got %s" % dtype)
    n, H, W = frames.shape[0] - 1, frames.shape[2], frames.shape[3]
    count = n - first if count is None else int(count)
    if first < 0 or count < 1 or first + count > n:
        raise ValueError("pairs [%d, %d) of %d" % (first, first + count, n))
    if out is None:
        out, out_first = torch.empty(count, 6, H, W, dtype=dtype, device=frames.device), 0
    else:
        native.require_device(out)
        out_first = first if out_first is None else int(out_first)
        if out.dim() != 4 or tuple(out.shape[1:]) != (6, H, W) or out.dtype != dtype or not out.is_contiguous() or \
                out_first < 0 or out_first + count > out.shape[0]:
            raise ValueError("out: contiguous %s [>=%d,6,%d,%d], got %s %s" % (dtype, out_first + count, H, W, tuple(out.shape),
                                                                              out.dtype))
    native.call("td_pose_pairs_u8", frames.contiguous(), n, H, W, int(first), count, dtype, out, out_first)
    return out


def trajectory_hip(rel, out=None):
    """trajectory_numpy as td_odom_trajectory: rel float32 / float64 [n,4,4] -> float64 [n+1,3,4]."""
    rel, f64 = _rel(rel)
    n = rel.shape[0]
    out = _out(out, (n + 1, 3, 4), torch.float64, rel.device, "out")
    native.call("td_odom_trajectory", rel, f64, n, out)
    return out


def snippet_ates_hip(rel, gt_poses, track_length=TRACK_LENGTH, out=None):
    """snippet_ates_numpy as td_odom_snippet_ate: rel [n,4,4], gt_poses float64 [n+1,3,4] -> float64 [n]."""
    rel, f64 = _rel(rel)
    n = rel.shape[0]
    gt_poses = _poses(gt_poses, "gt_poses", n + 1)
    if not 2 <= int(track_length) <= 16:
        raise ValueError("track_length: 2 ... 16, got %r" % (track_length,))
    out = _out(out, (n,), torch.float64, rel.device, "out")
    native.call("td_odom_snippet_ate", rel, f64, gt_poses, n, int(track_length), out)
    return out


def num_first_frames(m, step=STEP):
    return (int(m) + int(step) - 1) // int(step)


def sequence_errors_hip(gt_poses, pred_poses, lengths=LENGTHS, step=STEP, align_scale=True, rows=None, valid=None, summary=None):
    """sequence_errors_numpy as td_odom_sequence_errors -> (rows float64 [F,L,5], valid uint8 [F,L], summary float64 [2] = (scale,
    total distance)), F = ceil(m / step) first frames.  A segment that does not fit has valid 0 (and NaN errors), not a zero row;
    ``compact_rows`` drops those on the host."""
    gt_poses = _poses(gt_poses, "gt_poses")
    m = gt_poses.shape[0]
    pred_poses = _poses(pred_poses, "pred_poses", m)
    lengths = [float(v) for v in lengths]
    if not 1 <= len(lengths) <= MAX_LENGTHS or min(lengths) <= 0 or int(step) < 1:
        raise ValueError("lengths: 1 ... %d positive values, step >= 1" % MAX_LENGTHS)
    F, L = num_first_frames(m, step), len(lengths)
    dev = gt_poses.device
    rows = _out(rows, (F, L, 5), torch.float64, dev, "rows")
    valid = _out(valid, (F, L), torch.uint8, dev, "valid")
    summary = _out(summary, (2,), torch.float64, dev, "summary")
    dist = torch.empty(m, dtype=torch.float64, device=dev)
    native.call("td_odom_sequence_errors", gt_poses, pred_poses, m, (ctypes.c_double * L)(*lengths), L, int(step), bool(align_scale),
                dist, rows, valid, summary)
    return rows, valid, summary


def compact_rows(rows, valid):
    """Host side of sequence_errors_hip: numpy [F,L,5] + [F,L] -> the valid rows [k,5] in the toolkit's order."""
    rows, valid = np.asarray(rows, dtype=np.float64).reshape(-1, 5), np.asarray(valid).reshape(-1)
    return rows[valid != 0]


# ---------------------------------------------------------------------------------------------------------------------------

def dataset_frames_u8(dataset):
    """The n+1 frames behind a dataset of n consecutive-frame lines, each decoded once: uint8 [n+1,3,H,W] on the host."""
    n = len(dataset)
    if n < 1:
        raise ValueError("an odometry dataset needs at least one frame pair")
    if not hasattr(dataset, "frame_u8"):
        raise TypeError("dataset: needs frame_u8(index, offset) (mono.datasets.KITTIOdomDataset has it)")
    return torch.stack([dataset.frame_u8(i, 0) for i in range(n)] + [dataset.frame_u8(n - 1, 1)], 0)


class OdometryEvaluator:
    """evaluate(dataset, gt_poses) -> OdometryResult.

    model       a model of this build with ``PoseEncoder`` and ``PoseDecoder``.  fp32 runs them where they stand (their own copy
                if the model lives on another device) and restores the training mode; bf16 runs the BatchNorm-folded copy under
                autocast, as DepthEvaluator does.  The caller's model is never moved or changed.
    device      'cuda[:i]': frames are uploaded once as uint8, td_pose_pairs_u8 fills each batch, td_pose_fwd writes the relative
                transforms, the three metric kernels score them and ONE copy brings the results to the host; 'cpu': the host
                statements.
    The frames are used at the dataset's size; like the reference's eval_pose.py there is no 192 x 640 resize of the training step.
    """

    def __init__(self, model, device, batch_size=12, precision="fp32"):
        self.device = infer.check_precision(device, precision, batch_size)
        self.on_hip = self.device.type == "cuda"
        for part in ("PoseEncoder", "PoseDecoder"):
            if not hasattr(model, part):
                raise TypeError("model: no %s" % part)
        self.model = model
        self.batch_size = int(batch_size)
        self.precision = precision

    def _pose_vectors(self, net, pairs):
        if self.precision == "bf16":
            pairs = pairs.contiguous(memory_format=torch.channels_last)
        with infer.autocast_for(self.precision):
            axisangle, translation = net.PoseDecoder(net.PoseEncoder(pairs))
        return axisangle[:, 0].float(), translation[:, 0].float()

    def relative_poses(self, dataset, frames=None):
        """float32 [n,4,4] on the evaluator's device: transformation_from_parameters(axisangle[:, 0], translation[:, 0]) of every
        consecutive pair (frame i+1 -> frame i).  ``frames``: the dataset's frames as dataset_frames_u8 gives them, for a caller that
        holds them already (on either device: they are not decoded or uploaded again)."""
        frames = dataset_frames_u8(dataset) if frames is None else frames
        n = frames.shape[0] - 1
        net, restore = infer.eval_network(self.model, self.device, self.precision)
        with torch.no_grad(), restore:
            if not self.on_hip:
                pairs = pairs_torch(frames)
                out = []
                for at in range(0, n, self.batch_size):
                    axisangle, translation = self._pose_vectors(net, pairs[at:at + self.batch_size])
                    out.append(net.transformation_from_parameters(axisangle, translation, invert=False))
                return torch.cat(out, 0)
            resident = frames.to(self.device)                                  # every frame: one upload, as bytes
            rel = torch.empty(n, 4, 4, dtype=torch.float32, device=self.device)
            batch = torch.empty(min(self.batch_size, n), 6, frames.shape[2], frames.shape[3], dtype=torch.float32, device=self.device)
            no_invert = native.int_array([0])
            for at in range(0, n, self.batch_size):
                count = min(self.batch_size, n - at)
                pairs_hip(resident, torch.float32, at, count, out=batch, out_first=0)
                axisangle, translation = self._pose_vectors(net, batch[:count])
                axisangle, translation = axisangle.reshape(count, 3).contiguous(), translation.reshape(count, 3).contiguous()
                native.call("td_pose_fwd", axisangle, translation, no_invert, None, 1, count, rel[at:at + count], None)
            return rel

    def evaluate(self, dataset, gt_poses, track_length=TRACK_LENGTH, lengths=LENGTHS, step=STEP, relative=None):
        """``gt_poses``: the sequence's ground truth [n+1,3,4] (load_kitti_poses).  ``relative``: relative transforms computed
        before (relative_poses), to score them without running the network again."""
        rel = self.relative_poses(dataset) if relative is None else relative
        n = rel.shape[0]
        gt = np.ascontiguousarray(np.asarray(gt_poses, dtype=np.float64)[:, :3])
        if gt.shape != (n + 1, 3, 4):
            raise ValueError("gt_poses: [%d,3,4] for %d frame pairs, got %s" % (n + 1, n, gt.shape))
        lengths = tuple(lengths)
        if not self.on_hip:
            rel_np = rel.detach().cpu().numpy()
            poses = trajectory_numpy(rel_np)
            ates = snippet_ates_numpy(rel_np, gt, track_length)
            rows, scale, distance = sequence_errors_numpy(gt, poses, lengths, step, True)
        else:
            F, L = num_first_frames(n + 1, step), len(lengths)
            sizes = [(n + 1) * 12, n, F * L * 5, 2]                            # poses, ates, rows, summary (float64), then valid
            off = np.concatenate([[0], np.cumsum(sizes)]) * 8
            buf = torch.empty(int(off[-1]) + F * L, dtype=torch.uint8, device=self.device)
            f64 = [buf[int(a):int(b)].view(torch.float64) for a, b in zip(off[:-1], off[1:])]
            poses_d, ates_d, rows_d, summary_d = f64[0].view(n + 1, 3, 4), f64[1], f64[2].view(F, L, 5), f64[3]
            valid_d = buf[int(off[-1]):].view(F, L)
            gt_d = torch.from_numpy(gt).to(self.device)
            trajectory_hip(rel, out=poses_d)
            snippet_ates_hip(rel, gt_d, track_length, out=ates_d)
            sequence_errors_hip(gt_d, poses_d, lengths, step, True, rows=rows_d, valid=valid_d, summary=summary_d)
            host = buf.cpu().numpy()                                           # the one copy
            h64 = [host[int(a):int(b)].view(np.float64) for a, b in zip(off[:-1], off[1:])]
            poses, ates = h64[0].reshape(n + 1, 3, 4).copy(), h64[1].copy()
            rows = compact_rows(h64[2], host[int(off[-1]):])
            scale, distance = float(h64[3][0]), float(h64[3][1])
        t_err, r_err = overall_errors(rows)
        with np.errstate(invalid="ignore"):
            ate_mean, ate_std = float(np.mean(ates)), float(np.std(ates))
        return OdometryResult(ate_mean, ate_std, t_err, r_err, scale, distance, poses, ates, rows, rel)
