"""A fused cloud aligned to the lidar before it is scored: a similarity transform x' = c R x + t that maps the predicted cloud into the
reference's frame, estimated by iterated closest points (nearest neighbour, closed-form solve, repeat).  cloud_eval scores two clouds
only if they already share a frame and a scale; a cloud fused with a self-supervised model's own poses has neither.  The closed form
is Umeyama's (IEEE PAMI 1991), which the reference ships as ``umeyama_alignment`` (mono/tools/geometry.py): the solve has a parity gate.

Layers, as in cloud_eval.py:
  * host statements in numpy (``transform_numpy``, ``moments_numpy``): the host path (``device='cpu'``) and what the kernels are tested
    against, written in the kernels' operation order; ``align_numpy`` is the whole loop on them;
  * ``transform_hip``, ``moments_hip`` (csrc/td_align.hip): device tensors only, a CPU tensor is an error;
  * ``solve_from_moments`` and ``similarity_from_poses``: the closed form, on the HOST for both paths (numpy's SVD of a 3x3);
  * ``CloudAligner``: two clouds -> Alignment.

Transform (float64; every product and sum rounded on its own):
    out_k = c ((R_k0 x + R_k1 y) + R_k2 z) + t_k
Moments.  A row i is matched iff 0 <= index_i < M and d2_i <= trim2 (a NaN fails); index and d2 are the nearest-neighbour query's.
With p = cur_i - origin and q = ref[index_i] - origin a matched row contributes the 17 values
    p (3),  q (3),  q_r p_c (9, row-major),  (p_x p_x + p_y p_y) + p_z p_z,  d2_i
and any other row +0.0 in every slot; an index >= M or < -1 reads nothing and is counted (bad_index).  The order of the sums is fixed
and a function of N alone.  Stage 1: rows 256 b ... 256 b + 255 (rows past N are +0.0) are reduced by the halving tree, for s = 128,
64, ..., 1: row j += row j + s for j < s; row 0 is partial b.  Stage 2: "thread" j of 256 adds partials j, j + 256, ... one after the
other onto +0.0, and the same tree over the 256 threads follows.  Both paths therefore feed the host solve the same bits, and the
transform, the history and the iteration count of an alignment are IDENTICAL between 'cpu' and the device.

Why about an origin: the covariance is sum(q p^T) / n - mean_q mean_p^T, a difference of two numbers of the size |x|^2 whose result is
of the size of the cloud's extent squared; taken about the centre of the reference's bounding box the two are of one size.
Solve:  mean_p = m[0:3] / n, mean_q = m[3:6] / n, cov = m[6:15] / n - outer(mean_q, mean_p), sigma = m[15] / n - mean_p . mean_p;
u, d, v = svd(cov), S = diag(1, 1, -1) when det(u) det(v) < 0, R = u S v, c = trace(diag(d) S) / sigma (or 1), t = mean_q - c R mean_p.
Compose (o: the origin):  c <- dc c,  R <- dR R,  t <- dc dR (t - o) + dt + o.

Limits: point-to-point only, one direction (predicted into reference), no outlier model beyond ``trim``, a planar scene leaves the
in-plane motion unconstrained; every default is UNTUNED and no real cloud has been aligned.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import cloud_eval, native

SLOTS = 17                            # csrc/td_align.hip: TD_ICP_SLOTS
BLOCK = 256                           # rows per workgroup of stage 1, threads of stage 2
MODES = ("similarity", "rigid")

Alignment = collections.namedtuple("Alignment", "scale R t iterations converged history")
Alignment.__doc__ = """x' = scale R x + t maps the predicted cloud into the reference's frame: scale a Python float, R float64 [3,3], t float64
[3] (numpy, on the host);  iterations: the passes that ran (len(history));  converged: the last step was the identity within ``tol``;
history: one (matched, rms) per pass, the number of matched rows and sqrt(sum d2 / matched) over them BEFORE that pass's step (0.0
when nothing matched)."""


def _rt(R, t):
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float64)).reshape(-1)
    t = np.ascontiguousarray(np.asarray(t, dtype=np.float64)).reshape(-1)
    if R.shape != (9,) or t.shape != (3,):
        raise ValueError("R: 3x3, t: 3; got %s, %s" % (R.shape, t.shape))
    return R, t


def matrix(c, R, t):
    """-> the 4x4 [[c R, t], [0, 1]]."""
    T = np.eye(4)
    T[:3, :3] = float(c) * np.asarray(R, np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(t, np.float64).reshape(3)
    return T


# ---------------------------------------------------------------------------------------------------------------------------
# host statements

def transform_numpy(src, c, R, t):
    """src float64 [N,3] -> float64 [N,3]: out_k = c ((R_k0 x + R_k1 y) + R_k2 z) + t_k, column by column in td_cloud_transform's
    order (no matrix product: its order of sums is the BLAS's)."""
    s = cloud_eval._xyz64(src, "src")
    R, t = _rt(R, t)
    c = np.float64(c)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty_like(s)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            out[:, k] = c * ((R[3 * k] * x + R[3 * k + 1] * y) + R[3 * k + 2] * z) + t[k]
    return out


def _tree(a):
    """float64 [L,256,17] -> [L,17]: for s = 128 ... 1: row j += row j + s for j < s.  In place."""
    s = BLOCK // 2
    while s:
        a[:, :s] += a[:, s:2 * s]
        s >>= 1
    return a[:, 0]


def _padded(rows, multiple):
    """[n,17] -> [ceil(n / multiple), multiple, 17], the rows past n +0.0."""
    n = len(rows)
    groups = -(-n // multiple)
    out = np.zeros((groups * multiple, SLOTS))
    out[:n] = rows
    return out.reshape(groups, multiple, SLOTS)


def moments_numpy(cur, ref, index, d2, trim2, origin):
    """cur float64 [N,3], ref float64 [M,3] in ORIGINAL order, index int64 [N], d2 float64 [N] (nearest_numpy's) -> (m float64 [17],
    matched, bad_index).  The statement td_icp_moments is tested against: the same rows, the same two-stage tree."""
    cur, ref = cloud_eval._xyz64(cur, "cur"), cloud_eval._xyz64(ref, "ref")
    index = np.ascontiguousarray(index, dtype=np.int64)
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64)).reshape(-1)
    N, M = len(cur), len(ref)
    if index.shape != (N,) or d2.shape != (N,) or o.shape != (3,) or not np.isfinite(o).all() or not float(trim2) >= 0:
        raise ValueError("index [N], d2 [N], a finite origin [3], trim2 >= 0; got %s, %s, %r, %r" % (index.shape, d2.shape, origin, trim2))
    bad = (index >= M) | (index < -1)
    with np.errstate(invalid="ignore", over="ignore"):
        who = np.nonzero((index >= 0) & (index < M) & (d2 <= np.float64(trim2)))[0]          # a NaN fails
        rows = np.zeros((N, SLOTS))
        p, q = cur[who] - o, ref[index[who]] - o
        rows[who, 0:3], rows[who, 3:6] = p, q
        for r in range(3):
            for c in range(3):
                rows[who, 6 + 3 * r + c] = q[:, r] * p[:, c]
        rows[who, 15] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        rows[who, 16] = d2[who]
        partials = _tree(_padded(rows, BLOCK))                  # stage 1: [ceil(N / 256), 17]
        acc = np.zeros((BLOCK, SLOTS))
        for chunk in _padded(partials, BLOCK):                  # stage 2: thread j adds partials j, j + 256, ... in that order
            acc = acc + chunk                                   # (a thread that has run out adds +0.0, which changes no bit)
        m = _tree(acc[None])[0].copy()
    return m, int(len(who)), int(np.count_nonzero(bad))


def _umeyama(mean_p, mean_q, cov, sigma, with_scale):
    """The tail of Umeyama's closed form -> (c, R, t), or None when it is degenerate."""
    if not (np.isfinite(cov).all() and np.isfinite(mean_p).all() and np.isfinite(mean_q).all() and np.isfinite(sigma) and sigma > 0):
        return None
    u, d, v = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(u) * np.linalg.det(v) < 0.0:
        S[2, 2] = -1.0
    R = u.dot(S).dot(v)
    c = float(np.trace(np.diag(d).dot(S)) / sigma) if with_scale else 1.0
    t = mean_q - c * R.dot(mean_p)
    if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(c) and c > 0):
        return None
    return c, R, t


def solve_from_moments(n, m, with_scale=True):
    """n matched rows and their 17 sums -> (c, R, t) with q ~ c R p + t in the least-squares sense (Umeyama), about the moments'
    origin; None when the solve is degenerate: n < 3, a variance that is not positive, anything not finite.  Host, numpy."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    n = int(n)
    if m.shape != (SLOTS,):
        raise ValueError("m: the 17 sums, got %s" % (m.shape,))
    if n < 3 or not np.isfinite(m).all():
        return None
    mean_p, mean_q = m[0:3] / n, m[3:6] / n
    cov = m[6:15].reshape(3, 3) / n - np.outer(mean_q, mean_p)
    sigma = m[15] / n - mean_p.dot(mean_p)
    return _umeyama(mean_p, mean_q, cov, sigma, with_scale)


def _centres(poses, name):
    P = np.asarray(poses.cpu() if torch.is_tensor(poses) else poses, dtype=np.float64)
    if P.ndim != 3 or P.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("%s: [m,3,4] or [m,4,4] camera-to-world, got %s" % (name, P.shape))
    return np.ascontiguousarray(P[:, :3, 3])


def similarity_from_poses(pred_poses, gt_poses, with_scale=True):
    """The closed form on the camera centres of two trajectories -> (c, R, t) with gt_centre ~ c R pred_centre + t, written centred
    like the reference's umeyama_alignment.  The initial guess for a cloud fused with the model's own poses: ICP cannot start from
    the identity when the scale is off by 36.  ValueError when the trajectories do not determine it."""
    x, y = _centres(pred_poses, "pred_poses"), _centres(gt_poses, "gt_poses")
    if x.shape != y.shape or len(x) < 3:
        raise ValueError("two trajectories of one length, at least 3 poses; got %s, %s" % (x.shape, y.shape))
    n = len(x)
    mean_x, mean_y = x.mean(0), y.mean(0)
    xc, yc = x - mean_x, y - mean_y
    sigma = float((xc * xc).sum() / n)
    cov = yc.T.dot(xc) / n
    out = _umeyama(mean_x, mean_y, cov, sigma, with_scale)
    if out is None:
        raise ValueError("the camera centres do not determine a similarity transform (all in one point, or not finite)")
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def transform_hip(src, c, R, t, out=None):
    """transform_numpy as one launch of td_cloud_transform -> float64 [N,3] on src's device.  ``out``: a float64 [N,3] device tensor
    to write into (src itself is allowed), or None for a fresh one.  No synchronisation."""
    s = cloud_eval._f64_points(src, "src")
    R, t = _rt(R, t)
    out = torch.empty_like(s) if out is None else cloud_eval._f64_points(out, "out")
    if out.shape != s.shape or not out.is_contiguous():
        raise ValueError("out: contiguous float64 %s, got %s" % (tuple(s.shape), tuple(out.shape)))
    if s.shape[0] == 0:                  # an empty tensor has no pointer to pass
        return out
    native.call("td_cloud_transform", s, s.shape[0], float(c), (ctypes.c_double * 9)(*R), (ctypes.c_double * 3)(*t), out)
    return out


def moments_hip(cur, ref, index, d2, trim2, origin, out=None):
    """moments_numpy as td_icp_moments -> a float64 [19] device tensor: the 17 sums, then matched and bad_index as the bits of two
    int64 (``moments_to_host`` reads it).  ``out``: such a tensor to overwrite, or None for a fresh one.  No synchronisation."""
    cur, ref = cloud_eval._f64_points(cur, "cur"), cloud_eval._f64_points(ref, "ref")
    N, M = cur.shape[0], ref.shape[0]
    native.require_device(index, d2)
    if index.dtype != torch.int64 or tuple(index.shape) != (N,) or d2.dtype != torch.float64 or tuple(d2.shape) != (N,):
        raise ValueError("index int64 [%d], d2 float64 [%d]; got %s %s, %s %s" % (N, N, tuple(index.shape), index.dtype, tuple(d2.shape), d2.dtype))
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64)).reshape(-1)
    if o.shape != (3,):
        raise ValueError("origin: 3 numbers, got %s" % (o.shape,))
    need = native.load().td_icp_moments_workspace(N)
    workspace = torch.empty(need // 8, dtype=torch.float64, device=cur.device) if N else None
    if out is None:
        out = torch.empty(SLOTS + 2, dtype=torch.float64, device=cur.device)
    native.require_device(out)
    if out.dtype != torch.float64 or tuple(out.shape) != (SLOTS + 2,) or not out.is_contiguous():
        raise ValueError("out: contiguous float64 [%d], got %s %s" % (SLOTS + 2, tuple(out.shape), out.dtype))
    native.call("td_icp_moments", cur if N else None, N, ref if M else None, M, index.contiguous() if N else None,
                d2.contiguous() if N else None, float(trim2), (ctypes.c_double * 3)(*o), workspace, need, out)
    return out


def moments_to_host(out):
    """moments_hip's tensor -> (m float64 [17], matched, bad_index): ONE copy of 19 numbers, which synchronises."""
    host = out.cpu().numpy()
    counters = host[SLOTS:].view(np.int64)
    return host[:SLOTS].copy(), int(counters[0]), int(counters[1])


# ---------------------------------------------------------------------------------------------------------------------------

def _bbox_origin(lo, hi):
    return 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64))


class CloudAligner:
    """align(pred_xyz, ref_xyz, init=(1.0, I, 0)) -> Alignment: iterated closest points from the predicted cloud into the reference.

    device      'cuda[:i]': cloud_eval.grid_hip once, then per pass transform_hip, cloud_eval.nearest_hip, moments_hip and ONE copy of
                19 numbers to the host, where the step is solved and composed; the clouds may be numpy arrays or tensors anywhere.
                'cpu': the same loop on transform_numpy, nearest_numpy and moments_numpy.  The host solve is fed the same bits on
                both, so the two paths return identical Alignments.
    tau         the radius of the correspondence search, in the reference's units; UNTUNED
    mode        'similarity' (scale, rotation, translation) or 'rigid' (the scale stays the initial guess's)
    iters       at most this many passes;  tol: a pass whose step has |dc - 1|, max |dR - I| and max |dt| / tau all <= tol ends the
                loop with converged = True
    trim        correspondences farther apart than this are left out (default: tau, nothing is left out);  stride: every stride-th
                predicted point is used
    A pass whose solve is degenerate (fewer than 3 matched rows, no variance, something not finite) ends the loop with the last good
    transform and converged = False.  The origin of the moments is the centre of the bounding box of the reference's finite points."""

    def __init__(self, device, tau, mode="similarity", iters=30, trim=None, stride=1, tol=1e-9):
        self.device = torch.device(device)
        self.on_hip = self.device.type == "cuda"
        self.tau = float(tau)
        cloud_eval.inv_cell(self.tau)
        if mode not in MODES:
            raise ValueError("mode: one of %r, got %r" % (MODES, mode))
        self.mode, self.iters, self.stride, self.tol = mode, int(iters), int(stride), float(tol)
        self.trim = self.tau if trim is None else float(trim)
        if self.iters < 0 or self.stride < 1 or not self.trim >= 0 or not self.tol >= 0:
            raise ValueError("iters >= 0, stride >= 1, trim >= 0, tol >= 0; got %r, %r, %r, %r" % (iters, stride, trim, tol))

    def _setup(self, pred_xyz, ref_xyz):
        """-> (queries, ref, grid, origin) on the path's side."""
        if not self.on_hip:
            pred, ref = cloud_eval._xyz64(pred_xyz, "pred_xyz"), cloud_eval._xyz64(ref_xyz, "ref_xyz")
            finite = ref[np.isfinite(ref).all(1)]
            origin = _bbox_origin(finite.min(0), finite.max(0)) if len(finite) else np.zeros(3)
            return np.ascontiguousarray(pred[::self.stride]), ref, cloud_eval.grid_numpy(ref, self.tau), origin
        pred = torch.as_tensor(pred_xyz).to(self.device, torch.float64)
        ref = torch.as_tensor(ref_xyz).to(self.device, torch.float64).contiguous()
        if pred.dim() != 2 or pred.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != 3:
            raise ValueError("pred_xyz [n,3], ref_xyz [m,3]; got %s, %s" % (tuple(pred.shape), tuple(ref.shape)))
        finite = ref[torch.isfinite(ref).all(1)]
        origin = np.zeros(3)
        if finite.shape[0]:              # min and max are exact: both paths get the same origin
            box = torch.stack([finite.min(0).values, finite.max(0).values]).cpu().numpy()
            origin = _bbox_origin(box[0], box[1])
        return pred[::self.stride].contiguous(), ref, cloud_eval.grid_hip(ref, self.tau), origin

    def _pass(self, queries, ref, grid, origin, c, R, t, trim2):
        """One transform, query and reduction -> (m [17], matched, bad_index) on the host."""
        if not self.on_hip:
            cur = transform_numpy(queries, c, R, t)
            nb = cloud_eval.nearest_numpy(cur, grid, self.tau, ())
            return moments_numpy(cur, ref, nb.index, nb.d2, trim2, origin)
        cur = transform_hip(queries, c, R, t)
        nb = cloud_eval.nearest_hip(cur, grid, self.tau, ())
        return moments_to_host(moments_hip(cur, ref, nb.index, nb.d2, trim2, origin))

    def align(self, pred_xyz, ref_xyz, init=None):
        c, R, t = (1.0, np.eye(3), np.zeros(3)) if init is None else init
        c, R, t = float(c), np.array(R, dtype=np.float64).reshape(3, 3), np.array(t, dtype=np.float64).reshape(3)
        if not (np.isfinite(c) and c > 0 and np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError("init: a positive scale, a finite rotation and translation; got %r" % (init,))
        queries, ref, grid, origin = self._setup(pred_xyz, ref_xyz)
        trim2 = self.trim * self.trim
        history, converged, eye = [], False, np.eye(3)
        for _ in range(self.iters):
            m, matched, _ = self._pass(queries, ref, grid, origin, c, R, t, trim2)
            history.append((matched, math.sqrt(m[16] / matched) if matched else 0.0))
            step = solve_from_moments(matched, m, self.mode == "similarity")
            if step is None:
                break
            dc, dR, dt = step
            c, R, t = dc * c, dR.dot(R), dc * dR.dot(t - origin) + dt + origin
            if abs(dc - 1.0) <= self.tol and np.abs(dR - eye).max() <= self.tol and np.abs(dt).max() / self.tau <= self.tol:
                converged = True
                break
        return Alignment(c, R, t, len(history), converged, tuple(history))


def align_numpy(pred_xyz, ref_xyz, tau, mode="similarity", iters=30, trim=None, stride=1, tol=1e-9, init=None):
    """The statement of CloudAligner.align: the loop on the numpy statements -> Alignment."""
    return CloudAligner("cpu", tau, mode, iters, trim, stride, tol).align(pred_xyz, ref_xyz, init)
