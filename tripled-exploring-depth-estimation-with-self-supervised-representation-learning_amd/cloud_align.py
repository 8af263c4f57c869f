"""A fused cloud aligned to the lidar before it is scored: a similarity transform x' = c R x + t that maps the predicted cloud into the
reference's frame, estimated by iterated closest points (nearest neighbour, closed-form solve, repeat).  cloud_eval scores two clouds
only if they already share a frame and a scale; a cloud fused with a self-supervised model's own poses has neither.  The closed form
is Umeyama's (IEEE PAMI 1991), which the reference ships as ``umeyama_alignment`` (mono/tools/geometry.py): the solve has a parity gate.

Layers, as in cloud_eval.py:
  * host statements in numpy (``transform_numpy``, ``moments_numpy``, ``plane_moments_numpy``): the host path (``device='cpu'``) and
    what the kernels are tested against, written in the kernels' operation order; ``align_numpy`` is the whole loop on them;
  * ``transform_hip``, ``moments_hip``, ``plane_moments_hip`` (csrc/td_align.hip): device tensors only, a CPU tensor is an error;
  * ``solve_from_moments`` and ``similarity_from_poses``: the closed form, on the HOST for both paths (numpy's SVD of a 3x3);
    ``solve_plane_step``: the point-to-plane step, on the host likewise (numpy's eigh of a 7x7);
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

Point to plane (criterion="plane", Chen and Medioni).  Point to point registers one sampling lattice on the other; two clouds that
sample the same surfaces differently are registered by the distance ALONG THE REFERENCE'S NORMAL instead.  The normals are
cloud_normals' (once per alignment, of the reference against its own grid).  A row is matched iff 0 <= index_i < M, d2_i <= trim2 and
normals[index_i] is not all zero; a row that passes the first two and whose neighbour has no normal is counted (no_normal).  With p =
cur_i - origin, q = ref[j] - origin, n = normals[j], g = p - q:
    a = (p_y n_z - p_z n_y,  p_z n_x - p_x n_z,  p_x n_y - p_y n_x,  n_x,  n_y,  n_z,  (p_x n_x + p_y n_y) + p_z n_z)
    r = (n_x g_x + n_y g_y) + n_z g_z
which is the residual n . (x' - q) of the linearised step x' = p + w x p + sigma p + tau in the unknowns (w, tau, sigma): r + a . x.
A matched row contributes the 37 values  a_i a_j for i <= j, row-major (28),  a_i r (7),  r r,  d2_i;  any other row +0.0.  The sums run
through the same two-stage tree as the 17 (``plane_moments_numpy``, td_icp_plane_moments); three counters follow: matched, bad_index,
no_normal.  ``solve_plane_step`` on the HOST: the symmetric 7x7 A = sum a a^T (the leading 6x6 for 'rigid') and b = sum a r, rows and
columns of rotation and scale divided by ``length`` (the largest half-extent of the reference's bounding box: without it the
eigenvalues mix units), numpy.linalg.eigh, the eigenvalues > rcond largest kept, the minimum-norm solution of A x = -b over them,
unscaled; dR by Rodrigues' formula from w, dc = exp(sigma), dt = tau; composed like a point-to-point step.  A direction the scene does
not constrain (the translation along a corridor) is DROPPED and reported, not solved for: the step has no component along it.

Limits: one direction (predicted into reference), no outlier model beyond ``trim``, no robust kernel; point to point leaves a planar
scene's in-plane motion unconstrained and ends a sampling lattice away from the truth, point to plane needs normals (a reference too
sparse or too rough for them matches nothing) and a start inside the linearisation's reach; every default (max_curvature = 0.01 and
rcond = 1e-3 among them, taken from a float64 prototype on the synthetic street) is UNTUNED and no real cloud has been aligned.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import cloud_eval, cloud_normals, native

SLOTS = native.CONSTANTS["TD_ICP_SLOTS"]
BLOCK = 256                           # rows per workgroup of stage 1, threads of stage 2
MODES = ("similarity", "rigid")
PLANE_SLOTS = native.CONSTANTS["TD_ICP_PLANE_SLOTS"]
CRITERIA = ("point", "plane")

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
    """float64 [L,256,S] -> [L,S]: for s = 128 ... 1: row j += row j + s for j < s.  In place."""
    s = BLOCK // 2
    while s:
        a[:, :s] += a[:, s:2 * s]
        s >>= 1
    return a[:, 0]


def _padded(rows, multiple):
    """[n,S] -> [ceil(n / multiple), multiple, S], the rows past n +0.0."""
    n, slots = rows.shape
    groups = -(-n // multiple)
    out = np.zeros((groups * multiple, slots))
    out[:n] = rows
    return out.reshape(groups, multiple, slots)


def _two_stage(rows):
    """[N,S] -> [S]: the two-stage tree of the module docstring."""
    partials = _tree(_padded(rows, BLOCK))                      # stage 1: [ceil(N / 256), S]
    acc = np.zeros((BLOCK, rows.shape[1]))
    for chunk in _padded(partials, BLOCK):                      # stage 2: thread j adds partials j, j + 256, ... in that order
        acc = acc + chunk                                       # (a thread that has run out adds +0.0, which changes no bit)
    return _tree(acc[None])[0].copy()


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
        m = _two_stage(rows)
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


def plane_moments_numpy(cur, ref, normals, index, d2, trim2, origin):
    """cur float64 [N,3], ref and normals float64 [M,3] in ORIGINAL order, index int64 [N], d2 float64 [N] -> (m float64 [37], matched,
    bad_index, no_normal).  The statement td_icp_plane_moments is tested against: the same rows, the same two-stage tree."""
    cur, ref, normals = cloud_eval._xyz64(cur, "cur"), cloud_eval._xyz64(ref, "ref"), cloud_eval._xyz64(normals, "normals")
    index = np.ascontiguousarray(index, dtype=np.int64)
    d2 = np.ascontiguousarray(d2, dtype=np.float64)
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64)).reshape(-1)
    N, M = len(cur), len(ref)
    if index.shape != (N,) or d2.shape != (N,) or o.shape != (3,) or not np.isfinite(o).all() or not float(trim2) >= 0 or normals.shape != ref.shape:
        raise ValueError("index [N], d2 [N], normals like ref, a finite origin [3], trim2 >= 0; got %s, %s, %s, %r, %r" % (
            index.shape, d2.shape, normals.shape, origin, trim2))
    bad = (index >= M) | (index < -1)
    with np.errstate(invalid="ignore", over="ignore"):
        near = np.nonzero((index >= 0) & (index < M) & (d2 <= np.float64(trim2)))[0]          # a NaN fails
        flat = (normals[index[near]] == 0.0).all(1)
        who = near[~flat]
        rows = np.zeros((N, PLANE_SLOTS))
        p, q, n = cur[who] - o, ref[index[who]] - o, normals[index[who]]
        g = p - q
        a = [p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1], p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2], (p[:, 0] * n[:, 0] + p[:, 1] * n[:, 1]) + p[:, 2] * n[:, 2]]
        r = (n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]
        at = 0
        for i in range(7):
            for j in range(i, 7):
                rows[who, at] = a[i] * a[j]
                at += 1
        for i in range(7):
            rows[who, 28 + i] = a[i] * r
        rows[who, 35] = r * r
        rows[who, 36] = d2[who]
        m = _two_stage(rows)
    return m, int(len(who)), int(np.count_nonzero(bad)), int(np.count_nonzero(flat))


def _rodrigues(w):
    """The rotation exp([w]_x), float64."""
    w = np.asarray(w, np.float64)
    angle = float(np.sqrt(w.dot(w)))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if angle < 1e-8:                       # sin(x) / x and (1 - cos(x)) / x^2 to their first terms: the error is below 1e-17
        return np.eye(3) + K + 0.5 * K.dot(K)
    return np.eye(3) + (math.sin(angle) / angle) * K + ((1.0 - math.cos(angle)) / (angle * angle)) * K.dot(K)


def solve_plane_step(n, m, with_scale=True, length=1.0, rcond=1e-3):
    """n matched rows and their 37 sums -> (dc, dR, dt, rank, dropped_direction), the point-to-plane step about the moments' origin
    (module docstring), or None when there is none: n < 6, anything not finite, rank 0.  ``length`` scales the rotation and scale
    unknowns to the translation's units; ``rcond``: eigenvalues <= rcond largest are dropped.  rank: the eigenvalues kept (at most 7,
    6 without scale);  dropped_direction: None at full rank, else float64 [dropped, 7 or 6], the unit eigenvectors that were dropped,
    in the scaled unknowns (w length, tau, sigma length): the square of an entry is the direction's weight on that unknown.  Host."""
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    n, length, rcond = int(n), float(length), float(rcond)
    if m.shape != (PLANE_SLOTS,):
        raise ValueError("m: the 37 sums, got %s" % (m.shape,))
    if not (np.isfinite(length) and length > 0 and 0 <= rcond < 1):
        raise ValueError("length > 0 and 0 <= rcond < 1; got %r, %r" % (length, rcond))
    if n < 6 or not np.isfinite(m).all():
        return None
    A = np.zeros((7, 7))
    A[np.triu_indices(7)] = m[:28]
    A = A + np.triu(A, 1).T
    b = m[28:35].copy()
    dim = 7 if with_scale else 6
    D = np.array([1.0 / length] * 3 + [1.0] * 3 + [1.0 / length])[:dim]
    A, b = A[:dim, :dim] * D[:, None] * D[None, :], b[:dim] * D
    lam, vec = np.linalg.eigh(A)
    if not (np.isfinite(lam).all() and np.isfinite(vec).all()) or not lam[-1] > 0:
        return None
    keep = lam > rcond * lam[-1]
    rank = int(np.count_nonzero(keep))
    if rank == 0:
        return None
    y = -(vec[:, keep] * (vec[:, keep].T.dot(b) / lam[keep])).sum(1)
    x = y * D
    dR, dt = _rodrigues(x[0:3]), x[3:6].copy()
    dc = math.exp(x[6]) if with_scale else 1.0
    if not (np.isfinite(dR).all() and np.isfinite(dt).all() and np.isfinite(dc) and dc > 0):
        return None
    return dc, dR, dt, rank, (None if rank == dim else np.ascontiguousarray(vec[:, ~keep].T))


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


def plane_moments_hip(cur, ref, normals, index, d2, trim2, origin, out=None):
    """plane_moments_numpy as td_icp_plane_moments -> a float64 [40] device tensor: the 37 sums, then matched, bad_index and no_normal
    as the bits of three int64 (``plane_moments_to_host`` reads it).  ``out``: such a tensor to overwrite, or None.  No synchronisation."""
    cur, ref, normals = cloud_eval._f64_points(cur, "cur"), cloud_eval._f64_points(ref, "ref"), cloud_eval._f64_points(normals, "normals")
    N, M = cur.shape[0], ref.shape[0]
    native.require_device(index, d2)
    if index.dtype != torch.int64 or tuple(index.shape) != (N,) or d2.dtype != torch.float64 or tuple(d2.shape) != (N,) or normals.shape != ref.shape:
        raise ValueError("index int64 [%d], d2 float64 [%d], normals float64 [%d,3]; got %s %s, %s %s, %s" % (
            N, N, M, tuple(index.shape), index.dtype, tuple(d2.shape), d2.dtype, tuple(normals.shape)))
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64)).reshape(-1)
    if o.shape != (3,):
        raise ValueError("origin: 3 numbers, got %s" % (o.shape,))
    need = native.load().td_icp_plane_moments_workspace(N)
    workspace = torch.empty(need // 8, dtype=torch.float64, device=cur.device) if N else None
    if out is None:
        out = torch.empty(PLANE_SLOTS + 3, dtype=torch.float64, device=cur.device)
    native.require_device(out)
    if out.dtype != torch.float64 or tuple(out.shape) != (PLANE_SLOTS + 3,) or not out.is_contiguous():
        raise ValueError("out: contiguous float64 [%d], got %s %s" % (PLANE_SLOTS + 3, tuple(out.shape), out.dtype))
    native.call("td_icp_plane_moments", cur if N else None, N, ref if M else None, normals if M else None, M, index.contiguous() if N else None,
                d2.contiguous() if N else None, float(trim2), (ctypes.c_double * 3)(*o), workspace, need, out)
    return out


def plane_moments_to_host(out):
    """plane_moments_hip's tensor -> (m float64 [37], matched, bad_index, no_normal): ONE copy of 40 numbers, which synchronises."""
    host = out.cpu().numpy()
    counters = host[PLANE_SLOTS:].view(np.int64)
    return host[:PLANE_SLOTS].copy(), int(counters[0]), int(counters[1]), int(counters[2])


# ---------------------------------------------------------------------------------------------------------------------------

def _bbox_origin(lo, hi):
    return 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64))


def _bbox_length(lo, hi):
    """The largest half-extent, exact on both paths like the origin; 1.0 for a box with none."""
    half = float((0.5 * (np.asarray(hi, np.float64) - np.asarray(lo, np.float64))).max())
    return half if np.isfinite(half) and half > 0 else 1.0


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
    criterion   'point' (the default: Umeyama's closed form on the pairs) or 'plane' (the distance along the reference's normal,
                module docstring): the reference's normals are computed ONCE per alignment (cloud_normals, radius ``normal_radius``,
                default tau, with ``min_neighbours`` and ``max_curvature``), per pass plane_moments_hip / _numpy and ONE copy of 40
                numbers, the step is solve_plane_step with ``rcond`` and the largest half-extent of the reference's bounding box as
                its length.  All five are keyword-only; the last four are read, and checked, by 'plane' alone and are UNTUNED.
    A pass whose solve is degenerate (fewer than 3 matched rows, no variance, something not finite; for 'plane' fewer than 6 or rank 0)
    ends the loop with the last good transform and converged = False.  The origin of the moments is the centre of the bounding box of
    the reference's finite points.
    After align():  ``history`` of the Alignment is (matched, rms of the POINT distances) per pass for both criteria;  with 'plane',
    ``plane_history`` holds one (plane_rms, rank, dropped_direction) per pass (sqrt(sum r r / matched), solve_plane_step's rank and
    dropped directions; rank 0 and None where the solve was degenerate) and ``normal_stats`` the reference's normal counters (a dict
    under cloud_normals.CAUSES); with 'point' they are () and None."""

    def __init__(self, device, tau, mode="similarity", iters=30, trim=None, stride=1, tol=1e-9, *, criterion="point", normal_radius=None,
                 min_neighbours=6, max_curvature=0.01, rcond=1e-3):
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
        if criterion not in CRITERIA:
            raise ValueError("criterion: one of %r, got %r" % (CRITERIA, criterion))
        self.criterion, self.rcond = criterion, float(rcond)
        self.normals = None                   # 'point' neither reads nor checks the last four arguments
        if criterion == "plane":
            if not 0 <= self.rcond < 1:
                raise ValueError("rcond: inside [0, 1), got %r" % (rcond,))
            self.normals = cloud_normals.CloudNormals(self.device, self.tau, normal_radius, min_neighbours, max_curvature)      # checks its own
        self.plane_history, self.normal_stats = (), None

    def _setup(self, pred_xyz, ref_xyz):
        """-> (queries, ref, grid, origin, length, normals) on the path's side; normals: None for 'point'."""
        plane = self.criterion == "plane"
        if not self.on_hip:
            pred, ref = cloud_eval._xyz64(pred_xyz, "pred_xyz"), cloud_eval._xyz64(ref_xyz, "ref_xyz")
            finite = ref[np.isfinite(ref).all(1)]
            box = (finite.min(0), finite.max(0)) if len(finite) else (np.zeros(3), np.zeros(3))
            grid = cloud_eval.grid_numpy(ref, self.tau)
            normals = self.normals.estimate(ref, grid) if plane else None
            return np.ascontiguousarray(pred[::self.stride]), ref, grid, _bbox_origin(*box), _bbox_length(*box), normals
        pred = torch.as_tensor(pred_xyz).to(self.device, torch.float64)
        ref = torch.as_tensor(ref_xyz).to(self.device, torch.float64).contiguous()
        if pred.dim() != 2 or pred.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != 3:
            raise ValueError("pred_xyz [n,3], ref_xyz [m,3]; got %s, %s" % (tuple(pred.shape), tuple(ref.shape)))
        finite = ref[torch.isfinite(ref).all(1)]
        box = np.zeros((2, 3))
        if finite.shape[0]:              # min and max are exact: both paths get the same origin
            box = torch.stack([finite.min(0).values, finite.max(0).values]).cpu().numpy()
        grid = cloud_eval.grid_hip(ref, self.tau)
        normals = self.normals.estimate(ref, grid) if plane else None
        return pred[::self.stride].contiguous(), ref, grid, _bbox_origin(box[0], box[1]), _bbox_length(box[0], box[1]), normals

    def _pass(self, queries, ref, grid, origin, c, R, t, trim2, normals=None):
        """One transform, query and reduction -> (m [17], matched, bad_index) on the host; with normals (m [37], matched, bad_index,
        no_normal)."""
        if not self.on_hip:
            cur = transform_numpy(queries, c, R, t)
            nb = cloud_eval.nearest_numpy(cur, grid, self.tau, ())
            if normals is not None:
                return plane_moments_numpy(cur, ref, normals, nb.index, nb.d2, trim2, origin)
            return moments_numpy(cur, ref, nb.index, nb.d2, trim2, origin)
        cur = transform_hip(queries, c, R, t)
        nb = cloud_eval.nearest_hip(cur, grid, self.tau, ())
        if normals is not None:
            return plane_moments_to_host(plane_moments_hip(cur, ref, normals, nb.index, nb.d2, trim2, origin))
        return moments_to_host(moments_hip(cur, ref, nb.index, nb.d2, trim2, origin))

    def align(self, pred_xyz, ref_xyz, init=None):
        c, R, t = (1.0, np.eye(3), np.zeros(3)) if init is None else init
        c, R, t = float(c), np.array(R, dtype=np.float64).reshape(3, 3), np.array(t, dtype=np.float64).reshape(3)
        if not (np.isfinite(c) and c > 0 and np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError("init: a positive scale, a finite rotation and translation; got %r" % (init,))
        queries, ref, grid, origin, length, normals = self._setup(pred_xyz, ref_xyz)
        plane = normals is not None
        self.plane_history, self.normal_stats = (), (normals.stats if plane else None)
        trim2 = self.trim * self.trim
        history, planes, converged, eye = [], [], False, np.eye(3)
        for _ in range(self.iters):
            if plane:
                m, matched, _, _ = self._pass(queries, ref, grid, origin, c, R, t, trim2, normals.normal)
                history.append((matched, math.sqrt(m[36] / matched) if matched else 0.0))
                step = solve_plane_step(matched, m, self.mode == "similarity", length, self.rcond)
                planes.append((math.sqrt(m[35] / matched) if matched else 0.0,) + ((0, None) if step is None else step[3:]))
                self.plane_history = tuple(planes)
            else:
                m, matched, _ = self._pass(queries, ref, grid, origin, c, R, t, trim2)
                history.append((matched, math.sqrt(m[16] / matched) if matched else 0.0))
                step = solve_from_moments(matched, m, self.mode == "similarity")
            if step is None:
                break
            dc, dR, dt = step[:3]
            c, R, t = dc * c, dR.dot(R), dc * dR.dot(t - origin) + dt + origin
            if abs(dc - 1.0) <= self.tol and np.abs(dR - eye).max() <= self.tol and np.abs(dt).max() / self.tau <= self.tol:
                converged = True
                break
        return Alignment(c, R, t, len(history), converged, tuple(history))


def align_numpy(pred_xyz, ref_xyz, tau, mode="similarity", iters=30, trim=None, stride=1, tol=1e-9, init=None, *, criterion="point",
                normal_radius=None, min_neighbours=6, max_curvature=0.01, rcond=1e-3):
    """The statement of CloudAligner.align: the loop on the numpy statements -> Alignment."""
    return CloudAligner("cpu", tau, mode, iters, trim, stride, tol, criterion=criterion, normal_radius=normal_radius,
                        min_neighbours=min_neighbours, max_curvature=max_curvature, rcond=rcond).align(pred_xyz, ref_xyz, init)
