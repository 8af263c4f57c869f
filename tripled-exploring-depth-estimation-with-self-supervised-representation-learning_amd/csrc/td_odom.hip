// KITTI odometry evaluation on the device (reference scripts/eval_pose.py, scripts/draw_odometry.py,
// mono/tools/kitti_evaluation_toolkit.py):
//   td_pose_pairs_u8         uint8 frames -> the pose network's input pairs (ToTensor + channel cat), fp32 / bf16
//   td_odom_trajectory       relative transforms -> global poses, G_{k+1} = G_k inv(M_k): chunked ordered scan in one workgroup
//   td_odom_snippet_ate      the 5-frame snippet ATE of eval_pose.py, one thread per snippet
//   td_odom_sequence_errors  Umeyama scale, cumulative distances, one thread per (first_frame, length) segment
// All pose arithmetic is float64 (float32 inputs are widened exactly), every sum has a fixed order and there are no
// floating-point atomics: two calls on the same inputs return the same bits.  The file is built with -ffp-contract=off, so the
// sequential distance sum rounds exactly like the toolkit's Python loop.
#include <math.h>

#include "td_common.h"
#include "td_vec8.h"

namespace td {

// ---------------------------------------------------------------------------------------------------------------------------
// pairs

// Pair i = cat(frame i, frame i+1) is the 6 H W contiguous bytes that start at frame i: a streaming conversion.
// VEC = 8: one 8-byte load per thread (the caller guarantees 3 H W % 8 == 0 and aligned bases); VEC = 1: scalar.
template <int VEC, bool BF16>
__global__ __launch_bounds__(TD_THREADS) void pose_pairs_kernel(const uint8_t* __restrict__ frames, long long frame_elems,
                                                                int first, long long out_first, void* __restrict__ out) {
  const long long row_elems = 2 * frame_elems;
  const long long k = ((long long)blockIdx.x * TD_THREADS + threadIdx.x) * VEC;
  if (k >= row_elems) return;
  const int r = blockIdx.y;
  const uint8_t* src = frames + (long long)(first + r) * frame_elems + k;
  const long long o = (out_first + r) * row_elems + k;
  if (VEC == 8) {
    const uint2 w = *reinterpret_cast<const uint2*>(src);
    float v[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = (float)((w.x >> (8 * j)) & 0xffu) / 255.f;
      v[4 + j] = (float)((w.y >> (8 * j)) & 0xffu) / 255.f;
    }
    if (BF16) {
      uint4 p;
      p.x = f2bf(v[0]) | ((unsigned)f2bf(v[1]) << 16);
      p.y = f2bf(v[2]) | ((unsigned)f2bf(v[3]) << 16);
      p.z = f2bf(v[4]) | ((unsigned)f2bf(v[5]) << 16);
      p.w = f2bf(v[6]) | ((unsigned)f2bf(v[7]) << 16);
      *reinterpret_cast<uint4*>(static_cast<unsigned short*>(out) + o) = p;
    } else {
      float4* dst = reinterpret_cast<float4*>(static_cast<float*>(out) + o);
      dst[0] = make_float4(v[0], v[1], v[2], v[3]);
      dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
  } else {
    const float v = (float)src[0] / 255.f;
    if (BF16) static_cast<unsigned short*>(out)[o] = f2bf(v);
    else static_cast<float*>(out)[o] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// affine 3x4 transforms in float64: m[0..11] = rows of [A | t]

struct Aff { double m[12]; };

__device__ __forceinline__ Aff aff_identity() {
  Aff r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.m[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
  return r;
}

// top three rows of a row-major [.,4,4] (stride 16) or [.,3,4] (stride 12) matrix
template <typename T>
__device__ __forceinline__ Aff aff_load(const T* p) {
  Aff r;
#pragma unroll
  for (int k = 0; k < 12; ++k) r.m[k] = (double)p[k];
  return r;
}

__device__ __forceinline__ Aff aff_mul(const Aff& a, const Aff& b) {      // a b
  Aff r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double s = (a.m[i * 4 + 0] * b.m[j] + a.m[i * 4 + 1] * b.m[4 + j]) + a.m[i * 4 + 2] * b.m[8 + j];
      if (j == 3) s += a.m[i * 4 + 3];
      r.m[i * 4 + j] = s;
    }
  }
  return r;
}

// affine inverse: A^-1 by cofactors, -A^-1 t.  NOT the transpose: a float32 Rodrigues matrix is orthogonal to ~1e-7 only.
__device__ __forceinline__ Aff aff_inv(const Aff& a) {
  const double a00 = a.m[0], a01 = a.m[1], a02 = a.m[2], a10 = a.m[4], a11 = a.m[5], a12 = a.m[6], a20 = a.m[8], a21 = a.m[9],
               a22 = a.m[10];
  const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
  const double det = (a00 * c00 + a01 * c01) + a02 * c02;
  const double id = 1.0 / det;
  Aff r;
  r.m[0] = c00 * id; r.m[1] = (a02 * a21 - a01 * a22) * id; r.m[2] = (a01 * a12 - a02 * a11) * id;
  r.m[4] = c01 * id; r.m[5] = (a00 * a22 - a02 * a20) * id; r.m[6] = (a02 * a10 - a00 * a12) * id;
  r.m[8] = c02 * id; r.m[9] = (a01 * a20 - a00 * a21) * id; r.m[10] = (a00 * a11 - a01 * a10) * id;
#pragma unroll
  for (int i = 0; i < 3; ++i)
    r.m[i * 4 + 3] = -((r.m[i * 4 + 0] * a.m[3] + r.m[i * 4 + 1] * a.m[7]) + r.m[i * 4 + 2] * a.m[11]);
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// trajectory: G_0 = I, G_{k+1} = G_k inv(M_k)   (draw_odometry.py:62-74)

// One workgroup.  Thread j owns the contiguous chunk [j c, (j+1) c): it composes the chunk in order, the workgroup scans the
// chunk totals in LDS (Hillis-Steele, the earlier operand always on the left: composition is associative, not commutative),
// and the thread composes its chunk again starting from the product of everything before it.
template <typename T>
__global__ __launch_bounds__(TD_ODOM_THREADS) void odom_trajectory_kernel(const T* __restrict__ M, int n, double* __restrict__ G) {
  __shared__ double tot[2][TD_ODOM_THREADS][12];
  const int j = threadIdx.x;
  const int c = (n + TD_ODOM_THREADS - 1) / TD_ODOM_THREADS;
  const long long lo = (long long)j * c;
  const int k0 = lo < n ? (int)lo : n, k1 = lo + c < n ? (int)(lo + c) : n;
  Aff acc = aff_identity();
  for (int k = k0; k < k1; ++k) acc = aff_mul(acc, aff_inv(aff_load(M + (size_t)k * 16)));
#pragma unroll
  for (int e = 0; e < 12; ++e) tot[0][j][e] = acc.m[e];
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < TD_ODOM_THREADS; off <<= 1) {
    Aff mine = aff_load(tot[cur][j]);
    if (j >= off) mine = aff_mul(aff_load(tot[cur][j - off]), mine);
#pragma unroll
    for (int e = 0; e < 12; ++e) tot[cur ^ 1][j][e] = mine.m[e];
    cur ^= 1;
    __syncthreads();
  }
  acc = j == 0 ? aff_identity() : aff_load(tot[cur][j - 1]);      // exclusive prefix
  if (j == 0) {
#pragma unroll
    for (int e = 0; e < 12; ++e) G[e] = acc.m[e];
  }
  for (int k = k0; k < k1; ++k) {
    acc = aff_mul(acc, aff_inv(aff_load(M + (size_t)k * 16)));
    double* g = G + (size_t)(k + 1) * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) g[e] = acc.m[e];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// snippet ATE (eval_pose.py:66-80, dump_xyz, compute_ate)

template <typename T>
__global__ __launch_bounds__(TD_ODOM_THREADS) void odom_snippet_ate_kernel(const T* __restrict__ M, const double* __restrict__ Ggt,
                                                                           int n, int track_length, double* __restrict__ ates) {
  const int i = blockIdx.x * TD_ODOM_THREADS + threadIdx.x;
  if (i >= n) return;
  const int cnt = (track_length - 1 < n - i) ? track_length - 1 : n - i;      // transforms in this snippet; points: cnt + 1
  Aff cp = aff_identity(), cg = aff_identity();
  double pp[16][3], gg[16][3];
  pp[0][0] = pp[0][1] = pp[0][2] = 0.0;
  gg[0][0] = gg[0][1] = gg[0][2] = 0.0;
  for (int s = 0; s < cnt; ++s) {
    const int k = i + s;
    cp = aff_mul(cp, aff_load(M + (size_t)k * 16));
    // gt_local = inv(inv(G_k) G_{k+1})
    const Aff loc = aff_inv(aff_mul(aff_inv(aff_load(Ggt + (size_t)k * 12)), aff_load(Ggt + (size_t)(k + 1) * 12)));
    cg = aff_mul(cg, loc);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      pp[s + 1][d] = cp.m[d * 4 + 3];
      gg[s + 1][d] = cg.m[d * 4 + 3];
    }
  }
  // offset = gt[0] - pred[0] (both snippets start at the origin: 0, added as the reference does)
  double num = 0.0, den = 0.0;
  for (int s = 0; s <= cnt; ++s)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double p = pp[s][d] + (gg[0][d] - pp[0][d]);
      pp[s][d] = p;
      num += gg[s][d] * p;
      den += p * p;
    }
  const double scale = num / den;      // 0 / 0 -> NaN, as numpy
  double sq = 0.0;
  for (int s = 0; s <= cnt; ++s)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double e = pp[s][d] * scale - gg[s][d];
      sq += e * e;
    }
  ates[i] = sqrt(sq) / (double)(cnt + 1);
}

// ---------------------------------------------------------------------------------------------------------------------------
// sequence errors (kitti_evaluation_toolkit.py: trajectoryDistances, lastFrameFromSegmentLength, calcSequenceErrors;
// geometry.umeyama_alignment's scale for align_trajectory(correct_only_scale=True))

struct SeqArgs {
  const double* gt;      // [m,3,4]
  const double* pred;    // [m,3,4]
  int m, n_lengths, step, align;
  double lengths[TD_ODOM_MAX_LENGTHS];
  double* dist;          // [m] (out)
  double* rows;          // [F,L,5] (out)
  uint8_t* valid;        // [F,L] (out)
  double* summary;       // [2] = (scale, total distance) (out)
};

// K sums over the workgroup in LDS, fixed tree -> bit-reproducible; result in every thread through red[0][.]
template <int K>
__device__ __forceinline__ void block_reduce(double (*red)[10], const double* v) {
  const int j = threadIdx.x;
#pragma unroll
  for (int e = 0; e < K; ++e) red[j][e] = v[e];
  __syncthreads();
  for (int s = TD_ODOM_THREADS / 2; s > 0; s >>= 1) {
    if (j < s) {
#pragma unroll
      for (int e = 0; e < K; ++e) red[j][e] += red[j + s][e];
    }
    __syncthreads();
  }
}

// Singular values of a 3x3 by one-sided (Hestenes) Jacobi: rotate column pairs until they are orthogonal; the column norms
// are the singular values.  Fixed sweep count (convergence is quadratic; 3x3 needs 4-6 sweeps).
__device__ void singular_values_3x3(double a[3][3], double d[3]) {
  for (int sweep = 0; sweep < 16; ++sweep) {
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < 3; ++i) {
          alpha += a[i][p] * a[i][p];
          beta += a[i][q] * a[i][q];
          gamma += a[i][p] * a[i][q];
        }
        if (gamma == 0.0) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double x = a[i][p], y = a[i][q];
          a[i][p] = c * x - s * y;
          a[i][q] = s * x + c * y;
        }
      }
  }
  for (int q = 0; q < 3; ++q) d[q] = sqrt((a[0][q] * a[0][q] + a[1][q] * a[1][q]) + a[2][q] * a[2][q]);
}

__global__ __launch_bounds__(TD_ODOM_THREADS) void odom_sequence_errors_kernel(const SeqArgs a) {
  __shared__ double red[TD_ODOM_THREADS][10];
  __shared__ double s_scale;
  const int j = threadIdx.x, m = a.m;
  double scale = 1.0;
  if (a.align) {
    // x = predicted positions, y = ground-truth positions
    double v[10];
    for (int e = 0; e < 6; ++e) v[e] = 0.0;
    for (int i = j; i < m; i += TD_ODOM_THREADS)
      for (int d = 0; d < 3; ++d) {
        v[d] += a.pred[(size_t)i * 12 + d * 4 + 3];
        v[3 + d] += a.gt[(size_t)i * 12 + d * 4 + 3];
      }
    block_reduce<6>(red, v);
    double mx[3], my[3];
    for (int d = 0; d < 3; ++d) {
      mx[d] = red[0][d] / (double)m;
      my[d] = red[0][3 + d] / (double)m;
    }
    __syncthreads();
    for (int e = 0; e < 10; ++e) v[e] = 0.0;
    for (int i = j; i < m; i += TD_ODOM_THREADS) {
      double dx[3], dy[3];
      for (int d = 0; d < 3; ++d) {
        dx[d] = a.pred[(size_t)i * 12 + d * 4 + 3] - mx[d];
        dy[d] = a.gt[(size_t)i * 12 + d * 4 + 3] - my[d];
      }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) v[r * 3 + c] += dy[r] * dx[c];      // outer(y - mean_y, x - mean_x)
      v[9] += (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2];
    }
    block_reduce<10>(red, v);
    if (j == 0) {
      double cov[3][3], d[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) cov[r][c] = red[0][r * 3 + c] / (double)m;
      const double sigma_x = red[0][9] / (double)m;
      const double det = (cov[0][0] * (cov[1][1] * cov[2][2] - cov[1][2] * cov[2][1])
                          - cov[0][1] * (cov[1][0] * cov[2][2] - cov[1][2] * cov[2][0]))
                         + cov[0][2] * (cov[1][0] * cov[2][1] - cov[1][1] * cov[2][0]);
      singular_values_3x3(cov, d);
      const double dmin = fmin(d[0], fmin(d[1], d[2]));
      double tr = (d[0] + d[1]) + d[2];
      if (det < 0.0) tr -= 2.0 * dmin;      // S = diag(1, 1, sign(det(u) det(v))) weighs the SMALLEST singular value
      s_scale = tr / sigma_x;
    }
    __syncthreads();
    scale = s_scale;
  }
  if (j == 64 % TD_ODOM_THREADS) {
    // trajectoryDistances: sequential, in index order, so that every segment end is the toolkit's
    double acc = 0.0;
    a.dist[0] = 0.0;
    for (int i = 0; i + 1 < m; ++i) {
      const double dx = a.gt[(size_t)i * 12 + 3] - a.gt[(size_t)(i + 1) * 12 + 3];
      const double dy = a.gt[(size_t)i * 12 + 7] - a.gt[(size_t)(i + 1) * 12 + 7];
      const double dz = a.gt[(size_t)i * 12 + 11] - a.gt[(size_t)(i + 1) * 12 + 11];
      acc = acc + sqrt((dx * dx + dy * dy) + dz * dz);
      a.dist[i + 1] = acc;
    }
    a.summary[0] = scale;
    a.summary[1] = acc;
  }
  __threadfence_block();
  __syncthreads();
  const int F = (m + a.step - 1) / a.step, L = a.n_lengths;
  for (int idx = j; idx < F * L; idx += TD_ODOM_THREADS) {
    const int f = idx / L, l = idx - f * L;
    const int first = f * a.step;
    const double len = a.lengths[l];
    const double thr = a.dist[first] + len;
    // first i in [first, m) with dist[i] > thr; dist is non-decreasing
    int lo = first, hi = m;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (a.dist[mid] > thr) hi = mid; else lo = mid + 1;
    }
    double* row = a.rows + (size_t)idx * 5;
    row[0] = (double)first;
    row[3] = len;
    if (lo >= m) {
      const double nan = __longlong_as_double(0x7ff8000000000000LL);
      row[1] = nan; row[2] = nan; row[4] = nan;
      a.valid[idx] = 0;
      continue;
    }
    const int last = lo;
    Aff p0 = aff_load(a.pred + (size_t)first * 12), p1 = aff_load(a.pred + (size_t)last * 12);
    for (int d = 0; d < 3; ++d) {
      p0.m[d * 4 + 3] = scale * p0.m[d * 4 + 3];
      p1.m[d * 4 + 3] = scale * p1.m[d * 4 + 3];
    }
    const Aff dgt = aff_mul(aff_inv(aff_load(a.gt + (size_t)first * 12)), aff_load(a.gt + (size_t)last * 12));
    const Aff dpr = aff_mul(aff_inv(p0), p1);
    const Aff err = aff_mul(aff_inv(dpr), dgt);
    const double dd = 0.5 * (((err.m[0] + err.m[5]) + err.m[10]) - 1.0);
    const double r_err = acos(fmax(fmin(dd, 1.0), -1.0));
    const double t_err = sqrt((err.m[3] * err.m[3] + err.m[7] * err.m[7]) + err.m[11] * err.m[11]);
    const double num_frames = (double)(last - first) + 1.0;
    row[1] = r_err / len;
    row[2] = t_err / len;
    row[4] = len / (0.1 * num_frames);
    a.valid[idx] = 1;
  }
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_pose_pairs_u8(const uint8_t* frames, int n, int H, int W, int first, int count, int dtype, void* out,
                                long long out_first, td_stream_t stream) {
  if (!frames || !out || n <= 0 || H <= 0 || W <= 0 || first < 0 || count <= 0 || (long long)first + count > n || out_first < 0 ||
      (dtype != TD_DTYPE_F32 && dtype != TD_DTYPE_BF16))
    return TD_ERR_BAD_ARG;
  const long long frame_elems = 3LL * H * W;
  const bool vec = frame_elems % 8 == 0 && td::aligned_to(frames, 8) && td::aligned_to(out, 16);
  const dim3 grid(td::blocks_1d(vec ? 2 * frame_elems / 8 : 2 * frame_elems), (unsigned)count), block(TD_THREADS);
  if (!grid.x || count > 65535) return TD_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (vec && dtype == TD_DTYPE_F32)
    hipLaunchKernelGGL((td::pose_pairs_kernel<8, false>), grid, block, 0, s, frames, frame_elems, first, out_first, out);
  else if (vec)
    hipLaunchKernelGGL((td::pose_pairs_kernel<8, true>), grid, block, 0, s, frames, frame_elems, first, out_first, out);
  else if (dtype == TD_DTYPE_F32)
    hipLaunchKernelGGL((td::pose_pairs_kernel<1, false>), grid, block, 0, s, frames, frame_elems, first, out_first, out);
  else
    hipLaunchKernelGGL((td::pose_pairs_kernel<1, true>), grid, block, 0, s, frames, frame_elems, first, out_first, out);
  return td::record_launch_error(hipGetLastError(), "td_pose_pairs_u8");
}

extern "C" int td_odom_trajectory(const void* rel, int rel_f64, int n, double* poses, td_stream_t stream) {
  if (!rel || !poses || n <= 0 || (rel_f64 != 0 && rel_f64 != 1)) return TD_ERR_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (rel_f64)
    hipLaunchKernelGGL((td::odom_trajectory_kernel<double>), dim3(1), dim3(TD_ODOM_THREADS), 0, s, (const double*)rel, n, poses);
  else
    hipLaunchKernelGGL((td::odom_trajectory_kernel<float>), dim3(1), dim3(TD_ODOM_THREADS), 0, s, (const float*)rel, n, poses);
  return td::record_launch_error(hipGetLastError(), "td_odom_trajectory");
}

extern "C" int td_odom_snippet_ate(const void* rel, int rel_f64, const double* gt_poses, int n, int track_length, double* ates,
                                   td_stream_t stream) {
  if (!rel || !gt_poses || !ates || n <= 0 || (rel_f64 != 0 && rel_f64 != 1) || track_length < 2 || track_length > 16)
    return TD_ERR_BAD_ARG;
  const dim3 grid((n + TD_ODOM_THREADS - 1) / TD_ODOM_THREADS), block(TD_ODOM_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (rel_f64)
    hipLaunchKernelGGL((td::odom_snippet_ate_kernel<double>), grid, block, 0, s, (const double*)rel, gt_poses, n, track_length, ates);
  else
    hipLaunchKernelGGL((td::odom_snippet_ate_kernel<float>), grid, block, 0, s, (const float*)rel, gt_poses, n, track_length, ates);
  return td::record_launch_error(hipGetLastError(), "td_odom_snippet_ate");
}

extern "C" int td_odom_sequence_errors(const double* gt_poses, const double* pred_poses, int m, const double* lengths, int n_lengths,
                                       int step, int align_scale, double* dist, double* rows, uint8_t* valid, double* summary,
                                       td_stream_t stream) {
  if (!gt_poses || !pred_poses || !lengths || !dist || !rows || !valid || !summary || m <= 0 || n_lengths <= 0 ||
      n_lengths > TD_ODOM_MAX_LENGTHS || step <= 0)
    return TD_ERR_BAD_ARG;
  td::SeqArgs a;
  a.gt = gt_poses; a.pred = pred_poses; a.m = m; a.n_lengths = n_lengths; a.step = step; a.align = align_scale ? 1 : 0;
  for (int i = 0; i < TD_ODOM_MAX_LENGTHS; ++i) a.lengths[i] = i < n_lengths ? lengths[i] : 0.0;
  for (int i = 0; i < n_lengths; ++i)
    if (!(lengths[i] > 0.0)) return TD_ERR_BAD_ARG;
  a.dist = dist; a.rows = rows; a.valid = valid; a.summary = summary;
  hipLaunchKernelGGL(td::odom_sequence_errors_kernel, dim3(1), dim3(TD_ODOM_THREADS), 0, (hipStream_t)stream, a);
  return td::record_launch_error(hipGetLastError(), "td_odom_sequence_errors");
}
