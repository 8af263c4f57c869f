// A fused cloud aligned to the lidar by iterated closest points (tripled_amd/cloud_align.py): the two device pieces of a loop whose
// correspondences come from td_nn_query (td_nn.hip) and whose closed-form solve (Umeyama) runs on the host.
//   td_cloud_transform   one thread per point: out = c R x + t
//   td_icp_moments       the correspondences reduced to the 17 sums the closed form needs, plus two counters
//   td_icp_plane_moments the same correspondences and the reference's normals reduced to the 37 sums of the point-to-plane step (the
//                        upper triangle of sum a a^T, sum a r, sum r r, sum d2), plus three counters; same tree, same order of sums
// float64 throughout, built with -ffp-contract=off: every product and sum is rounded on its own, in the order written here.  No
// floating-point atomics and no kernel waits on another workgroup: the moments are summed in a FIXED order that depends on N alone
// (stage 1: one workgroup per 256 consecutive rows, the LDS halving tree of td_odom.hip's block_reduce; stage 2: one workgroup, thread j
// adds partials j, j + 256, ... in that order from +0.0, then the same tree), so the result is bit-reproducible and equals
// cloud_align.moments_numpy bit for bit.  The counters are integers: LDS first, then one 64-bit atomic per workgroup and counter.
#include <math.h>

#include "td_common.h"

namespace td {

struct TransformArgs {
  const double* src;      // [N,3]
  double* out;            // [N,3] (may be src)
  long long N;
  double c, R[9], t[3];
};

__global__ __launch_bounds__(TD_THREADS) void cloud_transform_kernel(const TransformArgs a) {
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i >= a.N) return;
  const double x = a.src[i * 3], y = a.src[i * 3 + 1], z = a.src[i * 3 + 2];
#pragma unroll
  for (int k = 0; k < 3; ++k) a.out[i * 3 + k] = a.c * ((a.R[3 * k] * x + a.R[3 * k + 1] * y) + a.R[3 * k + 2] * z) + a.t[k];
}

struct MomentsArgs {
  const double* cur;          // [N,3]
  const double* ref;          // [M,3] in ORIGINAL order
  const long long* index;     // [N]
  const double* d2;           // [N]
  long long N, M, blocks;     // blocks = ceil(N / 256): the rows of partials
  double trim2, origin[3];
  double* partials;           // [blocks,17]
  double* out;                // [17]
  unsigned long long* counters;      // [2]: matched, bad_index (the 16 bytes behind out's 17 doubles)
};

// red[e][j] += red[e][j + s] for s = 128 ... 1: td_odom.hip's block_reduce with the slot as the slow axis, so that the threads of a
// wave touch consecutive doubles (no bank conflict at any s >= 16).  The sums land in red[e][0].
__device__ __forceinline__ void moments_tree(double (*red)[TD_THREADS], const double* v) {
  const int j = threadIdx.x;
#pragma unroll
  for (int e = 0; e < TD_ICP_SLOTS; ++e) red[e][j] = v[e];
  __syncthreads();
  for (int s = TD_THREADS / 2; s > 0; s >>= 1) {
    if (j < s) {
#pragma unroll
      for (int e = 0; e < TD_ICP_SLOTS; ++e) red[e][j] += red[e][j + s];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(TD_THREADS) void icp_moments_rows_kernel(const MomentsArgs a) {
  __shared__ double red[TD_ICP_SLOTS][TD_THREADS];      // 34 816 bytes: four workgroups (16 waves) per CU of 160 KiB
  __shared__ unsigned cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  double v[TD_ICP_SLOTS];
#pragma unroll
  for (int e = 0; e < TD_ICP_SLOTS; ++e) v[e] = 0.0;
  if (i < a.N) {
    const long long j = a.index[i];
    const double d2 = a.d2[i];
    if (j >= a.M || j < -1) {
      atomicAdd(&cnt[1], 1u);      // LDS; nothing is read through such an index
    } else if (j >= 0 && d2 <= a.trim2) {      // a NaN fails
      atomicAdd(&cnt[0], 1u);
      double p[3], q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        p[k] = a.cur[i * 3 + k] - a.origin[k];
        q[k] = a.ref[j * 3 + k] - a.origin[k];
        v[k] = p[k];
        v[3 + k] = q[k];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[6 + 3 * r + c] = q[r] * p[c];
      v[15] = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
      v[16] = d2;
    }
  }
  moments_tree(red, v);
  if (threadIdx.x < TD_ICP_SLOTS) a.partials[(long long)blockIdx.x * TD_ICP_SLOTS + threadIdx.x] = red[threadIdx.x][0];
  if (threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

__global__ __launch_bounds__(TD_THREADS) void icp_moments_finish_kernel(const MomentsArgs a) {
  __shared__ double red[TD_ICP_SLOTS][TD_THREADS];
  double v[TD_ICP_SLOTS];
#pragma unroll
  for (int e = 0; e < TD_ICP_SLOTS; ++e) v[e] = 0.0;
  for (long long k = threadIdx.x; k < a.blocks; k += TD_THREADS) {
#pragma unroll
    for (int e = 0; e < TD_ICP_SLOTS; ++e) v[e] += a.partials[k * TD_ICP_SLOTS + e];
  }
  moments_tree(red, v);
  if (threadIdx.x < TD_ICP_SLOTS) a.out[threadIdx.x] = red[threadIdx.x][0];
}

// ---- point to plane ------------------------------------------------------------------------------------------------------------------
#define TD_ICP_PLANE_GROUP 13      // slots per trip through the LDS tree: 37 = 13 + 13 + 11

struct PlaneMomentsArgs {
  const double* cur;          // [N,3]
  const double* ref;          // [M,3] in ORIGINAL order
  const double* normals;      // [M,3] likewise; all zero: the point has no normal
  const long long* index;     // [N]
  const double* d2;           // [N]
  long long N, M, blocks;     // blocks = ceil(N / 256): the rows of partials
  double trim2, origin[3];
  double* partials;           // [blocks,37]
  double* out;                // [37]
  unsigned long long* counters;      // [3]: matched, bad_index, no_normal (the 24 bytes behind out's 37 doubles)
};

// moments_tree for slots E0 ... E0 + G - 1 of v: the same additions in the same order as one tree over all 37 would make (the slots
// never mix), out of a third of the LDS: 13 x 256 doubles = 26 624 bytes instead of 75 776.  The sums of the group land in
// red[e][0]; thread e < G stores red[e][0] to dst[E0 + e].  Every index into v is a compile-time constant: v stays in registers.
template <int E0, int G>
__device__ __forceinline__ void plane_tree_group(double (*red)[TD_THREADS], const double* v, double* dst) {
  const int j = threadIdx.x;
#pragma unroll
  for (int e = 0; e < G; ++e) red[e][j] = v[E0 + e];
  __syncthreads();
  for (int s = TD_THREADS / 2; s > 0; s >>= 1) {
    if (j < s) {
#pragma unroll
      for (int e = 0; e < G; ++e) red[e][j] += red[e][j + s];
    }
    __syncthreads();
  }
  if (j < G) dst[E0 + j] = red[j][0];
  __syncthreads();      // red is written again by the next group
}

__device__ __forceinline__ void plane_tree(double (*red)[TD_THREADS], const double* v, double* dst) {
  plane_tree_group<0, TD_ICP_PLANE_GROUP>(red, v, dst);
  plane_tree_group<TD_ICP_PLANE_GROUP, TD_ICP_PLANE_GROUP>(red, v, dst);
  plane_tree_group<2 * TD_ICP_PLANE_GROUP, TD_ICP_PLANE_SLOTS - 2 * TD_ICP_PLANE_GROUP>(red, v, dst);
}

__global__ __launch_bounds__(TD_THREADS) void icp_plane_moments_rows_kernel(const PlaneMomentsArgs a) {
  __shared__ double red[TD_ICP_PLANE_GROUP][TD_THREADS];      // 26 624 bytes
  __shared__ unsigned cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  double v[TD_ICP_PLANE_SLOTS];
#pragma unroll
  for (int e = 0; e < TD_ICP_PLANE_SLOTS; ++e) v[e] = 0.0;
  if (i < a.N) {
    const long long j = a.index[i];
    const double d2 = a.d2[i];
    if (j >= a.M || j < -1) {
      atomicAdd(&cnt[1], 1u);      // LDS; nothing is read through such an index
    } else if (j >= 0 && d2 <= a.trim2) {      // a NaN fails
      const double nx = a.normals[j * 3], ny = a.normals[j * 3 + 1], nz = a.normals[j * 3 + 2];
      if (nx == 0.0 && ny == 0.0 && nz == 0.0) {
        atomicAdd(&cnt[2], 1u);
      } else {
        atomicAdd(&cnt[0], 1u);
        double p[3], g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          p[k] = a.cur[i * 3 + k] - a.origin[k];
          const double q = a.ref[j * 3 + k] - a.origin[k];
          g[k] = p[k] - q;
        }
        double c[7];
        c[0] = p[1] * nz - p[2] * ny;
        c[1] = p[2] * nx - p[0] * nz;
        c[2] = p[0] * ny - p[1] * nx;
        c[3] = nx; c[4] = ny; c[5] = nz;
        c[6] = (p[0] * nx + p[1] * ny) + p[2] * nz;
        const double r = (nx * g[0] + ny * g[1]) + nz * g[2];
        int at = 0;
#pragma unroll
        for (int s = 0; s < 7; ++s)
#pragma unroll
          for (int t = s; t < 7; ++t) v[at++] = c[s] * c[t];
#pragma unroll
        for (int s = 0; s < 7; ++s) v[28 + s] = c[s] * r;
        v[35] = r * r;
        v[36] = d2;
      }
    }
  }
  plane_tree(red, v, a.partials + (long long)blockIdx.x * TD_ICP_PLANE_SLOTS);
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

__global__ __launch_bounds__(TD_THREADS) void icp_plane_moments_finish_kernel(const PlaneMomentsArgs a) {
  __shared__ double red[TD_ICP_PLANE_GROUP][TD_THREADS];
  double v[TD_ICP_PLANE_SLOTS];
#pragma unroll
  for (int e = 0; e < TD_ICP_PLANE_SLOTS; ++e) v[e] = 0.0;
  for (long long k = threadIdx.x; k < a.blocks; k += TD_THREADS) {
#pragma unroll
    for (int e = 0; e < TD_ICP_PLANE_SLOTS; ++e) v[e] += a.partials[k * TD_ICP_PLANE_SLOTS + e];
  }
  plane_tree(red, v, a.out);
}

static inline bool all_finite(const double* v, int n) {
  for (int k = 0; k < n; ++k)
    if (!isfinite(v[k])) return false;
  return true;
}

}  // namespace td

extern "C" int td_cloud_transform(const double* src, long long N, double c, const double* R, const double* t, double* out,
                                  td_stream_t stream) {
  if (!src || !out || !R || !t || N < 0 || !isfinite(c) || !td::all_finite(R, 9) || !td::all_finite(t, 3)) return TD_ERR_BAD_ARG;
  if (N == 0) return TD_OK;
  td::TransformArgs a;
  a.src = src; a.out = out; a.N = N; a.c = c;
  for (int k = 0; k < 9; ++k) a.R[k] = R[k];
  for (int k = 0; k < 3; ++k) a.t[k] = t[k];
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::cloud_transform_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  return td::record_launch_error(hipGetLastError(), "td_cloud_transform");
}

extern "C" long long td_icp_moments_workspace(long long N) {
  if (N <= 0) return 0;
  return ((N + TD_THREADS - 1) / TD_THREADS) * TD_ICP_SLOTS * (long long)sizeof(double);
}

extern "C" int td_icp_moments(const double* cur, long long N, const double* ref, long long M, const long long* index, const double* d2,
                              double trim2, const double* origin, void* workspace, long long workspace_bytes, double* out,
                              td_stream_t stream) {
  if (!out || !origin || N < 0 || M < 0 || !(trim2 >= 0.0) || !td::all_finite(origin, 3) || workspace_bytes < 0 ||
      (N > 0 && (!cur || !index || !d2 || !workspace)) || (N > 0 && M > 0 && !ref) || !td::aligned_to(out, 8) ||
      !td::aligned_to(workspace, 8))
    return TD_ERR_BAD_ARG;
  if (workspace_bytes < td_icp_moments_workspace(N)) return TD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // the 17 sums and the two counters start from zero: N = 0 ends here, with out zeroed
  const hipError_t e = hipMemsetAsync(out, 0, (TD_ICP_SLOTS + 2) * sizeof(double), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_icp_moments (clear)");
  if (N == 0) return TD_OK;
  td::MomentsArgs a;
  a.cur = cur; a.ref = ref; a.index = index; a.d2 = d2; a.N = N; a.M = M;
  a.trim2 = trim2;
  for (int k = 0; k < 3; ++k) a.origin[k] = origin[k];
  a.partials = static_cast<double*>(workspace); a.out = out;
  a.counters = reinterpret_cast<unsigned long long*>(out + TD_ICP_SLOTS);
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  a.blocks = blocks;
  hipLaunchKernelGGL(td::icp_moments_rows_kernel, dim3(blocks), dim3(TD_THREADS), 0, st, a);
  const int rc = td::record_launch_error(hipGetLastError(), "td_icp_moments (rows)");
  if (rc != TD_OK) return rc;
  hipLaunchKernelGGL(td::icp_moments_finish_kernel, dim3(1), dim3(TD_THREADS), 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_icp_moments (finish)");
}

extern "C" long long td_icp_plane_moments_workspace(long long N) {
  if (N <= 0) return 0;
  return ((N + TD_THREADS - 1) / TD_THREADS) * TD_ICP_PLANE_SLOTS * (long long)sizeof(double);
}

extern "C" int td_icp_plane_moments(const double* cur, long long N, const double* ref, const double* normals, long long M,
                                    const long long* index, const double* d2, double trim2, const double* origin, void* workspace,
                                    long long workspace_bytes, double* out, td_stream_t stream) {
  if (!out || !origin || N < 0 || M < 0 || !(trim2 >= 0.0) || !td::all_finite(origin, 3) || workspace_bytes < 0 ||
      (N > 0 && (!cur || !index || !d2 || !workspace)) || (N > 0 && M > 0 && (!ref || !normals)) || !td::aligned_to(out, 8) ||
      !td::aligned_to(workspace, 8))
    return TD_ERR_BAD_ARG;
  if (workspace_bytes < td_icp_plane_moments_workspace(N)) return TD_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  // the 37 sums and the three counters start from zero: N = 0 ends here, with out zeroed
  const hipError_t e = hipMemsetAsync(out, 0, (TD_ICP_PLANE_SLOTS + 3) * sizeof(double), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_icp_plane_moments (clear)");
  if (N == 0) return TD_OK;
  td::PlaneMomentsArgs a;
  a.cur = cur; a.ref = ref; a.normals = normals; a.index = index; a.d2 = d2; a.N = N; a.M = M;
  a.trim2 = trim2;
  for (int k = 0; k < 3; ++k) a.origin[k] = origin[k];
  a.partials = static_cast<double*>(workspace); a.out = out;
  a.counters = reinterpret_cast<unsigned long long*>(out + TD_ICP_PLANE_SLOTS);
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  a.blocks = blocks;
  hipLaunchKernelGGL(td::icp_plane_moments_rows_kernel, dim3(blocks), dim3(TD_THREADS), 0, st, a);
  const int rc = td::record_launch_error(hipGetLastError(), "td_icp_plane_moments (rows)");
  if (rc != TD_OK) return rc;
  hipLaunchKernelGGL(td::icp_plane_moments_finish_kernel, dim3(1), dim3(TD_THREADS), 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_icp_plane_moments (finish)");
}
