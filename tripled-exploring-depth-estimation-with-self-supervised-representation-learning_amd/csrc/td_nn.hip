// Nearest neighbour within a radius between two clouds of millions of points (tripled_amd/cloud_eval.py):
//   td_nn_query   one thread per query against a reference that is sorted into a uniform grid of cells
// The grid is a sorted list, not a tree and not a hash table: the reference's cell keys (td_cloud.hip's packing, cell edge a
// little over tau) are sorted by torch.sort, td_cloud_heads and torch.cumsum give cell_key [C], cell_start [C+1] and the sort's
// permutation `order` [M'].  With inv_cell = (1 - 2^-20) / tau two points within tau lie in cells at most one apart on every axis,
// so the 27 cells around the query's hold every candidate: the answer is exact.  z sits in the key's low bits, so the three
// z-neighbours of a (dx, dy) column are adjacent in key order: one lower bound per column (9, not 27) and a walk over at most
// three cells.  The winner is the smallest d2 and among equal d2 the lowest ORIGINAL index, so it depends neither on the sort's
// order inside a cell nor on the order the cells are visited.  No sqrt, no floating-point atomics, no kernel waits on another
// workgroup; built with -ffp-contract=off: d2 = ((dx dx) + (dy dy)) + (dz dz), each operation rounded on its own.
#include <math.h>

#include "td_common.h"

namespace td {

#define TD_NN_HALF 1048576        // cell coordinates lie in [-2^20, 2^20): td_cloud.hip's TD_CLOUD_HALF
#define TD_NN_MAX_THRESHOLDS 16

struct NnArgs {
  const double* query;           // [N,3]
  const double* points;          // [M',3] the reference, in cell order
  const long long* order;        // [M'] original index of every sorted point
  const long long* cell_key;     // [C] ascending
  const long long* cell_start;   // [C+1]
  long long N, M, C;
  double inv_cell, tau2;
  double thr2[TD_NN_MAX_THRESHOLDS];
  int K;
  double* d2;                    // [N] (out)
  long long* index;              // [N] (out)
  unsigned long long* counts;    // [K+2]: += within threshold k ..., found, invalid
};

// the first c in [0, C] with cell_key[c] >= key; at most 64 halvings, every read inside [0, C)
__device__ __forceinline__ long long nn_lower_bound(const long long* __restrict__ cell_key, long long C, long long key) {
  long long lo = 0, hi = C;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (cell_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long nn_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(TD_THREADS) void nn_query_kernel(const NnArgs a) {
  __shared__ unsigned cnt[TD_NN_MAX_THRESHOLDS + 2];
  if (threadIdx.x < TD_NN_MAX_THRESHOLDS + 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i < a.N) {
    const double qx = a.query[i * 3], qy = a.query[i * 3 + 1], qz = a.query[i * 3 + 2];
    const double fx = floor(qx * a.inv_cell), fy = floor(qy * a.inv_cell), fz = floor(qz * a.inv_cell);
    const double lo = -(double)TD_NN_HALF, hi = (double)TD_NN_HALF;
    double best = INFINITY;
    long long best_index = -1;
    // a NaN or an inf fails a comparison
    const bool valid = isfinite(qx) && isfinite(qy) && isfinite(qz) && fx >= lo && fx < hi && fy >= lo && fy < hi && fz >= lo && fz < hi;
    if (valid) {
      const long long ix = (long long)fx, iy = (long long)fy, iz = (long long)fz;
      const long long z0 = iz - 1 < -TD_NN_HALF ? -TD_NN_HALF : iz - 1;
      const long long z1 = iz + 1 > TD_NN_HALF - 1 ? TD_NN_HALF - 1 : iz + 1;
      for (int dx = -1; dx <= 1; ++dx) {
        const long long cx = ix + dx;
        if (cx < -TD_NN_HALF || cx >= TD_NN_HALF) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const long long cy = iy + dy;
          if (cy < -TD_NN_HALF || cy >= TD_NN_HALF) continue;
          const long long column = ((cx + TD_NN_HALF) << 42) | ((cy + TD_NN_HALF) << 21);
          const long long k0 = column | (z0 + TD_NN_HALF), k1 = column | (z1 + TD_NN_HALF);
          const long long c0 = nn_lower_bound(a.cell_key, a.C, k0);
          long long c1 = c0;
          while (c1 < a.C && c1 < c0 + 3 && a.cell_key[c1] <= k1) ++c1;      // at most the three z-neighbours
          if (c1 == c0) continue;
          const long long p0 = nn_clamp(a.cell_start[c0], a.M), p1 = nn_clamp(a.cell_start[c1], a.M);      // c1 <= C: inside [C+1]
          for (long long p = p0; p < p1; ++p) {
            const double ex = a.points[p * 3] - qx, ey = a.points[p * 3 + 1] - qy, ez = a.points[p * 3 + 2] - qz;
            const double d2 = ((ex * ex) + (ey * ey)) + (ez * ez);
            if (d2 <= a.tau2 && d2 <= best) {      // a NaN fails
              const long long j = a.order[p];
              if (d2 < best || j < best_index) {
                best = d2;
                best_index = j;
              }
            }
          }
        }
      }
    }
    a.d2[i] = best;
    a.index[i] = best_index;
    if (!valid) {
      atomicAdd(&cnt[a.K + 1], 1u);      // LDS
    } else if (best_index >= 0) {
      atomicAdd(&cnt[a.K], 1u);
      for (int k = 0; k < a.K; ++k)
        if (best <= a.thr2[k]) atomicAdd(&cnt[k], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < a.K + 2 && cnt[threadIdx.x]) atomicAdd(a.counts + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

}  // namespace td

extern "C" int td_nn_query(const double* query, long long N, const double* points, const long long* order, long long M,
                           const long long* cell_key, const long long* cell_start, long long C, double tau, const double* thr2, int K,
                           double* d2, long long* index, long long* counts, td_stream_t stream) {
  if (!query || !cell_start || !d2 || !index || !counts || N < 0 || M < 0 || C < 0 || C > M || K < 0 || K > TD_NN_MAX_THRESHOLDS ||
      (K > 0 && !thr2) || !(tau > 0.0) || !isfinite(tau) || (M > 0 && (!points || !order)) || (C > 0 && !cell_key))
    return TD_ERR_BAD_ARG;
  if (N == 0) return TD_OK;
  td::NnArgs a;
  a.query = query; a.points = points; a.order = order; a.cell_key = cell_key; a.cell_start = cell_start;
  a.N = N; a.M = M; a.C = C;
  a.inv_cell = (1.0 - 0x1p-20) / tau;      // cloud_eval.inv_cell: the grid was built with the same two operations
  a.tau2 = tau * tau;
  for (int k = 0; k < TD_NN_MAX_THRESHOLDS; ++k) a.thr2[k] = k < K ? thr2[k] : 0.0;
  a.K = K; a.d2 = d2; a.index = index; a.counts = reinterpret_cast<unsigned long long*>(counts);
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::nn_query_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  return td::record_launch_error(hipGetLastError(), "td_nn_query");
}
