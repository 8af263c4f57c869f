// Nearest neighbour within a radius between two clouds of millions of points (tripled_amd/cloud_eval.py):
//   td_nn_query   one thread per query against a reference that is sorted into a uniform grid of cells
// The grid is a sorted list, not a tree and not a hash table: the reference's cell keys (td_grid.h's packing, cell edge a
// little over tau) are sorted by torch.sort, td_cloud_heads and torch.cumsum give cell_key [C], cell_start [C+1] and the sort's
// permutation `order` [M'].  The 27 cells around the query's hold every candidate (td_grid.h), so the answer is exact.  The winner
// is the smallest d2 and among equal d2 the lowest ORIGINAL index, so it depends neither on the sort's order inside a cell nor on
// the order the cells are visited.  No sqrt, no floating-point atomics, no kernel waits on another
// workgroup; built with -ffp-contract=off: d2 = ((dx dx) + (dy dy)) + (dz dz), each operation rounded on its own.
#include <math.h>

#include "td_grid.h"

namespace td {

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

__global__ __launch_bounds__(TD_THREADS) void nn_query_kernel(const NnArgs a) {
  __shared__ unsigned cnt[TD_NN_MAX_THRESHOLDS + 2];
  if (threadIdx.x < TD_NN_MAX_THRESHOLDS + 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i < a.N) {
    const double qx = a.query[i * 3], qy = a.query[i * 3 + 1], qz = a.query[i * 3 + 2];
    double best = INFINITY;
    long long best_index = -1;
    long long ix, iy, iz;
    const bool valid = grid_cell_of(qx, qy, qz, a.inv_cell, ix, iy, iz);
    if (valid) {
      const long long z0 = iz - 1 < -TD_KEY_HALF ? -TD_KEY_HALF : iz - 1;
      const long long z1 = iz + 1 > TD_KEY_HALF - 1 ? TD_KEY_HALF - 1 : iz + 1;
      for (int dx = -1; dx <= 1; ++dx) {
        const long long cx = ix + dx;
        if (cx < -TD_KEY_HALF || cx >= TD_KEY_HALF) continue;
        for (int dy = -1; dy <= 1; ++dy) {
          const long long cy = iy + dy;
          if (cy < -TD_KEY_HALF || cy >= TD_KEY_HALF) continue;
          const long long c0 = grid_lower_bound(a.cell_key, a.C, key_pack(cx, cy, z0));
          long long c1 = c0;
          while (c1 < a.C && c1 < c0 + 3 && a.cell_key[c1] <= key_pack(cx, cy, z1)) ++c1;      // at most the three z-neighbours
          if (c1 == c0) continue;
          const long long p0 = grid_row(a.cell_start[c0], a.M), p1 = grid_row(a.cell_start[c1], a.M);      // c1 <= C: inside [C+1]
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
