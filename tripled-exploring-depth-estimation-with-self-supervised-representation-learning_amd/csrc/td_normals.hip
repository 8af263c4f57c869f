// Surface normals of a cloud (tripled_amd/cloud_normals.py):
//   td_cloud_normals   one thread per query against a cloud that is sorted into td_nn_query's uniform grid of cells
// The query walks the grid the way td_nn_query does (td_nn.hip, over td_grid.h's pieces) and gathers, over every
// grid point within `radius` of it, ten 64-bit INTEGER sums of the offsets quantised to radius 2^-18: the count, the three first and
// the six second moments.  Integer sums do not depend on the order of the points inside a cell or on the order the cells are visited,
// like the project's other exact kernels.  The covariance, its eigen-decomposition (cyclic Jacobi, a FIXED number of sweeps, only
// + - * /, sqrt and comparisons) and the normal follow per query in float64 in the order written in cloud_normals.py's docstring;
// built with -ffp-contract=off, so every product and sum is rounded on its own and the result equals cloud_normals.normals_numpy bit
// for bit.  No floating-point atomics and no kernel waits on another workgroup; the five class counters go to LDS first, then one
// 64-bit atomic per workgroup and counter.  Everything the Jacobi touches has a compile-time index: no scratch.
#include <math.h>

#include "td_grid.h"

namespace td {

#define TD_NORMALS_MAX_POINTS (1LL << 26)

struct NormalsArgs {
  const double* query;           // [N,3]
  const double* points;          // [M,3] the cloud, in cell order
  const long long* cell_key;     // [C] ascending
  const long long* cell_start;   // [C+1]
  long long N, M, C;
  double inv_cell, radius2, Q, max_curvature;
  long long min_neighbours;
  double* normal;                // [N,3] (out)
  double* curvature;             // [N] (out)
  long long* count;              // [N] (out)
  unsigned long long* counters;  // [5]: += valid, few, degenerate, rough, invalid
};

// One Jacobi rotation in the (p, q) plane of the symmetric matrix (app, aqq, apq; arp, arq: the third row's entries) and of the rows
// of V (v0p, v0q, ...).  Skipped when apq is exactly 0.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double sign = theta < 0.0 ? -1.0 : 1.0;
  const double t = sign / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  double x = arp, y = arq;
  arp = c * x - s * y;
  arq = s * x + c * y;
  x = v0p; y = v0q;
  v0p = c * x - s * y;
  v0q = s * x + c * y;
  x = v1p; y = v1q;
  v1p = c * x - s * y;
  v1q = s * x + c * y;
  x = v2p; y = v2q;
  v2p = c * x - s * y;
  v2q = s * x + c * y;
}

__global__ __launch_bounds__(TD_THREADS) void cloud_normals_kernel(const NormalsArgs a) {
  __shared__ unsigned cnt[5];
  if (threadIdx.x < 5) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i < a.N) {
    const double qx = a.query[i * 3], qy = a.query[i * 3 + 1], qz = a.query[i * 3 + 2];
    long long ix, iy, iz;
    const bool valid = grid_cell_of(qx, qy, qz, a.inv_cell, ix, iy, iz);
    long long n = 0, sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
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
            if (d2 <= a.radius2) {      // a NaN fails; |e_k Q| <= 2^18 (1 + 2^-52): the conversions cannot overflow
              const long long kx = (long long)rint(ex * a.Q), ky = (long long)rint(ey * a.Q), kz = (long long)rint(ez * a.Q);
              n += 1;
              sx += kx; sy += ky; sz += kz;
              sxx += kx * kx; sxy += kx * ky; sxz += kx * kz;
              syy += ky * ky; syz += ky * kz; szz += kz * kz;
            }
          }
        }
      }
    }
    double nx = 0.0, ny = 0.0, nz = 0.0, curvature = INFINITY;
    int cause = 4;                                   // invalid
    if (valid) {
      cause = 1;                                     // few
      if (n >= a.min_neighbours) {
        const double dn = (double)n;
        const double mx = (double)sx / dn, my = (double)sy / dn, mz = (double)sz / dn;
        double a00 = (double)sxx / dn - mx * mx, a01 = (double)sxy / dn - mx * my, a02 = (double)sxz / dn - mx * mz;
        double a11 = (double)syy / dn - my * my, a12 = (double)syz / dn - my * mz, a22 = (double)szz / dn - mz * mz;
        double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
        for (int sweep = 0; sweep < TD_NORMALS_SWEEPS; ++sweep) {      // never fewer: no early exit
          jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1), r = 2
          jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2), r = 1
          jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2), r = 0
        }
        int at = a11 < a00 ? 1 : 0;
        if (a22 < (at == 1 ? a11 : a00)) at = 2;
        const double lmin = at == 0 ? a00 : (at == 1 ? a11 : a22);
        const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;      // finite here, or rejected below
        const double inner = hi01 < a22 ? hi01 : a22;
        const double mid = lo01 > inner ? lo01 : inner;
        const double trace = (a00 + a11) + a22;
        double x = at == 0 ? v00 : (at == 1 ? v01 : v02);
        double y = at == 0 ? v10 : (at == 1 ? v11 : v12);
        double z = at == 0 ? v20 : (at == 1 ? v21 : v22);
        const double norm = sqrt(((x * x) + (y * y)) + (z * z));
        x = x / norm; y = y / norm; z = z / norm;
        int big = fabs(y) > fabs(x) ? 1 : 0;
        if (fabs(z) > (big == 1 ? fabs(y) : fabs(x))) big = 2;
        const double lead = big == 0 ? x : (big == 1 ? y : z);
        if (lead < 0.0) { x = -x; y = -y; z = -z; }
        const double curv = (lmin > 0.0 ? lmin : 0.0) / trace;
        const bool fine = trace > 0.0 && mid > 0.0 && isfinite(a00) && isfinite(a11) && isfinite(a22) && isfinite(x) && isfinite(y) &&
                          isfinite(z) && isfinite(curv);
        cause = 2;                                   // degenerate
        if (fine) {
          curvature = curv;
          cause = 3;                                 // rough
          if (!(curv > a.max_curvature)) {
            cause = 0;
            nx = x; ny = y; nz = z;
          }
        }
      }
    }
    a.normal[i * 3] = nx;
    a.normal[i * 3 + 1] = ny;
    a.normal[i * 3 + 2] = nz;
    a.curvature[i] = curvature;
    a.count[i] = valid ? n : 0;
    atomicAdd(&cnt[cause], 1u);      // LDS
  }
  __syncthreads();
  if (threadIdx.x < 5 && cnt[threadIdx.x]) atomicAdd(a.counters + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

}  // namespace td

extern "C" int td_cloud_normals(const double* query, long long N, const double* points, long long M, const long long* cell_key,
                                const long long* cell_start, long long C, double tau, double radius, double Q, long long min_neighbours,
                                double max_curvature, double* normal, double* curvature, long long* count, long long* counters,
                                td_stream_t stream) {
  if (!query || !cell_start || !normal || !curvature || !count || !counters || N < 0 || M < 0 || C < 0 || C > M || !(tau > 0.0) ||
      !isfinite(tau) || !(radius > 0.0) || !(radius <= tau) || !(fabs(Q * radius - 0x1p18) <= 0x1p-32) || min_neighbours < 3 ||
      !(max_curvature >= 0.0) ||
      (M > 0 && !points) || (C > 0 && !cell_key))
    return TD_ERR_BAD_ARG;
  // Q is 2^18 / radius to rounding (two roundings of 2^-53 each leave Q radius within 2^-33 of 2^18; a NaN or an inf fails): only then
  // is |i_k| <= 2^18 + 1, which the conversions to int64 and the bound on M rest on
  if (M >= TD_NORMALS_MAX_POINTS) return TD_ERR_UNSUPPORTED;      // the integer sums could overflow
  if (N == 0) return TD_OK;
  td::NormalsArgs a;
  a.query = query; a.points = points; a.cell_key = cell_key; a.cell_start = cell_start;
  a.N = N; a.M = M; a.C = C;
  a.inv_cell = (1.0 - 0x1p-20) / tau;      // cloud_eval.inv_cell: the grid was built with the same two operations
  a.radius2 = radius * radius;
  a.Q = Q; a.max_curvature = max_curvature; a.min_neighbours = min_neighbours;
  a.normal = normal; a.curvature = curvature; a.count = count;
  a.counters = reinterpret_cast<unsigned long long*>(counters);
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::cloud_normals_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  return td::record_launch_error(hipGetLastError(), "td_cloud_normals");
}
