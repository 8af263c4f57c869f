// What the cloud kernels share (td_cloud, td_tsdf, td_tsdf_cast, td_scan, td_views, td_nn, td_normals): the voxel / cell key, the pieces of the walk over a grid of
// cells sorted by it, and the camera-to-world transform.  Every user is built with -ffp-contract=off: each float64 product and sum below is
// rounded on its own, as the numpy statements (cloud.grid_keys_numpy, cloud_eval.walk_numpy) round it.
#pragma once
#include <math.h>

#include "td_common.h"

// key = ((ix + 2^20) << 42) | ((iy + 2^20) << 21) | (iz + 2^20): ascending key order is x major, then y, then z
#define TD_KEY_HALF 1048576                      // voxel and cell coordinates lie in [-2^20, 2^20)
#define TD_KEY_INVALID 0x7fffffffffffffffLL      // no voxel: the sort puts it last
#define TD_KEY_SHIFT_X 42
#define TD_KEY_SHIFT_Y 21

namespace td {

__device__ __forceinline__ long long key_pack(long long ix, long long iy, long long iz) {
  return ((ix + TD_KEY_HALF) << TD_KEY_SHIFT_X) | ((iy + TD_KEY_HALF) << TD_KEY_SHIFT_Y) | (iz + TD_KEY_HALF);
}

__device__ __forceinline__ bool key_in_range(double fx, double fy, double fz) {      // a NaN fails every comparison
  const double lo = -(double)TD_KEY_HALF, hi = (double)TD_KEY_HALF;
  return fx >= lo && fx < hi && fy >= lo && fy < hi && fz >= lo && fz < hi;
}

// Grid coordinates g = world inv_voxel -> the key of the voxel floor(g); TD_KEY_INVALID when a coordinate is out of range or the voxel
// is the one corner voxel whose key is the sentinel.  offset: the position inside the voxel, 10 bits per axis, the low 30 bits of a
// payload (the colours above them are the caller's); written only with a valid key.
__device__ __forceinline__ long long voxel_key(double gx, double gy, double gz, unsigned long long& offset) {
  const double fx = floor(gx), fy = floor(gy), fz = floor(gz);
  if (!key_in_range(fx, fy, fz)) return TD_KEY_INVALID;
  const long long key = key_pack((long long)fx, (long long)fy, (long long)fz);
  if (key == TD_KEY_INVALID) return key;
  int qx = (int)floor((gx - fx) * 1024.0), qy = (int)floor((gy - fy) * 1024.0), qz = (int)floor((gz - fz) * 1024.0);
  qx = qx > 1023 ? 1023 : qx;
  qy = qy > 1023 ? 1023 : qy;
  qz = qz > 1023 ? 1023 : qz;
  offset = (unsigned long long)qx | ((unsigned long long)qy << 10) | ((unsigned long long)qz << 20);
  return key;
}

// world_k = ((r_k0 x + r_k1 y) + r_k2 z) + scale t_k for the camera-to-world pose P = [r | t], row-major 3x4
__device__ __forceinline__ void camera_to_world(const double* __restrict__ P, double scale, double x, double y, double z, double& wx,
                                                double& wy, double& wz) {
  wx = ((P[0] * x + P[1] * y) + P[2] * z) + scale * P[3];
  wy = ((P[4] * x + P[5] * y) + P[6] * z) + scale * P[7];
  wz = ((P[8] * x + P[9] * y) + P[10] * z) + scale * P[11];
}

// A row of the TSDF map (td_tsdf, td_tsdf_cast): S = sum q - 2^20 w, the summed signed distance, an exact integer
#define TD_TSDF_ONE 1048576      // 2^20: the distance `trunc` as an integer
__device__ __forceinline__ long long tsdf_sum(const long long* __restrict__ r) {
  return (r[1] + 1024 * r[2] + (long long)TD_TSDF_ONE * r[3]) - (long long)TD_TSDF_ONE * r[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// A cloud sorted into a uniform grid of cells (cloud_eval.grid_hip): cell_key [C] ascending, cell_start [C+1], points in cell order.
// With inv_cell = (1 - 2^-20) / tau two points within tau lie in cells at most one apart on every axis, so the 27 cells around a
// query's hold every candidate.

// the query's cell; false for a query that is not finite or out of the key range (a NaN or an inf fails a comparison)
__device__ __forceinline__ bool grid_cell_of(double qx, double qy, double qz, double inv_cell, long long& ix, long long& iy,
                                             long long& iz) {
  const double fx = floor(qx * inv_cell), fy = floor(qy * inv_cell), fz = floor(qz * inv_cell);
  const bool valid = isfinite(qx) && isfinite(qy) && isfinite(qz) && key_in_range(fx, fy, fz);
  if (valid) { ix = (long long)fx; iy = (long long)fy; iz = (long long)fz; }
  return valid;
}

// the first c in [0, C] with cell_key[c] >= key; at most 64 halvings, every read inside [0, C)
__device__ __forceinline__ long long grid_lower_bound(const long long* __restrict__ cell_key, long long C, long long key) {
  long long lo = 0, hi = C;
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const long long mid = lo + ((hi - lo) >> 1);
    if (cell_key[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Row v of cell_start clamped into [0, M], whatever cell_start holds.  The walk both grid kernels write out over these pieces: z sits
// in the key's low bits, so the three z-neighbours of a (dx, dy) column are adjacent in key order: one lower bound per column (9, not
// 27), then at most three cells.  (Why the loop nest itself is not a shared template: DESIGN 23.)
__device__ __forceinline__ long long grid_row(long long v, long long M) { return v < 0 ? 0 : (v > M ? M : v); }

}  // namespace td
