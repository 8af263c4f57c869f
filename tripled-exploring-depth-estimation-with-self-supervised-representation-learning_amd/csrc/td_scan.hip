// A batch of velodyne scans as the (voxel key, packed payload) pairs of td_cloud.hip (tripled_amd/cloud_eval.py):
//   td_scan_keys   points of S scans of mixed lengths -> camera frame -> (optional) view test -> world frame -> key, payload
// The pairs go through the unchanged torch.sort / td_cloud_heads / td_cloud_reduce_* / td_cloud_finish chain, so the lidar cloud is
// fused by the same integer sums as the predicted one: bit-identical from run to run, independent of the batch size.  Built with
// -ffp-contract=off: every float64 product and sum is rounded on its own, as the numpy statement (cloud_eval.scan_keys_numpy) rounds it.
#include <math.h>

#include "td_grid.h"
#include "td_pixel.h"

namespace td {

struct ScanKeyArgs {
  const float* points;         // [n,4] x, y, z, reflectance
  const long long* offsets;    // [S+1]
  const double* poses;         // [S,3,4] camera-to-world
  double tr[12];               // velodyne to camera, row-major 3x4
  double k[6];                 // rows 0 and 1 of K's 3x3 block
  long long n;
  int S, H, W;
  double min_depth, max_range, inv_voxel;
  long long* key;              // [n] (out)
  unsigned long long* payload; // [n] (out)
  unsigned long long* stats;   // [5] or NULL: += valid, point, depth, view, range
};

// The scan that owns point i: the last s with offsets[s] <= i, found in at most 32 halvings of [0, S]; -1 when no scan owns it
// (i in front of offsets[0], at or beyond offsets[s+1], or offsets that run backwards).  Every read of offsets is inside [0, S].
__device__ __forceinline__ int scan_of(const long long* __restrict__ offsets, int S, long long i) {
  int lo = 0, hi = S + 1;      // the first entry in [lo, hi) that is > i
  for (int it = 0; it < 32 && lo < hi; ++it) {
    const int mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  const int s = lo - 1;
  if (s < 0 || s >= S) return -1;
  return (offsets[s] <= i && i < offsets[s + 1]) ? s : -1;
}

template <bool VEC>
__global__ __launch_bounds__(TD_THREADS) void scan_keys_kernel(const ScanKeyArgs a) {
  __shared__ unsigned cnt[5];
  if (a.stats) counters_begin<5>(cnt);
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  int cause = -1;
  if (i < a.n) {
    float p[4];
    if (VEC) {
      const f4 v = *reinterpret_cast<const f4*>(a.points + i * 4);
      p[0] = v[0]; p[1] = v[1]; p[2] = v[2]; p[3] = v[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) p[j] = a.points[i * 4 + j];
    }
    long long kk = TD_KEY_INVALID;
    unsigned long long pp = 0;
    const int s = scan_of(a.offsets, a.S, i);
    cause = 0;
    if (s < 0 || !isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) {
      cause = 1;
    } else {
      const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
      const double cx = ((a.tr[0] * x + a.tr[1] * y) + a.tr[2] * z) + a.tr[3];
      const double cy = ((a.tr[4] * x + a.tr[5] * y) + a.tr[6] * z) + a.tr[7];
      const double cz = ((a.tr[8] * x + a.tr[9] * y) + a.tr[10] * z) + a.tr[11];
      if (!(cz >= a.min_depth && cz <= a.max_range)) {
        cause = 2;
      } else {
        if (a.H > 0) {
          const double u = ((a.k[0] * cx + a.k[1] * cy) + a.k[2] * cz) / cz;
          const double v = ((a.k[3] * cx + a.k[4] * cy) + a.k[5] * cz) / cz;
          if (!(u >= 0.0 && u <= (double)(a.W - 1) && v >= 0.0 && v <= (double)(a.H - 1))) cause = 3;      // a NaN fails
        }
        if (cause == 0) {
          double wx, wy, wz;
          camera_to_world(a.poses + (long long)s * 12, 1.0, cx, cy, cz, wx, wy, wz);      // 1.0 t is t exactly
          kk = voxel_key(wx * a.inv_voxel, wy * a.inv_voxel, wz * a.inv_voxel, pp);
          if (kk == TD_KEY_INVALID) {
            cause = 4;
          } else {
            double c = floor((double)p[3] * 255.0 + 0.5);
            c = c >= 0.0 ? (c <= 255.0 ? c : 255.0) : 0.0;      // a NaN reflectance is 0
            const unsigned long long grey = (unsigned long long)c;
            pp |= (grey << 30) | (grey << 38) | (grey << 46);
          }
        }
      }
    }
    a.key[i] = kk;
    a.payload[i] = pp;
  }
  if (a.stats) {
    if (cause >= 0) atomicAdd(&cnt[cause], 1u);      // LDS
    counters_end<5>(cnt, a.stats);
  }
}

}  // namespace td

extern "C" int td_scan_keys(const float* points, long long n, const long long* offsets, int S, const double* Tr, const double* poses,
                            const double* K, int H, int W, double min_depth, double max_range, double inv_voxel, long long* key,
                            unsigned long long* payload, long long* stats, td_stream_t stream) {
  if (!points || !offsets || !Tr || !poses || !key || !payload || n < 0 || S < 1 || H < 0 || W < 0 || (H > 0 && (!K || W < 1)) ||
      !(inv_voxel > 0.0) || !(min_depth <= max_range))
    return TD_ERR_BAD_ARG;
  if (n == 0) return TD_OK;
  td::ScanKeyArgs a;
  a.points = points; a.offsets = offsets; a.poses = poses;
  for (int k = 0; k < 12; ++k) a.tr[k] = Tr[k];
  for (int k = 0; k < 6; ++k) a.k[k] = H > 0 ? K[k] : 0.0;
  a.n = n; a.S = S; a.H = H; a.W = W;
  a.min_depth = min_depth; a.max_range = max_range; a.inv_voxel = inv_voxel;
  a.key = key; a.payload = payload; a.stats = reinterpret_cast<unsigned long long*>(stats);
  const unsigned blocks = td::blocks_1d(n);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  if (td::aligned_to(points, 16)) hipLaunchKernelGGL((td::scan_keys_kernel<true>), dim3(blocks), dim3(TD_THREADS), 0, s, a);
  else hipLaunchKernelGGL((td::scan_keys_kernel<false>), dim3(blocks), dim3(TD_THREADS), 0, s, a);
  return td::record_launch_error(hipGetLastError(), "td_scan_keys");
}
