// Truncated signed distance fusion of depth maps and poses (tripled_amd/tsdf.py):
//   td_tsdf_samples   pixels -> 4T+1 (voxel key, packed payload) pairs each: the voxels a pixel's ray meets inside the band around its
//                     surface, with the projective signed distance as an offset-binary integer in the payload's 30 offset bits
//   td_tsdf_surface   the key-sorted voxel map -> a point, a normal, a colour and a weight on every +x / +y / +z edge the averaged
//                     distance changes sign on
// Between the two runs the unchanged chain of td_cloud.hip (torch.sort, td_cloud_heads, cumsum, td_cloud_reduce_packed, merge): its
// sums are linear in the payload's fields, so sum v = sum q_x + 1024 sum q_y + 2^20 sum q_z.  Everything accumulated is an integer.
// The file is built with -ffp-contract=off: every float64 operation is rounded on its own, as the numpy statements (tsdf.samples_numpy,
// tsdf.surface_numpy) round it.  No kernel waits on another workgroup, there are no floating-point atomics.
#include <math.h>

#include "td_grid.h"
#include "td_pixel.h"

namespace td {

// ---------------------------------------------------------------------------------------------------------------------------
// samples

struct TsdfSampleArgs {
  const float* depth;          // [B,H,W]
  const uint8_t* color;        // [B,3,H,W]
  const double* poses;         // [B,3,4] camera-to-world
  const double* ik;            // [9] the 3x3 block of inv_K, row-major (device)
  const uint8_t* mask;         // [B,H,W] or NULL: 0 drops the pixel
  int B, H, W, T, stride, border;
  double depth_scale, pose_scale, voxel, inv_voxel, min_depth, max_range;
  float edge;
  long long* key;              // [4T+1][B*H*W] (out)
  unsigned long long* payload; // [4T+1][B*H*W] (out)
  unsigned long long* stats;   // [TD_TSDF_SAMPLE_STATS] or NULL
};

// td_pixel.h's run of VEC columns per thread and its causes 1 ... 5: what td_cloud_keys drops, then the mask.  Output is slot-major: the
// VEC pairs of one slot are one store, and a wave's stores of a slot are contiguous.
template <int VEC>
__global__ __launch_bounds__(TD_THREADS) void tsdf_samples_kernel(const TsdfSampleArgs a) {
  __shared__ unsigned cnt[TD_TSDF_SAMPLE_STATS];
  if (a.stats) counters_begin<TD_TSDF_SAMPLE_STATS>(cnt);
  const int T = a.T;
  const long long npix = (long long)a.B * a.H * a.W;
  unsigned local[TD_TSDF_SAMPLE_STATS];
#pragma unroll
  for (int k = 0; k < TD_TSDF_SAMPLE_STATS; ++k) local[k] = 0;
  PixelRun<VEC> r;
  if (pixel_run_load<VEC>(a, a.mask, r)) {
    const long long pix = r.pix;
    double P[12], ik[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)r.b * 12 + k];
#pragma unroll
    for (int k = 0; k < 9; ++k) ik[k] = a.ik[k];
    const double v = (double)r.y;
    bool ok[VEC];
    double r0[VEC], r1[VEC], r2[VEC], pz[VEC];
    unsigned long long rgb[VEC];
    long long prev[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      pixel_ray(ik, (double)(r.x0 + j), v, r0[j], r1[j], r2[j]);
      pz[j] = r.ds[j] * r2[j];
      ok[j] = r.cause[j] == 0;
      rgb[j] = pixel_rgb(r, j);
      prev[j] = TD_KEY_INVALID;
      local[r.cause[j]] += 1;
    }
    const double half = a.voxel * 0.5;
    const double trunc = (double)T * a.voxel;
    const double scale = (double)TD_TSDF_ONE / trunc;
    for (int s = -2 * T; s <= 2 * T; ++s) {
      long long key[VEC];
      unsigned long long pay[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        long long kk = TD_KEY_INVALID;
        unsigned long long pp = 0;
        if (ok[j]) {
          const double dz = pz[j] + (double)s * half;
          const double f = dz / r2[j];
          double wx, wy, wz;
          camera_to_world(P, a.pose_scale, r0[j] * f, r1[j] * f, r2[j] * f, wx, wy, wz);
          const double gx = wx * a.inv_voxel, gy = wy * a.inv_voxel, gz = wz * a.inv_voxel;
          unsigned long long offset = 0;
          const long long k = voxel_key(gx, gy, gz, offset);
          if (k == TD_KEY_INVALID) {
            local[9] += 1;
          } else if (s > -2 * T && k == prev[j]) {
            local[7] += 1;
          } else {
            const double ex = (floor(gx) + 0.5) * a.voxel - a.pose_scale * P[3];
            const double ey = (floor(gy) + 0.5) * a.voxel - a.pose_scale * P[7];
            const double ez = (floor(gz) + 0.5) * a.voxel - a.pose_scale * P[11];
            const double zc = (P[2] * ex + P[6] * ey) + P[10] * ez;
            const double sdf = pz[j] - zc;
            if (!(fabs(sdf) <= trunc)) {
              local[8] += 1;
            } else {
              long long q = (long long)rint(sdf * scale);
              q = q > TD_TSDF_ONE ? TD_TSDF_ONE : (q < -TD_TSDF_ONE ? -TD_TSDF_ONE : q);
              kk = k;
              pp = (unsigned long long)(q + TD_TSDF_ONE) | rgb[j];
              local[6] += 1;
            }
          }
          prev[j] = k;
        }
        key[j] = kk;
        pay[j] = pp;
      }
      const long long at = (long long)(s + 2 * T) * npix + pix;
      store_run<VEC>(a.key + at, key);
      store_run<VEC>(a.payload + at, pay);
    }
  }
  if (a.stats) counters_end<TD_TSDF_SAMPLE_STATS>(cnt, local, a.stats);
}

// ---------------------------------------------------------------------------------------------------------------------------
// surface

// The index of the neighbour of voxel `idx` (key `key`) one step along `axis` (0 x, 1 y, 2 z) in direction dir = +-1, or -1.  The
// coordinate field is tested first: the last coordinate has no + neighbour and the first no - neighbour, and nothing is ever carried
// into the next field.  z sits in the low bits, so a z neighbour is adjacent in key order.
__device__ __forceinline__ long long tsdf_neighbour(const long long* __restrict__ keys, long long V, long long idx, long long key, int axis,
                                                    int dir) {
  const int shift = axis == 0 ? TD_KEY_SHIFT_X : (axis == 1 ? TD_KEY_SHIFT_Y : 0);
  const long long mask = 2 * TD_KEY_HALF - 1;
  const long long field = (key >> shift) & mask;
  if (dir > 0 ? field == mask : field == 0) return -1;
  const long long kb = dir > 0 ? key + (1LL << shift) : key - (1LL << shift);
  if (kb == TD_KEY_INVALID) return -1;
  long long j;
  if (axis == 2) {
    j = idx + dir;
    if (j < 0 || j >= V) return -1;
  } else {
    j = grid_lower_bound(keys, V, kb);
    if (j >= V) return -1;
  }
  return keys[j] == kb ? j : -1;
}

// The gradient of D = S / w at voxel idx, in voxels: central where both neighbours on an axis qualify, one-sided where one does, else 0.
__device__ __forceinline__ void tsdf_gradient(const long long* __restrict__ keys, const long long* __restrict__ sums, long long V,
                                              long long idx, long long min_weight, double* g) {
  const long long key = keys[idx];
  const double Dv = (double)tsdf_sum(sums + idx * 7) / (double)sums[idx * 7];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
    const long long p = tsdf_neighbour(keys, V, idx, key, axis, 1), m = tsdf_neighbour(keys, V, idx, key, axis, -1);
    const bool hp = p >= 0 && sums[(p < 0 ? 0 : p) * 7] >= min_weight, hm = m >= 0 && sums[(m < 0 ? 0 : m) * 7] >= min_weight;
    double Dp = 0.0, Dm = 0.0;
    if (hp) Dp = (double)tsdf_sum(sums + p * 7) / (double)sums[p * 7];
    if (hm) Dm = (double)tsdf_sum(sums + m * 7) / (double)sums[m * 7];
    g[axis] = hp && hm ? (Dp - Dm) / 2.0 : (hp ? Dp - Dv : (hm ? Dv - Dm : 0.0));
  }
}

// One thread per voxel a; its three + edges go to the slots [a][axis].  Only mask is written for an edge without a crossing.
__global__ __launch_bounds__(TD_THREADS) void tsdf_surface_kernel(const long long* __restrict__ keys, const long long* __restrict__ sums,
                                                                  long long V, double voxel, long long min_weight,
                                                                  float* __restrict__ xyz, float* __restrict__ normal,
                                                                  uint8_t* __restrict__ rgb, int* __restrict__ weight,
                                                                  uint8_t* __restrict__ mask, unsigned long long* __restrict__ stats) {
  __shared__ unsigned cnt[TD_TSDF_SURFACE_STATS];
  if (stats) counters_begin<TD_TSDF_SURFACE_STATS>(cnt);
  const long long a = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  unsigned local[TD_TSDF_SURFACE_STATS] = {0, 0, 0, 0, 0};
  if (a < V) {
    const long long key = keys[a];
    const long long* ra = sums + a * 7;
    const long long wa = ra[0];
    const bool a_ok = wa >= min_weight;
    if (!a_ok) local[0] += 1;
    const long long Sa = tsdf_sum(ra);
    const long long fmask = 2 * TD_KEY_HALF - 1;
    const double ia[3] = {(double)(((key >> TD_KEY_SHIFT_X) & fmask) - TD_KEY_HALF), (double)(((key >> TD_KEY_SHIFT_Y) & fmask) - TD_KEY_HALF),
                          (double)((key & fmask) - TD_KEY_HALF)};
    bool have_ga = false;
    double ga[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
      const long long b = a_ok ? tsdf_neighbour(keys, V, a, key, axis, 1) : -1;
      bool cross = false;
      if (b >= 0) {
        const long long* rb = sums + b * 7;
        const long long wb = rb[0], Sb = tsdf_sum(rb);
        cross = wb >= min_weight && ((Sa >= 0) != (Sb >= 0));
        if (cross) {
          const double Da = (double)Sa / (double)wa, Db = (double)Sb / (double)wb;
          const double t = Da / (Da - Db);
          if (!have_ga) {
            tsdf_gradient(keys, sums, V, a, min_weight, ga);
            have_ga = true;
          }
          double gb[3];
          tsdf_gradient(keys, sums, V, b, min_weight, gb);
          const double g0 = (1.0 - t) * ga[0] + t * gb[0], g1 = (1.0 - t) * ga[1] + t * gb[1], g2 = (1.0 - t) * ga[2] + t * gb[2];
          const double norm = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
          const long long o = (a * 3 + axis) * 3;
          const bool has_normal = norm > 0.0;
          normal[o] = has_normal ? (float)(g0 / norm) : 0.f;
          normal[o + 1] = has_normal ? (float)(g1 / norm) : 0.f;
          normal[o + 2] = has_normal ? (float)(g2 / norm) : 0.f;
          if (!has_normal) local[4] += 1;
#pragma unroll
          for (int k = 0; k < 3; ++k) xyz[o + k] = (float)(k == axis ? ((ia[k] + 0.5) + t) * voxel : (ia[k] + 0.5) * voxel);
          const long long* rc = t < 0.5 ? ra : rb;
          const long long n = rc[0];
#pragma unroll
          for (int k = 0; k < 3; ++k) rgb[o + k] = n > 0 ? (uint8_t)((2 * rc[4 + k] + n) / (2 * n)) : (uint8_t)0;
          const long long wmin = wa < wb ? wa : wb;
          weight[a * 3 + axis] = wmin > 0x7fffffffLL ? 0x7fffffff : (int)wmin;
          local[1 + axis] += 1;
        }
      }
      mask[a * 3 + axis] = cross ? 1 : 0;
    }
  }
  if (stats) counters_end<TD_TSDF_SURFACE_STATS>(cnt, local, stats);
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_tsdf_samples(const float* depth, const uint8_t* color, const double* poses, const double* inv_K, const uint8_t* mask,
                               int B, int H, int W, int T, double depth_scale, double pose_scale, double voxel, double inv_voxel,
                               int stride, int border, double min_depth, double max_range, float edge, long long* key,
                               unsigned long long* payload, long long* stats, td_stream_t stream) {
  if (!depth || !color || !poses || !inv_K || !key || !payload || B < 0 || H <= 0 || W <= 0 || T < 1 || T > TD_TSDF_MAX_T ||
      stride < 1 || border < 0 || !(voxel > 0.0) || !(inv_voxel > 0.0) || !(edge >= 0.f))
    return TD_ERR_BAD_ARG;
  if (B == 0) return TD_OK;
  td::TsdfSampleArgs a;
  a.depth = depth; a.color = color; a.poses = poses; a.ik = inv_K; a.mask = mask;
  a.B = B; a.H = H; a.W = W; a.T = T; a.stride = stride; a.border = border;
  a.depth_scale = depth_scale; a.pose_scale = pose_scale; a.voxel = voxel; a.inv_voxel = inv_voxel;
  a.min_depth = min_depth; a.max_range = max_range;
  a.edge = edge; a.key = key; a.payload = payload; a.stats = reinterpret_cast<unsigned long long*>(stats);
  // a slot's plane starts B H W elements on, a multiple of the run: the alignment of key and payload holds for every slot
  return td::launch_pixel_runs(td::tsdf_samples_kernel<4>, td::tsdf_samples_kernel<2>, td::tsdf_samples_kernel<1>, a, mask, stream,
                               "td_tsdf_samples");
}

extern "C" int td_tsdf_surface(const long long* keys, const long long* sums, long long V, double voxel, long long min_weight, float* xyz,
                               float* normal, uint8_t* rgb, int* weight, uint8_t* mask, long long* stats, td_stream_t stream) {
  if (!keys || !sums || !xyz || !normal || !rgb || !weight || !mask || V < 0 || !(voxel > 0.0) || min_weight < 1) return TD_ERR_BAD_ARG;
  if (V == 0) return TD_OK;
  const unsigned blocks = td::blocks_1d(V);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::tsdf_surface_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, keys, sums, V, voxel, min_weight,
                     xyz, normal, rgb, weight, mask, reinterpret_cast<unsigned long long*>(stats));
  return td::record_launch_error(hipGetLastError(), "td_tsdf_surface");
}
