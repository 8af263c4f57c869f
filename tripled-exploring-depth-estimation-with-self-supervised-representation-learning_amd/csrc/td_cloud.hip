// Fusion of a sequence's depth maps and camera poses into a voxel-averaged coloured point cloud (tripled_amd/cloud.py):
//   td_cloud_keys            pixels -> (voxel key, packed payload), float64 arithmetic, plain coalesced stores
//   td_cloud_heads           sorted keys -> 1 where a voxel's run starts
//   td_cloud_reduce_packed   segmented integer sum of the sorted points into voxel rows (gather through the sort's permutation)
//   td_cloud_reduce_rows     the same body over already-summed rows: merges a chunk's voxels into the running map
//   td_cloud_finish          voxel sums -> xyz, rgb, count, keep
// Store, sort (torch.sort), then sum per destination: no hash table, no kernel waits on another workgroup.  Everything that is
// accumulated is an integer, so the result does not depend on the order in which points or partial sums arrive: two runs, and two
// ways of cutting a sequence into batches, return the same bits.  The file is built with -ffp-contract=off: every float64 product
// and sum of td_cloud_keys is rounded on its own, as the numpy statement (cloud.keys_numpy) rounds it.
#include <math.h>

#include "td_grid.h"
#include "td_pixel.h"

namespace td {

#define TD_CLOUD_ITERS 8           // a wave's stretch of the sorted array: 8 x 64 elements
#define TD_CLOUD_STRETCH (64 * TD_CLOUD_ITERS)

// ---------------------------------------------------------------------------------------------------------------------------
// keys

struct CloudKeyArgs {
  const float* depth;          // [B,H,W]
  const uint8_t* color;        // [B,3,H,W]
  const double* poses;         // [B,3,4] camera-to-world
  double ik[9];                // the 3x3 block of inv_K, row-major
  int B, H, W, stride, border;
  double depth_scale, pose_scale, inv_voxel, min_depth, max_range;
  float edge;
  long long* key;              // [B*H*W] (out)
  unsigned long long* payload; // [B*H*W] (out)
  unsigned long long* stats;   // [6] or NULL: += valid, off-lattice, border, depth, edge, range
};

// td_pixel.h's run of VEC columns per thread and its causes 1 ... 4; cause 5 here is a voxel out of the key's range.
template <int VEC>
__global__ __launch_bounds__(TD_THREADS) void cloud_keys_kernel(const CloudKeyArgs a) {
  __shared__ unsigned cnt[6];
  if (a.stats) counters_begin<6>(cnt);
  unsigned local[6] = {0, 0, 0, 0, 0, 0};
  PixelRun<VEC> r;
  if (pixel_run_load<VEC>(a, nullptr, r)) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)r.b * 12 + k];
    const double v = (double)r.y;
    long long key[VEC];
    unsigned long long pay[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      int cause = r.cause[j];
      long long kk = TD_KEY_INVALID;
      unsigned long long pp = 0;
      if (cause == 0) {
        double r0, r1, r2;
        pixel_ray(a.ik, (double)(r.x0 + j), v, r0, r1, r2);
        const double ds = r.ds[j];
        const double px = ds * r0, py = ds * r1, pz = ds * r2;
        double wx, wy, wz;
        camera_to_world(P, a.pose_scale, px, py, pz, wx, wy, wz);
        kk = voxel_key(wx * a.inv_voxel, wy * a.inv_voxel, wz * a.inv_voxel, pp);
        if (kk == TD_KEY_INVALID) cause = 5;
        else pp |= pixel_rgb(r, j);
      }
      key[j] = kk;
      pay[j] = pp;
      local[cause] += 1;
    }
    store_run<VEC>(a.key + r.pix, key);
    store_run<VEC>(a.payload + r.pix, pay);
  }
  if (a.stats) counters_end<6>(cnt, local, a.stats);
}

// ---------------------------------------------------------------------------------------------------------------------------
// heads

__global__ __launch_bounds__(TD_THREADS) void cloud_heads_kernel(const long long* __restrict__ keys, long long N,
                                                                 int* __restrict__ flags) {
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i >= N) return;
  const long long k = keys[i];
  flags[i] = (k != TD_KEY_INVALID && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// segmented sum

// One row of a voxel: count, sum qx, sum qy, sum qz, sum r, sum g, sum b.
__device__ __forceinline__ void unpack_payload(unsigned long long p, long long* v) {
  v[0] = 1;
  v[1] = (long long)(p & 1023u);
  v[2] = (long long)((p >> 10) & 1023u);
  v[3] = (long long)((p >> 20) & 1023u);
  v[4] = (long long)((p >> 30) & 255u);
  v[5] = (long long)((p >> 38) & 255u);
  v[6] = (long long)((p >> 46) & 255u);
}

__device__ __forceinline__ void put_row(long long* __restrict__ sums, long long s, long long V, const long long* v, bool atomic) {
  if (s < 1 || s > V) return;      // inconsistent seg / V: never write outside the rows
  long long* dst = sums + (s - 1) * 7;
  if (atomic) {
#pragma unroll
    for (int j = 0; j < 7; ++j) atomicAdd(reinterpret_cast<unsigned long long*>(dst + j), (unsigned long long)v[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 7; ++j) dst[j] = v[j];
  }
}

// A wave owns TD_CLOUD_STRETCH consecutive elements of the sorted array and walks them 64 at a time.  Within 64 elements a
// segmented inclusive scan (the segment number is the key of the scan: the array is sorted, so equal numbers are adjacent) leaves a
// run's total in its last lane; a run that is still open at lane 63 is carried, wave-uniformly, into the next 64.  A run whose first
// and last element both lie in the stretch is written with plain stores by its last lane.  Only the stretch's first run (when it
// began in an earlier stretch) and its last (when it goes on) are added with integer atomics into the zero-initialised rows.
template <bool PACKED>
__global__ __launch_bounds__(TD_THREADS) void cloud_reduce_kernel(const long long* __restrict__ keys, const long long* __restrict__ seg,
                                                                  const long long* __restrict__ perm, const void* __restrict__ src,
                                                                  long long n_src, long long N, long long V,
                                                                  long long* __restrict__ out_keys, long long* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (TD_THREADS / 64) + (threadIdx.x >> 6);
  const long long base = wave * TD_CLOUD_STRETCH;
  if (base >= N || keys[base] == TD_KEY_INVALID) return;      // wave-uniform: invalid keys are sorted last
  const long long end = base + TD_CLOUD_STRETCH < N ? base + TD_CLOUD_STRETCH : N;
  const long long first_s = seg[base];
  const bool first_open = base > 0 && seg[base - 1] == first_s;      // the first run began before this stretch
  bool carry_on = false;
  long long carry_s = 0, carry[7] = {0, 0, 0, 0, 0, 0, 0};
  for (long long at = base; at < end; at += 64) {
    const long long idx = at + lane;
    const long long k = idx < end ? keys[idx] : TD_KEY_INVALID;
    const bool valid = k != TD_KEY_INVALID;
    const long long s = valid ? seg[idx] : -1;
    long long v[7] = {0, 0, 0, 0, 0, 0, 0};
    if (valid) {
      const long long at_src = perm ? perm[idx] : idx;
      if (at_src >= 0 && at_src < n_src) {
        if (PACKED) {
          unpack_payload(static_cast<const unsigned long long*>(src)[at_src], v);
        } else {
          const long long* r = static_cast<const long long*>(src) + at_src * 7;
#pragma unroll
          for (int j = 0; j < 7; ++j) v[j] = r[j];
        }
      }
      if ((idx == 0 || seg[idx - 1] != s) && s >= 1 && s <= V) out_keys[s - 1] = k;      // the run's head names the voxel
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long so = __shfl_up(s, off, 64);
      long long t[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) t[j] = __shfl_up(v[j], off, 64);
      if (lane >= off && so == s) {
#pragma unroll
        for (int j = 0; j < 7; ++j) v[j] += t[j];
      }
    }
    const long long s0 = __shfl(s, 0, 64);
    if (carry_on) {
      if (s0 != carry_s) {      // the carried run ended on the last element of the previous 64: lanes 0 ... 6 write a column each
        long long val = carry[0];
#pragma unroll
        for (int j = 1; j < 7; ++j) val = lane == j ? carry[j] : val;
        if (lane < 7 && carry_s >= 1 && carry_s <= V) {
          long long* dst = sums + (carry_s - 1) * 7 + lane;
          if (carry_s == first_s && first_open) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)val);
          else *dst = val;
        }
      } else if (s == carry_s) {
#pragma unroll
        for (int j = 0; j < 7; ++j) v[j] += carry[j];
      }
    }
    const long long s_next = __shfl_down(s, 1, 64);
    if (valid && lane < 63 && s_next != s) put_row(sums, s, V, v, s == first_s && first_open);
    carry_on = __shfl((int)valid, 63, 64) != 0;
    if (!carry_on) break;      // lane 63 is invalid: so is everything after it
    carry_s = __shfl(s, 63, 64);
#pragma unroll
    for (int j = 0; j < 7; ++j) carry[j] = __shfl(v[j], 63, 64);
  }
  if (carry_on) {
    const bool closed = end >= N || keys[end] == TD_KEY_INVALID || seg[end] != carry_s;
    const bool atomic = !closed || (carry_s == first_s && first_open);
    long long val = carry[0];
#pragma unroll
    for (int j = 1; j < 7; ++j) val = lane == j ? carry[j] : val;
    if (lane < 7 && carry_s >= 1 && carry_s <= V) {
      long long* dst = sums + (carry_s - 1) * 7 + lane;
      if (atomic) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)val);
      else *dst = val;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// finish

__global__ __launch_bounds__(TD_THREADS) void cloud_finish_kernel(const long long* __restrict__ keys, const long long* __restrict__ sums,
                                                                  long long V, double voxel, long long min_count,
                                                                  float* __restrict__ xyz, uint8_t* __restrict__ rgb,
                                                                  int* __restrict__ count, uint8_t* __restrict__ keep) {
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (i >= V) return;
  const long long k = keys[i];
  const long long* s = sums + i * 7;
  const long long n = s[0];
  const long long mask = 2 * TD_KEY_HALF - 1;
  const long long c[3] = {((k >> TD_KEY_SHIFT_X) & mask) - TD_KEY_HALF, ((k >> TD_KEY_SHIFT_Y) & mask) - TD_KEY_HALF, (k & mask) - TD_KEY_HALF};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    xyz[i * 3 + d] = (float)(((double)c[d] + ((double)s[1 + d] / (double)n + 0.5) / 1024.0) * voxel);
    rgb[i * 3 + d] = n > 0 ? (uint8_t)((2 * s[4 + d] + n) / (2 * n)) : (uint8_t)0;
  }
  count[i] = n > 0x7fffffffLL ? 0x7fffffff : (int)n;
  keep[i] = n >= min_count ? 1 : 0;
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_cloud_keys(const float* depth, const uint8_t* color, const double* poses, const double* inv_K, int B, int H, int W,
                             double depth_scale, double pose_scale, double inv_voxel, int stride, int border, double min_depth,
                             double max_range, float edge, long long* key, unsigned long long* payload, long long* stats,
                             td_stream_t stream) {
  if (!depth || !color || !poses || !inv_K || !key || !payload || B < 0 || H <= 0 || W <= 0 || stride < 1 || border < 0 ||
      !(inv_voxel > 0.0) || !(edge >= 0.f))
    return TD_ERR_BAD_ARG;
  if (B == 0) return TD_OK;
  td::CloudKeyArgs a;
  a.depth = depth; a.color = color; a.poses = poses;
  for (int k = 0; k < 9; ++k) a.ik[k] = inv_K[k];
  a.B = B; a.H = H; a.W = W; a.stride = stride; a.border = border;
  a.depth_scale = depth_scale; a.pose_scale = pose_scale; a.inv_voxel = inv_voxel; a.min_depth = min_depth; a.max_range = max_range;
  a.edge = edge; a.key = key; a.payload = payload; a.stats = reinterpret_cast<unsigned long long*>(stats);
  return td::launch_pixel_runs(td::cloud_keys_kernel<4>, td::cloud_keys_kernel<2>, td::cloud_keys_kernel<1>, a, nullptr, stream, "td_cloud_keys");
}

extern "C" int td_cloud_heads(const long long* keys, long long N, int* flags, td_stream_t stream) {
  if (!keys || !flags || N < 0) return TD_ERR_BAD_ARG;
  if (N == 0) return TD_OK;
  const unsigned blocks = td::blocks_1d(N);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::cloud_heads_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, keys, N, flags);
  return td::record_launch_error(hipGetLastError(), "td_cloud_heads");
}

template <bool PACKED>
static int cloud_reduce(const long long* keys, const long long* seg, const long long* perm, const void* src, long long n_src,
                        long long N, long long V, long long* out_keys, long long* sums, td_stream_t stream, const char* what) {
  if (!keys || !seg || !src || !out_keys || !sums || N < 0 || V < 0 || n_src < 0 || V > N) return TD_ERR_BAD_ARG;
  if (N == 0 || V == 0) return TD_OK;
  const long long waves = (N + TD_CLOUD_STRETCH - 1) / TD_CLOUD_STRETCH;
  const unsigned blocks = td::blocks_1d(waves * 64);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((td::cloud_reduce_kernel<PACKED>), dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, keys, seg,
                     perm, src, n_src, N, V, out_keys, sums);
  return td::record_launch_error(hipGetLastError(), what);
}

extern "C" int td_cloud_reduce_packed(const long long* keys, const long long* seg, const long long* perm,
                                      const unsigned long long* payload, long long n_src, long long N, long long V,
                                      long long* out_keys, long long* sums, td_stream_t stream) {
  return cloud_reduce<true>(keys, seg, perm, payload, n_src, N, V, out_keys, sums, stream, "td_cloud_reduce_packed");
}

extern "C" int td_cloud_reduce_rows(const long long* keys, const long long* seg, const long long* perm, const long long* rows,
                                    long long n_src, long long N, long long V, long long* out_keys, long long* sums,
                                    td_stream_t stream) {
  return cloud_reduce<false>(keys, seg, perm, rows, n_src, N, V, out_keys, sums, stream, "td_cloud_reduce_rows");
}

extern "C" int td_cloud_finish(const long long* keys, const long long* sums, long long V, double voxel, long long min_count, float* xyz,
                               uint8_t* rgb, int* count, uint8_t* keep, td_stream_t stream) {
  if (!keys || !sums || !xyz || !rgb || !count || !keep || V < 0 || !(voxel > 0.0)) return TD_ERR_BAD_ARG;
  if (V == 0) return TD_OK;
  const unsigned blocks = td::blocks_1d(V);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(td::cloud_finish_kernel, dim3(blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, keys, sums, V, voxel,
                     min_count, xyz, rgb, count, keep);
  return td::record_launch_error(hipGetLastError(), "td_cloud_finish");
}
