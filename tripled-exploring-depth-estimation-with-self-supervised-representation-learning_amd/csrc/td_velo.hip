// KITTI ground-truth depth maps from velodyne scans (tripled_amd/velodyne.py): the reference's generate_depth_map,
// mono/datasets/kitti_utils.py:50-102, for a batch of frames of different sizes.
//   clear     one fill of the four index tables (all ones = "nobody") and one of the stats rows (zero)
//   scatter   per point: project in float64, then four 64-bit integer atomic minima: the last point of its pixel, the first and the
//             last point of its duplicate group, the smallest depth of the group
//   resolve   per pixel of the padded [B,Hmax,Wmax] map: the depth of the pixel's last point, replaced by the group's minimum when the
//             group has more than one point and its first point lies on this pixel; negative -> 0; float32
// Every table entry is a minimum of integers, so the result does not depend on the order in which points arrive: two runs return the
// same bits, and they equal the numpy statement (velodyne.depth_map_numpy).  A maximum of point indices is kept as the minimum of
// the complements of index + 1 (the complement of index 0 would be the fill value), and a minimum of doubles as the minimum of an
// order-preserving map of their bits, so that one kind of atomic and one fill value serve all four tables.  The resolve pass projects
// the winning point again instead of reading a stored depth: the same statements compiled once give the same bits, and a table of
// doubles written by "the last point" would need a second scatter pass.  No kernel waits on another workgroup; there are no
// floating-point atomics.  The file is built with -ffp-contract=off: every float64 product and sum is rounded on its own, as the
// statement rounds it.
#include <math.h>

#include "td_common.h"

namespace td {

#define TD_VELO_NONE 0xffffffffffffffffULL
#define TD_VELO_SIGN 0x8000000000000000ULL

struct VeloArgs {
  const float* points;             // [Ntot,4]
  const long long* offsets;        // [B+1]
  const double* P;                 // [B,3,4]
  const int* sizes;                // [B,2] = (H, W)
  int B, Hmax, Wmax, vel_depth;
  unsigned long long* last;        // [B, Hmax Wmax]          ~(last point of the pixel + 1)
  unsigned long long* gfirst;      // [B, Hmax (Wmax-1) + 1]  (first point of the group) << 1 | (that point's column is 0)
  unsigned long long* glast;       // [B, Hmax (Wmax-1) + 1]  ~(last point of the group + 1)
  unsigned long long* gmin;        // [B, Hmax (Wmax-1) + 1]  ordered bits of the group's smallest depth
  float* gt;                       // [B,Hmax,Wmax] (out)
  unsigned long long* stats;       // [B,6] (out): points, behind, outside, valid, pixels hit, pixels clamped
};

// doubles -> unsigned integers with the same order (negative values included; -0.0 sorts below +0.0)
__device__ __forceinline__ unsigned long long ordered_bits(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b & TD_VELO_SIGN) ? ~b : (b | TD_VELO_SIGN);
}

__device__ __forceinline__ double from_ordered_bits(unsigned long long k) {
  const unsigned long long b = (k & TD_VELO_SIGN) ? (k & ~TD_VELO_SIGN) : ~k;
  return __longlong_as_double((long long)b);
}

__device__ __forceinline__ double row_dot(const double* __restrict__ p, double x, double y, double z) {
  return ((p[0] * x + p[1] * y) + p[2] * z) + p[3];
}

// (x, y, z) of point i; VEC: one 16-byte load (the base is 16-byte aligned), else three dword loads
template <bool VEC>
__device__ __forceinline__ void load_point(const float* __restrict__ pts, long long i, float& x, float& y, float& z) {
  if (VEC) {
    const f4 v = *reinterpret_cast<const f4*>(pts + i * 4);
    x = v[0]; y = v[1]; z = v[2];
  } else {
    x = pts[i * 4]; y = pts[i * 4 + 1]; z = pts[i * 4 + 2];
  }
}

struct VeloFrame {
  int H, W;
  long long first, n;
  bool ok;
};

__device__ __forceinline__ VeloFrame velo_frame(const VeloArgs& a, int b) {
  VeloFrame f;
  f.H = a.sizes[2 * b];
  f.W = a.sizes[2 * b + 1];
  f.first = a.offsets[b];
  f.n = a.offsets[b + 1] - f.first;
  f.ok = f.H >= 1 && f.H <= a.Hmax && f.W >= 2 && f.W <= a.Wmax && f.first >= 0 && f.n >= 0;
  return f;
}

// grid (blocks per frame, B): the block's threads stride through frame blockIdx.y's points.  The launch does not depend on the number
// of points, which only the device knows (offsets).
template <bool VEC>
__global__ __launch_bounds__(TD_THREADS) void velo_scatter_kernel(const VeloArgs a) {
  __shared__ unsigned cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const VeloFrame f = velo_frame(a, b);
  unsigned long long* st = a.stats + (long long)b * 6;
  if (!f.ok) {      // a size the tables cannot hold, or offsets that run backwards: the row says so, the map is zero
    if (blockIdx.x == 0 && threadIdx.x < 6) st[threadIdx.x] = TD_VELO_NONE;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = (unsigned long long)f.n;
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.P[(long long)b * 12 + k];
  const long long plane = (long long)a.Hmax * a.Wmax, groups = (long long)a.Hmax * (a.Wmax - 1) + 1;
  unsigned long long* last = a.last + (long long)b * plane;
  unsigned long long* gfirst = a.gfirst + (long long)b * groups;
  unsigned long long* glast = a.glast + (long long)b * groups;
  unsigned long long* gmin = a.gmin + (long long)b * groups;
  const float* pts = a.points + f.first * 4;
  const double Wd = (double)f.W, Hd = (double)f.H;
  unsigned local[3] = {0, 0, 0};      // behind, outside, valid
  for (long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x; i < f.n; i += (long long)gridDim.x * TD_THREADS) {
    float xf, yf, zf;
    load_point<VEC>(pts, i, xf, yf, zf);
    if (xf < 0.f) { local[0] += 1; continue; }
    if (!(xf >= 0.f)) { local[1] += 1; continue; }      // NaN
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double r0 = row_dot(P, x, y, z), r1 = row_dot(P + 4, x, y, z), r2 = row_dot(P + 8, x, y, z);
    const double u = rint(r0 / r2) - 1.0, v = rint(r1 / r2) - 1.0;
    if (!(u >= 0.0 && u < Wd && v >= 0.0 && v < Hd)) { local[1] += 1; continue; }      // a NaN fails every comparison
    local[2] += 1;
    const int ui = (int)u, vi = (int)v;
    const double d = a.vel_depth ? x : r2;
    const long long pix = (long long)vi * f.W + ui;
    const long long g = (long long)vi * (f.W - 1) + ui;      // the reference's index + 1: pixel (0,0) is entry 0
    const unsigned long long idx = (unsigned long long)i;
    atomicMin(last + pix, ~(idx + 1));
    atomicMin(gfirst + g, (idx << 1) | (ui == 0 ? 1ULL : 0ULL));
    atomicMin(glast + g, ~(idx + 1));
    atomicMin(gmin + g, ordered_bits(d));
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (local[k]) atomicAdd(&cnt[k], local[k]);      // LDS
  __syncthreads();
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(st + 1 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// grid (blocks per padded plane, B): one thread per pixel of gt[b]
template <bool VEC>
__global__ __launch_bounds__(TD_THREADS) void velo_resolve_kernel(const VeloArgs a) {
  __shared__ unsigned cnt[2];
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const VeloFrame f = velo_frame(a, b);
  const long long plane = (long long)a.Hmax * a.Wmax, groups = (long long)a.Hmax * (a.Wmax - 1) + 1;
  const long long at = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  bool hit = false, clamped = false;
  if (at < plane) {
    const unsigned at32 = (unsigned)at;      // a plane holds fewer than 2^31 pixels (td_velo_depth_workspace_bytes)
    const int yy = (int)(at32 / (unsigned)a.Wmax), xx = (int)(at32 - (unsigned)yy * (unsigned)a.Wmax);
    double d = 0.0;
    if (f.ok && yy < f.H && xx < f.W) {
      const unsigned long long l = a.last[(long long)b * plane + (long long)yy * f.W + xx];
      if (l != TD_VELO_NONE && ~l - 1 < (unsigned long long)f.n) {
        hit = true;
        const long long g = (long long)b * groups + (long long)yy * (f.W - 1) + xx;
        const unsigned long long gf = a.gfirst[g];
        if (gf != TD_VELO_NONE && (gf >> 1) != ~a.glast[g] - 1 && (gf & 1ULL) == (xx == 0 ? 1ULL : 0ULL)) {
          d = from_ordered_bits(a.gmin[g]);
        } else {
          float xf, yf, zf;
          load_point<VEC>(a.points + f.first * 4, (long long)(~l - 1), xf, yf, zf);
          d = a.vel_depth ? (double)xf : row_dot(a.P + (long long)b * 12 + 8, (double)xf, (double)yf, (double)zf);
        }
        if (d < 0.0) { d = 0.0; clamped = true; }
      }
    }
    a.gt[(long long)b * plane + at] = (float)d;
  }
  if (hit) atomicAdd(&cnt[0], 1u);      // LDS
  if (clamped) atomicAdd(&cnt[1], 1u);
  __syncthreads();
  if (f.ok && threadIdx.x < 2 && cnt[threadIdx.x]) atomicAdd(a.stats + (long long)b * 6 + 4 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

static inline long long velo_entries(long long B, long long Hmax, long long Wmax) {
  return B * (Hmax * Wmax + 3 * (Hmax * (Wmax - 1) + 1));
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" long long td_velo_depth_workspace_bytes(int B, int Hmax, int Wmax) {
  if (B <= 0 || B > 65535 || Hmax < 1 || Wmax < 2 || (long long)Hmax * Wmax > 0x7fffffffLL) return 0;
  return td::velo_entries(B, Hmax, Wmax) * 8;
}

extern "C" int td_velo_depth(const float* points, const long long* offsets, int B, const double* P, const int* sizes, int Hmax,
                             int Wmax, int vel_depth, void* workspace, long long workspace_bytes, float* gt, long long* stats,
                             td_stream_t stream) {
  // points may be NULL only with no points at all, which the host cannot see: it is refused like the others
  if (!points || !offsets || !P || !sizes || !workspace || !gt || !stats || B <= 0 || Hmax < 1 || Wmax < 2) return TD_ERR_BAD_ARG;
  const long long need = td_velo_depth_workspace_bytes(B, Hmax, Wmax);
  if (need <= 0) return TD_ERR_UNSUPPORTED;
  if (workspace_bytes < need || !td::aligned_to(workspace, 8) || !td::aligned_to(points, 4)) return TD_ERR_BAD_ARG;
  const long long plane = (long long)Hmax * Wmax, groups = (long long)Hmax * (Wmax - 1) + 1;
  td::VeloArgs a;
  a.points = points; a.offsets = offsets; a.P = P; a.sizes = sizes;
  a.B = B; a.Hmax = Hmax; a.Wmax = Wmax; a.vel_depth = vel_depth ? 1 : 0;
  a.last = static_cast<unsigned long long*>(workspace);
  a.gfirst = a.last + (long long)B * plane;
  a.glast = a.gfirst + (long long)B * groups;
  a.gmin = a.glast + (long long)B * groups;
  a.gt = gt;
  a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0xff, (size_t)need, st);
  if (e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)B * 6 * sizeof(long long), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_velo_depth (clear)");
  // enough workgroups per frame to fill the chip at any B, few enough that a block's three stat atomics stay rare
  int per_frame = 2048 / B;
  per_frame = per_frame < 32 ? 32 : (per_frame > 512 ? 512 : per_frame);
  const bool vec = td::aligned_to(points, 16);
  const dim3 block(TD_THREADS), sgrid(per_frame, B), rgrid(td::blocks_1d(plane), B);
  if (vec) hipLaunchKernelGGL((td::velo_scatter_kernel<true>), sgrid, block, 0, st, a);
  else hipLaunchKernelGGL((td::velo_scatter_kernel<false>), sgrid, block, 0, st, a);
  int rc = td::record_launch_error(hipGetLastError(), "td_velo_depth (scatter)");
  if (rc != TD_OK) return rc;
  if (vec) hipLaunchKernelGGL((td::velo_resolve_kernel<true>), rgrid, block, 0, st, a);
  else hipLaunchKernelGGL((td::velo_resolve_kernel<false>), rgrid, block, 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_velo_depth (resolve)");
}
