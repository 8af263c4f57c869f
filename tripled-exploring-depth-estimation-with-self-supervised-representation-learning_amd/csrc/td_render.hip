// A fused point cloud drawn into camera views (tripled_amd/render.py): a z-buffered point renderer.  The reference has no such
// program.
//   clear     one fill of the [C,H,W] buffer of 64-bit integers (all ones = "nothing drawn") and one of the stats rows (zero)
//   scatter   per point and camera: project in float64, then one 64-bit integer atomic minimum per covered pixel of
//             (bits of float32(z)) << 32 | point index
//   resolve   per pixel: the depth from the high word, the colour of the point in the low word, the index itself
// near > 0 makes float32(z) non-negative, so its bit pattern orders like its value: the minimum is the nearest point, and among equal
// float32(z) the lowest index.  A minimum of integers does not depend on the order in which points arrive: two runs return the same
// bits, and they equal the numpy statement (render.render_numpy).  No kernel waits on another workgroup; there are no floating-point
// atomics.  The file is built with -ffp-contract=off: every float64 product, sum and quotient is rounded on its own, as the statement
// rounds it.
#include <math.h>

#include "td_common.h"

namespace td {

#define TD_RENDER_NONE 0xffffffffffffffffULL

struct RenderArgs {
  const float* xyz;                // [V,3]
  const uint8_t* rgb;              // [V,3]
  long long V;
  const double* poses;             // [C,3,4] camera-to-world
  double k[6];                     // the first two rows of K's 3x3 block
  int C, H, W, ortho;
  double pose_scale, z_near, z_far, splat;
  uint8_t background[3];
  unsigned long long* buffer;      // [C, H W]
  float* depth;                    // [C,H,W] (out)
  uint8_t* color;                  // [C,3,H,W] (out)
  int* index;                      // [C,H,W] (out)
  unsigned long long* stats;       // [C,5] (out): points, out of range, outside, drawn, pixels hit
};

// grid (blocks per camera, C): the block's threads stride through the points for camera blockIdx.y
__global__ __launch_bounds__(TD_THREADS) void render_scatter_kernel(const RenderArgs a) {
  __shared__ unsigned cnt[3];
  if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
  __syncthreads();
  const int c = blockIdx.y;
  unsigned long long* st = a.stats + (long long)c * 5;
  if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = (unsigned long long)a.V;
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)c * 12 + k];
  const double t0 = a.pose_scale * P[3], t1 = a.pose_scale * P[7], t2 = a.pose_scale * P[11];
  const double k00 = a.k[0], k01 = a.k[1], k02 = a.k[2], k10 = a.k[3], k11 = a.k[4], k12 = a.k[5];
  const double sk = a.splat * k00;
  const double Wl = (double)(a.W - 1), Hl = (double)(a.H - 1);
  unsigned long long* buf = a.buffer + (long long)c * ((long long)a.H * a.W);
  unsigned local[3] = {0, 0, 0};      // out of range, outside, drawn
  for (long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x; i < a.V; i += (long long)gridDim.x * TD_THREADS) {
    const double e0 = (double)a.xyz[i * 3] - t0, e1 = (double)a.xyz[i * 3 + 1] - t1, e2 = (double)a.xyz[i * 3 + 2] - t2;
    const double q0 = (P[0] * e0 + P[4] * e1) + P[8] * e2;      // the transpose of R
    const double q1 = (P[1] * e0 + P[5] * e1) + P[9] * e2;
    const double z = (P[2] * e0 + P[6] * e1) + P[10] * e2;
    if (!(z >= a.z_near && z <= a.z_far)) { local[0] += 1; continue; }      // a NaN fails
    double u, v, s;
    if (a.ortho) {
      u = (k00 * q0 + k01 * q1) + k02;
      v = (k10 * q0 + k11 * q1) + k12;
      s = sk;
    } else {
      u = ((k00 * q0 + k01 * q1) + k02 * z) / z;
      v = ((k10 * q0 + k11 * q1) + k12 * z) / z;
      s = sk / z;
    }
    const double ui = rint(u), vi = rint(v);      // half to even
    double r = floor(0.5 * s);
    r = r > (double)TD_RENDER_MAX_SPLAT ? (double)TD_RENDER_MAX_SPLAT : r;      // a NaN stays one and fails below
    if (!(ui + r >= 0.0 && ui - r <= Wl && vi + r >= 0.0 && vi - r <= Hl)) { local[1] += 1; continue; }
    local[2] += 1;
    // the compares bound ui by [-r, W-1+r] and r by (-W, 8]: the conversions are exact
    const int x = (int)ui, y = (int)vi, ri = (int)r;
    const int x0 = x - ri < 0 ? 0 : x - ri, x1 = x + ri > a.W - 1 ? a.W - 1 : x + ri;
    const int y0 = y - ri < 0 ? 0 : y - ri, y1 = y + ri > a.H - 1 ? a.H - 1 : y + ri;
    const unsigned long long packed = ((unsigned long long)__float_as_uint((float)z) << 32) | (unsigned long long)i;
    for (int yy = y0; yy <= y1; ++yy) {
      unsigned long long* row = buf + (long long)yy * a.W;
      for (int xx = x0; xx <= x1; ++xx) {
        // an entry only ever decreases: one that reads smaller already stays smaller, and its atomic can be skipped (a stale
        // read is a larger one and costs an atomic that changes nothing)
        if (row[xx] > packed) atomicMin(row + xx, packed);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (local[k]) atomicAdd(&cnt[k], local[k]);      // LDS
  __syncthreads();
  if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(st + 1 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// grid (blocks per plane, C): one thread per pixel
__global__ __launch_bounds__(TD_THREADS) void render_resolve_kernel(const RenderArgs a) {
  __shared__ unsigned cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int c = blockIdx.y;
  const long long plane = (long long)a.H * a.W;
  const long long at = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  bool hit = false;
  if (at < plane) {
    const unsigned long long p = a.buffer[(long long)c * plane + at];
    const long long i = (long long)(p & 0xffffffffULL);
    hit = p != TD_RENDER_NONE && i < a.V;
    uint8_t* col = a.color + (long long)c * 3 * plane + at;
    a.depth[(long long)c * plane + at] = hit ? __uint_as_float((unsigned)(p >> 32)) : 0.f;
    a.index[(long long)c * plane + at] = hit ? (int)i : -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) col[k * plane] = hit ? a.rgb[i * 3 + k] : a.background[k];
  }
  if (hit) atomicAdd(&cnt, 1u);      // LDS
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(a.stats + (long long)c * 5 + 4, (unsigned long long)cnt);
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" long long td_cloud_render_workspace_bytes(int C, int H, int W) {
  if (C <= 0 || C > 65535 || H < 1 || W < 1 || (long long)H * W > 0x7fffffffLL) return 0;
  return (long long)C * H * W * 8;
}

extern "C" int td_cloud_render(const float* xyz, const uint8_t* rgb, long long V, const double* poses, const double* K, int C, int H,
                               int W, double pose_scale, double z_near, double z_far, double splat, int ortho, int bg_r, int bg_g,
                               int bg_b, void* workspace, long long workspace_bytes, float* depth, uint8_t* color, int* index,
                               long long* stats, td_stream_t stream) {
  if (!xyz || !rgb || !poses || !K || !workspace || !depth || !color || !index || !stats || C <= 0 || H < 1 || W < 1 || V < 0)
    return TD_ERR_BAD_ARG;
  if (!(z_near > 0.0) || !isfinite(z_far) || !(z_far >= z_near) || !(splat >= 0.0) || !isfinite(splat)) return TD_ERR_BAD_ARG;
  if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) return TD_ERR_BAD_ARG;
  const long long need = td_cloud_render_workspace_bytes(C, H, W);
  if (need <= 0 || V >= 0x7fffffffLL) return TD_ERR_UNSUPPORTED;
  if (workspace_bytes < need || !td::aligned_to(workspace, 8) || !td::aligned_to(xyz, 4)) return TD_ERR_BAD_ARG;
  const long long plane = (long long)H * W;
  td::RenderArgs a;
  a.xyz = xyz; a.rgb = rgb; a.V = V; a.poses = poses;
  for (int k = 0; k < 6; ++k) a.k[k] = K[k];
  a.C = C; a.H = H; a.W = W; a.ortho = ortho ? 1 : 0;
  a.pose_scale = pose_scale; a.z_near = z_near; a.z_far = z_far; a.splat = splat;
  a.background[0] = (uint8_t)bg_r; a.background[1] = (uint8_t)bg_g; a.background[2] = (uint8_t)bg_b;
  a.buffer = static_cast<unsigned long long*>(workspace);
  a.depth = depth; a.color = color; a.index = index;
  a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0xff, (size_t)need, st);
  if (e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)C * 5 * sizeof(long long), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_cloud_render (clear)");
  const dim3 block(TD_THREADS);
  if (V > 0) {
    // enough workgroups per camera to fill the chip at any C, few enough that a block's three stat atomics stay rare (td_velo_depth)
    int per_camera = 2048 / C;
    per_camera = per_camera < 32 ? 32 : (per_camera > 512 ? 512 : per_camera);
    hipLaunchKernelGGL(td::render_scatter_kernel, dim3(per_camera, C), block, 0, st, a);
    const int rc = td::record_launch_error(hipGetLastError(), "td_cloud_render (scatter)");
    if (rc != TD_OK) return rc;
  }
  hipLaunchKernelGGL(td::render_resolve_kernel, dim3(td::blocks_1d(plane), C), block, 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_cloud_render (resolve)");
}
