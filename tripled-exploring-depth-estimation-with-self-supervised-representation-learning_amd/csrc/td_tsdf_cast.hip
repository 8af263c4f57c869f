// The fused TSDF map ray-cast into camera views (tripled_amd/tsdf.py: raycast_numpy is the statement, equalled bit for bit):
//   td_tsdf_cast   one thread per pixel walks its ray through the key-sorted voxel map in steps of the camera's z, stops at the first
//                  front-facing zero crossing of the trilinearly interpolated distance, and writes the interpolated depth, the
//                  camera-space normal from the interpolant's gradient, and the colour and weight of the voxel the hit lies in.
// The statement (float64, every operation rounded on its own; the file is built with -ffp-contract=off).  A voxel qualifies when
// w >= min_weight; D = (double)S / (double)w.  ray = pixel_ray(x, y);  step = step_voxels voxel;  n_steps = floor((z_far - z_near) /
// step) + 1.  For s = 0 ... n_steps-1:  z_s = z_near + (double)s step;  f = z_s / ray_z;  world = camera_to_world(ray f);  g = world
// inv_voxel.  corners(g): h = g - 0.5, i = floor(h), f = h - i; known when every i_k lies in [-2^20, 2^20 - 1) and the eight voxels
// i + {0,1}^3 exist, qualify and are not the sentinel.  The value interpolates along z, then y, then x, each a + f (b - a).  prev =
// sample s-1 if known.  Hit: prev known, v_prev >= 0, v < 0: t = v_prev / (v_prev - v), z_hit = z_(s-1) + t step.  Back face: prev
// known, v_prev < 0, v >= 0: the ray ends without a hit.  Out of samples: a miss.  At a hit the corners of g_hit (from z_hit as g from
// z_s) are fetched again; the gradient G of the interpolant (d/dx: differences along x, interpolated along z then y; d/dy: along z then
// x; d/dz: along y then x), n = G / sqrt((G_0 G_0 + G_1 G_1) + G_2 G_2), m_k = (R_0k n_0 + R_1k n_1) + R_2k n_2 as float32, not turned
// towards the viewer; (0, 0, 0) and counted when the corners are not all known or |G| is not > 0.  Colour and weight: the voxel
// floor(g_hit), the corner c_k = (floor(g_k) != i_k); with unknown corners at g_hit, the same rule on sample s.
// Everything accumulated is an integer (the counters).  No kernel waits on another workgroup, there are no floating-point atomics.
//
// Layout.  A wave owns an 8 x 8 tile of pixels, a block of four waves 32 x 8: neighbouring rays meet the same key ranges, so a wave's
// binary searches walk the same cache lines, and rays of a tile end at about the same sample.  z is the low key field: the +z corner
// of a column is the next row, a sample costs four lower bounds, not eight, and the fetch leaves at the first missing corner.  (A
// two-level form that asked a sorted table of the occupied 8 x 8 x 8 blocks first was built and measured, lost, and was dropped:
// DESIGN.md 32.)
#include <math.h>

#include "td_grid.h"
#include "td_pixel.h"

#define TD_CAST_TILE_W 32      // a block's pixels: four 8 x 8 wave tiles side by side
#define TD_CAST_TILE_H 8

namespace td {

struct CastArgs {
  const long long* keys;       // [V] ascending, unique
  const long long* sums;       // [V,7]
  long long V;
  const double* poses;         // [C,3,4] camera-to-world
  const double* ik;            // [9] the 3x3 block of inv_K, row-major (device)
  int H, W, tiles_x, n_steps;
  long long min_weight;
  double inv_voxel, z_near, step, pose_scale;
  uint8_t background[3];
  float* depth;                // [C,H,W]
  float* normal;               // [C,3,H,W]
  uint8_t* color;              // [C,3,H,W]
  int* weight;                 // [C,H,W]
  unsigned long long* stats;   // [C,TD_TSDF_CAST_STATS]
};

// the eight corners of a known sample: D in (dx, dy, dz) order, the fractions, floor(h), and the row of each column's lower voxel
struct CastCorners {
  double D[8], f[3], i[3];
  long long row00, row01, row10, row11;      // (dx, dy); scalars, not an array: the pick below must stay a select, out of scratch
};

__device__ __forceinline__ void cast_grid(const CastArgs& a, const double* __restrict__ P, double r0, double r1, double r2, double z,
                                          double* g) {
  const double f = z / r2;
  double wx, wy, wz;
  camera_to_world(P, a.pose_scale, r0 * f, r1 * f, r2 * f, wx, wy, wz);
  g[0] = wx * a.inv_voxel;
  g[1] = wy * a.inv_voxel;
  g[2] = wz * a.inv_voxel;
}

// corners(g).  Every read of keys and sums is at a row inside [0, V).
__device__ __forceinline__ bool cast_corners(const CastArgs& a, const double* g, CastCorners& c) {
  const double lo = -(double)TD_KEY_HALF, hi = (double)(TD_KEY_HALF - 1);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double h = g[k] - 0.5;
    c.i[k] = floor(h);
    c.f[k] = h - c.i[k];
  }
  if (!(c.i[0] >= lo && c.i[0] < hi && c.i[1] >= lo && c.i[1] < hi && c.i[2] >= lo && c.i[2] < hi)) return false;      // a NaN fails
  const long long k000 = key_pack((long long)c.i[0], (long long)c.i[1], (long long)c.i[2]);
#pragma unroll
  for (int q = 0; q < 4; ++q) {      // no field is at its last coordinate: the additions carry nothing
    const long long kb = k000 + ((long long)(q >> 1) << TD_KEY_SHIFT_X) + ((long long)(q & 1) << TD_KEY_SHIFT_Y);
    const long long j = grid_lower_bound(a.keys, a.V, kb);
    if (!(j + 1 < a.V) || kb + 1 == TD_KEY_INVALID) return false;
    if (a.keys[j] != kb || a.keys[j + 1] != kb + 1) return false;
    const long long* r = a.sums + j * 7;
    const long long w0 = r[0], w1 = r[7];
    if (w0 < a.min_weight || w1 < a.min_weight) return false;
    c.D[2 * q] = (double)tsdf_sum(r) / (double)w0;
    c.D[2 * q + 1] = (double)tsdf_sum(r + 7) / (double)w1;
    if (q == 0) c.row00 = j;
    if (q == 1) c.row01 = j;
    if (q == 2) c.row10 = j;
    if (q == 3) c.row11 = j;
  }
  return true;
}

__device__ __forceinline__ double cast_lerp(double a, double b, double f) { return a + f * (b - a); }

// along z, then y, then x
__device__ __forceinline__ double cast_value(const CastCorners& c) {
  const double c00 = cast_lerp(c.D[0], c.D[1], c.f[2]), c01 = cast_lerp(c.D[2], c.D[3], c.f[2]);
  const double c10 = cast_lerp(c.D[4], c.D[5], c.f[2]), c11 = cast_lerp(c.D[6], c.D[7], c.f[2]);
  return cast_lerp(cast_lerp(c00, c01, c.f[1]), cast_lerp(c10, c11, c.f[1]), c.f[0]);
}

// the row of the voxel floor(g) among the corners
__device__ __forceinline__ long long cast_voxel_row(const CastCorners& c, const double* g) {
  const long long cx = floor(g[0]) != c.i[0], cy = floor(g[1]) != c.i[1], cz = floor(g[2]) != c.i[2];
  const long long mx = -cx, my = -cy;      // all ones or zero: the pick is arithmetic on the four values
  return ((c.row00 & ~mx & ~my) | (c.row01 & ~mx & my) | (c.row10 & mx & ~my) | (c.row11 & mx & my)) + cz;
}

__global__ __launch_bounds__(TD_THREADS) void tsdf_cast_kernel(const CastArgs a) {
  __shared__ unsigned cnt[TD_TSDF_CAST_STATS];
  counters_begin<TD_TSDF_CAST_STATS>(cnt);
  const int cam = blockIdx.y;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tile_x * TD_CAST_TILE_W + wave * 8 + (lane & 7), y = tile_y * TD_CAST_TILE_H + (lane >> 3);
  unsigned local[TD_TSDF_CAST_STATS] = {0, 0, 0, 0, 0};
  if (x < a.W && y < a.H) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)cam * 12 + k];
    double ik[9], r0, r1, r2;
#pragma unroll
    for (int k = 0; k < 9; ++k) ik[k] = a.ik[k];
    pixel_ray(ik, (double)x, (double)y, r0, r1, r2);
    bool prev_known = false, hit = false, back = false;
    double v_prev = 0.0, v = 0.0, g[3];
    CastCorners c;
    int s = 0;
    for (; s < a.n_steps; ++s) {
      cast_grid(a, P, r0, r1, r2, a.z_near + (double)s * a.step, g);
      const bool known = cast_corners(a, g, c);
      if (known) {
        v = cast_value(c);
        hit = prev_known && v_prev >= 0.0 && v < 0.0;
        back = prev_known && v_prev < 0.0 && v >= 0.0;
        if (hit || back) break;
        v_prev = v;
      }
      prev_known = known;
    }
    const long long plane = (long long)a.H * a.W;
    const long long pix = (long long)cam * plane + (long long)y * a.W + x;
    const long long pix3 = (long long)cam * 3 * plane + (long long)y * a.W + x;
    float depth = 0.f, m[3] = {0.f, 0.f, 0.f};
    uint8_t rgb[3] = {a.background[0], a.background[1], a.background[2]};
    int weight = 0;
    local[0] = 1;
    if (hit) {
      local[1] = 1;
      const double t = v_prev / (v_prev - v);
      const double z_hit = (a.z_near + (double)(s - 1) * a.step) + t * a.step;
      depth = (float)z_hit;
      long long row = cast_voxel_row(c, g);      // sample s, unless the corners of the hit are known
      double gh[3];
      cast_grid(a, P, r0, r1, r2, z_hit, gh);
      bool has_normal = false;
      if (cast_corners(a, gh, c)) {
        row = cast_voxel_row(c, gh);
        const double* D = c.D;
        const double G0 = cast_lerp(cast_lerp(D[4] - D[0], D[5] - D[1], c.f[2]), cast_lerp(D[6] - D[2], D[7] - D[3], c.f[2]), c.f[1]);
        const double G1 = cast_lerp(cast_lerp(D[2] - D[0], D[3] - D[1], c.f[2]), cast_lerp(D[6] - D[4], D[7] - D[5], c.f[2]), c.f[0]);
        const double G2 = cast_lerp(cast_lerp(D[1] - D[0], D[3] - D[2], c.f[1]), cast_lerp(D[5] - D[4], D[7] - D[6], c.f[1]), c.f[0]);
        const double norm = sqrt((G0 * G0 + G1 * G1) + G2 * G2);
        if (norm > 0.0) {
          const double n0 = G0 / norm, n1 = G1 / norm, n2 = G2 / norm;
          has_normal = true;
#pragma unroll
          for (int k = 0; k < 3; ++k) m[k] = (float)((P[k] * n0 + P[4 + k] * n1) + P[8 + k] * n2);
        }
      }
      if (!has_normal) local[4] = 1;
      const long long* r = a.sums + row * 7;
      const long long n = r[0];
#pragma unroll
      for (int k = 0; k < 3; ++k) rgb[k] = (uint8_t)((2 * r[4 + k] + n) / (2 * n));      // n >= min_weight >= 1
      weight = n > 0x7fffffffLL ? 0x7fffffff : (int)n;
    } else {
      local[2] = back ? 1 : 0;
      local[3] = back ? 0 : 1;
    }
    a.depth[pix] = depth;
    a.weight[pix] = weight;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a.normal[pix3 + k * plane] = m[k];
      a.color[pix3 + k * plane] = rgb[k];
    }
  }
  counters_end<TD_TSDF_CAST_STATS>(cnt, local, a.stats + (long long)cam * TD_TSDF_CAST_STATS);
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_tsdf_cast(const long long* keys, const long long* sums, long long V, const double* poses, const double* inv_K, int C, int H, int W, double voxel, double inv_voxel,
                            long long min_weight, double z_near, double z_far, double step_voxels, double pose_scale, int bg_r, int bg_g,
                            int bg_b, float* depth, float* normal, uint8_t* color, int* weight, long long* stats, td_stream_t stream) {
  if (!keys || !sums || !poses || !inv_K || !depth || !normal || !color || !weight || !stats || V < 0 || C < 0 || H < 1 || W < 1)
    return TD_ERR_BAD_ARG;
  if (!(voxel > 0.0) || !isfinite(voxel) || !(inv_voxel > 0.0) || !isfinite(inv_voxel) || min_weight < 1) return TD_ERR_BAD_ARG;
  if (!(z_near > 0.0) || !isfinite(z_far) || !(z_far >= z_near) || !(step_voxels > 0.0) || !isfinite(step_voxels) || !isfinite(pose_scale))
    return TD_ERR_BAD_ARG;
  if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) return TD_ERR_BAD_ARG;
  const double step = step_voxels * voxel;
  if (!(step > 0.0)) return TD_ERR_BAD_ARG;
  const double steps = floor((z_far - z_near) / step) + 1.0;
  if (!(steps <= (double)TD_TSDF_CAST_MAX_STEPS)) return TD_ERR_UNSUPPORTED;
  const long long tiles_x = ((long long)W + TD_CAST_TILE_W - 1) / TD_CAST_TILE_W, tiles_y = ((long long)H + TD_CAST_TILE_H - 1) / TD_CAST_TILE_H;
  if (C > 65535 || (long long)H * W > 0x7fffffffLL || tiles_x * tiles_y > 0x7fffffffLL) return TD_ERR_UNSUPPORTED;
  if (C == 0) return TD_OK;
  td::CastArgs a;
  a.keys = keys; a.sums = sums; a.V = V; a.poses = poses;
  a.ik = inv_K;
  a.H = H; a.W = W; a.tiles_x = (int)tiles_x; a.n_steps = (int)steps;
  a.min_weight = min_weight; a.inv_voxel = inv_voxel; a.z_near = z_near; a.step = step; a.pose_scale = pose_scale;
  a.background[0] = (uint8_t)bg_r; a.background[1] = (uint8_t)bg_g; a.background[2] = (uint8_t)bg_b;
  a.depth = depth; a.normal = normal; a.color = color; a.weight = weight;
  a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(stats, 0, (size_t)C * TD_TSDF_CAST_STATS * sizeof(long long), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_tsdf_cast (clear)");
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)C), block(TD_THREADS);
  hipLaunchKernelGGL(td::tsdf_cast_kernel, grid, block, 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_tsdf_cast");
}
