// Surfel rendering of a fused cloud (tripled_amd/render.py, tripled_amd/cloud_normals.py): every point an oriented disc in space.
// The reference has no such program.
//   td_normals_orient         one thread per point: the nearest camera centre (staged through LDS in chunks of 256) decides the sign
//                             of the point's normal
//   td_cloud_render_surfels   clear / scatter / resolve like td_cloud_render (td_render.hip), the same [C, H W] table of 64-bit
//                             integer minima.  scatter: per point and camera the disc's centre and normal in the camera, a
//                             conservative pixel box, and per pixel of the box the ray-disc intersection; a covered pixel takes the
//                             minimum of (bits of float32(t)) << 32 | point index.  resolve: per pixel the winner's depth, index,
//                             camera-space normal and shaded colour, recomputed from the index.
// Work distribution of the scatter: a thread draws a box of at most TD_SURFEL_OWN pixels itself and appends a larger one to an LDS
// queue, which the workgroup drains after every pass of its grid-stride loop, one wave per box with the lanes across its pixels
// (form 2), or every thread draws its own box whatever its size (form 1).  A minimum of integers does not depend on the order of
// arrival: both forms return the same bits, and they equal render.render_surfels_numpy.  No kernel waits on another workgroup, there
// are no floating-point atomics, and the file is built with -ffp-contract=off: every float64 operation is rounded on its own.
#include <math.h>

#include "td_common.h"

namespace td {

#define TD_SURFEL_NONE 0xffffffffffffffffULL
#define TD_SURFEL_OWN 4                // a box of at most this many pixels is drawn by its own thread (form 2); measured: DESIGN 27
#define TD_ORIENT_CHUNK 256

// ---------------------------------------------------------------------------------------------------------------------------
// orientation

struct OrientArgs {
  const float* xyz;                // [V,3]
  const float* normal;             // [V,3]
  long long V;
  const double* poses;             // [C,3,4]
  int C;
  double pose_scale;
  float* out;                      // [V,3] (out)
  int* camera;                     // [V] (out)
  unsigned long long* stats;       // [4]: flipped, kept, none, invalid
};

__global__ __launch_bounds__(TD_THREADS) void normals_orient_kernel(const OrientArgs a) {
  __shared__ double centre[TD_ORIENT_CHUNK * 3];
  __shared__ unsigned cnt[4];
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  const long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  const bool live = i < a.V;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) { px = (double)a.xyz[i * 3]; py = (double)a.xyz[i * 3 + 1]; pz = (double)a.xyz[i * 3 + 2]; }
  int cam = -1;
  double best = 0.0, w0 = 0.0, w1 = 0.0, w2 = 0.0;
  for (int c0 = 0; c0 < a.C; c0 += TD_ORIENT_CHUNK) {      // uniform: every thread takes part in the staging
    const int n = a.C - c0 < TD_ORIENT_CHUNK ? a.C - c0 : TD_ORIENT_CHUNK;
    __syncthreads();                                       // the previous chunk has been read (and cnt is cleared)
    for (int j = threadIdx.x; j < n; j += TD_THREADS) {
      const double* P = a.poses + (long long)(c0 + j) * 12;
      centre[j * 3] = a.pose_scale * P[3];
      centre[j * 3 + 1] = a.pose_scale * P[7];
      centre[j * 3 + 2] = a.pose_scale * P[11];
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < n; ++j) {
        const double dx = centre[j * 3] - px, dy = centre[j * 3 + 1] - py, dz = centre[j * 3 + 2] - pz;
        const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        if (d2 == d2 && (cam < 0 || d2 < best)) { cam = c0 + j; best = d2; w0 = dx; w1 = dy; w2 = dz; }      // a NaN never wins
      }
    }
  }
  if (live) {
    float n0 = a.normal[i * 3], n1 = a.normal[i * 3 + 1], n2 = a.normal[i * 3 + 2];
    int cls;
    if (n0 == 0.f && n1 == 0.f && n2 == 0.f) cls = 2;      // none
    else if (cam < 0) cls = 3;                             // invalid: no camera at a distance that is a number
    else {
      const double s = (((double)n0 * w0) + ((double)n1 * w1)) + ((double)n2 * w2);
      if (s != s) cls = 3;
      else if (s < 0.0) { cls = 0; n0 = -n0; n1 = -n1; n2 = -n2; }
      else cls = 1;
    }
    a.out[i * 3] = n0; a.out[i * 3 + 1] = n1; a.out[i * 3 + 2] = n2;
    a.camera[i] = cam;
    atomicAdd(&cnt[cls], 1u);      // LDS
  }
  __syncthreads();
  if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(a.stats + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// rendering

struct SurfelArgs {
  const float* xyz;                // [V,3]
  const uint8_t* rgb;              // [V,3]
  const float* normal;             // [V,3]
  long long V;
  const double* poses;             // [C,3,4] camera-to-world
  double k00, k01, k02, k11, k12;
  int C, H, W, ortho, cull;
  double pose_scale, z_near, z_far, radius, radius2, ambient, one_minus_ambient;
  uint8_t background[3];
  unsigned long long* buffer;      // [C, H W]
  float* depth;                    // [C,H,W] (out)
  uint8_t* color;                  // [C,3,H,W] (out)
  int* index;                      // [C,H,W] (out)
  float* nmap;                     // [C,3,H,W] (out)
  unsigned long long* stats;       // [C,8] (out)
};

struct Surfel {
  double q0, q1, z, m0, m1, m2;
  bool billboard;
};

// the disc's centre and normal in the camera P (the pose's twelve entries; t: pose_scale times its translation)
__device__ __forceinline__ Surfel surfel_setup(const SurfelArgs& a, const double* P, double t0, double t1, double t2, long long i) {
  Surfel s;
  const double e0 = (double)a.xyz[i * 3] - t0, e1 = (double)a.xyz[i * 3 + 1] - t1, e2 = (double)a.xyz[i * 3 + 2] - t2;
  s.q0 = (P[0] * e0 + P[4] * e1) + P[8] * e2;      // the transpose of R
  s.q1 = (P[1] * e0 + P[5] * e1) + P[9] * e2;
  s.z = (P[2] * e0 + P[6] * e1) + P[10] * e2;
  const float f0 = a.normal[i * 3], f1 = a.normal[i * 3 + 1], f2 = a.normal[i * 3 + 2];
  s.billboard = f0 == 0.f && f1 == 0.f && f2 == 0.f;
  const double n0 = (double)f0, n1 = (double)f1, n2 = (double)f2;
  s.m0 = (P[0] * n0 + P[4] * n1) + P[8] * n2;
  s.m1 = (P[1] * n0 + P[5] * n1) + P[9] * n2;
  s.m2 = (P[2] * n0 + P[6] * n1) + P[10] * n2;
  if (s.billboard) { s.m0 = 0.0; s.m1 = 0.0; s.m2 = -1.0; }
  return s;
}

// the ray of pixel (x, y) against the disc: true when the pixel is covered.  t: the hit's depth, den: m . dir, (d0, d1): the ray
__device__ __forceinline__ bool surfel_pixel(const SurfelArgs& a, const Surfel& s, int x, int y, double& t, double& den, double& d0,
                                             double& d1) {
  d1 = ((double)y - a.k12) / a.k11;
  d0 = (((double)x - a.k02) - a.k01 * d1) / a.k00;
  double num;
  if (a.ortho) {
    den = s.m2;
    num = ((s.m0 * (s.q0 - d0)) + (s.m1 * (s.q1 - d1))) + (s.m2 * s.z);
  } else {
    den = ((s.m0 * d0) + (s.m1 * d1)) + s.m2;
    num = ((s.m0 * s.q0) + (s.m1 * s.q1)) + (s.m2 * s.z);
  }
  t = 0.0;
  if (!(den < 0.0 || den > 0.0)) return false;      // edge-on, or a NaN
  t = num / den;
  const double h0 = a.ortho ? d0 : t * d0, h1 = a.ortho ? d1 : t * d1;
  const double e0 = h0 - s.q0, e1 = h1 - s.q1, e2 = t - s.z;
  const double dist2 = ((e0 * e0) + (e1 * e1)) + (e2 * e2);
  return dist2 <= a.radius2 && t >= a.z_near && t <= a.z_far;      // a NaN fails
}

__device__ __forceinline__ void surfel_offer(const SurfelArgs& a, const Surfel& s, unsigned long long* buf, unsigned idx, int x, int y) {
  double t, den, d0, d1;
  if (!surfel_pixel(a, s, x, y, t, den, d0, d1)) return;
  const unsigned long long packed = ((unsigned long long)__float_as_uint((float)t) << 32) | (unsigned long long)idx;
  unsigned long long* at = buf + (long long)y * a.W + x;
  // an entry only ever decreases: one that reads smaller already stays smaller, and its atomic can be skipped (td_render.hip)
  if (*at > packed) atomicMin(at, packed);
}

// grid (blocks per camera, C): the block's threads stride through the points for camera blockIdx.y
template <bool COOP>
__global__ __launch_bounds__(TD_THREADS) void surfel_scatter_kernel(const SurfelArgs a) {
  __shared__ unsigned cnt[6];
  __shared__ unsigned queued;
  __shared__ double qd[COOP ? 6 : 1][TD_THREADS];
  __shared__ unsigned qi[COOP ? TD_THREADS : 1];
  __shared__ int qbox[COOP ? TD_THREADS : 1][4];      // x0, y0, width, pixels
  if (threadIdx.x < 6) cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) queued = 0;
  __syncthreads();
  const int c = blockIdx.y;
  unsigned long long* st = a.stats + (long long)c * 8;
  if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = (unsigned long long)a.V;
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)c * 12 + k];
  const double t0 = a.pose_scale * P[3], t1 = a.pose_scale * P[7], t2 = a.pose_scale * P[11];
  const double Wl = (double)(a.W - 1), Hl = (double)(a.H - 1);
  const double ak01 = fabs(a.k01);
  unsigned long long* buf = a.buffer + (long long)c * ((long long)a.H * a.W);
  unsigned local[6] = {0, 0, 0, 0, 0, 0};      // out of range, outside, culled, capped, billboards, drawn
  // the trip count is the same for every thread of the block: the queue is drained between barriers
  for (long long base = (long long)blockIdx.x * TD_THREADS; base < a.V; base += (long long)gridDim.x * TD_THREADS) {
    const long long i = base + threadIdx.x;
    if (i < a.V) {
      const Surfel s = surfel_setup(a, P, t0, t1, t2, i);
      do {
        if (!(s.z >= a.z_near && s.z <= a.z_far)) { local[0] += 1; break; }      // a NaN fails
        double u, v, bx, by;
        if (a.ortho) {
          if (a.cull && s.m2 > 0.0) { local[2] += 1; break; }
          u = (a.k00 * s.q0 + a.k01 * s.q1) + a.k02;
          v = a.k11 * s.q1 + a.k12;
          bx = (a.k00 + ak01) * a.radius;
          by = a.k11 * a.radius;
        } else {
          if (a.cull && ((s.m0 * s.q0) + (s.m1 * s.q1)) + (s.m2 * s.z) > 0.0) { local[2] += 1; break; }
          u = ((a.k00 * s.q0 + a.k01 * s.q1) + a.k02 * s.z) / s.z;
          v = (a.k11 * s.q1 + a.k12 * s.z) / s.z;
          double tm = s.z - a.radius;
          tm = tm < a.z_near ? a.z_near : tm;                       // no hit in range is nearer
          const double g = a.radius / tm;
          const double ax = g * (1.0 + fabs(s.q0) / s.z), ay = g * (1.0 + fabs(s.q1) / s.z);
          bx = a.k00 * ax + ak01 * ay;
          by = a.k11 * ay;
        }
        const double ui = rint(u), vi = rint(v);      // half to even
        const double b = bx > by ? bx : by;
        double r = floor(b + TD_SURFEL_SLACK);
        const bool capped = r > (double)TD_SURFEL_MAX;
        r = capped ? (double)TD_SURFEL_MAX : r;       // a NaN stays one and fails below
        if (!(ui + r >= 0.0 && ui - r <= Wl && vi + r >= 0.0 && vi - r <= Hl)) { local[1] += 1; break; }
        local[5] += 1;
        if (capped) local[3] += 1;
        if (s.billboard) local[4] += 1;
        // the compares bound ui by [-r, W-1+r] and r by [0, 16] (b + slack of a number is a number): the conversions are exact
        const long long x = (long long)ui, y = (long long)vi, ri = (long long)r;
        const int x0 = x - ri < 0 ? 0 : (int)(x - ri), x1 = x + ri > a.W - 1 ? a.W - 1 : (int)(x + ri);      // inside the image
        const int y0 = y - ri < 0 ? 0 : (int)(y - ri), y1 = y + ri > a.H - 1 ? a.H - 1 : (int)(y + ri);
        bool own = true;
        if constexpr (COOP) {
          own = (x1 - x0 + 1) * (y1 - y0 + 1) <= TD_SURFEL_OWN;
          if (!own) {
            const unsigned slot = atomicAdd(&queued, 1u);      // LDS; at most one per thread and pass: slot < TD_THREADS
            qd[0][slot] = s.q0; qd[1][slot] = s.q1; qd[2][slot] = s.z;
            qd[3][slot] = s.m0; qd[4][slot] = s.m1; qd[5][slot] = s.m2;
            qi[slot] = (unsigned)i;
            qbox[slot][0] = x0; qbox[slot][1] = y0; qbox[slot][2] = x1 - x0 + 1; qbox[slot][3] = (x1 - x0 + 1) * (y1 - y0 + 1);
          }
        }
        if (own) {
          for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) surfel_offer(a, s, buf, (unsigned)i, xx, yy);
        }
      } while (false);
    }
    if constexpr (COOP) {
      __syncthreads();
      const unsigned n = queued;
      __syncthreads();
      if (threadIdx.x == 0) queued = 0;
      const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
      for (unsigned e = wave; e < n; e += TD_THREADS / 64) {
        Surfel s;
        s.q0 = qd[0][e]; s.q1 = qd[1][e]; s.z = qd[2][e];
        s.m0 = qd[3][e]; s.m1 = qd[4][e]; s.m2 = qd[5][e];
        s.billboard = false;      // m is (0, 0, -1) already
        const int bx0 = qbox[e][0], by0 = qbox[e][1], bw = qbox[e][2], area = qbox[e][3];
        const unsigned idx = qi[e];
        for (int p = lane; p < area; p += 64) {
          const int row = p / bw;
          surfel_offer(a, s, buf, idx, bx0 + (p - row * bw), by0 + row);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    if (local[k]) atomicAdd(&cnt[k], local[k]);      // LDS
  __syncthreads();
  if (threadIdx.x < 6 && cnt[threadIdx.x]) atomicAdd(st + 1 + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

// grid (blocks per plane, C): one thread per pixel; the winner's disc is set up again and its ray intersected again
__global__ __launch_bounds__(TD_THREADS) void surfel_resolve_kernel(const SurfelArgs a) {
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
    hit = p != TD_SURFEL_NONE && i < a.V;
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    uint8_t col[3] = {a.background[0], a.background[1], a.background[2]};
    if (hit) {
      double P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = a.poses[(long long)c * 12 + k];
      const Surfel s = surfel_setup(a, P, a.pose_scale * P[3], a.pose_scale * P[7], a.pose_scale * P[11], i);
      const int y = (int)(at / a.W), x = (int)(at - (long long)y * a.W);
      double t, den, d0, d1;
      surfel_pixel(a, s, x, y, t, den, d0, d1);
      const bool away = den > 0.0;      // the normal points away from the viewer
      n0 = (float)s.m0; n1 = (float)s.m1; n2 = (float)s.m2;
      if (away) { n0 = -n0; n1 = -n1; n2 = -n2; }
#pragma unroll
      for (int k = 0; k < 3; ++k) col[k] = a.rgb[i * 3 + k];
      if (a.ambient != 1.0) {
        const double dd = a.ortho ? 1.0 : ((d0 * d0) + (d1 * d1)) + 1.0;
        const double shade = fabs(den) / sqrt(dd);
        const double f = a.ambient + a.one_minus_ambient * shade;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double val = floor((double)col[k] * f + 0.5);
          col[k] = val >= 255.0 ? (uint8_t)255 : (val > 0.0 ? (uint8_t)val : (uint8_t)0);      // a NaN gives 0; none arises from a winner
        }
      }
    }
    a.depth[(long long)c * plane + at] = hit ? __uint_as_float((unsigned)(p >> 32)) : 0.f;
    a.index[(long long)c * plane + at] = hit ? (int)i : -1;
    uint8_t* cout = a.color + (long long)c * 3 * plane + at;
    float* nout = a.nmap + (long long)c * 3 * plane + at;
#pragma unroll
    for (int k = 0; k < 3; ++k) cout[k * plane] = col[k];
    nout[0] = n0; nout[plane] = n1; nout[2 * plane] = n2;
  }
  if (hit) atomicAdd(&cnt, 1u);      // LDS
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(a.stats + (long long)c * 8 + 7, (unsigned long long)cnt);
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_normals_orient(const float* xyz, const float* normal, long long V, const double* poses, int C, double pose_scale,
                                 float* out_normal, int* camera, long long* stats, td_stream_t stream) {
  if (!xyz || !normal || !poses || !out_normal || !camera || !stats || V < 0 || C <= 0) return TD_ERR_BAD_ARG;
  if (!td::aligned_to(xyz, 4) || !td::aligned_to(normal, 4) || !td::aligned_to(poses, 8) || !td::aligned_to(stats, 8)) return TD_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(long long), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_normals_orient (clear)");
  if (V == 0) return TD_OK;
  const unsigned blocks = td::blocks_1d(V);
  if (!blocks) return TD_ERR_UNSUPPORTED;
  td::OrientArgs a;
  a.xyz = xyz; a.normal = normal; a.V = V; a.poses = poses; a.C = C; a.pose_scale = pose_scale;
  a.out = out_normal; a.camera = camera; a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipLaunchKernelGGL(td::normals_orient_kernel, dim3(blocks), dim3(TD_THREADS), 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_normals_orient");
}

extern "C" int td_cloud_render_surfels(const float* xyz, const uint8_t* rgb, const float* normal, long long V, const double* poses,
                                       const double* K, int C, int H, int W, double pose_scale, double z_near, double z_far,
                                       double radius, int ortho, int cull, double ambient, int form, int bg_r, int bg_g, int bg_b,
                                       void* workspace, long long workspace_bytes, float* depth, uint8_t* color, int* index,
                                       float* normal_map, long long* stats, td_stream_t stream) {
  if (!xyz || !rgb || !normal || !poses || !K || !workspace || !depth || !color || !index || !normal_map || !stats || C <= 0 || H < 1 ||
      W < 1 || V < 0)
    return TD_ERR_BAD_ARG;
  if (!(z_near > 0.0) || !isfinite(z_far) || !(z_far >= z_near) || !(radius > 0.0) || !isfinite(radius) || !(ambient >= 0.0) ||
      !(ambient <= 1.0) || form < 0 || form > 2)
    return TD_ERR_BAD_ARG;
  // the rays invert K's upper triangle: K10 must be 0 and the focal lengths positive
  for (int k = 0; k < 6; ++k)
    if (!isfinite(K[k])) return TD_ERR_BAD_ARG;
  if (!(K[0] > 0.0) || !(K[4] > 0.0) || K[3] != 0.0) return TD_ERR_BAD_ARG;
  if (bg_r < 0 || bg_r > 255 || bg_g < 0 || bg_g > 255 || bg_b < 0 || bg_b > 255) return TD_ERR_BAD_ARG;
  const long long need = td_cloud_render_workspace_bytes(C, H, W);
  if (need <= 0 || V >= 0x7fffffffLL) return TD_ERR_UNSUPPORTED;
  if (workspace_bytes < need || !td::aligned_to(workspace, 8) || !td::aligned_to(xyz, 4) || !td::aligned_to(normal, 4)) return TD_ERR_BAD_ARG;
  const long long plane = (long long)H * W;
  td::SurfelArgs a;
  a.xyz = xyz; a.rgb = rgb; a.normal = normal; a.V = V; a.poses = poses;
  a.k00 = K[0]; a.k01 = K[1]; a.k02 = K[2]; a.k11 = K[4]; a.k12 = K[5];
  a.C = C; a.H = H; a.W = W; a.ortho = ortho ? 1 : 0; a.cull = cull ? 1 : 0;
  a.pose_scale = pose_scale; a.z_near = z_near; a.z_far = z_far; a.radius = radius; a.radius2 = radius * radius;
  a.ambient = ambient; a.one_minus_ambient = 1.0 - ambient;
  a.background[0] = (uint8_t)bg_r; a.background[1] = (uint8_t)bg_g; a.background[2] = (uint8_t)bg_b;
  a.buffer = static_cast<unsigned long long*>(workspace);
  a.depth = depth; a.color = color; a.index = index; a.nmap = normal_map;
  a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0xff, (size_t)need, st);
  if (e == hipSuccess) e = hipMemsetAsync(stats, 0, (size_t)C * 8 * sizeof(long long), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_cloud_render_surfels (clear)");
  const dim3 block(TD_THREADS);
  if (V > 0) {
    int per_camera = 2048 / C;      // td_cloud_render's choice
    per_camera = per_camera < 32 ? 32 : (per_camera > 512 ? 512 : per_camera);
    if (form == 1) hipLaunchKernelGGL(td::surfel_scatter_kernel<false>, dim3(per_camera, C), block, 0, st, a);
    else hipLaunchKernelGGL(td::surfel_scatter_kernel<true>, dim3(per_camera, C), block, 0, st, a);
    const int rc = td::record_launch_error(hipGetLastError(), "td_cloud_render_surfels (scatter)");
    if (rc != TD_OK) return rc;
  }
  hipLaunchKernelGGL(td::surfel_resolve_kernel, dim3(td::blocks_1d(plane), C), block, 0, st, a);
  return td::record_launch_error(hipGetLastError(), "td_cloud_render_surfels (resolve)");
}
