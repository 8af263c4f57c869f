// The pixel front end of the per-pixel kernels (td_cloud_keys, td_tsdf_samples): a thread's run of columns, the single-frame validity
// rules, the pixel's ray, the per-block counters and the launch.  The rules are ONE piece of code, so "td_tsdf_samples drops what
// td_cloud_keys drops" holds by construction; cloud.pixel_causes_numpy is their numpy statement.  Every user is built with
// -ffp-contract=off.  Everything here is inlined and every array is indexed by constants once unrolled: nothing goes to scratch.
#pragma once
#include <math.h>

#include "td_common.h"

namespace td {

// VEC consecutive elements as one access (the caller guarantees sizeof(T) * VEC alignment)
template <int VEC, typename T>
__device__ __forceinline__ void load_run(const T* __restrict__ p, T* out) {
  struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
  const Pack pk = *reinterpret_cast<const Pack*>(p);
#pragma unroll
  for (int j = 0; j < VEC; ++j) out[j] = pk.v[j];
}

template <int VEC, typename T>
__device__ __forceinline__ void store_run(T* __restrict__ p, const T* in) {
  struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
  Pack pk;
#pragma unroll
  for (int j = 0; j < VEC; ++j) pk.v[j] = in[j];
  *reinterpret_cast<Pack*>(p) = pk;
}

// the flying-pixel test against one neighbour, float32 on the unscaled depths
__device__ __forceinline__ bool edge_bad(float d, float nb, float edge) {
  return !isfinite(nb) || fabsf(d - nb) > edge * fminf(d, nb);
}

// ray_k = (m_k0 u + m_k1 v) + m_k2 for the 3x3 block m of inv_K, row-major: the pixel (u, v) at integer coordinates
__device__ __forceinline__ void pixel_ray(const double* __restrict__ ik, double u, double v, double& r0, double& r1, double& r2) {
  r0 = (ik[0] * u + ik[1] * v) + ik[2];
  r1 = (ik[3] * u + ik[4] * v) + ik[5];
  r2 = (ik[6] * u + ik[7] * v) + ik[8];
}

// A thread owns VEC consecutive columns x0 ... x0 + VEC - 1 of row y of frame b; VEC divides W, so the flat pixel index of chunk c is
// c * VEC and a wave's loads and stores are contiguous.
template <int VEC>
struct PixelRun {
  int b, y, x0;
  long long pix;                   // the flat index of the run's first pixel
  float d[VEC];                    // the depths as stored
  double ds[VEC];                  // (double)d * depth_scale
  uint8_t cr[VEC], cg[VEC], cb[VEC];
  int cause[VEC];                  // the first that holds: 1 off the stride's lattice, 2 border, 3 depth, 4 flying pixel, 5 mask; else 0
};

// Loads this thread's run and applies the rules; false for a thread beyond the last run.  Args: depth [B,H,W], color [B,3,H,W], B, H,
// W, stride, border, depth_scale, min_depth, max_range, edge.  mask: [B,H,W] (0 drops the pixel) or NULL.  The rows above and below are
// read with the run's alignment, the left and right neighbours are two scalar loads of lines the neighbouring threads already hold;
// none of the four is read unless edge > 0.
template <int VEC, typename Args>
__device__ __forceinline__ bool pixel_run_load(const Args& a, const uint8_t* __restrict__ mask, PixelRun<VEC>& r) {
  const int H = a.H, W = a.W;
  const long long cpr = W / VEC;
  const long long c = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (c >= (long long)a.B * H * cpr) return false;
  const long long row = c / cpr;
  const int x0 = (int)(c - row * cpr) * VEC;
  const int b = (int)(row / H);
  const int y = (int)(row - (long long)b * H);
  const long long pix = c * VEC;
  const long long plane = (long long)H * W;
  r.b = b; r.y = y; r.x0 = x0; r.pix = pix;
  float up[VEC], dn[VEC];
  uint8_t mk[VEC];
  load_run<VEC>(a.depth + pix, r.d);
  const uint8_t* col = a.color + ((long long)b * 3 * H + y) * W + x0;
  load_run<VEC>(col, r.cr);
  load_run<VEC>(col + plane, r.cg);
  load_run<VEC>(col + 2 * plane, r.cb);
  if (mask) load_run<VEC>(mask + pix, mk);
  const bool use_edge = a.edge > 0.f;
  const bool has_up = y > 0, has_dn = y + 1 < H, has_l = x0 > 0, has_r = x0 + VEC < W;
  float left = 0.f, right = 0.f;
  if (use_edge) {
    if (has_up) load_run<VEC>(a.depth + pix - W, up);
    if (has_dn) load_run<VEC>(a.depth + pix + W, dn);
    if (has_l) left = a.depth[pix - 1];
    if (has_r) right = a.depth[pix + VEC];
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int x = x0 + j;
    const float d = r.d[j];
    int cause = 0;
    const double ds = (double)d * a.depth_scale;
    if (x % a.stride != 0 || y % a.stride != 0) cause = 1;
    else if (x < a.border || x >= W - a.border || y < a.border || y >= H - a.border) cause = 2;
    else if (!isfinite(d) || !(ds >= a.min_depth && ds <= a.max_range)) cause = 3;
    else if (use_edge) {
      bool bad = false;
      if (has_up) bad = bad || edge_bad(d, up[j], a.edge);
      if (has_dn) bad = bad || edge_bad(d, dn[j], a.edge);
      if (j > 0) bad = bad || edge_bad(d, r.d[j > 0 ? j - 1 : 0], a.edge);
      else if (has_l) bad = bad || edge_bad(d, left, a.edge);
      if (j + 1 < VEC) bad = bad || edge_bad(d, r.d[j + 1 < VEC ? j + 1 : j], a.edge);
      else if (has_r) bad = bad || edge_bad(d, right, a.edge);
      if (bad) cause = 4;
    }
    if (cause == 0 && mask && mk[j] == 0) cause = 5;
    r.ds[j] = ds;
    r.cause[j] = cause;
  }
  return true;
}

// the run's colours in a payload's bits 30 ... 53
template <int VEC>
__device__ __forceinline__ unsigned long long pixel_rgb(const PixelRun<VEC>& r, int j) {
  return ((unsigned long long)r.cr[j] << 30) | ((unsigned long long)r.cg[j] << 38) | ((unsigned long long)r.cb[j] << 46);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Per-block counters: cnt[N] in LDS, zeroed by a prologue; an epilogue adds each one that is not zero to stats with one global atomic.
// How a kernel adds into cnt in between is its own (a thread's totals `local`, one cause, wave ballots).  The caller's `if (stats)`
// around each call is wave-uniform.
template <int N>
__device__ __forceinline__ void counters_begin(unsigned* cnt) {
  if (threadIdx.x < N) cnt[threadIdx.x] = 0;
  __syncthreads();
}

template <int N>
__device__ __forceinline__ void counters_end(const unsigned* cnt, unsigned long long* __restrict__ stats) {
  __syncthreads();
  if (threadIdx.x < N && cnt[threadIdx.x]) atomicAdd(stats + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

template <int N>      // a thread's totals into cnt first
__device__ __forceinline__ void counters_end(unsigned* cnt, const unsigned* local, unsigned long long* __restrict__ stats) {
#pragma unroll
  for (int k = 0; k < N; ++k)
    if (local[k]) atomicAdd(&cnt[k], local[k]);      // LDS
  counters_end<N>(cnt, stats);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The launch: the widest run (4, 2 or 1 columns) the row length and the base pointers allow, one thread per run.  k4, k2, k1: the
// kernel for each width.  Args as above, with key and payload [.. B*H*W] (out); mask: [B,H,W] or NULL.
template <typename Args>
static int launch_pixel_runs(void (*k4)(Args), void (*k2)(Args), void (*k1)(Args), const Args& a, const uint8_t* mask, td_stream_t stream,
                             const char* what) {
  int vec = 4;
  while (vec > 1 && !(a.W % vec == 0 && aligned_to(a.depth, 4 * vec) && aligned_to(a.color, vec) && (!mask || aligned_to(mask, vec)) &&
                      aligned_to(a.key, 8 * vec) && aligned_to(a.payload, 8 * vec)))
    vec >>= 1;
  const dim3 grid(blocks_1d((long long)a.B * a.H * (a.W / vec))), block(TD_THREADS);
  if (!grid.x) return TD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(vec == 4 ? k4 : (vec == 2 ? k2 : k1), grid, block, 0, (hipStream_t)stream, a);
  return record_launch_error(hipGetLastError(), what);
}

}  // namespace td
