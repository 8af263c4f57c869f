// Multi-view consistency of a sequence's depth maps (tripled_amd/cloud.py: views_numpy is the statement):
//   td_cloud_views   per pixel of a centre frame, the number of neighbouring frames that, reprojected, see the same depth there;
//                    optionally the removal of the pixels with too few such frames from the (key, payload) pairs of td_cloud_keys
// One launch, plain vector stores, no kernel waits on another workgroup.  A workgroup works on pixels of ONE centre frame, so the
// frame numbers of the centre and of its neighbours are wave-uniform and their 12 pose doubles are scalar loads.  Offsets inside a
// frame are 32-bit (a frame is at most 2^29 pixels); only the frame's base is a 64-bit, wave-uniform address.  The file is built
// with -ffp-contract=off and contains no fma: every float64 product, sum and quotient is rounded on its own, as numpy rounds it.
#include <math.h>

#include "td_grid.h"
#include "td_pixel.h"

namespace td {

#define TD_VIEWS_MAX_PLANE (1LL << 29)             // pixels of a frame: byte offsets inside it fit 32 bits

struct CloudViewArgs {
  const float* depth;          // [N,H,W]
  const double* poses;         // [N,3,4] camera-to-world
  double k[9], ik[9];          // the 3x3 blocks of K and of inv_K, row-major
  int N, H, W, c0, c1, lo, hi, radius, min_views;
  unsigned blocks_per_frame;
  double tol, depth_scale, pose_scale, min_depth, max_range;
  long long* key;              // [(c1-c0)*H*W] (in/out) or NULL
  unsigned long long* payload; // [(c1-c0)*H*W] (in/out) or NULL, with key
  uint8_t* votes;              // [(c1-c0)*H*W] (out) or NULL
  unsigned long long* stats;   // [2] or NULL: += pixels tested, pixels dropped
};

__device__ __forceinline__ bool view_depth_ok(float d, double ds, double min_depth, double max_range) {
  return isfinite(d) && ds >= min_depth && ds <= max_range;
}

// pixel `pixel` of a frame: a 32-bit byte offset from the wave-uniform frame base
__device__ __forceinline__ float view_tap(const float* __restrict__ frame, unsigned pixel) { return ld_at(frame, pixel * 4u); }

__global__ __launch_bounds__(TD_THREADS) void cloud_views_kernel(const CloudViewArgs a) {
  __shared__ unsigned cnt[2];
  if (a.stats) counters_begin<2>(cnt);
  const int H = a.H, W = a.W;
  const unsigned plane = (unsigned)H * (unsigned)W;
  const unsigned ci = blockIdx.x / a.blocks_per_frame;                                    // wave-uniform: the centre's number
  const unsigned pix = (blockIdx.x - ci * a.blocks_per_frame) * TD_THREADS + threadIdx.x;
  const int i = a.c0 + (int)ci;
  bool tested = false, dropped = false;
  if (pix < plane) {
    const long long out = (long long)ci * plane + pix;
    tested = a.key ? a.key[out] != TD_KEY_INVALID : true;
    int n = 0;
    if (tested) {
      const float* __restrict__ centre = a.depth + (long long)i * plane;
      const float d = view_tap(centre, pix);
      const double ds = (double)d * a.depth_scale;
      if (view_depth_ok(d, ds, a.min_depth, a.max_range)) {
        const unsigned y = pix / (unsigned)W, x = pix - y * (unsigned)W;
        double r0, r1, r2;
        pixel_ray(a.ik, (double)x, (double)y, r0, r1, r2);
        const double px = ds * r0, py = ds * r1, pz = ds * r2;
        double wx, wy, wz;
        camera_to_world(a.poses + (long long)i * 12, a.pose_scale, px, py, pz, wx, wy, wz);
        int first = i - a.radius;                      // the window is shifted, not shortened, at the ends of [lo, hi)
        first = first < a.lo ? a.lo : first;
        first = first > a.hi - 1 - 2 * a.radius ? a.hi - 1 - 2 * a.radius : first;
        const double umax = (double)(W - 1), vmax = (double)(H - 1);
        for (int j = first; j <= first + 2 * a.radius; ++j) {      // wave-uniform
          if (j == i) continue;
          const double* __restrict__ Pj = a.poses + (long long)j * 12;
          const double ex = wx - a.pose_scale * Pj[3], ey = wy - a.pose_scale * Pj[7], ez = wz - a.pose_scale * Pj[11];
          const double qx = (Pj[0] * ex + Pj[4] * ey) + Pj[8] * ez;      // the transpose of the rotation: the stated inverse
          const double qy = (Pj[1] * ex + Pj[5] * ey) + Pj[9] * ez;
          const double z = (Pj[2] * ex + Pj[6] * ey) + Pj[10] * ez;
          const double X = (a.k[0] * qx + a.k[1] * qy) + a.k[2] * z;
          const double Y = (a.k[3] * qx + a.k[4] * qy) + a.k[5] * z;
          const double uj = X / z, vj = Y / z;
          if (!(z > 0.0 && uj >= 0.0 && uj <= umax && vj >= 0.0 && vj <= vmax)) continue;      // a NaN fails
          int x0 = (int)floor(uj), y0 = (int)floor(vj);           // in [0, W-1] x [0, H-1]: the conversion is exact
          x0 = x0 > W - 2 ? W - 2 : x0;
          y0 = y0 > H - 2 ? H - 2 : y0;
          const double fx = uj - (double)x0, fy = vj - (double)y0;
          const float* __restrict__ frame = a.depth + (long long)j * plane;
          const unsigned at = (unsigned)y0 * (unsigned)W + (unsigned)x0;      // at + W + 1 <= plane - 1
          const float d00 = view_tap(frame, at), d01 = view_tap(frame, at + 1u);
          const float d10 = view_tap(frame, at + (unsigned)W), d11 = view_tap(frame, at + (unsigned)W + 1u);
          const double t00 = (double)d00 * a.depth_scale, t01 = (double)d01 * a.depth_scale;
          const double t10 = (double)d10 * a.depth_scale, t11 = (double)d11 * a.depth_scale;
          if (!(view_depth_ok(d00, t00, a.min_depth, a.max_range) && view_depth_ok(d01, t01, a.min_depth, a.max_range) &&
                view_depth_ok(d10, t10, a.min_depth, a.max_range) && view_depth_ok(d11, t11, a.min_depth, a.max_range)))
            continue;
          const double top = t00 + fx * (t01 - t00);
          const double bot = t10 + fx * (t11 - t10);
          const double s = top + fy * (bot - top);
          if (fabs(z - s) <= a.tol * fmin(z, s)) n += 1;
        }
      }
      if (n < a.min_views) {
        dropped = true;
        if (a.key) {
          a.key[out] = TD_KEY_INVALID;
          a.payload[out] = 0ULL;
        }
      }
    }
    if (a.votes) a.votes[out] = (uint8_t)n;
  }
  if (a.stats) {
    const unsigned long long bt = __ballot(tested), bd = __ballot(dropped);
    if ((threadIdx.x & 63) == 0) {
      if (bt) atomicAdd(&cnt[0], (unsigned)__popcll(bt));      // LDS
      if (bd) atomicAdd(&cnt[1], (unsigned)__popcll(bd));
    }
    counters_end<2>(cnt, a.stats);
  }
}

}  // namespace td

// ---------------------------------------------------------------------------------------------------------------------------

extern "C" int td_cloud_views(const float* depth, const double* poses, const double* K, const double* inv_K, int N, int H, int W, int c0,
                              int c1, int lo, int hi, int radius, int min_views, double tol, double depth_scale, double pose_scale,
                              double min_depth, double max_range, long long* key, unsigned long long* payload, uint8_t* votes,
                              long long* stats, td_stream_t stream) {
  if (!depth || !poses || !K || !inv_K || (key == nullptr) != (payload == nullptr) || (!key && !votes) || N < 0 || H < 2 || W < 2 ||
      radius < 1 || radius > TD_VIEWS_MAX_RADIUS || min_views < 0 || min_views > 2 * radius || !(tol >= 0.0) || lo < 0 || hi < lo ||
      hi > N || c0 < lo || c1 < c0 || c1 > hi)
    return TD_ERR_BAD_ARG;
  if (N == 0 || c0 == c1) return TD_OK;
  if (hi - lo < 2 * radius + 1) return TD_ERR_BAD_ARG;      // every centre has 2 radius neighbours inside [lo, hi)
  const long long plane = (long long)H * W;
  if (plane > TD_VIEWS_MAX_PLANE) return TD_ERR_UNSUPPORTED;
  const long long per_frame = (plane + TD_THREADS - 1) / TD_THREADS;
  const long long blocks = per_frame * (c1 - c0);
  if (blocks > 0x7fffffffLL) return TD_ERR_UNSUPPORTED;
  td::CloudViewArgs a;
  a.depth = depth; a.poses = poses;
  for (int k = 0; k < 9; ++k) { a.k[k] = K[k]; a.ik[k] = inv_K[k]; }
  a.N = N; a.H = H; a.W = W; a.c0 = c0; a.c1 = c1; a.lo = lo; a.hi = hi; a.radius = radius; a.min_views = min_views;
  a.blocks_per_frame = (unsigned)per_frame;
  a.tol = tol; a.depth_scale = depth_scale; a.pose_scale = pose_scale; a.min_depth = min_depth; a.max_range = max_range;
  a.key = key; a.payload = payload; a.votes = votes; a.stats = reinterpret_cast<unsigned long long*>(stats);
  hipLaunchKernelGGL(td::cloud_views_kernel, dim3((unsigned)blocks), dim3(TD_THREADS), 0, (hipStream_t)stream, a);
  return td::record_launch_error(hipGetLastError(), "td_cloud_views");
}
