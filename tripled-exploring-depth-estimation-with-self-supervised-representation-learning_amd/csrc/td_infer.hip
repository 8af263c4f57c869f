// Depth inference around the network forward: image -> network input, network disparity -> full-size disparity and depth,
// disparity -> colour picture.  Three memory-bound streams, one launch each:
//   td_infer_preprocess   reference scripts/infer.py:25-30 (float conversion, permute, bilinear resize, /255) and the mirrored
//                         second pass of the flip post-processing
//   td_disp_postprocess   reference scripts/infer.py:41-46 (resize to the image size, disparity -> depth) and
//                         scripts/eval_depth_pp.py:22-28 (batch_post_process_disparity)
//   td_colorize           plt.imsave(..., cmap='magma', vmax=np.percentile(., 95)), scripts/infer.py:65-66
// Every thread owns V consecutive output columns of one row (V * 4 bytes per store: 16 where the row length and the
// pointers allow it), consecutive threads consecutive runs, so a wave writes one contiguous stretch per plane.  The bilinear
// taps are gathers (2 x 2 source pixels per output pixel) and stay scalar loads; their lines are shared by neighbouring
// threads, so each input byte comes from HBM once.  Coordinates follow ATen's upsample_bilinear2d (align_corners=False):
// td::up_index.  The file is compiled with -ffp-contract=off: every product and sum below is rounded on its own.
#include "td_common.h"
#include "td_vec8.h"

namespace td {

template <int V>
__device__ __forceinline__ void store_run(float* p, const float* v) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (V == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  } else {
    p[0] = v[0];
  }
}

template <typename T>      // float, or bf16 bits as unsigned short
__device__ __forceinline__ float as_float(T v) {
  if constexpr (sizeof(T) == 2) return bf2f(v);
  else return v;
}

// ---- image -> network input ----------------------------------------------------------------------------------------------
// img [B,H0,W0,3] uint8 -> out [B*(1+mirror),3,h,w]; thread = V columns x 3 channels of one output row.
template <int V>
__global__ __launch_bounds__(TD_THREADS) void infer_preprocess_kernel(const uint8_t* __restrict__ img, int B, int H0, int W0,
                                                                      int h, int w, int mirror, float ry, float rx,
                                                                      float* __restrict__ out) {
  const int runs = w / V;
  const long long gid = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (gid >= (long long)B * h * runs) return;
  const int xr = (int)(gid % runs), y = (int)((gid / runs) % h), n = (int)(gid / ((long long)runs * h));
  const UpIdx vy = up_index(y, ry, H0);
  const uint8_t* row0 = img + ((size_t)n * H0 + vy.i0) * W0 * 3;
  const uint8_t* row1 = img + ((size_t)n * H0 + vy.i1) * W0 * 3;
  float val[3][V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const UpIdx vx = up_index(xr * V + i, rx, W0);
    const uint8_t *p00 = row0 + vx.i0 * 3, *p01 = row0 + vx.i1 * 3, *p10 = row1 + vx.i0 * 3, *p11 = row1 + vx.i1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float t = vy.l0 * (vx.l0 * (float)p00[c] + vx.l1 * (float)p01[c]) +
                      vy.l1 * (vx.l0 * (float)p10[c] + vx.l1 * (float)p11[c]);
      val[c][i] = t / 255.f;
    }
  }
  const size_t plane = (size_t)h * w;
#pragma unroll
  for (int c = 0; c < 3; ++c) store_run<V>(out + ((size_t)n * 3 + c) * plane + (size_t)y * w + xr * V, val[c]);
  if (mirror) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float rev[V];
#pragma unroll
      for (int i = 0; i < V; ++i) rev[i] = val[c][V - 1 - i];
      store_run<V>(out + ((size_t)(B + n) * 3 + c) * plane + (size_t)y * w + (w - V - xr * V), rev);
    }
  }
}

// ---- network disparity -> full-size disparity and depth ----------------------------------------------------------------------
// l_mask of batch_post_process_disparity at column x of a w-wide map: 1 - clip(20 (x / (w - 1) - 0.05), 0, 1)
__device__ __forceinline__ float left_mask(int x, int w) {
  const float t = 20.f * ((float)x / (float)(w - 1) - 0.05f);
  return 1.f - fminf(fmaxf(t, 0.f), 1.f);
}

// one bilinear tap: the left prediction, or its blend with the un-mirrored right prediction
template <typename T, bool PAIRED>
__device__ __forceinline__ float disp_tap(const T* __restrict__ l, const T* __restrict__ r, int w, int y, int x) {
  const float lv = as_float(l[(size_t)y * w + x]);
  if (!PAIRED) return lv;
  const float rv = as_float(r[(size_t)y * w + (w - 1 - x)]);
  const float lm = left_mask(x, w), rm = left_mask(w - 1 - x, w);
  return rm * lv + lm * rv + (1.f - lm - rm) * (0.5f * (lv + rv));
}

template <typename T, bool PAIRED, int V>
__global__ __launch_bounds__(TD_THREADS) void disp_postprocess_kernel(const T* __restrict__ disp, int B, int h, int w, int H0,
                                                                      int W0, float ry, float rx, float a, float b,
                                                                      float depth_scale, float* __restrict__ disp_out,
                                                                      float* __restrict__ depth_out) {
  const int runs = W0 / V;
  const long long gid = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (gid >= (long long)B * H0 * runs) return;
  const int xr = (int)(gid % runs), y = (int)((gid / runs) % H0), n = (int)(gid / ((long long)runs * H0));
  const T* l = disp + (size_t)n * h * w;
  const T* r = disp + (size_t)(PAIRED ? B + n : n) * h * w;
  const UpIdx vy = up_index(y, ry, h);
  float dv[V], zv[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    const UpIdx vx = up_index(xr * V + i, rx, w);
    const float d = vy.l0 * (vx.l0 * disp_tap<T, PAIRED>(l, r, w, vy.i0, vx.i0) + vx.l1 * disp_tap<T, PAIRED>(l, r, w, vy.i0, vx.i1)) +
                    vy.l1 * (vx.l0 * disp_tap<T, PAIRED>(l, r, w, vy.i1, vx.i0) + vx.l1 * disp_tap<T, PAIRED>(l, r, w, vy.i1, vx.i1));
    dv[i] = d;
    zv[i] = depth_scale / (a * d + b);
  }
  const size_t o = ((size_t)n * H0 + y) * W0 + (size_t)xr * V;
  store_run<V>(disp_out + o, dv);
  if (depth_out) store_run<V>(depth_out + o, zv);
}

// ---- colour map -----------------------------------------------------------------------------------------------------------------
// x [B,n] -> out [B,n,3] through a 256-entry table kept in LDS; thread = V pixels (V = 4: one 16-byte load, one 12-byte store)
template <int V>
__global__ __launch_bounds__(TD_THREADS) void colorize_kernel(const float* __restrict__ x, int B, long long n,
                                                              const float* __restrict__ vmin, const float* __restrict__ vmax,
                                                              const uint8_t* __restrict__ lut, uint8_t* __restrict__ out) {
  __shared__ uint8_t table[768];
  for (int i = threadIdx.x; i < 768; i += TD_THREADS) table[i] = lut[i];
  __syncthreads();
  const long long runs = n / V;
  const long long gid = (long long)blockIdx.x * TD_THREADS + threadIdx.x;
  if (gid >= (long long)B * runs) return;
  const int img = (int)(gid / runs);
  const size_t first = (size_t)img * n + (size_t)(gid % runs) * V;
  const float lo = vmin[img], span = vmax[img] - lo;
  float v[V];
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(x + first);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = x[first];
  }
  uint8_t px[3 * V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    float t = floorf(((v[i] - lo) / span) * 256.f);
    t = fminf(fmaxf(t, 0.f), 255.f);          // (a NaN, 0 / 0 of a constant image, takes entry 0)
    const int idx = (int)t * 3;
    px[3 * i] = table[idx]; px[3 * i + 1] = table[idx + 1]; px[3 * i + 2] = table[idx + 2];
  }
  uint8_t* o = out + first * 3;
  if constexpr (V == 4) {
    unsigned words[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      words[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    unsigned* ow = reinterpret_cast<unsigned*>(o);
    ow[0] = words[0]; ow[1] = words[1]; ow[2] = words[2];
  } else {
    o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
  }
}

}  // namespace td

extern "C" int td_infer_preprocess(const uint8_t* img_u8, int B, int H0, int W0, int h, int w, int mirror, float* out,
                                   td_stream_t stream) {
  if (!img_u8 || !out || B <= 0 || H0 <= 0 || W0 <= 0 || h <= 0 || w <= 0) return TD_ERR_BAD_ARG;
  if (mirror != 0 && mirror != 1) return TD_ERR_BAD_ARG;
  if ((long long)H0 * W0 * 3 > 0x7fffffffLL) return TD_ERR_UNSUPPORTED;      // tap offsets inside one image are ints
  const float ry = (float)H0 / (float)h, rx = (float)W0 / (float)w;
  const int V = (w % 4 == 0 && td::aligned_to(out, 16)) ? 4 : 1;
  const dim3 grid(td::blocks_1d((long long)B * h * (w / V))), block(TD_THREADS);
  if (!grid.x) return TD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (V == 4)
    hipLaunchKernelGGL((td::infer_preprocess_kernel<4>), grid, block, 0, st, img_u8, B, H0, W0, h, w, mirror, ry, rx, out);
  else
    hipLaunchKernelGGL((td::infer_preprocess_kernel<1>), grid, block, 0, st, img_u8, B, H0, W0, h, w, mirror, ry, rx, out);
  return td::record_launch_error(hipGetLastError(), "td_infer_preprocess");
}

template <typename T, bool PAIRED>
static void launch_postprocess(const void* disp, int B, int h, int w, int H0, int W0, float a, float b, float depth_scale,
                               float* disp_out, float* depth_out, int V, hipStream_t st) {
  const float ry = (float)h / (float)H0, rx = (float)w / (float)W0;
  const dim3 grid(td::blocks_1d((long long)B * H0 * (W0 / V))), block(TD_THREADS);      // the caller has checked that it fits
  const T* d = (const T*)disp;
  if (V == 4)
    hipLaunchKernelGGL((td::disp_postprocess_kernel<T, PAIRED, 4>), grid, block, 0, st, d, B, h, w, H0, W0, ry, rx, a, b,
                       depth_scale, disp_out, depth_out);
  else if (V == 2)
    hipLaunchKernelGGL((td::disp_postprocess_kernel<T, PAIRED, 2>), grid, block, 0, st, d, B, h, w, H0, W0, ry, rx, a, b,
                       depth_scale, disp_out, depth_out);
  else
    hipLaunchKernelGGL((td::disp_postprocess_kernel<T, PAIRED, 1>), grid, block, 0, st, d, B, h, w, H0, W0, ry, rx, a, b,
                       depth_scale, disp_out, depth_out);
}

extern "C" int td_disp_postprocess(const void* disp, int dtype, int B, int h, int w, int paired, int H0, int W0, float a,
                                   float b, float depth_scale, float* disp_out, float* depth_out, td_stream_t stream) {
  if (!disp || !disp_out || B <= 0 || h <= 0 || w <= 0 || H0 <= 0 || W0 <= 0) return TD_ERR_BAD_ARG;
  if (paired != 0 && paired != 1) return TD_ERR_BAD_ARG;
  if (dtype != TD_DTYPE_F32 && dtype != TD_DTYPE_BF16) return TD_ERR_UNSUPPORTED;
  if (paired && w < 2) return TD_ERR_UNSUPPORTED;                             // the blend ramp divides by w - 1
  int V = 1;
  for (int cand = 4; cand > 1; cand >>= 1)
    if (W0 % cand == 0 && td::aligned_to(disp_out, 4 * cand) && (!depth_out || td::aligned_to(depth_out, 4 * cand))) {
      V = cand;
      break;
    }
  if (!td::blocks_1d((long long)B * H0 * (W0 / V))) return TD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TD_DTYPE_F32) {
    if (paired) launch_postprocess<float, true>(disp, B, h, w, H0, W0, a, b, depth_scale, disp_out, depth_out, V, st);
    else launch_postprocess<float, false>(disp, B, h, w, H0, W0, a, b, depth_scale, disp_out, depth_out, V, st);
  } else {
    if (paired) launch_postprocess<unsigned short, true>(disp, B, h, w, H0, W0, a, b, depth_scale, disp_out, depth_out, V, st);
    else launch_postprocess<unsigned short, false>(disp, B, h, w, H0, W0, a, b, depth_scale, disp_out, depth_out, V, st);
  }
  return td::record_launch_error(hipGetLastError(), "td_disp_postprocess");
}

extern "C" int td_colorize(const float* x, int B, long long n, const float* vmin, const float* vmax, const uint8_t* lut,
                           uint8_t* out, td_stream_t stream) {
  if (!x || !vmin || !vmax || !lut || !out || B <= 0 || n <= 0) return TD_ERR_BAD_ARG;
  const int V = (n % 4 == 0 && td::aligned_to(x, 16) && td::aligned_to(out, 4)) ? 4 : 1;
  const dim3 grid(td::blocks_1d((long long)B * (n / V))), block(TD_THREADS);
  if (!grid.x) return TD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (V == 4) hipLaunchKernelGGL((td::colorize_kernel<4>), grid, block, 0, st, x, B, n, vmin, vmax, lut, out);
  else hipLaunchKernelGGL((td::colorize_kernel<1>), grid, block, 0, st, x, B, n, vmin, vmax, lut, out);
  return td::record_launch_error(hipGetLastError(), "td_colorize");
}
