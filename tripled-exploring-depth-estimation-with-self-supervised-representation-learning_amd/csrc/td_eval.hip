// KITTI depth evaluation of a batch on the device: the per-image protocol of mono/core/evaluation/eval_hooks.py
// (evaluate_disparity; reference scripts/eval_depth.py:73-101) as a fixed chain of launches, with no host round trip.
//   td_eval_depth      disparity [B,h,w] + padded ground truth [B,Hmax,Wmax] -> [B,8] metrics and [B] pixel counts
//   td_masked_median   np.median over the positive entries of each row of [B,n] (the select of td_eval_depth on its own)
// The chain (10 launches whatever B is):
//   clear         one memset of the select state and the histograms
//   resample      one pass over the padded plane: inside the crop, inside the image and with min < gt < max the scaled disparity is
//                 resized by cv2's INTER_LINEAR definition (coordinate in double, interpolation in float32) and inverted; every
//                 other pixel of the dense workspace gets 0 ("not in the mask": a valid prediction is never 0)
//   3 x (hist, scan)  exact radix select over the float bit patterns (positive floats order like unsigned integers), 11 / 11 / 10
//                 bits per pass, of the prediction and of the ground truth at once.  Each block builds its histograms in LDS and
//                 merges them into the image's global ones with integer atomicAdd (order-independent); a one-block-per-image scan
//                 picks the bin.  np.median of an even count needs ranks (N-1)/2 and N/2, which can part ways at any pass: each
//                 carries its own prefix and its own histogram from the pass after they part (before, the two are equal).
//   sums, finish  every block writes its partial sums (double) and threshold counts (int) to its own slot; one thread per image
//                 adds the slots in a fixed order.  There are no float atomics anywhere: two calls give the same bits.
// The file is compiled with -ffp-contract=off: every product and sum below is rounded on its own, in double as in float.
#include <math.h>

#include "td_common.h"
#include "td_vec8.h"

namespace td {
namespace ev {

constexpr int BINS = 2048;           // 11 bits (the last pass uses 1024 of them)
constexpr int MAX_BLOCKS = 64;       // blocks per image of the hist and sums kernels = partial slots per image
constexpr int ELEMS_PER_BLOCK = TD_THREADS * 8;

// select state of one image (row); slot k = 2 * stream + which: stream 0 = prediction (or the values of td_masked_median),
// stream 1 = ground truth; which 0 = rank (N-1)/2, which 1 = rank N/2
struct RowState {
  int count;
  unsigned prefix[4];                // the bits decided so far, right-aligned
  int rank[4];                       // rank among the elements that share the prefix
  float med[2];
  float scale;                       // med[1] / med[0]
  int pad[4];
};
static_assert(sizeof(RowState) == 64, "RowState layout");

template <typename T>      // float, or bf16 bits as unsigned short
__device__ __forceinline__ float as_float(T v) {
  if constexpr (sizeof(T) == 2) return bf2f(v);
  else return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cv2 INTER_LINEAR source coordinate of output index q (eval_hooks.resize_bilinear): (q + 0.5) * (n_in / n_out) - 0.5 in double,
// floored without clamping at 0, both taps clipped to the border
struct Axis {
  int i0, i1;
  float l0, l1;
};

__device__ __forceinline__ Axis axis_index(int q, double ratio, int n_in) {
  const double s = ((double)q + 0.5) * ratio - 0.5;
  const double f = floor(s);
  const double lam = s - f;
  const int i = (int)f;
  Axis r;
  r.i0 = clampi(i, 0, n_in - 1);
  r.i1 = clampi(i + 1, 0, n_in - 1);
  r.l1 = (float)lam;
  r.l0 = (float)(1.0 - lam);
  return r;
}

// ---- resample and mask ---------------------------------------------------------------------------------------------------------
// grid (blocks, B); pred [B,Hmax*Wmax] is written completely
template <typename T>
__global__ __launch_bounds__(TD_THREADS) void resample_mask_kernel(const T* __restrict__ disp, int h, int w, float a, float b,
                                                                   const float* __restrict__ gt, int Hmax, int Wmax,
                                                                   const int* __restrict__ sizes, const int* __restrict__ crops,
                                                                   float min_depth, float max_depth, float* __restrict__ pred) {
  const int img = blockIdx.y;
  const int P = Hmax * Wmax;
  const int gh = clampi(sizes[2 * img], 0, Hmax), gw = clampi(sizes[2 * img + 1], 0, Wmax);
  const int y0 = clampi(crops[4 * img], 0, gh), y1 = clampi(crops[4 * img + 1], 0, gh);
  const int x0 = clampi(crops[4 * img + 2], 0, gw), x1 = clampi(crops[4 * img + 3], 0, gw);
  const double ry = (double)h / (double)(gh > 0 ? gh : 1), rx = (double)w / (double)(gw > 0 ? gw : 1);
  const T* d = disp + (size_t)img * h * w;
  const float* g = gt + (size_t)img * P;
  float* out = pred + (size_t)img * P;
  for (int i = blockIdx.x * TD_THREADS + threadIdx.x; i < P; i += gridDim.x * TD_THREADS) {
    const int y = i / Wmax, x = i - y * Wmax;
    float v = 0.f;
    if (y >= y0 && y < y1 && x >= x0 && x < x1) {
      const float z = g[i];
      if (z > min_depth && z < max_depth) {
        const Axis vy = axis_index(y, ry, h);
        const Axis vx = axis_index(x, rx, w);
        const T *r0 = d + (size_t)vy.i0 * w, *r1 = d + (size_t)vy.i1 * w;
        // the affine on the four taps first, as the host resizes the scaled disparity; rows first, then columns
        const float t00 = b + a * as_float(r0[vx.i0]), t01 = b + a * as_float(r0[vx.i1]);
        const float t10 = b + a * as_float(r1[vx.i0]), t11 = b + a * as_float(r1[vx.i1]);
        const float c0 = t00 * vy.l0 + t10 * vy.l1;
        const float c1 = t01 * vy.l0 + t11 * vy.l1;
        v = 1.f / (c0 * vx.l0 + c1 * vx.l1);
      }
    }
    out[i] = v;
  }
}

// ---- radix select --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int pass_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int pass_bits(int pass) { return pass == 2 ? 10 : 11; }

// grid (blocks, B); key [B,n]: an entry takes part iff key > 0; stream 0 = key, stream 1 = v1 (NS == 2).
// hist: this pass's [B][2 * NS][BINS] (zero on entry).  Pass 0 fills slot `which = 0` only (the two ranks share it) and counts.
template <int NS>
__global__ __launch_bounds__(TD_THREADS) void hist_kernel(const float* __restrict__ key, const float* __restrict__ v1, long long n,
                                                          int pass, RowState* state, int* hist) {
  __shared__ int lh[2 * NS * BINS];
  __shared__ int wave_count[TD_THREADS / 64];
  const int row = blockIdx.y;
  for (int i = threadIdx.x; i < 2 * NS * BINS; i += TD_THREADS) lh[i] = 0;
  unsigned pre[2 * NS];
#pragma unroll
  for (int k = 0; k < 2 * NS; ++k) pre[k] = state[row].prefix[k];
  __syncthreads();
  const int shift = pass_shift(pass), up = shift + pass_bits(pass);
  const unsigned mask = (1u << pass_bits(pass)) - 1u;
  const float* kr = key + (size_t)row * n;
  const float* vr = NS == 2 ? v1 + (size_t)row * n : nullptr;
  int present = 0;
  for (long long i = (long long)blockIdx.x * TD_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * TD_THREADS) {
    const float k = kr[i];
    if (!(k > 0.f)) continue;
    ++present;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const unsigned bits = __float_as_uint(s == 0 ? k : vr[i]);
      const unsigned bin = (bits >> shift) & mask;
      if (pass == 0) {
        atomicAdd(&lh[(2 * s) * BINS + bin], 1);
      } else {
        const unsigned hi = bits >> up;
        if (hi == pre[2 * s]) atomicAdd(&lh[(2 * s) * BINS + bin], 1);
        if (hi == pre[2 * s + 1]) atomicAdd(&lh[(2 * s + 1) * BINS + bin], 1);
      }
    }
  }
  __syncthreads();
  int* gh = hist + (size_t)row * 2 * NS * BINS;
  for (int i = threadIdx.x; i < 2 * NS * BINS; i += TD_THREADS) {
    const int c = lh[i];
    if (c) atomicAdd(&gh[i], c);
  }
  if (pass == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) present += __shfl_down(present, o, 64);
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = present;
    __syncthreads();
    if (threadIdx.x == 0) {
      int c = 0;
      for (int i = 0; i < TD_THREADS / 64; ++i) c += wave_count[i];
      if (c) atomicAdd(&state[row].count, c);
    }
  }
}

// grid B, block 2 * NS waves: wave k finds the bin of slot k's rank in its histogram and extends the slot's prefix.  After the
// last pass the prefixes are the two middle values themselves: median = 0.5f * (lower + upper), np.median's for float32.
template <int NS>
__global__ __launch_bounds__(128 * NS) void scan_kernel(int pass, RowState* state, const int* __restrict__ hist,
                                                        float* median_out, int* count_out) {
  __shared__ unsigned new_prefix[2 * NS];
  __shared__ int new_rank[2 * NS];
  const int row = blockIdx.x;
  const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
  RowState* st = state + row;
  const int N = st->count;
  const int r = pass == 0 ? ((k & 1) ? N / 2 : (N - 1) / 2) : st->rank[k];
  const unsigned old = pass == 0 ? 0u : st->prefix[k];
  const int nbits = pass_bits(pass);
  const int per = (1 << nbits) / 64;
  const int* hr = hist + ((size_t)row * 2 * NS + (pass == 0 ? (k & ~1) : k)) * BINS + lane * per;
  int sum = 0;
  for (int j = 0; j < per; ++j) sum += hr[j];
  int inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  const int exc = inc - sum;
  if (lane == 0) {                      // N == 0: no lane owns a rank
    new_prefix[k] = old << nbits;
    new_rank[k] = 0;
  }
  __syncthreads();
  if (N > 0 && r >= exc && r < inc) {   // exactly one lane of the wave
    int acc = exc, bin = per - 1;
    for (int j = 0; j < per; ++j) {
      const int c = hr[j];
      if (r < acc + c) {
        bin = j;
        break;
      }
      acc += c;
    }
    new_prefix[k] = (old << nbits) | (unsigned)(lane * per + bin);
    new_rank[k] = r - acc;
  }
  __syncthreads();
  if (threadIdx.x < 2 * NS) {
    st->prefix[threadIdx.x] = new_prefix[threadIdx.x];
    st->rank[threadIdx.x] = new_rank[threadIdx.x];
  }
  if (pass == 2 && threadIdx.x == 0) {
    float med[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      med[s] = N > 0 ? 0.5f * (__uint_as_float(new_prefix[2 * s]) + __uint_as_float(new_prefix[2 * s + 1])) : nanf("");
      st->med[s] = med[s];
    }
    if (NS == 2) st->scale = med[1] / med[0];
    if (median_out) median_out[row] = med[0];
    if (count_out) count_out[row] = N;
  }
}

// ---- the seven metrics ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// grid (blocks, B); block (x, img) writes part_d[img][x][0..3] = sums of |d|/gt, d^2/gt, d^2, (log gt - log pred)^2 and
// part_i[img][x][0..2] = counts of max(gt/pred, pred/gt) < 1.25, 1.25^2, 1.25^3.  Each term is formed in float32 as
// compute_errors forms it (pixel_error.py); only the accumulation is wider.
__global__ __launch_bounds__(TD_THREADS) void sums_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int P,
                                                          const RowState* __restrict__ state, int stereo, float min_depth,
                                                          float max_depth, double* __restrict__ part_d, int* __restrict__ part_i) {
  __shared__ double sd[TD_THREADS / 64][4];
  __shared__ int si[TD_THREADS / 64][3];
  const int img = blockIdx.y;
  const float mult = stereo ? (float)TD_STEREO_SCALE_FACTOR : state[img].scale;
  const float* p = pred + (size_t)img * P;
  const float* g = gt + (size_t)img * P;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int c[3] = {0, 0, 0};
  for (int i = blockIdx.x * TD_THREADS + threadIdx.x; i < P; i += gridDim.x * TD_THREADS) {
    float z = p[i];
    if (!(z > 0.f)) continue;
    const float t = g[i];
    z = z * mult;
    z = fminf(fmaxf(z, min_depth), max_depth);
    const float ratio = fmaxf(t / z, z / t);
    c[0] += ratio < 1.25f;
    c[1] += ratio < 1.5625f;
    c[2] += ratio < 1.953125f;
    const float d = t - z;
    const float d2 = d * d;
    const float dl = (float)log((double)t) - (float)log((double)z);
    s[0] += (double)(fabsf(d) / t);
    s[1] += (double)(d2 / t);
    s[2] += (double)d2;
    s[3] += (double)(dl * dl);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double v = wave_sum_f64(s[j]);
    if (lane == 0) sd[wid][j] = v;
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int v = wave_sum_i32(c[j]);
    if (lane == 0) si[wid][j] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double v = 0.0;
    for (int i = 0; i < TD_THREADS / 64; ++i) v += sd[i][threadIdx.x];
    part_d[((size_t)img * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = v;
  } else if (threadIdx.x < 7) {
    const int j = threadIdx.x - 4;
    int v = 0;
    for (int i = 0; i < TD_THREADS / 64; ++i) v += si[i][j];
    part_i[((size_t)img * gridDim.x + blockIdx.x) * 4 + j] = v;
  }
}

// one thread per image: the slots in order, then abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale
__global__ __launch_bounds__(64) void finish_kernel(const double* __restrict__ part_d, const int* __restrict__ part_i, int slots,
                                                    const RowState* __restrict__ state, int B, float* __restrict__ metrics,
                                                    int* __restrict__ counts) {
  const int img = blockIdx.x * 64 + threadIdx.x;
  if (img >= B) return;
  const int N = state[img].count;
  float* m = metrics + (size_t)img * 8;
  counts[img] = N;
  if (N <= 0) {
    for (int j = 0; j < 8; ++j) m[j] = nanf("");
    return;
  }
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  long long c[3] = {0, 0, 0};
  for (int k = 0; k < slots; ++k) {
    for (int j = 0; j < 4; ++j) s[j] += part_d[((size_t)img * slots + k) * 4 + j];
    for (int j = 0; j < 3; ++j) c[j] += part_i[((size_t)img * slots + k) * 4 + j];
  }
  const double n = (double)N;
  m[0] = (float)(s[0] / n);
  m[1] = (float)(s[1] / n);
  m[2] = (float)sqrt(s[2] / n);
  m[3] = (float)sqrt(s[3] / n);
  for (int j = 0; j < 3; ++j) m[4 + j] = (float)((double)c[j] / n);
  m[7] = state[img].scale;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static inline int blocks_for(long long n) {
  const long long b = (n + ELEMS_PER_BLOCK - 1) / ELEMS_PER_BLOCK;
  return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

static inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }

// workspace of td_eval_depth: [partial doubles][partial ints][state][histograms of the 3 passes][pred]
struct EvalLayout {
  size_t part_d, part_i, state, hist, pred, total, clear_bytes;
};

static inline EvalLayout eval_layout(int B, long long P) {
  EvalLayout l;
  l.part_d = 0;
  l.part_i = l.part_d + (size_t)B * MAX_BLOCKS * 4 * sizeof(double);
  l.state = l.part_i + (size_t)B * MAX_BLOCKS * 4 * sizeof(int);
  l.hist = l.state + (size_t)B * sizeof(RowState);
  l.pred = l.hist + (size_t)3 * B * 4 * BINS * sizeof(int);
  l.clear_bytes = l.pred - l.state;
  l.total = round_up(l.pred + (size_t)B * (size_t)P * sizeof(float), 256);
  return l;
}

// workspace of td_masked_median: [state][histograms of the 3 passes]
static inline size_t median_bytes(int B) { return (size_t)B * sizeof(RowState) + (size_t)3 * B * 2 * BINS * sizeof(int); }

// the three (hist, scan) rounds; `hist` holds 3 x [B][2 * NS][BINS] ints, cleared
template <int NS>
static void launch_select(const float* key, const float* v1, int B, long long n, RowState* state, int* hist, float* median_out,
                          int* count_out, hipStream_t st) {
  const dim3 grid((unsigned)blocks_for(n), (unsigned)B), block(TD_THREADS);
  for (int pass = 0; pass < 3; ++pass) {
    int* h = hist + (size_t)pass * B * 2 * NS * BINS;
    hipLaunchKernelGGL((hist_kernel<NS>), grid, block, 0, st, key, v1, n, pass, state, h);
    hipLaunchKernelGGL((scan_kernel<NS>), dim3((unsigned)B), dim3(128 * NS), 0, st, pass, state, (const int*)h, median_out,
                       count_out);
  }
}

}  // namespace ev
}  // namespace td

extern "C" long long td_eval_depth_workspace_bytes(int B, int Hmax, int Wmax) {
  if (B <= 0 || Hmax <= 0 || Wmax <= 0 || B > 65535 || (long long)Hmax * Wmax > (1LL << 30)) return 0;
  return (long long)td::ev::eval_layout(B, (long long)Hmax * Wmax).total;
}

extern "C" long long td_masked_median_workspace_bytes(int B) {
  if (B <= 0 || B > 65535) return 0;
  return (long long)td::ev::median_bytes(B);
}

extern "C" int td_eval_depth(const void* disp, int dtype, int B, int h, int w, float a, float b, const float* gt, int Hmax, int Wmax,
                             const int* sizes, const int* crops, float min_depth, float max_depth, int stereo, void* workspace,
                             long long workspace_bytes, float* metrics, int* counts, td_stream_t stream) {
  using namespace td::ev;
  if (!disp || !gt || !sizes || !crops || !workspace || !metrics || !counts) return TD_ERR_BAD_ARG;
  if (B <= 0 || h <= 0 || w <= 0 || Hmax <= 0 || Wmax <= 0) return TD_ERR_BAD_ARG;
  if (!(min_depth >= 0.f) || !(max_depth > min_depth) || (stereo != 0 && stereo != 1)) return TD_ERR_BAD_ARG;
  if (!td::aligned_to(workspace, 8)) return TD_ERR_BAD_ARG;
  if (dtype != TD_DTYPE_F32 && dtype != TD_DTYPE_BF16) return TD_ERR_UNSUPPORTED;
  const long long P = (long long)Hmax * Wmax;
  if (B > 65535 || P > (1LL << 30) || (long long)h * w > (1LL << 30)) return TD_ERR_UNSUPPORTED;
  const EvalLayout l = eval_layout(B, P);
  if (workspace_bytes < (long long)l.total) return TD_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  double* part_d = reinterpret_cast<double*>(ws + l.part_d);
  int* part_i = reinterpret_cast<int*>(ws + l.part_i);
  RowState* state = reinterpret_cast<RowState*>(ws + l.state);
  int* hist = reinterpret_cast<int*>(ws + l.hist);
  float* pred = reinterpret_cast<float*>(ws + l.pred);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws + l.state, 0, l.clear_bytes, st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_eval_depth (clear)");
  const int blocks = blocks_for(P);
  const dim3 grid((unsigned)blocks, (unsigned)B), block(TD_THREADS);
  // the resample pass has no LDS to fill: more, shorter blocks
  const long long rb = (P + TD_THREADS * 4 - 1) / (TD_THREADS * 4);
  const dim3 rgrid((unsigned)(rb > 1024 ? 1024 : rb), (unsigned)B);
  if (dtype == TD_DTYPE_F32)
    hipLaunchKernelGGL((resample_mask_kernel<float>), rgrid, block, 0, st, (const float*)disp, h, w, a, b, gt, Hmax, Wmax, sizes,
                       crops, min_depth, max_depth, pred);
  else
    hipLaunchKernelGGL((resample_mask_kernel<unsigned short>), rgrid, block, 0, st, (const unsigned short*)disp, h, w, a, b, gt, Hmax,
                       Wmax, sizes, crops, min_depth, max_depth, pred);
  launch_select<2>(pred, gt, B, P, state, hist, nullptr, nullptr, st);
  hipLaunchKernelGGL(sums_kernel, grid, block, 0, st, (const float*)pred, gt, (int)P, (const RowState*)state, stereo, min_depth,
                     max_depth, part_d, part_i);
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const double*)part_d, (const int*)part_i,
                     blocks, (const RowState*)state, B, metrics, counts);
  return td::record_launch_error(hipGetLastError(), "td_eval_depth");
}

extern "C" int td_masked_median(const float* values, int B, long long n, void* workspace, long long workspace_bytes, float* median,
                                int* count, td_stream_t stream) {
  using namespace td::ev;
  if (!values || !workspace || !median || !count || B <= 0 || n <= 0) return TD_ERR_BAD_ARG;
  if (!td::aligned_to(workspace, 4)) return TD_ERR_BAD_ARG;
  if (B > 65535 || n > 0x7fffffffLL) return TD_ERR_UNSUPPORTED;
  if (workspace_bytes < (long long)median_bytes(B)) return TD_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  RowState* state = reinterpret_cast<RowState*>(ws);
  int* hist = reinterpret_cast<int*>(ws + (size_t)B * sizeof(RowState));
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(ws, 0, median_bytes(B), st);
  if (e != hipSuccess) return td::record_launch_error(e, "td_masked_median (clear)");
  launch_select<1>(values, nullptr, B, n, state, hist, median, count, st);
  return td::record_launch_error(hipGetLastError(), "td_masked_median");
}
