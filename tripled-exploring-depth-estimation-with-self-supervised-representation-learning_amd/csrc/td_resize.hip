// Image.resize((W, H), LANCZOS) and Image.transpose(FLIP_LEFT_RIGHT) of uint8 frames on the device, bit-equal to Pillow's 8-bit
// resampler.  Replaces, for the "raw_u8" wire format, MonoDataset's per-frame resize and flip in the loader workers (reference:
// mono/datasets/mono_dataset.py:60-63 `transforms.Resize(..., interpolation=Image.ANTIALIAS)`, :129-143 `color.transpose(...)`).
//
// The arithmetic is Pillow's (Resample.c: ImagingResampleHorizontal_8bpc, then ..Vertical_8bpc): per pass
//   out = clamp((2^21 + sum_t k[t] * pixel[min + t]) >> 22, 0, 255),  int32 accumulation, a uint8 image between the passes,
// with the 22-bit fixed-point coefficient tables built on the host in float64 (tripled_amd/resize.py: lanczos_coeffs).  A pass that
// Pillow skips (equal sizes) arrives as the one-tap identity table, which returns the input byte exactly.
//
// ONE launch.  A 256-thread block owns (image, channel, band of `band` output rows).  The source rows the band needs -- rows
// [r0, r1) by the vertical bounds of its first and last row -- are resampled horizontally into an LDS tile of uint8 [r1 - r0][W],
// eight source rows at a time: the rows are staged in LDS with aligned dword loads (a row of a 1242-wide canvas starts on any byte,
// so the staged row keeps its 0..3 byte phase), then a thread takes one output column and all eight rows: one coefficient load
// (table transposed to [tap][column]: consecutive lanes, consecutive ints) feeds eight LDS byte reads (lanes two bytes apart share
// dwords: broadcast, no bank conflict) and eight 24-bit multiply-adds.  The flip reads the staged row at w - 1 - column.  The vertical
// pass reads the tile four columns at a time (one dword per tap, conflict-free) and stores four packed bytes.  The band is the
// largest of 16, 8, 4, 2, 1 rows whose tile fits 48 KiB of LDS with the staging rows: 44 x 640 + 8 x 1252 bytes = 38 KiB at
// 375x1242 -> 192x640, where the horizontal pass runs 1.4 times (bands overlap by the vertical support).
// Only the top-left (h, w) of a canvas enters a result.  The kernel does not rely on the tables for that: source columns are clamped to
// [0, w - 1] and source rows to [r0, min(.., h)) against the sizes in the launch arguments, which the entry point checks against the
// canvas, so tables of another size give wrong bytes inside the valid region at worst, never a read outside it.
//
// Two entry points share the body through a small address functor.  td_lanczos_resize_u8 reads canvases [N,3,Hc,Wc].
// td_lanczos_resize_u8_indexed (the "resident" wire format) reads planar frames [3,h,w] with tight rows at per-image int64 byte offsets
// of one store: rows of odd width start on every byte phase, which the dword staging already carries, and the byte-wise tail is that of
// the store.  An offset whose frame would leave the store is refused by the block before it reads anything (status 3, zero-filled).
#include "td_common.h"

#include <algorithm>
#include <climits>

namespace td {

struct ResizeDesc { int h, w, ksx, ksy, off_kx, off_bx, off_ky, off_by; };
struct ResizeBank { ResizeDesc d[TD_RESIZE_MAX_SIZES]; };       // by value in the kernel arguments (512 bytes)

constexpr int RS_ROWS = 8;                   // source rows staged and resampled per round
constexpr int RS_THREADS = 256;
constexpr int RS_LDS_BUDGET = 48 * 1024;
constexpr int RS_HALF = 1 << 21;             // 2^(PRECISION_BITS - 1)

__device__ __forceinline__ unsigned clip8(int acc) {
  const int v = acc >> 22;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ void zero_band(uint8_t* __restrict__ out, int y0, int y1, int W) {
  const int n = (y1 - y0) * W;
  for (int i = threadIdx.x; i < n; i += RS_THREADS) out[(size_t)y0 * W + i] = 0;
}

// Where image n, channel c lies.  ``locate`` gives the valid size (h, w), the byte offset of the plane in ``src`` and its row stride;
// false: the image cannot be read (zero-filled, status 3).  Everything after it is shared by the two entry points.
struct CanvasSource {                        // td_lanczos_resize_u8: [N,3,Hc,Wc], the image in the top-left of its canvas
  int Hc, Wc;
  __device__ __forceinline__ bool locate(int n, int c, const ResizeDesc& d, int& h, int& w, size_t& plane, int& stride) const {
    h = min(d.h, Hc);
    w = min(d.w, Wc);
    plane = (size_t)(n * 3 + c) * Hc * Wc;
    stride = Wc;
    return true;
  }
};

struct StoreSource {                         // td_lanczos_resize_u8_indexed: planar [3,h,w] at offsets[n] of a byte store, rows tight
  const long long* __restrict__ offsets;
  long long bytes;
  __device__ __forceinline__ bool locate(int n, int c, const ResizeDesc& d, int& h, int& w, size_t& plane, int& stride) const {
    h = d.h;
    w = d.w;
    stride = d.w;
    const long long off = offsets[n];
    const long long frame = 3ll * d.h * d.w;
    plane = 0;
    if (off < 0 || frame > bytes || off > bytes - frame) return false;       // the frame would leave the store: nothing is read
    plane = (size_t)off + (size_t)c * d.h * d.w;
    return true;
  }
};

template <class Source>
__device__ __forceinline__ void lanczos_resize_body(unsigned char* lds, const uint8_t* __restrict__ src, const Source source,
                                                    const int* __restrict__ meta, const int* __restrict__ tables, const ResizeBank& bank,
                                                    int n_sizes, int H, int W, int band, int span_max, int Wp, int SW,
                                                    long long total_bytes, int packed_store, uint8_t* __restrict__ dst,
                                                    int* __restrict__ status) {
  unsigned char* stage = lds;                        // [RS_ROWS][SW]: source rows, each at its byte phase
  unsigned char* tile = lds + RS_ROWS * SW;          // [span_max][Wp]: horizontally resampled rows r0 ...
  const int n = blockIdx.z, c = blockIdx.y;
  const int y0 = blockIdx.x * band;
  const int y1 = min(y0 + band, H);
  uint8_t* out = dst + (size_t)(n * 3 + c) * H * W;
  const int s = __builtin_amdgcn_readfirstlane(meta[2 * n]);
  const bool flip = __builtin_amdgcn_readfirstlane(meta[2 * n + 1]) != 0;
  if (s < 0 || s >= n_sizes) {                       // a size index outside the bank: no table to apply
    zero_band(out, y0, y1, W);
    if (threadIdx.x == 0) status[0] = 1;
    return;
  }
  const ResizeDesc d = bank.d[s];
  int h, w, stride;
  size_t plane;
  if (!source.locate(n, c, d, h, w, plane, stride)) {
    zero_band(out, y0, y1, W);
    if (threadIdx.x == 0) status[0] = 3;
    return;
  }
  const int* __restrict__ kxT = tables + d.off_kx;   // [ksx][W]
  const int* __restrict__ bx = tables + d.off_bx;    // [W][2]
  const int* __restrict__ ky = tables + d.off_ky;    // [H][ksy]
  const int* __restrict__ by = tables + d.off_by;    // [H][2]
  const int r0 = __builtin_amdgcn_readfirstlane(by[2 * y0]);
  const int r1 = min(__builtin_amdgcn_readfirstlane(by[2 * (y1 - 1)] + by[2 * (y1 - 1) + 1]), h);
  if (r0 < 0 || r1 - r0 > span_max) {                // tables that do not belong to these sizes: the tile would not hold the band
    zero_band(out, y0, y1, W);
    if (threadIdx.x == 0) status[0] = 2;
    return;
  }
  const int DW = SW >> 2;
  const uint32_t* __restrict__ src32 = reinterpret_cast<const uint32_t*>(src);

  for (int rs = r0; rs < r1; rs += RS_ROWS) {
    const int nr = min(RS_ROWS, r1 - rs);
    // ---- stage nr source rows: aligned dwords covering [base, base + w) of each row
    for (int idx = threadIdx.x; idx < nr * DW; idx += RS_THREADS) {
      const int r = idx / DW, j = idx - r * DW;
      const size_t base = plane + (size_t)(rs + r) * stride;
      const int ndw = ((int)(base & 3) + w + 3) >> 2;
      if (j >= ndw) continue;
      const size_t di = (base >> 2) + j;
      uint32_t v = 0;
      if ((long long)(di + 1) * 4 <= total_bytes) {
        v = src32[di];
      } else {                                        // the last 1..3 bytes of the whole array
        for (int b = 0; b < 4; ++b)
          if ((long long)(di * 4 + b) < total_bytes) v |= (uint32_t)src[di * 4 + b] << (8 * b);
      }
      reinterpret_cast<uint32_t*>(stage)[r * DW + j] = v;
    }
    __syncthreads();
    // ---- horizontal pass: one thread = one output column x all staged rows
    int roff[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) roff[r] = r * SW + (int)((plane + (size_t)(rs + r) * stride) & 3);
    for (int x = threadIdx.x; x < W; x += RS_THREADS) {
      const int xmin = bx[2 * x], cnt = min(bx[2 * x + 1], d.ksx);
      int acc[RS_ROWS];
#pragma unroll
      for (int r = 0; r < RS_ROWS; ++r) acc[r] = RS_HALF;
      for (int t = 0; t < cnt; ++t) {
        const int k = kxT[t * W + x];
        int col = xmin + t;
        col = flip ? w - 1 - col : col;
        col = min(max(col, 0), w - 1);
#pragma unroll
        for (int r = 0; r < RS_ROWS; ++r) acc[r] += __mul24(k, (int)stage[roff[r] + col]);
      }
      unsigned char* trow = tile + (rs - r0) * Wp + x;
#pragma unroll
      for (int r = 0; r < RS_ROWS; ++r)
        if (r < nr) trow[r * Wp] = (unsigned char)clip8(acc[r]);
    }
    __syncthreads();
  }

  // ---- vertical pass from the tile: four columns per thread
  const int G = Wp >> 2;
  const int span = r1 - r0;
  for (int idx = threadIdx.x; idx < (y1 - y0) * G; idx += RS_THREADS) {
    const int yy = idx / G, xg = idx - yy * G;
    const int y = y0 + yy;
    const int ymin = by[2 * y];
    const int first = min(max(ymin - r0, 0), span);
    const int cnt = min(min(by[2 * y + 1], d.ksy), span - first);
    const uint32_t* col = reinterpret_cast<const uint32_t*>(tile) + first * G + xg;
    const int* __restrict__ kk = ky + y * d.ksy;
    int a0 = RS_HALF, a1 = RS_HALF, a2 = RS_HALF, a3 = RS_HALF;
    for (int t = 0; t < cnt; ++t) {
      const int k = kk[t];
      const uint32_t p = col[t * G];
      a0 += __mul24(k, (int)(p & 255u));
      a1 += __mul24(k, (int)((p >> 8) & 255u));
      a2 += __mul24(k, (int)((p >> 16) & 255u));
      a3 += __mul24(k, (int)(p >> 24));
    }
    const unsigned b0 = clip8(a0), b1 = clip8(a1), b2 = clip8(a2), b3 = clip8(a3);
    const int x = xg * 4;
    uint8_t* o = out + (size_t)y * W + x;
    if (packed_store) {
      *reinterpret_cast<uint32_t*>(o) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
      if (x < W) o[0] = (uint8_t)b0;
      if (x + 1 < W) o[1] = (uint8_t)b1;
      if (x + 2 < W) o[2] = (uint8_t)b2;
      if (x + 3 < W) o[3] = (uint8_t)b3;
    }
  }
}

__global__ __launch_bounds__(RS_THREADS) void lanczos_resize_kernel(const uint8_t* __restrict__ src, const int* __restrict__ meta,
                                                                    const int* __restrict__ tables, const ResizeBank bank, int n_sizes,
                                                                    int Hc, int Wc, int H, int W, int band, int span_max, int Wp, int SW,
                                                                    long long total_bytes, int packed_store, uint8_t* __restrict__ dst,
                                                                    int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char lds[];
  lanczos_resize_body(lds, src, CanvasSource{Hc, Wc}, meta, tables, bank, n_sizes, H, W, band, span_max, Wp, SW, total_bytes,
                      packed_store, dst, status);
}

__global__ __launch_bounds__(RS_THREADS) void lanczos_resize_indexed_kernel(const uint8_t* __restrict__ store, long long store_bytes,
                                                                            const long long* __restrict__ offsets,
                                                                            const int* __restrict__ meta, const int* __restrict__ tables,
                                                                            const ResizeBank bank, int n_sizes, int H, int W, int band,
                                                                            int span_max, int Wp, int SW, int packed_store,
                                                                            uint8_t* __restrict__ dst, int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char lds[];
  lanczos_resize_body(lds, store, StoreSource{offsets, store_bytes}, meta, tables, bank, n_sizes, H, W, band, span_max, Wp, SW,
                      store_bytes, packed_store, dst, status);
}

// The launch geometry both entry points share.  ``h_max`` x ``w_max`` bounds every source the launch can meet (the canvas, or the
// largest size of the bank): the staging rows are as wide as w_max, and no band needs more tile rows than h_max.
struct ResizePlan { ResizeBank bank; int band, span_max, Wp, SW, bands; size_t lds; };

static int plan_resize(const int* desc, int n_sizes, long long table_ints, int H, int W, int h_limit, int w_limit, int* h_max, int* w_max,
                       ResizePlan* plan) {
  if (n_sizes < 1 || n_sizes > TD_RESIZE_MAX_SIZES) return TD_ERR_BAD_ARG;
  plan->bank = {};
  double max_scale_y = 0.0;
  int max_ksy = 1, hm = 0, wm = 0;
  for (int i = 0; i < n_sizes; ++i) {
    ResizeDesc& d = plan->bank.d[i];
    const int* p = desc + 8 * i;
    d.h = p[0]; d.w = p[1]; d.ksx = p[2]; d.ksy = p[3]; d.off_kx = p[4]; d.off_bx = p[5]; d.off_ky = p[6]; d.off_by = p[7];
    if (d.h < 1 || d.w < 1 || d.h > h_limit || d.w > w_limit || d.ksx < 1 || d.ksy < 1) return TD_ERR_BAD_ARG;   // a size larger than the canvas
    if (d.off_kx < 0 || d.off_bx < 0 || d.off_ky < 0 || d.off_by < 0) return TD_ERR_BAD_ARG;
    if ((long long)d.off_kx + (long long)d.ksx * W > table_ints || (long long)d.off_bx + 2ll * W > table_ints ||
        (long long)d.off_ky + (long long)d.ksy * H > table_ints || (long long)d.off_by + 2ll * H > table_ints)
      return TD_ERR_BAD_ARG;
    const double sy = (double)d.h / (double)H;
    if (sy > max_scale_y) max_scale_y = sy;
    if (d.ksy > max_ksy) max_ksy = d.ksy;
    if (d.h > hm) hm = d.h;
    if (d.w > wm) wm = d.w;
  }
  if (*h_max <= 0) *h_max = hm;
  if (*w_max <= 0) *w_max = wm;
  if ((long long)H * W >= (1ll << 30) || (long long)*h_max * *w_max >= (1ll << 30)) return TD_ERR_UNSUPPORTED;
  plan->Wp = (W + 3) & ~3;
  plan->SW = ((*w_max + 3) & ~3) + 8;
  // rows of the tile a band needs: the first rows of its first and last output row lie <= ceil((band - 1) scale) + 1 apart, the
  // last row adds its taps
  plan->band = 0;
  plan->span_max = 0;
  for (int b = 16; b >= 1; b >>= 1) {
    long long span = (long long)ceil((double)(b - 1) * max_scale_y) + 1 + max_ksy;
    if (span > *h_max) span = *h_max;
    if ((long long)RS_ROWS * plan->SW + span * plan->Wp <= RS_LDS_BUDGET) { plan->band = b; plan->span_max = (int)span; break; }
  }
  if (plan->band == 0) return TD_ERR_UNSUPPORTED;    // rows too wide for the tile
  plan->bands = (H + plan->band - 1) / plan->band;
  if (plan->bands > 65535) return TD_ERR_UNSUPPORTED;
  plan->lds = (size_t)RS_ROWS * plan->SW + (size_t)plan->span_max * plan->Wp;
  return TD_OK;
}

}  // namespace td

extern "C" int td_lanczos_resize_u8(const uint8_t* src, const int* meta, const int* meta_host, const int* tables, long long table_ints,
                                    const int* desc, int n_sizes, int N, int Hc, int Wc, int H, int W, uint8_t* dst, int* status,
                                    td_stream_t stream) {
  if (!src || !meta || !tables || !desc || !dst || !status || N <= 0 || Hc <= 0 || Wc <= 0 || H <= 0 || W <= 0 || table_ints <= 0)
    return TD_ERR_BAD_ARG;
  if (n_sizes < 1 || n_sizes > TD_RESIZE_MAX_SIZES) return TD_ERR_BAD_ARG;
  if (meta_host)
    for (int n = 0; n < N; ++n)
      if (meta_host[2 * n] < 0 || meta_host[2 * n] >= n_sizes) return TD_ERR_BAD_ARG;
  td::ResizePlan plan;
  int h_max = Hc, w_max = Wc;
  const int rc = td::plan_resize(desc, n_sizes, table_ints, H, W, Hc, Wc, &h_max, &w_max, &plan);
  if (rc == TD_ERR_BAD_ARG) return rc;
  if (!td::aligned_to(src, 4) || N > 65535) return TD_ERR_UNSUPPORTED;
  if (rc != TD_OK) return rc;
  const long long total = (long long)N * 3 * Hc * Wc;
  const int packed = ((W & 3) == 0 && td::aligned_to(dst, 4)) ? 1 : 0;
  hipLaunchKernelGGL(td::lanczos_resize_kernel, dim3(plan.bands, 3, N), dim3(td::RS_THREADS), plan.lds, (hipStream_t)stream, src, meta,
                     tables, plan.bank, n_sizes, Hc, Wc, H, W, plan.band, plan.span_max, plan.Wp, plan.SW, total, packed, dst, status);
  return td::record_launch_error(hipGetLastError(), "td_lanczos_resize_u8");
}

extern "C" int td_lanczos_resize_u8_indexed(const uint8_t* store, long long store_bytes, const long long* offsets,
                                            const long long* offsets_host, const int* meta, const int* meta_host, const int* tables,
                                            long long table_ints, const int* desc, int n_sizes, int N, int H, int W, uint8_t* dst,
                                            int* status, td_stream_t stream) {
  if (!store || !offsets || !meta || !tables || !desc || !dst || !status || store_bytes <= 0 || N <= 0 || H <= 0 || W <= 0 ||
      table_ints <= 0)
    return TD_ERR_BAD_ARG;
  if (n_sizes < 1 || n_sizes > TD_RESIZE_MAX_SIZES) return TD_ERR_BAD_ARG;
  if (meta_host)
    for (int n = 0; n < N; ++n)
      if (meta_host[2 * n] < 0 || meta_host[2 * n] >= n_sizes) return TD_ERR_BAD_ARG;
  td::ResizePlan plan;
  int h_max = 0, w_max = 0;                          // no canvas: the largest size of the bank
  const int rc = td::plan_resize(desc, n_sizes, table_ints, H, W, INT_MAX, INT_MAX, &h_max, &w_max, &plan);
  if (rc == TD_ERR_BAD_ARG) return rc;
  if (offsets_host) {
    // with the size indices the whole frame is checked; without them, the smallest frame of the bank (a necessary condition)
    long long least = LLONG_MAX;
    for (int i = 0; i < n_sizes; ++i) least = std::min(least, 3ll * plan.bank.d[i].h * plan.bank.d[i].w);
    for (int n = 0; n < N; ++n) {
      const long long frame = meta_host ? 3ll * plan.bank.d[meta_host[2 * n]].h * plan.bank.d[meta_host[2 * n]].w : least;
      if (offsets_host[n] < 0 || frame > store_bytes || offsets_host[n] > store_bytes - frame) return TD_ERR_BAD_ARG;
    }
  }
  if (!td::aligned_to(store, 4) || N > 65535) return TD_ERR_UNSUPPORTED;
  if (rc != TD_OK) return rc;
  const int packed = ((W & 3) == 0 && td::aligned_to(dst, 4)) ? 1 : 0;
  hipLaunchKernelGGL(td::lanczos_resize_indexed_kernel, dim3(plan.bands, 3, N), dim3(td::RS_THREADS), plan.lds, (hipStream_t)stream, store,
                     store_bytes, offsets, meta, tables, plan.bank, n_sizes, H, W, plan.band, plan.span_max, plan.Wp, plan.SW, packed, dst,
                     status);
  return td::record_launch_error(hipGetLastError(), "td_lanczos_resize_u8_indexed");
}
