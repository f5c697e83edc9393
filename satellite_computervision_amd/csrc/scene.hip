// Device-resident sliding-window prediction (utils/prediction_tools.py:133-156): the two HBM-bound kernels around the model.
//   scene_gather : windows of a resident (H, W, c) scene -> fp32 NHWC chips the inference plans read in place (replaces the window
//                  slicing of :149 and np.array([chip]) of :152); out-of-scene coordinates are reflected (np.pad mode='reflect') and
//                  then clamped, so no origin can make the kernel read outside the scene
//   scene_scatter: the centre of every predicted chip -> its place in a resident (H, W, ldd) map, clipped to the map (replaces the
//                  crop and `template[...] +=` of :154 and the crops of :267 / :349)
//   series_gather: windows of a resident (t, c, h, w) time stack -> the time-major (steps, n, side, side, cpad) storage tensor the
//                  ConvLSTM2D models read in place: the window slicing, np.moveaxis(cut, 2, 4), normalize_timeseries
//                  (utils/processing.py:185-193, :937-972) and satcv_ingest_seq in one pass; same reflect-then-clamp rule
// Lanes run along a row in all three: a chip row is side * c contiguous source elements (side contiguous samples of a band plane for
// the planar stack), a centre row is crop_w contiguous map pixels.
#include "common.hpp"
#include <cstdlib>

#define EW_BLOCK 256
// grid-stride kernels on a bounded number of workgroups per CU (elementwise.hip: 6 per CU; SATCV_EW_PER_CU overrides)
static inline int ew_grid(long long items) {
  const int cap = ew_grid_cap();
  long long b = (items + EW_BLOCK - 1) / EW_BLOCK;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
#define LAUNCH_OK(name)                                                          \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      satcv_set_error(name " launch: %s", hipGetErrorString(e__));               \
      return SATCV_ERR_HIP;                                                      \
    }                                                                            \
  } while (0)

namespace {

// np.pad(mode='reflect') index of coordinate i on an axis of n samples (the edge sample is not repeated), then clamped: one
// reflection is exact for |overhang| < n, anything further lands on an edge sample -- always inside [0, n)
__device__ __forceinline__ int mirror(long long i, int n) {
  if (i < 0) i = -i;
  else if (i >= n) i = 2LL * (n - 1) - i;
  return (int)(i < 0 ? 0 : (i > n - 1 ? n - 1 : i));
}

// (float)((double)src / rescale): one correctly rounded double division and one rounding to float, what
// (scene.astype(float64) / rescale).astype(float32) computes; rescale == 0 converts only
template <typename S>
__device__ __forceinline__ float to_f32(S s, double rescale) {
  return rescale != 0.0 ? (float)((double)s / rescale) : (float)s;
}

// ---------------------------------------------------------------- gather, c == ldc == 4 (the 4-band scene into its own tensor)
// one lane per chip pixel: ONE 4-element load (8 B of u16, 16 B of f32) and one 16-byte store, consecutive lanes on consecutive
// pixels of the row
template <typename S>
__global__ __launch_bounds__(EW_BLOCK) void scene_gather4_kernel(const satcv_scene_gather_desc d) {
  struct alignas(4 * sizeof(S)) S4 { S v[4]; };
  const S4* __restrict__ src = reinterpret_cast<const S4*>(d.src);
  float4* __restrict__ dst = reinterpret_cast<float4*>(d.dst);
  const int side = d.side;
  const long long total = (long long)d.n * side * side;
  for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const int px = (int)(it % side);
    const int r = (int)((it / side) % side);
    const int k = (int)(it / ((long long)side * side));
    const int* o = d.origins + 2 * (size_t)(d.first + k);
    const int sy = mirror((long long)o[0] - d.off + r, d.h);
    const int sx = mirror((long long)o[1] - d.off + px, d.w_);
    const S4 s = src[(size_t)sy * d.w_ + sx];
    dst[it] = make_float4(to_f32(s.v[0], d.rescale), to_f32(s.v[1], d.rescale), to_f32(s.v[2], d.rescale), to_f32(s.v[3], d.rescale));
  }
}

// ---------------------------------------------------------------- gather, any c / ldc / coff
// one lane per ELEMENT of a chip row (side * c of them, contiguous in the scene wherever the row is not reflected): consecutive
// lanes read consecutive source elements and write consecutive floats of the pixel's channel slice
template <typename S>
__global__ __launch_bounds__(EW_BLOCK) void scene_gather_kernel(const satcv_scene_gather_desc d) {
  const S* __restrict__ src = reinterpret_cast<const S*>(d.src);
  const int side = d.side, c = d.c, row = side * c;
  const long long total = (long long)d.n * side * row;
  for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const int j = (int)(it % row);
    const int px = j / c, ch = j - px * c;
    const long long rk = it / row;                       // k * side + r: the chip row
    const int r = (int)(rk % side);
    const int k = (int)(rk / side);
    const int* o = d.origins + 2 * (size_t)(d.first + k);
    const int sy = mirror((long long)o[0] - d.off + r, d.h);
    const int sx = mirror((long long)o[1] - d.off + px, d.w_);
    d.dst[((size_t)rk * side + px) * d.ldc + d.coff + ch] = to_f32(src[((size_t)sy * d.w_ + sx) * c + ch], d.rescale);
  }
}

// ---------------------------------------------------------------- series gather (planar time stack -> time-major storage tensor)
// one lane per destination pixel and 8-channel group, the pixel's x fastest: the (up to) 8 loads of a lane are one sample of 8 band
// planes each, consecutive lanes on consecutive samples of a plane row; the 8 values leave as ONE 16-byte store (bf16; two for f32).
// The groups of a chip row follow each other in item order, so the two halves of a pixel's 32 bytes are written by neighbouring waves.
// value = (float)((double)v / maxval), NaN -> 0: normalize_timeseries followed by the generator's astype(float32)
template <typename S, typename T>
__global__ __launch_bounds__(EW_BLOCK) void series_gather_kernel(const satcv_series_gather_desc d) {
  const S* __restrict__ src = reinterpret_cast<const S*>(d.src);
  T* __restrict__ dst = reinterpret_cast<T*>(d.dst);
  const int side = d.side, groups = d.cpad / 8;
  const long long plane = (long long)d.h * d.w_;
  const long long total = (long long)d.steps * d.n * side * groups * side;
  for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const int px = (int)(it % side);
    long long q = it / side;
    const int g = (int)(q % groups); q /= groups;
    const int r = (int)(q % side); q /= side;            // q = s * n + k: the destination image
    const int k = (int)(q % d.n), s = (int)(q / d.n);
    const int* o = d.origins + 2 * (size_t)(d.first + k);
    const int sy = mirror((long long)o[0] - d.off + r, d.h);
    const int sx = mirror((long long)o[1] - d.off + px, d.w_);
    const S* p = src + ((long long)s * d.c + g * 8) * plane + (long long)sy * d.w_ + sx;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float f = 0.f;
      if (g * 8 + e < d.c) {
        f = (float)((double)p[e * plane] / d.maxval);
        f = f != f ? 0.f : f;
      }
      v[e] = f;
    }
    store8<T>(dst + ((q * side + r) * side + px) * d.cpad + g * 8, v);
  }
}

// ---------------------------------------------------------------- scatter
// one lane per centre pixel, consecutive lanes along the row.  LDS > 0: the whole source pixel (LDS channels, one vector load -- the
// unwanted channels share its cache line anyway) and a select; LDS == 0: the channel range with scalar loads.
// Plain read-modify-write: the centres of one launch are pairwise disjoint (contract), launches on a stream are ordered.
template <typename S, typename D, int LDS>
__global__ __launch_bounds__(EW_BLOCK) void scene_scatter_kernel(const satcv_scene_scatter_desc d) {
  const S* __restrict__ src = reinterpret_cast<const S*>(d.src);
  D* __restrict__ dst = reinterpret_cast<D*>(d.dst);
  const int cw = d.crop_w, chh = d.crop_h;
  const long long total = (long long)d.n * chh * cw;
  for (long long it = blockIdx.x * (long long)blockDim.x + threadIdx.x; it < total; it += (long long)gridDim.x * blockDim.x) {
    const int px = (int)(it % cw);
    const int r = (int)((it / cw) % chh);
    const int k = (int)(it / ((long long)cw * chh));
    const int* o = d.origins + 2 * (size_t)(d.first + k);
    const long long y = (long long)o[0] + r, x = (long long)o[1] + px;
    if (y < 0 || y >= d.h || x < 0 || x >= d.w_) continue;           // clipped to the map
    const size_t sp = ((size_t)k * d.sh + d.crop_y + r) * d.sw + d.crop_x + px;
    D* q = dst + ((size_t)y * d.w_ + (size_t)x) * d.ldd + d.doff;
    if constexpr (LDS > 0) {
      struct alignas(LDS * sizeof(S)) SV { S v[LDS]; };
      const SV s = reinterpret_cast<const SV*>(src)[sp];
#pragma unroll
      for (int e = 0; e < LDS; ++e) {
        const int j = e - d.c0;
        if (j >= 0 && j < d.nc) q[j] = d.accumulate ? (D)(q[j] + (D)s.v[e]) : (D)s.v[e];
      }
    } else {
      const S* s = src + sp * d.lds + d.c0;
      for (int j = 0; j < d.nc; ++j) q[j] = d.accumulate ? (D)(q[j] + (D)s[j]) : (D)s[j];
    }
  }
}

template <typename S, typename D>
void launch_scatter(const satcv_scene_scatter_desc& d, hipStream_t st) {
  const dim3 grid(ew_grid((long long)d.n * d.crop_h * d.crop_w)), block(EW_BLOCK);
  const bool vec = (uintptr_t)d.src % (d.lds * sizeof(S)) == 0;
  if (vec && d.lds == 1) hipLaunchKernelGGL((scene_scatter_kernel<S, D, 1>), grid, block, 0, st, d);
  else if (vec && d.lds == 2) hipLaunchKernelGGL((scene_scatter_kernel<S, D, 2>), grid, block, 0, st, d);
  else if (vec && d.lds == 4) hipLaunchKernelGGL((scene_scatter_kernel<S, D, 4>), grid, block, 0, st, d);
  else hipLaunchKernelGGL((scene_scatter_kernel<S, D, 0>), grid, block, 0, st, d);
}

template <typename S>
void launch_gather(const satcv_scene_gather_desc& d, hipStream_t st) {
  const bool four = d.c == 4 && d.ldc == 4 && d.coff == 0 && (uintptr_t)d.src % (4 * sizeof(S)) == 0 && (uintptr_t)d.dst % 16 == 0;
  if (four) hipLaunchKernelGGL(scene_gather4_kernel<S>, dim3(ew_grid((long long)d.n * d.side * d.side)), dim3(EW_BLOCK), 0, st, d);
  else hipLaunchKernelGGL(scene_gather_kernel<S>, dim3(ew_grid((long long)d.n * d.side * d.side * d.c)), dim3(EW_BLOCK), 0, st, d);
}

template <typename S>
void launch_series_gather(const satcv_series_gather_desc& d, hipStream_t st) {
  const dim3 grid(ew_grid((long long)d.steps * d.n * d.side * d.side * (d.cpad / 8))), block(EW_BLOCK);
  if (d.dtype == SATCV_BF16) hipLaunchKernelGGL((series_gather_kernel<S, bf16>), grid, block, 0, st, d);
  else hipLaunchKernelGGL((series_gather_kernel<S, float>), grid, block, 0, st, d);
}

}  // namespace

extern "C" int satcv_scene_gather(const satcv_scene_gather_desc* d, void* stream) {
  SATCV_CHECK(d && d->src && d->origins && d->dst, "scene_gather: null pointer");
  SATCV_CHECK(d->h > 0 && d->w_ > 0 && d->c > 0 && d->side > 0 && d->off >= 0 && d->n > 0, "scene_gather: sizes must be positive (off >= 0)");
  SATCV_CHECK(d->src_kind >= 0 && d->src_kind <= 3, "scene_gather: src_kind %d (0 u8, 1 u16, 2 f32, 3 i16)", d->src_kind);
  SATCV_CHECK(d->coff >= 0 && d->ldc > 0 && (long long)d->coff + d->c <= d->ldc, "scene_gather: destination channel range (coff + c <= ldc)");
  SATCV_CHECK(d->first >= 0 && d->total > 0 && (long long)d->first + d->n <= d->total, "scene_gather: chips [first, first + n) outside the origin table");
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "scene_gather: scene beyond 2^31 pixels");
  SATCV_CHECK(satcv_pixels_ok(d->n, d->side, d->side, 1) && (long long)d->n * d->side * d->side * d->ldc < (1LL << 31), "scene_gather: chips beyond 2^31 elements");
  const hipStream_t st = (hipStream_t)stream;
  switch (d->src_kind) {
    case 0: launch_gather<uint8_t>(*d, st); break;
    case 1: launch_gather<uint16_t>(*d, st); break;
    case 2: launch_gather<float>(*d, st); break;
    default: launch_gather<int16_t>(*d, st); break;
  }
  LAUNCH_OK("scene_gather");
  return SATCV_OK;
}

extern "C" int satcv_series_gather(const satcv_series_gather_desc* d, void* stream) {
  SATCV_CHECK(d && d->src && d->origins && d->dst, "series_gather: null pointer");
  SATCV_CHECK(d->t > 0 && d->c > 0 && d->h > 0 && d->w_ > 0 && d->side > 0 && d->off >= 0 && d->n > 0, "series_gather: sizes must be positive (off >= 0)");
  SATCV_CHECK(d->src_kind >= 1 && d->src_kind <= 3, "series_gather: src_kind %d (1 u16, 2 f32, 3 i16)", d->src_kind);
  SATCV_CHECK(d->steps > 0 && d->steps <= d->t, "series_gather: steps %d outside 1 .. t = %d", d->steps, d->t);
  SATCV_CHECK(d->maxval == d->maxval && d->maxval != 0.0, "series_gather: maxval must be a non-zero number");
  SATCV_CHECK(d->dtype == SATCV_BF16 || d->dtype == SATCV_F32, "series_gather: dtype %d (bf16 or f32 storage)", d->dtype);
  SATCV_CHECK(d->cpad > 0 && d->cpad % 8 == 0 && d->cpad >= d->c, "series_gather: destination channels (cpad %% 8 == 0, cpad >= c)");
  SATCV_CHECK((uintptr_t)d->dst % 16 == 0, "series_gather: dst must be 16-byte aligned");
  SATCV_CHECK(d->first >= 0 && d->total > 0 && (long long)d->first + d->n <= d->total, "series_gather: chips [first, first + n) outside the origin table");
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "series_gather: acquisition beyond 2^31 pixels");
  SATCV_CHECK(satcv_pixels_ok((long long)d->steps * d->n, d->side, d->side, 1) &&
              (long long)d->steps * d->n * d->side * d->side * d->cpad < (1LL << 31), "series_gather: chips beyond 2^31 elements");
  const hipStream_t st = (hipStream_t)stream;
  switch (d->src_kind) {
    case 1: launch_series_gather<uint16_t>(*d, st); break;
    case 2: launch_series_gather<float>(*d, st); break;
    default: launch_series_gather<int16_t>(*d, st); break;
  }
  LAUNCH_OK("series_gather");
  return SATCV_OK;
}

extern "C" int satcv_scene_scatter(const satcv_scene_scatter_desc* d, void* stream) {
  SATCV_CHECK(d && d->src && d->origins && d->dst, "scene_scatter: null pointer");
  SATCV_CHECK(d->n > 0 && d->sh > 0 && d->sw > 0 && d->lds > 0 && d->nc > 0 && d->h > 0 && d->w_ > 0 && d->ldd > 0, "scene_scatter: sizes must be positive");
  SATCV_CHECK(d->crop_y >= 0 && d->crop_x >= 0 && d->crop_h > 0 && d->crop_w > 0 && (long long)d->crop_y + d->crop_h <= d->sh &&
              (long long)d->crop_x + d->crop_w <= d->sw, "scene_scatter: crop outside the chip");
  SATCV_CHECK(d->c0 >= 0 && (long long)d->c0 + d->nc <= d->lds, "scene_scatter: source channel range (c0 + nc <= lds)");
  SATCV_CHECK(d->doff >= 0 && (long long)d->doff + d->nc <= d->ldd, "scene_scatter: destination channel range (doff + nc <= ldd)");
  SATCV_CHECK(d->src_kind == 2 || d->src_kind == 5, "scene_scatter: src_kind %d (2 f32, 5 i32)", d->src_kind);
  SATCV_CHECK(d->dst_kind == 2 || d->dst_kind == 0, "scene_scatter: dst_kind %d (2 f32, 0 u8)", d->dst_kind);
  SATCV_CHECK(d->dst_kind != 0 || (d->src_kind == 5 && !d->accumulate), "scene_scatter: a u8 map takes i32 classes, without accumulation");
  SATCV_CHECK(d->first >= 0 && d->total > 0 && (long long)d->first + d->n <= d->total, "scene_scatter: chips [first, first + n) outside the origin table");
  SATCV_CHECK(satcv_pixels_ok(d->n, d->sh, d->sw, 1) && (long long)d->n * d->sh * d->sw * d->lds < (1LL << 31), "scene_scatter: chips beyond 2^31 elements");
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "scene_scatter: map beyond 2^31 pixels");
  const hipStream_t st = (hipStream_t)stream;
  if (d->src_kind == 2) launch_scatter<float, float>(*d, st);
  else if (d->dst_kind == 2) launch_scatter<int32_t, float>(*d, st);
  else launch_scatter<int32_t, uint8_t>(*d, st);
  LAUNCH_OK("scene_scatter");
  return SATCV_OK;
}
