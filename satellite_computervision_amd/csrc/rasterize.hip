// Polygon rasterization and raster masking (raster_tools.rasterize / geometry_mask / clip): what the reference leaves to
// rio.clip([aoi], crs) (utils/pc_tools.py:595-606; commented out at :384, :439, :493).  The rule is that of include/satcv.h, "Polygon
// rasterization", and of rasterize_core.hpp (the crossing column), shared by the host loop and the kernels.
//   crossings   one lane per (work item, row): an edge table entry spans at most RZ_ITEM_ROWS rows, lane k takes row r0 + k and appends
//               key = g << 32 | col at row_start[i] + atomicAdd(cursor[i], 1).  The host derived row_start from the row ranges, so the
//               slots of a row are exactly its crossings; the arrival order is arbitrary and the sort below removes it
//   fill        one workgroup per (row, strip of RZ_STRIP columns).  The row's keys are sorted in LDS (bitonic, padded to a power of two
//               with the largest key); a closed ring crosses every row an even number of times, so the sorted keys of one geometry are
//               consecutive pairs (2p, 2p + 1) = one span [col, col') each.  A wave takes a pair, its lanes the columns of the span, and
//               raises an LDS strip of int32 winners with atomicMax(g + 1): the last geometry in list order wins whatever the order of
//               arrival, with no barrier per span.  Then the strip is stored: mask or burn, any kind, the warp's destination addressing
//   mask_apply  streaming (planar rasters, and flat maps with ld = 1): a lane takes 16 bytes of samples and as many mask bytes per step;
//               pixel-interleaved rasters with ld > 1 take one pixel and its channels per lane.  In place a vector wholly inside the mask
//               is neither read nor written, one wholly outside is written without being read
// LDS per fill workgroup: RZ_MAX_KEYS * 8 + RZ_STRIP * 4 = 64 KiB, static: two workgroups per CU.  No scratch.
// Compiled with floating-point contraction off (rasterize_core.hpp), as warp.hip and reproject.hip are.
#include "common.hpp"
#include "raster_kinds.hpp"

#pragma clang fp contract(off)

#include "rasterize_core.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int RZ_BLOCK = 256;
constexpr int RZ_ITEM_ROWS = 64;        // rows of one work item: one wave's worth
constexpr int RZ_MAX_KEYS = 4096;       // crossings of one row (32 KiB of LDS)
constexpr int RZ_STRIP = 8192;          // columns of one fill workgroup (32 KiB of LDS)
constexpr int RZ_FIELDS = 7;            // x0, y0, x1, y1, r0, r1, g

// N elements of T at any address, moved as one item (a plane of an odd map starts anywhere)
template <typename T, int N>
struct __attribute__((packed, aligned(1))) RzItem {
  typedef T vec __attribute__((ext_vector_type(N)));
  vec v;
};
template <typename T, int N>
__device__ __forceinline__ typename RzItem<T, N>::vec rz_load(const T* p) { return reinterpret_cast<const RzItem<T, N>*>(p)->v; }
template <typename T, int N>
__device__ __forceinline__ void rz_store(T* p, typename RzItem<T, N>::vec v) { reinterpret_cast<RzItem<T, N>*>(p)->v = v; }

// ---------------------------------------------------------------- crossings
// keys has row_start[h] slots; a slot index is checked against the row's end, so a table the host mis-sized could lose a key but never
// write outside the row's slots
__global__ __launch_bounds__(RZ_BLOCK) void crossings_kernel(const double* __restrict__ items, const long long n_items, const int32_t* __restrict__ row_start,
                                                             int32_t* __restrict__ cursor, unsigned long long* __restrict__ keys, const int h, const int w) {
  const long long t = (long long)blockIdx.x * RZ_BLOCK + threadIdx.x;
  const long long it = t / RZ_ITEM_ROWS;
  if (it >= n_items) return;
  const double* e = items + it * RZ_FIELDS;
  const int r0 = (int)e[4], r1 = (int)e[5];
  const int i = r0 + (int)(t - it * RZ_ITEM_ROWS);
  if (i >= r1 || i < 0 || i >= h) return;
  const int col = crossing_col(e[0], e[1], e[2], e[3], i, w);
  const unsigned long long key = ((unsigned long long)(unsigned)(int)e[6] << 32) | (unsigned)col;
  const int at = row_start[i] + atomicAdd(&cursor[i], 1);
  if (at < row_start[i + 1]) keys[at] = key;
}

// ---------------------------------------------------------------- fill
template <typename T>
__global__ __launch_bounds__(RZ_BLOCK) void fill_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ row_start, const T* __restrict__ values,
                                                        const T inside, const T outside, const int keep, T* __restrict__ dst, const int h, const int w,
                                                        const int layout, const int ld, const int coff) {
  __shared__ unsigned long long sk[RZ_MAX_KEYS];
  __shared__ int win[RZ_STRIP];
  const int tid = threadIdx.x;
  const int i = blockIdx.x;
  const int s0 = blockIdx.y * RZ_STRIP;
  const int sw = min(RZ_STRIP, w - s0);
  const int begin = row_start[i];
  const int n = min(row_start[i + 1] - begin, RZ_MAX_KEYS);      // (the host refuses a longer row)
  int P = 2;
  while (P < n) P <<= 1;
  for (int k = tid; k < P; k += RZ_BLOCK) sk[k] = k < n ? keys[begin + k] : ~0ull;
  for (int j = tid; j < sw; j += RZ_BLOCK) win[j] = 0;
  __syncthreads();
  if (n > 1) {                                                   // (n is the same in every lane of the workgroup)
    for (int k = 2; k <= P; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += RZ_BLOCK) {
          const int a = 2 * j * (t / j) + (t % j), b = a + j;
          const unsigned long long va = sk[a], vb = sk[b];
          const bool up = (a & k) == 0;
          if ((va > vb) == up) {
            sk[a] = vb;
            sk[b] = va;
          }
        }
        __syncthreads();
      }
    }
  }
  const int wave = tid >> 6, lane = tid & 63;
  for (int p = wave; 2 * p + 1 < n; p += RZ_BLOCK / 64) {
    const unsigned long long k0 = sk[2 * p], k1 = sk[2 * p + 1];
    const int g1 = (int)(k0 >> 32) + 1;
    const int c0 = max((int)(unsigned)k0, s0) - s0, c1 = min((int)(unsigned)k1, s0 + sw) - s0;
    for (int j = c0 + lane; j < c1; j += 64) atomicMax(&win[j], g1);
  }
  __syncthreads();
  for (int j = tid; j < sw; j += RZ_BLOCK) {
    const int g1 = win[j];
    if (g1 == 0 && keep) continue;
    const T v = g1 == 0 ? outside : values ? values[g1 - 1] : inside;
    const size_t col = (size_t)(s0 + j);
    const size_t at = layout == 0 ? ((size_t)i * w + col) * ld + coff : ((size_t)coff * h + i) * w + col;
    dst[at] = v;
  }
}

// ---------------------------------------------------------------- mask apply
// planar: blockIdx.y is the plane; src == dst is in place
template <typename T>
__global__ __launch_bounds__(RZ_BLOCK) void mask_apply_planar_kernel(const uint8_t* __restrict__ mask, const T* src, T* dst, const int npix, const int invert, const T nd) {
  constexpr int VEC = 16 / sizeof(T);
  const T* sp = src + (size_t)blockIdx.y * npix;
  T* dp = dst + (size_t)blockIdx.y * npix;
  const bool in_place = sp == dp;
  const int nvec = npix / VEC;
  for (int v = blockIdx.x * RZ_BLOCK + threadIdx.x; v < nvec; v += gridDim.x * RZ_BLOCK) {
    const size_t at = (size_t)v * VEC;
    const auto m = rz_load<uint8_t, VEC>(mask + at);
    int in = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) in += ((m[e] != 0) != (invert != 0)) ? 1 : 0;
    typename RzItem<T, VEC>::vec o;
    if (in == 0) {
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = nd;
    } else {
      if (in == VEC && in_place) continue;
      o = rz_load<T, VEC>(sp + at);
#pragma unroll
      for (int e = 0; e < VEC; ++e) o[e] = ((m[e] != 0) != (invert != 0)) ? o[e] : nd;
    }
    rz_store<T, VEC>(dp + at, o);
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < npix - nvec * VEC) {
    const int at = nvec * VEC + (int)threadIdx.x;
    const bool in = (mask[at] != 0) != (invert != 0);
    if (!in) dp[at] = nd;
    else if (!in_place) dp[at] = sp[at];
  }
}

// pixel-interleaved: a lane takes one pixel and its c channels
template <typename T>
__global__ __launch_bounds__(RZ_BLOCK) void mask_apply_hwc_kernel(const uint8_t* __restrict__ mask, const T* src, T* dst, const int npix, const int c, const int ld,
                                                                  const int invert, const T nd) {
  const bool in_place = src == dst;
  for (long long p = (long long)blockIdx.x * RZ_BLOCK + threadIdx.x; p < npix; p += (long long)gridDim.x * RZ_BLOCK) {
    const bool in = (mask[p] != 0) != (invert != 0);
    if (in && in_place) continue;
    const T* sp = src + (size_t)p * ld;
    T* dp = dst + (size_t)p * ld;
    for (int k = 0; k < c; ++k) dp[k] = in ? sp[k] : nd;
  }
}

int rz_stream_grid(long long items) {
  long long g = (items + RZ_BLOCK - 1) / RZ_BLOCK;
  const long long cap = ew_grid_cap();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---------------------------------------------------------------- the workspace
struct RzLayout {
  long long items, keys, row_start, cursor, values, bytes;
};
long long up16(long long v) { return (v + 15) / 16 * 16; }
RzLayout rz_layout(long long n_items, int h, long long n_keys, int n_geoms) {
  RzLayout l;
  l.items = 0;
  l.keys = up16(n_items * RZ_FIELDS * 8);
  l.row_start = l.keys + up16(n_keys * 8);
  l.cursor = l.row_start + up16(((long long)h + 1) * 4);
  l.values = l.cursor + up16((long long)h * 4);
  l.bytes = l.values + up16((long long)n_geoms * 4);
  return l;
}

// ---------------------------------------------------------------- what the host refuses
int rz_table_refused(const satcv_rasterize_desc* d, const char* who) {
  SATCV_CHECK(d->h > 0 && d->w_ > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "%s: grid beyond 2^31 pixels", who);
  SATCV_CHECK(d->n_items >= 0 && d->n_items < (1LL << 26), "%s: n_items = %lld (0 ... 2^26 - 1)", who, (long long)d->n_items);
  SATCV_CHECK(d->n_geoms >= 0, "%s: n_geoms = %d", who, d->n_geoms);
  SATCV_CHECK(d->row_start, "%s: null pointer (row_start)", who);
  SATCV_CHECK(d->n_items == 0 || d->edges, "%s: null pointer (edges)", who);
  std::vector<int32_t> diff((size_t)d->h + 1, 0);
  for (long long k = 0; k < d->n_items; ++k) {
    const double* e = d->edges + k * RZ_FIELDS;
    SATCV_CHECK(std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2]) && std::isfinite(e[3]), "%s: edge %lld has a non-finite vertex", who, k);
    SATCV_CHECK(e[1] < e[3], "%s: edge %lld is not ordered (y0 = %.17g, y1 = %.17g; y0 < y1, horizontal edges are dropped)", who, k, e[1], e[3]);
    SATCV_CHECK(e[4] >= 0.0 && e[5] <= (double)d->h && e[4] <= e[5] && e[4] == floor(e[4]) && e[5] == floor(e[5]),
                "%s: edge %lld has the row range [%g, %g) outside [0, %d]", who, k, e[4], e[5], d->h);
    const int r0 = (int)e[4], r1 = (int)e[5];
    SATCV_CHECK(r1 - r0 <= RZ_ITEM_ROWS, "%s: edge %lld spans %d rows (a work item has at most %d)", who, k, r1 - r0, RZ_ITEM_ROWS);
    SATCV_CHECK(r0 == r1 || (edge_crosses_row(e[1], e[3], r0) && edge_crosses_row(e[1], e[3], r1 - 1)),
                "%s: edge %lld does not cross the rows %d ... %d it names", who, k, r0, r1 - 1);
    SATCV_CHECK(e[6] >= 0.0 && e[6] < (double)d->n_geoms && e[6] == floor(e[6]), "%s: edge %lld names geometry %g of %d", who, k, e[6], d->n_geoms);
    diff[r0] += 1;
    diff[r1] -= 1;
  }
  SATCV_CHECK(d->row_start[0] == 0, "%s: row_start[0] = %d does not match the edge table (0)", who, d->row_start[0]);
  long long run = 0, total = 0;
  for (int i = 0; i < d->h; ++i) {
    run += diff[i];
    SATCV_CHECK(run <= RZ_MAX_KEYS, "%s: row %d has %lld crossings (at most %d)", who, i, run, RZ_MAX_KEYS);
    total += run;
    SATCV_CHECK(total < (1LL << 31) && (long long)d->row_start[i + 1] == total, "%s: row_start[%d] = %d does not match the edge table (%lld)", who, i + 1,
                d->row_start[i + 1], total);
  }
  return SATCV_OK;
}

int rz_dst_refused(const satcv_rasterize_desc* d, const char* who) {
  SATCV_CHECK(d->dst, "%s: null pointer (dst)", who);
  SATCV_CHECK(d->mode == 0 || d->mode == 1, "%s: mode %d (0 mask, 1 burn)", who, d->mode);
  SATCV_CHECK(kind_ok(d->dst_kind), "%s: dst_kind %d (0 u8, 1 u16, 2 f32, 3 i16, 5 i32)", who, d->dst_kind);
  SATCV_CHECK(d->mode == 1 || d->dst_kind == 0, "%s: a mask is u8 (kind 0), got dst_kind %d", who, d->dst_kind);
  SATCV_CHECK(d->mode == 0 || d->n_geoms == 0 || d->values, "%s: null pointer (values)", who);
  SATCV_CHECK(d->dst_layout == 0 || d->dst_layout == 1, "%s: dst_layout %d (0 pixel-interleaved, 1 planar)", who, d->dst_layout);
  SATCV_CHECK(d->dst_coff >= 0 && d->dst_ld >= 1 && d->dst_coff < d->dst_ld, "%s: channel %d does not fit ld = %d", who, d->dst_coff, d->dst_ld);
  SATCV_CHECK((long long)d->h * d->w_ * d->dst_ld < (1LL << 40), "%s: destination beyond 2^40 samples", who);
  SATCV_CHECK(d->on_device == 0 || d->on_device == 1, "%s: on_device %d (0 host pointers, 1 device pointers)", who, d->on_device);
  SATCV_CHECK((uintptr_t)d->dst % kind_bytes(d->dst_kind) == 0, "%s: misaligned pointer (dst)", who);
  return SATCV_OK;
}

// the same rule on the CPU: dst is a host pointer
template <typename T>
void rasterize_host(const satcv_rasterize_desc* d, T inside, T outside) {
  const int h = d->h, w = d->w_;
  const T* values = d->mode == 1 ? reinterpret_cast<const T*>(d->values) : nullptr;
  T* dst = reinterpret_cast<T*>(d->dst);
  std::vector<unsigned long long> keys((size_t)d->row_start[h]);
  std::vector<int32_t> cursor((size_t)h, 0);
  for (long long k = 0; k < d->n_items; ++k) {
    const double* e = d->edges + k * RZ_FIELDS;
    for (int i = (int)e[4]; i < (int)e[5]; ++i) {
      const int col = crossing_col(e[0], e[1], e[2], e[3], i, w);
      keys[(size_t)d->row_start[i] + cursor[i]++] = ((unsigned long long)(unsigned)(int)e[6] << 32) | (unsigned)col;
    }
  }
  std::vector<int> win((size_t)w);
  for (int i = 0; i < h; ++i) {
    unsigned long long* rk = keys.data() + d->row_start[i];
    const int n = d->row_start[i + 1] - d->row_start[i];
    std::sort(rk, rk + n);
    std::fill(win.begin(), win.end(), 0);
    for (int p = 0; 2 * p + 1 < n; ++p) {
      const int g1 = (int)(rk[2 * p] >> 32) + 1;
      for (int j = (int)(unsigned)rk[2 * p]; j < (int)(unsigned)rk[2 * p + 1]; ++j) win[j] = std::max(win[j], g1);
    }
    for (int j = 0; j < w; ++j) {
      if (win[j] == 0 && d->keep) continue;
      const T v = win[j] == 0 ? outside : values ? values[win[j] - 1] : inside;
      const size_t at = d->dst_layout == 0 ? ((size_t)i * w + j) * d->dst_ld + d->dst_coff : ((size_t)d->dst_coff * h + i) * w + j;
      dst[at] = v;
    }
  }
}

template <typename T>
int rasterize_device(const satcv_rasterize_desc* d, T inside, T outside, hipStream_t st) {
  const long long n_keys = d->row_start[d->h];
  const RzLayout l = rz_layout(d->n_items, d->h, n_keys, d->n_geoms);
  char* ws = reinterpret_cast<char*>(d->workspace);
  if (d->n_items) SATCV_HIP(hipMemcpyAsync(ws + l.items, d->edges, (size_t)d->n_items * RZ_FIELDS * 8, hipMemcpyHostToDevice, st));
  SATCV_HIP(hipMemcpyAsync(ws + l.row_start, d->row_start, ((size_t)d->h + 1) * 4, hipMemcpyHostToDevice, st));
  const bool burn = d->mode == 1 && d->n_geoms > 0;
  if (burn) SATCV_HIP(hipMemcpyAsync(ws + l.values, d->values, (size_t)d->n_geoms * sizeof(T), hipMemcpyHostToDevice, st));
  SATCV_HIP(hipMemsetAsync(ws + l.cursor, 0, (size_t)d->h * 4, st));
  const int32_t* row_start = reinterpret_cast<const int32_t*>(ws + l.row_start);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + l.keys);
  if (d->n_items) {
    const long long threads = d->n_items * RZ_ITEM_ROWS;
    const int rc = satcv_launch(crossings_kernel, dim3((unsigned)((threads + RZ_BLOCK - 1) / RZ_BLOCK)), dim3(RZ_BLOCK), 0, st, "rasterize (crossings)",
                                reinterpret_cast<const double*>(ws + l.items), (long long)d->n_items, row_start, reinterpret_cast<int32_t*>(ws + l.cursor), keys, (int)d->h,
                                (int)d->w_);
    if (rc) return rc;
  }
  // rows along x (up to 2^31 - 1 workgroups), strips along y (w / RZ_STRIP < 65536)
  const int strips = (d->w_ + RZ_STRIP - 1) / RZ_STRIP;
  return satcv_launch(fill_kernel<T>, dim3(d->h, strips), dim3(RZ_BLOCK), 0, st, "rasterize (fill)", (const unsigned long long*)keys, row_start,
                      burn ? reinterpret_cast<const T*>(ws + l.values) : (const T*)nullptr, inside, outside, (int)d->keep, reinterpret_cast<T*>(d->dst), (int)d->h, (int)d->w_,
                      (int)d->dst_layout, (int)d->dst_ld, (int)d->dst_coff);
}

}  // namespace

extern "C" int satcv_rasterize_workspace(int64_t n_items, int32_t h, int64_t n_keys, int32_t n_geoms, int64_t* bytes) {
  const char* who = "rasterize_workspace";
  SATCV_CHECK(bytes, "%s: null pointer (bytes)", who);
  SATCV_CHECK(n_items >= 0 && n_items < (1LL << 26) && h > 0 && n_keys >= 0 && n_keys < (1LL << 31) && n_geoms >= 0, "%s: n_items = %lld, h = %d, n_keys = %lld, n_geoms = %d",
              who, (long long)n_items, h, (long long)n_keys, n_geoms);
  *bytes = rz_layout(n_items, h, n_keys, n_geoms).bytes;
  return SATCV_OK;
}

extern "C" int satcv_rasterize(const satcv_rasterize_desc* d, void* stream) {
  const char* who = "rasterize";
  SATCV_CHECK(d, "%s: null pointer (descriptor)", who);
  if (const int rc = rz_dst_refused(d, who)) return rc;
  if (const int rc = rz_table_refused(d, who)) return rc;
  if (d->on_device) {
    const long long need = rz_layout(d->n_items, d->h, d->row_start[d->h], d->n_geoms).bytes;
    SATCV_CHECK(d->workspace, "%s: null pointer (workspace)", who);
    SATCV_CHECK((uintptr_t)d->workspace % 16 == 0, "%s: misaligned pointer (workspace)", who);
    SATCV_CHECK(d->workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (satcv_rasterize_workspace)", who, (long long)d->workspace_bytes, need);
    const char* w0 = reinterpret_cast<const char*>(d->workspace);
    const char* d0 = reinterpret_cast<const char*>(d->dst);
    const long long dbytes = (long long)d->h * d->w_ * d->dst_ld * kind_bytes(d->dst_kind);
    SATCV_CHECK(d0 + dbytes <= w0 || w0 + d->workspace_bytes <= d0, "%s: dst overlaps the workspace", who);
    // the table is copied from pageable host memory that the caller may release on return: a captured copy would be replayed from it
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SATCV_HIP(hipStreamIsCapturing((hipStream_t)stream, &cap));
    SATCV_CHECK(cap == hipStreamCaptureStatusNone, "%s: the stream is being captured into a graph (the edge table is copied from host memory)", who);
  }
  const hipStream_t st = (hipStream_t)stream;
  return by_kind(d->dst_kind, [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T inside = d->mode == 0 ? (T)(d->invert ? 0 : 1) : (T)0;
    const T outside = d->mode == 0 ? (T)(d->invert ? 1 : 0) : nodata_as<T>(d->fill);
    if (!d->on_device) {
      rasterize_host<T>(d, inside, outside);
      return SATCV_OK;
    }
    return rasterize_device<T>(d, inside, outside, st);
  });
}

extern "C" int satcv_raster_mask_apply(const satcv_mask_apply_desc* d, void* stream) {
  const char* who = "raster_mask_apply";
  SATCV_CHECK(d && d->mask && d->src && d->dst, "%s: null pointer (descriptor, mask, src, dst)", who);
  SATCV_CHECK(kind_ok(d->kind), "%s: kind %d (0 u8, 1 u16, 2 f32, 3 i16, 5 i32)", who, d->kind);
  SATCV_CHECK(d->layout == 0 || d->layout == 1, "%s: layout %d (0 pixel-interleaved, 1 planar)", who, d->layout);
  SATCV_CHECK(d->h > 0 && d->w_ > 0 && d->c > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "%s: map beyond 2^31 pixels", who);
  SATCV_CHECK(d->coff >= 0 && d->ld >= 1 && (long long)d->coff + d->c <= d->ld, "%s: channels %d ... %d do not fit ld = %d", who, d->coff, d->coff + d->c - 1, d->ld);
  SATCV_CHECK(d->layout == 0 || d->c <= 65535, "%s: %d planes in one call (at most 65535)", who, d->c);
  const long long npix = (long long)d->h * d->w_, sz = kind_bytes(d->kind);
  SATCV_CHECK(npix * d->ld < (1LL << 40), "%s: raster beyond 2^40 samples", who);
  SATCV_CHECK((uintptr_t)d->src % sz == 0 && (uintptr_t)d->dst % sz == 0, "%s: misaligned pointer", who);
  const char* s0 = reinterpret_cast<const char*>(d->src);
  const char* d0 = reinterpret_cast<const char*>(d->dst);
  const char* m0 = reinterpret_cast<const char*>(d->mask);
  const long long bytes = npix * d->ld * sz;
  SATCV_CHECK(s0 == d0 || d0 + bytes <= s0 || s0 + bytes <= d0, "%s: dst overlaps src (in place is dst == src)", who);
  SATCV_CHECK(d0 + bytes <= m0 || m0 + npix <= d0, "%s: dst overlaps the mask", who);
  const hipStream_t st = (hipStream_t)stream;
  return by_kind(d->kind, [&](auto tag) -> int {
    typedef decltype(tag) T;
    const T nd = d->has_nodata ? nodata_as<T>(d->nodata) : nodata_as<T>(NAN);
    const T* src = reinterpret_cast<const T*>(d->src);
    T* dst = reinterpret_cast<T*>(d->dst);
    if (d->layout == 1 || d->ld == 1) {                      // (one channel per pixel is one plane: a flat (h, w_) map streams too)
      const size_t off = d->layout == 1 ? (size_t)d->coff * npix : 0;
      return satcv_launch(mask_apply_planar_kernel<T>, dim3(rz_stream_grid(npix / (16 / (int)sizeof(T))), d->c), dim3(RZ_BLOCK), 0, st, who, d->mask, src + off, dst + off,
                          (int)npix, (int)d->invert, nd);
    }
    return satcv_launch(mask_apply_hwc_kernel<T>, dim3(rz_stream_grid(npix)), dim3(RZ_BLOCK), 0, st, who, d->mask, src + d->coff, dst + d->coff, (int)npix, (int)d->c,
                        (int)d->ld, (int)d->invert, nd);
  });
}
