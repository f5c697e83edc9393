// Radiometric calibration between scenes (utils/calibration.py on arrays): the overlap region of two rasters, per-band histograms of
// a region, the histogram-matching table of equalize (:136-182), the percentile table of clamp_and_scale (:12-45) and the kernel that
// sends a raster through a per-band table.  The rules are in include/satcv.h; every decision is integer arithmetic on the stored
// sample values, so the results are bit-reproducible -- also the histogram, whose atomics add integers.
//
//   overlap    streaming: a lane takes 16 bytes of every plane of both rasters per step and writes as many region bytes
//   histogram  the only scattering kernel of the library.  One workgroup per strip of H_STRIP samples of one plane: the values 0 ...
//              split - 1 (where reflectances lie, in the signed kind too) are counted in an LDS-private histogram (ds_add_u32), the others
//              straight in global memory; at the end the workgroup adds its non-zero private bins to global memory.  65536 uint32 bins are 256 KiB and do not fit the 160 KiB of LDS, hence the split
//   match_lut  one workgroup per band: a lane sums its chunk of both histograms, the chunk sums are scanned in LDS, then every entry is
//              a binary search over the chunk sums and a walk of at most one chunk (64 bins) of image 1's histogram
//   scale_lut  the same scan; the percentile is one search, the table a division in double per entry
//   apply      planar destinations stream like overlap (16 bytes of samples per lane, one table gather per sample, whole-vector stores
//              where every sample is valid); pixel-interleaved destinations take one pixel and all its bands per lane.  A band's table
//              is 128 KiB (u16) or 256 KiB (f32): it stays in the L2 and is not staged in LDS
// No plane needs any alignment: the 16-byte items are loaded and stored as packed structs (a plane of an odd map starts anywhere).
#include "raster_kinds.hpp"

namespace {

constexpr int C_BLOCK = 256;          // streaming kernels
constexpr int H_BLOCK = 512;          // histogram
constexpr int H_STRIP = 1 << 18;      // samples of one plane per histogram workgroup
constexpr int H_SPLIT = 16384;        // private bins of the 16-bit kinds by default (64 KiB of LDS, two workgroups per CU: profiles/calibration_probe.txt)
constexpr int H_SPLIT_MAX = 32768;    // 128 KiB

template <typename S> struct Bins {
  static constexpr int N = sizeof(S) == 1 ? 256 : 65536;
  static constexpr int BIAS = std::is_signed<S>::value ? 32768 : 0;
  static constexpr int THREADS = sizeof(S) == 1 ? 256 : 1024;       // of the table kernels: N / THREADS bins per lane
};
template <typename S> __host__ __device__ __forceinline__ int bin_of(S v) { return (int)v + Bins<S>::BIAS; }
template <typename S> __host__ __device__ __forceinline__ S value_of(int k) { return (S)(k - Bins<S>::BIAS); }

bool calib_kind_ok(int k) { return k == 0 || k == 1 || k == 3; }
template <typename F>
int by_calib_kind(int kind, F&& f) {
  switch (kind) {
    case 0: return f(uint8_t{});
    case 1: return f(uint16_t{});
    default: return f(int16_t{});
  }
}

// nodata as a value of the kind; false when it is none (then no sample equals it)
template <typename S>
bool nodata_in_kind(int has_nodata, double v, S& out) {
  out = 0;
  if (!has_nodata || !(v == v)) return false;
  const double lo = (double)std::numeric_limits<S>::min(), hi = (double)std::numeric_limits<S>::max();
  if (v < lo || v > hi || v != (double)(long long)v) return false;
  out = (S)(long long)v;
  return true;
}

// N elements of T at any address, moved as one item
template <typename T, int N>
struct __attribute__((packed, aligned(1))) Item {
  typedef T vec __attribute__((ext_vector_type(N)));
  vec v;
};
template <typename T, int N>
__device__ __forceinline__ typename Item<T, N>::vec load_item(const T* p) { return reinterpret_cast<const Item<T, N>*>(p)->v; }
template <typename T, int N>
__device__ __forceinline__ void store_item(T* p, typename Item<T, N>::vec v) { reinterpret_cast<Item<T, N>*>(p)->v = v; }

int stream_grid(long long items) {
  long long g = (items + C_BLOCK - 1) / C_BLOCK;
  const long long cap = ew_grid_cap();
  return (int)(g < 1 ? 1 : g > cap ? cap : g);
}

// ---------------------------------------------------------------- overlap
template <typename S>
__global__ __launch_bounds__(C_BLOCK) void overlap_kernel(const S* __restrict__ a, const S* __restrict__ b, const uint8_t* __restrict__ mask,
                                                          uint8_t* __restrict__ region, int c, int npix, bool has_nd, S nd) {
  constexpr int VEC = 16 / sizeof(S);
  const int nvec = npix / VEC;
  for (int v = blockIdx.x * C_BLOCK + threadIdx.x; v < nvec; v += gridDim.x * C_BLOCK) {
    const size_t i = (size_t)v * VEC;
    bool ok[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) ok[e] = true;
    for (int band = 0; band < c; ++band) {
      const size_t at = (size_t)band * npix + i;
      const auto sa = load_item<S, VEC>(a + at);
#pragma unroll
      for (int e = 0; e < VEC; ++e) ok[e] = ok[e] && sample_valid<S>(sa[e], has_nd, nd);
      if (b) {
        const auto sb = load_item<S, VEC>(b + at);
#pragma unroll
        for (int e = 0; e < VEC; ++e) ok[e] = ok[e] && sample_valid<S>(sb[e], has_nd, nd);
      }
    }
    if (mask) {
      const auto m = load_item<uint8_t, VEC>(mask + i);
#pragma unroll
      for (int e = 0; e < VEC; ++e) ok[e] = ok[e] && m[e] != 0;
    }
    typename Item<uint8_t, VEC>::vec r;
#pragma unroll
    for (int e = 0; e < VEC; ++e) r[e] = ok[e] ? 1 : 0;
    store_item<uint8_t, VEC>(region + i, r);
  }
  // the last npix % VEC pixels, one per lane of the first workgroup
  if (blockIdx.x == 0 && (int)threadIdx.x < npix - nvec * VEC) {
    const int i = nvec * VEC + (int)threadIdx.x;
    bool ok = !mask || mask[i] != 0;
    for (int band = 0; band < c; ++band) {
      const size_t at = (size_t)band * npix + i;
      ok = ok && sample_valid<S>(a[at], has_nd, nd) && (!b || sample_valid<S>(b[at], has_nd, nd));
    }
    region[i] = ok ? 1 : 0;
  }
}

// ---------------------------------------------------------------- histogram
// grid: c * strips workgroups; priv: `split` words of dynamic LDS (none for split = 0) for the bins BIAS ... BIAS + split - 1, the values
// 0 ... split - 1.  bin < Bins<S>::N by the type; priv[rel] only for 0 <= rel < split (one unsigned compare).
template <typename S>
__global__ __launch_bounds__(H_BLOCK) void histogram_kernel(const S* __restrict__ src, const uint8_t* __restrict__ region, uint32_t* __restrict__ hist,
                                                            int npix, int strips, int split) {
  extern __shared__ unsigned priv[];
  constexpr int VEC = 16 / sizeof(S);
  const int tid = threadIdx.x;
  const int band = blockIdx.x / strips, strip = blockIdx.x - band * strips;
  const int begin = strip * H_STRIP, end = (int)min((long long)npix, (long long)begin + H_STRIP);          // strips = ceil(npix / H_STRIP): begin < npix < 2^31
  const S* plane = src + (size_t)band * npix;
  uint32_t* gh = hist + (size_t)band * Bins<S>::N;
  for (int k = tid; k < split; k += H_BLOCK) priv[k] = 0;
  __syncthreads();
  auto count = [&](S s) {
    const int bin = bin_of<S>(s), rel = bin - Bins<S>::BIAS;
    if ((unsigned)rel < (unsigned)split) atomicAdd(&priv[rel], 1u);
    else atomicAdd(&gh[bin], 1u);
  };
  const int nvec = (end - begin) / VEC;
  for (int v = tid; v < nvec; v += H_BLOCK) {
    const size_t i = (size_t)begin + (size_t)v * VEC;
    const auto s = load_item<S, VEC>(plane + i);
    const auto m = load_item<uint8_t, VEC>(region + i);
#pragma unroll
    for (int e = 0; e < VEC; ++e)
      if (m[e]) count(s[e]);
  }
  const int rest = begin + nvec * VEC;                                          // fewer than VEC samples remain
  if (tid < end - rest && region[rest + tid]) count(plane[rest + tid]);
  __syncthreads();
  for (int k = tid; k < split; k += H_BLOCK) {
    const unsigned n = priv[k];
    if (n) atomicAdd(&gh[Bins<S>::BIAS + k], n);                      // split <= 32768: inside the band's row
  }
}

// ---------------------------------------------------------------- the table kernels
// inclusive scan of one value per lane over the workgroup (Hillis-Steele in LDS); sh has blockDim.x words
__device__ __forceinline__ unsigned block_scan(unsigned* sh, unsigned v) {
  const int tid = threadIdx.x, n = blockDim.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < n; o <<= 1) {
    const unsigned t = tid >= o ? sh[tid - o] : 0u;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  return sh[tid];
}

// the smallest bin u with cum[u] * mul >= target, given cum[N - 1] * mul >= target: the first chunk whose inclusive sum reaches the
// target (binary search over the scanned chunk sums in LDS), then a walk inside that chunk
template <int THREADS, int CH>
__device__ __forceinline__ int first_bin(const unsigned* chunk_cum, const uint32_t* __restrict__ h, unsigned long long mul, unsigned long long target) {
  int lo = 0, hi = THREADS - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned long long)chunk_cum[mid] * mul >= target) hi = mid;
    else lo = mid + 1;
  }
  unsigned run = lo ? chunk_cum[lo - 1] : 0u;
  int u = lo * CH + CH - 1;
  bool found = false;
#pragma unroll 8
  for (int j = 0; j < CH; ++j) {
    run += h[lo * CH + j];
    if (!found && (unsigned long long)run * mul >= target) {
      u = lo * CH + j;
      found = true;
    }
  }
  return u;
}

template <typename S>
__global__ __launch_bounds__(Bins<S>::THREADS) void match_lut_kernel(const uint32_t* __restrict__ h1, const uint32_t* __restrict__ h2, S* __restrict__ lut,
                                                                     int64_t* __restrict__ counts) {
  constexpr int N = Bins<S>::N, THREADS = Bins<S>::THREADS, CH = N / THREADS;
  __shared__ unsigned c1[THREADS], c2[THREADS];
  const int tid = threadIdx.x, band = blockIdx.x;
  const uint32_t* g1 = h1 + (size_t)band * N;
  const uint32_t* g2 = h2 + (size_t)band * N;
  unsigned s1 = 0, s2 = 0;
#pragma unroll 8
  for (int e = 0; e < CH; ++e) {
    s1 += g1[tid * CH + e];
    s2 += g2[tid * CH + e];
  }
  block_scan(c1, s1);
  unsigned run2 = block_scan(c2, s2) - s2;
  const unsigned long long n1 = c1[THREADS - 1], n2 = c2[THREADS - 1];
  if (tid == 0 && counts) {
    counts[2 * band] = (int64_t)n1;
    counts[2 * band + 1] = (int64_t)n2;
  }
  S* out = lut + (size_t)band * N + tid * CH;
  if (n1 == 0 || n2 == 0) {                                          // (the same answer in every lane)
    for (int e = 0; e < CH; ++e) out[e] = value_of<S>(tid * CH + e);
    return;
  }
  for (int e = 0; e < CH; ++e) {
    run2 += g2[tid * CH + e];
    // (below image 2's smallest occupied bin the count is 0 and bin 0 would answer, occupied or not: it counts as 1)
    out[e] = value_of<S>(first_bin<THREADS, CH>(c1, g1, n2, (unsigned long long)(run2 ? run2 : 1u) * n1));
  }
}

template <typename S>
__global__ __launch_bounds__(Bins<S>::THREADS) void scale_lut_kernel(const uint32_t* __restrict__ h, int p, float* __restrict__ table, int32_t* __restrict__ upper) {
  constexpr int N = Bins<S>::N, THREADS = Bins<S>::THREADS, CH = N / THREADS;
  __shared__ unsigned cum[THREADS];
  const int tid = threadIdx.x, band = blockIdx.x;
  const uint32_t* g = h + (size_t)band * N;
  unsigned s = 0;
#pragma unroll 8
  for (int e = 0; e < CH; ++e) s += g[tid * CH + e];
  block_scan(cum, s);
  const unsigned long long n = cum[THREADS - 1];
  float* out = table + (size_t)band * N + tid * CH;
  int up = -1;
  if (n) up = (int)value_of<S>(first_bin<THREADS, CH>(cum, g, 100ull, (unsigned long long)p * n));
  if (tid == 0) upper[band] = up;
  const bool none = n == 0 || up == 0;
  for (int e = 0; e < CH; ++e) {
    const int v = (int)value_of<S>(tid * CH + e);
    out[e] = none ? NAN : (float)((double)(v < up ? v : up) / (double)up);
  }
}

// ---------------------------------------------------------------- apply
// planar destination: blockIdx.y is the band; the gather runs for invalid samples too (every bin lies inside the table)
template <typename S, typename D>
__global__ __launch_bounds__(C_BLOCK) void apply_planar_kernel(const S* src, const D* __restrict__ table, D* dst, int npix, int coff,
                                                               bool has_nd, S nd, bool keep, D fill) {
  constexpr int VEC = 16 / sizeof(S);
  const int band = blockIdx.y;
  const S* sp = src + (size_t)band * npix;
  const D* tb = table + (size_t)band * Bins<S>::N;
  D* dp = dst + (size_t)(coff + band) * npix;
  const int nvec = npix / VEC;
  for (int v = blockIdx.x * C_BLOCK + threadIdx.x; v < nvec; v += gridDim.x * C_BLOCK) {
    const size_t i = (size_t)v * VEC;
    const auto s = load_item<S, VEC>(sp + i);
    typename Item<D, VEC>::vec o;
    bool all = true;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      o[e] = tb[bin_of<S>(s[e])];
      all = all && sample_valid<S>(s[e], has_nd, nd);
    }
    if (all) {
      store_item<D, VEC>(dp + i, o);
    } else {
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        if (sample_valid<S>(s[e], has_nd, nd)) dp[i + e] = o[e];
        else if (!keep) dp[i + e] = fill;
      }
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < npix - nvec * VEC) {
    const int i = nvec * VEC + (int)threadIdx.x;
    const S s = sp[i];
    if (sample_valid<S>(s, has_nd, nd)) dp[i] = tb[bin_of<S>(s)];
    else if (!keep) dp[i] = fill;
  }
}

// pixel-interleaved destination: a lane takes one pixel and all its bands, so neighbouring lanes write neighbouring pixels
template <typename S, typename D>
__global__ __launch_bounds__(C_BLOCK) void apply_hwc_kernel(const S* __restrict__ src, const D* __restrict__ table, D* __restrict__ dst, int npix, int c,
                                                            int ld, int coff, bool has_nd, S nd, bool keep, D fill) {
  for (long long i = blockIdx.x * C_BLOCK + threadIdx.x; i < npix; i += gridDim.x * C_BLOCK) {
    D* dp = dst + (size_t)i * ld + coff;
    for (int band = 0; band < c; ++band) {
      const S s = src[(size_t)band * npix + i];
      const D o = table[(size_t)band * Bins<S>::N + bin_of<S>(s)];
      if (sample_valid<S>(s, has_nd, nd)) dp[band] = o;
      else if (!keep) dp[band] = fill;
    }
  }
}

// the checks every entry shares
int calib_shape_ok(const char* who, int kind, int c, int h, int w) {
  SATCV_CHECK(calib_kind_ok(kind), "%s: kind %d (0 u8, 1 u16, 3 i16; f32 and i32 rasters are not binned)", who, kind);
  SATCV_CHECK(c >= 1 && c <= 16, "%s: c = %d bands (1 ... 16)", who, c);
  SATCV_CHECK(h > 0 && w > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(satcv_pixels_ok(1, h, w, 1), "%s: map beyond 2^31 pixels", who);
  return SATCV_OK;
}

template <typename S, typename D>
int launch_apply(const satcv_calib_apply_desc* d, D fill, hipStream_t st) {
  S nd;
  const bool has_nd = nodata_in_kind<S>(d->has_nodata, d->nodata, nd);
  const int npix = d->h * d->w_;
  const S* src = reinterpret_cast<const S*>(d->src);
  const D* table = reinterpret_cast<const D*>(d->table);
  D* dst = reinterpret_cast<D*>(d->dst);
  if (d->dst_layout == 1)
    return satcv_launch(apply_planar_kernel<S, D>, dim3(stream_grid(npix / (16 / (int)sizeof(S))), d->c), dim3(C_BLOCK), 0, st, "calib_apply", src, table, dst, npix,
                        (int)d->dst_coff, has_nd, nd, d->keep != 0, fill);
  return satcv_launch(apply_hwc_kernel<S, D>, dim3(stream_grid(npix)), dim3(C_BLOCK), 0, st, "calib_apply", src, table, dst, npix, (int)d->c, (int)d->dst_ld,
                      (int)d->dst_coff, has_nd, nd, d->keep != 0, fill);
}

}  // namespace

extern "C" int satcv_calib_overlap(const void* a, const void* b, int32_t kind, int32_t c, int32_t h, int32_t w_, int32_t has_nodata, double nodata,
                                   const uint8_t* mask, uint8_t* region, void* stream) {
  SATCV_CHECK(a && region, "calib_overlap: null pointer (a, region)");
  { const int rc = calib_shape_ok("calib_overlap", kind, c, h, w_); if (rc) return rc; }
  const int npix = h * w_;
  return by_calib_kind(kind, [&](auto tag) -> int {
    typedef decltype(tag) S;
    S nd;
    const bool has_nd = nodata_in_kind<S>(has_nodata, nodata, nd);
    return satcv_launch(overlap_kernel<S>, dim3(stream_grid(npix / (16 / (int)sizeof(S)))), dim3(C_BLOCK), 0, (hipStream_t)stream, "calib_overlap",
                        reinterpret_cast<const S*>(a), reinterpret_cast<const S*>(b), mask, region, (int)c, npix, has_nd, nd);
  });
}

extern "C" int satcv_calib_histogram(const void* src, int32_t kind, int32_t c, int32_t h, int32_t w_, const uint8_t* region, uint32_t* hist,
                                     int32_t split, void* stream) {
  SATCV_CHECK(src && region && hist, "calib_histogram: null pointer (src, region, hist)");
  { const int rc = calib_shape_ok("calib_histogram", kind, c, h, w_); if (rc) return rc; }
  SATCV_CHECK(split <= H_SPLIT_MAX, "calib_histogram: split = %d private bins (at most %d)", split, H_SPLIT_MAX);
  const int npix = h * w_;
  const int strips = (int)(((long long)npix + H_STRIP - 1) / H_STRIP);
  const hipStream_t st = (hipStream_t)stream;
  return by_calib_kind(kind, [&](auto tag) -> int {
    typedef decltype(tag) S;
    constexpr int N = Bins<S>::N;
    SATCV_HIP(hipMemsetAsync(hist, 0, (size_t)c * N * sizeof(uint32_t), st));
    const int priv = split < 0 ? 0 : sizeof(S) == 1 ? N : split == 0 ? H_SPLIT : split;
    return satcv_launch(histogram_kernel<S>, dim3(c * strips), dim3(H_BLOCK), (size_t)priv * sizeof(unsigned), st, "calib_histogram",
                        reinterpret_cast<const S*>(src), region, hist, npix, strips, priv);
  });
}

extern "C" int satcv_calib_match_lut(const uint32_t* hist1, const uint32_t* hist2, int32_t kind, int32_t c, void* lut, int64_t* counts, void* stream) {
  SATCV_CHECK(hist1 && hist2 && lut, "calib_match_lut: null pointer (hist1, hist2, lut)");
  { const int rc = calib_shape_ok("calib_match_lut", kind, c, 1, 1); if (rc) return rc; }
  return by_calib_kind(kind, [&](auto tag) -> int {
    typedef decltype(tag) S;
    return satcv_launch(match_lut_kernel<S>, dim3(c), dim3(Bins<S>::THREADS), 0, (hipStream_t)stream, "calib_match_lut", hist1, hist2, reinterpret_cast<S*>(lut),
                        counts);
  });
}

extern "C" int satcv_calib_scale_lut(const uint32_t* hist, int32_t kind, int32_t c, int32_t p, float* table, int32_t* upper, void* stream) {
  SATCV_CHECK(hist && table && upper, "calib_scale_lut: null pointer (hist, table, upper)");
  { const int rc = calib_shape_ok("calib_scale_lut", kind, c, 1, 1); if (rc) return rc; }
  SATCV_CHECK(p >= 1 && p <= 100, "calib_scale_lut: p = %d (a percentile 1 ... 100)", p);
  return by_calib_kind(kind, [&](auto tag) -> int {
    typedef decltype(tag) S;
    return satcv_launch(scale_lut_kernel<S>, dim3(c), dim3(Bins<S>::THREADS), 0, (hipStream_t)stream, "calib_scale_lut", hist, (int)p, table, upper);
  });
}

extern "C" int satcv_calib_apply(const satcv_calib_apply_desc* d, void* stream) {
  SATCV_CHECK(d && d->src && d->table && d->dst, "calib_apply: null pointer (descriptor, src, table, dst)");
  { const int rc = calib_shape_ok("calib_apply", d->src_kind, d->c, d->h, d->w_); if (rc) return rc; }
  SATCV_CHECK(d->dst_kind == d->src_kind || d->dst_kind == 2, "calib_apply: dst_kind %d is neither the source kind %d nor 2 (f32)", d->dst_kind, d->src_kind);
  SATCV_CHECK(d->dst_layout == 0 || d->dst_layout == 1, "calib_apply: dst_layout %d (0 pixel-interleaved, 1 planar)", d->dst_layout);
  SATCV_CHECK(d->dst_coff >= 0 && d->dst_ld >= 1 && (long long)d->dst_coff + d->c <= d->dst_ld, "calib_apply: channels %d ... %d do not fit ld = %d", d->dst_coff,
              d->dst_coff + d->c - 1, d->dst_ld);
  const long long npix = (long long)d->h * d->w_;
  SATCV_CHECK(npix * d->dst_ld < (1LL << 40), "calib_apply: destination beyond 2^40 samples");
  const long long ssz = kind_bytes(d->src_kind), dsz = kind_bytes(d->dst_kind);
  const char* s0 = reinterpret_cast<const char*>(d->src);
  const char* d0 = reinterpret_cast<const char*>(d->dst);
  const bool in_place = d->dst_layout == 1 && d->dst_kind == d->src_kind && d0 + (long long)d->dst_coff * npix * dsz == s0;
  const bool apart = d0 + npix * d->dst_ld * dsz <= s0 || s0 + npix * d->c * ssz <= d0;
  SATCV_CHECK(in_place || apart, "calib_apply: dst overlaps src (in place is planar, of the source kind, band for band)");
  const hipStream_t st = (hipStream_t)stream;
  const bool f32 = d->dst_kind == 2;
  return by_calib_kind(d->src_kind, [&](auto tag) -> int {
    typedef decltype(tag) S;
    if (f32) return launch_apply<S, float>(d, NAN, st);
    S nd;
    nodata_in_kind<S>(d->has_nodata, d->nodata, nd);
    return launch_apply<S, S>(d, nd, st);
  });
}
