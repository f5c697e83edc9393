// Median composite of an image time stack (utils/pc_tools.py:620-668 `run_local`, left of the chip loop), one launch:
//   nodata (x > 0 else NaN, :376) -> harmonize_to_old (:284-326: max(x, offset) - offset for the acquisitions that carry an offset)
//   -> NaN-skipping median over time (:642-643) -> normalize_dataArray over the bands of a pixel (:90-107)
// src is (t, c, h, w) planar; both outputs are (h, w, ld) float32 at a channel offset, the layout scene_gather reads.
//
// Register path (t <= 32): lanes run along the flattened (y, x) axis, so every (time, band) plane is read in full lines.  The t samples
// of one band sit in registers and go through a compile-time Batcher merge-exchange network (instantiated for 4 / 8 / 16 / 32 slots).
// There is no select chain behind the network: nodata samples and the unused slots of an instantiation are keyed ALTERNATELY to the
// bottom (0) and the top (all ones / +inf) of the order, the first one to the bottom, so that with n valid samples among N slots the
// valid run is centred: n odd -> the median is slot N/2, n even -> the mean of slots N/2 - 1 and N/2, n = 0 -> NaN.  Only those two
// slots are read, so the compiler drops every compare-exchange that cannot reach them.  A valid 0 or a valid 65535 that ties with a
// key is harmless: tied slots hold equal values, and the count -- not the key -- says whether a slot is read.
//   16-bit stacks: a lane owns TWO neighbouring pixels in one register (one 32-bit load per sample pair); the nodata rule, the
//   harmonisation and every compare-exchange are packed 16-bit instructions (v_pk_max_i16 / v_pk_min_u16 / v_pk_max_u16 / v_pk_sub_u16).
//   f32 stacks: one pixel per lane, v_min_f32 / v_max_f32.
// The band medians of a pixel wait in LDS (8 bytes per band and pixel, private to the lane: no barrier) for the normalisation, which
// runs in double precision from the double medians and is rounded once on store.
// General path (32 < t <= SATCV_COMPOSITE_MAX_T, and maps of a single pixel): 64 lanes per workgroup, the samples of a band as ordered
// 32-bit keys in LDS, the k-th smallest found bit by bit (32 counting passes over LDS) -- exact, same trip count in every lane.
// No lane-dependent branch surrounds a load: lanes past the end of the map repeat the last item and skip their stores.
//
// satcv_median_composite_masked is a second instantiation of the same kernels (MaskedArgs): the composites the reference's models were
// trained on took the median over acquisitions masked by utils/ee_tools.py (basicQA :159, maskTOA :288, maskSR :270, mask :257).  A sample
// is valid iff v > 0 and its bit in the clear bit-planes of satcv_quality_mask (csrc/quality.hip) is set; the plane of output band b comes
// from a band table, so a stack that carries its quality planes is composited without a copy.  Register paths load the pixel's mask word
// once, outside the band loop; the packed 16-bit path folds the bit into the validity `m`.  The unmasked instantiations are unchanged.
#include "common.hpp"
#include <cmath>
#include <utility>

namespace {

constexpr int CP_BLOCK = 256;        // register path
constexpr int CP_GBLOCK = 64;        // general path
constexpr int CP_MAX_GRID = 2048;    // workgroups; the rest is a grid-stride loop

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

struct Args {
  satcv_composite_desc d;
  int npix;          // h * w
  int items;         // lanes of work: ceil(npix / pixels per lane)
  int vec_med, vec_norm;      // 16-byte stores possible (c, ld, coff multiples of 4, base 16-byte aligned)
  static constexpr bool masked = false;
};
// satcv_median_composite_masked: the same kernels, instantiated with a band table and the clear bit-planes of satcv_quality_mask
struct MaskedArgs : Args {
  const unsigned* clear;      // (ceil(t / 32), h, w) words, or null: every sample clear
  int cs;                     // planes per acquisition in src
  unsigned long long bands;   // the plane of output band b in bits [4 b, 4 b + 4): a scalar shift, no table in registers
  static constexpr bool masked = true;
};
// the plane of (acquisition j, output band b)
template <typename A>
__device__ __forceinline__ size_t plane_of(const A& a, int j, int c, int b) {
  if constexpr (A::masked) return (size_t)j * a.cs + (unsigned)((a.bands >> (4 * b)) & 15u);
  else return (size_t)j * c + b;
}
// an f32 sample takes part: > 0, and clear under a mask
template <typename A>
__device__ __forceinline__ int valid_of(float v, unsigned w, int j) {
  if constexpr (A::masked) return (v > 0.f) & (int)((w >> j) & 1u);
  else return v > 0.f;
}
// word k of pixel p's clear mask (a wave-uniform branch: all ones without a mask)
template <typename A>
__device__ __forceinline__ unsigned clear_word(const A& a, int k, size_t p) {
  if constexpr (A::masked) return a.clear ? a.clear[(size_t)k * a.npix + p] : 0xffffffffu;
  else return 0xffffffffu;
}

// ---------------------------------------------------------------- Batcher's merge-exchange network for N = 2^k slots
template <int N>
struct Net {
  int a[N * (N - 1) / 2 + 1], b[N * (N - 1) / 2 + 1];
  int n;
};
template <int N>
constexpr Net<N> make_net() {
  Net<N> r{};
  int q = 0;
  for (int p = 1; p < N; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= N - 1 - k; j += 2 * k)
        for (int i = 0; i <= (k - 1 < N - j - k - 1 ? k - 1 : N - j - k - 1); ++i)
          if ((i + j) / (p * 2) == (i + j + k) / (p * 2)) {
            r.a[q] = i + j;
            r.b[q] = i + j + k;
            ++q;
          }
  r.n = q;
  return r;
}

__device__ __forceinline__ void cex(u16x2& x, u16x2& y) {
  const u16x2 lo = __builtin_elementwise_min(x, y), hi = __builtin_elementwise_max(x, y);
  x = lo;
  y = hi;
}
__device__ __forceinline__ void cex(float& x, float& y) {
  const float lo = fminf(x, y), hi = fmaxf(x, y);
  x = lo;
  y = hi;
}
template <int N, int Q, typename E>
__device__ __forceinline__ void net_step(E (&s)[N]) {
  constexpr int ia = make_net<N>().a[Q], ib = make_net<N>().b[Q];
  cex(s[ia], s[ib]);
}
template <int N, typename E, size_t... Q>
__device__ __forceinline__ void net_apply(E (&s)[N], std::index_sequence<Q...>) {
  (net_step<N, (int)Q>(s), ...);
}
template <int N, typename E>
__device__ __forceinline__ void net_sort(E (&s)[N]) {
  net_apply<N>(s, std::make_index_sequence<make_net<N>().n>());
}

// median of n valid samples centred in N slots (see the head of the file), in double
__device__ __forceinline__ double centre_median(float below, float mid, int n) {
  if (n == 0) return NAN;
  return (n & 1) ? (double)mid : ((double)below + (double)mid) * 0.5;
}

// acquisition j's offset, > 0 or 0 (none), kept in a scalar register; 16-bit stacks take it rounded to an integer <= 65535 (satcv.h)
template <bool INTEGER>
__device__ __forceinline__ float offset_of(const float* offsets, int j, int t) {
  float o = (offsets && j < t) ? fmaxf(offsets[j], 0.f) : 0.f;
  if (INTEGER) o = fminf(rintf(o), 65535.f);
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(o)));
}

// ---------------------------------------------------------------- normalisation + stores of one pixel
// med: this lane's band medians in LDS, band b at med[b * stride].  mean / sd (ddof 0) over the bands that are present, in double.
__device__ __forceinline__ void finish_pixel(const Args& a, const double* med, int stride, size_t pix) {
  const satcv_composite_desc& d = a.d;
  const int c = d.c;
  int n = 0;
  double sum = 0.0;
  for (int b = 0; b < c; ++b) {
    const double m = med[b * stride];
    if (m == m) { sum += m; ++n; }
  }
  const double mean = sum / (double)n;                   // n == 0: NaN, every band is NaN anyway
  double ss = 0.0;
  for (int b = 0; b < c; ++b) {
    const double m = med[b * stride];
    if (m == m) ss += (m - mean) * (m - mean);
  }
  const double r = 1.0 / (sqrt(ss / (double)n) + 1e-6);  // one division per pixel; (m - mean) * r differs from the quotient by < 2^-52 relative
  if (d.median) {
    float* q = d.median + pix * d.ld_med + d.coff_med;
    if (a.vec_med) {
      for (int b = 0; b < c; b += 4)
        *reinterpret_cast<float4*>(q + b) = make_float4((float)med[b * stride], (float)med[(b + 1) * stride], (float)med[(b + 2) * stride], (float)med[(b + 3) * stride]);
    } else {
      for (int b = 0; b < c; ++b) q[b] = (float)med[b * stride];
    }
  }
  if (d.norm) {
    float* q = d.norm + pix * d.ld_norm + d.coff_norm;
    const bool fill = d.use_fill != 0;
    auto nv = [&](int b) {
      const float v = (float)((med[b * stride] - mean) * r);
      return (fill && v != v) ? d.fill : v;
    };
    if (a.vec_norm) {
      for (int b = 0; b < c; b += 4) *reinterpret_cast<float4*>(q + b) = make_float4(nv(b), nv(b + 1), nv(b + 2), nv(b + 3));
    } else {
      for (int b = 0; b < c; ++b) q[b] = nv(b);
    }
  }
}

// ---------------------------------------------------------------- register path, 16-bit stacks: two pixels per lane
struct __attribute__((packed, aligned(2))) Pair16 { unsigned v; };     // a plane of an odd map starts on a 2-byte boundary

template <bool SIGNED, int N, typename A>
__global__ __launch_bounds__(CP_BLOCK) void composite16_kernel(const A a) {
  extern __shared__ double cp_med[];                     // [c][2][CP_BLOCK]
  const satcv_composite_desc& d = a.d;
  const unsigned short* __restrict__ src = reinterpret_cast<const unsigned short*>(d.src);
  const int t = d.t, c = d.c, npix = a.npix, tid = threadIdx.x;
  const u16x2 one = {1, 1}, zero = {0, 0};
  unsigned off[N];                                       // (offset, offset) per acquisition
#pragma unroll
  for (int j = 0; j < N; ++j) off[j] = (unsigned)offset_of<true>(d.offsets, j, t) * 0x10001u;
  for (int base = blockIdx.x * CP_BLOCK; base < a.items; base += gridDim.x * CP_BLOCK) {
    const bool live = base + tid < a.items;
    const int it = live ? base + tid : a.items - 1;
    // the last lane of an odd map holds ONE pixel: it loads the pair that ends on it and shifts (npix >= 2 on this path)
    const bool tail = 2 * it + 1 >= npix;
    const size_t e0 = tail ? (size_t)npix - 2 : (size_t)2 * it;
    // the clear bits of the lane's two pixels, loaded once (N <= 32: one word each) and interleaved by halves, so that a shift by
    // j % 16 brings acquisition j's two bits to bit 0 of the two 16-bit fields: w01[j / 16] >> (j % 16) & 0x00010001
    unsigned w01[2] = {0, 0};
    if constexpr (A::masked) {
      const unsigned wx = clear_word(a, 0, tail ? (size_t)npix - 1 : e0), wy = clear_word(a, 0, tail ? (size_t)npix - 1 : e0 + 1);
      w01[0] = (wx & 0xffffu) | (wy << 16);
      w01[1] = (wx >> 16) | (wy & 0xffff0000u);
    }
    for (int b = 0; b < c; ++b) {
      u16x2 s[N];
      u16x2 par = zero, cnt = zero;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        unsigned raw = 0;
        if (j < t) raw = reinterpret_cast<const Pair16*>(src + plane_of(a, j, c, b) * npix + e0)->v;      // wave-uniform condition
        raw = tail ? raw >> 16 : raw;
        u16x2 v = __builtin_bit_cast(u16x2, raw);
        if (SIGNED) v = __builtin_bit_cast(u16x2, __builtin_elementwise_max(__builtin_bit_cast(i16x2, v), __builtin_bit_cast(i16x2, zero)));
        u16x2 valid = one;
        if constexpr (A::masked) valid = __builtin_bit_cast(u16x2, (w01[j / 16] >> (j % 16)) & 0x00010001u);      // the clear bits are part of `m`
        const u16x2 m = __builtin_elementwise_min(v, valid);      // 1 = valid (x > 0, and clear)
        const u16x2 inv = m ^ one;
        const u16x2 top = inv & par;                               // the 2nd, 4th, ... nodata sample goes to the top
        par ^= inv;
        cnt += m;
        const u16x2 o = __builtin_bit_cast(u16x2, off[j]);
        u16x2 u = __builtin_elementwise_max(v, o) - o;             // nodata stays 0: the bottom key
        if constexpr (A::masked) u *= m;                           // ... and a sample that is not clear becomes it
        s[j] = u | (zero - top);
      }
      net_sort<N>(s);
      cp_med[(b * 2 + 0) * CP_BLOCK + tid] = centre_median((float)s[N / 2 - 1].x, (float)s[N / 2].x, cnt.x);
      cp_med[(b * 2 + 1) * CP_BLOCK + tid] = centre_median((float)s[N / 2 - 1].y, (float)s[N / 2].y, cnt.y);
    }
    if (live) {
      finish_pixel(a, cp_med + tid, 2 * CP_BLOCK, tail ? (size_t)npix - 1 : (size_t)2 * it);
      if (!tail) finish_pixel(a, cp_med + CP_BLOCK + tid, 2 * CP_BLOCK, (size_t)2 * it + 1);
    }
  }
}

// ---------------------------------------------------------------- register path, f32 stacks: one pixel per lane
template <int N, typename A>
__global__ __launch_bounds__(CP_BLOCK) void composite32_kernel(const A a) {
  extern __shared__ double cp_med[];                     // [c][CP_BLOCK]
  const satcv_composite_desc& d = a.d;
  const float* __restrict__ src = reinterpret_cast<const float*>(d.src);
  const int t = d.t, c = d.c, npix = a.npix, tid = threadIdx.x;
  float off[N];
#pragma unroll
  for (int j = 0; j < N; ++j) off[j] = offset_of<false>(d.offsets, j, t);
  for (int base = blockIdx.x * CP_BLOCK; base < a.items; base += gridDim.x * CP_BLOCK) {
    const bool live = base + tid < a.items;
    const int it = live ? base + tid : a.items - 1;
    unsigned w = 0;                                       // the pixel's clear bits, loaded once (N <= 32: one word)
    if constexpr (A::masked) w = clear_word(a, 0, (size_t)it);
    for (int b = 0; b < c; ++b) {
      float s[N];
      int par = 0, cnt = 0;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        float v = 0.f;
        if (j < t) v = src[plane_of(a, j, c, b) * npix + it];         // wave-uniform condition
        const int valid = valid_of<A>(v, w, j);                    // NaN and negative values are nodata
        const int top = (valid ^ 1) & par;
        par ^= valid ^ 1;
        cnt += valid;
        s[j] = valid ? fmaxf(v, off[j]) - off[j] : (top ? INFINITY : 0.f);
      }
      net_sort<N>(s);
      cp_med[b * CP_BLOCK + tid] = centre_median(s[N / 2 - 1], s[N / 2], cnt);
    }
    if (live) finish_pixel(a, cp_med + tid, CP_BLOCK, (size_t)it);
  }
}

// ---------------------------------------------------------------- general path: any t up to SATCV_COMPOSITE_MAX_T
// keys: the float bits of a valid sample after the harmonisation (>= +0, so they order as unsigned integers), all ones for nodata
template <typename S, typename A>
__global__ __launch_bounds__(CP_GBLOCK) void composite_general_kernel(const A a) {
  extern __shared__ double cp_med[];                     // [c][CP_GBLOCK] doubles, then [t][CP_GBLOCK] keys
  const satcv_composite_desc& d = a.d;
  const S* __restrict__ src = reinterpret_cast<const S*>(d.src);
  const int t = d.t, c = d.c, npix = a.npix, tid = threadIdx.x;
  unsigned* key = reinterpret_cast<unsigned*>(cp_med + (size_t)c * CP_GBLOCK) + tid;
  for (int base = blockIdx.x * CP_GBLOCK; base < a.items; base += gridDim.x * CP_GBLOCK) {
    const bool live = base + tid < a.items;
    const int it = live ? base + tid : a.items - 1;
    for (int b = 0; b < c; ++b) {
      int n = 0;
      unsigned w = 0xffffffffu;
      for (int j = 0; j < t; ++j) {
        const float v = (float)src[plane_of(a, j, c, b) * npix + it];
        const float off = offset_of<!std::is_same<S, float>::value>(d.offsets, j, t);
        bool valid = v > 0.f;
        if constexpr (A::masked) {
          if ((j & 31) == 0) w = clear_word(a, j >> 5, (size_t)it);      // wave-uniform condition
          valid = valid && ((w >> (j & 31)) & 1u);
        }
        n += valid;
        key[j * CP_GBLOCK] = valid ? __float_as_uint(fmaxf(v, off) - off) : 0xffffffffu;
      }
      const int k = (n - 1) >> 1;                        // the lower middle of the valid samples (n == 0: unused)
      unsigned lo = 0;                                   // the largest x with #{key < x} <= k is the k-th smallest key
      for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = lo | (1u << bit);
        int less = 0;
        for (int j = 0; j < t; ++j) less += key[j * CP_GBLOCK] < cand;
        lo = less <= k ? cand : lo;
      }
      int le = 0;
      unsigned next = 0xffffffffu;                       // the upper middle: lo again if it is repeated, else the next key above it
      for (int j = 0; j < t; ++j) {
        const unsigned x = key[j * CP_GBLOCK];
        le += x <= lo;
        next = (x > lo && x < next) ? x : next;
      }
      const unsigned hi = le >= k + 2 ? lo : next;
      cp_med[b * CP_GBLOCK + tid] = centre_median(__uint_as_float(lo), __uint_as_float((n & 1) ? lo : hi), n);
    }
    if (live) finish_pixel(a, cp_med + tid, CP_GBLOCK, (size_t)it);
  }
}

template <typename K, typename A>
int launch(K kern, const A& a, int block, size_t lds, hipStream_t st) {
  const int rc = satcv_ensure_dynamic_lds(reinterpret_cast<const void*>(kern), lds);
  if (rc != SATCV_OK) return rc;
  int grid = (a.items + block - 1) / block;
  if (grid > CP_MAX_GRID) grid = CP_MAX_GRID;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, a);
  return SATCV_OK;
}

template <bool SIGNED, typename A>
int launch16(const A& a, hipStream_t st) {
  const size_t lds = (size_t)a.d.c * 2 * CP_BLOCK * sizeof(double);
  const int t = a.d.t;
  if (t <= 4) return launch(composite16_kernel<SIGNED, 4, A>, a, CP_BLOCK, lds, st);
  if (t <= 8) return launch(composite16_kernel<SIGNED, 8, A>, a, CP_BLOCK, lds, st);
  if (t <= 16) return launch(composite16_kernel<SIGNED, 16, A>, a, CP_BLOCK, lds, st);
  return launch(composite16_kernel<SIGNED, 32, A>, a, CP_BLOCK, lds, st);
}

template <typename A>
int launch32(const A& a, hipStream_t st) {
  const size_t lds = (size_t)a.d.c * CP_BLOCK * sizeof(double);
  const int t = a.d.t;
  if (t <= 4) return launch(composite32_kernel<4, A>, a, CP_BLOCK, lds, st);
  if (t <= 8) return launch(composite32_kernel<8, A>, a, CP_BLOCK, lds, st);
  if (t <= 16) return launch(composite32_kernel<16, A>, a, CP_BLOCK, lds, st);
  return launch(composite32_kernel<32, A>, a, CP_BLOCK, lds, st);
}

// the checks both entry points share
int check_desc(const satcv_composite_desc* d, const char* who) {
  SATCV_CHECK(d && d->src, "%s: null pointer (src)", who);
  SATCV_CHECK(d->median || d->norm, "%s: both outputs are null", who);
  SATCV_CHECK(d->t > 0 && d->c > 0 && d->h > 0 && d->w_ > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(d->c <= 16, "%s: c = %d bands (at most 16)", who, d->c);
  SATCV_CHECK(d->src_kind >= 1 && d->src_kind <= 3, "%s: src_kind %d (1 u16, 2 f32, 3 i16)", who, d->src_kind);
  SATCV_CHECK(!d->median || (d->coff_med >= 0 && d->ld_med > 0 && (long long)d->coff_med + d->c <= d->ld_med),
              "%s: median channel range (coff_med + c <= ld_med)", who);
  SATCV_CHECK(!d->norm || (d->coff_norm >= 0 && d->ld_norm > 0 && (long long)d->coff_norm + d->c <= d->ld_norm),
              "%s: norm channel range (coff_norm + c <= ld_norm)", who);
  SATCV_CHECK(d->t <= SATCV_COMPOSITE_MAX_T, "%s: t = %d acquisitions (at most %d)", who, d->t, SATCV_COMPOSITE_MAX_T);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "%s: map beyond 2^31 pixels", who);
  return SATCV_OK;
}

// a is complete but for the fields set here
template <typename A>
int run(A& a, const char* who, void* stream) {
  const satcv_composite_desc* d = &a.d;
  a.npix = d->h * d->w_;
  const bool c4 = d->c % 4 == 0;
  a.vec_med = d->median && c4 && d->ld_med % 4 == 0 && d->coff_med % 4 == 0 && (uintptr_t)d->median % 16 == 0;
  a.vec_norm = d->norm && c4 && d->ld_norm % 4 == 0 && d->coff_norm % 4 == 0 && (uintptr_t)d->norm % 16 == 0;
  const hipStream_t st = (hipStream_t)stream;
  int rc;
  if (d->t > 32 || a.npix < 2) {
    a.items = a.npix;
    const size_t lds = (size_t)CP_GBLOCK * (d->c * sizeof(double) + d->t * sizeof(unsigned));
    if (d->src_kind == 1) rc = launch(composite_general_kernel<uint16_t, A>, a, CP_GBLOCK, lds, st);
    else if (d->src_kind == 2) rc = launch(composite_general_kernel<float, A>, a, CP_GBLOCK, lds, st);
    else rc = launch(composite_general_kernel<int16_t, A>, a, CP_GBLOCK, lds, st);
  } else if (d->src_kind == 2) {
    a.items = a.npix;
    rc = launch32(a, st);
  } else {
    a.items = (a.npix + 1) / 2;
    rc = d->src_kind == 1 ? launch16<false>(a, st) : launch16<true>(a, st);
  }
  if (rc != SATCV_OK) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    satcv_set_error("%s launch: %s", who, hipGetErrorString(e));
    return SATCV_ERR_HIP;
  }
  return SATCV_OK;
}

}  // namespace

extern "C" int satcv_median_composite(const satcv_composite_desc* d, void* stream) {
  const int rc = check_desc(d, "median_composite");
  if (rc != SATCV_OK) return rc;
  Args a;
  a.d = *d;
  return run(a, "median_composite", stream);
}

extern "C" int satcv_median_composite_masked(const satcv_composite_masked_desc* d, void* stream) {
  SATCV_CHECK(d, "median_composite_masked: null pointer (descriptor)");
  const int rc = check_desc(&d->base, "median_composite_masked");
  if (rc != SATCV_OK) return rc;
  SATCV_CHECK(d->cs >= 1 && d->cs <= 16, "median_composite_masked: cs = %d planes per acquisition (1 ... 16)", d->cs);
  for (int b = 0; b < d->base.c; ++b)
    SATCV_CHECK(d->band_idx[b] >= 0 && d->band_idx[b] < d->cs, "median_composite_masked: band_idx[%d] = %d out of range (cs = %d)", b, d->band_idx[b], d->cs);
  MaskedArgs a;
  a.d = d->base;
  a.clear = d->clear;
  a.cs = d->cs;
  a.bands = 0;
  for (int b = 0; b < d->base.c; ++b) a.bands |= (unsigned long long)d->band_idx[b] << (4 * b);
  return run(a, "median_composite_masked", stream);
}
