// Sentinel-2 quality masks of a resident time stack (utils/ee_tools.py on arrays), one launch:
//   basicQA :159-180 (QA60 cloud / cirrus bits), sentinelCloudScore :218-255 with the `cloudScore <= 15` of maskTOA :301, waterScore
//   :115-157 with the `<= 0.25` of mask :264, the `B11 > 900` shadow test of mask :267 and the scene classification of maskSR :270-286.
// src is (t, cs, h, w) planar; the outputs are the clear bit-planes (ceil(t / 32), h, w) uint32 that satcv_median_composite_masked
// reads -- a pixel's mask of up to 32 acquisitions is one register there --, the cloud score (t, h, w) uint8 and the water score
// (t, h, w) float32.  The rules and their exact-arithmetic definition are in include/satcv.h.
//
// Lanes run along the flattened (y, x) axis, so every (time, role) plane is read in full lines; 16-bit stacks give a lane TWO
// neighbouring pixels from one 32-bit load per plane (maps of one pixel: one pixel per lane).  Only the planes of the selected rules
// and outputs are read.  No branch at all surrounds a load: lanes past the end of the map repeat the last item and skip their stores.  The acquisitions of a pixel are walked in order and their bits gathered in a register that is
// stored once per 32 acquisitions.
// 16-bit kinds decide in integer arithmetic: every threshold as a cross-multiplied inequality (64-bit products for the z-score term
// of the water rule); the cloud score, where it is asked for, through floor divisions.  f32 stacks evaluate the same expressions in double.
#include "common.hpp"
#include <cmath>
#include <type_traits>

namespace {

constexpr int Q_BLOCK = 256;
constexpr int Q_MAX_GRID = 2048;     // workgroups; the rest is a grid-stride loop

enum { R_B1, R_B2, R_B3, R_B4, R_B8, R_B10, R_B11, R_B12, R_QA60, R_SCL };
constexpr unsigned bit(int r) { return 1u << r; }
constexpr unsigned NEED_CLOUD = bit(R_B1) | bit(R_B2) | bit(R_B3) | bit(R_B4) | bit(R_B8) | bit(R_B10) | bit(R_B11);
constexpr unsigned NEED_SHADOW = bit(R_B11);
constexpr unsigned NEED_WATER = bit(R_B2) | bit(R_B3) | bit(R_B4) | bit(R_B8) | bit(R_B11) | bit(R_B12);
constexpr unsigned SCL_MASKED = bit(0) | bit(2) | bit(3) | bit(8) | bit(9) | bit(10) | bit(11);

struct Args {
  satcv_quality_desc d;
  int npix;          // h * w
  int items;         // lanes of work: ceil(npix / pixels per lane)
  int plane[SATCV_Q_ROLES];   // the plane each role is loaded from: its own where the role is needed, else that of a needed role
};

struct __attribute__((packed, aligned(2))) Pair16 { unsigned v; };     // a plane of an odd map starts on a 2-byte boundary
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef short i16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- exact helpers, int (16-bit stacks) and double (f32 stacks)
// floor(a / b) for b > 0 and |a / b| <= 1000: a float estimate (off by less than 1: (float)a, the reciprocal and the product err by
// 2^-21 relative together) and one exact correction step either way
__device__ __forceinline__ int floor_quot(int a, int b) {
  int q = (int)floorf((float)a * __builtin_amdgcn_rcpf((float)b));
  const int r = a - q * b;
  return q + (r >= b) - (r < 0);
}
// the quotient of two integers is either an integer (then the division is exact) or at least 1 / b away from one: the floor of the
// correctly rounded double quotient is the floor of the rational
__device__ __forceinline__ double floor_quot(double a, double b) { return floor(a / b); }

// floor(a / C) for a >= 0 and a constant: an unsigned division the compiler turns into a multiplication
template <int C>
__device__ __forceinline__ int floor_const(int a) { return (int)((unsigned)a / (unsigned)C); }
template <int C>
__device__ __forceinline__ double floor_const(double a) { return floor(a / (double)C); }

// L^2 > 16 (5 sq - sum^2): 64-bit products for the integers (L <= 20 * 65535, sq <= 5 * 65535^2)
__device__ __forceinline__ bool z_above_quarter(int L, int sum, long long sq) {
  return (long long)L * L > 16 * (5 * sq - (long long)sum * sum);
}
__device__ __forceinline__ bool z_above_quarter(double L, double sum, double sq) { return L * L > 16.0 * (5.0 * sq - sum * sum); }

template <typename T> struct Wide { typedef long long type; };
template <> struct Wide<double> { typedef double type; };

// floor(min(100, t1 ... t6)) limited to 0 ... 100 (sentinelCloudScore :218-255, `.multiply(100).byte()`); x: harmonised DN by role
template <typename T>
__device__ __forceinline__ int cloud_score_of(const T (&x)[8]) {
  // (B2 - 1000) / 40 = B2 / 40 - 25 and so on: the numerators stay >= 0 (2040 = 34 * 60)
  T s = floor_const<40>(x[R_B2]) - (T)25;
  const T f2 = floor_const<20>(x[R_B1]) - (T)50;
  const T f3 = floor_const<5>(x[R_B1] + x[R_B10]) - (T)300;
  const T f4 = floor_const<60>(x[R_B2] + x[R_B3] + x[R_B4] + (T)40) - (T)34;
  const T d5 = x[R_B8] + x[R_B11], d6 = x[R_B3] + x[R_B11];
  const T one = (T)1;
  // a zero denominator: the normalised difference is 0 (satcv.h); the division runs on 1 and its result is dropped
  const T q5 = floor_quot((T)500 * (x[R_B8] - x[R_B11]), d5 > (T)0 ? d5 : one);
  const T q6 = floor_quot((T)500 * (x[R_B11] - x[R_B3]), d6 > (T)0 ? d6 : one);
  const T f5 = (d5 > (T)0 ? q5 : (T)0) + (T)50;
  const T f6 = (d6 > (T)0 ? q6 : (T)0) + (T)400;
  s = s < f2 ? s : f2;
  s = s < f3 ? s : f3;
  s = s < f4 ? s : f4;
  s = s < f5 ? s : f5;
  s = s < f6 ? s : f6;
  s = s < (T)100 ? s : (T)100;
  s = s > (T)0 ? s : (T)0;
  return (int)s;
}

// all three terms of waterScore (:115-157) above 1/4, division-free
template <typename T>
__device__ __forceinline__ bool is_water(const T (&x)[8]) {
  typedef typename Wide<T>::type W;
  const bool w1 = x[R_B8] + x[R_B11] + x[R_B12] < (T)3125;                   // (3500 - S) / 1500 > 1/4
  const T sum = x[R_B3] + x[R_B4] + x[R_B8] + x[R_B11] + x[R_B12];
  const W sq = (W)x[R_B3] * (W)x[R_B3] + (W)x[R_B4] * (W)x[R_B4] + (W)x[R_B8] * (W)x[R_B8] + (W)x[R_B11] * (W)x[R_B11] + (W)x[R_B12] * (W)x[R_B12];
  const T L = (T)20 * x[R_B2] - sum;                                         // (B2 - sd) / mean > 1/4  <=>  L > 4 sqrt(5 sq - sum^2), mean > 0
  const bool w2 = sum > (T)0 && L > (T)0 && z_above_quarter(L, sum, sq);
  const bool w3 = (T)40 * (x[R_B3] - x[R_B11]) > (T)17 * (x[R_B3] + x[R_B11]);      // ((B3 - B11) / (B3 + B11) - 0.3) / 0.5 > 1/4; false for 0 / 0
  return w1 && w2 && w3;
}

// waterScore in double, rounded once by the caller
template <typename T>
__device__ __forceinline__ double water_score_of(const T (&x)[8]) {
  const double b2 = (double)x[R_B2], b3 = (double)x[R_B3], b4 = (double)x[R_B4], b8 = (double)x[R_B8], b11 = (double)x[R_B11], b12 = (double)x[R_B12];
  const double w1 = fmin(fmax((3500.0 - (b8 + b11 + b12)) / 1500.0, 0.0), 1.0);
  const double sum = b3 + b4 + b8 + b11 + b12;
  const double sq = b3 * b3 + b4 * b4 + b8 * b8 + b11 * b11 + b12 * b12;
  const double sd = sqrt(fmax(5.0 * sq - sum * sum, 0.0)) / 5.0;
  const double w2 = sum > 0.0 ? fmin(fmax((b2 - sd) / (sum / 5.0), 0.0), 1.0) : 0.0;
  const double nd = b3 + b11 > 0.0 ? (b3 - b11) / (b3 + b11) : 0.0;
  const double w3 = (nd - 0.3) / 0.5;
  return fmin(fmax(fmin(fmin(1.0, w1), fmin(w2, w3)), 0.0), 1.0);
}

// a code (QA60, SCL) as an integer; ok = false for a NaN of an f32 stack
__device__ __forceinline__ int code_of(float v, bool& ok) {
  ok = v == v;
  return (int)fminf(fmaxf(ok ? v : 0.f, -2147483648.f), 2147483520.f);
}

// cloud_score <= cm for 0 <= cm < 100 without the score: some term below m = cm + 1, each as a cross-multiplied inequality
// (t5 < m  <=>  (550 - m) B8 < (450 + m) B11,  t6 < m  <=>  (900 - m) B11 < (100 + m) B3; a zero denominator leaves the constants 50, 400)
template <typename T>
__device__ __forceinline__ bool cloud_below(const T (&x)[8], int cm) {
  const T m = (T)(cm + 1);
  const T d5 = x[R_B8] + x[R_B11], d6 = x[R_B3] + x[R_B11];
  bool c = x[R_B2] < (T)1000 + (T)40 * m;
  c = c || x[R_B1] < (T)1000 + (T)20 * m;
  c = c || x[R_B1] + x[R_B10] < (T)1500 + (T)5 * m;
  c = c || x[R_B2] + x[R_B3] + x[R_B4] < (T)2000 + (T)60 * m;
  c = c || (d5 > (T)0 ? ((T)550 - m) * x[R_B8] < ((T)450 + m) * x[R_B11] : (T)50 < m);
  c = c || (d6 > (T)0 ? ((T)900 - m) * x[R_B11] < ((T)100 + m) * x[R_B3] : (T)400 < m);
  return c;
}

// ---------------------------------------------------------------- one sample of one pixel
// x: the harmonised DN by role (0 where nodata); vcloud / vshadow / vwater: every band the rule reads is valid; qa, scl: the codes
// (qa_ok / scl_ok false for a NaN of an f32 stack).  Every `rules` / output test is wave-uniform.
template <typename T>
__device__ __forceinline__ void sample(const Args& a, const T (&x)[8], bool vcloud, bool vshadow, bool vwater, int qa, bool qa_ok, int scl, bool scl_ok,
                                       bool& clear, int& cloud, float& water) {
  const satcv_quality_desc& d = a.d;
  bool pass = true;
  if (d.rules & SATCV_Q_QA60) pass = pass && qa_ok && (qa & (1024 | 2048)) == 0;
  if (d.rules & SATCV_Q_SCL) pass = pass && scl_ok && !(scl >= 0 && scl < 32 && ((SCL_MASKED >> scl) & 1u));
  if (d.cloud_score) {
    const int s = cloud_score_of<T>(x);
    cloud = vcloud ? s : 255;
    if (d.rules & SATCV_Q_CLOUD) pass = pass && vcloud && s <= d.cloud_max;
  } else if (d.rules & SATCV_Q_CLOUD) {
    // the same decision without the score: cloud_score is 0 ... 100, so cloud_max < 0 passes nothing and cloud_max >= 100 everything
    pass = pass && vcloud && (d.cloud_max >= 100 || (d.cloud_max >= 0 && cloud_below<T>(x, d.cloud_max)));
  }
  if (d.rules & SATCV_Q_SHADOW) pass = pass && vshadow && (float)x[R_B11] > d.shadow_min;
  if (d.rules & SATCV_Q_WATER) pass = pass && vwater && !is_water<T>(x);
  if (d.water_score) water = vwater ? (float)water_score_of<T>(x) : NAN;
  clear = pass;
}

// an acquisition's offset as loaded (see composite.hip): > 0 or 0, a scalar; 16-bit stacks take it rounded to an integer <= 65535
template <bool INTEGER>
__device__ __forceinline__ float offset_of(float o) {
  o = fmaxf(o, 0.f);
  if (INTEGER) o = fminf(rintf(o), 65535.f);
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(o)));
}

// ---------------------------------------------------------------- the kernel: S the stored type, PPL pixels per lane (2: 16-bit stacks, npix >= 2)
// All ten role planes are loaded in one branch-free group per acquisition, so their latencies overlap: a role that is not needed reads
// the plane of one that is (a.plane, the second load of a line is served by the cache and costs no memory traffic), and its value is
// never used.  16-bit pairs: the nodata rule (signed kinds: max(v, 0)), max(v, off) - off and the per-rule validity (the minimum over
// the rule's bands is > 0) are packed 16-bit instructions on both pixels; nodata stays 0 through the harmonisation.
template <typename S, int PPL>
__global__ __launch_bounds__(Q_BLOCK) void quality_kernel(const Args a) {
  constexpr bool F32 = std::is_same<S, float>::value;
  typedef typename std::conditional<F32, double, int>::type T;     // the arithmetic of the decisions
  const satcv_quality_desc& d = a.d;
  const S* __restrict__ src = reinterpret_cast<const S*>(d.src);
  const int t = d.t, npix = a.npix, tid = threadIdx.x;
  const size_t step = (size_t)d.cs * npix;                          // elements per acquisition
  for (int base = blockIdx.x * Q_BLOCK; base < a.items; base += gridDim.x * Q_BLOCK) {
    const bool live = base + tid < a.items;
    const int it = live ? base + tid : a.items - 1;
    // PPL = 2: the last lane of an odd map holds ONE pixel: it loads the pair that ends on it and shifts
    const bool tail = PPL == 2 && 2 * it + 1 >= npix;
    const size_t e0 = PPL == 2 ? (tail ? (size_t)npix - 2 : (size_t)2 * it) : (size_t)it;
    const size_t pix0 = PPL == 2 ? (tail ? (size_t)npix - 1 : (size_t)2 * it) : (size_t)it;
    const int np = (PPL == 2 && !tail) ? 2 : 1;                      // pixels this lane stores
    unsigned word[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) word[p] = 0;
    float off_next = d.offsets ? d.offsets[0] : 0.f;
    for (int j = 0; j < t; ++j) {
      const S* at = src + (size_t)j * step + e0;
      // the next acquisition's offset is loaded with this one's planes (its index stays inside the table), so no iteration waits for it alone
      const float off_now = off_next;
      off_next = d.offsets ? d.offsets[j + 1 < t ? j + 1 : j] : 0.f;
      T x[PPL][8];
      bool vcloud[PPL], vshadow[PPL], vwater[PPL], qa_ok[PPL], scl_ok[PPL];
      int qa[PPL], scl[PPL];
      if constexpr (PPL == 2) {
        const unsigned o = (unsigned)offset_of<true>(off_now);
        const u16x2 off = {(unsigned short)o, (unsigned short)o}, zero = {0, 0};
        u16x2 v[SATCV_Q_ROLES], h[8];
#pragma unroll
        for (int r = 0; r < SATCV_Q_ROLES; ++r) {
          unsigned w = reinterpret_cast<const Pair16*>(at + (size_t)a.plane[r] * npix)->v;
          w = tail ? w >> 16 : w;
          v[r] = __builtin_bit_cast(u16x2, w);
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          if (std::is_signed<S>::value) v[r] = __builtin_bit_cast(u16x2, __builtin_elementwise_max(__builtin_bit_cast(i16x2, v[r]), __builtin_bit_cast(i16x2, zero)));
          h[r] = __builtin_elementwise_max(v[r], off) - off;
        }
        auto lo = [](u16x2 p, u16x2 q) { return __builtin_elementwise_min(p, q); };
        const u16x2 m37 = lo(v[R_B3], v[R_B4]), m8b = lo(v[R_B8], v[R_B11]), m2 = lo(lo(m37, m8b), v[R_B2]);      // B2, B3, B4, B8, B11
        const u16x2 mc = lo(m2, lo(v[R_B1], v[R_B10])), mw = lo(m2, v[R_B12]);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int r = 0; r < 8; ++r) x[p][r] = (int)h[r][p];
          vcloud[p] = mc[p] != 0;
          vwater[p] = mw[p] != 0;
          vshadow[p] = v[R_B11][p] != 0;
          qa[p] = std::is_signed<S>::value ? (int)(short)v[R_QA60][p] : (int)v[R_QA60][p];
          scl[p] = std::is_signed<S>::value ? (int)(short)v[R_SCL][p] : (int)v[R_SCL][p];
          qa_ok[p] = scl_ok[p] = true;
        }
      } else {
        const float off = offset_of<!F32>(off_now);
        float v[SATCV_Q_ROLES];
#pragma unroll
        for (int r = 0; r < SATCV_Q_ROLES; ++r) v[r] = (float)at[(size_t)a.plane[r] * npix];       // 16-bit values are exact in fp32
        bool ok[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          ok[r] = v[r] > 0.f;                                          // NaN and negative values are nodata
          x[0][r] = ok[r] ? (T)(fmaxf(v[r], off) - off) : (T)0;       // f32: rounded to fp32, the sample the composite sees
        }
        const bool m2 = ok[R_B2] && ok[R_B3] && ok[R_B4] && ok[R_B8] && ok[R_B11];
        vcloud[0] = m2 && ok[R_B1] && ok[R_B10];
        vwater[0] = m2 && ok[R_B12];
        vshadow[0] = ok[R_B11];
        qa[0] = code_of(v[R_QA60], qa_ok[0]);
        scl[0] = code_of(v[R_SCL], scl_ok[0]);
      }
#pragma unroll
      for (int p = 0; p < PPL; ++p) {
        bool clear = false;
        int cloud = 255;
        float water = NAN;
        sample<T>(a, x[p], vcloud[p], vshadow[p], vwater[p], qa[p], qa_ok[p], scl[p], scl_ok[p], clear, cloud, water);
        word[p] |= (clear ? 1u : 0u) << (j & 31);
        if (live && p < np) {
          const size_t o = (size_t)j * npix + pix0 + p;
          if (d.cloud_score) d.cloud_score[o] = (uint8_t)cloud;
          if (d.water_score) d.water_score[o] = water;
        }
      }
      if ((j & 31) == 31 || j == t - 1) {                            // wave-uniform condition
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          if (d.clear && live && p < np) d.clear[(size_t)(j >> 5) * npix + pix0 + p] = word[p];
          word[p] = 0;
        }
      }
    }
  }
}

template <typename K>
int launch(K kern, const Args& a, hipStream_t st) {
  int grid = (a.items + Q_BLOCK - 1) / Q_BLOCK;
  if (grid > Q_MAX_GRID) grid = Q_MAX_GRID;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(Q_BLOCK), 0, st, a);
  return SATCV_OK;
}

}  // namespace

extern "C" int satcv_quality_mask(const satcv_quality_desc* d, void* stream) {
  SATCV_CHECK(d && d->src, "quality_mask: null pointer (src)");
  SATCV_CHECK(d->clear || d->cloud_score || d->water_score, "quality_mask: every output is null");
  SATCV_CHECK(d->t > 0 && d->cs > 0 && d->h > 0 && d->w_ > 0, "quality_mask: sizes must be positive");
  SATCV_CHECK(d->cs <= 16, "quality_mask: cs = %d planes per acquisition (at most 16)", d->cs);
  SATCV_CHECK(d->src_kind >= 1 && d->src_kind <= 3, "quality_mask: src_kind %d (1 u16, 2 f32, 3 i16)", d->src_kind);
  SATCV_CHECK(d->t <= SATCV_COMPOSITE_MAX_T, "quality_mask: t = %d acquisitions (at most %d)", d->t, SATCV_COMPOSITE_MAX_T);
  SATCV_CHECK(satcv_pixels_ok(1, d->h, d->w_, 1), "quality_mask: map beyond 2^31 pixels");
  SATCV_CHECK(d->rules || d->cloud_score || d->water_score, "quality_mask: no rule is selected and no score is asked for");
  SATCV_CHECK((d->rules & ~(SATCV_Q_QA60 | SATCV_Q_CLOUD | SATCV_Q_SHADOW | SATCV_Q_WATER | SATCV_Q_SCL)) == 0, "quality_mask: rules %d has unknown bits", d->rules);
  unsigned need = 0;
  if (d->rules & SATCV_Q_QA60) need |= bit(R_QA60);
  if (d->rules & SATCV_Q_SCL) need |= bit(R_SCL);
  if ((d->rules & SATCV_Q_CLOUD) || d->cloud_score) need |= NEED_CLOUD;
  if (d->rules & SATCV_Q_SHADOW) need |= NEED_SHADOW;
  if ((d->rules & SATCV_Q_WATER) || d->water_score) need |= NEED_WATER;
  static const char* const names[SATCV_Q_ROLES] = {"B1", "B2", "B3", "B4", "B8", "B10", "B11", "B12", "QA60", "SCL"};
  for (int r = 0; r < SATCV_Q_ROLES; ++r) {
    if (!((need >> r) & 1u)) continue;
    SATCV_CHECK(d->band[r] >= 0, "quality_mask: role %s is absent but a selected rule or output reads it", names[r]);
    SATCV_CHECK(d->band[r] < d->cs, "quality_mask: role %s at plane %d out of range (cs = %d)", names[r], d->band[r], d->cs);
  }
  Args a;
  a.d = *d;
  a.npix = d->h * d->w_;
  int first = 0;
  while (!((need >> first) & 1u)) ++first;                           // an output is non-null or a rule is set: some role is needed ...
  for (int r = 0; r < SATCV_Q_ROLES; ++r) a.plane[r] = d->band[((need >> r) & 1u) ? r : first];
  const hipStream_t st = (hipStream_t)stream;
  if (d->src_kind == 2) {
    a.items = a.npix;
    launch(quality_kernel<float, 1>, a, st);
  } else if (a.npix < 2) {
    a.items = a.npix;
    if (d->src_kind == 1) launch(quality_kernel<uint16_t, 1>, a, st);
    else launch(quality_kernel<int16_t, 1>, a, st);
  } else {
    a.items = (a.npix + 1) / 2;
    if (d->src_kind == 1) launch(quality_kernel<uint16_t, 2>, a, st);
    else launch(quality_kernel<int16_t, 2>, a, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    satcv_set_error("quality_mask launch: %s", hipGetErrorString(e));
    return SATCV_ERR_HIP;
  }
  return SATCV_OK;
}
