// What satcv_raster_warp (warp.hip) and satcv_raster_reproject (reproject.hip) share: the descriptor checks, the launch plan and the
// per-pixel part of the kernels -- taps, weights, validity, rounding and the band packs of include/satcv.h, "Raster alignment".  The two
// kernels differ only in where a destination pixel's source-grid coordinates (u, v) come from: `warp_pixels` takes them from a functor.
//   Coord::operator()(d, gi, gj, u, v)   the coordinates of the centre of the destination pixel (row gi, column gj), global indices as
//                                        doubles.  A pixel without coordinates gets NaN: floor(NaN) is NaN, `local_index` places it
//                                        outside every window, so every tap is invalid and the result is invalid -- no extra branch.
//   Coord::footprint(d, gi, gj, ...)     the axis-parallel footprint of the average rule (method 3); only the affine map has one.
// Include after `#pragma clang fp contract(off)`: u = su * (j + 0.5) + ou as a fused multiply-add moves floor(u) on real grids.
#pragma once
#include "common.hpp"
#include "raster_kinds.hpp"

namespace {

constexpr int WP_BLOCK = 256;
constexpr int WP_MAX_GRID = 8192;        // 256 CUs x 8 workgroups x 4: the rest is the grid-stride loop

template <typename T, int N>
struct alignas(sizeof(T) * N) Pack {
  T v[N];
};

// what the host derives from the descriptor once
struct WarpPlan {
  int ntx, nty;          // taps per axis of the average rule: ceil(|s|) + 1
  int vec_src, vec_dst;  // a pack of NB bands is one aligned load / store
};

template <typename D>
__device__ __forceinline__ D to_dst(double v) {
  if constexpr (std::is_same<D, float>::value) return (float)v;
  else {
    const double r = rint(v);                                          // half to even
    const double lo = (double)std::numeric_limits<D>::min(), hi = (double)std::numeric_limits<D>::max();
    if (r <= lo) return std::numeric_limits<D>::min();
    if (r >= hi) return std::numeric_limits<D>::max();
    return (D)r;
  }
}

// NB bands from b0 on of the source pixel (y, x) of the window (inside it)
template <typename S, int NB>
__device__ __forceinline__ void load_pack(const S* __restrict__ src, const satcv_warp_desc& d, int vec, int y, int x, int b0, S (&out)[NB]) {
  const long long pix = (long long)y * d.sw + x;
  if (d.src_layout == 0) {
    const S* p = src + pix * d.src_ld + d.src_coff + b0;
    if (NB > 1 && vec) {
      const Pack<S, NB> q = *reinterpret_cast<const Pack<S, NB>*>(p);
#pragma unroll
      for (int k = 0; k < NB; ++k) out[k] = q.v[k];
    } else {
#pragma unroll
      for (int k = 0; k < NB; ++k) out[k] = p[k];
    }
  } else {
    const long long plane = (long long)d.sh * d.sw;
#pragma unroll
    for (int k = 0; k < NB; ++k) out[k] = src[(long long)(d.src_coff + b0 + k) * plane + pix];
  }
}

// the local index of a source-grid coordinate (an integer-valued double) on an axis of n samples from `origin` on: the origin is subtracted
// after floor; -1 outside the window (tested in float64: a coordinate far outside, or NaN, must not wrap an int)
__device__ __forceinline__ int local_index(double k, int origin, int n) {
  const double l = k - (double)origin;
  return (l >= 0.0 && l < (double)n) ? (int)l : -1;
}

// the affine map of satcv_raster_warp
struct AffineCoord {
  __device__ __forceinline__ void operator()(const satcv_warp_desc& d, double gi, double gj, double& u, double& v) const {
    u = d.su * (gj + 0.5) + d.ou;
    v = d.sv * (gi + 0.5) + d.ov;
  }
  __device__ __forceinline__ void footprint(const satcv_warp_desc& d, double gi, double gj, double& ulo, double& uhi, double& vlo, double& vhi) const {
    const double ua = d.su * gj + d.ou, ub = d.su * (gj + 1.0) + d.ou;
    const double va = d.sv * gi + d.ov, vb = d.sv * (gi + 1.0) + d.ov;
    ulo = fmin(ua, ub); uhi = fmax(ua, ub);
    vlo = fmin(va, vb); vhi = fmax(va, vb);
  }
};

// Every destination pixel of the launch (grid-stride loop over 64-bit pixel indices), all its bands.  METHOD is the resampling rule: every
// loop over taps has compile-time bounds and a method carries only its own registers
template <typename S, typename D, int NB, int METHOD, typename Coord>
__device__ __forceinline__ void warp_pixels(const satcv_warp_desc& d, const WarpPlan& p, const D dst_nd, const int has_nd, const S src_nd, const Coord& coord) {
  const S* __restrict__ src = (const S*)d.src;
  D* __restrict__ dst = (D*)d.dst;
  const long long total = (long long)d.dh * d.dw;
  for (long long i = (long long)blockIdx.x * WP_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * WP_BLOCK) {
    const int li = (int)(i / d.dw), lj = (int)(i - (long long)li * d.dw);
    const double gj = (double)((long long)d.dst_col0 + lj), gi = (double)((long long)d.dst_row0 + li);
    // ---- taps and weights of this pixel: the same for every band
    constexpr int T0 = METHOD == 2 ? 0 : 1, T1 = METHOD == 2 ? 3 : METHOD == 1 ? 2 : 1;      // methods 0-2: tap range per axis (nearest: tap 1 alone)
    int ix[4];                                                // columns: local index per tap, -1 outside the window
    bool hx[4];                                               //          the tap lies in the pixel that contains the point
    double cwx[4], bwx[4];                                    //          cubic and bilinear weights
    int iy1 = -1;                                             // nearest: the row
    double y0 = 0.0, cy = 0.0, s = 0.0, s2 = 0.0, s3 = 0.0;   // rows: taps, flags and weights are made per row in the tap loop
    double ulo = 0.0, uhi = 0.0, vlo = 0.0, vhi = 0.0;        // method 3: the footprint
    if constexpr (METHOD == 3) {
      coord.footprint(d, gi, gj, ulo, uhi, vlo, vhi);
    } else {
      double u, v;
      coord(d, gi, gj, u, v);
      const double cx = floor(u);
      cy = floor(v);
      if constexpr (METHOD == 0) {
        ix[1] = local_index(cx, d.src_col0, d.sw);
        iy1 = local_index(cy, d.src_row0, d.sh);
      } else {
        const double x0 = floor(u - 0.5);
        const double t = u - 0.5 - x0;
        y0 = floor(v - 0.5);
        s = v - 0.5 - y0;
#pragma unroll
        for (int k = T0; k <= T1; ++k) {
          const double kx = x0 + (double)(k - 1);
          ix[k] = local_index(kx, d.src_col0, d.sw);
          hx[k] = kx == cx;
        }
        bwx[1] = 1.0 - t; bwx[2] = t;
        if constexpr (METHOD == 2) {
          const double t2 = t * t, t3 = t2 * t;
          s2 = s * s; s3 = s2 * s;
          cwx[0] = -0.5 * t3 + t2 - 0.5 * t; cwx[1] = 1.5 * t3 - 2.5 * t2 + 1.0; cwx[2] = -1.5 * t3 + 2.0 * t2 + 0.5 * t; cwx[3] = 0.5 * t3 - 0.5 * t2;
        }
      }
    }
    for (int b0 = 0; b0 < d.c; b0 += NB) {
      D out[NB];
      bool ok[NB];
      if constexpr (METHOD == 0) {                            // a copy (a cast for f32 from an integer kind): no arithmetic
        const bool in = ix[1] >= 0 && iy1 >= 0;
        S smp[NB];
        if (in) load_pack<S, NB>(src, d, p.vec_src, iy1, ix[1], b0, smp);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          ok[k] = in && sample_valid<S>(smp[k], has_nd != 0, src_nd);
          out[k] = ok[k] ? (D)smp[k] : dst_nd;
        }
      } else {
        double val[NB];
        if constexpr (METHOD == 3) {
          double acc[NB], ws[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) { acc[k] = 0.0; ws[k] = 0.0; }
          const double ky0 = floor(vlo), kx0 = floor(ulo);
          for (int ty = 0; ty < p.nty; ++ty) {
            const double ky = ky0 + (double)ty, wy = fmin(vhi, ky + 1.0) - fmax(vlo, ky);
            const int ly = local_index(ky, d.src_row0, d.sh);
            if (!(wy > 0.0) || ly < 0) continue;
            for (int tx = 0; tx < p.ntx; ++tx) {
              const double kx = kx0 + (double)tx, wx = fmin(uhi, kx + 1.0) - fmax(ulo, kx);
              const int lx = local_index(kx, d.src_col0, d.sw);
              if (!(wx > 0.0) || lx < 0) continue;
              S smp[NB];
              load_pack<S, NB>(src, d, p.vec_src, ly, lx, b0, smp);
              const double w = wy * wx;
#pragma unroll
              for (int k = 0; k < NB; ++k) {
                const bool g = sample_valid<S>(smp[k], has_nd != 0, src_nd);
                acc[k] = g ? acc[k] + w * (double)smp[k] : acc[k];
                ws[k] = g ? ws[k] + w : ws[k];
              }
            }
          }
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            ok[k] = ws[k] > 0.0;
            val[k] = acc[k] / ws[k];
          }
        } else {
          double cacc[NB], bacc[NB], bws[NB];
          bool call[NB], centre[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) { cacc[k] = 0.0; bacc[k] = 0.0; bws[k] = 0.0; call[k] = true; centre[k] = false; }
          // one row of taps: its columns are unrolled, so their loads are in flight together.  The cubic rule runs its four rows as a
          // loop (all 16 taps unrolled need every register a lane can have); the row's weight is chosen by the row, not indexed
          auto row = [&](const int r) {
            const double ky = y0 + (double)(r - 1);
            const int iyr = local_index(ky, d.src_row0, d.sh);
            const bool hyr = ky == cy, rbil = r == 1 || r == 2;
            const double bwy = r == 1 ? 1.0 - s : s;
            double cwy = 0.0;
            if constexpr (METHOD == 2)
              cwy = r == 0 ? -0.5 * s3 + s2 - 0.5 * s : r == 1 ? 1.5 * s3 - 2.5 * s2 + 1.0 : r == 2 ? -1.5 * s3 + 2.0 * s2 + 0.5 * s : 0.5 * s3 - 0.5 * s2;
#pragma unroll
            for (int q = T0; q <= T1; ++q) {
              const bool in = iyr >= 0 && ix[q] >= 0;
              const bool bil = rbil && q >= 1 && q <= 2;              // a tap of the bilinear rule
              S smp[NB];
              if (in) load_pack<S, NB>(src, d, p.vec_src, iyr, ix[q], b0, smp);
#pragma unroll
              for (int k = 0; k < NB; ++k) {
                const bool g = in && sample_valid<S>(smp[k], has_nd != 0, src_nd);
                const double x = g ? (double)smp[k] : 0.0;
                if constexpr (METHOD == 2) {
                  call[k] = call[k] && g;
                  cacc[k] = cacc[k] + (cwy * cwx[q]) * x;
                }
                if (bil) {
                  const double bw = bwy * bwx[q];
                  bacc[k] = g ? bacc[k] + bw * x : bacc[k];
                  bws[k] = g ? bws[k] + bw : bws[k];
                  centre[k] = centre[k] || (hyr && hx[q] && g);
                }
              }
            }
          };
          if constexpr (METHOD == 2) {
#pragma unroll 1
            for (int r = 0; r < 4; ++r) row(r);
          } else {
            row(1);
            row(2);
          }
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const bool cubic = METHOD == 2 && call[k];
            ok[k] = cubic || centre[k];
            val[k] = cubic ? cacc[k] : bacc[k] / bws[k];
          }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) out[k] = ok[k] ? to_dst<D>(val[k]) : dst_nd;
      }
      // ---- the pack leaves: one store where every sample of it is written, sample by sample otherwise
      bool all = true;
#pragma unroll
      for (int k = 0; k < NB; ++k) all = all && ok[k];
      if (d.dst_layout == 0) {
        D* o = dst + ((long long)li * d.dw + lj) * d.dst_ld + d.dst_coff + b0;
        if (NB > 1 && p.vec_dst && (all || !d.keep)) {
          Pack<D, NB> q;
#pragma unroll
          for (int k = 0; k < NB; ++k) q.v[k] = out[k];
          *reinterpret_cast<Pack<D, NB>*>(o) = q;
        } else {
#pragma unroll
          for (int k = 0; k < NB; ++k)
            if (ok[k] || !d.keep) o[k] = out[k];
        }
      } else {
        const long long plane = (long long)d.dh * d.dw;
#pragma unroll
        for (int k = 0; k < NB; ++k)
          if (ok[k] || !d.keep) dst[(long long)(d.dst_coff + b0 + k) * plane + (long long)li * d.dw + lj] = out[k];
      }
    }
  }
}

// src_nodata in the source's kind; a value the kind cannot hold equals no sample
template <typename S>
bool nodata_in_kind(double v, S* out) {
  if (!(v == v)) return false;
  if constexpr (std::is_same<S, float>::value) {
    *out = (float)v;
    return (double)*out == v;
  } else {
    if (v < (double)std::numeric_limits<S>::min() || v > (double)std::numeric_limits<S>::max() || v != floor(v)) return false;
    *out = (S)v;
    return true;
  }
}

// The launch plan of a descriptor: band pack, vector paths, nodata in both kinds, grid.  `launch(nb, plan, dst nodata, has_nd, src nodata,
// grid, block)` starts the kernel; nb arrives as std::integral_constant<int, 4 / 2 / 1>.  `affine`: the average rule's tap counts
template <typename S, typename D, typename F>
void plan_and_launch(const satcv_warp_desc& d, bool affine, F&& launch) {
  const int nb = d.c % 4 == 0 ? 4 : d.c % 2 == 0 ? 2 : 1;
  WarpPlan p;
  p.ntx = affine ? (int)ceil(fabs(d.su)) + 1 : 0;
  p.nty = affine ? (int)ceil(fabs(d.sv)) + 1 : 0;
  p.vec_src = d.src_layout == 0 && d.src_ld % nb == 0 && d.src_coff % nb == 0 && (uintptr_t)d.src % (sizeof(S) * nb) == 0;
  p.vec_dst = d.dst_layout == 0 && d.dst_ld % nb == 0 && d.dst_coff % nb == 0 && (uintptr_t)d.dst % (sizeof(D) * nb) == 0;
  D nd;
  if (d.has_dst_nodata) nd = nodata_as<D>(d.dst_nodata);
  else if constexpr (std::is_same<D, float>::value) nd = NAN;
  else nd = 0;
  const long long total = (long long)d.dh * d.dw, g = (total + WP_BLOCK - 1) / WP_BLOCK;
  const dim3 grid((unsigned)(g > WP_MAX_GRID ? WP_MAX_GRID : g)), block(WP_BLOCK);
  S src_nd = 0;
  const int has_nd = d.has_src_nodata && nodata_in_kind<S>(d.src_nodata, &src_nd);
  if (nb == 4) launch(std::integral_constant<int, 4>{}, p, nd, has_nd, src_nd, grid, block);
  else if (nb == 2) launch(std::integral_constant<int, 2>{}, p, nd, has_nd, src_nd, grid, block);
  else launch(std::integral_constant<int, 1>{}, p, nd, has_nd, src_nd, grid, block);
}

// what both entry points refuse about a descriptor (the scale and method checks are the caller's)
int warp_desc_refused(const satcv_warp_desc* d, const char* who) {
  SATCV_CHECK(d && d->src && d->dst, "%s: null pointer (descriptor, src or dst)", who);
  SATCV_CHECK(kind_ok(d->src_kind) && kind_ok(d->dst_kind), "%s: unknown kind %d -> %d (0 u8, 1 u16, 2 f32, 3 i16, 5 i32)", who, d->src_kind, d->dst_kind);
  SATCV_CHECK(d->dst_kind == d->src_kind || d->dst_kind == 2, "%s: dst_kind %d is neither the source's kind %d nor f32", who, d->dst_kind, d->src_kind);
  SATCV_CHECK((d->src_layout == 0 || d->src_layout == 1) && (d->dst_layout == 0 || d->dst_layout == 1), "%s: layout %d -> %d (0 (h, w, ld), 1 (ld, h, w))", who,
              d->src_layout, d->dst_layout);
  SATCV_CHECK(d->resampling >= 0 && d->resampling <= 3, "%s: resampling %d (0 nearest, 1 bilinear, 2 cubic, 3 average)", who, d->resampling);
  SATCV_CHECK(d->sh > 0 && d->sw > 0 && d->dh > 0 && d->dw > 0 && d->c > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(d->c <= 16, "%s: c = %d bands (at most 16)", who, d->c);
  SATCV_CHECK(satcv_pixels_ok(1, d->sh, d->sw, 1) && satcv_pixels_ok(1, d->dh, d->dw, 1), "%s: raster beyond 2^31 pixels", who);
  SATCV_CHECK(d->src_ld > 0 && d->src_coff >= 0 && (long long)d->src_coff + d->c <= d->src_ld && d->dst_ld > 0 && d->dst_coff >= 0 &&
                  (long long)d->dst_coff + d->c <= d->dst_ld,
              "%s: channel range (coff + c <= ld, for src and dst)", who);
  return SATCV_OK;
}

// the second half: pointers (checked after the scales, as satcv_raster_warp always did)
int warp_pointers_refused(const satcv_warp_desc* d, const char* who) {
  const int sb = kind_bytes(d->src_kind), db = kind_bytes(d->dst_kind);
  SATCV_CHECK((uintptr_t)d->src % sb == 0 && (uintptr_t)d->dst % db == 0, "%s: misaligned pointer", who);
  const uintptr_t s0 = (uintptr_t)d->src, s1 = s0 + (uintptr_t)((long long)d->sh * d->sw * d->src_ld * sb);
  const uintptr_t d0 = (uintptr_t)d->dst, d1 = d0 + (uintptr_t)((long long)d->dh * d->dw * d->dst_ld * db);
  SATCV_CHECK(s1 <= d0 || d1 <= s0, "%s: src and dst overlap", who);
  return SATCV_OK;
}

}  // namespace
