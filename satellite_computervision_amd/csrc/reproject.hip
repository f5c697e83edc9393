// Reprojection between coordinate systems (raster_tools.reproject / pixel_coords / transform_points; read_warped(reproject=True)): what
// the reference leaves to PROJ behind gdal.Warp, stackstac.stack(epsg=) and rasterio's transform_bounds (utils/pc_tools.py:152-186,
// utils/prediction_tools.py:560-600).  The rules are those of include/satcv.h, "Reprojection between coordinate systems", and of
// crs_core.hpp (the projections); the sampling is warp_sample.hpp's, shared with satcv_raster_warp.
//   satcv_crs_transform      points of one CRS in another; on the host (the same crs_core.hpp) or one thread per point
//   satcv_grid_coords        per pixel of a window of the destination grid the source coordinates (u, v) of its centre: `rp_chain`
//   satcv_raster_reproject   warp_pixels with (u, v) from `rp_chain` -- ONE THREAD PER DESTINATION PIXEL runs the float64 chain once
//                            (inverse of the destination's projection, forward of the source's: some 20 transcendental calls for two
//                            transverse Mercators, Newton steps included), then the taps, weights and band packs of the warp.  One
//                            instantiation per rule, as there.  No LDS.
// The whole file is compiled with floating-point contraction off, as warp.hip is: the oracle of the tests does not fuse, and the two
// kernels must produce the same u and v bit for bit.
#include "common.hpp"
#include "raster_kinds.hpp"

#pragma clang fp contract(off)

#include "crs_core.hpp"
#include "warp_sample.hpp"

namespace {

// satcv_reproject_map with what `crs_prepare` derives, made once on the host
struct RpMap {
  crs_plan dst, src;
  double da, dc, de, df;
  int has_st;
  double sa, sc, se, sf;
};

// source coordinates of the centre of destination pixel (row gi, column gj), global indices: NaN where the chain is not ok
__device__ __forceinline__ void rp_chain(const RpMap& m, double gi, double gj, double& u, double& v) {
  const double X = m.da * (gj + 0.5) + m.dc, Y = m.de * (gi + 0.5) + m.df;
  double xs, ys;
  crs_chain(m.dst, m.src, X, Y, xs, ys);
  if (m.has_st) {
    u = (xs - m.sc) / m.sa;
    v = (ys - m.sf) / m.se;
  } else {
    u = xs;
    v = ys;
  }
}

struct ChainCoord {
  const RpMap& m;
  __device__ __forceinline__ void operator()(const satcv_warp_desc&, double gi, double gj, double& u, double& v) const { rp_chain(m, gi, gj, u, v); }
  __device__ __forceinline__ void footprint(const satcv_warp_desc&, double, double, double&, double&, double&, double&) const {}      // (method 3 is refused)
};

template <typename S, typename D, int NB, int METHOD>
__global__ __launch_bounds__(WP_BLOCK) void reproject_kernel(const satcv_warp_desc d, const WarpPlan p, const D dst_nd, const int has_nd, const S src_nd, const RpMap m) {
  warp_pixels<S, D, NB, METHOD>(d, p, dst_nd, has_nd, src_nd, ChainCoord{m});
}

__global__ __launch_bounds__(WP_BLOCK) void grid_coords_kernel(const RpMap m, const int dh, const int dw, const int row0, const int col0, double* __restrict__ u,
                                                               double* __restrict__ v) {
  const long long total = (long long)dh * dw;
  for (long long i = (long long)blockIdx.x * WP_BLOCK + threadIdx.x; i < total; i += (long long)gridDim.x * WP_BLOCK) {
    const int li = (int)(i / dw), lj = (int)(i - (long long)li * dw);
    const double gj = (double)((long long)col0 + lj), gi = (double)((long long)row0 + li);
    double uu, vv;
    rp_chain(m, gi, gj, uu, vv);
    u[i] = uu;
    v[i] = vv;
  }
}

__global__ __launch_bounds__(WP_BLOCK) void crs_transform_kernel(const crs_plan from, const crs_plan to, const double* x, const double* y, double* xo, double* yo,
                                                                 uint8_t* ok, const long long n) {
  for (long long i = (long long)blockIdx.x * WP_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * WP_BLOCK) {
    double a, b;
    const bool good = crs_chain(from, to, x[i], y[i], a, b);
    xo[i] = a;
    yo[i] = b;
    if (ok) ok[i] = good ? 1 : 0;
  }
}

int crs_refused(const satcv_crs* c, const char* who, const char* which) {
  SATCV_CHECK(c->kind >= 0 && c->kind <= 2, "%s: %s CRS of unknown kind %d (0 geographic, 1 transverse Mercator, 2 spherical Mercator)", who, which, c->kind);
  SATCV_CHECK(std::isfinite(c->a) && std::isfinite(c->inv_f) && std::isfinite(c->lon0) && std::isfinite(c->k0) && std::isfinite(c->fe) && std::isfinite(c->fn),
              "%s: %s CRS has a non-finite parameter", who, which);
  SATCV_CHECK(c->a > 0.0 && c->inv_f > 0.0, "%s: %s CRS needs a > 0 and inv_f > 0, got a = %g, inv_f = %g", who, which, c->a, c->inv_f);
  return SATCV_OK;
}

int map_refused(const satcv_reproject_map* m, const char* who, RpMap* out) {
  SATCV_CHECK(m, "%s: null map", who);
  if (const int rc = crs_refused(&m->dst_crs, who, "the destination")) return rc;
  if (const int rc = crs_refused(&m->src_crs, who, "the source")) return rc;
  SATCV_CHECK(std::isfinite(m->dst_a) && std::isfinite(m->dst_e) && m->dst_a != 0.0 && m->dst_e != 0.0, "%s: destination transform scale (%g, %g) must be finite and not zero",
              who, m->dst_a, m->dst_e);
  SATCV_CHECK(std::isfinite(m->dst_c) && std::isfinite(m->dst_f), "%s: destination transform origin (%g, %g) must be finite", who, m->dst_c, m->dst_f);
  if (m->has_src_transform) {
    SATCV_CHECK(std::isfinite(m->src_a) && std::isfinite(m->src_e) && m->src_a != 0.0 && m->src_e != 0.0, "%s: source transform scale (%g, %g) must be finite and not zero", who,
                m->src_a, m->src_e);
    SATCV_CHECK(std::isfinite(m->src_c) && std::isfinite(m->src_f), "%s: source transform origin (%g, %g) must be finite", who, m->src_c, m->src_f);
  }
  out->dst = crs_prepare(m->dst_crs);
  out->src = crs_prepare(m->src_crs);
  out->da = m->dst_a; out->dc = m->dst_c; out->de = m->dst_e; out->df = m->dst_f;
  out->has_st = m->has_src_transform != 0;
  out->sa = m->src_a; out->sc = m->src_c; out->se = m->src_e; out->sf = m->src_f;
  return SATCV_OK;
}

dim3 grid_for(long long total) {
  const long long g = (total + WP_BLOCK - 1) / WP_BLOCK;
  return dim3((unsigned)(g > WP_MAX_GRID ? WP_MAX_GRID : g));
}

template <typename S, typename D>
void launch_reproject(const satcv_warp_desc& d, const RpMap& m, hipStream_t st) {
  plan_and_launch<S, D>(d, false, [&](auto nb, const WarpPlan& p, D nd, int has_nd, S src_nd, dim3 grid, dim3 block) {
    constexpr int NB = decltype(nb)::value;
    switch (d.resampling) {
      case 0: hipLaunchKernelGGL((reproject_kernel<S, D, NB, 0>), grid, block, 0, st, d, p, nd, has_nd, src_nd, m); break;
      case 1: hipLaunchKernelGGL((reproject_kernel<S, D, NB, 1>), grid, block, 0, st, d, p, nd, has_nd, src_nd, m); break;
      default: hipLaunchKernelGGL((reproject_kernel<S, D, NB, 2>), grid, block, 0, st, d, p, nd, has_nd, src_nd, m); break;
    }
  });
}

}  // namespace

extern "C" int satcv_crs_transform(const satcv_crs* from, const satcv_crs* to, const double* x, const double* y, double* xo, double* yo, uint8_t* ok, int64_t n,
                                   int32_t on_device, void* stream) {
  const char* who = "crs_transform";
  SATCV_CHECK(from && to, "%s: null CRS", who);
  if (const int rc = crs_refused(from, who, "the source")) return rc;
  if (const int rc = crs_refused(to, who, "the destination")) return rc;
  SATCV_CHECK(n >= 0, "%s: n = %lld points", who, (long long)n);
  if (n == 0) return SATCV_OK;
  SATCV_CHECK(x && y && xo && yo, "%s: null pointer (x, y, xo or yo)", who);
  SATCV_CHECK(on_device == 0 || on_device == 1, "%s: on_device %d (0 host pointers, 1 device pointers)", who, on_device);
  const crs_plan pf = crs_prepare(*from), pt = crs_prepare(*to);
  if (!on_device) {
    for (int64_t i = 0; i < n; ++i) {
      double a, b;
      const bool good = crs_chain(pf, pt, x[i], y[i], a, b);
      xo[i] = a;
      yo[i] = b;
      if (ok) ok[i] = good ? 1 : 0;
    }
    return SATCV_OK;
  }
  SATCV_CHECK((uintptr_t)x % 8 == 0 && (uintptr_t)y % 8 == 0 && (uintptr_t)xo % 8 == 0 && (uintptr_t)yo % 8 == 0, "%s: misaligned pointer", who);
  hipLaunchKernelGGL(crs_transform_kernel, grid_for(n), dim3(WP_BLOCK), 0, (hipStream_t)stream, pf, pt, x, y, xo, yo, ok, (long long)n);
  return launched(who);
}

extern "C" int satcv_grid_coords(const satcv_reproject_map* m, int32_t dh, int32_t dw, int32_t row0, int32_t col0, double* u, double* v, void* stream) {
  const char* who = "grid_coords";
  RpMap rm;
  if (const int rc = map_refused(m, who, &rm)) return rc;
  SATCV_CHECK(dh > 0 && dw > 0, "%s: sizes must be positive", who);
  SATCV_CHECK(satcv_pixels_ok(1, dh, dw, 1), "%s: window beyond 2^31 pixels", who);
  SATCV_CHECK(u && v, "%s: null pointer (u or v)", who);
  SATCV_CHECK((uintptr_t)u % 8 == 0 && (uintptr_t)v % 8 == 0, "%s: misaligned pointer", who);
  hipLaunchKernelGGL(grid_coords_kernel, grid_for((long long)dh * dw), dim3(WP_BLOCK), 0, (hipStream_t)stream, rm, dh, dw, row0, col0, u, v);
  return launched(who);
}

extern "C" int satcv_raster_reproject(const satcv_warp_desc* d, const satcv_reproject_map* m, void* stream) {
  const char* who = "raster_reproject";
  if (const int rc = warp_desc_refused(d, who)) return rc;
  SATCV_CHECK(d->resampling != 3, "%s: resampling 3 (average) between two coordinate systems: the footprint of a pixel is no axis-parallel rectangle", who);
  RpMap rm;
  if (const int rc = map_refused(m, who, &rm)) return rc;
  if (const int rc = warp_pointers_refused(d, who)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  by_kind(d->src_kind, [&](auto sv) {
    using S = decltype(sv);
    if (d->dst_kind == d->src_kind) launch_reproject<S, S>(*d, rm, st);
    else launch_reproject<S, float>(*d, rm, st);
    return 0;
  });
  return launched(who);
}
