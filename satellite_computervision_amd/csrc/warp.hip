// Raster alignment (raster_tools.warp / read_warped / read_mosaic / read_aligned_stack): a resident raster resampled onto another grid
// of the same coordinate system -- what the reference leaves to stackstac.stack(resolution=), gdal.BuildVRT, rioxarray's merge_arrays
// and reproject_match (utils/pc_tools.py:152-186, 251-282, 368-431).  The rules are those of include/satcv.h, "Raster alignment".
//   satcv_raster_warp   nearest / bilinear / cubic / average, nodata-aware.  ONE THREAD PER DESTINATION PIXEL, all its bands: the
//                       coordinates, taps and weights are computed once per pixel in float64, neighbouring lanes take neighbouring
//                       columns (their taps are neighbours too: the gather coalesces as far as the scale lets it), bands travel in
//                       packs of NB = 4 / 2 / 1 -- one load per tap and one store per pack where the layout and the address allow.
//                       One instantiation per rule: nearest is a copy without arithmetic; the cubic and the bilinear rule share one
//                       unrolled pass over the 4 x 4 taps (bilinear's are its centre), so a sample that falls back from cubic costs no
//                       second read and no lane diverges; the only data-dependent operations are the per-sample validity selects (in
//                       the source's kind).  No LDS.  Grid-stride loop over 64-bit pixel indices.
// The whole file is compiled with floating-point contraction off: u = su * (j + 0.5) + ou as a fused multiply-add moves floor(u) on
// real grids ("Aligning rasters"), and the float64 oracle of the tests does not fuse either.
#include "common.hpp"
#include "raster_kinds.hpp"

#pragma clang fp contract(off)

#include "warp_sample.hpp"      // the per-pixel part, shared with satcv_raster_reproject (reproject.hip)

namespace {

template <typename S, typename D, int NB, int METHOD>
__global__ __launch_bounds__(WP_BLOCK) void warp_kernel(const satcv_warp_desc d, const WarpPlan p, const D dst_nd, const int has_nd, const S src_nd) {
  warp_pixels<S, D, NB, METHOD>(d, p, dst_nd, has_nd, src_nd, AffineCoord{});
}

template <typename S, typename D>
void launch_warp(const satcv_warp_desc& d, hipStream_t st) {
  plan_and_launch<S, D>(d, true, [&](auto nb, const WarpPlan& p, D nd, int has_nd, S src_nd, dim3 grid, dim3 block) {
    constexpr int NB = decltype(nb)::value;
    switch (d.resampling) {
      case 0: hipLaunchKernelGGL((warp_kernel<S, D, NB, 0>), grid, block, 0, st, d, p, nd, has_nd, src_nd); break;
      case 1: hipLaunchKernelGGL((warp_kernel<S, D, NB, 1>), grid, block, 0, st, d, p, nd, has_nd, src_nd); break;
      case 2: hipLaunchKernelGGL((warp_kernel<S, D, NB, 2>), grid, block, 0, st, d, p, nd, has_nd, src_nd); break;
      default: hipLaunchKernelGGL((warp_kernel<S, D, NB, 3>), grid, block, 0, st, d, p, nd, has_nd, src_nd); break;
    }
  });
}

}  // namespace

extern "C" int satcv_raster_warp(const satcv_warp_desc* d, void* stream) {
  const char* who = "raster_warp";
  if (const int rc = warp_desc_refused(d, who)) return rc;
  SATCV_CHECK(std::isfinite(d->su) && std::isfinite(d->sv) && d->su != 0.0 && d->sv != 0.0, "%s: scale (%g, %g) must be finite and not zero", who, d->su, d->sv);
  SATCV_CHECK(std::isfinite(d->ou) && std::isfinite(d->ov), "%s: offset (%g, %g) must be finite", who, d->ou, d->ov);
  SATCV_CHECK(!(d->resampling == 3 && (fabs(d->su) > 64.0 || fabs(d->sv) > 64.0)),
              "%s: average over a footprint of %g x %g source pixels (at most 64 per axis): read an overview of the source instead", who, fabs(d->su), fabs(d->sv));
  if (const int rc = warp_pointers_refused(d, who)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  by_kind(d->src_kind, [&](auto sv) {
    using S = decltype(sv);
    if (d->dst_kind == d->src_kind) launch_warp<S, S>(*d, st);
    else launch_warp<S, float>(*d, st);
    return 0;
  });
  return launched(who);
}
