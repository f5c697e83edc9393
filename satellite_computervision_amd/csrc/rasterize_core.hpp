// The polygon rasterization rule (include/satcv.h, "Polygon rasterization"): the one source of the host loop and of the kernels of
// rasterize.hip, as crs_core.hpp is for the projections.  Vertices are grid pixel coordinates in float64; an edge is ordered so that
// y0 < y1 (horizontal edges are dropped before they get here).  Floating-point contraction is off: the float64 oracle of the tests
// (tests/rasterize_oracle.py) does not fuse, and the crossing column must agree with it bit for bit.
#pragma once
#include <cmath>

#pragma clang fp contract(off)

// the edge crosses the centre line of row i
__host__ __device__ inline bool edge_crosses_row(double y0, double y1, int i) {
  const double yc = (double)i + 0.5;
  return y0 <= yc && yc < y1;
}

// the column at which the fill toggles in row i: pixels j >= col lie right of the crossing.  x = x0 + (yc - y0) * (x1 - x0) / (y1 - y0),
// product first, then the quotient, then the sum, each rounded on its own; col = floor(x + 0.5) clamped to [0, W] as a double, before
// the integer conversion (a crossing far outside the grid still toggles the whole row or nothing; NaN cannot arise from finite vertices
// with y0 < y1 short of an overflow of the product, and would clamp to 0)
__host__ __device__ inline int crossing_col(double x0, double y0, double x1, double y1, int i, int W) {
  const double yc = (double)i + 0.5;
  const double x = x0 + (yc - y0) * (x1 - x0) / (y1 - y0);
  double c = floor(x + 0.5);
  if (!(c > 0.0)) c = 0.0;
  if (c > (double)W) c = (double)W;
  return (int)c;
}
