// Map projections of satcv_crs (include/satcv.h, "Reprojection between coordinate systems"): what the reference leaves to PROJ behind
// gdal.Warp, stackstac.stack(epsg=) and rasterio's transform_bounds (utils/pc_tools.py:152-186, utils/prediction_tools.py:560-600).
// One source for the host loop and for the kernels of reproject.hip: every function is __host__ __device__, float64, and compiled with
// floating-point contraction off.  tests/crs_oracle.py says the rules below again in float64 NumPy.
//
//   crs_inverse(plan, x, y)     -> (lon, lat, ok)     coordinates of the CRS -> longitude, latitude in degrees
//   crs_forward(plan, lon, lat) -> (x, y, ok)         the way back
//
// A CRS is kind 0 geographic (x = longitude, y = latitude, degrees), 1 transverse Mercator, 2 spherical (web) Mercator, with the
// ellipsoid (a, inv_f), the central meridian lon0 (degrees), the scale k0 and the false easting / northing fe, fn (metres; the origin's
// latitude is 0).  `crs_prepare` derives what does not depend on the point (e, the rectifying radius, the series coefficients) once
// per call on the host.
//
// Longitude: d = lon - lon0; when |d| > 180, d = d - 360 rint(d / 360) (half to even); a longitude inside lon0 +- 180 is used as given.
// Geographic (lon0 = 0): x = d, y = lat, both ways.
// Transverse Mercator: Krueger's series in the third flattening n = f / (2 - f), carried to n^6 (Karney 2011, "Transverse Mercator
//   with an accuracy of a few nanometers", eqs. 35 / 36 with the alpha_j / beta_j of eqs. 7-11 extended to n^6), e^2 = f (2 - f),
//   A = a / (1 + n) (1 + n^2 / 4 + n^4 / 64 + n^6 / 256).
//   forward   tau' = sinh(atanh(sin phi) - e atanh(e sin phi))                            (through the conformal latitude)
//             xi' = atan2(tau', cos lam), eta' = asinh(sin lam / sqrt(tau'^2 + cos^2 lam)), lam = d in radians
//             xi + i eta = zeta' + sum_{j=1..6} alpha_j sin(2 j zeta'), zeta' = xi' + i eta'
//             x = fe + k0 A eta, y = fn + k0 A xi
//   inverse   xi = (y - fn) / (k0 A), eta = (x - fe) / (k0 A), zeta' = zeta - sum_{j=1..6} beta_j sin(2 j zeta)
//             tau' = sin xi' / sqrt(sinh^2 eta' + cos^2 xi'), lam = atan2(sinh eta', cos xi')
//             tau from tau' by Newton steps on tau'(tau) = tau sqrt(1 + sigma^2) - sigma sqrt(1 + tau^2), sigma = sinh(e atanh(e tau /
//             sqrt(1 + tau^2))), from tau = tau' / (1 - e^2), with the step (tau' - tau'_i) / sqrt(1 + tau'_i^2) (1 + (1 - e^2) tau^2) /
//             ((1 - e^2) sqrt(1 + tau^2)), until |step| <= 1e-12 max(1, |tau|) (at most 8 steps; two or three are taken); phi = atan tau
//   The complex sums are evaluated by Clenshaw's recurrence from ONE sin / cos of 2 xi and ONE sinh / cosh of 2 eta:
//   b_k = c_k + 2 cos(2 zeta) b_{k+1} - b_{k+2}, sum = b_1 sin(2 zeta) -- a handful of transcendental calls per point, not 24.
// Spherical Mercator: x = fe + a lam, y = fn + a atanh(sin phi) on the GEOGRAPHIC latitude; back lam = (x - fe) / a,
//   phi = atan(sinh((y - fn) / a)).
// Datum: WGS84 and NAD83 coordinates are taken as the same point (no datum shift: at most 1-2 m, PROJ's "ballpark" for these pairs);
//   only the ellipsoid differs.
// Domain: the result is not ok (and NaN) when an input is not finite, |lat| > 90, for a transverse Mercator the wrapped |lon - lon0| >
//   30 degrees (the n^6 series is good to nanometres there), for the spherical Mercator |y - fn| > pi a (the square world, both ways),
//   or a result is not finite.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/satcv.h"

#pragma clang fp contract(off)

#ifndef __HIPCC__
#define __host__
#define __device__
#endif

namespace {

constexpr double CRS_PI = 3.14159265358979323846;
constexpr double CRS_RAD = CRS_PI / 180.0;     // radians per degree
constexpr double CRS_TM_SPAN = 30.0;           // degrees off the central meridian

struct crs_plan {
  int32_t kind;
  double a, lon0, fe, fn;
  double e, e2m;            // eccentricity, 1 - e^2
  double ak0;               // k0 A
  double alp[6], bet[6];
};

__host__ __device__ inline crs_plan crs_prepare(const satcv_crs& c) {
  crs_plan p;
  p.kind = c.kind; p.a = c.a; p.lon0 = c.lon0; p.fe = c.fe; p.fn = c.fn;
  const double f = 1.0 / c.inv_f, n = f / (2.0 - f), e2 = f * (2.0 - f);
  p.e = sqrt(e2);
  p.e2m = 1.0 - e2;
  const double n2 = n * n, n3 = n2 * n, n4 = n2 * n2, n5 = n4 * n, n6 = n3 * n3;
  p.ak0 = c.k0 * (c.a / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0 + n6 / 256.0));
  p.alp[0] = n / 2.0 - 2.0 * n2 / 3.0 + 5.0 * n3 / 16.0 + 41.0 * n4 / 180.0 - 127.0 * n5 / 288.0 + 7891.0 * n6 / 37800.0;
  p.alp[1] = 13.0 * n2 / 48.0 - 3.0 * n3 / 5.0 + 557.0 * n4 / 1440.0 + 281.0 * n5 / 630.0 - 1983433.0 * n6 / 1935360.0;
  p.alp[2] = 61.0 * n3 / 240.0 - 103.0 * n4 / 140.0 + 15061.0 * n5 / 26880.0 + 167603.0 * n6 / 181440.0;
  p.alp[3] = 49561.0 * n4 / 161280.0 - 179.0 * n5 / 168.0 + 6601661.0 * n6 / 7257600.0;
  p.alp[4] = 34729.0 * n5 / 80640.0 - 3418889.0 * n6 / 1995840.0;
  p.alp[5] = 212378941.0 * n6 / 319334400.0;
  p.bet[0] = n / 2.0 - 2.0 * n2 / 3.0 + 37.0 * n3 / 96.0 - n4 / 360.0 - 81.0 * n5 / 512.0 + 96199.0 * n6 / 604800.0;
  p.bet[1] = n2 / 48.0 + n3 / 15.0 - 437.0 * n4 / 1440.0 + 46.0 * n5 / 105.0 - 1118711.0 * n6 / 3870720.0;
  p.bet[2] = 17.0 * n3 / 480.0 - 37.0 * n4 / 840.0 - 209.0 * n5 / 4480.0 + 5569.0 * n6 / 90720.0;
  p.bet[3] = 4397.0 * n4 / 161280.0 - 11.0 * n5 / 504.0 - 830251.0 * n6 / 7257600.0;
  p.bet[4] = 4583.0 * n5 / 161280.0 - 108847.0 * n6 / 3991680.0;
  p.bet[5] = 20648693.0 * n6 / 638668800.0;
  return p;
}

__host__ __device__ inline bool crs_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN too

// sum_{j=1..6} c_j sin(2 j (xi + i eta)) by Clenshaw's recurrence: -> (re, im)
__host__ __device__ inline void crs_clenshaw(const double (&c)[6], double xi, double eta, double& re, double& im) {
  const double s0 = sin(2.0 * xi), c0 = cos(2.0 * xi);
  const double ex = exp(2.0 * eta), exi = 1.0 / ex;
  const double ch0 = 0.5 * (ex + exi), sh0 = 0.5 * (ex - exi);
  const double ar = 2.0 * (c0 * ch0), ai = -2.0 * (s0 * sh0);      // 2 cos(2 zeta)
  double b1r = 0.0, b1i = 0.0, b2r = 0.0, b2i = 0.0;
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    const double br = c[k] + (ar * b1r - ai * b1i) - b2r;
    const double bi = (ar * b1i + ai * b1r) - b2i;
    b2r = b1r; b2i = b1i;
    b1r = br; b1i = bi;
  }
  const double sr = s0 * ch0, si = c0 * sh0;                        // sin(2 zeta)
  re = sr * b1r - si * b1i;
  im = sr * b1i + si * b1r;
}

// d = lon - lon0 wrapped to +- 180 degrees
__host__ __device__ inline double crs_wrap(double d) {
  return fabs(d) > 180.0 ? d - 360.0 * rint(d / 360.0) : d;
}

// tau'(tau): the tangent of the conformal latitude
__host__ __device__ inline double crs_taup(double tau, double e) {
  const double t1 = sqrt(1.0 + tau * tau);
  const double sig = sinh(e * atanh(e * (tau / t1)));
  return tau * sqrt(1.0 + sig * sig) - sig * t1;
}

__host__ __device__ inline bool crs_inverse(const crs_plan& p, double x, double y, double& lon, double& lat) {
  const double nan = NAN;
  lon = nan; lat = nan;
  if (!(crs_finite(x) && crs_finite(y))) return false;
  double d, la;
  if (p.kind == 0) {
    d = crs_wrap(x - p.lon0);
    la = y;
  } else if (p.kind == 2) {
    const double yy = (y - p.fn) / p.a;
    if (fabs(yy) > CRS_PI) return false;
    d = crs_wrap((x - p.fe) / p.a / CRS_RAD);
    la = atan(sinh(yy)) / CRS_RAD;
  } else {
    const double xi = (y - p.fn) / p.ak0, eta = (x - p.fe) / p.ak0;
    double re, im;
    crs_clenshaw(p.bet, xi, eta, re, im);
    const double xip = xi - re, etap = eta - im;
    const double sh = sinh(etap), cx = cos(xip);
    const double taup = sin(xip) / sqrt(sh * sh + cx * cx);
    d = atan2(sh, cx) / CRS_RAD;
    double tau = taup / p.e2m;
    for (int it = 0; it < 8; ++it) {
      const double ti = crs_taup(tau, p.e);
      const double step = (taup - ti) / sqrt(1.0 + ti * ti) * ((1.0 + p.e2m * (tau * tau)) / (p.e2m * sqrt(1.0 + tau * tau)));
      tau = tau + step;
      if (!(fabs(step) > 1e-12 * fmax(1.0, fabs(tau)))) break;
    }
    la = atan(tau) / CRS_RAD;
    if (!(fabs(d) <= CRS_TM_SPAN)) return false;
  }
  if (!(fabs(la) <= 90.0) || !crs_finite(d)) return false;
  lon = p.lon0 + d;
  lat = la;
  return true;
}

__host__ __device__ inline bool crs_forward(const crs_plan& p, double lon, double lat, double& x, double& y) {
  const double nan = NAN;
  x = nan; y = nan;
  if (!(crs_finite(lon) && crs_finite(lat)) || fabs(lat) > 90.0) return false;
  const double d = crs_wrap(lon - p.lon0);
  double xx, yy;
  if (p.kind == 0) {
    xx = p.lon0 + d;
    yy = lat;
  } else if (p.kind == 2) {
    const double m = atanh(sin(lat * CRS_RAD));
    if (!(fabs(m) <= CRS_PI)) return false;
    xx = p.fe + p.a * (d * CRS_RAD);
    yy = p.fn + p.a * m;
  } else {
    if (fabs(d) > CRS_TM_SPAN) return false;
    const double sp = sin(lat * CRS_RAD), lam = d * CRS_RAD;
    const double taup = sinh(atanh(sp) - p.e * atanh(p.e * sp));
    const double cl = cos(lam), sl = sin(lam);
    const double xip = atan2(taup, cl), etap = asinh(sl / sqrt(taup * taup + cl * cl));
    double re, im;
    crs_clenshaw(p.alp, xip, etap, re, im);
    xx = p.fe + p.ak0 * (etap + im);
    yy = p.fn + p.ak0 * (xip + re);
  }
  if (!(crs_finite(xx) && crs_finite(yy))) return false;
  x = xx; y = yy;
  return true;
}

// a point of one CRS in another: inverse, then forward
__host__ __device__ inline bool crs_chain(const crs_plan& from, const crs_plan& to, double x, double y, double& xo, double& yo) {
  double lon, lat;
  if (!crs_inverse(from, x, y, lon, lat)) { xo = NAN; yo = NAN; return false; }
  return crs_forward(to, lon, lat, xo, yo);
}

}  // namespace
