"""Float64 NumPy restatement of the projections of csrc/crs_core.hpp (include/satcv.h, "Reprojection between coordinate systems"),
written from the rules of that header's comment and independent of satellite_computervision_amd/crs.py (helper module, no tests in it;
shared by tests/test_crs_cpu.py and tests/test_reproject_gpu.py).

The series functions take the arithmetic as a namespace (`NP` below, or `mp_namespace()` for mpmath at any precision), so the same
text runs in float64 and at 40 digits.  Unlike the kernels the sums are written out term by term (sin(2 j xi) cosh(2 j eta), 24
transcendental calls), not by Clenshaw's recurrence, and Newton takes a fixed number of steps: agreement is to rounding, not bit for
bit.  `sample` is the reprojection's sampling GIVEN u and v -- the warp's rules of tests/warp_oracle.py at per-pixel coordinates."""
import numpy as np

try:
    from tests import warp_oracle as WO
except ImportError:            # (imported from a test that put tests/ itself on the path)
    import warp_oracle as WO

WGS84 = (6378137.0, 298.257223563)
GRS80 = (6378137.0, 298.257222101)
TM_SPAN = 30.0
NEWTON_STEPS = 8


def crs(code):
    """the parameters of an EPSG code, from the definitions of the codes (not from crs.py): a dict kind, a, inv_f, lon0, k0, fe, fn"""
    def utm(zone, ell, south):
        return dict(kind=1, a=ell[0], inv_f=ell[1], lon0=6.0 * zone - 183.0, k0=0.9996, fe=500000.0, fn=1e7 if south else 0.0)
    if code == 4326:
        return dict(kind=0, a=WGS84[0], inv_f=WGS84[1], lon0=0.0, k0=1.0, fe=0.0, fn=0.0)
    if code == 4269:
        return dict(kind=0, a=GRS80[0], inv_f=GRS80[1], lon0=0.0, k0=1.0, fe=0.0, fn=0.0)
    if code == 3857:
        return dict(kind=2, a=WGS84[0], inv_f=WGS84[1], lon0=0.0, k0=1.0, fe=0.0, fn=0.0)
    if 32601 <= code <= 32660:
        return utm(code - 32600, WGS84, False)
    if 32701 <= code <= 32760:
        return utm(code - 32700, WGS84, True)
    if 26901 <= code <= 26923:
        return utm(code - 26900, GRS80, False)
    raise KeyError(code)


class NP:
    """float64 NumPy arithmetic"""
    sin, cos, sinh, cosh, atanh, asinh, atan, atan2, sqrt = np.sin, np.cos, np.sinh, np.cosh, np.arctanh, np.arcsinh, np.arctan, np.arctan2, np.sqrt
    num = staticmethod(float)


def mp_namespace():
    import mpmath as mp

    class MP:
        sin, cos, sinh, cosh, atanh, asinh, atan, atan2, sqrt = mp.sin, mp.cos, mp.sinh, mp.cosh, mp.atanh, mp.asinh, mp.atan, mp.atan2, mp.sqrt
        num = staticmethod(mp.mpf)
    return MP


def tm_constants(X, a, inv_f, k0):
    """(e, 1 - e^2, k0 A, alpha[1..6], beta[1..6]) of Krueger's series to n^6"""
    N = X.num
    f = N(1) / N(inv_f)
    n = f / (2 - f)
    e2 = f * (2 - f)
    A = N(a) / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64 + n ** 6 / 256)
    q = lambda p, d: N(p) / N(d)
    alp = [n / 2 - q(2, 3) * n ** 2 + q(5, 16) * n ** 3 + q(41, 180) * n ** 4 - q(127, 288) * n ** 5 + q(7891, 37800) * n ** 6,
           q(13, 48) * n ** 2 - q(3, 5) * n ** 3 + q(557, 1440) * n ** 4 + q(281, 630) * n ** 5 - q(1983433, 1935360) * n ** 6,
           q(61, 240) * n ** 3 - q(103, 140) * n ** 4 + q(15061, 26880) * n ** 5 + q(167603, 181440) * n ** 6,
           q(49561, 161280) * n ** 4 - q(179, 168) * n ** 5 + q(6601661, 7257600) * n ** 6,
           q(34729, 80640) * n ** 5 - q(3418889, 1995840) * n ** 6,
           q(212378941, 319334400) * n ** 6]
    bet = [n / 2 - q(2, 3) * n ** 2 + q(37, 96) * n ** 3 - q(1, 360) * n ** 4 - q(81, 512) * n ** 5 + q(96199, 604800) * n ** 6,
           q(1, 48) * n ** 2 + q(1, 15) * n ** 3 - q(437, 1440) * n ** 4 + q(46, 105) * n ** 5 - q(1118711, 3870720) * n ** 6,
           q(17, 480) * n ** 3 - q(37, 840) * n ** 4 - q(209, 4480) * n ** 5 + q(5569, 90720) * n ** 6,
           q(4397, 161280) * n ** 4 - q(11, 504) * n ** 5 - q(830251, 7257600) * n ** 6,
           q(4583, 161280) * n ** 5 - q(108847, 3991680) * n ** 6,
           q(20648693, 638668800) * n ** 6]
    return X.sqrt(e2), 1 - e2, N(k0) * A, alp, bet


def tm_forward_core(X, consts, lam, phi):
    """(eta, xi) scaled by k0 A -> (x - fe, y - fn) of the transverse Mercator; lam, phi in radians"""
    e, _, ak0, alp, _ = consts
    sp = X.sin(phi)
    taup = X.sinh(X.atanh(sp) - e * X.atanh(e * sp))
    cl = X.cos(lam)
    xip = X.atan2(taup, cl)
    etap = X.asinh(X.sin(lam) / X.sqrt(taup * taup + cl * cl))
    xi, eta = xip, etap
    for j in range(1, 7):
        xi = xi + alp[j - 1] * X.sin(2 * j * xip) * X.cosh(2 * j * etap)
        eta = eta + alp[j - 1] * X.cos(2 * j * xip) * X.sinh(2 * j * etap)
    return ak0 * eta, ak0 * xi


def tm_inverse_core(X, consts, dx, dy):
    """(x - fe, y - fn) -> (lam, phi) in radians"""
    e, e2m, ak0, _, bet = consts
    xi, eta = dy / ak0, dx / ak0
    xip, etap = xi, eta
    for j in range(1, 7):
        xip = xip - bet[j - 1] * X.sin(2 * j * xi) * X.cosh(2 * j * eta)
        etap = etap - bet[j - 1] * X.cos(2 * j * xi) * X.sinh(2 * j * eta)
    sh, cx = X.sinh(etap), X.cos(xip)
    taup = X.sin(xip) / X.sqrt(sh * sh + cx * cx)
    lam = X.atan2(sh, cx)
    tau = taup / e2m
    for _ in range(NEWTON_STEPS):
        t1 = X.sqrt(1 + tau * tau)
        sig = X.sinh(e * X.atanh(e * tau / t1))
        ti = tau * X.sqrt(1 + sig * sig) - sig * t1
        tau = tau + (taup - ti) / X.sqrt(1 + ti * ti) * (1 + e2m * tau * tau) / (e2m * t1)
    return lam, X.atan(tau)


def wrap(d):
    d = np.asarray(d, np.float64)
    with np.errstate(invalid='ignore'):
        return np.where(np.abs(d) > 180.0, d - 360.0 * np.rint(d / 360.0), d)


def inverse(c, x, y):
    """coordinates of the CRS `c` (a dict of `crs`) -> (lon, lat, ok), degrees; NaN where not ok"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ok = np.isfinite(x) & np.isfinite(y)
    xs, ys = np.where(ok, x, c['fe']), np.where(ok, y, c['fn'])
    with np.errstate(all='ignore'):
        if c['kind'] == 0:
            d, lat = wrap(xs - c['lon0']), ys
        elif c['kind'] == 2:
            yy = (ys - c['fn']) / c['a']
            ok &= np.abs(yy) <= np.pi
            d, lat = wrap(np.degrees((xs - c['fe']) / c['a'])), np.degrees(np.arctan(np.sinh(yy)))
        else:
            k = tm_constants(NP, c['a'], c['inv_f'], c['k0'])
            lam, phi = tm_inverse_core(NP, k, xs - c['fe'], ys - c['fn'])
            d, lat = np.degrees(lam), np.degrees(phi)
            ok &= np.abs(d) <= TM_SPAN
        ok &= np.abs(lat) <= 90.0
    return np.where(ok, c['lon0'] + d, np.nan), np.where(ok, lat, np.nan), ok


def forward(c, lon, lat):
    """(lon, lat) in degrees -> (x, y, ok) of the CRS `c`; NaN where not ok"""
    lon, lat = np.asarray(lon, np.float64), np.asarray(lat, np.float64)
    with np.errstate(all='ignore'):
        ok = np.isfinite(lon) & np.isfinite(lat) & (np.abs(lat) <= 90.0)
        lo, la = np.where(ok, lon, c['lon0']), np.where(ok, lat, 0.0)
        d = wrap(lo - c['lon0'])
        if c['kind'] == 0:
            x, y = c['lon0'] + d, la
        elif c['kind'] == 2:
            m = np.arctanh(np.sin(np.radians(la)))
            ok &= np.abs(m) <= np.pi
            x, y = c['fe'] + c['a'] * np.radians(d), c['fn'] + c['a'] * m
        else:
            ok &= np.abs(d) <= TM_SPAN
            k = tm_constants(NP, c['a'], c['inv_f'], c['k0'])
            dx, dy = tm_forward_core(NP, k, np.radians(np.where(ok, d, 0.0)), np.radians(la))
            x, y = c['fe'] + dx, c['fn'] + dy
        ok &= np.isfinite(x) & np.isfinite(y)
    return np.where(ok, x, np.nan), np.where(ok, y, np.nan), ok


def transform(src, dst, x, y):
    """points of the CRS `src` in `dst` (dicts of `crs`): -> (x, y, ok)"""
    lon, lat, ok = inverse(src, x, y)
    xo, yo, ok2 = forward(dst, lon, lat)
    return xo, yo, ok & ok2


def grid_coords(dst, dst_transform, src, src_transform, shape, origin=(0, 0)):
    """the chain of satcv_grid_coords: (u, v, ok), each (H, W), for the window of `shape` at `origin` of the destination grid; transforms
    in Affine order, src_transform None: source CRS units"""
    a_d, _, c_d, _, e_d, f_d = dst_transform
    i = float(origin[0]) + np.arange(shape[0], dtype=np.float64)
    j = float(origin[1]) + np.arange(shape[1], dtype=np.float64)
    X, Y = np.broadcast_to((a_d * (j + 0.5) + c_d)[None, :], shape), np.broadcast_to((e_d * (i + 0.5) + f_d)[:, None], shape)
    xs, ys, ok = transform(dst, src, X, Y)
    if src_transform is None:
        return xs, ys, ok
    a_s, _, c_s, _, e_s, f_s = src_transform
    return (xs - c_s) / a_s, (ys - f_s) / e_s, ok


# ------------------------------------------------------------------------------------------------------------ sampling, given u and v
def _take_at(src, ky, kx, origin, src_nodata):
    """samples of the window `src` (h, w, c) at the per-pixel source-grid indices ky, kx (H, W): -> float64 (H, W, c) (0 where
    invalid), bool valid.  The window test is per axis, as the kernel's; the samples and their validity are warp_oracle._take's."""
    h, w, c = src.shape
    with np.errstate(invalid='ignore'):
        ly, lx = ky - float(origin[0]), kx - float(origin[1])
        inside = (ly >= 0) & (ly < h) & (lx >= 0) & (lx < w)
    lin = np.where(inside, np.where(inside, ly, 0.0) * w + np.where(inside, lx, 0.0), -1.0)
    val, ok = WO._take(src.reshape(1, h * w, c), np.zeros(1), lin.reshape(-1), (0, 0), src_nodata)
    return val.reshape(ky.shape + (c,)), ok.reshape(ky.shape + (c,))


def sample(src, u, v, resampling, src_nodata=None, dst_nodata=None, dst_dtype=None, src_origin=(0, 0), keep_into=None):
    """The rules 0 nearest / 1 bilinear / 2 cubic of satcv_raster_warp at the per-pixel source coordinates u, v (H, W; NaN: no
    coordinates, the pixel is invalid).  src (h, w, c) or (h, w), the window whose [0, 0] is source pixel `src_origin`.  -> (result of
    dst_dtype, float64 value before the final rounding with NaN where invalid), as warp_oracle.warp_ref."""
    flat = src.ndim == 2
    src = src[..., None] if flat else src
    m = WO.METHODS.index(resampling)
    assert m < 3
    shape = u.shape + (src.shape[2],)
    with np.errstate(invalid='ignore', divide='ignore'):
        cx, cy = np.floor(u), np.floor(v)
        if m == 0:
            val, ok = _take_at(src, cy, cx, src_origin, src_nodata)
            v64 = np.where(ok, val, np.nan)
        else:
            x0, y0 = np.floor(u - 0.5), np.floor(v - 0.5)
            t, s = u - 0.5 - x0, v - 0.5 - y0
            cwx, cwy = WO.cubic_weights(t), WO.cubic_weights(s)
            bwx, bwy = [0 * t, 1.0 - t, t, 0 * t], [0 * s, 1.0 - s, s, 0 * s]
            cacc, bacc, bws = np.zeros(shape), np.zeros(shape), np.zeros(shape)
            call, centre = np.ones(shape, bool), np.zeros(shape, bool)
            taps = range(0, 4) if m == 2 else range(1, 3)
            for r in taps:                                      # rows outer, columns inner
                for q in taps:
                    ky, kx = y0 + (r - 1), x0 + (q - 1)
                    val, g = _take_at(src, ky, kx, src_origin, src_nodata)
                    cw, bw = (cwy[r] * cwx[q])[..., None], (bwy[r] * bwx[q])[..., None]
                    call &= g
                    cacc = cacc + cw * val
                    if 1 <= r <= 2 and 1 <= q <= 2:
                        bacc = np.where(g, bacc + bw * val, bacc)
                        bws = np.where(g, bws + bw, bws)
                        centre |= g & ((ky == cy) & (kx == cx))[..., None]
            cubic = call if m == 2 else np.zeros_like(call)
            ok = cubic | centre
            v64 = np.where(ok, np.where(cubic, cacc, bacc / bws), np.nan)
    dtype = src.dtype if dst_dtype is None else dst_dtype
    keep = None if keep_into is None else (np.asarray(keep_into)[..., None] if flat else np.asarray(keep_into))
    res = WO._round(v64, ok, dtype, dst_nodata, keep)
    return (res[..., 0], v64[..., 0]) if flat else (res, v64)
