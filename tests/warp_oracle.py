"""Float64 NumPy restatement of satcv_raster_warp (include/satcv.h, "Raster alignment"), written from the rules of the header (helper
module, no tests in it; shared by tests/test_warp_cpu.py and tests/test_warp_gpu.py).

NumPy neither fuses a multiply with an add nor reorders a sum that is written as a chain of binary operations, so every expression
below is evaluated exactly as the kernel evaluates it (which is compiled with floating-point contraction off): coordinates, weights
and the tap sums agree bit for bit, and the only differences a test has to allow are those of the division and of libm's rounding."""
import numpy as np

METHODS = ('nearest', 'bilinear', 'cubic', 'average')


def coefficients(src_transform, dst_transform):
    """(su, ou, sv, ov) from two Affine transforms (a, b, c, d, e, f)"""
    a_s, _, c_s, _, e_s, f_s = (float(v) for v in src_transform)
    a_d, _, c_d, _, e_d, f_d = (float(v) for v in dst_transform)
    return a_d / a_s, (c_d - c_s) / a_s, e_d / e_s, (f_d - f_s) / e_s


def cubic_weights(t):
    """Catmull-Rom (a = -0.5) weights of the taps x0 - 1 .. x0 + 2, from t, t * t and t * t * t as the header writes them"""
    t = np.asarray(t, np.float64)
    t2 = t * t
    t3 = t2 * t
    return [-0.5 * t3 + t2 - 0.5 * t, 1.5 * t3 - 2.5 * t2 + 1.0, -1.5 * t3 + 2.0 * t2 + 0.5 * t, 0.5 * t3 - 0.5 * t2]


def _take(src, ky, kx, origin, src_nodata):
    """samples of the window at the source-grid indices ky (H,) x kx (W,): -> float64 (H, W, c) (0 where invalid), bool valid"""
    h, w = src.shape[:2]
    ly, lx = ky - float(origin[0]), kx - float(origin[1])
    in_y, in_x = (ly >= 0) & (ly < h), (lx >= 0) & (lx < w)
    iy, ix = np.where(in_y, ly, 0).astype(np.int64), np.where(in_x, lx, 0).astype(np.int64)
    val = src[iy[:, None], ix[None, :]].astype(np.float64)
    ok = (in_y[:, None] & in_x[None, :])[..., None] & ~np.isnan(val)
    if src_nodata is not None:
        ok &= val != float(src_nodata)
    return np.where(ok, val, 0.0), ok


def _round(v64, ok, dtype, dst_nodata, keep_into):
    dtype = np.dtype(dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        if dtype.kind == 'f':
            res = v64.astype(dtype)
        else:
            info = np.iinfo(dtype)
            res = np.clip(np.rint(np.where(ok, v64, 0.0)), info.min, info.max).astype(dtype)      # rint: half to even
    if keep_into is not None:
        return np.where(ok, res, np.asarray(keep_into, dtype))
    if dst_nodata is None:
        fill = np.nan if dtype.kind == 'f' else 0
    elif dtype.kind == 'f':
        fill = dst_nodata
    else:
        fill = 0 if dst_nodata != dst_nodata else min(max(float(dst_nodata), np.iinfo(dtype).min), np.iinfo(dtype).max)
    return np.where(ok, res, np.asarray(fill).astype(dtype))


def warp_ref(src, su, ou, sv, ov, dst_shape, resampling, src_nodata=None, dst_nodata=None, dst_dtype=None, src_origin=(0, 0), dst_origin=(0, 0),
             keep_into=None):
    """src: (h, w, c) or (h, w) window of the source grid whose [0, 0] is pixel `src_origin`; -> (result of dst_dtype (None: the
    source's), float64 value before the final rounding with NaN where the result is invalid).  keep_into: the (H, W, c) destination an
    invalid result leaves untouched (keep = 1); otherwise invalid is dst_nodata, without one NaN / 0."""
    flat = src.ndim == 2
    src = src[..., None] if flat else src
    H, W = dst_shape
    gi = float(dst_origin[0]) + np.arange(H, dtype=np.float64)
    gj = float(dst_origin[1]) + np.arange(W, dtype=np.float64)
    c = src.shape[2]
    m = METHODS.index(resampling)
    with np.errstate(invalid='ignore', divide='ignore'):
        if m == 3:
            ua, ub = su * gj + ou, su * (gj + 1.0) + ou
            va, vb = sv * gi + ov, sv * (gi + 1.0) + ov
            ulo, uhi, vlo, vhi = np.minimum(ua, ub), np.maximum(ua, ub), np.minimum(va, vb), np.maximum(va, vb)
            ntx, nty = int(np.ceil(abs(su))) + 1, int(np.ceil(abs(sv))) + 1
            acc, ws = np.zeros((H, W, c)), np.zeros((H, W, c))
            for iy in range(nty):
                ky = np.floor(vlo) + iy
                wy = np.minimum(vhi, ky + 1.0) - np.maximum(vlo, ky)
                for ix in range(ntx):
                    kx = np.floor(ulo) + ix
                    wx = np.minimum(uhi, kx + 1.0) - np.maximum(ulo, kx)
                    val, ok = _take(src, ky, kx, src_origin, src_nodata)
                    w = (wy[:, None] * wx[None, :])[..., None]
                    g = ok & (wy > 0)[:, None, None] & (wx > 0)[None, :, None]
                    acc = np.where(g, acc + w * val, acc)
                    ws = np.where(g, ws + w, ws)
            ok = ws > 0
            v64 = np.where(ok, acc / ws, np.nan)
        else:
            u, v = su * (gj + 0.5) + ou, sv * (gi + 0.5) + ov
            cx, cy = np.floor(u), np.floor(v)
            if m == 0:
                val, ok = _take(src, cy, cx, src_origin, src_nodata)
                v64 = np.where(ok, (0.0 + 1.0 * val) / 1.0, np.nan)
            else:
                x0, y0 = np.floor(u - 0.5), np.floor(v - 0.5)
                t, s = u - 0.5 - x0, v - 0.5 - y0
                cwx, cwy = cubic_weights(t), cubic_weights(s)
                bwx, bwy = [0 * t, 1.0 - t, t, 0 * t], [0 * s, 1.0 - s, s, 0 * s]
                cacc, bacc, bws = np.zeros((H, W, c)), np.zeros((H, W, c)), np.zeros((H, W, c))
                call, centre = np.ones((H, W, c), bool), np.zeros((H, W, c), bool)
                taps = range(0, 4) if m == 2 else range(1, 3)
                for r in taps:
                    for q in taps:
                        ky, kx = y0 + (r - 1), x0 + (q - 1)
                        val, g = _take(src, ky, kx, src_origin, src_nodata)
                        cw = (cwy[r][:, None] * cwx[q][None, :])[..., None]
                        bw = (bwy[r][:, None] * bwx[q][None, :])[..., None]
                        call &= g
                        cacc = cacc + cw * val
                        if 1 <= r <= 2 and 1 <= q <= 2:
                            bacc = np.where(g, bacc + bw * val, bacc)
                            bws = np.where(g, bws + bw, bws)
                            centre |= g & ((ky == cy)[:, None] & (kx == cx)[None, :])[..., None]
                cubic = call if m == 2 else np.zeros_like(call)
                ok = cubic | centre
                v64 = np.where(ok, np.where(cubic, cacc, bacc / bws), np.nan)
    dtype = src.dtype if dst_dtype is None else dst_dtype
    keep = None if keep_into is None else (np.asarray(keep_into)[..., None] if flat else np.asarray(keep_into))
    res = _round(v64, ok, dtype, dst_nodata, keep)
    return (res[..., 0], v64[..., 0]) if flat else (res, v64)


def warp_between(src, src_transform, dst_transform, dst_shape, resampling, **kw):
    """`warp_ref` with the coefficients derived from two Affine transforms"""
    return warp_ref(src, *coefficients(src_transform, dst_transform), dst_shape, resampling, **kw)
