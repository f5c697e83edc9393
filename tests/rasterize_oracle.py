"""The polygon rasterization rule of include/satcv.h ("Polygon rasterization") said again in float64 NumPy, sharing no code with the
library: every edge of every ring is tested against every row, and a pixel is inside a geometry iff the number of that geometry's
crossings of its row with col <= j is odd.

    geometry   a list of rings; a ring an (n, 2) array-like of (px, py) in grid pixel coordinates, closed implicitly
    edge       endpoints ordered so that y0 < y1 (y0 == y1 dropped); crosses row i iff y0 <= i + 0.5 < y1, at
               x = x0 + ((i + 0.5) - y0) * (x1 - x0) / (y1 - y0); col = floor(x + 0.5) clamped to [0, W]
    mask       the union of the geometries; burn: the value of the last geometry in list order that covers the pixel
"""
import numpy as np


def pixels(ring, transform):
    """a ring of map coordinates in grid pixel coordinates: px = (X - c) / a, py = (Y - f) / e"""
    a, _, c, _, e, f = transform
    r = np.asarray(ring, np.float64)
    return np.stack([(r[:, 0] - c) / a, (r[:, 1] - f) / e], axis=1)


def edges(rings):
    """(E, 4) x0, y0, x1, y1 with y0 < y1 of all rings of one geometry"""
    out = []
    for ring in rings:
        r = np.asarray(ring, np.float64)
        if len(r) > 1 and (r[0] == r[-1]).all():
            r = r[:-1]
        for k in range(len(r)):
            (xa, ya), (xb, yb) = r[k], r[(k + 1) % len(r)]
            if ya == yb:
                continue
            out.append((xa, ya, xb, yb) if ya < yb else (xb, yb, xa, ya))
    return np.asarray(out, np.float64).reshape(-1, 4)


def crossings(rings, shape):
    """-> (crosses (E, H) bool, col (E, H) int64) of one geometry on a grid of `shape`"""
    H, W = shape
    e = edges(rings)
    yc = np.arange(H, dtype=np.float64)[None, :] + 0.5
    x0, y0, x1, y1 = (e[:, k][:, None] for k in range(4))
    crosses = (y0 <= yc) & (yc < y1)
    with np.errstate(all='ignore'):
        x = x0 + (yc - y0) * (x1 - x0) / (y1 - y0)
        col = np.clip(np.floor(x + 0.5), 0.0, float(W))
    return crosses, np.where(crosses, col, 0).astype(np.int64)


def inside(rings, shape):
    """(H, W) bool: the pixels of one geometry"""
    H, W = shape
    crosses, col = crossings(rings, shape)
    cnt = np.zeros((H, W + 1), np.int64)
    rows = np.broadcast_to(np.arange(H)[None, :], crosses.shape)
    np.add.at(cnt, (rows[crosses], col[crosses]), 1)
    return np.cumsum(cnt, axis=1)[:, :W] % 2 == 1


def row_counts(geoms, shape):
    """(H,) the number of crossings of every row, over all geometries"""
    return sum((crossings(g, shape)[0].sum(axis=0) for g in geoms), np.zeros(shape[0], np.int64))


def mask(geoms, shape, invert=False):
    m = np.zeros(shape, bool)
    for g in geoms:
        m |= inside(g, shape)
    return (m != bool(invert)).astype(np.uint8)


def burn(geoms, shape, values, fill=0, dtype=np.uint8, out=None):
    """the value of the last geometry in list order that covers a pixel; `fill` elsewhere, or what `out` held"""
    res = np.full(shape, fill, dtype) if out is None else out.copy()
    for g, v in zip(geoms, values):
        res[inside(g, shape)] = v
    return res


def apply_mask(arr, m, nodata, invert=False, layout='hwc'):
    """arr with nodata where the (H, W) mask is 0 (invert: is not 0)"""
    out = arr.copy()
    gone = (m != 0) == bool(invert)
    if layout == 'hwc':
        out[gone] = nodata
    else:
        out[..., gone] = nodata
    return out
