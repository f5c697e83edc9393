"""Host code of polygon rasterization, without torch (as `tiff_container` is for the container): GeoJSON-like geometries as rings, the
edge table of satcv_rasterize (include/satcv.h, "Polygon rasterization"), and the window and polygon helpers of the reference's
utils/raster_tools.py:70-331 on GeoJSON, WKT `POLYGON` strings and coordinate lists instead of shapely.  `raster_tools` imports these
names; what touches the device (`rasterize`, `geometry_mask`, `clip`) lives there.
"""
import re

import numpy as np

ITEM_ROWS = 64           # rows of one work item of the edge table (csrc/rasterize.hip)
MAX_ROW_KEYS = 4096      # crossings of one row
FIELDS = 7               # x0, y0, x1, y1, r0, r1, g


# ----------------------------------------------------------------------------------------------------------------- geometries
def _ring(coords, what):
    """one ring as a float64 (n, 2) array without its closing vertex; ValueError for fewer than three distinct vertices"""
    try:
        pts = np.asarray(coords, np.float64)                      # (positions of one length: one conversion)
        if pts.ndim != 2 or pts.shape[1] < 2:
            raise ValueError
        pts = np.ascontiguousarray(pts[:, :2])
    except (TypeError, ValueError):
        try:
            pts = np.asarray([(p[0], p[1]) for p in coords], np.float64).reshape(-1, 2)
        except (TypeError, IndexError, ValueError):
            raise ValueError(f'{what}: a ring is a list of (x, y) positions') from None
    if len(pts) > 1 and np.array_equal(pts[0], pts[-1]):
        pts = pts[:-1]
    # three distinct vertices: one that differs from the first, and one that differs from both
    other = (pts != pts[0]).any(axis=1) if len(pts) else np.zeros(0, bool)
    if not other.any() or not (other & (pts != pts[np.argmax(other)]).any(axis=1)).any():
        raise ValueError(f'{what}: a ring needs at least three distinct vertices, got {len(pts)}')
    return pts


def _polygon(coords, what):
    if not isinstance(coords, (list, tuple)) or not coords:
        raise ValueError(f'{what}: a Polygon has at least one ring')
    return [_ring(r, what) for r in coords]


def geometry_rings(geom):
    """GeoJSON-like input as a list of geometries, each a list of rings (float64 (n, 2) arrays, closing vertex dropped).  Accepted: a
    `Polygon`, a `MultiPolygon` (ONE geometry: all rings of all parts, filled even-odd), a `Feature`, a `FeatureCollection`, a
    `GeometryCollection` of those (each member its own geometry), any object with `__geo_interface__`, and a list or tuple of them.
    ValueError for every other type -- lines and points are not rasterized -- and for a ring with fewer than three distinct vertices."""
    if hasattr(geom, '__geo_interface__'):
        geom = geom.__geo_interface__
    if isinstance(geom, (list, tuple)):
        return [g for member in geom for g in geometry_rings(member)]
    if not isinstance(geom, dict) or 'type' not in geom:
        raise ValueError(f'a geometry is a GeoJSON-like mapping with a "type", an object with __geo_interface__ or a list of them, got {type(geom).__name__}')
    kind = geom['type']
    if kind == 'Polygon':
        return [_polygon(geom.get('coordinates'), 'Polygon')]
    if kind == 'MultiPolygon':
        parts = geom.get('coordinates')
        if not isinstance(parts, (list, tuple)) or not parts:
            raise ValueError('MultiPolygon: at least one part')
        return [[r for part in parts for r in _polygon(part, 'MultiPolygon')]]
    if kind == 'Feature':
        if geom.get('geometry') is None:
            raise ValueError('Feature: no geometry')
        return geometry_rings(geom['geometry'])
    if kind == 'FeatureCollection':
        return [g for f in geom.get('features', ()) for g in geometry_rings(f)]
    if kind == 'GeometryCollection':
        return [g for m in geom.get('geometries', ()) for g in geometry_rings(m)]
    raise ValueError(f'geometry of type {kind!r}: only Polygon and MultiPolygon are rasterized (lines and points are not)')


def rings_bounds(geoms):
    """(left, bottom, right, top) over every vertex of `geometry_rings` output"""
    pts = np.concatenate([r for g in geoms for r in g]) if geoms else np.empty((0, 2))
    if not len(pts):
        raise ValueError('no geometry: bounds need at least one')
    return float(pts[:, 0].min()), float(pts[:, 1].min()), float(pts[:, 0].max()), float(pts[:, 1].max())


def to_pixels(geoms, transform):
    """vertices in grid pixel coordinates: px = (X - c) / a, py = (Y - f) / e, each operation rounded on its own"""
    a, _, c, _, e, f = transform
    return [[np.stack([(r[:, 0] - c) / a, (r[:, 1] - f) / e], axis=1) for r in g] for g in geoms]


# ----------------------------------------------------------------------------------------------------------------- the edge table
def _first_row(y, H):
    """the first row i of [0, H] with i + 0.5 >= y -- decided by that comparison: the guess of ceil(y - 0.5) is corrected by it"""
    y = np.clip(y, -1.0, H + 1.0)                             # (every comparison with i + 0.5, 0 <= i < H, is unchanged)
    r = np.ceil(y - 0.5)
    r = np.where((r - 1.0) + 0.5 >= y, r - 1.0, r)
    r = np.where(r + 0.5 < y, r + 1.0, r)
    return np.clip(r, 0, H).astype(np.int64)


def edge_table(geoms_px, shape):
    """The edge table of satcv_rasterize for geometries in pixel coordinates on a grid of `shape` (H, W): -> (table, row_start).
    table: float64 (n, 7) rows {x0, y0, x1, y1, r0, r1, g} with y0 < y1 (horizontal edges dropped), [r0, r1) the rows the edge crosses
    (y0 <= i + 0.5 < y1) clipped to [0, H), at most 64 rows per entry (longer edges are split), g the geometry index.  row_start:
    int32 (H + 1), the running sum of the per-row crossing counts, from the row ranges alone (a difference array).  ValueError for a
    non-finite vertex."""
    H, W = int(shape[0]), int(shape[1])
    cols = []
    for g, rings in enumerate(geoms_px):
        for r in rings:
            r = np.asarray(r, np.float64)
            if not np.isfinite(r).all():
                raise ValueError(f'geometry {g} has a non-finite vertex (outside a projection\'s domain?)')
            a, b = r, np.roll(r, -1, axis=0)
            up = a[:, 1] <= b[:, 1]
            lo, hi = np.where(up[:, None], a, b), np.where(up[:, None], b, a)
            keep = lo[:, 1] < hi[:, 1]
            cols.append(np.column_stack([lo[keep], hi[keep], np.full(int(keep.sum()), float(g))]))
    e = np.concatenate(cols) if cols else np.empty((0, 5))
    r0 = _first_row(e[:, 1], H)
    r1 = np.maximum(_first_row(e[:, 3], H), r0)
    live = r1 > r0
    e, r0, r1 = e[live], r0[live], r1[live]
    counts = np.cumsum(np.bincount(r0, minlength=H + 1) - np.bincount(r1, minlength=H + 1))[:H]
    row_start = np.concatenate([[0], np.cumsum(counts)])
    if row_start[-1] >= 2 ** 31:
        raise ValueError(f'{int(row_start[-1])} crossings: at most 2^31 - 1')
    pieces = (r1 - r0 + ITEM_ROWS - 1) // ITEM_ROWS
    idx = np.repeat(np.arange(len(e)), pieces)
    first = np.cumsum(pieces) - pieces
    k = np.arange(len(idx)) - first[idx]
    s0 = r0[idx] + k * ITEM_ROWS
    s1 = np.minimum(s0 + ITEM_ROWS, r1[idx])
    table = np.ascontiguousarray(np.column_stack([e[idx, :4], s0.astype(np.float64), s1.astype(np.float64), e[idx, 4]]), np.float64).reshape(-1, FIELDS)
    return table, np.ascontiguousarray(row_start, np.int32)


# ----------------------------------------------------------------------------------------------------------------- the helpers of utils/raster_tools.py
def convert(size, box):
    """utils/raster_tools.py:70-96: a pixel box [x0, y0, x1, y1] of an image of `size` (height, width) as normalised YOLO
    (x centre, y centre, width, height)"""
    sx, sy = 1. / size[1], 1. / size[0]
    return ((box[0] + box[2]) / 2.0 * sx, (box[1] + box[3]) / 2.0 * sy, (box[2] - box[0]) * sx, (box[3] - box[1]) * sy)


def make_window(cx, cy, window_size):
    """:98-118: the window (x0, y0, x1, y1) of `window_size` pixels around a centroid, `round` of centre -/+ window_size // 2"""
    half = window_size // 2
    return (round(cx - half), round(cy - half), round(cx + half), round(cy + half))


def win_jitter(window_size, jitter_frac=0.1):
    """:235-249: (dx, dy), two draws of np.random.randint(-v, v) with v = rint(jitter_frac * window_size), dx first"""
    v = np.rint(jitter_frac * window_size)
    dx = np.random.randint(-v, v)
    dy = np.random.randint(-v, v)
    return dx, dy


def make_jittered_window(cx, cy, image_h, image_w, window_size=1280, jitter_frac=0.1):
    """:287-331: the window of `window_size` around (cx, cy), shifted by `win_jitter` and moved back inside the image: (x0, y0, x1, y1).
    Prints the four numbers, as the reference does."""
    jx, jy = win_jitter(window_size, jitter_frac=jitter_frac)
    x0 = int(min(max(cx - window_size / 2 + jx, 0), image_w - window_size))
    y0 = int(min(max(cy - window_size / 2 + jy, 0), image_h - window_size))
    x1, y1 = x0 + window_size, y0 + window_size
    print('x0', x0, 'y0', y0, 'x1', x1, 'y1', y1)
    return x0, y0, x1, y1


_WKT = re.compile(r'^\s*POLYGON\s*(?:Z\s*)?\(\s*(\(.*\))\s*\)\s*$', re.I | re.S)


def parse_wkt_polygon(text):
    """a WKT `POLYGON ((x y, ...), (...))` string as a list of rings, each a list of (x, y); ValueError for anything else"""
    m = _WKT.match(text)
    if not m:
        raise ValueError(f'not a WKT POLYGON: {text[:40]!r}')
    rings = []
    for body in re.findall(r'\(([^()]*)\)', m.group(1)):
        try:
            rings.append([tuple(float(v) for v in p.split()[:2]) for p in body.split(',')])
        except ValueError:
            raise ValueError(f'not a WKT POLYGON: {text[:40]!r}') from None
        if any(len(p) != 2 for p in rings[-1]):
            raise ValueError(f'not a WKT POLYGON: {text[:40]!r}')
    return rings


def format_wkt_polygon(rings):
    return 'POLYGON (' + ', '.join('(' + ', '.join(f'{float(x)!r} {float(y)!r}' for x, y in r) + ')' for r in rings) + ')'


def _polygon_rings(geom):
    """-> (rings as lists of (x, y), form): form 'wkt', 'geojson' (a Polygon mapping) or 'list' (one ring as a coordinate list)"""
    if isinstance(geom, str):
        return parse_wkt_polygon(geom), 'wkt'
    if hasattr(geom, '__geo_interface__'):
        geom = geom.__geo_interface__
    if isinstance(geom, dict):
        if geom.get('type') != 'Polygon':
            raise ValueError(f'a Polygon mapping, got type {geom.get("type")!r}')
        return [[(float(p[0]), float(p[1])) for p in r] for r in geom['coordinates']], 'geojson'
    if isinstance(geom, (list, tuple, np.ndarray)):
        return [[(float(p[0]), float(p[1])) for p in geom]], 'list'
    raise TypeError('a geometry is a WKT POLYGON string, a GeoJSON Polygon mapping or a list of (x, y)')


def convert_poly_coords(geom, affine_obj=None, inverse=False, precision=None):
    """:144-214 without shapely and rasterio: a polygon in pixel coordinates georegistered by `affine_obj`, or with inverse=True a
    georeferenced polygon in pixel coordinates.  geom: a WKT `POLYGON` string, a GeoJSON Polygon mapping or one ring as a list of
    (x, y); the result has the same form.  affine_obj: six numbers in Affine order (a, b, c, d, e, f) -- x' = a x + b y + c,
    y' = d x + e y + f -- or the nine of a rasterio transform.  precision: decimals to round to (None: no rounding)."""
    if affine_obj is None:
        raise ValueError('affine_obj must be provided (a raster_src is not read here: pass read_info(path)[0].transform)')
    t = [float(v) for v in affine_obj]
    if len(t) == 9:
        t = t[:6]
    if len(t) != 6:
        raise ValueError(f'affine_obj is six numbers (a, b, c, d, e, f), got {len(t)}')
    a, b, c, d, e, f = t
    if inverse:
        det = a * e - b * d
        if det == 0:
            raise ValueError('affine_obj is not invertible')
        ia, ib, id_, ie = e / det, -b / det, -d / det, a / det
        a, b, c, d, e, f = ia, ib, -c * ia - f * ib, id_, ie, -c * id_ - f * ie
    rings, form = _polygon_rings(geom)
    out = [[(x * a + y * b + c, x * d + y * e + f) for x, y in r] for r in rings]
    if precision is not None:
        out = [[(round(x, precision), round(y, precision)) for x, y in r] for r in out]
    if form == 'wkt':
        return format_wkt_polygon(out)
    if form == 'geojson':
        return {'type': 'Polygon', 'coordinates': [[list(p) for p in r] for r in out]}
    return out[0]


def get_centroid(geom_pix, verbose=True):
    """:251-285: (cx, cy), the area-weighted centroid of a polygon (holes subtract) rounded with np.rint.  geom_pix as for
    `convert_poly_coords`.  verbose (default True, as in the reference) prints the bounds, their extent, the area and the unrounded
    centroid.  ValueError for a polygon of zero area."""
    rings, _ = _polygon_rings(geom_pix)
    area = mx = my = 0.0
    for k, r in enumerate(rings):
        p = np.asarray(r, np.float64)
        q = np.roll(p, -1, axis=0)
        cross = p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]
        a = cross.sum() / 2.0
        sign = (1.0 if k == 0 else -1.0) * (1.0 if a >= 0 else -1.0)       # (the shell adds, a hole subtracts, whatever their winding)
        area += sign * a
        mx += sign * ((p[:, 0] + q[:, 0]) * cross).sum() / 6.0
        my += sign * ((p[:, 1] + q[:, 1]) * cross).sum() / 6.0
    if area == 0:
        raise ValueError('a polygon of zero area has no area-weighted centroid')
    cx, cy = np.rint(mx / area), np.rint(my / area)
    if verbose:
        shell = np.asarray(rings[0], np.float64)
        bounds = (shell[:, 0].min(), shell[:, 1].min(), shell[:, 0].max(), shell[:, 1].max())
        print('  bounds:', bounds)
        print('  dx, dy:', bounds[2] - bounds[0], bounds[3] - bounds[1])
        print('  area:', area)
        print('centroid:', (mx / area, my / area))
    return cx, cy
