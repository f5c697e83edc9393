"""Reprojection without a GPU: the float64 oracle of tests/crs_oracle.py against published pins and against itself at 40 digits, the
host loop of satcv_crs_transform (the same csrc/crs_core.hpp the kernels run) against the oracle, the EPSG table, the host logic of
raster_tools (transform_points, transform_bounds, reproject_grid, reproject_window, auto_level, union_grid(reproject=True)),
prediction_tools.get_img_bounds, every refusal, and the C ABI (layouts, refusals before any launch).

Bounds.  Pins: the tolerance the published value allows (0.02 m for the rounded EPSG example, 1 mm elsewhere).  Oracle at 40 digits and
round trip: 1e-7 m.  Library against oracle: 1e-6 m for projected outputs, 1e-11 degrees for geographic ones -- some 150 times the
float64 rounding of the series measured at 40 digits (6.6e-9 m, 4.7e-14 degrees), and 1 / 600 000 of the finest pixel the project
handles.  `ok` is compared exactly, on points well inside and well outside every domain."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import crs_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODES = (4326, 4269, 3857, 32617, 32618, 32733, 26918)
TOL_M, TOL_DEG = 1e-6, 1e-11


def _rt():
    from satellite_computervision_amd import raster_tools as rt
    return rt


# ------------------------------------------------------------------------------------------------------------ the oracle against pins
def test_oracle_meets_the_epsg_guidance_note_example():
    """EPSG Guidance Note 7-2, Transverse Mercator: Airy 1830, lat0 49 N, lon0 2 W, k0 0.9996012717, FE 400000, FN -100000;
    50 30' N 0 30' E -> E 577274.99, N 69740.50 (parameters and result are published rounded: within 0.02 m).  satcv_crs has no
    latitude of origin: the northing of the origin on the central meridian goes into fn."""
    c = dict(kind=1, a=6377563.396, inv_f=299.32496, lon0=-2.0, k0=0.9996012717, fe=400000.0, fn=0.0)
    c['fn'] = -100000.0 - float(co.forward(c, -2.0, 49.0)[1])
    e, n, ok = co.forward(c, 0.5, 50.5)
    print(f'    E {float(e):.4f} N {float(n):.4f}')
    assert ok and abs(e - 577274.99) <= 0.02 and abs(n - 69740.50) <= 0.02
    lon, lat, ok = co.inverse(c, 577274.99, 69740.50)
    assert ok and abs(lon - 0.5) < 3e-7 and abs(lat - 50.5) < 3e-7


def test_oracle_meets_the_pole_the_origin_and_the_web_mercator_square():
    x, y, ok = co.forward(co.crs(32631), 3.0, 90.0)                       # the meridian quadrant of WGS84 is 10 001 965.7293 m
    assert ok and abs(y - 0.9996 * 10001965.7293) <= 1e-3 and abs(x - 500000.0) <= 1e-3
    for code, lon0 in ((32617, -81.0), (32733, 15.0), (26918, -75.0)):
        x, y, ok = co.forward(co.crs(code), lon0, 0.0)
        assert ok and x == 500000.0 and y == (1e7 if code == 32733 else 0.0)
    x, y, ok = co.forward(co.crs(3857), 180.0, 85.0511287798)
    assert ok and abs(x - 20037508.3428) <= 1e-3 and abs(y - 20037508.3428) <= 1e-3


def _chain_points(n=400, seed=3):
    """points of zone 17 N around its eastern edge, the ground the 17 N -> 18 N chain covers"""
    rng = np.random.default_rng(seed)
    lon, lat = rng.uniform(-84.0, -72.0, n), rng.uniform(-5.0, 72.0, n)
    x, y, ok = co.forward(co.crs(32617), lon, lat)
    assert ok.all()
    return x, y


def test_oracle_equals_itself_at_40_digits():
    import mpmath as mp
    x, y = _chain_points()
    s, d = co.crs(32617), co.crs(32618)
    xo, yo, ok = co.transform(s, d, x, y)
    lon, lat, _ = co.inverse(s, x, y)
    assert ok.all()
    with mp.workdps(40):
        X = co.mp_namespace()
        ks, kd = co.tm_constants(X, s['a'], s['inv_f'], s['k0']), co.tm_constants(X, d['a'], d['inv_f'], d['k0'])
        deg = mp.pi / 180
        err_m = err_deg = 0.0
        for k in range(x.size):
            lam, phi = co.tm_inverse_core(X, ks, mp.mpf(float(x[k])) - mp.mpf(s['fe']), mp.mpf(float(y[k])) - mp.mpf(s['fn']))
            lo = mp.mpf(s['lon0']) + lam / deg
            err_deg = max(err_deg, float(abs(lo - mp.mpf(float(lon[k])))), float(abs(phi / deg - mp.mpf(float(lat[k])))))
            dx, dy = co.tm_forward_core(X, kd, (lo - mp.mpf(d['lon0'])) * deg, phi)
            err_m = max(err_m, float(mp.sqrt((dx + mp.mpf(d['fe']) - mp.mpf(float(xo[k]))) ** 2 + (dy + mp.mpf(d['fn']) - mp.mpf(float(yo[k]))) ** 2)))
    print(f'    float64 against 40 digits: {err_m:.3e} m, {err_deg:.3e} degrees')
    assert err_m <= 1e-7 and err_deg <= 1e-12


def test_oracle_round_trip_exposes_truncation_and_coefficients():
    """alpha and beta are independent series: forward o inverse within 1e-7 m for |dlon| <= 30 degrees, latitudes -80 ... 84"""
    rng = np.random.default_rng(4)
    worst = 0.0
    for code in (32617, 32733, 26918):
        c = co.crs(code)
        lon, lat = c['lon0'] + rng.uniform(-30.0, 30.0, 4000), rng.uniform(-80.0, 84.0, 4000)
        x, y, ok = co.forward(c, lon, lat)
        lo, la, ok2 = co.inverse(c, x, y)
        x2, y2, ok3 = co.forward(c, lo, la)
        assert ok.all() and ok2.all() and ok3.all()
        worst = max(worst, float(np.hypot(x2 - x, y2 - y).max()))
    print(f'    round trip: {worst:.3e} m')
    assert worst <= 1e-7


# ------------------------------------------------------------------------------------------------------------ the library against the oracle
def _points_in(code, n, rng):
    """n points of the CRS `code` well inside its domain, both hemispheres and the neighbouring zones included"""
    c = co.crs(code)
    if c['kind'] == 1:
        lon, lat = c['lon0'] + rng.uniform(-12.0, 12.0, n), rng.uniform(-79.0, 83.0, n)
    else:
        lon, lat = rng.uniform(-179.0, 179.0, n), rng.uniform(-84.0, 84.0, n)
    x, y, ok = co.forward(c, lon, lat)
    assert ok.all()
    return x, y


def test_host_transform_equals_the_oracle_for_every_pair():
    rt = _rt()
    rng = np.random.default_rng(5)
    worst_m = worst_deg = 0.0
    for s in CODES:
        x, y = _points_in(s, 3000, rng)
        for d in CODES:
            xo, yo, ok = co.transform(co.crs(s), co.crs(d), x, y)
            gx, gy = rt.transform_points(x, y, s, d)
            assert np.array_equal(~np.isnan(gx), ok) and np.array_equal(np.isnan(gx), np.isnan(gy)), (s, d)
            if not ok.any():                                        # zone 33 and the American zones lie 90 degrees apart: exactly nothing is ok
                assert 32733 in (s, d) and {s, d} & {32617, 32618, 26918}, (s, d)
                continue
            assert ok.sum() > 300, (s, d)
            err = float(np.max(np.maximum(np.abs(gx - xo), np.abs(gy - yo))[ok]))
            if co.crs(d)['kind'] == 0:
                worst_deg = max(worst_deg, err)
                assert err <= TOL_DEG, (s, d, err)
            else:
                worst_m = max(worst_m, err)
                assert err <= TOL_M, (s, d, err)
    print(f'    library against oracle: {worst_m:.3e} m, {worst_deg:.3e} degrees')


def test_ok_is_exact_inside_and_outside_every_domain():
    from satellite_computervision_amd import _lib
    from satellite_computervision_amd.crs import crs_struct
    nan, inf = float('nan'), float('inf')
    cases = [  # (from, to, x, y, ok)
        (4326, 32618, -75.0, 40.0, 1), (4326, 32618, -50.0, 40.0, 1), (4326, 32618, -40.0, 40.0, 0), (4326, 32618, 120.0, 0.0, 0),
        (4326, 32618, -75.0, 95.0, 0), (4326, 32618, -75.0, -91.0, 0), (4326, 32618, nan, 0.0, 0), (4326, 32618, 0.0, inf, 0),
        (4326, 32618, 285.0, 40.0, 1), (4326, 32618, -435.0, 40.0, 1), (4326, 3857, 10.0, 80.0, 1), (4326, 3857, 10.0, 89.0, 0),
        (4326, 3857, 10.0, -89.9, 0), (3857, 4326, 1e6, 1.9e7, 1), (3857, 4326, 1e6, 2.2e7, 0), (3857, 4326, 1e6, -2.5e7, 0),
        (32618, 4326, 500000.0, 4.4e6, 1), (32618, 4326, 500000.0 + 5.0e6, 4.4e6, 0), (32618, 4326, -3.5e6, 4.4e6, 0), (32618, 4326, 500000.0, 1.2e7, 0),
        (32618, 4326, 500000.0, -inf, 0), (32733, 32633, 500000.0, 9.9e6, 1), (32617, 32618, 800000.0, 4.4e6, 1), (32601, 32660, 400000.0, 1e6, 1),
        (4326, 4269, 181.0, 10.0, 1), (4269, 4326, 10.0, 90.0, 1), (4269, 4326, 10.0, 90.5, 0)]
    for s, d, x, y, want in cases:
        xs, ys, xo, yo = (np.array([v]) for v in (x, y, 0.0, 0.0))
        ok = np.array([7], np.uint8)
        a, b = crs_struct(s), crs_struct(d)
        assert _lib.lib.satcv_crs_transform(ctypes.byref(a), ctypes.byref(b), xs.ctypes.data, ys.ctypes.data, xo.ctypes.data, yo.ctypes.data, ok.ctypes.data, 1, 0, None) == 0
        assert ok[0] == want and (np.isnan(xo[0]) and np.isnan(yo[0])) == (want == 0), (s, d, x, y)
        assert bool(co.transform(co.crs(s), co.crs(d), x, y)[2]) == bool(want), (s, d, x, y)
    # wrapped longitudes land on the same point; in place is allowed
    rt = _rt()
    a, b = rt.transform_points([285.0, -435.0], [40.0, 40.0], 4326, 32618), rt.transform_points([-75.0], [40.0], 4326, 32618)
    assert a[0][0] == a[0][1] == b[0][0] == 500000.0 and a[1][0] == b[1][0]
    assert rt.transform_points([181.0], [10.0], 4326, 4269)[0][0] == -179.0


# ------------------------------------------------------------------------------------------------------------ the EPSG table
def test_crs_params_knows_exactly_the_supported_families():
    from satellite_computervision_amd.crs import crs_params
    for code in (4326, 4269, 3857, 32601, 32617, 32660, 32701, 32733, 32760, 26901, 26918, 26923):
        got, want = crs_params(code), co.crs(code)
        assert got == want and crs_params(f'EPSG:{code}') == want, code
    assert crs_params(32617)['lon0'] == -81.0 and crs_params(32733)['fn'] == 1e7 and crs_params(26918)['inv_f'] == 298.257222101
    assert crs_params(4326)['kind'] == 0 and crs_params(32601)['kind'] == 1 and crs_params(3857)['kind'] == 2
    for code in (32600, 32661, 32700, 32761, 26900, 26924, 3395, 2154, 27700, 4258, 5070):
        with pytest.raises(ValueError, match='32601-32660'):
            crs_params(code)
    with pytest.raises(ValueError, match='WKT'):
        crs_params('PROJCS["x"]')


# ------------------------------------------------------------------------------------------------------------ host logic
TILE = (10.0, 0.0, 600000.0, 0.0, -10.0, 4500000.0)             # a 109.8 km tile at the eastern edge of zone 17 N
TILE_SHAPE = (10980, 10980)


def test_transform_bounds_densifies_the_edges():
    rt = _rt()
    left, bottom, right, top = 445000.0, 4400000.0, 555000.0, 4500000.0       # astride the central meridian: the top edge bulges north between its corners
    box = rt.transform_bounds(32617, 4326, left, bottom, right, top)
    cx, cy = rt.transform_points([left, right, right, left], [bottom, bottom, top, top], 32617, 4326)
    assert box[0] <= cx.min() and box[2] >= cx.max() and box[1] <= cy.min() and box[3] >= cy.max()
    assert box[3] > cy.max() + 1e-5 and box[0] == cx.min()
    assert rt.transform_bounds(32617, 4326, left, bottom, right, top, densify_pts=0) == (cx.min(), cy.min(), cx.max(), cy.max())
    assert rt.transform_bounds(32617, 32617, left, bottom, right, top) == pytest.approx((left, bottom, right, top), abs=1e-6)
    with pytest.raises(ValueError, match='densify_pts'):
        rt.transform_bounds(32617, 4326, left, bottom, right, top, densify_pts=-1)
    with pytest.raises(ValueError, match='domain'):
        rt.transform_bounds(4326, 32617, 60.0, 0.0, 61.0, 1.0)
    # a box of which a part lies outside the domain: the part inside decides
    part = rt.transform_bounds(4326, 3857, -10.0, 80.0, 10.0, 90.0)
    assert part[3] < 20037508.35 and part[1] == pytest.approx(co.forward(co.crs(3857), 0.0, 80.0)[1], abs=1e-6)


def test_reproject_grid_keeps_the_diagonal_pixel_count_and_snaps_outward():
    rt = _rt()
    src = rt.Grid(TILE, TILE_SHAPE, 32617)
    g = rt.reproject_grid(src, 32618)
    b = rt.transform_bounds(32617, 32618, *src.bounds)
    res = np.hypot(b[2] - b[0], b[3] - b[1]) / np.hypot(*TILE_SHAPE)
    assert g.crs == 'EPSG:32618' and g.resolution == (res, res) and g.transform[4] < 0
    gb = g.bounds
    assert gb[0] <= b[0] < gb[0] + res and gb[1] <= b[1] < gb[1] + res and gb[2] - res < b[2] <= gb[2] + 1e-6 and gb[3] - res < b[3] <= gb[3] + 1e-6
    assert abs(gb[0] / res - round(gb[0] / res)) < 1e-6
    g10 = rt.reproject_grid(src, 'EPSG:32618', resolution=10)
    assert g10.resolution == (10.0, 10.0) and all(v % 10 == 0 for v in g10.bounds)
    assert g10.bounds[0] <= b[0] and g10.bounds[3] >= b[3] and g10.shape == (round((g10.bounds[3] - g10.bounds[1]) / 10), round((g10.bounds[2] - g10.bounds[0]) / 10))
    given = rt.reproject_grid(src, 4326, resolution=1 / 8192, bounds=(-80.0, 40.0, -79.5, 40.25))
    assert given.shape == (2048, 4096) and given.transform == (1 / 8192, 0.0, -80.0, 0.0, -1 / 8192, 40.25)
    with pytest.raises(ValueError, match='no EPSG code'):
        rt.reproject_grid(rt.Grid(TILE, TILE_SHAPE), 32618)
    with pytest.raises(ValueError, match='32601-32660'):
        rt.reproject_grid(src, 2154)


def test_reproject_window_hand_worked():
    rt = _rt()
    # a geographic source of 1/64-degree pixels, south-up from (lon -76, lat 39); the destination is 4269 on the very same numbers (the
    # two geographic systems are taken as one), so the chain is the identity and the window is the warp's and one pixel more.  Dyadic
    # numbers: every coordinate is exact
    src_t, src_shape = (1 / 64, 0.0, -76.0, 0.0, 1 / 64, 39.0), (400, 600)
    grid = rt.Grid((1 / 32, 0.0, -75.0, 0.0, 1 / 32, 40.0), (50, 40), 4269)     # u = 2 (j + 0.5) + 64: 65 ... 143, v = 2 (i + 0.5) + 64: 65 ... 163
    for method, m in (('nearest', 0), ('bilinear', 1), ('cubic', 2)):
        lo, hi_u, hi_v = 65 - m - 1, 143 + m + 1, 163 + m + 1
        assert rt.reproject_window(src_t, src_shape, 4326, grid, method) == (lo, lo, hi_v - lo + 1, hi_u - lo + 1), method
        same = rt.warp_window(src_t, src_shape, grid, method)
        assert same == (lo + 1, lo + 1, hi_v - lo - 1, hi_u - lo - 1)
    assert rt.reproject_window(src_t, (100, 100), 4326, grid, 'nearest') == (64, 64, 36, 36)            # clipped to the raster
    assert rt.reproject_window(src_t, (60, 600), 4326, grid, 'nearest') is None                         # the grid lies below the raster
    assert rt.reproject_window(src_t, src_shape, 4326, rt.Grid((1 / 32, 0, -60.0, 0, 1 / 32, 40.0), (5, 5), 4269), 'cubic') is None      # beside it
    # a UTM grid on a UTM source of the neighbouring zone: the window holds the source pixel of every grid pixel (checked through the oracle)
    tile = rt.Grid(TILE, TILE_SHAPE, 32617)
    dst = rt.Grid((10.0, 0.0, 100000.0, 0.0, -10.0, 4480000.0), (300, 500), 32618)
    y0, x0, h, w = rt.reproject_window(TILE, TILE_SHAPE, 32617, dst, 'nearest')
    u, v, ok = co.grid_coords(co.crs(32618), dst.transform, co.crs(32617), TILE, dst.shape)
    assert ok.all() and y0 <= np.floor(v.min()) and x0 <= np.floor(u.min()) and y0 + h > np.floor(v.max()) and x0 + w > np.floor(u.max())
    assert h < 600 and w < 800 and (y0, x0) != (0, 0)
    # a grid that reaches beyond a domain keeps the whole source; one that lies outside it altogether reads nothing
    world = rt.Grid((40000.0, 0, -2.0e7, 0, -40000.0, 2.4e7), (1200, 1000), 3857)
    assert rt.reproject_window((1.0, 0, -180.0, 0, -1.0, 90.0), (180, 360), 4326, world, 'nearest') == (0, 0, 180, 360)
    beyond = rt.Grid((1000.0, 0, 0.0, 0, -1000.0, 2.6e7), (10, 10), 3857)
    assert rt.reproject_window((1.0, 0, -180.0, 0, -1.0, 90.0), (180, 360), 4326, beyond, 'nearest') is None
    assert tile.crs == 'EPSG:32617'


def test_measured_pixel_size_auto_level_and_union_grid_across_two_codes(tmp_path):
    rt = _rt()
    tile = rt.Grid(TILE, TILE_SHAPE, 32617)
    # 10 m pixels of zone 17 at its eastern edge, measured in zone 18: the ratio of the two scale factors, and the same on both axes
    ll = rt.transform_points([650000.0], [4450000.0], 32617, 4326)
    centre = rt.transform_points(ll[0], ll[1], 4326, 32618)
    px, py = rt.measured_pixel_size(TILE, 32617, 32618, (centre[0][0], centre[1][0]))
    assert 10.0 < px < 10.02 and abs(px - py) < 1e-4
    dpx = rt.measured_pixel_size((10.0, 0, 0, 0, -10.0, 0), 32618, 4326, (-75.0, 0.0))
    assert dpx[0] == pytest.approx(10.0 / (0.9996 * 6378137.0 * np.pi / 180), rel=1e-6) and dpx[1] == pytest.approx(10.0 / (0.9996 * 110574.3886), rel=1e-5)
    levels = [(10.0, 0, 600000.0, 0, -10.0, 4500000.0), (20.0, 0, 600000.0, 0, -20.0, 4500000.0), (40.0, 0, 600000.0, 0, -40.0, 4500000.0)]
    at = lambda res: rt.Grid((res, 0, centre[0][0] - 50 * res, 0, -res, centre[1][0] + 50 * res), (100, 100), 32618)
    assert rt.auto_level(levels, at(20.0)) == 1                                   # as before: the numbers alone
    assert rt.auto_level(levels, at(20.0), 'EPSG:32617') == 0                     # 20 m of zone 17 are 20.03 m here: too coarse
    assert rt.auto_level(levels, at(20.1), 'EPSG:32617') == 1 and rt.auto_level(levels, at(45.0), 'EPSG:32617') == 2
    assert rt.auto_level(levels, at(20.0), 'EPSG:32618') == 1
    # union_grid
    east = rt.Grid((10.0, 0.0, 300000.0, 0.0, -10.0, 4480000.0), (300, 500), 32618)
    with pytest.raises(ValueError, match='reprojection between coordinate systems is not done'):
        rt.union_grid([tile, east])
    u = rt.union_grid([tile, east], reproject=True)
    b = rt.transform_bounds(32618, 32617, *east.bounds)
    assert u.crs == 'EPSG:32617' and u.resolution == (10.0, 10.0)
    assert u.bounds[0] == tile.bounds[0] and u.bounds[2] >= b[2] and u.bounds[2] - 10 < b[2] and u.bounds[1] <= min(b[1], tile.bounds[1])
    u18 = rt.union_grid([tile, east], crs=32618, reproject=True)
    assert u18.crs == 'EPSG:32618' and u18.resolution == (10.0, 10.0) and u18.bounds[2] == east.bounds[2]
    assert u18.bounds[0] <= rt.transform_bounds(32617, 32618, *tile.bounds)[0]
    only = rt.union_grid([tile], crs=32618, reproject=True)                       # the finest source is the foreign one: its measured size
    assert 10.0 < only.resolution[0] < 10.03
    assert rt.union_grid([tile, tile], reproject=True) == rt.union_grid([tile, tile])
    with pytest.raises(ValueError, match='32601-32660'):
        rt.union_grid([tile, rt.Grid(TILE, (4, 4), 2154)], reproject=True)


def test_get_img_bounds(tmp_path):
    from satellite_computervision_amd import prediction_tools as pt
    rt = _rt()
    mixer = {'projection': {'crs': 'EPSG:32618', 'affine': {'doubleMatrix': [10.0, 0.0, 500000.0, 0.0, -10.0, 4400000.0]}}, 'patchDimensions': [256, 256]}
    jf = tmp_path / 'mixer.json'
    jf.write_text(json.dumps(mixer))
    img = np.zeros((200, 300), np.float32)
    assert pt.get_img_bounds(img, str(jf)) == [[4398000.0, 500000.0], [4400000.0, 503000.0]]
    (s, w), (n, e) = pt.get_img_bounds(img, str(jf), 'EPSG:4326')
    want = rt.transform_bounds(32618, 4326, 500000.0, 4398000.0, 503000.0, 4400000.0, densify_pts=21)
    assert (w, s, e, n) == want and w == -75.0 and 39.7 < s < n < 39.8 and -75.0 < e < -74.96
    (s3, w3), (n3, e3) = pt.get_img_bounds(img, str(jf), dst_crs='EPSG:3857')
    assert w3 == pytest.approx(-75.0 * np.pi / 180 * 6378137.0) and s3 < n3
    tif = rt.write_tiles(str(tmp_path / 'a.tif'), [(16, 16)], [[bytes(range(256))]], 'uint8', 1, 16, None, False, 255, (20.0, 0, 500000.0, 0, -20.0, 4400000.0), 32618)
    assert pt.get_img_bounds(tif, str(jf)) == [[4399680.0, 500000.0], [4400000.0, 500320.0]]
    with pytest.raises(ValueError, match='array'):
        pt.get_img_bounds(np.zeros((2, 3, 4)), str(jf))


def _tiny_file(path, transform, crs):
    return _rt().write_tiles(str(path), [(16, 16)], [[bytes(range(256))]], 'uint8', 1, 16, None, False, 255, transform, crs)


def test_new_value_errors_and_unchanged_refusals(tmp_path):
    rt = _rt()
    north = (10, 0, 500000, 0, -10, 4400160)
    a, b = _tiny_file(tmp_path / 'a.tif', north, 32617), _tiny_file(tmp_path / 'b.tif', north, 32618)
    odd = _tiny_file(tmp_path / 'odd.tif', north, 2154)
    g = rt.Grid(north, (16, 16), 32617)
    # with reproject left at its default every refusal stands, with its message
    for call in (lambda: rt.union_grid([a, b]), lambda: rt.union_grid([a], crs=4326), lambda: rt.read_warped(b, g), lambda: rt.read_mosaic([a, b]),
                 lambda: rt.read_aligned_stack([a, b]), lambda: rt.read_mosaic([a], grid=rt.Grid(north, (16, 16), 32618)),
                 lambda: rt.read_warped(b, g, reproject=False), lambda: rt.union_grid([a, b], reproject=False)):
        with pytest.raises(ValueError, match='reprojection between coordinate systems is not done'):
            call()
    from satellite_computervision_amd import pc_tools as pc, prediction_tools as pt
    with pytest.raises(ValueError, match='reprojection between coordinate systems is not done'):
        pc.predict_change_files([a], [b], None)
    # the new ones
    for call in (lambda: rt.read_warped(odd, g, reproject=True), lambda: rt.read_mosaic([a, odd], reproject=True), lambda: rt.union_grid([a, odd], reproject=True),
                 lambda: rt.read_aligned_stack([a, odd], reproject=True), lambda: rt.transform_points([0.0], [0.0], 4326, 2154),
                 lambda: rt.pixel_coords(g, crs=27700), lambda: pc.predict_change_files([a], [odd], None, reproject=True)):
        with pytest.raises(ValueError, match='32601-32660'):
            call()
    for call in (lambda: rt.read_warped(b, g, resampling='average', reproject=True), lambda: rt.reproject_window(north, (16, 16), 32618, g, 'average'),
                 lambda: rt.reproject(None, north, 32618, g, 'average')):
        with pytest.raises(ValueError, match="level='auto'"):
            call()
    with pytest.raises(ValueError, match='resampling must be one of'):
        rt.reproject_window(north, (16, 16), 32618, g, 'lanczos')
    with pytest.raises(ValueError, match='Grid'):
        rt.reproject(None, north, 32618, north)
    with pytest.raises(ValueError, match='Grid'):
        rt.pixel_coords(north)
    with pytest.raises(ValueError, match='EPSG codes'):
        rt.pixel_coords(rt.Grid(north, (4, 4)), crs=4326)
    with pytest.raises(ValueError, match='rotated or sheared'):
        rt.reproject_window((10, 1, 0, 0, -10, 0), (16, 16), 32618, g)
    with pytest.raises(ValueError, match='differ in shape'):
        rt.transform_points([0.0, 1.0], [0.0], 4326, 3857)
    with pytest.raises(ValueError, match='CUDA float64'):
        rt.transform_points(np.zeros(3), np.zeros(3), 4326, 3857, device=True)
    with pytest.raises(ValueError, match='CUDA tensor'):
        rt.reproject(np.zeros((4, 4), np.uint8), north, 32618, g)


def test_the_order_of_refusals_where_two_coincide(tmp_path):
    """`reproject` refuses the method before it names a code it cannot reproject; `read_warped(reproject=True)` names the code first,
    then the method, then the level; with one CRS the level comes before the method"""
    rt = _rt()
    north = (10, 0, 500000, 0, -10, 4400160)
    a, b = _tiny_file(tmp_path / 'a.tif', north, 32617), _tiny_file(tmp_path / 'b.tif', north, 32618)
    odd = _tiny_file(tmp_path / 'odd.tif', north, 2154)
    g = rt.Grid(north, (16, 16), 32617)
    for method, what in (('lanczos', 'resampling must be one of'), ('average', "level='auto'"), ('nearest', '32601-32660')):
        with pytest.raises(ValueError, match=what):
            rt.reproject(None, north, 2154, g, method)
    for path, method, what in ((odd, 'lanczos', '32601-32660'), (b, 'lanczos', 'resampling must be one of'), (b, 'average', "level='auto'"),
                               (b, 'nearest', 'the file has levels'), (a, 'lanczos', 'the file has levels')):
        with pytest.raises(ValueError, match=what):
            rt.read_warped(path, g, resampling=method, level=7, reproject=True)
    # with one CRS a transform that cannot be resampled is refused before the method
    for call in (lambda: rt.warp(None, (10, 1, 0, 0, -10, 0), g, 'lanczos'), lambda: rt.warp_window((10, 1, 0, 0, -10, 0), (16, 16), g, 'lanczos'),
                 lambda: rt.reproject(None, (10, 1, 0, 0, -10, 0), 32617, g, 'lanczos')):
        with pytest.raises(ValueError, match='rotated or sheared'):
            call()


# ------------------------------------------------------------------------------------------------------------ C ABI
def _fields(hdr, name):
    m = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S)
    out = []
    for decl in m.group(1).replace('\n', ' ').split(';'):
        decl = decl.strip()
        if decl:
            out += re.sub(r'^(const\s+)?\w+\*?\s+', '', decl).replace(' ', '').split(',')
    return out


def test_descriptors_mirror_the_header(tmp_path):
    from satellite_computervision_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    assert 'Reprojection between coordinate systems' in hdr
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {']
    for name, D in (('satcv_crs', _lib.Crs), ('satcv_reproject_map', _lib.ReprojectMap)):
        assert _fields(hdr, name) == [f[0] for f in D._fields_]
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in D._fields_]
    lines += ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.splitlines())
    for name, D in (('satcv_crs', _lib.Crs), ('satcv_reproject_map', _lib.ReprojectMap)):
        assert int(got[name]) == ctypes.sizeof(D)
        for f, _ in D._fields_:
            assert int(got[f'{name}.{f}']) == getattr(D, f).offset, (name, f)
    for sym in ('satcv_crs_transform', 'satcv_grid_coords', 'satcv_raster_reproject'):
        assert sym in _lib.EXPORTED_SYMBOLS and re.search(r'\bint %s\(' % sym, hdr)


def test_reproject_is_built_and_compiled_without_contraction():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_satcv_build_r', os.path.join(ROOT, 'satellite_computervision_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'reproject.hip' in b.SOURCES and 'warp.hip' in b.SOURCES
    text = open(os.path.join(b.CSRC, 'reproject.hip')).read()
    assert text.index('#pragma clang fp contract(off)') < text.index('#include "crs_core.hpp"') < text.index('#include "warp_sample.hpp"')
    assert '#pragma clang fp contract(off)' in open(os.path.join(b.CSRC, 'crs_core.hpp')).read()
    warp = open(os.path.join(b.CSRC, 'warp.hip')).read()
    assert warp.index('#pragma clang fp contract(off)') < warp.index('#include "warp_sample.hpp"')       # the shared sampling is compiled under the pragma in both


def test_refusals_of_the_c_abi():
    """refused on the host, with a message that names the entry point, before any launch (this test runs without a GPU)"""
    from satellite_computervision_amd import _lib
    from satellite_computervision_amd.crs import crs_struct
    lib, D, M, Crs = _lib.lib, _lib.WarpDesc, _lib.ReprojectMap, _lib.Crs
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 2048
    inf, nan = float('inf'), float('nan')

    def desc(**kw):
        return D(**dict(dict(src=p, src_kind=1, src_layout=0, sh=4, sw=4, src_ld=2, src_coff=0, src_row0=0, src_col0=0, dst=q, dst_kind=1, dst_layout=0,
                             dh=4, dw=4, dst_ld=2, dst_coff=0, dst_row0=0, dst_col0=0, c=2, su=0.0, ou=nan, sv=inf, ov=0.0, resampling=0, has_src_nodata=0,
                             src_nodata=0.0, has_dst_nodata=0, dst_nodata=0.0, keep=0), **kw))

    def crs(code=32618, **kw):
        c = crs_struct(code)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def rmap(**kw):
        return M(**dict(dict(dst_crs=crs(), dst_a=10.0, dst_c=5e5, dst_e=-10.0, dst_f=4.4e6, src_crs=crs(32617), has_src_transform=1, src_a=10.0, src_c=7e5, src_e=-10.0,
                             src_f=4.4e6), **kw))
    good = rmap()
    assert lib.satcv_raster_reproject(None, ctypes.byref(good), None) == -1 and b'raster_reproject' in lib.satcv_last_error()
    # what satcv_raster_warp refuses, except the scale checks (the descriptor above carries su = 0, ou = NaN, sv = inf: ignored)
    for d, word in ((desc(src=None), 'null'), (desc(dst=None), 'null'), (desc(src=p + 1), 'misaligned'), (desc(dst=q + 1), 'misaligned'),
                    (desc(src_kind=4), 'unknown kind'), (desc(dst_kind=3), 'neither'), (desc(src_layout=2), 'layout'), (desc(resampling=4), 'resampling'),
                    (desc(resampling=-1), 'resampling'), (desc(c=17, src_ld=17, dst_ld=17), 'at most 16'), (desc(c=3), 'channel range'),
                    (desc(dst_coff=-1), 'channel range'), (desc(sh=0), 'positive'), (desc(dw=0), 'positive'), (desc(sh=1 << 16, sw=1 << 16), '2^31'),
                    (desc(dst=p), 'overlap'), (desc(src=q + 16), 'overlap'), (desc(resampling=3), 'average')):
        assert lib.satcv_raster_reproject(ctypes.byref(d), ctypes.byref(good), None) == -1, word
        assert word.encode() in lib.satcv_last_error() and b'raster_reproject' in lib.satcv_last_error(), (word, lib.satcv_last_error())
    ok = desc()
    assert lib.satcv_raster_reproject(ctypes.byref(ok), None, None) == -1 and b'null map' in lib.satcv_last_error()
    u = (ctypes.c_double * 16)()
    bad_maps = ((rmap(dst_crs=crs(kind=3)), 'unknown kind'), (rmap(src_crs=crs(kind=-1)), 'unknown kind'), (rmap(dst_crs=crs(a=0.0)), 'a > 0'),
                (rmap(src_crs=crs(inv_f=-1.0)), 'inv_f > 0'), (rmap(dst_crs=crs(lon0=nan)), 'non-finite'), (rmap(src_crs=crs(fe=inf)), 'non-finite'),
                (rmap(src_crs=crs(a=nan)), 'non-finite'), (rmap(dst_crs=crs(k0=inf)), 'non-finite'), (rmap(dst_a=0.0), 'scale'), (rmap(dst_e=nan), 'scale'),
                (rmap(src_a=inf), 'scale'), (rmap(src_e=0.0), 'scale'), (rmap(dst_c=nan), 'origin'), (rmap(src_f=inf), 'origin'))
    for m, word in bad_maps:
        assert lib.satcv_raster_reproject(ctypes.byref(ok), ctypes.byref(m), None) == -1, word
        assert word.encode() in lib.satcv_last_error() and b'raster_reproject' in lib.satcv_last_error(), (word, lib.satcv_last_error())
        assert lib.satcv_grid_coords(ctypes.byref(m), 2, 2, 0, 0, u, u, None) == -1 and b'grid_coords' in lib.satcv_last_error(), word
    for args, word in (((None, 2, 2, 0, 0, u, u), 'null map'), ((ctypes.byref(good), 0, 2, 0, 0, u, u), 'positive'), ((ctypes.byref(good), 2, 2, 0, 0, None, u), 'null pointer'),
                       ((ctypes.byref(good), 1 << 16, 1 << 16, 0, 0, u, u), '2^31')):
        assert lib.satcv_grid_coords(*args, None) == -1 and word.encode() in lib.satcv_last_error(), word
    a, b = crs(4326), crs(3857)
    x = (ctypes.c_double * 2)(1.0, 2.0)
    for args, word in (((None, ctypes.byref(b), x, x, x, x, None, 2, 0), 'null CRS'), ((ctypes.byref(a), ctypes.byref(crs(kind=9)), x, x, x, x, None, 2, 0), 'unknown kind'),
                       ((ctypes.byref(a), ctypes.byref(b), None, x, x, x, None, 2, 0), 'null pointer'), ((ctypes.byref(a), ctypes.byref(b), x, x, x, x, None, -1, 0), 'points'),
                       ((ctypes.byref(a), ctypes.byref(b), x, x, x, x, None, 2, 2), 'on_device')):
        assert lib.satcv_crs_transform(*args, None) == -1 and word.encode() in lib.satcv_last_error() and b'crs_transform' in lib.satcv_last_error(), word
    assert lib.satcv_crs_transform(ctypes.byref(a), ctypes.byref(b), None, None, None, None, None, 0, 0, None) == 0
