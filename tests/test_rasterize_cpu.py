"""CPU checks of polygon rasterization: the consequences of the rule that are known without any code (rectangles, closed rings, fans
of triangles, a polygon and its complement), the NumPy oracle (tests/rasterize_oracle.py) against the library's host loop
(satcv_rasterize with on_device = 0, the same csrc/rasterize_core.hpp the kernels use) exactly, the edge table against brute-force
counts, `geometry_rings` on every form, every refusal of the C ABI (each before any launch, shown by a sentinel-filled destination),
and the window and polygon helpers of utils/raster_tools.py against fixtures of the reference's own bodies."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rasterize_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _poly(*rings):
    return {'type': 'Polygon', 'coordinates': [[list(p) for p in r] for r in rings]}


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def _grid(shape, transform=None):
    from satellite_computervision_amd import raster_tools as rt
    return rt.Grid(transform or (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), shape)


def comb(teeth, x0=1.0, pitch=2.0, top=0.0, mid=1.0, bottom=2.0):
    """a comb: a bar over rows [mid, bottom) and `teeth` teeth of one pixel over rows [top, mid): a row through the teeth is crossed
    2 * teeth times, a row through the bar twice"""
    pts = [(x0, bottom), (x0, top)]
    for k in range(teeth):
        a = x0 + k * pitch
        pts += [(a + 1.0, top), (a + 1.0, mid)] if k == 0 else [(a, mid), (a, top), (a + 1.0, top), (a + 1.0, mid)]
    pts += [(x0 + (teeth - 1) * pitch + 1.0, bottom)]
    return pts


def cases():
    """name -> (shape, [geometry as a list of rings in pixel coordinates]): every case the host loop and the kernels are held to"""
    rng = np.random.default_rng(5)
    out = {
        'one pixel': ((1, 1), [[_rect(-1, -1, 2, 2)]]),
        'one pixel missed': ((1, 1), [[_rect(0.6, 0.6, 2, 2)]]),
        'small': ((3, 5), [[[(0.2, 0.1), (4.9, 0.3), (2.5, 2.9)]]]),
        'hole': ((37, 53), [[_rect(4, 3, 47, 33), _rect(10.3, 8.2, 30.7, 20.5)]]),
        'multipolygon': ((37, 53), [[_rect(2, 2, 12, 12), _rect(20.5, 5.5, 40.5, 30.5), [(5, 20), (15, 35), (1, 30)]]]),
        'outside': ((37, 53), [[_rect(60, 40, 80, 50)], [_rect(-30, -30, -2, -1)]]),
        'partly outside': ((37, 53), [[[(-20.3, 10.2), (30.1, -15.7), (70.9, 20.2), (25.5, 60.1)]]]),
        'covers': ((37, 53), [[_rect(-5, -5, 100, 100)]]),
        'on centres': ((37, 53), [[[(2.5, 3.5), (10.5, 3.5), (10.5, 8.5), (2.5, 8.5)]], [[(20.5, 10.5), (30.5, 20.5), (20.5, 30.5), (10.5, 20.5)]]]),
        'comb 17': ((3, 53), [[comb(17)]]),                  # 34 crossings in row 0: one pair more than 32
        'comb 5': ((3, 53), [[comb(5)]]),                    # 10: one pair more than 8
        'random': ((37, 53), [[rng.uniform(-5, 58, (9, 2)).tolist()] for _ in range(6)]),
        'tall': ((300, 7), [[[(1.2, -3.0), (5.7, 150.2), (2.1, 310.0)]]]),      # edges of more than 64 rows: split work items
    }
    squares = []
    for k in range(300):
        x, y = (k % 20) * 2.5 + 0.25, (k // 20) * 2.25 + 0.25
        squares.append([_rect(x, y, x + 4, y + 4)])
    out['squares'] = ((37, 53), squares)
    return out


CASES = cases()


def _values(n):
    return [(k * 7) % 250 + 1 for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_rectangles_cover_what_the_rule_says():
    m = ro.mask([[_rect(2, 3, 10, 8)]], (12, 14))
    want = np.zeros((12, 14), np.uint8)
    want[3:8, 2:10] = 1
    assert np.array_equal(m, want)
    m = ro.mask([[_rect(2.5, 3.5, 10.5, 8.5)]], (12, 14))      # top and right centres in, bottom and left centres out
    want[:] = 0
    want[3:8, 3:11] = 1
    assert np.array_equal(m, want)


def test_the_library_covers_the_same_rectangles():
    from satellite_computervision_amd import raster_tools as rt
    for rect, rows, cols in ((_rect(2, 3, 10, 8), slice(3, 8), slice(2, 10)), (_rect(2.5, 3.5, 10.5, 8.5), slice(3, 8), slice(3, 11))):
        want = np.zeros((12, 14), np.uint8)
        want[rows, cols] = 1
        assert np.array_equal(rt.geometry_mask(_poly(rect), _grid((12, 14)), device=False), want)
        assert np.array_equal(rt.rasterize([(_poly(rect), 5)], _grid((12, 14)), fill=2, device=False), np.where(want != 0, 5, 2).astype(np.uint8))


def test_every_row_of_a_closed_ring_has_an_even_count_also_after_the_clamp():
    rng = np.random.default_rng(1)
    for k in range(50):
        ring = rng.uniform(-40, 90, (int(rng.integers(3, 12)), 2))
        if k % 2:
            ring = np.round(ring * 2) / 2
        assert not (ro.row_counts([[ring]], (37, 53)) % 2).any()
        crosses, col = ro.crossings([ring], (37, 53))
        assert col.min() >= 0 and col.max() <= 53


def test_fans_of_triangles_partition_their_outline():
    rng = np.random.default_rng(2)
    shape = (31, 33)
    fans = 0
    while fans < 200:
        n = int(rng.integers(4, 9))
        centre = np.round(rng.uniform(8, 24, 2) * 2) / 2
        ang = rng.uniform(0, 2 * np.pi, n)
        outline = np.round((centre + rng.uniform(3, 15, (n, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=1)) * 2) / 2
        ang = np.arctan2(outline[:, 1] - centre[1], outline[:, 0] - centre[0])      # (of the rounded vertices: rounding may reorder them)
        outline, ang = outline[np.argsort(ang)], np.sort(ang)
        gaps = np.diff(np.concatenate([ang, [ang[0] + 2 * np.pi]]))
        if gaps.max() >= np.pi - 1e-9 or gaps.min() <= 1e-9:
            continue                                            # (the centre must see every outline edge from inside, no two vertices on one ray)
        fans += 1
        total = np.zeros(shape, np.int64)
        for k in range(n):
            total += ro.inside([[centre, outline[k], outline[(k + 1) % n]]], shape)
        assert np.array_equal(total, ro.inside([outline], shape).astype(np.int64))      # no pixel twice, none missing
        if fans <= 25:                                          # the library's host loop on the same fans: every triangle its own geometry
            from satellite_computervision_amd import raster_tools as rt
            tris = [_poly([centre, outline[k], outline[(k + 1) % n]]) for k in range(n)]
            burned = rt.rasterize(tris, _grid(shape), values=list(range(1, n + 1)), fill=0, device=False)
            whole = rt.geometry_mask(_poly(outline), _grid(shape), device=False)
            assert np.array_equal(burned != 0, whole != 0)
            assert sum(int((rt.geometry_mask(t, _grid(shape), device=False) != 0).sum()) for t in tris) == int(whole.sum())      # none twice


def test_a_polygon_and_its_complement_with_a_hole_cover_the_grid_once():
    rng = np.random.default_rng(3)
    shape = (37, 53)
    for _ in range(20):
        ring = rng.uniform(2, 35, (7, 2))
        a = ro.inside([ring], shape).astype(np.int64)
        b = ro.inside([_rect(-1, -1, 60, 40), ring], shape).astype(np.int64)
        assert np.array_equal(a + b, np.ones(shape, np.int64))
        from satellite_computervision_amd import raster_tools as rt
        la = rt.geometry_mask(_poly(ring), _grid(shape), device=False).astype(np.int64)
        lb = rt.geometry_mask(_poly(_rect(-1, -1, 60, 40), ring), _grid(shape), device=False).astype(np.int64)
        assert np.array_equal(la, a) and np.array_equal(la + lb, np.ones(shape, np.int64))


def test_the_oracle_agrees_with_matplotlib_where_no_centre_is_near_an_edge():
    """`Path.contains_points` on pixel centres, recorded by tests/golden/make_vector_fixtures.py for polygons with no centre within 1e-6
    of an edge: an independent statement of "the centre lies inside"."""
    z = np.load(os.path.join(GOLD, 'vector_helpers_reference.npz'))
    shape = tuple(int(v) for v in z['path_shape'])
    assert len(z['path_rings']) == 40
    for ring, want in zip(z['path_rings'], z['path_inside']):
        assert np.array_equal(ro.inside([ring], shape), want.astype(bool))


# ---------------------------------------------------------------------------------------------------------------- the host loop
def _geojson(geoms):
    return [{'type': 'MultiPolygon', 'coordinates': [[[list(map(float, p)) for p in r]] for r in g]} for g in geoms]


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_host_loop_equals_the_oracle(name):
    from satellite_computervision_amd import raster_tools as rt
    shape, geoms = CASES[name]
    grid = _grid(shape)
    assert np.array_equal(rt.geometry_mask(_geojson(geoms), grid, device=False), ro.mask(geoms, shape))
    assert np.array_equal(rt.geometry_mask(_geojson(geoms), grid, invert=True, device=False), ro.mask(geoms, shape, invert=True))
    vals = _values(len(geoms))
    for dtype, fill in (('uint8', 0), ('int16', -3), ('float32', float('nan')), ('uint16', 65535), ('int32', -70000)):
        got = rt.rasterize(list(zip(_geojson(geoms), vals)), grid, fill=fill, dtype=dtype, device=False)
        assert got.dtype == np.dtype(dtype) and np.array_equal(got, ro.burn(geoms, shape, vals, fill, np.dtype(dtype)), equal_nan=True)


def test_keep_without_out_has_nothing_to_keep():
    from satellite_computervision_amd import raster_tools as rt
    shape, geoms = CASES['hole']
    got = rt.rasterize(_geojson(geoms), _grid(shape), values=[9], fill=4, dtype='int16', keep=True, device=False)
    assert np.array_equal(got, ro.burn(geoms, shape, [9], 4, np.int16))


def test_the_host_loop_on_a_georeferenced_grid_with_layouts_and_keep():
    from satellite_computervision_amd import raster_tools as rt
    t = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    grid = _grid((37, 53), t)
    ring = [(500031.0, 4099955.0), (500402.5, 4099990.0), (500480.0, 4099700.5), (500100.0, 4099651.0)]
    want = ro.inside([ro.pixels(ring, t)], (37, 53))
    assert want.any() and not want.all()
    for layout, shape, at in (('hwc', (37, 53, 3), np.s_[:, :, 1]), ('chw', (3, 37, 53), np.s_[1])):
        out = np.full(shape, 9, np.uint16)
        got = rt.rasterize([(_poly(ring), 500)], grid, dtype='uint16', out=out, channel_offset=1, layout=layout, keep=True, device=False)
        assert got is out
        exp = np.full(shape, 9, np.uint16)
        exp[at][want] = 500
        assert np.array_equal(out, exp)


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_edge_table_matches_brute_force_counts(name):
    from satellite_computervision_amd import polygons as pg
    shape, geoms = CASES[name]
    px = [[np.asarray(r, np.float64) for r in g] for g in geoms]
    table, row_start = pg.edge_table(px, shape)
    assert table.dtype == np.float64 and table.shape[1] == 7 and row_start.dtype == np.int32 and row_start.shape == (shape[0] + 1,)
    assert np.array_equal(np.diff(row_start), ro.row_counts(geoms, shape)) and row_start[0] == 0
    rows = np.arange(shape[0]) + 0.5
    got = np.zeros(shape[0], np.int64)
    for x0, y0, x1, y1, r0, r1, g in table:
        assert y0 < y1 and 0 <= r0 < r1 <= shape[0] and r1 - r0 <= 64 and 0 <= g < len(geoms)
        crosses = (y0 <= rows) & (rows < y1)
        assert crosses[int(r0):int(r1)].all()                  # every named row is crossed ...
        got[int(r0):int(r1)] += 1
    assert np.array_equal(got, ro.row_counts(geoms, shape))      # ... and none is left out


# ---------------------------------------------------------------------------------------------------------------- geometry_rings
def test_geometry_rings_accepts_every_form():
    from satellite_computervision_amd import raster_tools as rt
    p = _poly(_rect(0, 0, 4, 4) + [(0, 0)], _rect(1, 1, 2, 2))
    mp = {'type': 'MultiPolygon', 'coordinates': [p['coordinates'], [[list(q) for q in _rect(6, 6, 9, 9)]]]}
    feat = {'type': 'Feature', 'properties': {}, 'geometry': p}
    fc = {'type': 'FeatureCollection', 'features': [feat, {'type': 'Feature', 'geometry': mp}]}
    gc = {'type': 'GeometryCollection', 'geometries': [p, mp]}

    class Shape:
        __geo_interface__ = p

    one = rt.geometry_rings(p)
    assert len(one) == 1 and len(one[0]) == 2 and one[0][0].shape == (4, 2) and one[0][0].dtype == np.float64      # (the closing vertex is dropped)
    assert [len(g) for g in rt.geometry_rings(mp)] == [3]                       # one geometry: even-odd over all rings
    assert [len(g) for g in rt.geometry_rings(feat)] == [2]
    assert [len(g) for g in rt.geometry_rings(fc)] == [2, 3]
    assert [len(g) for g in rt.geometry_rings(gc)] == [2, 3]
    assert [len(g) for g in rt.geometry_rings(Shape())] == [2]
    assert [len(g) for g in rt.geometry_rings([p, Shape(), fc])] == [2, 2, 2, 3]
    assert rt.geometry_bounds(mp) == (0.0, 0.0, 9.0, 9.0)


def test_geometry_rings_refuses_the_rest():
    from satellite_computervision_amd import raster_tools as rt
    for bad in ({'type': 'Point', 'coordinates': [0, 0]}, {'type': 'LineString', 'coordinates': [[0, 0], [1, 1]]},
                {'type': 'MultiLineString', 'coordinates': [[[0, 0], [1, 1]]]}, {'type': 'MultiPoint', 'coordinates': [[0, 0]]},
                {'type': 'GeometryCollection', 'geometries': [{'type': 'Point', 'coordinates': [0, 0]}]}):
        with pytest.raises(ValueError, match='lines and points'):
            rt.geometry_rings(bad)
    for bad in (_poly([(0, 0), (1, 1)]), _poly([(0, 0), (1, 1), (0, 0)]), _poly([(0, 0), (1, 1), (1, 1), (0, 0)])):
        with pytest.raises(ValueError, match='three distinct'):
            rt.geometry_rings(bad)
    for bad in (3, 'POLYGON', {'coordinates': []}, {'type': 'Polygon', 'coordinates': []}, {'type': 'Feature', 'geometry': None}):
        with pytest.raises(ValueError):
            rt.geometry_rings(bad)
    grid = _grid((4, 4))
    with pytest.raises(ValueError, match='all_touched'):
        rt.rasterize([_poly(_rect(0, 0, 2, 2))], grid, all_touched=True, device=False)
    with pytest.raises(ValueError, match='all_touched'):
        rt.geometry_mask(_poly(_rect(0, 0, 2, 2)), grid, all_touched=True, device=False)
    with pytest.raises(ValueError, match='rotated'):
        rt.Grid((1.0, 0.1, 0.0, 0.0, 1.0, 0.0), (4, 4))
    with pytest.raises(ValueError, match='non-finite'):
        rt.geometry_mask(_poly([(0, 0), (float('nan'), 1), (2, 2)]), grid, device=False)
    with pytest.raises(ValueError, match='dtype'):
        rt.rasterize([_poly(_rect(0, 0, 2, 2))], grid, dtype='float64', device=False)
    with pytest.raises(ValueError, match='values'):
        rt.rasterize([_poly(_rect(0, 0, 2, 2))], grid, values=[1, 2], device=False)


def test_aoi_grid_holds_the_polygon_in_the_grids_crs():
    from satellite_computervision_amd import raster_tools as rt
    ring = [(-76.52, 38.91), (-76.48, 38.915), (-76.485, 38.95), (-76.525, 38.94)]
    g = rt.aoi_grid(_poly(ring), 10, 'EPSG:32618')
    xs, ys = rt.transform_points([p[0] for p in ring], [p[1] for p in ring], 'EPSG:4326', 'EPSG:32618')
    left, bottom, right, top = g.bounds
    assert g.crs == 'EPSG:32618' and g.resolution == (10.0, 10.0)
    assert left <= xs.min() and right >= xs.max() and bottom <= ys.min() and top >= ys.max()
    assert left % 10 == 0 and top % 10 == 0 and xs.min() - left < 200 and top - ys.max() < 200      # (the box of the polygon's bounds, turned by the grid convergence)
    assert rt.geometry_bounds(_poly(ring), 'EPSG:4326', 'EPSG:4326') == (-76.525, 38.91, -76.48, 38.95)
    # an EPSG:4326 polygon on the UTM grid is the rasterization of its transformed vertices
    m = rt.geometry_mask(_poly(ring), g, geom_crs='EPSG:4326', device=False)
    assert np.array_equal(m, ro.mask([[ro.pixels(np.stack([xs, ys], axis=1), g.transform)]], g.shape)) and m.any()


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def test_descriptor_layouts_match_the_header(tmp_path):
    from satellite_computervision_amd import _lib as L
    pairs = {'satcv_rasterize_desc': L.RasterizeDesc, 'satcv_mask_apply_desc': L.MaskApplyDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f'{cname}.{f}']) == getattr(cls, f).offset, f
    for sym in ('satcv_rasterize_workspace', 'satcv_rasterize', 'satcv_raster_mask_apply'):
        assert sym in L.EXPORTED_SYMBOLS


def _desc(shape=(8, 9), geoms=None, **over):
    """a valid host-loop descriptor of a triangle (kept alive by the returned holder), then `over`"""
    from satellite_computervision_amd import _lib as L
    from satellite_computervision_amd import polygons as pg
    geoms = geoms if geoms is not None else [[np.array([(1.0, 0.2), (7.5, 3.0), (2.0, 7.7)])]]
    table, row_start = pg.edge_table(geoms, shape)
    dst = np.full(shape, 77, np.uint8)
    hold = {'table': table, 'row_start': row_start, 'dst': dst, 'values': np.ones(max(len(geoms), 1), np.uint8)}
    d = L.RasterizeDesc(edges=table.ctypes.data, n_items=len(table), row_start=row_start.ctypes.data, h=shape[0], w_=shape[1], n_geoms=len(geoms), mode=0, invert=0,
                        values=None, fill=0.0, dst=dst.ctypes.data, dst_kind=0, dst_layout=0, dst_ld=1, dst_coff=0, keep=0, on_device=0)
    for k, v in over.items():
        setattr(d, k, v(hold) if callable(v) else v)
    return d, hold


def _refused(d, hold, text):
    from satellite_computervision_amd import _lib as L
    rc = L.lib.satcv_rasterize(ctypes.byref(d), None)
    msg = L.lib.satcv_last_error().decode()
    assert rc == -1 and msg.startswith('rasterize:') and text in msg, msg
    assert (hold['dst'] == 77).all()                            # nothing was written


def test_the_valid_descriptor_runs():
    from satellite_computervision_amd import _lib as L
    d, hold = _desc()
    assert L.lib.satcv_rasterize(ctypes.byref(d), None) == 0
    assert np.array_equal(hold['dst'], ro.mask([[[(1.0, 0.2), (7.5, 3.0), (2.0, 7.7)]]], (8, 9)))


def test_rasterize_refuses_on_the_host_and_writes_nothing():
    from satellite_computervision_amd import _lib as L
    assert L.lib.satcv_rasterize(None, None) == -1 and b'rasterize: null pointer' in L.lib.satcv_last_error()
    for over, text in ((dict(dst=None), 'null pointer (dst)'), (dict(row_start=None), 'null pointer (row_start)'), (dict(edges=None), 'null pointer (edges)'),
                       (dict(mode=1), 'null pointer (values)'), (dict(mode=2), 'mode 2'), (dict(dst_kind=4), 'dst_kind 4'), (dict(dst_kind=7), 'dst_kind 7'),
                       (dict(dst_kind=1), 'a mask is u8'), (dict(dst_layout=2), 'dst_layout 2'), (dict(h=0), 'sizes must be positive'),
                       (dict(w_=-1), 'sizes must be positive'), (dict(h=65536, w_=32768), '2^31'), (dict(dst_coff=1), 'does not fit ld'),
                       (dict(dst_coff=-1), 'does not fit ld'), (dict(dst_ld=0), 'does not fit ld'), (dict(on_device=2), 'on_device 2'),
                       (dict(n_geoms=0), 'names geometry'), (dict(n_items=-1), 'n_items'),
                       (dict(on_device=1), 'null pointer (workspace)')):
        d, hold = _desc(**over)
        _refused(d, hold, text)

    def edit(col, value, row=0):
        def f(hold):
            hold['table'][row, col] = value
            return hold['table'].ctypes.data
        return f
    for over, text in ((dict(edges=edit(0, float('nan'))), 'non-finite vertex'), (dict(edges=edit(3, float('inf'))), 'non-finite vertex'),
                       (dict(edges=edit(1, 100.0)), 'not ordered'), (dict(edges=edit(4, -1.0)), 'outside [0, 8]'), (dict(edges=edit(5, 9.0)), 'outside [0, 8]'),
                       (dict(edges=edit(4, 0.5)), 'outside [0, 8]'), (dict(edges=edit(6, 1.0)), 'names geometry 1 of 1'), (dict(edges=edit(6, -1.0)), 'names geometry'),
                       (dict(edges=edit(5, 8.0, row=0)), 'does not cross the rows')):
        d, hold = _desc(**over)
        _refused(d, hold, text)

    def shift(hold):
        hold['row_start'][3] += 1
        return hold['row_start'].ctypes.data
    d, hold = _desc(row_start=shift)
    _refused(d, hold, 'row_start[3]')

    def first(hold):
        hold['row_start'][0] = 1
        return hold['row_start'].ctypes.data
    d, hold = _desc(row_start=first)
    _refused(d, hold, 'row_start[0]')
    # a work item of more than 64 rows
    tall = [[np.array([(1.0, -1.0), (3.0, 200.0), (2.0, 100.0)])]]
    d, hold = _desc(shape=(150, 4), geoms=tall)
    hold['table'][0, 5] = hold['table'][0, 4] + 65
    _refused(d, hold, 'a work item has at most 64')


def test_rasterize_refuses_a_bad_workspace_on_the_host_and_writes_nothing():
    """on_device = 1 with HOST buffers: every refusal comes before the first HIP call, so nothing here touches a device.  (A workspace
    that merely touches dst is accepted; that case needs a device and is in tests/test_rasterize_gpu.py.)"""
    from satellite_computervision_amd import _lib as L
    d, hold = _desc()
    need = ctypes.c_int64()
    assert L.lib.satcv_rasterize_workspace(d.n_items, d.h, int(hold['row_start'][-1]), d.n_geoms, ctypes.byref(need)) == 0
    need, nd = int(need.value), d.h * d.w_
    big = np.full(need + nd + 512, 77, np.uint8)
    base = (big.ctypes.data + 15) // 16 * 16 + 128             # 16-aligned, 128 bytes of the buffer before it

    def refused(text, **over):
        dd, h = _desc(on_device=1, **over)
        _refused(dd, h, text)
        assert (big == 77).all()
    # apart from dst (the array of the descriptor's holder), large enough, but misaligned
    for off in (1, 4, 8):
        refused('misaligned pointer (workspace)', workspace=base + off, workspace_bytes=need + 16)
    # apart and aligned, one byte too small; zero; negative
    for nbytes in (need - 1, 0, -1):
        refused(f'workspace of {nbytes} bytes, {need} needed', workspace=base, workspace_bytes=nbytes)
    # dst inside the workspace; dst running into its start; dst starting in its last byte; the workspace inside dst
    refused('dst overlaps the workspace', workspace=base, workspace_bytes=need + nd + 64, dst=base + 16)
    refused('dst overlaps the workspace', workspace=base, workspace_bytes=need, dst=base - nd + 1)
    refused('dst overlaps the workspace', workspace=base, workspace_bytes=need, dst=base + need - 1)
    wide = dict(dst_ld=64, dst_coff=3)                         # dst of nd * 64 bytes would hold the workspace: only its extent matters, it is not written
    huge = np.full(nd * 64 + 64, 77, np.uint8)
    hb = (huge.ctypes.data + 15) // 16 * 16
    if need + 32 < nd * 64:
        refused('dst overlaps the workspace', workspace=hb + 16, workspace_bytes=need, dst=hb, **wide)
        assert (huge == 77).all()


def test_a_row_at_the_cap_runs_and_one_over_is_refused_naming_row_and_count():
    from satellite_computervision_amd import raster_tools as rt, _lib as L
    shape = (3, 4200)
    at_cap = [[comb(2048)]]                                     # 4096 crossings in row 0
    assert ro.row_counts(at_cap, shape)[0] == 4096
    assert np.array_equal(rt.geometry_mask(_geojson(at_cap), _grid(shape), device=False), ro.mask(at_cap, shape))
    over = [[comb(2048)], [_rect(10.2, -1.0, 20.7, 0.9)]]       # one pair more
    assert ro.row_counts(over, shape)[0] == 4098
    with pytest.raises(L.SatcvError, match=r'rasterize: row 0 has 4098 crossings \(at most 4096\)'):
        rt.geometry_mask(_geojson(over), _grid(shape), device=False)
    d, hold = _desc(shape=shape, geoms=[[np.asarray(r, np.float64) for r in g] for g in over])
    _refused(d, hold, 'row 0 has 4098 crossings')


def test_mask_apply_refuses_on_the_host():
    from satellite_computervision_amd import _lib as L
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    ok = dict(mask=p, h=2, w_=2, invert=0, src=p + 16, dst=p + 16, kind=0, layout=1, c=1, ld=1, coff=0, has_nodata=0, nodata=0.0)
    assert L.lib.satcv_raster_mask_apply(None, None) == -1 and b'raster_mask_apply: null pointer' in L.lib.satcv_last_error()
    for over, text in ((dict(mask=None), 'null pointer'), (dict(src=None), 'null pointer'), (dict(dst=None), 'null pointer'), (dict(kind=4), 'kind 4'),
                       (dict(layout=3), 'layout 3'), (dict(h=0), 'sizes must be positive'), (dict(c=0), 'sizes must be positive'), (dict(h=65536, w_=32768), '2^31'),
                       (dict(c=2), 'do not fit ld'), (dict(coff=1), 'do not fit ld'), (dict(kind=1, src=p + 17, dst=p + 17), 'misaligned'),
                       (dict(dst=p + 18), 'dst overlaps src'), (dict(src=p + 32, dst=p + 2), 'dst overlaps the mask')):
        d = L.MaskApplyDesc(**{**ok, **over})
        rc = L.lib.satcv_raster_mask_apply(ctypes.byref(d), None)
        msg = L.lib.satcv_last_error().decode()
        assert rc == -1 and msg.startswith('raster_mask_apply:') and text in msg, (over, msg)
    assert not buf.any()
    need = ctypes.c_int64()
    assert L.lib.satcv_rasterize_workspace(3, 8, 10, 1, ctypes.byref(need)) == 0 and need.value >= 3 * 56 + 80 + 36 + 32 + 4 and need.value % 16 == 0
    assert L.lib.satcv_rasterize_workspace(3, 8, 10, 1, None) == -1 and b'rasterize_workspace: null pointer' in L.lib.satcv_last_error()
    assert L.lib.satcv_rasterize_workspace(-1, 8, 10, 1, ctypes.byref(need)) == -1


# ---------------------------------------------------------------------------------------------------------------- the helpers
def test_window_helpers_match_the_reference_fixtures():
    """convert, make_window, win_jitter and make_jittered_window against outputs of the reference's own bodies (utils/raster_tools.py:70-331,
    run by tests/golden/make_vector_fixtures.py)"""
    from satellite_computervision_amd import raster_tools as rt
    z = np.load(os.path.join(GOLD, 'vector_helpers_reference.npz'))
    for s, b, want in zip(z['convert_size'], z['convert_box'], z['convert_out']):
        assert np.array_equal(np.array(rt.convert(tuple(int(v) for v in s), list(b))), want)
    for c, w, want in zip(z['window_cxy'], z['window_size'], z['window_out']):
        assert rt.make_window(float(c[0]), float(c[1]), int(w)) == tuple(int(v) for v in want)
    for k in range(len(z['jitter_seed'])):
        args = (float(z['jitter_centre'][k, 0]), float(z['jitter_centre'][k, 1]), int(z['jitter_dims'][k, 0]), int(z['jitter_dims'][k, 1]))
        np.random.seed(int(z['jitter_seed'][k]))
        assert tuple(rt.win_jitter(int(z['jitter_window'][k]), jitter_frac=float(z['jitter_frac'][k]))) == tuple(z['jitter_out'][k])
        np.random.seed(int(z['jitter_seed'][k]))
        got = rt.make_jittered_window(*args, window_size=int(z['jitter_window'][k]), jitter_frac=float(z['jitter_frac'][k]))
        assert got == tuple(int(v) for v in z['jittered_window_out'][k]) and all(isinstance(v, int) for v in got)


def test_convert_poly_coords_and_get_centroid_follow_their_formulas():
    """shapely is not available where the fixtures are made, so these two are held to their formulas: the affine map x' = a x + b y + c,
    y' = d x + e y + f and its inverse, and the area-weighted centroid rounded with np.rint."""
    from satellite_computervision_amd import raster_tools as rt
    t = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    ring = [(0.0, 0.0), (4.0, 0.0), (4.0, 2.5), (0.0, 2.5), (0.0, 0.0)]
    geo = rt.convert_poly_coords(ring, affine_obj=t)
    assert geo == [(500000.0 + 10 * x, 4100000.0 - 10 * y) for x, y in ring]
    assert np.allclose(rt.convert_poly_coords(geo, affine_obj=t, inverse=True), ring, rtol=0, atol=1e-9)
    assert rt.convert_poly_coords(ring, affine_obj=list(t) + [0.0, 0.0, 1.0]) == geo                      # the nine numbers of a rasterio transform
    sheared = (2.0, 0.5, 1.0, -0.25, 3.0, -2.0)
    back = rt.convert_poly_coords(rt.convert_poly_coords(ring, affine_obj=sheared), affine_obj=sheared, inverse=True)
    assert np.allclose(back, ring, rtol=0, atol=1e-12)
    wkt = 'POLYGON ((0 0, 4 0, 4 2.5, 0 2.5, 0 0), (1 1, 2 1, 2 2, 1 1))'
    out = rt.convert_poly_coords(wkt, affine_obj=t)
    assert isinstance(out, str) and out.startswith('POLYGON ((500000.0 4100000.0, 500040.0 4100000.0,') and out.count('(') == 3
    gj = rt.convert_poly_coords(_poly(ring), affine_obj=t)
    assert gj['type'] == 'Polygon' and [tuple(p) for p in gj['coordinates'][0]] == geo
    assert rt.convert_poly_coords([(0.12345, 1.98765)] * 3, affine_obj=(1, 0, 0, 0, 1, 0), precision=2) == [(0.12, 1.99)] * 3
    with pytest.raises(ValueError, match='affine_obj'):
        rt.convert_poly_coords(ring)
    with pytest.raises(TypeError):
        rt.convert_poly_coords(3, affine_obj=t)
    with pytest.raises(ValueError, match='WKT POLYGON'):
        rt.convert_poly_coords('LINESTRING (0 0, 1 1)', affine_obj=t)
    # centroids: a rectangle, an L (area-weighted, not the vertex mean), a square with a hole, either winding
    assert rt.get_centroid(_rect(0, 0, 10, 4)) == (5.0, 2.0)
    ell = [(0, 0), (10, 0), (10, 2), (2, 2), (2, 10), (0, 10)]       # area 36: centroid (2 * 10 * 5 + 2 * 8 * 1) / 36, symmetric
    want = np.rint((20 * 5 + 16 * 1) / 36.0)
    assert rt.get_centroid(ell) == (want, want) and rt.get_centroid(ell[::-1]) == (want, want)
    holed = 'POLYGON ((0 0, 12 0, 12 12, 0 12, 0 0), (6 0.5, 11.5 0.5, 11.5 11.5, 6 11.5, 6 0.5))'
    area = 144 - 5.5 * 11
    assert rt.get_centroid(holed) == (np.rint((144 * 6 - 60.5 * 8.75) / area), np.rint((144 * 6 - 60.5 * 6) / area))
    with pytest.raises(ValueError, match='zero area'):
        rt.get_centroid([(0, 0), (1, 1), (2, 2)])
