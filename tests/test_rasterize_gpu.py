"""GPU checks of polygon rasterization and raster masking (csrc/rasterize.hip: satcv_rasterize, satcv_raster_mask_apply;
raster_tools.rasterize, geometry_mask, mask_apply, clip; pc_tools.predict_change(region=), predict_change_files(aoi=)) against the
float64 oracle of tests/rasterize_oracle.py.

Bounds: every comparison is exact.  The crossing column is the same float64 expression in the oracle and in the kernel, which is
compiled without contraction; everything after it is integer arithmetic.

Shapes: (1, 1), (3, 5), (37, 53) (not a multiple of the wavefront), (3, 8197) (a strip is 8192 columns: two workgroups per row),
(300, 7) (edges of more than 64 rows: split work items), combs with one pair of crossings more than a power of two (the bitonic
padding) and with exactly 4096 crossings in a row (the cap); 300 overlapping squares for the order of the burn."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import calibration_oracle as co  # noqa: E402
import rasterize_oracle as ro  # noqa: E402
import warp_oracle as WO  # noqa: E402
from test_rasterize_cpu import CASES, _geojson, _poly, _rect, _values, comb  # noqa: E402

pytestmark = pytest.mark.gpu

STRIP = 8192
DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'float32')
FILL = {'uint8': 0, 'uint16': 65535, 'int16': -3, 'int32': -70000, 'float32': float('nan')}
GPU_CASES = dict(CASES)
GPU_CASES['strip'] = ((3, STRIP + 5), [[_rect(5.2, 0.2, STRIP + 3.6, 2.6)], [[(STRIP - 90.3, -1.0), (STRIP + 4.2, 1.4), (STRIP - 40.0, 4.0)]]])
GPU_CASES['cap'] = ((3, 4200), [[comb(2048)]])                  # 4096 crossings in row 0: the cap, and a full bitonic network


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, pc_tools as pc, raster_tools as rt, calibration as cal, _lib
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pc=pc, rt=rt, cal=cal, L=_lib)


def _grid(env, shape, transform=None, crs=None):
    return env['rt'].Grid(transform or (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), shape, crs)


def _dev(a):
    a = np.array(a, order='C')
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dtype):
    return t.contiguous().view(torch.uint8).cpu().numpy().view(dtype).reshape(tuple(t.shape))


_WANT = {}


def want_mask(name):
    if name not in _WANT:
        shape, geoms = GPU_CASES[name]
        _WANT[name] = ro.mask(geoms, shape)
        _WANT[name].setflags(write=False)
    return _WANT[name]


# ---------------------------------------------------------------------------------------------------------------- rasterize
@pytest.mark.parametrize('name', sorted(GPU_CASES))
def test_mask_and_burn_equal_the_oracle(env, name):
    rt = env['rt']
    shape, geoms = GPU_CASES[name]
    grid = _grid(env, shape)
    gj = _geojson(geoms)
    m = rt.geometry_mask(gj, grid)
    assert m.dtype == torch.uint8 and tuple(m.shape) == shape and np.array_equal(m.cpu().numpy(), want_mask(name))
    assert np.array_equal(rt.geometry_mask(gj, grid, invert=True).cpu().numpy(), 1 - want_mask(name))
    assert np.array_equal(rt.geometry_mask(gj, grid, device=False), want_mask(name))      # (the host loop: the same header)
    vals = _values(len(geoms))
    for dtype in DTYPES:
        got = _host(rt.rasterize(list(zip(gj, vals)), grid, fill=FILL[dtype], dtype=dtype), dtype)
        assert np.array_equal(got, ro.burn(geoms, shape, vals, FILL[dtype], np.dtype(dtype)), equal_nan=True), dtype


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', ['hwc', 'chw'])
def test_layouts_channel_offset_and_keep(env, dtype, layout):
    rt = env['rt']
    shape, geoms = GPU_CASES['squares']
    vals = [k % 100 + 1 for k in range(len(geoms))]
    nt = np.dtype(dtype)
    full = shape + (3,) if layout == 'hwc' else (3,) + shape
    at = np.s_[:, :, 2] if layout == 'hwc' else np.s_[2]
    before = np.random.default_rng(4).integers(101, 120, full).astype(nt)
    for keep in (False, True):
        out = _dev(before)
        got = rt.rasterize(_geojson(geoms), _grid(env, shape), values=vals, fill=7, dtype=dtype, out=out, channel_offset=2, layout=layout, keep=keep)
        assert got is out
        exp = before.copy()
        exp[at] = ro.burn(geoms, shape, vals, 7, nt, out=before[at] if keep else None)
        assert np.array_equal(_host(out, nt), exp)              # the other two channels are untouched


def test_two_runs_give_the_same_bytes_and_the_last_geometry_wins(env):
    rt = env['rt']
    shape, geoms = GPU_CASES['squares']
    vals = _values(len(geoms))
    runs = [rt.rasterize(_geojson(geoms), _grid(env, shape), values=vals, dtype='int32') for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    got = runs[0].cpu().numpy()
    last = np.zeros(shape, np.int64)
    for k, g in enumerate(geoms):
        last[ro.inside(g, shape)] = k + 1
    assert (last > 0).any() and np.array_equal(got[last > 0], np.array(vals)[last[last > 0] - 1])
    many = sum(ro.inside(g, shape).astype(np.int64) for g in geoms)
    assert many.max() >= 3                                      # (neighbours do overlap)


def test_a_row_over_the_cap_is_refused_with_no_launch(env):
    rt, L = env['rt'], env['L']
    shape = (3, 4200)
    over = [[comb(2048)], [_rect(10.2, -1.0, 20.7, 0.9)]]
    out = torch.full(shape, 77, dtype=torch.uint8, device='cuda')
    with pytest.raises(L.SatcvError, match=r'rasterize: row 0 has 4098 crossings \(at most 4096\)'):
        rt.rasterize(_geojson(over), _grid(env, shape), out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    with pytest.raises(ValueError, match='all_touched'):
        rt.geometry_mask(_geojson(over), _grid(env, shape), all_touched=True)


def test_keep_without_out_has_nothing_to_keep(env):
    rt = env['rt']
    shape, geoms = GPU_CASES['hole']
    got = rt.rasterize(_geojson(geoms), _grid(env, shape), values=[9], fill=4, dtype='int16', keep=True)
    assert np.array_equal(got.cpu().numpy(), ro.burn(geoms, shape, [9], 4, np.int16))


def test_a_workspace_that_touches_dst_runs_and_one_that_overlaps_is_refused(env):
    import ctypes
    from satellite_computervision_amd import polygons as pg
    L, ops = env['L'], env['ops']
    shape, geoms = GPU_CASES['hole']
    table, row_start = pg.edge_table([[np.asarray(r, np.float64) for r in g] for g in geoms], shape)
    need = ctypes.c_int64()
    L.check(L.lib.satcv_rasterize_workspace(len(table), shape[0], int(row_start[-1]), len(geoms), ctypes.byref(need)))
    need, nd = int(need.value), shape[0] * shape[1]
    lead = (nd + 15) // 16 * 16
    buf = torch.full((lead + need + 64,), 77, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0

    def call(dst, ws, nbytes):
        d = L.RasterizeDesc(edges=table.ctypes.data, n_items=len(table), row_start=row_start.ctypes.data, h=shape[0], w_=shape[1], n_geoms=len(geoms), mode=0, invert=0,
                            values=None, fill=0.0, dst=dst, dst_kind=0, dst_layout=0, dst_ld=1, dst_coff=0, keep=0, on_device=1, workspace=ws, workspace_bytes=nbytes)
        return L.lib.satcv_rasterize(ctypes.byref(d), ops.stream_ptr())
    base = buf.data_ptr()
    for dst, ws in ((base + lead - nd + 1, base + lead), (base + lead + need - 1, base + lead), (base + lead + 16, base + lead)):
        assert call(dst, ws, need if dst != base + lead + 16 else need + 64) == -1 and b'rasterize: dst overlaps the workspace' in L.lib.satcv_last_error()
    assert call(base, base + lead, need - 1) == -1 and b'needed' in L.lib.satcv_last_error()
    assert call(base, base + lead + 8, need) == -1 and b'misaligned pointer (workspace)' in L.lib.satcv_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 77).all())                              # nothing was launched
    # dst ends where the workspace begins (with nd a multiple of 16 exactly there): it runs
    assert call(base + lead - nd, base + lead, need) == 0
    got = buf[lead - nd:lead].view(shape).cpu().numpy()
    assert np.array_equal(got, want_mask('hole')) and bool((buf[:lead - nd] == 77).all()) and bool((buf[lead + need:] == 77).all())


def test_a_capturing_stream_is_refused(env):
    """the edge table is copied from host memory the caller releases: a captured copy would be replayed from it"""
    rt, L = env['rt'], env['L']
    shape, geoms = GPU_CASES['small']
    out = torch.full(shape, 77, dtype=torch.uint8, device='cuda')
    g = torch.cuda.CUDAGraph()
    with pytest.raises(L.SatcvError, match='rasterize: the stream is being captured'):
        with torch.cuda.graph(g):
            rt.rasterize(_geojson(geoms), _grid(env, shape), out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert np.array_equal(rt.geometry_mask(_geojson(geoms), _grid(env, shape)).cpu().numpy(), want_mask('small'))      # and the library goes on working


def test_a_polygon_of_another_crs_is_the_rasterization_of_its_transformed_vertices(env):
    rt = env['rt']
    t = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
    grid = _grid(env, (37, 53), t, 'EPSG:32633')
    corners = np.array([(400010.0, 4499950.0), (400430.5, 4499990.0), (400470.0, 4499700.5), (400100.0, 4499651.0), (400200.0, 4499800.0)])
    lon, lat = rt.transform_points(corners[:, 0], corners[:, 1], 'EPSG:32633', 'EPSG:4326')
    aoi = _poly(list(zip(lon.tolist(), lat.tolist())))
    xs, ys = rt.transform_points(lon, lat, 'EPSG:4326', 'EPSG:32633')
    got = rt.geometry_mask(aoi, grid, geom_crs='EPSG:4326')
    same = rt.geometry_mask(_poly(list(zip(xs.tolist(), ys.tolist()))), grid)
    assert torch.equal(got, same)
    want = ro.mask([[ro.pixels(np.stack([xs, ys], axis=1), t)]], (37, 53))
    assert want.any() and not want.all() and np.array_equal(got.cpu().numpy(), want)
    burned = rt.rasterize([(aoi, 9)], grid, geom_crs='EPSG:4326', dtype='int16', fill=-1)
    assert np.array_equal(burned.cpu().numpy(), np.where(want != 0, 9, -1).astype(np.int16))


# ---------------------------------------------------------------------------------------------------------------- mask_apply
def _sample(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    nt = np.dtype(dtype)
    if nt.kind == 'f':
        return (rng.standard_normal(shape) * 1000).astype(np.float32)
    info = np.iinfo(nt)
    return rng.integers(max(info.min, -30000), min(info.max, 30000), shape, endpoint=True).astype(nt)


def _in_canaries(a, pad=64):
    """a device tensor that holds `a` between two runs of canary bytes: -> (tensor view, the whole buffer)"""
    nt = a.dtype
    buf = np.frombuffer(np.full((a.size + 2 * pad) * nt.itemsize, 0xa5, np.uint8).tobytes(), nt).copy()
    buf[pad:pad + a.size] = a.ravel()
    whole = _dev(buf)
    return whole[pad:pad + a.size].view(a.shape), whole


def _canaries_intact(whole, n, dtype, pad=64):
    raw = _host(whole, np.dtype(dtype)).view(np.uint8)
    item = np.dtype(dtype).itemsize
    return bool((raw[:pad * item] == 0xa5).all() and (raw[(pad + n) * item:] == 0xa5).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('form', ['hwc', 'hw', 'chw', 'stack'])
def test_mask_apply_equals_the_oracle(env, dtype, form):
    rt = env['rt']
    H, W = 37, 53                                               # 53 samples a row: no plane is a multiple of 16 bytes, no plane but the first aligned
    shape = {'hwc': (H, W, 3), 'hw': (H, W), 'chw': (3, H, W), 'stack': (2, 3, H, W)}[form]
    layout = 'hwc' if form in ('hwc', 'hw') else 'chw'
    a = _sample(dtype, shape, 11)
    mask = want_mask('multipolygon')
    dm = _dev(mask)
    for invert in (False, True):
        for nodata in (None, 5):
            nd = nodata if nodata is not None else (np.nan if dtype == 'float32' else 0)
            want = ro.apply_mask(a, mask, nd, invert, layout)
            src = _dev(a)
            got = rt.mask_apply(src, dm, nodata=nodata, invert=invert, layout=layout)
            assert got is not src and np.array_equal(_host(got, dtype), want, equal_nan=True) and np.array_equal(_host(src, dtype), a)
            view, whole = _in_canaries(a)
            assert rt.mask_apply(view, dm, nodata=nodata, invert=invert, layout=layout, inplace=True) is view
            assert np.array_equal(_host(view, dtype), want, equal_nan=True) and _canaries_intact(whole, a.size, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_mask_apply_on_one_slot_of_a_stack_and_on_some_channels(env, dtype):
    ops, rt = env['ops'], env['rt']
    from satellite_computervision_amd.tiff_container import DTYPES as KINDS
    H, W, T, Cn = 37, 53, 3, 2
    mask = want_mask('hole')
    dm = _dev(mask)
    a = _sample(dtype, (T, Cn, H, W), 12)
    view, whole = _in_canaries(a)
    ops.raster_mask_apply(dm, view, view, KINDS[dtype][1], 1, H, W, Cn, 1 * Cn, T * Cn, nodata=9)      # slot 1, in place
    want = a.copy()
    want[1] = ro.apply_mask(a[1], mask, 9, False, 'chw')
    assert np.array_equal(_host(view, dtype), want) and _canaries_intact(whole, a.size, dtype)
    b = _sample(dtype, (H, W, 5), 13)                            # channels 1 ... 3 of 5, out of place: the others are not written
    src = _dev(b)
    dview, dwhole = _in_canaries(np.full_like(b, 1))
    ops.raster_mask_apply(dm, src, dview, KINDS[dtype][1], 0, H, W, 3, 1, 5, nodata=None, invert=True)
    want = np.full_like(b, 1)
    want[..., 1:4] = ro.apply_mask(b[..., 1:4], mask, np.nan if dtype == 'float32' else 0, True, 'hwc')
    assert np.array_equal(_host(dview, dtype), want, equal_nan=True) and _canaries_intact(dwhole, b.size, dtype)


def test_mask_apply_refuses_what_does_not_fit(env):
    rt = env['rt']
    a = torch.zeros((3, 8, 9), dtype=torch.float32, device='cuda')
    for call in (lambda: rt.mask_apply(a, torch.ones((8, 8), dtype=torch.uint8, device='cuda'), layout='chw'),
                 lambda: rt.mask_apply(a, torch.ones((8, 9), dtype=torch.float32, device='cuda'), layout='chw'),
                 lambda: rt.mask_apply(a.cpu(), torch.ones((8, 9), dtype=torch.uint8, device='cuda'), layout='chw'),
                 lambda: rt.mask_apply(a.double(), torch.ones((8, 9), dtype=torch.uint8, device='cuda'), layout='chw'),
                 lambda: rt.mask_apply(a[None, None], torch.ones((8, 9), dtype=torch.uint8, device='cuda'), layout='chw')):
        with pytest.raises(ValueError):
            call()


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_clip_masks_and_crops_to_the_window_of_the_geometry(env):
    rt = env['rt']
    t = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
    grid = _grid(env, (37, 53), t, 'EPSG:32633')
    ring = [(400063.0, 4499921.0), (400381.5, 4499899.0), (400340.0, 4499740.5), (400101.0, 4499760.0)]
    px = ro.pixels(ring, t)
    want_m = ro.mask([[px]], (37, 53))
    r0, r1, c0, c1 = int(np.floor(px[:, 1].min())), int(np.ceil(px[:, 1].max())), int(np.floor(px[:, 0].min())), int(np.ceil(px[:, 0].max()))
    assert (r0, r1, c0, c1) == (7, 26, 10, 43)
    a = _sample('uint16', (37, 53, 3), 21)
    got, g = rt.clip(_dev(a), grid, _poly(ring), nodata=0)
    assert tuple(got.shape) == (19, 33, 3) and np.array_equal(_host(got, np.uint16), ro.apply_mask(a, want_m, 0)[r0:r1, c0:c1])
    assert g == rt.Grid((10.0, 0.0, t[2] + 10.0 * c0, 0.0, -10.0, t[5] - 10.0 * r0), (19, 33), 'EPSG:32633')
    stack = _sample('float32', (2, 3, 37, 53), 22)
    got, g2 = rt.clip(_dev(stack), grid, _poly(ring), layout='chw')
    assert g2 == g and np.array_equal(_host(got, np.float32), ro.apply_mask(stack, want_m, np.nan, layout='chw')[..., r0:r1, c0:c1], equal_nan=True)
    src = _dev(a)
    whole, g3 = rt.clip(src, grid, _poly(ring), nodata=0, crop=False, inplace=True)
    assert whole is src and g3 == grid and np.array_equal(_host(src, np.uint16), ro.apply_mask(a, want_m, 0))
    with pytest.raises(ValueError, match='do not intersect'):
        rt.clip(_dev(a), grid, _poly(_rect(0.0, 0.0, 10.0, 10.0)))


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
def test_equalize_takes_its_region_from_a_geometry(env, name):
    rt, cal = env['rt'], env['cal']
    grid = _grid(env, (37, 53))
    region = rt.geometry_mask(_geojson(GPU_CASES['hole'][1]), grid)
    rng = np.random.default_rng(31)
    info = np.iinfo(name)
    a = rng.integers(info.min // 4, info.max // 4, (3, 37, 53)).astype(name)
    b = (a.astype(np.int64) // 2 + 3).astype(name)
    got = cal.equalize(_dev(a), _dev(b), region=region, dtype=name)
    assert np.array_equal(_host(got, name), co.equalize(a, b, None, want_mask('hole')))


T10 = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)


@pytest.fixture(scope='module')
def change(env, tmp_path_factory):
    """three tiny uint16 COGs of three bands on shifted 10 m grids, the smallest model of the file tests, an area of interest in
    EPSG:4326 and the call without it -- computed once"""
    rt, pc, mt = env['rt'], env['pc'], env['mt']
    d = tmp_path_factory.mktemp('aoi')
    mt.reset_uids(); mt.set_seed(6)
    m = mt.get_unet_model(2, 6, filters=[32, 64], factors=[2, 2])
    m.compute_dtype = 'bfloat16'
    rng = np.random.default_rng(8)
    arrs, ts, paths = [], [], []
    for k in range(3):
        shape = (70 + k, 90 - k)
        a = rng.integers(1, 9000, shape + (3,)).astype(np.uint16)
        a[5:9, 7:12] = 0
        t = (10.0, 0.0, T10[2] + 10.0 * k, 0.0, -10.0, T10[5] - 20.0 * k)
        arrs.append(a); ts.append(t)
        paths.append(rt.write_cog(a, str(d / f'c{k}.tif'), t, 'EPSG:32633', nodata=0, blocksize=16, compress='lzw', overviews=0))
    kw = dict(kernel=32, buff=16, batch_size=4, fill=0.0)
    plain = pc.predict_change_files(paths[:2], paths[2:], m, **kw)
    return dict(m=m, arrs=arrs, ts=ts, paths=paths, kw=kw, plain=plain, dir=d)


def _aligned(change, grid):
    return [WO.warp_between(a, t, grid.transform, grid.shape, 'nearest', src_nodata=0, dst_nodata=0)[0].transpose(2, 0, 1) for a, t in zip(change['arrs'], change['ts'])]


def test_predict_change_files_clips_to_an_area_of_interest(env, change):
    rt, pc = env['rt'], env['pc']
    corners = np.array([(400021.0, 4499951.0), (400790.5, 4499930.0), (400760.0, 4499390.5), (400400.0, 4499340.0), (400052.0, 4499420.0)])
    lon, lat = rt.transform_points(corners[:, 0], corners[:, 1], 'EPSG:32633', 'EPSG:4326')
    aoi = {'type': 'Feature', 'properties': {}, 'geometry': _poly(list(zip(lon.tolist(), lat.tolist())))}
    out_file = str(change['dir'] / 'clipped.tif')
    got = pc.predict_change_files(change['paths'][:2], change['paths'][2:], change['m'], aoi=aoi, out_file=out_file, **change['kw'])
    grid = rt.aoi_grid(aoi, 10.0, 'EPSG:32633')
    assert grid.shape[0] >= 48 and grid.shape[1] >= 48 and got[0].shape == grid.shape
    xs, ys = rt.transform_points(lon, lat, 'EPSG:4326', 'EPSG:32633')
    inside = ro.mask([[ro.pixels(np.stack([xs, ys], axis=1), grid.transform)]], grid.shape) != 0
    assert inside.any() and not inside.all()
    assert np.isnan(got[0][~inside]).all() and not np.isnan(got[0][inside]).any()      # the map is nodata outside the oracle mask, and only there
    stacks = _aligned(change, grid)
    for s in stacks:
        s[:, ~inside] = 0
    want = pc.predict_change(np.stack(stacks[:2]), np.stack(stacks[2:]), change['m'], **change['kw'])
    assert want[0][inside].max() > 0 and np.array_equal(got[0][inside], want[0][inside])
    for g, w_ in zip(got[1:], want[1:]):                        # the composites were made of clipped stacks
        assert np.array_equal(g, w_, equal_nan=True) and np.isnan(g[~inside]).all()
    back = rt.read_cog(out_file)
    assert back.transform == grid.transform and back.crs == 'EPSG:32633'
    assert np.array_equal(back.array.cpu().numpy()[..., 0], got[0], equal_nan=True)
    # a ready mask instead of files: the same map
    region = rt.geometry_mask(aoi, grid, geom_crs='EPSG:4326')
    plain = _aligned(change, grid)
    again = pc.predict_change(np.stack(plain[:2]), np.stack(plain[2:]), change['m'], region=region, **change['kw'])
    for g, w_ in zip(got, again):
        assert np.array_equal(g, w_, equal_nan=True)
    dev = torch.from_numpy(np.stack(plain[:2]).view(np.int16)).cuda()      # a resident stack of the caller's is not modified
    keep = dev.clone()
    pc.predict_change(dev.view(torch.uint16) if hasattr(torch, 'uint16') else dev, np.stack(plain[2:]), change['m'], region=region, **change['kw'])
    assert torch.equal(dev, keep)


def test_without_an_area_of_interest_nothing_changes(env, change):
    rt, pc = env['rt'], env['pc']
    paths, m, kw = change['paths'], change['m'], change['kw']
    explicit = pc.predict_change_files(paths[:2], paths[2:], m, aoi=None, **kw)
    grid = rt.union_grid(paths)
    stacks = _aligned(change, grid)
    direct = pc.predict_change(np.stack(stacks[:2]), np.stack(stacks[2:]), m, **kw)
    none = pc.predict_change(np.stack(stacks[:2]), np.stack(stacks[2:]), m, region=None, **kw)
    assert change['plain'][0].max() > 0
    for a, b, c, d in zip(change['plain'], explicit, direct, none):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes() and a.dtype == b.dtype == c.dtype == d.dtype and a.shape == c.shape
