"""GPU checks of raster alignment (csrc/warp.hip satcv_raster_warp; raster_tools.warp, read_warped, read_mosaic, read_aligned_stack;
pc_tools.predict_change_files, prediction_tools.predict_hybrid_raster) against the float64 oracle of tests/warp_oracle.py.

Bounds.  nearest, and every method on the dyadic geometries (an integer shift, exactly aligned 2 : 1 and 1 : 2 grids), are compared
exactly: the oracle evaluates the same float64 expressions in the same order and the kernel is compiled without contraction.  Elsewhere
the float64 value may differ in its last bits (the division, libm), so: float32 output |got - v64| <= 2^-23 S M, with v64 the oracle's
unrounded value, M the largest |valid source sample| and S = 1 (bilinear and average are convex) or 1.5625 (the cubic weight bound) --
twice the half-ulp of the one final rounding; integer output |got - clamp(v64)| <= 0.5 + 1e-9 max(1, |v64|), which is the correct
rounding except on a near-tie.  Validity (NaN, nodata, untouched) is always exact.

Shapes: a 37 x 53 source and a 41 x 67 destination (not a multiple of the wavefront, two workgroups).  A 41 x 67 grid of 3 m pixels spans
12 x 20 pixels of a 10 m source, so it cannot overhang a 37 x 53 source on four sides at once: geometry (i) is run at two placements,
over the top-left and over the bottom-right corner.  float32 sources hold moderate values: the kind does not saturate."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warp_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu

KIND = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3, np.dtype(np.int32): 5}
SH, SW, DH, DW = 37, 53, 41, 67
NODATA = {'uint8': 7, 'uint16': 7, 'int16': -7, 'int32': -7, 'float32': -9999.0}
CANARY = 0xa5
# name -> (su, ou, sv, ov); exact: dyadic arithmetic, every method is compared bit for bit
GEOMETRIES = {
    'up_top_left': (0.3, -2.105, 0.3, -1.805, False),          # (i) 10 m -> 3 m, 0.35 source pixels off, over the top-left corner
    'up_bottom_right': (0.3, 40.105, 0.3, 29.105, False),       # (i) the same over the bottom-right corner
    'down': (10.0, -23.5, 10.0, -13.5, False),                  # (ii) 1 m -> 10 m, 0.35 destination pixels off: 10 x 10 footprints, partly covered
    'shift': (1.0, 7.0, 1.0, -4.0, True),                       # (iii) an integer shift of (-4, +7) pixels
    'south_up': (0.45, 3.3, -0.45, 33.8, False),                # (iv) a south-up source
    'two_to_one': (2.0, 0.0, 2.0, 0.0, True),                   # (v) exactly aligned, 2 : 1
    'one_to_two': (0.5, 0.0, 0.5, 0.0, True),                   # (v) exactly aligned, 1 : 2
}
LAYOUTS = ('hwc', 'chw', 'slot')                                # 'slot': an hwc source into planes 1 .. c of a (c + 2, H, W) destination


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, pc_tools as pc, raster_tools as rt, lstm_tools as lt, _lib
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pt=pt, pc=pc, rt=rt, lt=lt, L=_lib)


def _dev(a):
    a = np.array(a, order='C')                                 # (a copy: the shared sources are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dtype):
    return t.contiguous().view(torch.uint8).cpu().numpy().view(dtype).reshape(tuple(t.shape))


def _same(a, b):
    """two device tensors hold the same bytes (uint16 tensors are compared as bytes)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _full_u16(shape, value):
    return torch.full(shape, value, dtype=torch.int16, device='cuda').view(torch.uint16)


_SOURCES = {}


def source(dtype, c, h=SH, w=SW, seed=0):
    """(h, w, c) of `dtype`: the kind's extremes, 5 % scattered nodata, a 6 x 6 nodata hole, NaNs for float32 (made once per kind)"""
    key = (dtype, c, h, w, seed)
    if key not in _SOURCES:
        rng = np.random.default_rng(seed + 17 * c)
        dt = np.dtype(dtype)
        nd = NODATA[dtype]
        if dt.kind == 'f':
            a = (rng.standard_normal((h, w, c)) * 3000).astype(np.float32)
            a[rng.random(a.shape) < 0.02] = np.nan
        else:
            info = np.iinfo(dt)
            a = rng.integers(info.min, info.max, (h, w, c), dtype=np.int64, endpoint=True)
            ext = rng.random(a.shape)
            a[ext < 0.08] = info.max
            a[ext > 0.92] = info.min
            a[a == nd] = nd + 1
            a = a.astype(dt)
        a[rng.random(a.shape) < 0.05] = nd
        a[h // 2:h // 2 + 6, w // 3:w // 3 + 6] = nd
        a.setflags(write=False)
        _SOURCES[key] = a
    return _SOURCES[key]


def run_warp(env, src, coeff, dst_shape, method, layout='hwc', dst_dtype=None, src_nodata=None, dst_nodata=None, keep=0, src_origin=(0, 0),
             dst_origin=(0, 0), into=None):
    """one satcv_raster_warp launch; src (h, w, c) host array.  -> (result (H, W, c) host array, the whole destination as bytes).  The
    destination is pre-filled with the canary (or `into`, (H, W, c)); 'slot' gives it c + 2 planes, of which 1 .. c are written."""
    L = env['L']
    h, w, c = src.shape
    H, W = dst_shape
    ddt = np.dtype(src.dtype if dst_dtype is None else dst_dtype)
    s = _dev(src if layout != 'chw' else src.transpose(2, 0, 1))
    ld, coff = (c + 2, 1) if layout == 'slot' else (c, 0)
    shape = (H, W, ld) if layout == 'hwc' else (ld, H, W)
    host = np.full(shape, CANARY, np.uint8).repeat(ddt.itemsize, axis=-1).view(ddt) if into is None else None
    if into is not None:
        host = np.ascontiguousarray(into if layout == 'hwc' else into.transpose(2, 0, 1)).astype(ddt)
        assert layout != 'slot'
    d = _dev(host)
    desc = L.WarpDesc(src=s.data_ptr(), src_kind=KIND[src.dtype], src_layout=1 if layout == 'chw' else 0, sh=h, sw=w, src_ld=c, src_coff=0,
                      src_row0=src_origin[0], src_col0=src_origin[1], dst=d.data_ptr(), dst_kind=KIND[ddt], dst_layout=0 if layout == 'hwc' else 1, dh=H, dw=W,
                      dst_ld=ld, dst_coff=coff, dst_row0=dst_origin[0], dst_col0=dst_origin[1], c=c, su=coeff[0], ou=coeff[1], sv=coeff[2], ov=coeff[3],
                      resampling=WO.METHODS.index(method), has_src_nodata=int(src_nodata is not None), src_nodata=float(src_nodata or 0),
                      has_dst_nodata=int(dst_nodata is not None), dst_nodata=float(dst_nodata or 0), keep=keep)
    L.check(L.lib.satcv_raster_warp(C.byref(desc), env['ops'].stream_ptr()))
    torch.cuda.synchronize()
    got = _host(d, ddt)
    res = got if layout == 'hwc' else got[coff:coff + c].transpose(1, 2, 0)
    return res, got


def compare(got, want, v64, src, src_nodata, dst_nodata, method, exact):
    """the bounds of the module docstring; got / want (H, W, c) of the destination kind"""
    ok = ~np.isnan(v64)
    assert ok.any() and (~ok).any()
    if got.dtype.kind == 'f':
        assert np.array_equal(np.isnan(got), ~ok) if dst_nodata is None else np.array_equal(got[~ok], want[~ok])
    else:
        assert np.array_equal(got[~ok], want[~ok]) and (want[~ok] == (0 if dst_nodata is None else dst_nodata)).all()
    if method == 'nearest' or exact:
        assert np.array_equal(got, want, equal_nan=True)
        return
    s64 = src.astype(np.float64)
    valid = ~np.isnan(s64) & (s64 != src_nodata if src_nodata is not None else True)
    M = np.abs(s64[valid]).max()
    S = 1.5625 if method == 'cubic' else 1.0
    g, v = got[ok].astype(np.float64), v64[ok]
    if got.dtype.kind == 'f':
        err, bound = np.abs(g - v), 2.0 ** -23 * S * M
        print(f'    f32 max err {err.max():.3e} (bound {bound:.3e})')
        assert err.max() <= bound
    else:
        info = np.iinfo(got.dtype)
        err = np.abs(g - np.clip(v, info.min, info.max))
        print(f'    int max err {err.max():.6f}')
        assert (err <= 0.5 + 1e-9 * np.maximum(1.0, np.abs(v))).all()


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize('geometry', list(GEOMETRIES))
def test_kernel_equals_the_oracle(env, geometry):
    """every kind (and integer -> float32) x every method on this geometry; the band count (1, 3, 16) and the layout (hwc, chw, hwc into a
    chw slot with ld = c + 2, coff = 1) rotate so that every (band count, layout) pair meets every method and every kind across the
    geometries.  Every byte outside the written channels keeps the canary."""
    *coeff, exact = GEOMETRIES[geometry]
    gi = list(GEOMETRIES).index(geometry)
    kinds = [('uint8', None), ('uint16', None), ('int16', None), ('int32', None), ('float32', None), ('uint16', 'float32'), ('int32', 'float32')]
    seen = set()
    for ki, (dtype, to) in enumerate(kinds):
        for mi, method in enumerate(WO.METHODS):
            n = ki * 4 + mi + gi
            c, layout = (1, 3, 16)[n % 3], LAYOUTS[(n // 3 + mi) % 3]
            seen.add((c, layout))
            src = source(dtype, c)
            nd = NODATA[dtype]
            ddt = np.dtype(to or dtype)
            dst_nd = None if ddt.kind == 'f' and n % 2 else (nd if ddt.kind != 'f' or to is None else -1.0)
            print(f'{geometry} {dtype}->{ddt} {method} c={c} {layout}')
            want, v64 = WO.warp_ref(src, *coeff, (DH, DW), method, src_nodata=nd, dst_nodata=dst_nd, dst_dtype=ddt)
            got, whole = run_warp(env, src, coeff, (DH, DW), method, layout, ddt, nd, dst_nd)
            compare(got, want, v64, src, nd, dst_nd, method, exact)
            if layout == 'slot':
                assert (whole[[0, -1]].view(np.uint8) == CANARY).all()
    assert len(seen) >= 6


def test_vector_and_scalar_band_paths_agree(env):
    """c = 4 and c = 2 travel as one load and one store per pixel where ld, coff and the address allow; a destination with ld = c + 1, a
    source read at an odd channel offset and keep with partly valid pixels take the sample-by-sample path: the same numbers"""
    L, coeff = env['L'], GEOMETRIES['up_top_left'][:4]
    for c in (4, 2):
        src = source('uint16', c)
        for method in ('bilinear', 'average'):
            want, v64 = WO.warp_ref(src, *coeff, (DH, DW), method, src_nodata=7, dst_nodata=7)
            got, _ = run_warp(env, src, coeff, (DH, DW), method, 'hwc', None, 7, 7)
            compare(got, want, v64, src, 7, 7, method, False)
            # the same through a wide source (ld = c + 1, coff = 1) into a wide destination (ld = c + 1, coff = 1), with keep
            wide = np.concatenate([np.full((SH, SW, 1), 9, np.uint16), src], axis=2)
            s, d = _dev(wide), torch.full((DH, DW, c + 1), 0x5a5a, dtype=torch.int16, device='cuda')
            desc = L.WarpDesc(src=s.data_ptr(), src_kind=1, src_layout=0, sh=SH, sw=SW, src_ld=c + 1, src_coff=1, src_row0=0, src_col0=0, dst=d.data_ptr(),
                              dst_kind=1, dst_layout=0, dh=DH, dw=DW, dst_ld=c + 1, dst_coff=1, dst_row0=0, dst_col0=0, c=c, su=coeff[0], ou=coeff[1],
                              sv=coeff[2], ov=coeff[3], resampling=WO.METHODS.index(method), has_src_nodata=1, src_nodata=7.0, has_dst_nodata=1,
                              dst_nodata=7.0, keep=1)
            L.check(L.lib.satcv_raster_warp(C.byref(desc), env['ops'].stream_ptr()))
            torch.cuda.synchronize()
            kept = _host(d, np.uint16)
            assert (kept[..., 0] == 0x5a5a).all()
            ok = ~np.isnan(v64)
            assert np.array_equal(kept[..., 1:][ok], got[ok]) and (kept[..., 1:][~ok] == 0x5a5a).all()


# ---------------------------------------------------------------------------------------------------------------- 2. windows and strips
@pytest.mark.parametrize('method', ['cubic', 'average'])
@pytest.mark.parametrize('geometry', ['up_top_left', 'down'])
def test_window_and_strips_equal_the_one_call_result(env, geometry, method):
    """the destination in three row strips (dst_row0), each from the window of the source that `warp_window` names for the strip
    (src_row0 / src_col0): bit for bit the one-call result"""
    rt = env['rt']
    su, ou, sv, ov, _ = GEOMETRIES[geometry]
    src = source('int16', 3)
    full, _ = run_warp(env, src, (su, ou, sv, ov), (DH, DW), method, 'hwc', np.float32, -7, None)
    src_t = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)                    # source pixel coordinates as map coordinates: the grid transform is the coefficients
    windows = []
    for r0, r1 in ((0, 2), (2, 3), (3, DH)):
        strip = rt.Grid((su, 0.0, ou, 0.0, sv, sv * r0 + ov), (r1 - r0, DW))
        win = rt.warp_window(src_t, (SH, SW), strip, method)
        if win is None:
            assert np.isnan(full[r0:r1]).all()
            continue
        y, x, h, w = win
        windows.append(win)
        part, _ = run_warp(env, np.ascontiguousarray(src[y:y + h, x:x + w]), (su, ou, sv, ov), (r1 - r0, DW), method, 'hwc', np.float32, -7, None,
                           src_origin=(y, x), dst_origin=(r0, 0))
        assert np.array_equal(part, full[r0:r1], equal_nan=True), (r0, r1)
    assert windows and any(w[2] < SH for w in windows)


# ---------------------------------------------------------------------------------------------------------------- 3. keep
@pytest.mark.parametrize('method', ['nearest', 'bilinear'])
def test_keep_builds_a_mosaic(env, method):
    a, b = source('uint16', 3, seed=1), source('uint16', 3, seed=2)
    ca, cb = (0.8, -3.3, 0.8, -2.1), (0.8, -30.3, 0.8, -12.1)  # b lies 27 x 10 source pixels further right / down: the two overlap in the middle
    fill = np.full((DH, DW, 3), 7, np.uint16)
    step, va = WO.warp_ref(a, *ca, (DH, DW), method, src_nodata=7, keep_into=fill)
    want, vb = WO.warp_ref(b, *cb, (DH, DW), method, src_nodata=7, keep_into=step)
    got1, _ = run_warp(env, a, ca, (DH, DW), method, 'hwc', None, 7, None, keep=1, into=fill)
    got, _ = run_warp(env, b, cb, (DH, DW), method, 'hwc', None, 7, None, keep=1, into=got1)
    both, none = ~np.isnan(va) & ~np.isnan(vb), np.isnan(va) & np.isnan(vb)
    assert both.any() and none.any() and (got[none] == 7).all()
    if method == 'nearest':
        assert np.array_equal(got1, step) and np.array_equal(got, want)
    else:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1 and (got != want).mean() < 1e-3
        assert np.array_equal(got == 7, want == 7)


# ---------------------------------------------------------------------------------------------------------------- 4. the readers
T10 = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
FH, FW = 64, 96


def _write(env, path, arr, transform, nodata=7, overviews='auto', resampling='nearest'):
    return env['rt'].write_cog(arr, str(path), transform, 'EPSG:32633', nodata=nodata, blocksize=16, compress='lzw', overviews=overviews,
                               resampling=resampling)


@pytest.fixture(scope='module')
def files(env, tmp_path_factory):
    """three uint16 files of 64 x 96 x 3 on three grids: 10 m; 10 m shifted by 3 pixels in both directions (another extent); 20 m"""
    d = tmp_path_factory.mktemp('warp')
    arrs = [source('uint16', 3, FH, FW, seed=s) for s in (3, 4, 5)]
    ts = [T10, (10.0, 0.0, T10[2] + 30.0, 0.0, -10.0, T10[5] - 30.0), (20.0, 0.0, T10[2] - 40.0, 0.0, -20.0, T10[5] + 60.0)]
    paths = [_write(env, d / f'f{k}.tif', a, t) for k, (a, t) in enumerate(zip(arrs, ts))]
    return dict(paths=paths, arrs=arrs, ts=ts, dir=d)


@pytest.mark.parametrize('method', WO.METHODS)
def test_read_warped_equals_warping_the_whole_file(env, files, method):
    rt = env['rt']
    grid = rt.Grid((4.0, 0.0, T10[2] + 101.0, 0.0, -4.0, T10[5] - 77.0), (50, 70), 'EPSG:32633')       # inside the file: a window is read
    assert rt.warp_window(T10, (FH, FW), grid, method)[2] < FH
    if method == 'average':
        grid = rt.Grid((25.0, 0.0, T10[2] + 95.0, 0.0, -25.0, T10[5] - 55.0), (30, 40), 'EPSG:32633')  # coarser, overhanging right and below
    whole = rt.read_cog(files['paths'][0])
    want = rt.warp(whole.array, whole.transform, grid, method, src_nodata=7)
    r = rt.read_warped(files['paths'][0], grid, resampling=method)
    assert r.transform == grid.transform and r.crs == 'EPSG:32633' and r.nodata == 7 and r.dtype == 'uint16'
    assert r.array.shape == grid.shape + (3,) and _same(r.array, want)
    ref, _ = WO.warp_between(files['arrs'][0], T10, grid.transform, grid.shape, method, src_nodata=7, dst_nodata=7)
    got = _host(r.array, np.uint16)
    assert np.abs(got.astype(np.int64) - ref.astype(np.int64)).max() <= (0 if method == 'nearest' else 1) and (got != ref).mean() < 1e-3
    # bands, layout, float32 output, a channel range of a wider scene
    sub = rt.read_warped(files['paths'][0], grid, bands=[2, 0], resampling=method, layout='chw', dtype='float32', nodata=-1.0)
    assert sub.array.shape == (2,) + grid.shape and sub.dtype == 'float32' and sub.nodata == -1.0
    f32 = sub.array.cpu().numpy()
    fref, _ = WO.warp_between(files['arrs'][0][..., [2, 0]], T10, grid.transform, grid.shape, method, src_nodata=7, dst_nodata=-1.0, dst_dtype=np.float32)
    assert np.array_equal(f32 == -1.0, fref.transpose(2, 0, 1) == -1.0) and np.allclose(f32, fref.transpose(2, 0, 1), rtol=0, atol=2.0 ** -23 * 1.5625 * 65535)
    scene = _full_u16(grid.shape + (6,), 0x1111)
    rt.read_warped(files['paths'][0], grid, resampling=method, out=scene, channel_offset=2)
    assert _same(scene[..., 2:5], want) and (_host(scene, np.uint16)[..., [0, 1, 5]] == 0x1111).all()


def test_read_warped_beside_the_file_reads_nothing(env, files, monkeypatch):
    rt = env['rt']
    monkeypatch.setattr(rt, 'read_cog', lambda *a, **k: pytest.fail('nothing is to be read'))
    away = rt.Grid((10.0, 0.0, T10[2] + 5000.0, 0.0, -10.0, T10[5]), (8, 9), 'EPSG:32633')
    r = rt.read_warped(files['paths'][0], away)
    assert r.array.shape == (8, 9, 3) and (_host(r.array, np.uint16) == 7).all()
    kept = _full_u16((3, 8, 9), 5)
    rt.read_warped(files['paths'][0], away, layout='chw', out=kept, keep=True)
    assert (_host(kept, np.uint16) == 5).all()
    rt.read_warped(files['paths'][0], away, layout='chw', out=kept)
    assert (_host(kept, np.uint16) == 7).all()


def test_level_auto_reads_the_overview(env, files):
    rt = env['rt']
    grid = rt.Grid((20.0, 0.0, T10[2] + 40.0, 0.0, -20.0, T10[5] - 20.0), (24, 40), 'EPSG:32633')     # 2x coarser
    lvl1 = rt.read_cog(files['paths'][0], level=1)
    assert lvl1.transform[0] == 20.0
    for method in ('nearest', 'bilinear'):
        want = rt.warp(lvl1.array, lvl1.transform, grid, method, src_nodata=7)
        got = rt.read_warped(files['paths'][0], grid, resampling=method, level='auto')
        assert _same(got.array, want)
        assert _same(rt.read_warped(files['paths'][0], grid, resampling=method, level=1).array, want)
    assert not _same(rt.read_warped(files['paths'][0], grid, resampling='bilinear').array, want)       # level 0, the default, is another raster


@pytest.mark.parametrize('first', [False, True])
def test_read_mosaic_of_two_overlapping_tiles(env, files, first):
    rt = env['rt']
    paths, arrs, ts = files['paths'][:2], files['arrs'][:2], files['ts'][:2]
    r = rt.read_mosaic(paths, first=first)
    grid = rt.union_grid(paths)
    assert grid.shape == (FH + 3, FW + 3) and r.transform == grid.transform and r.crs == 'EPSG:32633' and r.nodata == 7
    want = np.full(grid.shape + (3,), 7, np.uint16)
    order = [1, 0] if first else [0, 1]
    for k in order:
        want, _ = WO.warp_between(arrs[k], ts[k], grid.transform, grid.shape, 'nearest', src_nodata=7, keep_into=want)
    got = _host(r.array, np.uint16)
    assert np.array_equal(got, want) and (got[:3, FW:] == 7).all()
    assert not np.array_equal(got, _host(rt.read_mosaic(paths, first=not first).array, np.uint16))      # the order matters where both have data


def test_read_aligned_stack(env, files):
    rt, pc = env['rt'], env['pc']
    stack, transform, crs, nodata = rt.read_aligned_stack(files['paths'], resampling='nearest')
    grid = rt.union_grid(files['paths'])
    assert grid.resolution == (10.0, 10.0) and transform == grid.transform and crs == 'EPSG:32633' and nodata == 7
    assert tuple(stack.shape) == (3, 3) + grid.shape and stack.dtype == torch.uint16
    got = _host(stack, np.uint16)
    for t in range(3):
        want, _ = WO.warp_between(files['arrs'][t], files['ts'][t], grid.transform, grid.shape, 'nearest', src_nodata=7, dst_nodata=7)
        assert np.array_equal(got[t], want.transpose(2, 0, 1)), t
    median, norm = pc.median_composite(stack)                   # the stack is what the composite takes
    assert tuple(median.shape) == grid.shape + (3,) and torch.isfinite(norm).any()
    # an acquisition of two tiles, bilinear, on a given 20 m grid
    g20 = rt.union_grid(files['paths'], resolution=20)
    st2 = rt.read_aligned_stack([files['paths'][:2], files['paths'][2]], grid=g20, resampling='bilinear')[0]
    assert tuple(st2.shape) == (2, 3) + g20.shape
    mosaic = rt.read_mosaic(files['paths'][:2], grid=g20, resampling='bilinear', layout='chw')
    assert _same(st2[0], mosaic.array)
    assert _same(st2[1], rt.read_warped(files['paths'][2], g20, resampling='bilinear', layout='chw').array)


def test_read_aligned_stack_on_one_grid_equals_read_stack(env, files):
    rt = env['rt']
    paths = [files['paths'][0]] + [_write(env, files['dir'] / f'same{k}.tif', source('uint16', 3, FH, FW, seed=9 + k), T10) for k in range(2)]
    want = rt.read_stack(paths)
    got = rt.read_aligned_stack(paths)
    assert _same(got[0], want[0]) and got[1:] == want[1:]
    sub = rt.read_aligned_stack(paths, bands=[1])
    assert _same(sub[0], rt.read_stack(paths, bands=[1])[0])


# ---------------------------------------------------------------------------------------------------------------- 5. the drivers
def test_predict_hybrid_raster_equals_the_scene_predictor_on_aligned_inputs(env, tmp_path):
    """the smallest hybrid case of tests/hybrid_scene_cases.py (r = 6): the scene as a 1 m file, the series as 6 m files on grids that differ
    from the coarse grid by whole pixels and extent.  nearest copies samples, inference is deterministic: bit for bit."""
    import hybrid_scene_cases as HC
    rt, pt = env['rt'], env['pt']
    HY = HC.HYBRID
    m = HC.hybrid_model(env['lt'], env['mt'], 'bfloat16')
    scene, stack = HC.hybrid_scene('reference')
    H, W = HY['reference']['hi']
    h, w = HY['reference']['lo']
    t1 = (1.0, 0.0, 500000.0, 0.0, -1.0, 4100000.0)
    scene_file = _write(env, tmp_path / 'scene.tif', scene, t1, nodata=None)
    items = []
    for t in range(HY['T']):
        oy, ox = 2 + t, 3 - t                                   # every acquisition on its own, larger grid: the scene's extent starts at (oy, ox)
        big = np.full((h + 5, w + 6, HY['c']), -32768, np.int16)
        big[oy:oy + h, ox:ox + w] = stack[t].transpose(1, 2, 0)
        items.append(_write(env, tmp_path / f't{t}.tif', big, (6.0, 0.0, t1[2] - 6.0 * ox, 0.0, -6.0, t1[5] + 6.0 * oy), nodata=-32768))
    kw = dict(kernel=HY['kernel'], buff=HY['buff'], batch_size=HY['batch'], rescale=HC.RESCALE, maxval=HC.MAXVAL)
    out_file = str(tmp_path / 'map.tif')
    res = pt.predict_hybrid_raster(scene_file, items, m, out_file, channel=None, **kw)
    want = pt.predict_hybrid_scene(scene, stack[:HY['T']], m, channel=None, **kw)
    assert np.ptp(want) > 0 and np.array_equal(res.cpu().numpy(), want)
    back = rt.read_cog(out_file)
    assert back.transform == t1 and back.crs == 'EPSG:32633' and np.array_equal(back.array.cpu().numpy(), want)
    # a window of the scene: its own transform, the coarse grid follows
    win = (HY['kernel'], 0, H - HY['kernel'], W)
    res = pt.predict_hybrid_raster(scene_file, items, m, out_file, window=win, channel=None, **kw)
    want = pt.predict_hybrid_scene(scene[win[0]:], stack[:HY['T'], :, win[0] // HY['r']:], m, channel=None, **kw)
    assert np.array_equal(res.cpu().numpy(), want) and rt.read_cog(out_file).transform == (1.0, 0.0, t1[2], 0.0, -1.0, t1[5] - win[0])
    with pytest.raises(ValueError, match='trim_array'):
        pt.predict_hybrid_raster(scene_file, items, m, out_file, window=(0, 0, H - 1, W), **kw)


def test_predict_change_files_equals_predict_change_on_aligned_stacks(env, tmp_path):
    rt, pc, mt = env['rt'], env['pc'], env['mt']
    mt.reset_uids(); mt.set_seed(6)
    m = mt.get_unet_model(2, 6, filters=[32, 64], factors=[2, 2])
    m.compute_dtype = 'bfloat16'
    rng = np.random.default_rng(8)
    arrs, ts, paths = [], [], []
    for k in range(4):                                          # 10 m, 10 m shifted with another extent, 20 m, 10 m
        res = 20.0 if k == 2 else 10.0
        shape = (40, 52) if k == 2 else (70 + k, 90 - k)
        a = rng.integers(1, 9000, shape + (3,)).astype(np.uint16)
        a[5:9, 7:12] = 0
        t = (res, 0.0, T10[2] + 10.0 * k, 0.0, -res, T10[5] - 20.0 * k)
        arrs.append(a); ts.append(t)
        paths.append(_write(env, tmp_path / f'c{k}.tif', a, t, nodata=0, overviews=0))
    kw = dict(kernel=32, buff=16, batch_size=4, fill=0.0)
    out_file = str(tmp_path / 'change.tif')
    got = pc.predict_change_files(paths[:2], paths[2:], m, out_file=out_file, **kw)
    grid = rt.union_grid(paths)
    aligned = [WO.warp_between(a, t, grid.transform, grid.shape, 'nearest', src_nodata=0, dst_nodata=0)[0].transpose(2, 0, 1) for a, t in zip(arrs, ts)]
    want = pc.predict_change(np.stack(aligned[:2]), np.stack(aligned[2:]), m, **kw)
    assert want[0].max() > 0
    for g, w_ in zip(got, want):
        assert np.array_equal(g, w_, equal_nan=True)
    back = rt.read_cog(out_file)
    assert back.transform == grid.transform and back.crs == 'EPSG:32633' and np.array_equal(back.array.cpu().numpy()[..., 0], want[0])


def test_each_file_is_parsed_once(env, tmp_path, monkeypatch):
    """Within one call of read_aligned_stack, read_mosaic, read_warped and read_stack the container of every file is parsed exactly once
    (`read_info`, counted where raster_tools looks it up), and the result is, bit for bit, what the uncounted call returns.  Three
    48 x 40 two-band uint16 files with overlapping footprints: a and b on one 10 m grid, c at 20 m; a2 is a copy of a; d lies in the
    neighbouring UTM zone."""
    import shutil
    rt = env['rt']
    x, y = rt.transform_points([-78.0], [40.0], 4326, 32617)
    x0, y0 = round(float(x[0]) / 20) * 20.0, round(float(y[0]) / 20) * 20.0
    xd, yd = rt.transform_points([x0 + 150.0], [y0 - 90.0], 32617, 32618)
    placed = {'a': ((10.0, 0.0, x0, 0.0, -10.0, y0), 32617), 'b': ((10.0, 0.0, x0 + 200.0, 0.0, -10.0, y0 - 100.0), 32617),
              'c': ((20.0, 0.0, x0 - 100.0, 0.0, -20.0, y0 + 60.0), 32617),
              'd': ((10.0, 0.0, round(float(xd[0])), 0.0, -10.0, round(float(yd[0]))), 32618)}
    p = {k: rt.write_cog(source('uint16', 2, 48, 40, seed=i), str(tmp_path / f'{k}.tif'), t, code, nodata=7, blocksize=16)
         for i, (k, (t, code)) in enumerate(placed.items())}
    p['a2'] = shutil.copy(p['a'], str(tmp_path / 'a2.tif'))
    grid = rt.Grid((10.0, 0.0, x0 + 50.0, 0.0, -10.0, y0 - 30.0), (33, 29), 32617)
    cases = {'aligned stack': (lambda: rt.read_aligned_stack([p['a'], [p['b'], p['c']]])[0], 'abc'),
             'mosaic': (lambda: rt.read_mosaic([p['a'], p['b'], p['c']]).array, 'abc'),
             'warped': (lambda: rt.read_warped(p['a'], grid).array, 'a'),
             'stack': (lambda: rt.read_stack([p['a'], p['a2']])[0], ['a', 'a2']),
             'two-zone mosaic': (lambda: rt.read_mosaic([p['a'], p['b'], p['d']], reproject=True).array, 'abd')}
    want = {name: call() for name, (call, _) in cases.items()}
    parsed = []
    read_info = rt.read_info
    monkeypatch.setattr(rt, 'read_info', lambda path: (parsed.append(str(path)), read_info(path))[1])
    for name, (call, files) in cases.items():
        parsed.clear()
        got = call()
        assert sorted(parsed) == sorted(p[k] for k in files), (name, parsed)
        assert _same(got, want[name]), name
    assert (_host(want['two-zone mosaic'], np.uint16) != 7).all(axis=2).any() and want['aligned stack'].shape[:2] == (2, 2)
