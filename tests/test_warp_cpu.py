"""Raster alignment without a GPU: the float64 oracle of tests/warp_oracle.py against independent definitions (scipy.ndimage where they
coincide, block means, a linear ramp, plain indexing), the host grid arithmetic of raster_tools (Grid, union_grid, warp_window,
auto_level), every refusal, and the C ABI of satcv_raster_warp (descriptor layout, refusals before any launch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import warp_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _image(h=23, w=31, c=2, seed=0):
    return np.random.default_rng(seed).random((h, w, c)) * 100.0


# ------------------------------------------------------------------------------------------------------------ the rules
def test_bilinear_agrees_with_scipy_where_both_are_defined():
    """map_coordinates(order=1, mode='constant', cval=nan) in pixel-centre coordinates (u - 0.5): the same convex combination wherever
    all four taps are inside; in the half-pixel rim scipy yields NaN while the rule here renormalises over the taps inside."""
    from scipy import ndimage
    src = _image()
    su, ou, sv, ov = 0.37, 2.2, 0.41, 1.3
    H, W = 40, 50
    _, v64 = wo.warp_ref(src, su, ou, sv, ov, (H, W), 'bilinear', dst_dtype=np.float32)
    u = su * (np.arange(W) + 0.5) + ou
    v = sv * (np.arange(H) + 0.5) + ov
    vv, uu = np.meshgrid(v - 0.5, u - 0.5, indexing='ij')
    both = 0
    for b in range(src.shape[2]):
        ref = ndimage.map_coordinates(src[..., b], [vv, uu], order=1, mode='constant', cval=np.nan)
        ok = ~np.isnan(ref)
        assert not np.isnan(v64[..., b][ok]).any()
        assert np.abs(v64[..., b][ok] - ref[ok]).max() <= 1e-12 * 100
        both += int(ok.sum())
    assert both > 0.8 * H * W * src.shape[2]
    # the rim: inside the image by less than half a pixel -> defined here, NaN there
    _, edge = wo.warp_ref(src, 1.0, -0.25, 1.0, 0.0, (4, 4), 'bilinear', dst_dtype=np.float32)
    assert not np.isnan(edge[:, 0]).any() and np.array_equal(edge[0, 0], src[0, 0])


def test_nearest_is_plain_indexing():
    src = _image()
    su, ou, sv, ov = 0.3, 1.05, -0.3, 9.2          # a south-up source
    H, W = 25, 60
    res, _ = wo.warp_ref(src, su, ou, sv, ov, (H, W), 'nearest')
    for i in range(H):
        for j in range(W):
            y, x = int(np.floor(sv * (i + 0.5) + ov)), int(np.floor(su * (j + 0.5) + ou))
            inside = 0 <= y < src.shape[0] and 0 <= x < src.shape[1]
            assert np.array_equal(res[i, j], src[y, x]) if inside else np.isnan(res[i, j]).all()


@pytest.mark.parametrize('k', [2, 3, 10])
def test_average_at_an_integer_ratio_is_the_block_mean(k):
    src = np.random.default_rng(k).integers(0, 60000, (6 * k, 5 * k, 2)).astype(np.uint16)
    res, v64 = wo.warp_ref(src, float(k), 0.0, float(k), 0.0, (6, 5), 'average')
    blocks = src.reshape(6, k, 5, k, 2).astype(np.float64).sum(axis=(1, 3)) / (k * k)
    assert np.array_equal(v64, blocks)
    assert np.array_equal(res, np.rint(blocks).astype(np.uint16))


def test_average_skips_nodata_and_weights_partial_overlap():
    src = np.array([[1.0, 3.0, 5.0, 7.0]]).reshape(1, 4, 1)
    # footprint [0.5, 2.5) of one destination pixel: half of pixel 0, all of pixel 1, half of pixel 2
    _, v64 = wo.warp_ref(src, 2.0, 0.5, 1.0, 0.0, (1, 1), 'average', dst_dtype=np.float32)
    assert v64[0, 0, 0] == (0.5 * 1 + 1.0 * 3 + 0.5 * 5) / 2.0
    _, v64 = wo.warp_ref(src, 2.0, 0.5, 1.0, 0.0, (1, 1), 'average', src_nodata=3.0, dst_dtype=np.float32)
    assert v64[0, 0, 0] == (0.5 * 1 + 0.5 * 5) / 1.0
    _, v64 = wo.warp_ref(src, 2.0, 4.0, 1.0, 0.0, (1, 1), 'average', dst_dtype=np.float32)      # beside the raster: no weight
    assert np.isnan(v64).all()


def test_cubic_reproduces_a_linear_ramp_and_falls_back_to_bilinear():
    yy, xx = np.mgrid[0:20, 0:24].astype(np.float64)
    src = (3.0 * xx - 2.0 * yy + 5.0)[..., None]
    su, ou, sv, ov = 0.45, 3.1, 0.6, 2.7
    H, W = 20, 36
    _, v64 = wo.warp_ref(src, su, ou, sv, ov, (H, W), 'cubic', dst_dtype=np.float32)
    u = su * (np.arange(W) + 0.5) + ou
    v = sv * (np.arange(H) + 0.5) + ov
    want = 3.0 * (u[None, :] - 0.5) - 2.0 * (v[:, None] - 0.5) + 5.0
    assert np.abs(v64[..., 0] - want).max() <= 1e-9
    # a hole: every sample whose 16 taps touch it takes the bilinear rule, a sample inside it is invalid
    holed = src.copy()
    holed[8:11, 10:13] = np.nan
    _, c64 = wo.warp_ref(holed, su, ou, sv, ov, (H, W), 'cubic', dst_dtype=np.float32)
    _, b64 = wo.warp_ref(holed, su, ou, sv, ov, (H, W), 'bilinear', dst_dtype=np.float32)
    touched = c64 != v64
    assert touched.any() and np.array_equal(c64[touched], b64[touched], equal_nan=True) and np.isnan(c64).any()


def test_cubic_weights_sum_to_one_and_stay_below_the_bound():
    t = np.linspace(0.0, 1.0, 100001)
    w = np.array(wo.cubic_weights(t))
    assert np.abs(w.sum(axis=0) - 1.0).max() <= 1e-15
    assert np.abs(w).sum(axis=0).max() <= 1.25 + 1e-12         # per axis; 1.25^2 = 1.5625 for the 16 taps
    assert (np.abs(w).sum(axis=0).max()) ** 2 <= 1.5625 + 1e-12
    assert [float(x) for x in wo.cubic_weights(0.0)] == [0.0, 1.0, 0.0, 0.0]
    # the rejected alternative, a renormalised partial stencil: with only the containing tap and the negative lobes valid (t = 0.5 in both
    # axes) the weight sum is 0.5625^2 - 8 * 0.0625 * 0.5625 = 0.035, a 28-fold amplification
    w = np.outer(wo.cubic_weights(0.5), wo.cubic_weights(0.5))
    assert w[1, 1] + w[w < 0].sum() == 0.03515625


@pytest.mark.parametrize('method', wo.METHODS)
def test_an_integer_pixel_shift_is_a_copy(method):
    src = np.random.default_rng(3).integers(-30000, 30000, (12, 14, 3)).astype(np.int16)
    src[4, 5] = -32768
    res, _ = wo.warp_ref(src, 1.0, 7.0, 1.0, -4.0, (12, 14), method, dst_nodata=-1)
    want = np.full_like(src, -1)
    want[4:, :7] = src[:8, 7:]
    assert np.array_equal(res, want)


def test_window_and_strips_do_not_change_the_oracle():
    src = _image(30, 30, 1, seed=5)
    full, _ = wo.warp_ref(src, 0.31, 4.2, 0.29, 3.3, (50, 50), 'cubic', dst_dtype=np.float32)
    part, _ = wo.warp_ref(src[2:25, 3:27], 0.31, 4.2, 0.29, 3.3, (20, 50), 'cubic', dst_dtype=np.float32, src_origin=(2, 3), dst_origin=(10, 0))
    # rows 10 .. 29 need the source rows floor(0.29 * 10.5 + 3.3 - 0.5) - 1 = 4 .. floor(0.29 * 29.5 + 3.3 - 0.5) + 2 = 13
    assert np.array_equal(part[:, 2:-2], full[10:30, 2:-2], equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ grids
def test_grid_is_an_immutable_value():
    from satellite_computervision_amd import raster_tools as rt
    g = rt.Grid((10, 0, 600000, 0, -10, 5000000), (30, 40), 32633)
    assert g.shape == (30, 40) and g.crs == 'EPSG:32633' and g.resolution == (10.0, 10.0)
    assert g.bounds == (600000.0, 4999700.0, 600400.0, 5000000.0)
    assert g == rt.Grid((10.0, 0.0, 600000.0, 0.0, -10.0, 5000000.0), (30, 40), 'EPSG:32633') and hash(g) == hash(tuple(g))
    with pytest.raises(AttributeError):
        g.shape = (1, 1)
    south_up = rt.Grid((10, 0, 0, 0, 10, 100), (5, 5))
    assert south_up.bounds == (0.0, 100.0, 50.0, 150.0) and south_up.crs is None
    for bad in ((0, 0, 0, 0, -1, 0), (1, 0, 0, 0, float('nan'), 0)):
        with pytest.raises(ValueError, match='pixel size'):
            rt.Grid(bad, (1, 1))
    with pytest.raises(ValueError, match='positive integers'):
        rt.Grid((1, 0, 0, 0, -1, 0), (0, 4))


def test_union_grid_snaps_outward_to_multiples_of_the_resolution():
    from satellite_computervision_amd import raster_tools as rt
    a = rt.Grid((10, 0, 600005, 0, -10, 5000003), (10, 10), 32633)            # x 600005 .. 600105, y 4999903 .. 5000003
    g = rt.union_grid([a])
    assert g.transform == (10.0, 0.0, 600000.0, 0.0, -10.0, 5000010.0) and g.shape == (11, 11) and g.crs == 'EPSG:32633'
    b = rt.Grid((20, 0, 600100, 0, -20, 5000100), (4, 3), 32633)              # x 600100 .. 600160, y 5000020 .. 5000100
    g = rt.union_grid([a, b])                                                 # finest resolution, union of the bounds
    assert g.resolution == (10.0, 10.0) and g.bounds == (600000.0, 4999900.0, 600160.0, 5000100.0) and g.shape == (20, 16)
    g = rt.union_grid([a, b], resolution=60)
    assert g.bounds == (600000.0, 4999860.0, 600180.0, 5000100.0) and g.shape == (4, 3)      # 600005 / 60 = 10000.08, 4999903 / 60 = 83331.7
    g = rt.union_grid([a], resolution=(2.5, 5), bounds=(600001, 4999991, 600011, 5000001))
    assert g.transform == (2.5, 0.0, 600000.0, 0.0, -5.0, 5000005.0) and g.shape == (3, 5)
    g = rt.union_grid([], resolution=1, bounds=(0.2, 0.2, 3.5, 2.0), crs='EPSG:4326')
    assert g.bounds == (0.0, 0.0, 4.0, 2.0) and g.shape == (2, 4) and g.crs == 'EPSG:4326'
    south_up = rt.Grid((10, 0, 600000, 0, 10, 4999900), (10, 10))             # a south-up source: the union is north-up
    assert rt.union_grid([south_up]).transform == (10.0, 0.0, 600000.0, 0.0, -10.0, 5000000.0)
    info = rt.LevelInfo()
    info.index, info.shape, info.transform, info.epsg = 0, (10, 10), a.transform, 32633
    assert rt.union_grid([info]) == rt.union_grid([a])


def test_warp_window_margin_clipping_and_empty_intersection():
    from satellite_computervision_amd import raster_tools as rt
    src_t, shape = (10, 0, 1000, 0, -10, 2000), (100, 120)
    g = rt.Grid((10, 0, 1200, 0, -10, 1800), (30, 40))                       # rows 20 .. 49, columns 20 .. 59 of the source, aligned
    assert rt.warp_window(src_t, shape, g, 'nearest') == (20, 20, 30, 40)
    assert rt.warp_window(src_t, shape, g, 'bilinear') == (19, 19, 32, 42)
    assert rt.warp_window(src_t, shape, g, 'cubic') == (18, 18, 34, 44)
    assert rt.warp_window(src_t, shape, g, 'average') == (20, 20, 30, 40)
    half = rt.Grid((10, 0, 1205, 0, -10, 1795), (30, 40))                    # shifted by half a pixel: the footprint touches one more
    assert rt.warp_window(src_t, shape, half, 'average') == (20, 20, 31, 41)
    assert rt.warp_window(src_t, shape, half, 'nearest') == (21, 21, 30, 40)
    coarse = rt.Grid((30, 0, 1000, 0, -30, 2000), (10, 10))
    assert rt.warp_window(src_t, shape, coarse, 'average') == (0, 0, 30, 30)
    assert rt.warp_window(src_t, shape, coarse, 'nearest') == (1, 1, 28, 28)
    over = rt.Grid((10, 0, 980, 0, -10, 2020), (200, 200))                   # overhangs on every side: clipped to the raster
    for m in wo.METHODS:
        assert rt.warp_window(src_t, shape, over, m) == (0, 0, 100, 120)
    corner = rt.Grid((10, 0, 2190, 0, -10, 1010), (5, 5))                    # only the last pixel of the raster under the first of the grid
    assert rt.warp_window(src_t, shape, corner, 'nearest') == (99, 119, 1, 1)
    assert rt.warp_window(src_t, shape, corner, 'cubic') == (97, 117, 3, 3)
    for t in ((10, 0, 2200, 0, -10, 2000), (10, 0, 1000, 0, -10, 3000), (10, 0, 0, 0, -10, 2000)):
        assert rt.warp_window(src_t, shape, rt.Grid(t, (50, 50)), 'nearest') is None
    beside = rt.Grid((10, 0, 2200, 0, -10, 2000), (50, 50))                  # touches the edge: cubic's margin reaches in, the samples are still invalid
    assert rt.warp_window(src_t, shape, beside, 'cubic') == (0, 118, 52, 2)
    south_up = (10, 0, 1000, 0, 10, 1000)                                    # the same extent stored bottom row first
    assert rt.warp_window(south_up, shape, g, 'nearest') == (50, 20, 30, 40)


def test_auto_level_takes_the_coarsest_level_that_is_fine_enough():
    from satellite_computervision_amd import raster_tools as rt
    ts = [(10 * 2 ** k, 0, 0, 0, -10 * 2 ** k, 0) for k in range(4)]         # 10, 20, 40, 80 m
    at = lambda r: rt.auto_level(ts, rt.Grid((r[0], 0, 0, 0, -r[1], 0), (4, 4)))
    assert at((10, 10)) == 0 and at((20, 20)) == 1 and at((39, 39)) == 1 and at((40, 40)) == 2 and at((1000, 1000)) == 3
    assert at((5, 5)) == 0                                                   # finer than the image: the image
    assert at((80, 20)) == 1                                                 # either axis limits
    odd = [(10, 0, 0, 0, -10, 0), (10 * 65 / 33, 0, 0, 0, -10 * 65 / 33, 0)]  # the overview of an odd-sized image is a little finer than 2x
    assert rt.auto_level(odd, rt.Grid((20, 0, 0, 0, -20, 0), (4, 4))) == 1


# ------------------------------------------------------------------------------------------------------------ refusals
def _tiny_file(path, transform, crs):
    from satellite_computervision_amd import raster_tools as rt
    return rt.write_tiles(str(path), [(16, 16)], [[bytes(range(256))]], 'uint8', 1, 16, None, False, 255, transform, crs)


def test_value_errors_name_the_cause(tmp_path):
    from satellite_computervision_amd import raster_tools as rt
    north = (10, 0, 0, 0, -10, 160)
    a = _tiny_file(tmp_path / 'a.tif', north, 32633)
    b = _tiny_file(tmp_path / 'b.tif', north, 32634)
    rot = _tiny_file(tmp_path / 'rot.tif', (10, 1, 0, 0, -10, 160), 32633)
    g = rt.Grid(north, (16, 16), 32633)
    with pytest.raises(ValueError, match='rotated or sheared'):
        rt.Grid((10, 0.5, 0, 0, -10, 0), (4, 4))
    with pytest.raises(ValueError, match='rotated or sheared'):
        rt.union_grid([rot])
    with pytest.raises(ValueError, match='rotated or sheared'):
        rt.read_warped(rot, g)
    with pytest.raises(ValueError, match='rotated or sheared'):
        rt.warp_coefficients((10, 0, 0, 0.1, -10, 0), north)
    for call in (lambda: rt.union_grid([a, b]), lambda: rt.union_grid([a], crs=4326), lambda: rt.read_warped(b, g), lambda: rt.read_mosaic([a, b]),
                 lambda: rt.read_aligned_stack([a, b]), lambda: rt.read_mosaic([a], grid=rt.Grid(north, (16, 16), 32634))):
        with pytest.raises(ValueError, match='reprojection between coordinate systems is not done'):
            call()
    info = rt.read_info(a)[0]
    info.transform = None
    with pytest.raises(ValueError, match='has no transform'):
        rt.union_grid([info])
    with pytest.raises(ValueError, match='has no transform'):
        rt.warp_coefficients(None, north)
    with pytest.raises(ValueError, match='resampling must be one of'):
        rt.warp_window(north, (16, 16), g, 'lanczos')
    with pytest.raises(ValueError, match='overview'):
        rt.warp_window(north, (16, 16), rt.Grid((650, 0, 0, 0, -650, 160), (1, 1)), 'average')
    assert rt.warp_window(north, (16, 16), rt.Grid((640, 0, 0, 0, -640, 160), (1, 1)), 'average') == (0, 0, 16, 16)
    with pytest.raises(ValueError, match='Grid'):
        rt.read_warped(a, north)
    with pytest.raises(ValueError, match='at least one file'):
        rt.read_mosaic([])
    with pytest.raises(ValueError, match='at least one file'):
        rt.read_aligned_stack([a, []])
    with pytest.raises(ValueError, match='level'):
        rt.read_warped(a, g, level=3)
    with pytest.raises(ValueError, match='CUDA tensor'):
        rt.warp(np.zeros((4, 4), np.uint8), north, g)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_warp_descriptor_mirrors_the_header(tmp_path):
    from satellite_computervision_amd import _lib
    D = _lib.WarpDesc
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    body = hdr[hdr.index('typedef struct satcv_warp_desc {'):hdr.index('} satcv_warp_desc;')]
    fields = [n for line in body.splitlines()[1:] for decl in line.split(';') if decl.strip()
              for n in re.sub(r'^\s*(const\s+)?\w+\*?\s+', '', decl.strip()).replace(' ', '').split(',')]
    assert fields == [f[0] for f in D._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(satcv_warp_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(satcv_warp_desc, {f}));' for f, _ in D._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(D)
    for f, _ in D._fields_:
        assert int(got[f]) == getattr(D, f).offset, f
    assert 'satcv_raster_warp' in _lib.EXPORTED_SYMBOLS


def test_warp_is_built_and_compiled_without_contraction():
    import importlib.util
    spec = importlib.util.spec_from_file_location('_satcv_build_w', os.path.join(ROOT, 'satellite_computervision_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'warp.hip' in b.SOURCES
    assert '#pragma clang fp contract(off)' in open(os.path.join(b.CSRC, 'warp.hip')).read()


def test_warp_refusals_of_the_c_abi():
    """refused on the host, with a message that names the entry point, before any launch (this test runs without a GPU)"""
    from satellite_computervision_amd import _lib
    lib, D = _lib.lib, _lib.WarpDesc
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    q = p + 2048

    def desc(**kw):
        return D(**dict(dict(src=p, src_kind=1, src_layout=0, sh=4, sw=4, src_ld=2, src_coff=0, src_row0=0, src_col0=0, dst=q, dst_kind=1, dst_layout=0,
                             dh=4, dw=4, dst_ld=2, dst_coff=0, dst_row0=0, dst_col0=0, c=2, su=1.0, ou=0.0, sv=1.0, ov=0.0, resampling=0, has_src_nodata=0,
                             src_nodata=0.0, has_dst_nodata=0, dst_nodata=0.0, keep=0), **kw))
    assert lib.satcv_raster_warp(None, None) == -1 and b'raster_warp' in lib.satcv_last_error()
    inf, nan = float('inf'), float('nan')
    for d, word in ((desc(src=None), 'null'), (desc(dst=None), 'null'), (desc(src=p + 1), 'misaligned'), (desc(dst=q + 1), 'misaligned'),
                    (desc(src_kind=4), 'unknown kind'), (desc(dst_kind=7), 'unknown kind'), (desc(dst_kind=3), 'neither'), (desc(src_kind=2, dst_kind=1), 'neither'),
                    (desc(src_layout=2), 'layout'), (desc(dst_layout=-1), 'layout'), (desc(resampling=4), 'resampling'), (desc(resampling=-1), 'resampling'),
                    (desc(c=17, src_ld=17, dst_ld=17), 'at most 16'), (desc(c=3), 'channel range'), (desc(src_coff=1), 'channel range'),
                    (desc(dst_coff=1), 'channel range'), (desc(dst_coff=-1), 'channel range'), (desc(src_ld=0), 'channel range'),
                    (desc(su=0.0), 'scale'), (desc(sv=0.0), 'scale'), (desc(su=inf), 'scale'), (desc(sv=nan), 'scale'), (desc(ou=nan), 'offset'), (desc(ov=inf), 'offset'),
                    (desc(sh=0), 'positive'), (desc(dw=0), 'positive'), (desc(c=0), 'positive'), (desc(dh=-3), 'positive'),
                    (desc(sh=1 << 16, sw=1 << 16), '2^31'), (desc(dh=1 << 16, dw=1 << 15), '2^31'),
                    (desc(dst=p), 'overlap'), (desc(dst=p + 32), 'overlap'), (desc(src=q + 16), 'overlap'),
                    (desc(resampling=3, su=64.5), 'overview'), (desc(resampling=3, sv=-65.0), 'overview')):
        assert lib.satcv_raster_warp(ctypes.byref(d), None) == -1, word
        assert word.encode() in lib.satcv_last_error() and b'raster_warp' in lib.satcv_last_error(), (word, lib.satcv_last_error())
