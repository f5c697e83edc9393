"""CPU checks of the Cloud-Optimized GeoTIFF writer (satellite_computervision_amd/raster_tools.py, csrc/raster.hip): the LZW coder on the
host against a slow restatement and a decoder, files assembled by the container code against libtiff (through Pillow) and tifffile, the
layout rules, the argument refusals, and the host entries under AddressSanitizer.  No GPU is touched: the tiles come from
tests/tiff_oracle.py, the LZW streams from satcv_lzw_encode_host."""
import ctypes
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import tiff_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_PYTHON = '/opt/conda/bin/python3.9'         # side interpreter of the image that has tifffile
TRANSFORM = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)


def _lzw_inputs():
    rng = np.random.default_rng(0)
    strip = np.random.default_rng(1).integers(0, 256, 6000, dtype=np.uint8)
    grid = np.kron(rng.integers(0, 5, (20, 20), dtype=np.uint8), np.ones((8, 8), np.uint8))
    return {'empty': b'', 'one byte': b'\x07', 'constant': bytes([3]) * 6300, 'random 13000': rng.integers(0, 256, 13000, dtype=np.uint8).tobytes(),
            'class grid': grid.tobytes(), 'uint16': rng.integers(0, 65536, 4096, dtype=np.uint16).tobytes(),
            'strip 3972': strip[:3972].tobytes(), 'strip 3973': strip[:3973].tobytes(), 'strip 3974': strip[:3974].tobytes()}


def test_host_encoder_equals_the_reference_encoder_byte_for_byte():
    from satellite_computervision_amd import raster_tools as rt
    finals = {}
    for name, data in _lzw_inputs().items():
        info = {}
        ref = TO.lzw_encode_ref(data, info)
        assert TO.lzw_decode(ref) == data, name
        assert rt.lzw_encode(data) == ref, name
        assert len(ref) <= 2 * len(data) + 16, name
        finals[name] = info
    assert len(_lzw_inputs()['uint16']) == 8192
    # the last code of the 3973-byte strip fills the table exactly: Clear, then EOI at 9 bits
    assert finals['strip 3973']['final_next'] == 4094 and finals['strip 3972']['final_next'] == 4093
    assert finals['random 13000']['clears'] >= 2 and finals['constant']['clears'] == 0


def test_host_encoder_refuses_a_short_buffer_and_writes_nothing_past_it():
    from satellite_computervision_amd import _lib
    data = _lzw_inputs()['random 13000']
    ref = TO.lzw_encode_ref(data)
    size = ctypes.c_int64()
    buf = ctypes.create_string_buffer(b'\xaa' * (len(ref) + 8), len(ref) + 8)
    assert _lib.lib.satcv_lzw_encode_host(data, len(data), buf, len(ref) - 1, ctypes.byref(size)) == -1
    assert b'needs' in _lib.lib.satcv_last_error() and size.value == len(ref)
    assert buf.raw[len(ref) - 1:] == b'\xaa' * 9
    assert _lib.lib.satcv_lzw_encode_host(data, len(data), buf, len(ref), ctypes.byref(size)) == 0 and buf.raw[:len(ref)] == ref
    assert _lib.lib.satcv_lzw_encode_host(data, len(data), buf, len(ref), None) == -1
    assert _lib.lib.satcv_lzw_encode_host(None, 5, buf, 16, ctypes.byref(size)) == -1
    assert _lib.lib.satcv_lzw_encode_host(data, 1 << 30, buf, 16, ctypes.byref(size)) == -1


def _image(dtype, bands, h=70, w=90, seed=0):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = (yy[..., None] * 3 + xx[..., None] * 5 + np.arange(bands) * 40)
    if dt.kind == 'f':
        return (smooth / 7.0 + rng.random((h, w, bands))).astype(np.float32)
    info = np.iinfo(dt)
    noisy = smooth * (info.max // 600) + rng.integers(0, 4, (h, w, bands))
    if dt.kind == 'i':
        noisy = noisy - info.max // 3
    return noisy.astype(dt)


def _encode(tiles, compress):
    from satellite_computervision_amd import raster_tools as rt
    if compress == 'lzw':
        return [rt.lzw_encode(t.tobytes()) for t in tiles]
    if compress == 'deflate':
        return [zlib.compress(t.tobytes(), 6) for t in tiles]
    return [t.tobytes() for t in tiles]


def _write(path, img, compress, predictor=False, blocksize=32, nodata=255, overviews='auto', transform=TRANSFORM, crs='EPSG:32618', resampling='nearest'):
    """a file assembled by the container code from oracle-made tiles -> (levels, shapes)"""
    from satellite_computervision_amd import raster_tools as rt
    h, w, c = img.shape
    shapes = [(h, w)] + rt.overview_shapes(h, w, blocksize, overviews)
    levels = TO.pyramid_ref(img, shapes[1:], resampling, nodata)
    tiles = [_encode(TO.tiles_ref(l, blocksize, predictor, nodata), compress) for l in levels]
    rt.write_tiles(path, shapes, tiles, img.dtype.name, c, blocksize, compress, predictor, nodata, transform, crs)
    return levels, shapes


CASES = [(dt, c, comp, False) for dt, c in (('uint8', 1), ('uint8', 3), ('uint16', 1), ('float32', 1), ('int32', 1)) for comp in ('lzw', 'deflate', None)] + \
        [('uint8', 1, 'lzw', True), ('uint8', 3, 'lzw', True), ('uint16', 1, 'lzw', True), ('uint16', 1, 'deflate', True)]


@pytest.mark.parametrize('dtype,bands,compress,predictor', CASES)
def test_libtiff_reads_the_assembled_files(tmp_path, monkeypatch, dtype, bands, compress, predictor):
    """Pillow (libtiff) decodes the full-resolution image and every overview page: pixels equal.
    Pillow's own table of pixel modes knows three 8-bit samples only as Photometric 2 (RGB); the files carry Photometric 1 with two
    unspecified ExtraSamples (what GDAL writes for PHOTOMETRIC=MINISBLACK), so that one combination is added to the table for the test:
    libtiff decodes the tiles either way, the entry only names the layout of the decoded bytes."""
    from PIL import Image, TiffImagePlugin
    monkeypatch.setitem(TiffImagePlugin.OPEN_INFO, (TiffImagePlugin.II, 1, (1,), 1, (8, 8, 8), (0, 0)), ('RGB', 'RGB'))
    img = _image(dtype, bands)
    path = str(tmp_path / 'a.tif')
    levels, _ = _write(path, img, compress, predictor)
    buf = open(path, 'rb').read()
    ifds = TO.parse_tiff(buf)
    assert len(ifds) == len(levels) == 3                    # 70 x 90 -> 35 x 45 -> 18 x 23 at blocksize 32
    for k, lvl in enumerate(levels):
        assert np.array_equal(TO.read_level(buf, ifds[k]), lvl), k      # (the helper parser, used on the device files too)
    with Image.open(path) as im:
        assert im.n_frames == len(levels)
        for k, lvl in enumerate(levels):
            im.seek(k)
            got = np.asarray(im)
            got = got.reshape(lvl.shape) if got.ndim == 2 else got
            assert got.dtype == lvl.dtype and np.array_equal(got, lvl), (k, got.dtype)


def test_layout_rules(tmp_path):
    """header, every IFD (full resolution first, overviews by decreasing size), the IFDs' values -- all before the first tile byte; tile data
    from the smallest overview to the full resolution, tiles row-major, every tile on an even offset; tags ascending; subfile types"""
    img = _image('uint8', 3, 150, 201, seed=3)
    path = str(tmp_path / 'l.tif')
    levels, shapes = _write(path, img, 'lzw', True, blocksize=32)
    buf = open(path, 'rb').read()
    ifds = TO.parse_tiff(buf)
    assert buf[:4] == b'II*\0' and len(ifds) == len(shapes) == 4
    assert [(TO.tag(i, 257)[0], TO.tag(i, 256)[0]) for i in ifds] == shapes
    assert [TO.tag(i, 254)[0] for i in ifds] == [0, 1, 1, 1]
    first_tile = min(min(TO.tag(i, 324)) for i in ifds)
    pos = 8
    for i in ifds:
        assert i['offset'] == pos                            # IFDs back to back after the header
        pos = i['end']
        assert i['order'] == sorted(i['order'])
        assert all(lo % 2 == 0 and hi <= first_tile for lo, hi in i['value_spans']) and i['end'] <= first_tile
    flat = [(o, n) for i in reversed(ifds) for o, n in zip(TO.tag(i, 324), TO.tag(i, 325))]      # smallest overview first, tiles row-major
    assert all(o % 2 == 0 for o, _ in flat)
    assert all(flat[k][0] + flat[k][1] + (flat[k][1] & 1) == flat[k + 1][0] for k in range(len(flat) - 1))
    assert flat[-1][0] + flat[-1][1] + (flat[-1][1] & 1) == len(buf)
    want = [254, 256, 257, 258, 259, 262, 277, 284, 317, 322, 323, 324, 325, 338, 339, 33550, 33922, 34735, 42113]
    assert ifds[0]['order'] == want and ifds[1]['order'] == [t for t in want if t < 33000 or t == 42113]
    t0 = ifds[0]['tags']
    assert t0[258][2] == (8, 8, 8) and t0[259][2] == (5,) and t0[262][2] == (1,) and t0[277][2] == (3,) and t0[284][2] == (1,) and t0[317][2] == (2,)
    assert t0[338][2] == (0, 0) and t0[339][2] == (1, 1, 1) and t0[42113][2] == b'255\0'
    assert t0[33550][2] == (10.0, 10.0, 0.0) and t0[33922][2] == (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)
    assert t0[34735][2] == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32618)
    for k, lvl in enumerate(levels):
        assert np.array_equal(TO.read_level(buf, ifds[k]), lvl)
    # no nodata, no overviews, one band, a sheared transform, a geographic code
    _write(path, img[..., :1], None, nodata=None, overviews=0, transform=(1e-4, 2e-5, -77.0, 1e-5, -1e-4, 39.0), crs=4326)
    (only,) = TO.parse_tiff(open(path, 'rb').read())
    assert only['order'] == [254, 256, 257, 258, 259, 262, 277, 284, 322, 323, 324, 325, 339, 34264, 34735]
    assert only['tags'][34264][2] == (1e-4, 2e-5, 0.0, -77.0, 1e-5, -1e-4, 0.0, 39.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert only['tags'][34735][2] == (1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326)


def test_offsets_past_4_gib_name_bigtiff():
    from satellite_computervision_amd import raster_tools as rt
    with pytest.raises(ValueError, match='BigTIFF'):
        rt.build_container([(64, 64)], 'uint8', 1, 32, None, False, 255, TRANSFORM, 32618, [[1 << 30] * 4])


def _tifffile_available():
    try:
        return subprocess.run([SIDE_PYTHON, '-c', 'import tifffile'], capture_output=True, timeout=60).returncode == 0
    except (OSError, subprocess.SubprocessError):
        return False


READER = r'''
import json, sys, numpy as np, tifffile
out = []
for path in sys.argv[1:]:
    with tifffile.TiffFile(path) as t:
        p = t.pages[0]
        geo = t.geotiff_metadata or {}
        np.save(path + '.npy', p.asarray())
        np.save(path + '.last.npy', t.pages[len(t.pages) - 1].asarray())
        out.append({'tiled': bool(p.is_tiled), 'pages': len(t.pages), 'nodata': p.tags['GDAL_NODATA'].value if 'GDAL_NODATA' in p.tags else None,
                    'scale': list(geo.get('ModelPixelScale', [])), 'tiepoint': [float(v) for v in np.ravel(geo.get('ModelTiepoint', []))],
                    'transformation': [float(v) for v in np.ravel(geo.get('ModelTransformation', []))],
                    'model': str(geo.get('GTModelTypeGeoKey')), 'raster': str(geo.get('GTRasterTypeGeoKey')),
                    'projected': int(geo['ProjectedCSTypeGeoKey']) if 'ProjectedCSTypeGeoKey' in geo else None,
                    'geographic': int(geo['GeographicTypeGeoKey']) if 'GeographicTypeGeoKey' in geo else None,
                    'subfile': [int(q.tags['NewSubfileType'].value) for q in t.pages]})
print(json.dumps(out))
'''


def test_tifffile_reads_the_geotiff_keys_and_the_pixels(tmp_path):
    if not _tifffile_available():
        pytest.skip('no side interpreter with tifffile')
    img = _image('uint16', 3, seed=5)
    files = [str(tmp_path / n) for n in ('utm.tif', 'geo.tif', 'shear.tif')]
    levels, shapes = _write(files[0], img, 'deflate', crs='EPSG:32618')
    _write(files[1], img, 'deflate', transform=(1e-4, 0.0, -77.0, 0.0, -1e-4, 39.0), crs='EPSG:4326', nodata=None)
    _write(files[2], img, 'deflate', transform=(10.0, 1.0, 5.0, 2.0, -10.0, 7.0), crs=32618)
    r = subprocess.run([SIDE_PYTHON, '-c', READER] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    utm, geo, shear = json.loads(r.stdout.strip().splitlines()[-1])
    for res, f in zip((utm, geo, shear), files):
        assert res['tiled'] and res['pages'] == len(shapes) == 3 and res['subfile'] == [0, 1, 1]
        assert np.array_equal(np.load(f + '.npy'), img) and np.array_equal(np.load(f + '.last.npy'), levels[-1])
    assert utm['scale'] == [10.0, 10.0, 0.0] and utm['tiepoint'] == [0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0]
    assert 'Projected' in utm['model'] and 'IsArea' in utm['raster'] and utm['projected'] == 32618 and utm['geographic'] is None
    assert str(utm['nodata']).strip('\0') == '255'
    assert geo['scale'] == [1e-4, 1e-4, 0.0] and geo['tiepoint'] == [0.0, 0.0, 0.0, -77.0, 39.0, 0.0]
    assert 'Geographic' in geo['model'] and geo['geographic'] == 4326 and geo['projected'] is None and geo['nodata'] is None
    assert shear['scale'] == [] and shear['tiepoint'] == []
    assert shear['transformation'] == [10.0, 1.0, 0.0, 5.0, 2.0, -10.0, 0.0, 7.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def test_argument_refusals_of_the_python_interface(tmp_path):
    """every refusal comes before a launch (this test runs without a GPU)"""
    from satellite_computervision_amd import raster_tools as rt
    out = str(tmp_path / 'x.tif')
    a = np.zeros((8, 8), np.uint8)
    f = np.zeros((8, 8), np.float32)
    bad = [dict(arr=a, crs='PROJCS["WGS 84 / UTM zone 18N"]'), dict(arr=a, crs='EPSG:abc'), dict(arr=a, crs=None), dict(arr=a, crs=70000),
           dict(arr=a, dtype='float64'), dict(arr=a, compress='zstd'), dict(arr=a, blocksize=100), dict(arr=a, blocksize=0),
           dict(arr=f, predictor=True), dict(arr=a, dtype='float32', predictor=True), dict(arr=f, resampling='mode'), dict(arr=a, resampling='cubic'),
           dict(arr=a, scale=100.0), dict(arr=a, overviews=-1), dict(arr=a, overviews='all'), dict(arr=a, nodata=-1), dict(arr=a, nodata=0.5),
           dict(arr=a, transform=(1, 0, 0, 0, -1)), dict(arr=np.zeros((8, 8), np.int64)), dict(arr=np.zeros((8,), np.uint8)),
           dict(arr=np.zeros((4, 4, 17), np.uint8)), dict(arr=np.zeros((2, 2, 2, 2), np.uint8)), dict(arr=np.zeros((0, 4), np.uint8))]
    for kw in bad:
        kw = dict(dict(transform=TRANSFORM, crs='EPSG:32618'), **kw)
        with pytest.raises(ValueError):
            rt.write_cog(kw.pop('arr'), out, **kw)
        assert not os.path.exists(out), kw
    assert rt.parse_crs('EPSG:4326') == (4326, True) and rt.parse_crs(32618) == (32618, False) and rt.parse_crs('epsg:3999') == (3999, False)
    assert rt.parse_crs(4999) == (4999, True) and rt.parse_crs(5000) == (5000, False)
    assert rt.overview_shapes(10980, 10980, 512) == [(5490, 5490), (2745, 2745), (1373, 1373), (687, 687), (344, 344)]
    assert rt.overview_shapes(37, 53, 16, 9) == [(19, 27), (10, 14), (5, 7), (3, 4), (2, 2), (1, 1)] and rt.overview_shapes(64, 64, 64) == []
    with pytest.raises(ValueError):
        rt.numpy_to_raster(a, {'transform': list(TRANSFORM), 'crs': 'EPSG:32618', 'cols': 9, 'rows': 8}, out, 'uint8')


def test_descriptor_refusals_of_the_c_abi():
    """c > 16, a blocksize that is no multiple of 16, tile_bytes >= 2^30, the predictor on float, 'mode' on float, unknown kinds: refused on the
    host with a message; the descriptor mirrors the header"""
    from satellite_computervision_amd import _lib
    lib, D = _lib.lib, _lib.RasterDesc
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def desc(**kw):
        return D(**dict(dict(src=p, src_kind=0, h=4, w_=4, c=1, ld=1, coff=0, dst=p, dst_kind=0, blocksize=16), **kw))

    def refused(fn, d, word):
        assert fn(ctypes.byref(d), None) == -1, word
        assert word.encode() in lib.satcv_last_error(), (word, lib.satcv_last_error())
    for fn in (lib.satcv_raster_convert, lib.satcv_raster_overview, lib.satcv_raster_tiles):
        assert fn(None, None) == -1
        refused(fn, desc(src=None), 'null')
        refused(fn, desc(c=17, ld=17), 'at most 16')
        refused(fn, desc(src_kind=4, dst_kind=4), 'unknown kind')
        refused(fn, desc(src_kind=6, dst_kind=6), 'unknown kind')
        refused(fn, desc(h=1 << 16, w_=1 << 16), '2^31')
        refused(fn, desc(h=0), 'positive')
    refused(lib.satcv_raster_convert, desc(coff=1), 'coff + c <= ld')
    refused(lib.satcv_raster_convert, desc(scale=2.0), 'scale')
    refused(lib.satcv_raster_overview, desc(dst_kind=1), 'keeps the kind')
    refused(lib.satcv_raster_overview, desc(ld=3), 'contiguous')
    refused(lib.satcv_raster_overview, desc(src_kind=2, dst_kind=2, resampling=2), 'mode')
    refused(lib.satcv_raster_overview, desc(resampling=3), 'resampling')
    refused(lib.satcv_raster_tiles, desc(blocksize=24), 'multiple of 16')
    refused(lib.satcv_raster_tiles, desc(blocksize=0), 'multiple of 16')
    refused(lib.satcv_raster_tiles, desc(src_kind=2, dst_kind=2, predictor=1), 'predictor')
    refused(lib.satcv_raster_tiles, desc(src_kind=5, dst_kind=5, c=16, ld=16, blocksize=4096), '2^30')
    sizes = ctypes.create_string_buffer(64)
    for args, word in (((None, 1, 256, p, ctypes.addressof(sizes), None), 'null'), ((p, 0, 256, p, ctypes.addressof(sizes), None), 'tiles'),
                       ((p, 1, 1 << 30, p, ctypes.addressof(sizes), None), '2^30'), ((p, 1, 24, p, ctypes.addressof(sizes), None), 'multiple of 16'),
                       ((p + 1, 1, 256, p, ctypes.addressof(sizes), None), 'aligned')):
        assert lib.satcv_lzw_tiles(*args) == -1 and word.encode() in lib.satcv_last_error(), (word, lib.satcv_last_error())
    assert lib.satcv_bytes_compact(None, 16, p, p, 1, p, 16, None) == -1 and lib.satcv_bytes_compact(p, 0, p, p, 1, p, 16, None) == -1
    assert lib.satcv_bytes_compact(p, 16, p, p, 0, p, 16, None) == -1 and lib.satcv_bytes_compact(p, 16, p, p, 1, p, 0, None) == -1
    # the ctypes mirror against the header, as test_descriptor_layouts_match_the_header does for the older descriptors
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    body = hdr[hdr.index('typedef struct satcv_raster_desc {'):hdr.index('} satcv_raster_desc;')]
    import re
    fields = [n for line in body.splitlines()[1:] for decl in line.split(';') if decl.strip()
              for n in re.sub(r'^\s*(const\s+)?\w+\*?\s+', '', decl.strip()).replace(' ', '').split(',')]
    assert fields == [f[0] for f in D._fields_]


def test_layout_of_the_raster_descriptor(tmp_path):
    from satellite_computervision_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(satcv_raster_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(satcv_raster_desc, {f}));' for f, _ in _lib.RasterDesc._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_lib.RasterDesc)
    for f, _ in _lib.RasterDesc._fields_:
        assert int(got[f]) == getattr(_lib.RasterDesc, f).offset, f


def test_oracle_rules_on_hand_made_blocks():
    """the NumPy restatement itself, on values worked out by hand (it is the reference of the GPU tests)"""
    a = np.array([[1, 1, 5, 255], [2, 2, 255, 255], [7, 9, 4, 4]], np.uint8)[..., None]
    assert TO.overview_ref(a, 'nearest', 255)[..., 0].tolist() == [[1, 5], [7, 4]]
    assert TO.overview_ref(a, 'average', 255)[..., 0].tolist() == [[2, 5], [8, 4]]      # (1+1+2+2)/4 = 1.5 -> 2 (half up); 5; (7+9)/2; 4
    assert TO.overview_ref(a, 'mode', 255)[..., 0].tolist() == [[1, 5], [7, 4]]         # 2-2 tie -> the smallest
    b = np.array([[255, 255], [255, 255]], np.uint8)[..., None]
    assert TO.overview_ref(b, 'mode', 255).ravel().tolist() == [255] and TO.overview_ref(b, 'average', 255).ravel().tolist() == [255]
    assert TO.overview_ref(b, 'average', None).ravel().tolist() == [255]
    n = np.array([[-3, -4]], np.int16)[..., None]
    assert TO.overview_ref(n, 'average', None).ravel().tolist() == [-3]                  # floor((2 * -7 + 2) / 4) = -3
    f = np.array([[np.nan, 1.0], [np.nan, 2.0]], np.float32)[..., None]
    assert TO.overview_ref(f, 'average', None).ravel().tolist() == [1.5] and np.isnan(TO.overview_ref(f[:, :1], 'average', None)).all()
    v = np.array([np.nan, -3.2, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, -0.5], np.float32).reshape(1, -1, 1)
    assert TO.convert_ref(v, 'uint8', None, 255).ravel().tolist() == [255, 0, 0, 2, 2, 254, 255, 255, 0]
    assert TO.convert_ref(v, 'uint8', None, None).ravel().tolist()[0] == 0
    assert TO.convert_ref(np.array([[[70000], [-5]]], np.int32), 'uint8').ravel().tolist() == [255, 0]
    assert TO.convert_ref(np.array([[[40000]]], np.uint16), 'int16').ravel().tolist() == [32767]
    t = TO.tiles_ref(np.arange(6, dtype=np.uint8).reshape(1, 6, 1) * 50, 16, True, 255)
    assert t.shape == (1, 16, 16, 1) and t[0, 0, :8, 0].tolist() == [0, 50, 50, 50, 50, 50, 5, 0] and t[0, 1, :3, 0].tolist() == [255, 0, 0]


def test_host_entries_under_asan_ubsan(tmp_path):
    """tests/asan/raster_host_driver.c against the sanitizer-built host-only library (build.py::build_host_asan, which compiles every source,
    csrc/raster.hip included), linked in the normal way, as tests/test_host_cpu.py drives tests/asan/host_abi_driver.c: the LZW coder on the
    inputs above, with `cap` one byte too small, and the host-side refusals.  Any sanitizer report aborts the driver."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('_satcv_build', os.path.join(ROOT, 'satellite_computervision_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert 'raster.hip' in b.SOURCES
    so = b.build_host_asan()
    exe = tmp_path / 'raster_host_driver'
    clang = '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([clang, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-g', '-O1', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'asan', 'raster_host_driver.c'), '-o', str(exe), '-L', os.path.dirname(so), '-lsatcv_hostasan',
                    '-Wl,-rpath,' + os.path.dirname(so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'),
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    assert ' 0 failures' in r.stdout, r.stdout


def test_the_predictors_take_device_and_default_to_the_host_result():
    """every new argument defaults to the earlier behaviour"""
    import inspect
    from satellite_computervision_amd import pc_tools as pc, prediction_tools as pt
    for fn in (pt.predict_scene, pt.predict_series_scene, pt.predict_hybrid_scene, pt.predict_chips_device):
        assert inspect.signature(fn).parameters['device'].default is False, fn.__name__
    sig = inspect.signature(pc.predict_change).parameters
    assert all(sig[k].default is None for k in ('out_file', 'transform', 'crs'))
    assert list(inspect.signature(pt.write_geotiff_prediction).parameters) == ['image', 'jsonFile', 'aoi']
    assert list(inspect.signature(pt.write_geotiff_predictions).parameters) == ['imageDataset', 'model', 'jsonFile', 'outImgBase', 'outImgPath', 'kernel_buffer']
    maps = pt._Maps()
    assert list(inspect.signature(maps.host).parameters) == ['channel', 'device']
