"""CPU checks of the GeoTIFF / COG reader (satellite_computervision_amd/raster_tools.py `read_info`, `read_cog`; csrc/lzw_core.hpp `Decoder`):
the LZW decoder on the host against the decoder of tests/tiff_oracle.py, the container parser and the host read path on files of the
library's own writer and on libtiff's (tests/golden/tiff_read, made by tests/golden/make_tiff_fixtures.py), planar-2 and big-strip files
assembled by hand, every refusal, and the decoder on malformed streams under AddressSanitizer.  No GPU is touched.  Every comparison is
exact: decoding is integer work."""
import ctypes
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import tiff_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'tiff_read')
TRANSFORM = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
WINDOW = (17, 5, 40, 61)


# ------------------------------------------------------------------------------------------------------------ the decoder
def _drop_bits(stream, nbits):
    """the stream without its first nbits bits, zero-padded to a byte"""
    total = len(stream) * 8 - nbits
    v = int.from_bytes(stream, 'big') & ((1 << total) - 1)
    pad = -total % 8
    return (v << pad).to_bytes((total + pad) // 8, 'big')


def _streams():
    from satellite_computervision_amd import raster_tools as rt
    rng = np.random.default_rng(0)
    inputs = {'empty': b'', 'one byte': b'\x07', 'two bytes': b'\x07\x07', '70 000 zeros': bytes(70000),
              '20 000 random': rng.integers(0, 256, 20000, dtype=np.uint8).tobytes(), 'ramp': bytes(range(256)) * 24}
    out = []
    for name, data in inputs.items():
        info = {}
        ref = TO.lzw_encode_ref(data, info)
        out.append((name + ', reference encoder', ref, data))
        out.append((name + ', host encoder', rt.lzw_encode(data), data))
        if name == '20 000 random':
            assert info['clears'] >= 3
        if len(data) > 2:
            out.append((name + ', EOI cut off', ref[:-2], data))       # (EOI and its padding are 9 ... 16 bits: the last data code may go too)
            out.append((name + ', no leading Clear', _drop_bits(ref, 9), data))
    z = np.load(os.path.join(GOLD, 'expected.npz'))
    for name in z.files:                                      # libtiff's strips
        buf = open(os.path.join(GOLD, name + '.tif'), 'rb').read()
        (ifd,) = TO.parse_tiff(buf)
        for o, n in zip(TO.tag(ifd, 273), TO.tag(ifd, 279)):
            out.append((name + ' strip', buf[o:o + n], None))
    return out


def test_host_decoder_equals_the_oracle():
    """every width, a full table with its Clear and KwKwK strings (zeros), several Clears (random), streams without EOI and without
    the leading Clear, and libtiff's own streams; with exactly the room needed and with room to spare"""
    from satellite_computervision_amd import raster_tools as rt
    for name, stream, data in _streams():
        want = TO.lzw_decode(stream)
        if data is not None:
            assert (data.startswith(want) and len(data) - len(want) < 4096) if 'EOI cut off' in name else want == data, name
        for cap in (len(want), len(want) + 100):
            if 'EOI cut off' in name and cap > len(want):
                assert rt.lzw_decode(stream, cap) == (1, want), name       # no EOI and room left: truncated, the bytes so far are out
                continue
            assert rt.lzw_decode(stream, cap) == (0, want), (name, cap)


def test_host_decoder_statuses_and_refusals():
    from satellite_computervision_amd import _lib, raster_tools as rt
    data = bytes(range(256)) * 8
    s = TO.lzw_encode_ref(data)
    assert rt.lzw_decode(s[:len(s) // 2], len(data))[0] == 1
    assert rt.lzw_decode(b'', 4) == (1, b'') and rt.lzw_decode(s, 0) == (0, b'')
    status, got = rt.lzw_decode(TO.lzw_encode_ref(bytes(3000)), 2999)         # the last string would pass the cap: nothing of it is written
    assert status == 3 and got == bytes(len(got)) and len(got) < 2999
    bits = TO._Bits()
    for code in (256, 65, 300):                                                # 300 is above the next free code (259)
        bits.put(code, 9)
    assert rt.lzw_decode(bits.done(), 10) == (2, b'A')
    bits = TO._Bits()
    for code in (256, 258):                                                    # a table code straight after a Clear
        bits.put(code, 9)
    assert rt.lzw_decode(bits.done(), 10) == (2, b'')
    size, status = ctypes.c_int64(), ctypes.c_int32()
    buf = ctypes.create_string_buffer(16)
    lib = _lib.lib
    assert lib.satcv_lzw_decode_host(s, len(s), buf, 16, None, ctypes.byref(status)) == -1 and b'null' in lib.satcv_last_error()
    assert lib.satcv_lzw_decode_host(None, 4, buf, 16, ctypes.byref(size), ctypes.byref(status)) == -1
    assert lib.satcv_lzw_decode_host(s, -1, buf, 16, ctypes.byref(size), ctypes.byref(status)) == -1
    assert lib.satcv_lzw_decode_host(s, len(s), buf, 1 << 30, ctypes.byref(size), ctypes.byref(status)) == -1 and b'2^30' in lib.satcv_last_error()


# ------------------------------------------------------------------------------------------------------------ files of the library's writer
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


def _write(path, img, compress, predictor=False, blocksize=32, nodata=255, transform=TRANSFORM, crs='EPSG:32618'):
    """a file assembled by the library's container code from oracle-made tiles -> (levels, shapes)"""
    from satellite_computervision_amd import raster_tools as rt
    h, w, c = img.shape
    shapes = [(h, w)] + rt.overview_shapes(h, w, blocksize, 'auto')
    levels = TO.pyramid_ref(img, shapes[1:], 'nearest', nodata)
    enc = {'lzw': lambda t: rt.lzw_encode(t.tobytes()), 'deflate': lambda t: zlib.compress(t.tobytes(), 6), None: lambda t: t.tobytes()}[compress]
    tiles = [[enc(t) for t in TO.tiles_ref(l, blocksize, predictor, nodata)] for l in levels]
    rt.write_tiles(path, shapes, tiles, img.dtype.name, c, blocksize, compress, predictor, nodata, transform, crs)
    return levels, shapes


CASES = [(dt, c, comp, pred) for dt, c in (('uint8', 1), ('uint8', 3), ('uint16', 4), ('int16', 1), ('int32', 1), ('float32', 1))
         for comp in ('lzw', 'deflate', None) for pred in ((False,) if dt == 'float32' else (False, True))]


@pytest.mark.parametrize('dtype,bands,compress,predictor', CASES)
def test_parser_and_host_read_path_on_the_writers_files(tmp_path, dtype, bands, compress, predictor):
    from satellite_computervision_amd import raster_tools as rt
    img = _image(dtype, bands)
    path = str(tmp_path / 'a.tif')
    levels, shapes = _write(path, img, compress, predictor)
    infos = rt.read_info(path)
    assert [i.shape for i in infos] == shapes == [(70, 90), (35, 45), (18, 23)]
    assert [i.overview for i in infos] == [False, True, True] and [i.index for i in infos] == [0, 1, 2]
    for i in infos:
        assert (i.bands, i.dtype, i.block_shape, i.tiled, i.compression, i.predictor, i.planar, i.nodata) == \
               (bands, dtype, (32, 32), True, compress, predictor, 1, 255.0)
    assert infos[0].transform == TRANSFORM and infos[0].epsg == 32618 and infos[0].crs == 'EPSG:32618'
    assert infos[1].transform is None and infos[1].epsg is None
    buf = open(path, 'rb').read()
    ifds = TO.parse_tiff(buf)
    assert infos[0].offsets.tolist() == list(TO.tag(ifds[0], 324)) and infos[0].counts.tolist() == list(TO.tag(ifds[0], 325))
    full = rt.read_cog(path, device=False, decode='host')
    assert full.array.dtype == img.dtype and np.array_equal(full.array, TO.read_level(buf, ifds[0])) and np.array_equal(full.array, img)
    assert (full.transform, full.crs, full.nodata, full.dtype) == (TRANSFORM, 'EPSG:32618', 255.0, dtype)
    win = rt.read_cog(path, window=WINDOW, device=False, decode='host')
    assert np.array_equal(win.array, full.array[17:57, 5:66])
    assert win.transform == (10.0, 0.0, 399960.0 + 50.0, 0.0, -10.0, 4500000.0 - 170.0)
    one = rt.read_cog(path, level=1, device=False, decode='host')
    assert np.array_equal(one.array, levels[1]) and np.array_equal(one.array, TO.read_level(buf, ifds[1]))
    assert one.transform == (10.0 * 90 / 45, 0.0, 399960.0, 0.0, -10.0 * 70 / 35, 4500000.0) and one.crs == 'EPSG:32618'
    last = rt.read_cog(path, level=2, bands=[bands - 1], layout='chw', device=False)
    assert last.array.shape == (1, 18, 23) and np.array_equal(last.array[0], levels[2][..., bands - 1])


def test_geographic_and_sheared_georeferences(tmp_path):
    from satellite_computervision_amd import raster_tools as rt
    img = _image('uint8', 1)
    path = str(tmp_path / 'g.tif')
    _write(path, img, None, nodata=None, transform=(1e-4, 2e-5, -77.0, 1e-5, -1e-4, 39.0), crs=4326)
    info = rt.read_info(path)[0]
    assert info.transform == (1e-4, 2e-5, -77.0, 1e-5, -1e-4, 39.0) and info.epsg == 4326 and info.nodata is None
    r = rt.read_cog(path, window=(2, 3, 4, 5), device=False)
    assert r.transform == (1e-4, 2e-5, -77.0 + 3 * 1e-4 + 2 * 2e-5, 1e-5, -1e-4, 39.0 + 3 * 1e-5 - 2 * 1e-4) and r.nodata is None


def test_libtiff_fixtures():
    from satellite_computervision_amd import raster_tools as rt
    z = np.load(os.path.join(GOLD, 'expected.npz'))
    assert sorted(z.files) == ['classes_u8', 'noise_u16', 'rgb_u8', 'smooth_u16_pred2', 'zeros_u8']
    for name in z.files:
        path = os.path.join(GOLD, name + '.tif')
        want = z[name] if z[name].ndim == 3 else z[name][..., None]
        (info,) = rt.read_info(path)
        assert (info.shape, info.bands, info.dtype, info.tiled, info.compression, info.planar) == \
               (want.shape[:2], want.shape[2], want.dtype.name, False, 'lzw', 1), name
        assert info.predictor == name.endswith('pred2') and info.transform is None and info.epsg is None and not info.overview
        assert info.block_shape[1] == want.shape[1] and len(info.offsets) == -(-want.shape[0] // info.block_shape[0])
        r = rt.read_cog(path, device=False, decode='host')
        assert r.array.dtype == want.dtype and np.array_equal(r.array, want), name
        assert r.transform is None and r.crs is None and r.nodata is None
    assert len(rt.read_info(os.path.join(GOLD, 'zeros_u8.tif'))[0].offsets) == 2
    w = rt.read_cog(os.path.join(GOLD, 'smooth_u16_pred2.tif'), window=WINDOW, device=False)
    assert np.array_equal(w.array[..., 0], z['smooth_u16_pred2'][17:57, 5:66])


# ------------------------------------------------------------------------------------------------------------ files assembled by hand
def _tiff(tags, blobs):
    """a little-endian classic TIFF of one IFD: tags {tag: (type, values)}, the block list tags filled from `blobs` (offsets_tag, counts_tag)"""
    fmt = {3: 'H', 4: 'I', 12: 'd', 2: 's'}
    off_tag, cnt_tag = (324, 325) if 322 in tags else (273, 279)
    tags = dict(tags)
    tags[off_tag] = (4, [0] * len(blobs))
    tags[cnt_tag] = (4, [len(b) for b in blobs])
    order = sorted(tags)
    pos = 8 + 2 + 12 * len(order) + 4
    where = {}
    for t in order:
        typ, vals = tags[t]
        n = len(vals) * struct.calcsize(fmt[typ])
        if n > 4:
            where[t] = pos
            pos += n + (n & 1)
    offsets = []
    for b in blobs:
        offsets.append(pos)
        pos += len(b) + 1                                     # (odd gaps: block offsets are arbitrary)
    tags[off_tag] = (4, offsets)
    out = bytearray(pos)
    out[:8] = struct.pack('<2sHI', b'II', 42, 8)
    struct.pack_into('<H', out, 8, len(order))
    for i, t in enumerate(order):
        typ, vals = tags[t]
        raw = struct.pack('<%d%s' % (len(vals), fmt[typ]), *vals)
        struct.pack_into('<HHI', out, 10 + 12 * i, t, typ, len(vals))
        if len(raw) <= 4:
            out[18 + 12 * i:18 + 12 * i + len(raw)] = raw
        else:
            struct.pack_into('<I', out, 18 + 12 * i, where[t])
            out[where[t]:where[t] + len(raw)] = raw
    for o, b in zip(offsets, blobs):
        out[o:o + len(b)] = b
    return bytes(out)


def _hand_made(kind, img):
    """planar-2 tiles (16 x 32, LZW with predictor 2) or uncompressed / deflate strips of 7 rows, of an (h, w, c) uint16 image"""
    from satellite_computervision_amd import raster_tools as rt
    h, w, c = img.shape
    base = {256: (4, [w]), 257: (4, [h]), 258: (3, [16] * c), 262: (3, [1]), 277: (3, [c]), 339: (3, [1] * c)}
    if kind == 'planar':
        bh, bw = 16, 32
        blobs = []
        for b in range(c):
            pad = np.zeros((-(-h // bh) * bh, -(-w // bw) * bw), np.uint16)
            pad[:h, :w] = img[..., b]
            for by in range(pad.shape[0] // bh):
                for bx in range(pad.shape[1] // bw):
                    t = pad[by * bh:by * bh + bh, bx * bw:bx * bw + bw].copy()
                    t[:, 1:] = t[:, 1:] - t[:, :-1]
                    blobs.append(rt.lzw_encode(t.tobytes()))
        return _tiff({**base, 259: (3, [5]), 284: (3, [2]), 317: (3, [2]), 322: (4, [bw]), 323: (4, [bh])}, blobs)
    rows = 7 if kind != 'one strip' else h
    strips = [img[y:y + rows].tobytes() for y in range(0, h, rows)]                # the last strip holds only the rows that exist
    if kind == 'deflate strips':
        return _tiff({**base, 259: (3, [8]), 278: (4, [rows])}, [zlib.compress(s) for s in strips])
    if kind == 'lzw strips':
        return _tiff({**base, 259: (3, [5]), 278: (4, [rows])}, [rt.lzw_encode(s) for s in strips])
    return _tiff({**base, 259: (3, [1]), **({} if kind == 'one strip' else {278: (4, [rows])})}, strips)      # 'one strip': no RowsPerStrip at all


@pytest.mark.parametrize('kind', ['planar', 'strips', 'deflate strips', 'lzw strips', 'one strip'])
def test_planar_and_strip_files_assembled_by_hand(tmp_path, kind):
    from satellite_computervision_amd import raster_tools as rt
    img = _image('uint16', 3, 33, 129, seed=4)
    path = str(tmp_path / 'h.tif')
    open(path, 'wb').write(_hand_made(kind, img))
    (info,) = rt.read_info(path)
    assert info.planar == (2 if kind == 'planar' else 1) and info.tiled == (kind == 'planar')
    assert info.block_shape == {'planar': (16, 32), 'one strip': (33, 129)}.get(kind, (7, 129))
    assert np.array_equal(rt.read_cog(path, device=False).array, img)
    w = rt.read_cog(path, window=(9, 30, 20, 70), bands=[2, 0], layout='chw', device=False)
    assert np.array_equal(w.array, img[9:29, 30:100][..., [2, 0]].transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------------------ refusals
def _entry(buf, tag, ifd=0):
    """offset of the 12-byte entry of `tag` in the file"""
    i = TO.parse_tiff(buf)[ifd]
    return i['offset'] + 2 + 12 * i['order'].index(tag)


def test_every_refusal_names_what_the_file_has(tmp_path):
    from satellite_computervision_amd import raster_tools as rt
    good = str(tmp_path / 'good.tif')
    _write(good, _image('uint8', 1), 'lzw', True)
    rgb = str(tmp_path / 'rgb.tif')
    _write(rgb, _image('uint8', 3), None)
    gbuf, rbuf = open(good, 'rb').read(), open(rgb, 'rb').read()
    assert rt.read_info(good) and rt.read_info(rgb)

    made = []

    def patched(buf, at, raw):
        p = str(tmp_path / f'bad{len(made)}.tif')
        made.append(p)
        b = bytearray(buf)
        b[at:at + len(raw)] = raw
        open(p, 'wb').write(b)
        return p

    def value(buf, tag):                                      # where the (inline) value of a tag lies
        return _entry(buf, tag) + 8
    bits3 = struct.unpack_from('<I', rbuf, value(rbuf, 258))[0]           # three shorts lie out of line
    tiles = struct.unpack_from('<I', gbuf, value(gbuf, 324))[0]
    counts = struct.unpack_from('<I', gbuf, value(gbuf, 325))[0]
    cases = [(patched(gbuf, 0, b'MM'), 'big-endian'), (patched(gbuf, 2, struct.pack('<H', 43)), 'BigTIFF'),
             (patched(gbuf, value(gbuf, 259), struct.pack('<H', 7)), 'JPEG'), (patched(gbuf, value(gbuf, 259), struct.pack('<H', 6)), 'JPEG'),
             (patched(gbuf, value(gbuf, 259), struct.pack('<H', 50000)), 'ZSTD'), (patched(gbuf, value(gbuf, 259), struct.pack('<H', 50001)), 'WebP'),
             (patched(gbuf, value(gbuf, 259), struct.pack('<H', 32773)), 'Compression = 32773'),
             (patched(gbuf, value(gbuf, 317), struct.pack('<H', 3)), 'predictor 3'),
             (patched(gbuf, value(gbuf, 258), struct.pack('<H', 4)), '4 bits per sample'), (patched(gbuf, value(gbuf, 258), struct.pack('<H', 64)), '64 bits per sample'),
             (patched(rbuf, bits3 + 2, struct.pack('<H', 16)), 'differing kinds'),
             (patched(gbuf, value(gbuf, 277), struct.pack('<H', 17)), 'more than 16 bands'),
             (patched(gbuf, tiles + 4, struct.pack('<I', len(gbuf) - 3)), 'past the end of the file'),
             (patched(gbuf, counts, struct.pack('<I', len(gbuf))), 'past the end of the file'),
             (patched(gbuf, 4, struct.pack('<I', len(gbuf) + 10)), 'past the end of the file')]
    for path, word in cases:
        for call in (rt.read_info, lambda p: rt.read_cog(p, device=False)):
            with pytest.raises(ValueError, match=re.escape(word)):
                call(path)
    for window in ((60, 0, 20, 20), (0, 80, 5, 11), (-1, 0, 5, 5), (0, 0, 0, 5), (0, 0, 71, 90)):
        with pytest.raises(ValueError, match='outside the image'):
            rt.read_cog(good, window=window, device=False)
    for kw in (dict(level=3), dict(level=-1), dict(bands=[1]), dict(bands=[]), dict(bands=[0, 0]), dict(layout='cwh'), dict(decode='gpu'),
               dict(decode='device'), dict(window=(0, 0, 5)), dict(window=(0.5, 0, 5, 5))):
        with pytest.raises(ValueError):
            rt.read_cog(good, device=False, **kw)
    # a block that does not decode names the block and the status; an LSB-first ("old-style") looking stream is named as such
    b = bytearray(gbuf)
    info = rt.read_info(good)[0]
    at = int(info.offsets[4])
    bits = TO._Bits()
    for code in (256, 65, 300):
        bits.put(code, 9)
    bad = bits.done()
    b[at:at + len(bad)] = bad
    open(good, 'wb').write(b)
    with pytest.raises(ValueError, match=r'block 4 .*status 2 \(bad code\)') as e:
        rt.read_cog(good, device=False)
    assert 'old-style' not in str(e.value)
    b[at] = 0x01
    open(good, 'wb').write(b)
    with pytest.raises(ValueError, match=r"block 4 .*does not open with a Clear.*LSB-first 'old-style' LZW"):
        rt.read_cog(good, device=False)
    with pytest.raises(ValueError, match='differs .* in transform'):
        other = str(tmp_path / 'other.tif')
        _write(other, _image('uint8', 3), None, transform=(10.0, 0.0, 0.0, 0.0, -10.0, 0.0))
        rt.read_stack([rgb, other])


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_untile_descriptor_mirrors_the_header(tmp_path):
    from satellite_computervision_amd import _lib
    D = _lib.UntileDesc
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    body = hdr[hdr.index('typedef struct satcv_untile_desc {'):hdr.index('} satcv_untile_desc;')]
    fields = [n for line in body.splitlines()[1:] for decl in line.split(';') if decl.strip()
              for n in re.sub(r'^\s*(const\s+)?\w+\*?\s+', '', decl.strip()).replace(' ', '').replace('[16]', '').split(',')]
    assert fields == [f[0] for f in D._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(satcv_untile_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(satcv_untile_desc, {f}));' for f, _ in D._fields_] + ['  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / 'layout')], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(D)
    for f, _ in D._fields_:
        assert int(got[f]) == getattr(D, f).offset, f


def test_untile_and_decode_refusals_of_the_c_abi():
    """refused on the host, with a message, before any launch (this test runs without a GPU)"""
    from satellite_computervision_amd import _lib
    lib, D = _lib.lib, _lib.UntileDesc
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)

    def desc(**kw):
        return D(**dict(dict(src=p, src_stride=64, blocks=p, nblocks=1, bh=4, bw=4, across=1, per_plane=1, spp=1, planar=1, kind=0, predictor=0, row0=0,
                             col0=0, h=4, w_=4, dst=p, layout=0, ld=1, coff=0), **kw))
    assert lib.satcv_raster_untile(None, None) == -1
    for d, word in ((desc(src=None), 'null'), (desc(blocks=None), 'null'), (desc(kind=4), 'unknown kind'), (desc(spp=17), 'bands'), (desc(planar=3), 'planar'),
                    (desc(planar=2, per_plane=0), 'planar'), (desc(predictor=1), 'predictor'), (desc(predictor=3), 'predictor'),
                    (desc(kind=2, predictor=2), 'integer kinds'), (desc(layout=2), 'layout'), (desc(row0=-1), 'window'), (desc(h=0), 'positive'),
                    (desc(h=1 << 16, w_=1 << 16), '2^31'), (desc(bh=1 << 20, bw=1 << 20), '2^30'), (desc(src_stride=8), 'src_stride'),
                    (desc(kind=1, src_stride=33), 'src_stride'), (desc(kind=1, src=p + 1), 'misaligned'), (desc(coff=1), 'channel range'),
                    (desc(band_map=(ctypes.c_int32 * 16)(1)), 'band_map'), (desc(band_map=(ctypes.c_int32 * 16)(-1)), 'keeps no band')):
        assert lib.satcv_raster_untile(ctypes.byref(d), None) == -1, word
        assert word.encode() in lib.satcv_last_error(), (word, lib.satcv_last_error())
    for args, word in (((None, 16, p, p, 1, 16, p, 16, p, None, None), 'null'), ((p, 16, p, p, 0, 16, p, 16, p, None, None), 'blocks'),
                       ((p, 0, p, p, 1, 16, p, 16, p, None, None), 'payload_bytes'), ((p, 16, p, p, 1, 1 << 30, p, 1 << 30, p, None, None), '2^30'),
                       ((p, 16, p, p, 1, 16, p, 8, p, None, None), 'dst_stride'), ((p, 16, p + 4, p, 1, 16, p, 16, p, None, None), 'misaligned')):
        assert lib.satcv_lzw_decode_tiles(*args) == -1 and word.encode() in lib.satcv_last_error(), (word, lib.satcv_last_error())


def test_host_decoder_on_malformed_streams_under_asan_ubsan(tmp_path):
    """tests/asan/lzw_decode_driver.c, a stand-alone program, against the sanitizer-built host-only library (build.py::build_host_asan),
    linked in the normal way as tests/test_raster_cpu.py drives raster_host_driver.c: every truncation, every bit flip, planted codes, short
    caps, a full table.  Any sanitizer report aborts the driver.  tests/test_raster_read_gpu.py runs malformed blocks on the device."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('_satcv_build', os.path.join(ROOT, 'satellite_computervision_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    so = b.build_host_asan()
    exe = tmp_path / 'lzw_decode_driver'
    clang = '/opt/rocm/lib/llvm/bin/clang'
    subprocess.run([clang, '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-g', '-O1', '-I', os.path.join(ROOT, 'include'),
                    os.path.join(ROOT, 'tests', 'asan', 'lzw_decode_driver.c'), '-o', str(exe), '-L', os.path.dirname(so), '-lsatcv_hostasan',
                    '-Wl,-rpath,' + os.path.dirname(so)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1'),
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-4000:]
    assert ' 0 failures' in r.stdout, r.stdout


def test_new_entries_keep_the_older_signatures():
    import inspect
    from satellite_computervision_amd import prediction_tools as pt, raster_tools as rt
    assert list(inspect.signature(rt.read_cog).parameters) == ['path', 'window', 'level', 'bands', 'layout', 'device', 'decode', 'out']
    assert list(inspect.signature(rt.read_stack).parameters) == ['paths', 'window', 'bands']
    assert list(inspect.signature(pt.predict_raster).parameters)[:4] == ['in_file', 'm', 'out_file', 'window']
    assert list(inspect.signature(rt.write_cog).parameters)[:4] == ['arr', 'out_file', 'transform', 'crs']


def test_the_container_module_needs_neither_torch_nor_the_library():
    """`import satellite_computervision_amd.tiff_container` in a fresh interpreter loads neither torch nor the ctypes binding.  The
    package's own __init__ loads the library on purpose (there is no CPU fallback), so the child registers a bare namespace for the
    package first: what is held is that the module itself, and whatever it imports, needs neither."""
    code = ("import sys, types\n"
            f"pkg = types.ModuleType('satellite_computervision_amd'); pkg.__path__ = [{os.path.join(ROOT, 'satellite_computervision_amd')!r}]\n"
            "sys.modules['satellite_computervision_amd'] = pkg\n"
            "import satellite_computervision_amd.tiff_container as tc\n"
            "assert callable(tc.read_info) and callable(tc.build_container) and tc.LevelInfo.block_bytes\n"
            "bad = [m for m in sys.modules if m == 'torch' or m.startswith('torch.') or m.startswith('satellite_computervision_amd.') and m != tc.__name__]\n"
            "assert not bad, bad\n")
    import sys
    done = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
