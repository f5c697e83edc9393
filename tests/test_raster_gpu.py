"""GPU checks of the Cloud-Optimized GeoTIFF writer (csrc/raster.hip, satellite_computervision_amd/raster_tools.py): every kernel exact
against the NumPy restatement of tests/tiff_oracle.py, the device LZW byte for byte against the host coder, and files written from device
maps read back by the helper parser.  Shapes are the smallest that reach every branch: odd sizes, sizes that are no multiple of the tile,
more tiles than are resident at once, the 4094 reset and all three width steps of the coder."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KIND = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3, np.dtype(np.int32): 5}
TRANSFORM = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)


@pytest.fixture(scope='module')
def env():
    import tiff_oracle as TO
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, pc_tools as pc, raster_tools as rt, _lib
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pt=pt, pc=pc, rt=rt, L=_lib, TO=TO)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _out(shape, dtype):
    """a byte buffer for a result of `shape` and `dtype` (uint16 has no torch dtype everywhere: results come back as bytes)"""
    return torch.empty(tuple(shape[:-1]) + (shape[-1] * np.dtype(dtype).itemsize,), dtype=torch.uint8, device='cuda')


def _desc(env, src, src_dt, h, w, c, ld, coff, dst, dst_dt, **kw):
    nodata = kw.pop('nodata', None)
    return env['L'].RasterDesc(src=src.data_ptr(), src_kind=KIND[np.dtype(src_dt)], h=h, w_=w, c=c, ld=ld, coff=coff, dst=dst.data_ptr(),
                               dst_kind=KIND[np.dtype(dst_dt)], has_nodata=int(nodata is not None), nodata=float(nodata or 0), **kw)


def _call(env, name, *args):
    env['L'].check(getattr(env['L'].lib, name)(*args))


# ---------------------------------------------------------------------------------------------------------------- 1. convert
def _convert_source(rng, dtype, h, w, ld):
    dt = np.dtype(dtype)
    if dt == np.float32:
        a = (rng.random((h, w, ld)) * 3.2 - 0.3).astype(np.float32)                 # x 100: -30 ... 290, below 0 and above 255
        special = np.array([np.nan, -3.2, 0.5, 1.5, 2.5, 254.5, 300.0, 0.005, 0.015, 0.025, 2.545, 2.555, -0.005, np.inf, -np.inf, 3e9, -3e9, 655.345],
                           np.float32)
        a.reshape(-1)[:special.size * 7:7] = special
        a[5, 3:10, :] = special[:7, None]                                             # the issue's values in every band, as they are
        a[rng.random(a.shape) < 0.05] = np.nan
        a[7, :, :] = (np.arange(w, dtype=np.float32)[:, None] + 0.5) / 100          # exact halves after the multiply (where fp32 allows)
        return a
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max + 1, (h, w, ld), dtype=np.int64).astype(dt)
    a.reshape(-1)[:6] = np.array([info.min, info.max, 0, 255, 256, 1], np.int64).astype(dt)
    return a


@pytest.mark.parametrize('src_dt,dst_dt,scale', [(np.float32, np.uint8, 100.0), (np.float32, np.uint8, None), (np.float32, np.uint16, 100.0),
                                                 (np.float32, np.float32, 100.0), (np.float32, np.int32, 1e7), (np.int32, np.uint8, None),
                                                 (np.uint16, np.int16, None), (np.int16, np.float32, None), (np.uint8, np.int32, None)])
@pytest.mark.parametrize('c', [1, 3])
def test_convert_equals_the_oracle(env, src_dt, dst_dt, scale, c):
    TO = env['TO']
    h, w, ld, coff = 37, 53, 5, 1
    src = _convert_source(np.random.default_rng(3), src_dt, h, w, ld)
    if src_dt == np.float32 and scale is None:
        src = src * np.float32(100)
    for nodata in (255, None):
        want = TO.convert_ref(src[..., coff:coff + c], dst_dt, scale, nodata)
        d_src, d_dst = _dev(src), _out((h, w, c), dst_dt)
        _call(env, 'satcv_raster_convert', C.byref(_desc(env, d_src, src_dt, h, w, c, ld, coff, d_dst, dst_dt, scale=float(scale or 0), nodata=nodata)), env['ops'].stream_ptr())
        got = _host(d_dst, dst_dt).reshape(h, w, c)
        assert np.array_equal(got, want, equal_nan=True), (nodata, np.argwhere(got != want)[:5])
    if src_dt == np.float32 and dst_dt == np.uint8 and scale:
        v = TO.convert_ref(np.array([np.nan, -3.2, 0.5, 1.5, 2.5, 254.5, 300.0], np.float32).reshape(1, -1, 1), np.uint8, None, 255).ravel().tolist()
        assert v == [255, 0, 0, 2, 2, 254, 255]             # NaN -> nodata, saturation, half to even


# ---------------------------------------------------------------------------------------------------------------- 2. overviews
def _overview_chain(env, base, resampling, nodata):
    """every level down to 1 x 1 on the device, cascading: -> [level 1, level 2, ...]"""
    dt = base.dtype
    h, w, c = base.shape
    cur, levels = _dev(base), []
    while max(h, w) > 1:
        oh, ow = (h + 1) // 2, (w + 1) // 2
        nxt = _out((oh, ow, c), dt)
        _call(env, 'satcv_raster_overview', C.byref(_desc(env, cur, dt, h, w, c, c, 0, nxt, dt, resampling={'nearest': 0, 'average': 1, 'mode': 2}[resampling], nodata=nodata)),
              env['ops'].stream_ptr())
        levels.append(_host(nxt, dt).reshape(oh, ow, c))
        cur, h, w = nxt, oh, ow
    return levels


def _class_map(rng, h, w, c):
    a = rng.integers(0, 4, (h, w, c)).astype(np.uint8)                              # few classes: ties are everywhere
    a[rng.random(a.shape) < 0.25] = 255
    a[0:4, 0:6] = 255                                                                # blocks (and overview blocks) without a valid sample
    a[4:6, 0:2, 0] = [[1, 2], [2, 1]]                                                # a 2-2 tie: the smallest
    a[4:6, 2:4, 0] = [[3, 3], [0, 0]]
    a[6:8, 0:2, 0] = [[255, 7], [255, 255]]                                          # one valid sample
    return a


@pytest.mark.parametrize('shape', [(37, 53, 3), (64, 64, 1)])
@pytest.mark.parametrize('resampling', ['nearest', 'average', 'mode'])
def test_overviews_on_uint8_with_scattered_nodata(env, shape, resampling):
    TO = env['TO']
    base = _class_map(np.random.default_rng(5), *shape)
    for nodata in (255, None):
        got = _overview_chain(env, base, resampling, nodata)
        assert got[-1].shape[:2] == (1, 1)
        want = base
        for k, g in enumerate(got):
            want = TO.overview_ref(want, resampling, nodata)                         # the cascade of the oracle, level by level
            assert np.array_equal(g, want), (nodata, k, np.argwhere(g != want)[:5])
    if resampling != 'nearest':
        assert (TO.overview_ref(base, resampling, 255)[0:2, 0:3] == 255).all()


@pytest.mark.parametrize('dtype,resampling', [(np.float32, 'average'), (np.float32, 'nearest'), (np.int16, 'average'), (np.int32, 'mode'), (np.uint16, 'average')])
def test_overviews_of_the_other_kinds(env, dtype, resampling):
    TO = env['TO']
    rng = np.random.default_rng(6)
    h, w, c = 37, 53, 2
    if dtype == np.float32:
        base = (rng.standard_normal((h, w, c)) * 1000).astype(np.float32)
        base[rng.random(base.shape) < 0.3] = np.nan
        base[10:14, 10:14] = np.nan                                                  # blocks of NaN only
        base[rng.random(base.shape) < 0.05] = -9999.0
        nodatas = (None, -9999.0)
    else:
        info = np.iinfo(dtype)
        base = rng.integers(max(info.min, -40000), min(info.max, 40000), (h, w, c)).astype(dtype)      # negative sums: the floor
        base[rng.random(base.shape) < 0.3] = 255
        base[10:14, 10:14] = 255
        if resampling == 'mode':
            base[20:30] = rng.integers(-2, 2, (10, w, c))
        nodatas = (255, None)
    for nodata in nodatas:
        got = _overview_chain(env, base, resampling, nodata)
        want = base
        for k, g in enumerate(got):
            want = TO.overview_ref(want, resampling, nodata)
            assert np.array_equal(g.view('u%d' % g.itemsize), want.view('u%d' % want.itemsize)) or np.array_equal(g, want, equal_nan=True), (nodata, k)


# ---------------------------------------------------------------------------------------------------------------- 3. tiles
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('bs', [32, 16])
def test_tiles_equal_the_oracle(env, dtype, c, bs):
    TO = env['TO']
    rng = np.random.default_rng(7)
    h, w = 70, 90
    if dtype == np.float32:
        base = rng.standard_normal((h, w, c)).astype(np.float32)
    else:
        base = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, c)).astype(dtype)     # differences wrap in both directions
    for predictor in ((False, True) if dtype != np.float32 else (False,)):
        for nodata in (255, None):
            want = TO.tiles_ref(base, bs, predictor, nodata)
            dst = _out(want.shape, dtype)
            _call(env, 'satcv_raster_tiles', C.byref(_desc(env, _dev(base), dtype, h, w, c, c, 0, dst, dtype, blocksize=bs, predictor=int(predictor), nodata=nodata)),
                  env['ops'].stream_ptr())
            got = _host(dst, dtype).reshape(want.shape)
            assert got.shape[0] == -(-h // bs) * -(-w // bs)
            assert np.array_equal(got.view('u%d' % got.itemsize), want.view('u%d' % want.itemsize)), (predictor, nodata)


# ---------------------------------------------------------------------------------------------------------------- 4. LZW
def _host_lzw(env, tile):
    return env['rt'].lzw_encode(tile.tobytes())


def _lzw_on_device(env, tiles):
    n, tb = tiles.shape[0], int(np.prod(tiles.shape[1:]))
    slot = 2 * tb + 16
    d_tiles = _dev(tiles.reshape(n, tb))
    slots = torch.full((n, slot), 0xee, dtype=torch.uint8, device='cuda')
    sizes = torch.full((n,), -1, dtype=torch.int32, device='cuda')
    _call(env, 'satcv_lzw_tiles', d_tiles.data_ptr(), n, tb, slots.data_ptr(), sizes.data_ptr(), env['ops'].stream_ptr())
    return slots, sizes


def _check_lzw(env, tiles):
    slots, sizes = _lzw_on_device(env, tiles)
    got, sz = slots.cpu().numpy(), sizes.cpu().numpy()
    for i in range(tiles.shape[0]):
        want = _host_lzw(env, tiles[i])
        assert sz[i] == len(want), (i, sz[i], len(want))
        assert got[i, :sz[i]].tobytes() == want, i
    return slots, sizes, got, sz


def test_lzw_of_many_small_tiles_equals_the_host_coder(env):
    """1100 tiles of 64 x 64 uint8 -- more than the 4 x 256 that are resident at once -- constant, class grids, smooth, random.  A random
    tile of 4096 bytes passes the three width steps; the doubled random tiles pass the 4094 reset"""
    TO = env['TO']
    rng = np.random.default_rng(8)
    n = 1100
    tiles = np.empty((n, 64, 64), np.uint8)
    for i in range(n):
        k = i % 5
        if k == 0:
            tiles[i] = i % 251
        elif k == 1:
            tiles[i] = np.kron(rng.integers(0, 5, (8, 8)), np.ones((8, 8))).astype(np.uint8)
        elif k == 2:
            tiles[i] = rng.integers(0, 256, (64, 64))
        elif k == 3:
            tiles[i] = (np.add.outer(np.arange(64), np.arange(64)) // 3 + rng.integers(0, 2, (64, 64))) % 256
        else:
            tiles[i] = rng.integers(0, 3, (64, 64))
    info = {}
    TO.lzw_encode_ref(tiles[2].tobytes(), info)
    assert info['clears'] >= 1                              # 4096 random bytes: more than 3836 codes, so the 4094 reset and every width
    _check_lzw(env, tiles)


def test_lzw_of_large_tiles_and_compaction(env):
    """8 tiles of 128 x 128 x 3 uint8 (many input chunks and output flushes, several resets), then satcv_bytes_compact of their streams to
    even offsets inside a buffer with sentinels around and between"""
    rng = np.random.default_rng(9)
    tiles = np.empty((8, 128, 128, 3), np.uint8)
    tiles[0] = 9
    tiles[1] = rng.integers(0, 256, tiles[1].shape)
    tiles[2] = np.kron(rng.integers(0, 6, (16, 16, 1)), np.ones((8, 8, 3))).astype(np.uint8)
    tiles[3] = rng.integers(0, 2, tiles[3].shape)
    tiles[4] = (np.arange(128 * 128 * 3) % 253).reshape(128, 128, 3)
    tiles[5] = rng.integers(0, 256, tiles[5].shape)
    tiles[6] = np.repeat(rng.integers(0, 256, (128, 16, 3)), 8, axis=1)
    tiles[7] = rng.integers(0, 16, tiles[7].shape) * 16
    slots, sizes, got, sz = _check_lzw(env, tiles)
    assert sz.max() > tiles[0].size                         # random data expands: the slot of 2 x + 16 is needed
    lead, n = 64, len(sz)
    offs, pos = [], lead
    for s in sz[::-1]:                                      # any order of the offsets: here the last tile first, with gaps
        pos += pos & 1
        offs.append(pos)
        pos += int(s) + 3
    offs = np.array(offs[::-1], np.int64)
    total = pos + 64
    buf = torch.full((total,), 0x77, dtype=torch.uint8, device='cuda')
    _call(env, 'satcv_bytes_compact', slots.data_ptr(), slots.shape[1], sizes.data_ptr(), _dev(offs).data_ptr(), n, buf.data_ptr(), total, env['ops'].stream_ptr())
    out = buf.cpu().numpy()
    want = np.full(total, 0x77, np.uint8)
    for i in range(n):
        want[offs[i]:offs[i] + sz[i]] = got[i, :sz[i]]
    assert np.array_equal(out, want)
    # a destination that ends inside the last placed stream: nothing is written past dst_bytes
    short = int(offs.max() + 5)
    buf.fill_(0x77)
    _call(env, 'satcv_bytes_compact', slots.data_ptr(), slots.shape[1], sizes.data_ptr(), _dev(offs).data_ptr(), n, buf.data_ptr(), short, env['ops'].stream_ptr())
    out = buf.cpu().numpy()
    assert (out[short:] == 0x77).all() and np.array_equal(out[:short], want[:short])


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def _read(TO, path):
    buf = open(path, 'rb').read()
    ifds = TO.parse_tiff(buf)
    return buf, ifds, [TO.read_level(buf, i) for i in ifds]


@pytest.mark.parametrize('compress,predictor', [('lzw', True), ('lzw', False), ('deflate', False), (None, False)])
def test_write_cog_from_device_maps(env, tmp_path, compress, predictor):
    TO, rt = env['TO'], env['rt']
    rng = np.random.default_rng(10)
    H, W, bs = 200, 300, 64
    shapes = TO.auto_shapes(H, W, bs)
    assert shapes == [(100, 150), (50, 75), (25, 38)]
    # a uint8 class map, as predict_scene(..., classes=True, device=True) returns it: 255 where nothing is predicted
    cls = np.kron(rng.integers(0, 4, (25, 38)), np.ones((8, 8))).astype(np.uint8)[:H, :W]
    cls[:16] = 255
    cls[:, -16:] = 255
    path = str(tmp_path / 'cls.tif')
    assert rt.write_cog(_dev(cls), path, TRANSFORM, 'EPSG:32618', compress=compress, predictor=predictor, blocksize=bs, resampling='mode') == path
    buf, ifds, levels = _read(TO, path)
    want = TO.pyramid_ref(cls[..., None], shapes, 'mode', 255)
    assert len(levels) == 4 and all(np.array_equal(g, w) for g, w in zip(levels, want))
    t0 = ifds[0]['tags']
    assert t0[259][2] == ({'lzw': 5, 'deflate': 8, None: 1}[compress],) and (317 in t0) == predictor and t0[42113][2] == b'255\0'
    assert t0[33550][2] == (10.0, 10.0, 0.0) and t0[33922][2] == (0.0, 0.0, 0.0, 399960.0, 4500000.0, 0.0)
    assert t0[34735][2] == (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 32618)
    assert [TO.tag(i, 254)[0] for i in ifds] == [0, 1, 1, 1] and all(TO.tag(i, 322) == (bs,) for i in ifds)
    first_tile = min(min(TO.tag(i, 324)) for i in ifds)
    assert all(i['end'] <= first_tile and all(hi <= first_tile for _, hi in i['value_spans']) for i in ifds)
    flat = [o for i in reversed(ifds) for o in TO.tag(i, 324)]
    assert flat == sorted(flat) and all(o % 2 == 0 for o in flat)
    # a float32 probability map with NaN: a channel slice of a (H, W, 3) tensor, read where it lies
    prob = rng.random((H, W, 3)).astype(np.float32)
    prob[rng.random(prob.shape) < 0.1] = np.nan
    t = _dev(prob)
    if predictor:
        with pytest.raises(ValueError):
            rt.write_cog(t[..., 1], path, TRANSFORM, 4326, compress=compress, predictor=True, blocksize=bs)
    else:
        rt.write_cog(t[..., 1], path, (1e-4, 0.0, -77.0, 0.0, -1e-4, 39.0), 4326, compress=compress, blocksize=bs, resampling='average', nodata=None)
        buf, ifds, levels = _read(TO, path)
        want = TO.pyramid_ref(prob[..., 1:2], shapes, 'average', None)
        assert len(levels) == 4 and all(np.array_equal(g, w, equal_nan=True) for g, w in zip(levels, want))
        assert ifds[0]['tags'][34735][2][-4:] == (2048, 0, 1, 4326) and 42113 not in ifds[0]['tags']
    # probabilities x 100 into uint8, two bands of the three, with the predictor where it applies
    rt.write_cog(t[..., 1:3], path, TRANSFORM, 32618, dtype='uint8', scale=100.0, compress=compress, predictor=predictor, blocksize=bs, resampling='average')
    buf, ifds, levels = _read(TO, path)
    want = TO.pyramid_ref(TO.convert_ref(prob[..., 1:3], np.uint8, 100.0, 255), shapes, 'average', 255)
    assert all(np.array_equal(g, w) for g, w in zip(levels, want)) and ifds[0]['tags'][338][2] == (0,)
    # a host array takes the same path
    rt.numpy_to_raster(cls, {'transform': list(TRANSFORM) + [0, 0, 1], 'crs': 'EPSG:32618', 'cols': W, 'rows': H}, path, 'uint8')
    _, ifds, levels = _read(TO, path)
    assert np.array_equal(levels[0][..., 0], cls) and TO.tag(ifds[0], 322) == (512,) and TO.tag(ifds[0], 259) == (5,) and len(ifds) == 1


def test_pillow_reads_a_file_written_from_the_device(env, tmp_path):
    from PIL import Image
    rt = env['rt']
    img = (np.add.outer(np.arange(150), np.arange(201)) % 251).astype(np.uint8)
    path = str(tmp_path / 'p.tif')
    rt.write_cog(_dev(img), path, TRANSFORM, 32618, predictor=True, blocksize=64)
    with Image.open(path) as im:
        assert im.n_frames == 3 and np.array_equal(np.asarray(im), img)


def _randomise(m, seed):
    rng = np.random.default_rng(seed)
    w = {}
    for ps in m.param_specs:
        if ps.kind == 'kernel':
            w[ps.name] = (rng.standard_normal(ps.shape) * np.sqrt(2.0 / np.prod(ps.shape[:3]))).astype(np.float32)
        elif ps.kind == 'moving_var':
            w[ps.name] = (0.5 + rng.random(ps.shape)).astype(np.float32)
        elif ps.kind == 'gamma':
            w[ps.name] = (1 + 0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
        else:
            w[ps.name] = (0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
    m.set_weights_dict(w)


def _unet(mt, channels):
    mt.reset_uids(); mt.set_seed(6)
    m = mt.get_unet_model(2, channels, filters=[32, 64], factors=[2, 2])
    m.compute_dtype = 'bfloat16'
    _randomise(m, 6)
    return m


def test_predict_scene_device_results_equal_the_host_results(env, tmp_path):
    mt, pt, rt, TO = env['mt'], env['pt'], env['rt'], env['TO']
    rng = np.random.default_rng(11)
    m = _unet(mt, 4)
    scene = rng.random((200, 260, 4)).astype(np.float32)
    kw = dict(kernel=64, buff=32, batch_size=8)
    for extra in (dict(channel=1, classes=True), dict(channel=None), dict(channel=0, cover='full')):
        host = pt.predict_scene(scene, m, **kw, **extra)
        dev = pt.predict_scene(scene, m, device=True, **kw, **extra)
        host, dev = (host, dev) if isinstance(host, tuple) else ((host,), (dev,))
        assert len(host) == len(dev)
        for h, d in zip(host, dev):
            assert isinstance(d, torch.Tensor) and d.is_cuda and tuple(d.shape) == h.shape and np.array_equal(d.cpu().numpy(), h)
    probs, cls = pt.predict_scene(scene, m, device=True, classes=True, channel=1, **kw)
    assert cls.dtype == torch.uint8 and int(cls[0, 0]) == 255 and int((cls != 255).sum()) > 0
    # ... and they reach the writer without a round trip: the strided (H, W) views are read where they lie
    path = str(tmp_path / 'm.tif')
    rt.write_cog(cls, path, TRANSFORM, 32618, blocksize=64, resampling='mode')
    _, _, levels = _read(TO, path)
    assert np.array_equal(levels[0][..., 0], cls.cpu().numpy())
    rt.write_cog(probs, path, TRANSFORM, 32618, dtype='uint8', scale=100.0, blocksize=64)
    _, _, levels = _read(TO, path)
    assert np.array_equal(levels[0], TO.convert_ref(probs.cpu().numpy()[..., None], np.uint8, 100.0, 255))
    tiny = pt.predict_scene(scene[:50, :50], m, device=True, classes=True, **kw)            # too small for one chip: nothing predicted
    assert tiny[0].is_cuda and float(tiny[0].abs().sum()) == 0 and bool((tiny[1] == 255).all())
    idx = pt.generate_chip_indices(scene, 32, 64)
    want = pt.predict_chips_device(scene, idx, np.zeros(scene.shape[:2]), m, **kw)
    got = pt.predict_chips_device(scene, idx, None, m, device=True, **kw)
    assert got.is_cuda and np.array_equal(got.cpu().numpy().astype(np.float64), want)


def test_predict_change_writes_its_map(env, tmp_path):
    mt, pc, TO = env['mt'], env['pc'], env['TO']
    rng = np.random.default_rng(12)
    H, W, c = 200, 230, 4
    before = rng.integers(1, 6000, (3, c, H, W)).astype(np.uint16)
    after = rng.integers(1, 9000, (4, c, H, W)).astype(np.uint16)
    m = _unet(mt, 8)
    kw = dict(buff=32, kernel=64, batch_size=8, fill=0.0)
    plain = pc.predict_change(before, after, m, **kw)
    path = str(tmp_path / 'change.tif')
    out = pc.predict_change(before, after, m, out_file=path, transform=TRANSFORM, crs='EPSG:32618', cog_options=dict(dtype='float32', blocksize=64), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(plain, out))            # the return value is unchanged
    _, ifds, levels = _read(TO, path)
    assert levels[0].dtype == np.float32 and np.array_equal(levels[0][..., 0], out[0]) and out[0].max() > 0
    assert len(ifds) == 3 and TO.tag(ifds[0], 259) == (5,)
    with pytest.raises(ValueError):
        pc.predict_change(before, after, m, out_file=path, **kw)
    with pytest.raises(ValueError):
        pc.predict_change(before, after, m, transform=TRANSFORM, **kw)


def test_write_geotiff_predictions_from_a_mixer(env, tmp_path):
    import json
    mt, pt, TO = env['mt'], env['pt'], env['TO']
    rng = np.random.default_rng(13)
    m = _unet(mt, 4)
    patches = rng.random((6, 96, 96, 4)).astype(np.float32)
    mixer = {'patchesPerRow': 3, 'totalPatches': 6, 'patchDimensions': [64, 64],
             'projection': {'crs': 'EPSG:32618', 'affine': {'doubleMatrix': [10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0]}}}
    jf = str(tmp_path / 'mixer.json')
    json.dump(mixer, open(jf, 'w'))
    path = pt.write_geotiff_predictions(patches, m, jf, 'pred', str(tmp_path), kernel_buffer=[32, 32])
    assert path == str(tmp_path / 'pred.tif')
    _, ifds, levels = _read(TO, path)
    probs = m.predict(patches, batch_size=16)[0]
    want = np.zeros((128, 192), np.float32)
    for i in range(6):
        want[(i // 3) * 64:(i // 3 + 1) * 64, (i % 3) * 64:(i % 3 + 1) * 64] = probs[i, 16:80, 16:80, 0]
    assert len(ifds) == 1 and TO.tag(ifds[0], 259) == (1,) and 42113 not in ifds[0]['tags'] and np.array_equal(levels[0][..., 0], want)
    image = rng.integers(0, 30000, (70, 90, 2)).astype(np.int16)
    assert pt.write_geotiff_prediction(image, jf, str(tmp_path / 'aoi')) == str(tmp_path / 'aoi') + '.tif'
    _, ifds, levels = _read(TO, str(tmp_path / 'aoi.tif'))
    assert len(ifds) == 1 and levels[0].dtype == np.int16 and np.array_equal(levels[0], image) and TO.tag(ifds[0], 322) == (96,)


def test_to_float32_is_exact(env):
    """raster_tools.to_float32 (satcv_raster_convert on a raster or a stack of any rank) equals the NumPy cast: every integer kind with its
    extremes, int32 within +-2^24, which float32 holds exactly"""
    rt = env['rt']
    rng = np.random.default_rng(5)
    for dtype in (np.uint8, np.uint16, np.int16, np.int32):
        lo, hi = max(np.iinfo(dtype).min, -2 ** 24), min(np.iinfo(dtype).max, 2 ** 24)
        for shape in ((5, 7, 3), (2, 3, 5, 7)):
            a = rng.integers(lo, hi, shape, dtype=np.int64, endpoint=True).astype(dtype)
            a.flat[:4] = [lo, hi, 0, lo + 1]
            got = rt.to_float32(_dev(a), np.dtype(dtype).name)
            assert got.dtype == torch.float32 and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), a.astype(np.float32))
            if len(shape) == 3:                                # (the same tensor described to the kernel as an (H, W, C) raster)
                assert torch.equal(rt.to_float32(_dev(a), np.dtype(dtype).name, as_raster=True), got)
