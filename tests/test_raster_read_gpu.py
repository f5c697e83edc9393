"""GPU checks of the GeoTIFF / COG reader (csrc/raster.hip satcv_lzw_decode_tiles and satcv_raster_untile; raster_tools.read_cog, read_stack;
prediction_tools.predict_raster): the device decoder byte for byte against the host decoder and the source bytes, on many small blocks
at odd offsets, on 2 MB blocks whose strings outgrow the LDS ring, on libtiff's streams and on malformed ones; the untile kernel against a
NumPy restatement in this file; files written by write_cog read back bit for bit; stacks; file -> prediction -> file.  Every comparison
is exact: decoding is integer work.  Shapes are the smallest that reach every branch."""
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
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tiff_read')
WINDOW = (17, 5, 40, 61)
CANARY = 0x5a


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
    """the bytes of a device tensor as `dtype` (uint16 tensors travel as bytes)"""
    return t.contiguous().view(torch.uint8).cpu().numpy().view(dtype).reshape(tuple(t.shape))


# ---------------------------------------------------------------------------------------------------------------- 1. the decoder
def _decode(env, streams, block_bytes, stride, lead=3):
    """one satcv_lzw_decode_tiles launch over `streams`, packed at odd, unequal offsets behind `lead` bytes; every slot is block_bytes
    followed by stride - block_bytes canary bytes -> (slots (n, stride) uint8, status, lengths)"""
    n = len(streams)
    offs, pos = [], lead
    for k, s in enumerate(streams):
        offs.append(pos)
        pos += len(s) + (1, 2, 4, 7)[k % 4]                   # gaps of changing parity: no slice start is aligned on purpose
    payload = np.full(pos + 5, 0xee, np.uint8)
    for o, s in zip(offs, streams):
        payload[o:o + len(s)] = np.frombuffer(bytes(s), np.uint8)
    d_payload, d_offs, d_sizes = _dev(payload), _dev(np.array(offs, np.int64)), _dev(np.array([len(s) for s in streams], np.int32))
    slots = torch.full((n, stride), CANARY, dtype=torch.uint8, device='cuda')
    flags = torch.full((2 * n,), -7, dtype=torch.int32, device='cuda')
    L = env['L']
    L.check(L.lib.satcv_lzw_decode_tiles(d_payload.data_ptr(), payload.size, d_offs.data_ptr(), d_sizes.data_ptr(), n, block_bytes, slots.data_ptr(), stride,
                                         flags.data_ptr(), flags.data_ptr() + 4 * n, env['ops'].stream_ptr()))
    torch.cuda.synchronize()
    f = flags.cpu().numpy()
    return slots.cpu().numpy(), f[:n], f[n:]


def _check_blocks(env, datas, block_bytes, stride, encode=None):
    rt = env['rt']
    streams = [(encode or rt.lzw_encode)(d) for d in datas]
    slots, status, lengths = _decode(env, streams, block_bytes, stride)
    for i, (d, s) in enumerate(zip(datas, streams)):
        st, want = rt.lzw_decode(s, block_bytes)              # the host decoder, the same core
        assert st == 0 and want == bytes(d), i
        assert status[i] == 0 and lengths[i] == len(d), (i, status[i], lengths[i], len(d))
        assert slots[i, :len(d)].tobytes() == want, i
        assert (slots[i, len(d):] == CANARY).all(), i         # nothing past the decoded length, nothing past the block


def _small_block(rng, i):
    size = (256, 1024, 2048, 8192)[i % 4]                     # 16 x 16 u8 ... 32 x 32 x 4 u16
    what = i % 5
    if what == 0:
        return rng.integers(0, 256, size, dtype=np.uint8).tobytes()
    if what == 1:
        return np.kron(rng.integers(0, 4, size // 64, dtype=np.uint8), np.ones(64, np.uint8)).tobytes()
    if what == 2:
        return bytes(size)
    if what == 3:
        return (rng.integers(0, 40, size // 2) + 1000 + np.arange(size // 2)).astype(np.uint16).tobytes()
    return (np.arange(size) % 251).astype(np.uint8).tobytes()


def test_many_small_blocks_in_one_launch_equal_the_host_decoder(env):
    rng = np.random.default_rng(21)
    datas = [_small_block(rng, i) for i in range(300)]
    _check_blocks(env, datas, 8192, 8192 + 32)                # 16-byte aligned slots: the 16-byte store path
    _check_blocks(env, datas[:40], 8192, 8192 + 37)           # slots at odd addresses: the byte store path


def test_large_blocks_whose_strings_outgrow_the_ring(env):
    """512 x 512 x 4 u16 = 2 MB per block: zeros (strings of thousands of bytes, their sources long flushed: the global source path and copy
    rounds beyond 64 bytes), noise (the table fills again and again), a ramp, a class map with large uniform patches"""
    rng = np.random.default_rng(22)
    n = 512 * 512 * 4 * 2
    cls = np.kron(rng.integers(0, 5, (8, 8)), np.ones((64, 64))).astype(np.uint16)
    datas = [bytes(n), rng.integers(0, 256, n, dtype=np.uint8).tobytes(), (np.arange(n // 2) % 65536).astype(np.uint16).tobytes(),
             np.repeat(cls[..., None], 4, axis=2).tobytes()]
    assert all(len(d) == n for d in datas)
    _check_blocks(env, datas, n, n + 64)


def test_streams_without_eoi_and_without_the_leading_clear(env):
    TO, rt = env['TO'], env['rt']
    rng = np.random.default_rng(23)
    data = rng.integers(0, 7, 5000, dtype=np.uint8).tobytes()
    ref = TO.lzw_encode_ref(data)
    total = len(ref) * 8 - 9
    no_clear = ((int.from_bytes(ref, 'big') & ((1 << total) - 1)) << (-total % 8)).to_bytes((total + (-total % 8)) // 8, 'big')
    streams = [ref, ref[:-2], no_clear, ref]
    want = [TO.lzw_decode(s) for s in streams]
    assert want[0] == want[2] == data and data.startswith(want[1])
    slots, status, lengths = _decode(env, streams, 5000, 5000 + 24)
    assert status.tolist() == [0, 1 if len(want[1]) < 5000 else 0, 0, 0]          # (cut inside the last data code: input ends before the block is full)
    for i in range(4):
        assert lengths[i] == len(want[i]) and slots[i, :lengths[i]].tobytes() == want[i] and (slots[i, lengths[i]:] == CANARY).all()
        assert rt.lzw_decode(streams[i], 5000) == (int(status[i]), want[i])


def test_libtiff_streams_decode_on_the_device(env):
    TO, rt = env['TO'], env['rt']
    z = np.load(os.path.join(GOLD, 'expected.npz'))
    for name in z.files:
        path = os.path.join(GOLD, name + '.tif')
        buf = open(path, 'rb').read()
        (ifd,) = TO.parse_tiff(buf)
        (info,) = rt.read_info(path)
        streams = [buf[o:o + n] for o, n in zip(TO.tag(ifd, 273), TO.tag(ifd, 279))]
        want = z[name] if z[name].ndim == 3 else z[name][..., None]
        block_bytes = info.block_shape[0] * info.block_shape[1] * info.bands * want.dtype.itemsize
        slots, status, lengths = _decode(env, streams, block_bytes, block_bytes + 19)
        rows = 0
        for i, s in enumerate(streams):
            host = TO.lzw_decode(s)
            assert status[i] == 0 and lengths[i] == len(host) and slots[i, :len(host)].tobytes() == host, (name, i)
            if not info.predictor:
                part = want[rows:rows + info.block_shape[0]]
                assert host == part.tobytes(), (name, i)
                rows += part.shape[0]
        got = rt.read_cog(path, device=True, decode='device')
        assert got.array.is_cuda and np.array_equal(_host(got.array, want.dtype), want), name
        got = rt.read_cog(path, window=WINDOW if want.shape[0] == 70 else (100, 150, 150, 150), device=True, decode='host')
        r0, c0, h, w = WINDOW if want.shape[0] == 70 else (100, 150, 150, 150)
        assert np.array_equal(_host(got.array, want.dtype), want[r0:r0 + h, c0:c0 + w]), name


def test_malformed_blocks_end_with_a_status_and_write_nothing_out_of_range(env, tmp_path):
    """(the same decoder core passed tests/asan/lzw_decode_driver.c on the CPU)  Three of eight blocks are replaced: a slice cut halfway,
    a code above the next free one, a stream that decodes to more than the block"""
    TO, rt = env['TO'], env['rt']
    rng = np.random.default_rng(24)
    n = 4096
    datas = [np.kron(rng.integers(0, 9, n // 8, dtype=np.uint8), np.ones(8, np.uint8)).tobytes() for _ in range(8)]
    streams = [rt.lzw_encode(d) for d in datas]
    streams[1] = streams[1][:len(streams[1]) // 2]
    bad = int.from_bytes(streams[4], 'big') | (0x1ff << (len(streams[4]) * 8 - 27))           # the third code becomes 511: the next free one is 259
    streams[4] = bad.to_bytes(len(streams[4]), 'big')
    streams[6] = rt.lzw_encode(bytes([7]) * (n + 500))                                        # strings of 1, 2, 3 ... bytes: the 91st spans bytes 4095 ... 4185
    slots, status, lengths = _decode(env, streams, n, n + 48)
    assert status.tolist() == [0, 1, 0, 0, 2, 0, 3, 0]
    for i in range(8):
        st, want = rt.lzw_decode(streams[i], n)
        assert st == status[i] and lengths[i] == len(want) and slots[i, :len(want)].tobytes() == want, i
        assert (slots[i, len(want):] == CANARY).all(), i
        if st == 0:
            assert want == datas[i]
    # a slice that points outside the payload is clipped to it: truncated, nothing read
    L = env['L']
    payload = _dev(np.frombuffer(streams[0], np.uint8))
    offs, sizes = _dev(np.array([0, len(streams[0]) - 10, -5, 1 << 40], np.int64)), _dev(np.array([len(streams[0]), 1 << 30, 4, 4], np.int32))
    out = torch.full((4, n), CANARY, dtype=torch.uint8, device='cuda')
    flags = torch.zeros(4, dtype=torch.int32, device='cuda')
    L.check(L.lib.satcv_lzw_decode_tiles(payload.data_ptr(), len(streams[0]), offs.data_ptr(), sizes.data_ptr(), 4, n, out.data_ptr(), n, flags.data_ptr(), None,
                                         env['ops'].stream_ptr()))
    f = flags.cpu().tolist()
    assert f[0] == 0 and 0 <= f[1] <= 3 and f[2] == f[3] == 1 and out[0].cpu().numpy().tobytes() == datas[0]
    assert (out[2:] == CANARY).all()
    # read_cog names the block and the status
    img = np.kron(rng.integers(0, 9, (9, 12), dtype=np.uint8), np.ones((8, 8), np.uint8))[:70, :90]
    path = str(tmp_path / 'bad.tif')
    rt.write_cog(img, path, TRANSFORM, 32618, blocksize=32, overviews=0)
    info = rt.read_info(path)[0]
    b = bytearray(open(path, 'rb').read())
    at = int(info.offsets[5])
    b[at + 2] |= 0x3f
    b[at + 3] |= 0xe0                                         # the third code of tile 5 becomes 511
    open(path, 'wb').write(b)
    for decode in ('device', 'host'):
        with pytest.raises(ValueError, match=r'block 5 .*status 2 \(bad code\)'):
            rt.read_cog(path, decode=decode)
    assert np.array_equal(_host(rt.read_cog(path, window=(0, 0, 32, 90), decode='device').array, np.uint8)[..., 0], img[:32])       # the window avoids it


# ---------------------------------------------------------------------------------------------------------------- 2. untile
def _blocks_of(img, bh, bw, planar, predictor):
    """the decoded blocks of an (h, w, c) image as a file holds them: (n, bh, bw, cb) with edge blocks padded (the padding is made
    nonzero, it must be dropped), planar 2: band after band; predictor 2: differences along each block row, modulo 2^bits"""
    h, w, c = img.shape
    down, across = -(-h // bh), -(-w // bw)
    pad = np.full((down * bh, across * bw, c), 77, img.dtype)
    pad[:h, :w] = img
    planes = [pad] if planar == 1 else [pad[..., b:b + 1] for b in range(c)]
    out = []
    for p in planes:
        cb = p.shape[2]
        out.append(p.reshape(down, bh, across, bw, cb).transpose(0, 2, 1, 3, 4).reshape(down * across, bh, bw, cb))
    blocks = np.ascontiguousarray(np.concatenate(out))
    if predictor:
        u = blocks.view('u%d' % img.dtype.itemsize)
        d = u.copy()
        d[:, :, 1:] = u[:, :, 1:] - u[:, :, :-1]
        blocks = d.view(img.dtype)
    return blocks, across, down


def _untile_ref(blocks, index, bh, bw, across, per_plane, spp, planar, predictor, window, band_map, layout, dst):
    """satcv_raster_untile restated: a cumulative sum per block row and band in the unsigned type, then the scatter"""
    r0, c0, h, w = window
    dt = blocks.dtype
    for blk, t in zip(blocks, index):
        if predictor:
            blk = np.cumsum(blk.view('u%d' % dt.itemsize), axis=1, dtype=np.uint64).astype('u%d' % dt.itemsize).view(dt)
        plane, t2 = (t // per_plane, t % per_plane) if planar == 2 else (0, t)
        by, bx = t2 // across, t2 % across
        for py in range(bh):
            y = by * bh + py - r0
            if not 0 <= y < h:
                continue
            for px in range(bw):
                x = bx * bw + px - c0
                if not 0 <= x < w:
                    continue
                for b in range(blk.shape[2]):
                    band = plane if planar == 2 else b
                    if band_map[band] >= 0:
                        if layout == 0:
                            dst[y, x, band_map[band]] = blk[py, px, b]
                        else:
                            dst[band_map[band], y, x] = blk[py, px, b]
    return dst


def _sample_image(rng, dtype, h, w, c):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return rng.standard_normal((h, w, c)).astype(np.float32)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, (h, w, c), dtype=np.int64).astype(dt)      # full range: the running sums wrap


UNTILE_CASES = [  # (h, w), (bh, bw) -- 0: the image's width, a strip --, bands, dtype, predictor, planar, layout, window
    ((70, 90), (16, 16), 1, np.uint8, True, 1, 0, None), ((70, 90), (32, 32), 3, np.uint8, True, 1, 0, WINDOW),
    ((33, 129), (16, 16), 4, np.uint16, True, 1, 1, None), ((33, 129), (32, 32), 3, np.uint16, True, 2, 0, (9, 30, 20, 70)),
    ((70, 90), (32, 32), 4, np.int16, True, 2, 1, WINDOW), ((70, 90), (16, 16), 3, np.int32, True, 1, 1, WINDOW),
    ((33, 129), (7, 0), 3, np.uint16, True, 1, 0, None), ((70, 90), (7, 0), 4, np.int16, True, 2, 0, WINDOW),
    ((70, 90), (16, 80), 1, np.uint16, True, 1, 0, WINDOW), ((33, 129), (16, 144), 3, np.int32, True, 1, 0, None),
    ((70, 90), (16, 16), 1, np.float32, False, 1, 0, WINDOW), ((33, 129), (32, 32), 4, np.float32, False, 2, 1, None),
    ((70, 90), (32, 32), 3, np.uint8, False, 1, 1, WINDOW), ((33, 129), (16, 16), 4, np.uint16, False, 1, 0, (9, 30, 20, 70)),
    ((70, 90), (7, 0), 1, np.int16, False, 1, 0, None), ((33, 129), (32, 32), 3, np.int32, False, 2, 0, (9, 30, 20, 70)),
    ((70, 90), (16, 16), 4, np.int16, False, 1, 0, None), ((70, 90), (32, 32), 1, np.int32, True, 1, 0, None)]


@pytest.mark.parametrize('hw,block,c,dtype,predictor,planar,layout,window', UNTILE_CASES)
def test_untile_equals_the_numpy_restatement(env, hw, block, c, dtype, predictor, planar, layout, window):
    """edge blocks padded in both directions, blocks wider than 64 pixels (the scan's carry), only the blocks the window touches, a band subset
    written at a channel offset of a wider buffer whose other channels stay as they were"""
    L = env['L']
    rng = np.random.default_rng(31)
    (h, w), dt = hw, np.dtype(dtype)
    bh, bw = block[0], block[1] or w
    img = _sample_image(rng, dt, h, w, c)
    blocks, across, down = _blocks_of(img, bh, bw, planar, predictor)
    window = window or (0, 0, h, w)
    r0, c0, wh, ww = window
    keep = [b for b in range(c) if c < 3 or b != 1]                                # three and four bands: band 1 is dropped
    band_map = [-1] * 16
    for k, b in enumerate(reversed(keep)):                                         # ... and the rest change places
        band_map[b] = k
    plane = [by * across + bx for by in range(r0 // bh, (r0 + wh - 1) // bh + 1) for bx in range(c0 // bw, (c0 + ww - 1) // bw + 1)]
    index = plane if planar == 1 else [b * across * down + t for b in keep for t in plane]
    assert window == (0, 0, h, w) or len(index) < len(blocks)
    ld, coff = len(keep) + 3, 2
    shape = (wh, ww, ld) if layout == 0 else (ld, wh, ww)
    sentinel = _sample_image(rng, dt, *shape)
    want = sentinel.copy()
    view = want[..., coff:] if layout == 0 else want[coff:]
    _untile_ref(blocks[index], index, bh, bw, across, across * down, c, planar, predictor, window, band_map, layout, view)
    src = img[r0:r0 + wh, c0:c0 + ww][..., list(reversed(keep))]
    assert np.array_equal(view[..., :len(keep)] if layout == 0 else view[:len(keep)].transpose(1, 2, 0), src)      # the restatement inverts the tiling
    block_bytes = blocks[0].nbytes
    stride = (block_bytes + 15) // 16 * 16 + 16
    raw = np.full((len(index), stride), 0x33, np.uint8)
    raw[:, :block_bytes] = blocks[index].reshape(len(index), -1).view(np.uint8)
    d_src, d_idx, d_dst = _dev(raw), _dev(np.array(index, np.int32)), _dev(sentinel)
    d = L.UntileDesc(src=d_src.data_ptr(), src_stride=stride, blocks=d_idx.data_ptr(), nblocks=len(index), bh=bh, bw=bw, across=across, per_plane=across * down,
                     spp=c, planar=planar, kind=KIND[dt], predictor=2 if predictor else 0, row0=r0, col0=c0, h=wh, w_=ww, dst=d_dst.data_ptr(), layout=layout,
                     ld=ld, coff=coff, band_map=(C.c_int32 * 16)(*band_map))
    L.check(L.lib.satcv_raster_untile(C.byref(d), env['ops'].stream_ptr()))
    got = _host(d_dst, dt)
    assert np.array_equal(got.view('u%d' % dt.itemsize), want.view('u%d' % dt.itemsize))


# ---------------------------------------------------------------------------------------------------------------- 3. files
ROUND_TRIP = [(comp, pred, kind) for comp in ('lzw', 'deflate', None) for kind in ('u8', 'u16x4', 'f32') for pred in ((False,) if kind == 'f32' else (False, True))]


@pytest.mark.parametrize('compress,predictor,kind', ROUND_TRIP)
def test_write_cog_then_read_cog_returns_the_map_bit_for_bit(env, tmp_path, compress, predictor, kind):
    rt = env['rt']
    rng = np.random.default_rng(41)
    H, W, bs = 150, 201, 32
    if kind == 'u8':
        img = np.kron(rng.integers(0, 4, (19, 26)), np.ones((8, 8))).astype(np.uint8)[:H, :W, None]
    elif kind == 'u16x4':
        img = (rng.integers(0, 60, (H, W, 4)) + np.add.outer(np.arange(H) * 37, np.arange(W) * 11)[..., None] + np.arange(4) * 1000).astype(np.uint16)
    else:
        img = rng.standard_normal((H, W, 1)).astype(np.float32)
    path = str(tmp_path / 'rt.tif')
    nodata = None if kind == 'f32' else 255
    src = _dev(img) if img.dtype != np.uint16 else torch.from_numpy(img).cuda() if hasattr(torch, 'uint16') else img      # (a torch without uint16: the host array goes up)
    rt.write_cog(src, path, TRANSFORM, 'EPSG:32618', compress=compress, predictor=predictor, blocksize=bs, nodata=nodata)
    for decode in ('device', None):
        r = rt.read_cog(path, device=True, decode=decode)
        assert r.array.is_cuda and tuple(r.array.shape) == img.shape and np.array_equal(_host(r.array, img.dtype).view('u%d' % img.dtype.itemsize),
                                                                                      img.view('u%d' % img.dtype.itemsize)), decode
        assert (r.transform, r.crs, r.nodata, r.dtype) == (TRANSFORM, 'EPSG:32618', None if nodata is None else 255.0, img.dtype.name)
    pyramid = rt.device_pyramid(src, nodata=nodata, blocksize=bs)
    one = rt.read_cog(path, level=1, decode='device')
    assert torch.equal(one.array.view(torch.uint8), pyramid[1].contiguous().view(torch.uint8))
    assert one.transform == (10.0 * W / ((W + 1) // 2), 0.0, 399960.0, 0.0, -10.0 * H / ((H + 1) // 2), 4500000.0)
    win = rt.read_cog(path, window=WINDOW, bands=[img.shape[2] - 1], layout='chw', decode='device')
    assert np.array_equal(_host(win.array, img.dtype)[0].view('u%d' % img.dtype.itemsize), img[17:57, 5:66, -1].view('u%d' % img.dtype.itemsize))
    assert win.transform == (10.0, 0.0, 399960.0 + 50.0, 0.0, -10.0, 4500000.0 - 170.0)
    host = rt.read_cog(path, device=False)
    assert np.array_equal(host.array.view('u%d' % img.dtype.itemsize), img.view('u%d' % img.dtype.itemsize))
    with pytest.raises(ValueError):
        rt.read_cog(path, out=torch.empty((H, W, img.shape[2] + 1), dtype=torch.uint8, device='cuda'))


def test_read_stack_feeds_the_composite(env, tmp_path):
    rt, pc = env['rt'], env['pc']
    rng = np.random.default_rng(42)
    paths, images = [], []
    for t in range(3):
        img = rng.integers(1, 6000, (64, 64, 4)).astype(np.uint16)
        p = str(tmp_path / f's{t}.tif')
        rt.write_cog(img, p, TRANSFORM, 32618, predictor=True, blocksize=32, nodata=None, overviews=0)
        paths.append(p)
        images.append(img)
    stack, transform, crs, nodata = rt.read_stack(paths)
    host = np.stack([rt.read_cog(p, device=False, layout='chw').array for p in paths])
    assert np.array_equal(host, np.stack(images).transpose(0, 3, 1, 2))
    assert stack.is_cuda and tuple(stack.shape) == (3, 4, 64, 64) and np.array_equal(_host(stack, np.uint16), host)
    assert (transform, crs, nodata) == (TRANSFORM, 'EPSG:32618', None)
    for a, b in zip(pc.median_composite(stack), pc.median_composite(host)):
        assert torch.equal(a, b)
    part, t2, _, _ = rt.read_stack(paths, window=(8, 16, 40, 33), bands=[3, 1])
    assert np.array_equal(_host(part, np.uint16), host[:, [3, 1], 8:48, 16:49]) and t2 == (10.0, 0.0, 399960.0 + 160.0, 0.0, -10.0, 4500000.0 - 80.0)
    other = str(tmp_path / 'other.tif')
    rt.write_cog(images[0], other, TRANSFORM, 32617, blocksize=32, nodata=None, overviews=0)
    with pytest.raises(ValueError, match='other.tif differs .* in epsg'):
        rt.read_stack(paths + [other])


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


def test_predict_raster_from_file_to_file(env, tmp_path):
    mt, pt, rt, TO = env['mt'], env['pt'], env['rt'], env['TO']
    rng = np.random.default_rng(43)
    m = _unet(mt, 4)
    scene = (rng.integers(0, 3000, (640, 640, 4)) + np.add.outer(np.arange(640), np.arange(640))[..., None]).astype(np.uint16)
    src, out, ref = (str(tmp_path / n) for n in ('in.tif', 'out.tif', 'ref.tif'))
    transform = (10.0, 0.0, 500000.0, 0.0, -10.0, 4100000.0)
    rt.write_cog(scene, src, transform, 'EPSG:32633', predictor=True, blocksize=128, nodata=None)
    kw = dict(kernel=128, buff=64, batch_size=8, channel=1)
    res = pt.predict_raster(src, m, out, cog_options=dict(blocksize=128), **kw)
    want = pt.predict_scene(scene, m, device=True, **kw)
    assert res.is_cuda and torch.equal(res, want) and float(res.abs().max()) > 0
    rt.write_cog(want, ref, transform, 'EPSG:32633', blocksize=128)
    got, exp = open(out, 'rb').read(), open(ref, 'rb').read()
    gi, ei = TO.parse_tiff(got), TO.parse_tiff(exp)
    assert len(gi) == len(ei) == 4
    for a, b in zip(gi, ei):
        assert np.array_equal(TO.read_level(got, a), TO.read_level(exp, b))
    si = TO.parse_tiff(open(src, 'rb').read())[0]
    for tag in (33550, 33922, 34735):                         # the source's georeference reaches the output
        assert gi[0]['tags'][tag] == si['tags'][tag], tag
    assert np.array_equal(TO.read_level(got, gi[0])[..., 0], want.cpu().numpy())
    # a window: its own transform, the prediction of that part of the scene
    res = pt.predict_raster(src, m, out, window=(64, 128, 384, 320), cog_options=dict(blocksize=128), **kw)
    assert torch.equal(res, pt.predict_scene(scene[64:448, 128:448], m, device=True, **kw))
    assert rt.read_info(out)[0].transform == (10.0, 0.0, 500000.0 + 1280.0, 0.0, -10.0, 4100000.0 - 640.0) and rt.read_info(out)[0].epsg == 32633
    with pytest.raises(ValueError):
        pt.predict_raster(src, m, out, device=False)
    with pytest.raises(ValueError, match='georeferenced'):
        pt.predict_raster(os.path.join(GOLD, 'rgb_u8.tif'), m, out)
