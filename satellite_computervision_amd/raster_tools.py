"""The writers of the reference's utils/raster_tools.py (:367-461 `numpy_to_raster`, `arrays_to_cog`) without rasterio and GDAL: a map
that lies on the device is written as a Cloud-Optimized GeoTIFF -- tiled, with overviews, COMPRESS=LZW, nodata = 255 -- from there.

    map (host array or CUDA tensor) -> satcv_raster_convert (dtype, nodata) -> satcv_raster_overview (the pyramid, level by level)
      -> satcv_raster_tiles (tile-major layout, predictor 2) -> satcv_lzw_tiles (every tile of every level in one launch)
      -> satcv_bytes_compact -> one device-to-host copy of the file's tile payload -> header + IFDs + payload on disk

The container is this file's host code: little-endian classic TIFF, every IFD and every out-of-line value before the first tile byte,
tile data from the smallest overview to the full resolution (the order GDAL's COG driver writes, without its ghost header).  The
overview resampling rules are defined here (include/satcv.h, satcv_raster_overview), they are not GDAL's: GDAL's COG default is cubic.
Out of scope: reading GeoTIFFs, BigTIFF, the float predictor 3, `arrays_to_cog`'s window-by-window assembly from .npy files (its body
writes to an undefined `src`), cloud destinations, and the chip and window helpers of utils/raster_tools.py.
"""
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

DTYPES = {'uint8': (np.uint8, 0), 'uint16': (np.uint16, 1), 'float32': (np.float32, 2), 'int16': (np.int16, 3), 'int32': (np.int32, 5)}      # name -> (NumPy type, kind of satcv_raster_desc)
_SAMPLE_FORMAT = {'uint8': 1, 'uint16': 1, 'int16': 2, 'int32': 2, 'float32': 3}
_COMPRESSION = {None: 1, 'lzw': 5, 'deflate': 8}
_RESAMPLING = {'nearest': 0, 'average': 1, 'mode': 2}
_SHORT, _LONG, _ASCII, _DOUBLE = 3, 4, 2, 12


# ----------------------------------------------------------------------------------------------------------------- arguments
def parse_crs(crs):
    """'EPSG:n' or an int n -> (n, geographic).  The GeoKey model type is geographic iff 4000 <= n < 5000, otherwise projected: a
    documented rule, there is no EPSG database here.  Anything else, WKT included, raises ValueError."""
    if isinstance(crs, (int, np.integer)) and not isinstance(crs, bool):
        n = int(crs)
    elif isinstance(crs, str) and crs.strip().upper().startswith('EPSG:') and crs.strip()[5:].strip().isdigit():
        n = int(crs.strip()[5:])
    else:
        raise ValueError(f"crs must be 'EPSG:n' or an int, got {crs!r} (WKT and PROJ strings are not read)")
    if not 1 <= n <= 65535:
        raise ValueError(f'EPSG code {n} does not fit a GeoKey (1 ... 65535)')
    return n, 4000 <= n < 5000


def overview_shapes(h, w, blocksize, overviews='auto'):
    """[(h, w)] of the overview levels, largest first: every level halves the one before (ceil).  'auto' goes on until both sides are
    <= blocksize; an int is an explicit level count (0: none), limited by the 1 x 1 level."""
    shapes = []
    if overviews == 'auto':
        while max(h, w) > blocksize:
            h, w = (h + 1) // 2, (w + 1) // 2
            shapes.append((h, w))
        return shapes
    if isinstance(overviews, bool) or not isinstance(overviews, (int, np.integer)) or overviews < 0:
        raise ValueError(f"overviews must be 'auto' or a level count >= 0, got {overviews!r}")
    for _ in range(int(overviews)):
        if max(h, w) == 1:
            break
        h, w = (h + 1) // 2, (w + 1) // 2
        shapes.append((h, w))
    return shapes


def _check_options(dtype, nodata, compress, predictor, blocksize, resampling, transform):
    if dtype not in DTYPES:
        raise ValueError(f'dtype must be one of {sorted(DTYPES)}, got {dtype!r}')
    if compress not in _COMPRESSION:
        raise ValueError(f"compress must be 'lzw', 'deflate' or None, got {compress!r}")
    if resampling not in _RESAMPLING:
        raise ValueError(f"resampling must be 'nearest', 'average' or 'mode', got {resampling!r}")
    if isinstance(blocksize, bool) or not isinstance(blocksize, (int, np.integer)) or blocksize < 16 or blocksize % 16:
        raise ValueError(f'blocksize must be a positive multiple of 16, got {blocksize!r}')
    if predictor and dtype == 'float32':
        raise ValueError('predictor=True is TIFF predictor 2, for integer dtypes only')
    if resampling == 'mode' and dtype == 'float32':
        raise ValueError("resampling='mode' is for integer dtypes only")
    if nodata is not None and dtype != 'float32':
        info = np.iinfo(DTYPES[dtype][0])
        if float(nodata) != int(nodata) or not info.min <= int(nodata) <= info.max:
            raise ValueError(f'nodata = {nodata} is not a {dtype} value')
    transform = tuple(float(v) for v in transform)
    if len(transform) != 6:
        raise ValueError(f'transform is six numbers (a, b, c, d, e, f), got {len(transform)}')
    return transform


# ----------------------------------------------------------------------------------------------------------------- the container
def _nodata_text(nodata, dtype):
    if dtype != 'float32' or float(nodata) == int(nodata):
        return str(int(nodata))
    return 'nan' if nodata != nodata else repr(float(nodata))


def _geo_tags(transform, epsg, geographic):
    a, b, c, d, e, f = transform
    tags = []
    if b == 0 and d == 0 and a > 0 and e < 0:                 # north-up: scale and tiepoint
        tags.append((33550, _DOUBLE, (a, -e, 0.0)))
        tags.append((33922, _DOUBLE, (0.0, 0.0, 0.0, c, f, 0.0)))
    else:
        tags.append((34264, _DOUBLE, (a, b, 0.0, c, d, e, 0.0, f, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)))
    keys = [(1024, 0, 1, 2 if geographic else 1), (1025, 0, 1, 1), (2048 if geographic else 3072, 0, 1, epsg)]
    tags.append((34735, _SHORT, (1, 1, 0, len(keys)) + tuple(v for k in keys for v in k)))
    return tags


def _pack_value(typ, values):
    if typ == _ASCII:
        return values.encode('ascii') + b'\0'
    return struct.pack('<%d%s' % (len(values), {_SHORT: 'H', _LONG: 'I', _DOUBLE: 'd'}[typ]), *values)


def tile_grid(h, w, blocksize):
    return (h + blocksize - 1) // blocksize, (w + blocksize - 1) // blocksize


def build_container(shapes, dtype, bands, blocksize, compress, predictor, nodata, transform, crs, byte_counts):
    """The bytes of a COG in front of its tile data, and where every tile goes.

    shapes: [(h, w)] of the levels, full resolution first; byte_counts: per level (same order) the byte count of every tile, tiles
    row-major.  -> (head, offsets, total): `head` holds the header, every IFD (full resolution first, then the overviews by decreasing
    size) and the IFDs' out-of-line values; offsets: per level an int64 array of absolute file offsets; total: the file's size.  Tile
    data runs from the SMALLEST overview to the full resolution and every tile starts on an even offset.  ValueError naming BigTIFF when
    an offset would pass 2^32."""
    epsg, geographic = parse_crs(crs)
    itemsize = np.dtype(DTYPES[dtype][0]).itemsize
    counts = [np.asarray(c, np.int64).reshape(-1) for c in byte_counts]
    if len(counts) != len(shapes):
        raise ValueError(f'{len(shapes)} levels need {len(shapes)} byte count lists, got {len(counts)}')
    ifds = []
    for k, ((h, w), cnt) in enumerate(zip(shapes, counts)):
        nty, ntx = tile_grid(h, w, blocksize)
        if cnt.size != nty * ntx:
            raise ValueError(f'level {k} ({h} x {w}) has {nty * ntx} tiles, got {cnt.size} byte counts')
        tags = [(254, _LONG, (1 if k else 0,)), (256, _LONG, (w,)), (257, _LONG, (h,)), (258, _SHORT, (8 * itemsize,) * bands),
                (259, _SHORT, (_COMPRESSION[compress],)), (262, _SHORT, (1,)), (277, _SHORT, (bands,)), (284, _SHORT, (1,))]
        if predictor:
            tags.append((317, _SHORT, (2,)))
        tags += [(322, _LONG, (blocksize,)), (323, _LONG, (blocksize,)), (324, _LONG, None), (325, _LONG, tuple(int(v) for v in cnt))]
        if bands > 1:
            tags.append((338, _SHORT, (0,) * (bands - 1)))
        tags.append((339, _SHORT, (_SAMPLE_FORMAT[dtype],) * bands))
        if k == 0:
            tags += _geo_tags(transform, epsg, geographic)
        if nodata is not None:
            tags.append((42113, _ASCII, _nodata_text(nodata, dtype)))
        ifds.append(sorted(tags, key=lambda t: t[0]))
    # sizes first: IFDs back to back after the 8-byte header, then the out-of-line values (word-aligned), then the tile data
    pos = 8
    ifd_pos = []
    for tags in ifds:
        ifd_pos.append(pos)
        pos += 2 + 12 * len(tags) + 4

    def nbytes(typ, values, ntiles):
        if values is None:
            return 4 * ntiles
        return len(values) + 1 if typ == _ASCII else len(values) * {_SHORT: 2, _LONG: 4, _DOUBLE: 8}[typ]
    value_pos = {}
    for k, tags in enumerate(ifds):
        for tag, typ, values in tags:
            n = nbytes(typ, values, counts[k].size)
            if n > 4:
                value_pos[(k, tag)] = pos
                pos += n + (n & 1)
    data_start = pos
    offsets = [None] * len(shapes)
    for k in reversed(range(len(shapes))):                    # smallest overview first
        off = np.empty(counts[k].size, np.int64)
        for i, n in enumerate(counts[k]):
            off[i] = pos
            pos += int(n) + (int(n) & 1)
        offsets[k] = off
    total = pos
    if total > 0xffffffff:
        raise ValueError(f'the file would be {total} bytes: offsets past 2^32 need BigTIFF, which is not written')
    head = bytearray(data_start)
    head[0:8] = struct.pack('<2sHI', b'II', 42, ifd_pos[0])
    for k, tags in enumerate(ifds):
        p = ifd_pos[k]
        struct.pack_into('<H', head, p, len(tags))
        p += 2
        for tag, typ, values in tags:
            if values is None:
                values = tuple(int(v) for v in offsets[k])
            raw = _pack_value(typ, values)
            count = len(raw) if typ == _ASCII else len(values)
            struct.pack_into('<HHI', head, p, tag, typ, count)
            if len(raw) <= 4:
                head[p + 8:p + 8 + len(raw)] = raw
            else:
                at = value_pos[(k, tag)]
                struct.pack_into('<I', head, p + 8, at)
                head[at:at + len(raw)] = raw
            p += 12
        struct.pack_into('<I', head, p, ifd_pos[k + 1] if k + 1 < len(ifds) else 0)
    return bytes(head), offsets, total


def write_tiles(out_file, shapes, tiles, dtype, bands, blocksize, compress, predictor, nodata, transform, crs):
    """Write a COG from tiles that are already encoded: tiles[k][i] is the byte string of tile i (row-major) of level k, full resolution
    first, in the compression named by `compress`.  The layout is `build_container`'s."""
    head, offsets, total = build_container(shapes, dtype, bands, blocksize, compress, predictor, nodata, transform, crs,
                                           [[len(t) for t in level] for level in tiles])
    with open(out_file, 'wb') as f:
        f.write(head)
        for k in reversed(range(len(shapes))):
            for off, t in zip(offsets[k], tiles[k]):
                f.seek(int(off))
                f.write(t)
        f.truncate(total)
    return out_file


def lzw_encode(data):
    """TIFF LZW of a bytes-like object on the CPU (satcv_lzw_encode_host, the coder the device runs per tile)"""
    import ctypes as C
    from ._lib import check, lib
    data = bytes(data)
    cap = 2 * len(data) + 16
    dst = C.create_string_buffer(cap)
    size = C.c_int64()
    check(lib.satcv_lzw_encode_host(data, len(data), dst, cap, C.byref(size)))
    return dst.raw[:size.value]


def _deflate_all(tiles):
    """zlib level 6 of every tile, in a pool of at most 16 threads (zlib releases the interpreter lock)"""
    import os
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as ex:
        return list(ex.map(lambda t: zlib.compress(t, 6), tiles))


# ----------------------------------------------------------------------------------------------------------------- the device side
def _inspect(arr):
    """What a map is, without touching the device: (obj, kind, H, W, C, ld, coff).  obj is the CUDA tensor to read where it lies, or the
    host array to upload.  ValueError for anything `write_cog` does not take."""
    import torch
    if isinstance(arr, torch.Tensor) and arr.is_cuda:
        t = arr
        kinds = {torch.uint8: 0, torch.float32: 2, torch.float64: 2, torch.int16: 3, torch.int32: 5}
        if hasattr(torch, 'uint16'):
            kinds[torch.uint16] = 1
        if t.dtype not in kinds:
            raise ValueError(f'a map is uint8, uint16, int16, int32, float32 or float64, got {t.dtype}')
        if t.dim() not in (2, 3) or 0 in t.shape:
            raise ValueError(f'expected a non-empty (H, W) or (H, W, C) map, got shape {tuple(t.shape)}')
        H, W = int(t.shape[0]), int(t.shape[1])
        C_ = int(t.shape[2]) if t.dim() == 3 else 1
        if C_ > 16:
            raise ValueError(f'{C_} bands: a map has at most 16')
        ld = int(t.stride(1)) if W > 1 else (int(t.stride(0)) if H > 1 else C_)
        ok = ld >= C_ and (W == 1 or t.stride(1) == ld) and (H == 1 or t.stride(0) == W * ld) and (t.dim() == 2 or C_ == 1 or t.stride(2) == 1)
        if not ok:
            raise ValueError(f'a tensor map is contiguous (H, W[, C]) or a channel slice t[..., a:b] of a contiguous (H, W, ld) tensor; '
                             f'got shape {tuple(t.shape)} with strides {tuple(t.stride())}')
        coff = int(t.storage_offset()) % ld
        if coff + C_ > ld:
            coff = 0                          # (a view that starts inside a row of its base: the descriptor reads from its first sample)
        return t, kinds[t.dtype], H, W, C_, ld, coff
    if isinstance(arr, torch.Tensor):
        arr = arr.numpy()
    a = np.asarray(arr)
    by_np = {np.dtype(v[0]): v[1] for v in DTYPES.values()}
    by_np[np.dtype(np.float64)] = 2
    if a.dtype not in by_np:
        raise ValueError(f'a map is uint8, uint16, int16, int32, float32 or float64, got {a.dtype}')
    if a.ndim not in (2, 3) or 0 in a.shape:
        raise ValueError(f'expected a non-empty (H, W) or (H, W, C) map, got shape {a.shape}')
    H, W = a.shape[:2]
    C_ = a.shape[2] if a.ndim == 3 else 1
    if C_ > 16:
        raise ValueError(f'{C_} bands: a map has at most 16')
    return a, by_np[a.dtype], int(H), int(W), int(C_), int(C_), 0


def _resident(obj, ld, coff):
    """(tensor that owns the samples, address of channel 0 of pixel 0 of the (H, W, ld) raster): a host array goes up once, float64
    becomes float32 first (on the host, as `pc_tools.median_composite` does; a float64 tensor on the device)"""
    import torch
    from .prediction_tools import _to_device
    if isinstance(obj, torch.Tensor):
        if obj.dtype == torch.float64:
            obj = obj.to(torch.float32).contiguous()
            return obj, obj.data_ptr(), obj.shape[2] if obj.dim() == 3 else 1, 0
        return obj, obj.data_ptr() - coff * obj.element_size(), ld, coff
    if obj.dtype == np.float64:
        obj = obj.astype(np.float32)
    t = _to_device(obj, 'the map')
    return t, t.data_ptr(), ld, coff


_stage_hook = None       # tools/cog_probe.py sets a callable: it receives a stage's name once the stage's launches are issued


def _mark(stage):
    if _stage_hook is not None:
        _stage_hook(stage)


_TORCH_OF = {'uint8': 'uint8', 'uint16': 'int16', 'int16': 'int16', 'int32': 'int32', 'float32': 'float32'}      # storage of a kind (bytes only)
_NAME_OF_KIND = {v[1]: k for k, v in DTYPES.items()}


def _desc(src_ptr, src_kind, h, w, c, ld, coff, dst, dst_kind, scale=0.0, nodata=None, resampling=0, blocksize=0, predictor=0):
    from ._lib import RasterDesc
    return RasterDesc(src=src_ptr, src_kind=src_kind, h=h, w_=w, c=c, ld=ld, coff=coff, dst=dst.data_ptr(), dst_kind=dst_kind, scale=float(scale or 0.0),
                      has_nodata=int(nodata is not None), nodata=float(nodata if nodata is not None else 0.0), resampling=resampling,
                      blocksize=blocksize, predictor=int(bool(predictor)))


def _device_pyramid(info, dtype, nodata, scale, shapes, resampling):
    """The converted map and its overviews as device tensors (h, w, C), full resolution first: -> (tensors, their addresses).  A map that
    already is a contiguous raster of `dtype` is read where it lies."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    obj, kind, H, W, C_, ld, coff = info
    owner, ptr, ld, coff = _resident(obj, ld, coff)
    _mark('upload')
    dkind = DTYPES[dtype][1]
    td = getattr(torch, _TORCH_OF[dtype])
    st = ops.stream_ptr()
    if dkind == kind and ld == C_ and coff == 0 and scale is None:
        base, base_ptr = owner, ptr
    else:
        base = _device_empty((H, W, C_), td, 'the converted map')
        base_ptr = base.data_ptr()
        check(lib.satcv_raster_convert(C.byref(_desc(ptr, kind, H, W, C_, ld, coff, base, dkind, scale, nodata)), st))
    _mark('convert')
    levels, ptrs = [base], [base_ptr]
    for (h, w), (oh, ow) in zip(shapes[:-1], shapes[1:]):
        nxt = _device_empty((oh, ow, C_), td, 'an overview')
        check(lib.satcv_raster_overview(C.byref(_desc(ptrs[-1], dkind, h, w, C_, C_, 0, nxt, dkind, 0.0, nodata, _RESAMPLING[resampling])), st))
        levels.append(nxt)
        ptrs.append(nxt.data_ptr())
    _mark('pyramid')
    return levels, ptrs


def device_pyramid(arr, dtype=None, nodata=255, scale=None, blocksize=512, overviews='auto', resampling='nearest'):
    """The first two stages of `write_cog` on their own: the map converted to `dtype` and its overviews, as device tensors [(h, w, C)],
    full resolution first.  Arguments as for `write_cog`."""
    info, dtype, shapes, _ = _plan(arr, dtype, nodata, scale, None, False, blocksize, overviews, resampling, (0,) * 6)
    return _device_pyramid(info, dtype, nodata, scale, shapes, resampling)[0]


def _plan(arr, dtype, nodata, scale, compress, predictor, blocksize, overviews, resampling, transform):
    """every check of `write_cog` that needs no device: -> (info of `_inspect`, dtype name, [(h, w)] of the levels, full resolution first,
    the transform as six floats)"""
    info = _inspect(arr)
    _, kind, H, W, C_, _, _ = info
    dtype = _NAME_OF_KIND[kind] if dtype is None else dtype
    transform = _check_options(dtype, nodata, compress, predictor, blocksize, resampling, transform)
    if scale is not None and kind != 2:
        raise ValueError('scale is for float32 sources only')
    tile_bytes = int(blocksize) ** 2 * C_ * np.dtype(DTYPES[dtype][0]).itemsize
    if tile_bytes >= 1 << 30:
        raise ValueError(f'a tile of {tile_bytes} bytes: tiles stay below 2^30 bytes, lower blocksize')
    return info, dtype, [(H, W)] + overview_shapes(H, W, int(blocksize), overviews), transform


def write_cog(arr, out_file, transform, crs, dtype=None, nodata=255, scale=None, compress='lzw', predictor=False, blocksize=512,
              overviews='auto', resampling='nearest'):
    """Write a map as a Cloud-Optimized GeoTIFF, from the device; returns `out_file`.

    arr: (H, W) or (H, W, C), C <= 16 -- a host array of uint8 / uint16 / int16 / int32 / float32 / float64 (float64 becomes float32 on
    the host, as `pc_tools.median_composite` does; the array is uploaded once), or a CUDA tensor of those kinds, read where it lies: a
    contiguous tensor, or a channel slice t[..., a:b] of a contiguous (H, W, ld) tensor.  Anything else raises ValueError before a launch.
    transform: six numbers in rasterio's Affine order (a, b, c, d, e, f); scale and tiepoint tags are written for a north-up transform
    (b == d == 0, a > 0 > e), a ModelTransformation otherwise.  crs: 'EPSG:n' or an int (`parse_crs`).
    dtype: 'uint8', 'uint16', 'int16', 'int32' or 'float32'; None keeps the array's own.  Conversion rules: satcv_raster_convert --
    float32 to an integer dtype rounds half to even and saturates, NaN becomes nodata; scale (float32 sources only) is one fp32
    multiply before the rounding, e.g. probabilities x 100 into uint8.
    nodata: written as GDAL_NODATA, fills the tile padding, and is skipped by the 'average' and 'mode' overviews; None: no tag, padding 0.
    compress: 'lzw' (on the device), 'deflate' (host zlib level 6 on the uncompressed tiles, in a pool of at most 16 threads) or None.
    predictor=True: TIFF predictor 2, integer dtypes only.  blocksize: the tile side, a multiple of 16.
    overviews: 'auto' halves the image (ceil) until both sides are <= blocksize, or an explicit level count (0: none); resampling:
    'nearest', 'average' or 'mode' ('mode' for integer dtypes only), the rules of satcv_raster_overview, not GDAL's.
    With 'lzw' the host waits once for the per-tile byte counts, and the compressed bytes come back in one copy."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    parse_crs(crs)
    info, dtype, shapes, transform = _plan(arr, dtype, nodata, scale, compress, predictor, blocksize, overviews, resampling, transform)
    blocksize, C_ = int(blocksize), info[4]
    dkind = DTYPES[dtype][1]
    tile_bytes = blocksize * blocksize * C_ * np.dtype(DTYPES[dtype][0]).itemsize
    levels, ptrs = _device_pyramid(info, dtype, nodata, scale, shapes, resampling)
    ntiles = [int(np.prod(tile_grid(h, w, blocksize))) for h, w in shapes]
    n = sum(ntiles)
    st = ops.stream_ptr()
    # every level's tiles in one buffer, in file order: the smallest overview first
    tiles = _device_empty((n, tile_bytes), torch.uint8, 'the tile buffer')
    first = {}
    at = 0
    for k in reversed(range(len(levels))):
        first[k] = at
        h, w = shapes[k]
        d = _desc(ptrs[k], dkind, h, w, C_, C_, 0, tiles, dkind, 0.0, nodata, 0, blocksize, predictor)
        d.dst = tiles.data_ptr() + at * tile_bytes
        check(lib.satcv_raster_tiles(C.byref(d), st))
        at += ntiles[k]
    _mark('tiles')
    if compress == 'lzw':
        slot = 2 * tile_bytes + 16
        slots = _device_empty((n, slot), torch.uint8, 'the compressed tiles')
        sizes = _device_empty((n,), torch.int32, 'the tile sizes')
        check(lib.satcv_lzw_tiles(tiles.data_ptr(), n, tile_bytes, slots.data_ptr(), sizes.data_ptr(), st))
        _mark('lzw')
        counts = sizes.cpu().numpy().astype(np.int64)          # the one host synchronisation
        _mark('sizes')
        per_level = [counts[first[k]:first[k] + ntiles[k]] for k in range(len(levels))]
        head, offsets, total = build_container(shapes, dtype, C_, blocksize, compress, predictor, nodata, transform, crs, per_level)
        rel = np.concatenate([offsets[k] for k in reversed(range(len(levels)))]) - len(head)
        _mark('container')
        payload = _device_empty((total - len(head),), torch.uint8, 'the tile payload', 0)
        off_dev = torch.from_numpy(rel).to('cuda')
        check(lib.satcv_bytes_compact(slots.data_ptr(), slot, sizes.data_ptr(), off_dev.data_ptr(), n, payload.data_ptr(), payload.numel(), st))
        _mark('compact')
        data = payload.cpu().numpy()                           # one copy: exactly the file's tile payload
        _mark('copy')
        with open(out_file, 'wb') as f:
            f.write(head)
            f.write(data.data)
        _mark('file')
        return out_file
    raw = tiles.cpu().numpy()
    _mark('copy')
    blobs = [raw[i].tobytes() for i in range(n)] if compress is None else _deflate_all([raw[i].data for i in range(n)])
    _mark('deflate')
    per_level = [blobs[first[k]:first[k] + ntiles[k]] for k in range(len(levels))]
    write_tiles(out_file, shapes, per_level, dtype, C_, blocksize, compress, predictor, nodata, transform, crs)
    _mark('file')
    return out_file


def numpy_to_raster(arr, mixer, out_file, dtype):
    """utils/raster_tools.py:367-409 without the temporary file: `arr` as a Cloud-Optimized GeoTIFF `out_file` of `dtype` with
    COMPRESS=LZW and nodata = 255.

    arr: (H, W) or (H, W, C), C <= 16, as the reference's docstring says.  (The reference's body reads `C = arr.shape[0]` and opens the
    file with count = 1, so it only runs for one band; here every band is written.)  mixer: 'transform' (its first six numbers, Affine
    order), 'crs', 'cols' and 'rows', which must equal the array's width and height (ValueError otherwise)."""
    shape = tuple(getattr(arr, 'shape', ()))
    if len(shape) not in (2, 3):
        raise ValueError(f'expected an (H, W) or (H, W, C) array, got shape {shape}')
    if int(mixer['cols']) != shape[1] or int(mixer['rows']) != shape[0]:
        raise ValueError(f"mixer announces {mixer['rows']} rows x {mixer['cols']} cols, the array is {shape[0]} x {shape[1]}")
    return write_cog(arr, out_file, tuple(mixer['transform'][0:6]), mixer['crs'], dtype=dtype, nodata=255, compress='lzw')
