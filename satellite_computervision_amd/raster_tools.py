"""The writers of the reference's utils/raster_tools.py (:367-461 `numpy_to_raster`, `arrays_to_cog`) without rasterio and GDAL: a map
that lies on the device is written as a Cloud-Optimized GeoTIFF -- tiled, with overviews, COMPRESS=LZW, nodata = 255 -- from there.
The second half of the file is the way back (`read_info`, `read_cog`, `read_stack`): what the reference asks of rasterio's
`open().read(window=)` and rioxarray's `open_rasterio` (utils/pc_tools.py:131-186, 328-386).  The last part aligns rasters of one CRS that do not share
a pixel grid (`union_grid`, `warp`, `read_warped`, `read_mosaic`, `read_aligned_stack`): stackstac's, BuildVRT's and reproject_match's part; the
end of the file takes points, bounds and rasters between coordinate systems (`transform_points`, `transform_bounds`, `reproject_grid`,
`pixel_coords`, `reproject`, and `reproject=True` of the readers): PROJ's part behind gdal.Warp and stackstac.stack(epsg=).

    map (host array or CUDA tensor) -> satcv_raster_convert (dtype, nodata) -> satcv_raster_overview (the pyramid, level by level)
      -> satcv_raster_tiles (tile-major layout, predictor 2) -> satcv_lzw_tiles (every tile of every level in one launch)
      -> satcv_bytes_compact -> one device-to-host copy of the file's tile payload -> header + IFDs + payload on disk

The container is this file's host code: little-endian classic TIFF, every IFD and every out-of-line value before the first tile byte,
tile data from the smallest overview to the full resolution (the order GDAL's COG driver writes, without its ghost header).  The
overview resampling rules are defined here (include/satcv.h, satcv_raster_overview), they are not GDAL's: GDAL's COG default is cubic.
Out of scope: BigTIFF, the float predictor 3, `arrays_to_cog`'s window-by-window assembly from .npy files (its body
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
def _tensor_kinds():
    """torch dtype -> kind of satcv_raster_desc (float64 is converted to float32 before a kernel reads it)"""
    import torch
    kinds = {torch.uint8: 0, torch.float32: 2, torch.float64: 2, torch.int16: 3, torch.int32: 5}
    if hasattr(torch, 'uint16'):
        kinds[torch.uint16] = 1
    return kinds


def _inspect(arr):
    """What a map is, without touching the device: (obj, kind, H, W, C, ld, coff).  obj is the CUDA tensor to read where it lies, or the
    host array to upload.  ValueError for anything `write_cog` does not take."""
    import torch
    if isinstance(arr, torch.Tensor) and arr.is_cuda:
        t = arr
        kinds = _tensor_kinds()
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


_stage_hook = None       # tools/cog_probe.py and tools/cog_read_probe.py set a callable: it receives a stage's name once the stage's launches are issued


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


# ---------------------------------------------------------------------------------------------------------------------------------
# The reader: GeoTIFF / COG -> resident raster.
#
#     container parsed on the host (read_info) -> the blocks the window touches, read into ONE pinned buffer behind their offsets, sizes
#       and indices -> one host-to-device copy -> satcv_lzw_decode_tiles (one wavefront per block) -> satcv_raster_untile (predictor 2,
#       window, band subset, destination layout) -> a device tensor in the file's own kind
#
# Deflate blocks are inflated on the host (zlib, at most 16 threads) and go up raw; uncompressed blocks go up as they are; decode='host'
# does the same for LZW with satcv_lzw_decode_host.  Read: little-endian classic TIFF, tiles or strips, planar configuration 1 or 2,
# 8 / 16 / 32-bit samples of one kind, predictor 1 or 2.  Refused by name: big-endian files, BigTIFF, JPEG and every other compression,
# the floating-point predictor, other sample widths, bands of differing kinds, more than 16 bands, blocks that point past the file.
_TIFF_TYPES = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 5: 'II', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 10: 'ii', 11: 'f', 12: 'd', 16: 'Q'}
_COMPRESSION_NAMES = {1: None, 5: 'lzw', 8: 'deflate', 32946: 'deflate'}
_FOREIGN_COMPRESSION = {2: 'CCITT RLE', 3: 'CCITT fax 3', 4: 'CCITT fax 4', 6: 'old-style JPEG', 7: 'JPEG', 32773: 'PackBits', 34712: 'JPEG 2000',
                        34887: 'LERC', 34925: 'LZMA', 50000: 'ZSTD', 50001: 'WebP', 50002: 'JPEG XL'}
_KIND_OF_FORMAT = {(8, 1): 'uint8', (16, 1): 'uint16', (16, 2): 'int16', (32, 2): 'int32', (32, 3): 'float32'}
STATUS_NAMES = {0: 'ok', 1: 'truncated input', 2: 'bad code', 3: 'overlong'}       # satcv_lzw_decode_tiles


class LevelInfo:
    """One IFD of a file, as `read_info` returns it: shape (h, w), bands, dtype (name), block_shape (bh, bw), tiled, compression (None,
    'lzw' or 'deflate'), predictor (bool: TIFF predictor 2), planar (1 or 2), nodata (float or None), transform (six numbers in Affine
    order, or None), epsg (int or None), crs ('EPSG:n' or None), overview (NewSubfileType bit 0), offsets / counts (int64 arrays of the
    block list) and index (the IFD's place in the file)."""
    __slots__ = ('index', 'shape', 'bands', 'dtype', 'block_shape', 'tiled', 'compression', 'predictor', 'planar', 'nodata', 'transform', 'epsg',
                 'overview', 'offsets', 'counts')

    @property
    def crs(self):
        return None if self.epsg is None else f'EPSG:{self.epsg}'

    def __repr__(self):
        return 'LevelInfo(' + ', '.join(f'{k}={getattr(self, k)!r}' for k in self.__slots__[:-2]) + ')'


class Raster:
    """What `read_cog` returns: array (a CUDA tensor, or a NumPy array with device=False), transform (Affine order, of the window and
    level that were read), crs ('EPSG:n' or None), nodata, dtype (name of the file's kind)."""
    __slots__ = ('array', 'transform', 'crs', 'nodata', 'dtype')

    def __init__(self, array, transform, crs, nodata, dtype):
        self.array, self.transform, self.crs, self.nodata, self.dtype = array, transform, crs, nodata, dtype


def _read_at(f, at, n, size, what):
    if at < 0 or at + n > size:
        raise ValueError(f'{what} at offset {at} ({n} bytes) points past the end of the file ({size} bytes)')
    f.seek(at)
    return f.read(n)


def _parse_ifd(f, pos, size, index):
    n = struct.unpack('<H', _read_at(f, pos, 2, size, f'IFD {index}'))[0]
    raw = _read_at(f, pos + 2, 12 * n + 4, size, f'IFD {index}')
    tags = {}
    for i in range(n):
        tag, typ, count, val = struct.unpack_from('<HHI4s', raw, 12 * i)
        if typ not in _TIFF_TYPES:
            continue
        nbytes = struct.calcsize('<' + _TIFF_TYPES[typ]) * count
        if nbytes > 4:
            val = _read_at(f, struct.unpack('<I', val)[0], nbytes, size, f'the value of tag {tag} of IFD {index}')
        val = val[:nbytes]
        if typ == 2:
            tags[tag] = val
        elif typ in (4, 16) and count > 64:
            tags[tag] = np.frombuffer(val, '<u4' if typ == 4 else '<u8').astype(np.int64)
        else:
            v = struct.unpack('<%d%s' % (count * len(_TIFF_TYPES[typ]), _TIFF_TYPES[typ][0]), val)
            tags[tag] = tuple(a / b if b else float('nan') for a, b in zip(v[::2], v[1::2])) if typ in (5, 10) else v
    return tags, struct.unpack_from('<I', raw, 12 * n)[0]


def _geo(tags):
    """(transform or None, epsg or None) of an IFD's GeoTIFF tags"""
    keys = {}
    gk = tags.get(34735)
    if gk is not None and len(gk) >= 4:
        for i in range(int(gk[3])):
            k = gk[4 + 4 * i:8 + 4 * i]
            if len(k) == 4 and k[1] == 0:
                keys[int(k[0])] = int(k[3])
    epsg = keys.get(3072, keys.get(2048))
    if epsg is not None and not 1 <= epsg < 32767:
        epsg = None                                           # 32767: user-defined, there is no EPSG database here
    transform = None
    if 34264 in tags and len(tags[34264]) == 16:
        m = tags[34264]
        transform = (m[0], m[1], m[3], m[4], m[5], m[7])
    elif 33550 in tags and 33922 in tags and len(tags[33922]) >= 6:
        (sx, sy), (i, j, _, x, y) = tags[33550][:2], tags[33922][:5]
        transform = (sx, 0.0, x - i * sx, 0.0, -sy, y + j * sy)
    if transform is not None and keys.get(1025) == 2:         # RasterPixelIsPoint: the tiepoint is a pixel centre
        a, b, c, d, e, f_ = transform
        transform = (a, b, c - 0.5 * (a + b), d, e, f_ - 0.5 * (d + e))
    return (tuple(float(v) for v in transform) if transform is not None else None), epsg


def _level_info(tags, index, size):
    def one(tag, default=None):
        v = tags.get(tag)
        return default if v is None or len(v) == 0 else int(v[0])
    who = f'IFD {index}'
    info = LevelInfo()
    info.index = index
    w, h = one(256), one(257)
    if not w or not h:
        raise ValueError(f'{who} has no ImageWidth / ImageLength')
    info.shape = (h, w)
    info.bands = spp = one(277, 1)
    if spp > 16:
        raise ValueError(f'{who} has {spp} bands: more than 16 bands are not read')
    comp = one(259, 1)
    if comp not in _COMPRESSION_NAMES:
        name = _FOREIGN_COMPRESSION.get(comp, 'unknown')
        raise ValueError(f'{who} is compressed with {name} (Compression = {comp}): only none (1), LZW (5) and deflate (8, 32946) are read'
                         + ('; JPEG blocks are out of scope' if 'JPEG' in name else ''))
    info.compression = _COMPRESSION_NAMES[comp]
    bits = tuple(int(v) for v in tags.get(258, (1,)))
    fmts = tuple(int(v) for v in tags.get(339, (1,) * len(bits)))
    if len(set(bits)) > 1 or len(set(fmts)) > 1:
        raise ValueError(f'{who} has bands of differing kinds (BitsPerSample {bits}, SampleFormat {fmts}): one kind per file is read')
    if bits[0] not in (8, 16, 32):
        raise ValueError(f'{who} has {bits[0]} bits per sample: 8, 16 and 32 are read')
    if (bits[0], fmts[0]) not in _KIND_OF_FORMAT:
        raise ValueError(f'{who} has {bits[0]}-bit samples of SampleFormat {fmts[0]}: uint8, uint16, int16, int32 and float32 are read')
    info.dtype = _KIND_OF_FORMAT[(bits[0], fmts[0])]
    pred = one(317, 1)
    if pred == 3:
        raise ValueError(f'{who} uses predictor 3 (floating-point), which is not read; predictor 1 and 2 are')
    if pred not in (1, 2) or (pred == 2 and info.dtype == 'float32'):
        raise ValueError(f'{who} uses predictor {pred} on {info.dtype} samples: 1 (none) and 2 (integer kinds) are read')
    info.predictor = pred == 2
    info.planar = one(284, 1)
    if info.planar not in (1, 2):
        raise ValueError(f'{who} has PlanarConfiguration {info.planar}')
    info.tiled = 322 in tags
    if info.tiled:
        bw, bh = one(322), one(323)
        offs, cnts = tags.get(324), tags.get(325)
    else:
        bw, bh = w, min(one(278, h) or h, h)
        offs, cnts = tags.get(273), tags.get(279)
    if not bw or not bh or offs is None or cnts is None:
        raise ValueError(f'{who} has no complete block list (tile or strip shape, offsets and byte counts)')
    info.block_shape = (bh, bw)
    nblocks = -(-h // bh) * -(-w // bw) * (spp if info.planar == 2 else 1)
    info.offsets, info.counts = np.asarray(offs, np.int64).reshape(-1), np.asarray(cnts, np.int64).reshape(-1)
    if info.offsets.size != nblocks or info.counts.size != nblocks:
        raise ValueError(f'{who} needs {nblocks} blocks, its lists have {info.offsets.size} offsets and {info.counts.size} byte counts')
    bad = np.nonzero((info.offsets + info.counts > size) | (info.counts < 0))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f'{who}: block {i} at offset {int(info.offsets[i])} with {int(info.counts[i])} bytes points past the end of the file ({size} bytes)')
    if bh * bw * (spp if info.planar == 1 else 1) * (bits[0] // 8) >= 1 << 30:
        raise ValueError(f'{who} has blocks of {bh} x {bw}: blocks stay below 2^30 bytes')
    nd = tags.get(42113)
    info.nodata = None
    if nd is not None:
        try:
            info.nodata = float(bytes(nd).split(b'\0')[0].decode('ascii').strip())
        except ValueError:
            pass
    info.transform, info.epsg = _geo(tags)
    info.overview = bool(one(254, 0) & 1)
    return info


def read_info(path):
    """[LevelInfo] of every IFD of a GeoTIFF, in file order (a COG: the full resolution, then its overviews).  Only the container is
    read.  ValueError, naming what the file has, for: a big-endian (MM) file, BigTIFF, a compression other than none / LZW / deflate,
    predictor 3, bits per sample other than 8 / 16 / 32, bands of differing kinds, more than 16 bands, and block offsets or byte counts
    that point past the end of the file."""
    import os
    size = os.path.getsize(path)
    with open(path, 'rb') as f:
        head = f.read(8)
        if len(head) < 8 or head[:2] not in (b'II', b'MM'):
            raise ValueError(f'{path} is not a TIFF file')
        if head[:2] == b'MM':
            raise ValueError(f'{path} is a big-endian (MM) TIFF: only little-endian (II) files are read')
        version = struct.unpack('<H', head[2:4])[0]
        if version == 43:
            raise ValueError(f'{path} is a BigTIFF (version 43): only classic TIFF (version 42) is read')
        if version != 42:
            raise ValueError(f'{path} has TIFF version {version}, expected 42')
        pos = struct.unpack('<I', head[4:8])[0]
        infos, seen = [], set()
        while pos:
            if pos in seen:
                raise ValueError(f'{path}: the IFD chain loops at offset {pos}')
            seen.add(pos)
            tags, pos = _parse_ifd(f, pos, size, len(infos))
            infos.append(_level_info(tags, len(infos), size))
    if not infos:
        raise ValueError(f'{path} has no image')
    return infos


def _levels(infos):
    """the image and its overview chain: IFD 0, then every IFD marked as an overview"""
    return [infos[0]] + [i for i in infos[1:] if i.overview]


def _window_transform(base, full_hw, level_hw, row0, col0):
    if base is None:
        return None
    a, b, c, d, e, f = base
    sx, sy = full_hw[1] / level_hw[1], full_hw[0] / level_hw[0]
    a, b, d, e = a * sx, b * sy, d * sx, e * sy
    return (a, b, c + col0 * a + row0 * b, d, e, f + col0 * d + row0 * e)


def _plan_read(info, window, bands):
    """-> (row0, col0, h, w), band list, file indices of the blocks the window touches (row-major; planar 2: band after band)"""
    H, W = info.shape
    if window is None:
        window = (0, 0, H, W)
    if len(window) != 4 or any(isinstance(v, bool) or int(v) != v for v in window):
        raise ValueError(f'window is four integers (row0, col0, h, w), got {window!r}')
    row0, col0, h, w = (int(v) for v in window)
    if row0 < 0 or col0 < 0 or h < 1 or w < 1 or row0 + h > H or col0 + w > W:
        raise ValueError(f'window {(row0, col0, h, w)} lies outside the image of {H} x {W}')
    if bands is None:
        bands = list(range(info.bands))
    bands = [int(b) for b in bands]
    if not bands or len(set(bands)) != len(bands) or min(bands) < 0 or max(bands) >= info.bands:
        raise ValueError(f'bands must be distinct indices below {info.bands}, got {bands}')
    bh, bw = info.block_shape
    across, down = -(-W // bw), -(-H // bh)
    plane = [by * across + bx for by in range(row0 // bh, (row0 + h - 1) // bh + 1) for bx in range(col0 // bw, (col0 + w - 1) // bw + 1)]
    blocks = plane if info.planar == 1 else [b * across * down + t for b in sorted(bands) for t in plane]
    return (row0, col0, h, w), bands, blocks


def _stream_hint(stream):
    first = (int.from_bytes(bytes(stream[:2]), 'big') >> 7) if len(stream) >= 2 else 256
    return '' if first == 256 else ("; the stream does not open with a Clear code (its first 9 bits, MSB-first, are %d): this may be the LSB-first "
                                    "'old-style' LZW, which is not supported" % first)


def lzw_decode(stream, cap):
    """TIFF LZW of a bytes-like object decoded on the CPU (satcv_lzw_decode_host): -> (status, bytes), at most `cap` bytes"""
    import ctypes as C
    from ._lib import check, lib
    stream = bytes(stream)
    dst = C.create_string_buffer(max(int(cap), 1))
    size, status = C.c_int64(), C.c_int32()
    check(lib.satcv_lzw_decode_host(stream, len(stream), dst, int(cap), C.byref(size), C.byref(status)))
    return status.value, dst.raw[:size.value]


def _expected_bytes(info, blocks):
    """per block the bytes it must decode to: a full block, but only the rows inside the image for the last strip"""
    H, W = info.shape
    bh, bw = info.block_shape
    eb = np.dtype(DTYPES[info.dtype][0]).itemsize
    cb = info.bands if info.planar == 1 else 1
    if info.tiled:
        return [bh * bw * cb * eb] * len(blocks)
    down = -(-H // bh)
    return [min(bh, H - (t % down) * bh) * bw * cb * eb for t in blocks]


def _refuse_block(t, status, stream):
    raise ValueError(f'block {t} does not decode: status {status} ({STATUS_NAMES.get(status, "?")})' + _stream_hint(stream))


def _decode_host(info, blocks, slices, into, stride):
    """the blocks decoded on the host into `into` (a uint8 array), block j at j * stride; at most 16 threads"""
    import ctypes as C
    import os
    from ._lib import check, lib
    want = _expected_bytes(info, blocks)
    block_bytes = info.block_shape[0] * info.block_shape[1] * (info.bands if info.planar == 1 else 1) * np.dtype(DTYPES[info.dtype][0]).itemsize

    def one(j):
        raw, dst = slices[j], into[j * stride:j * stride + stride]
        if info.compression is None:
            got = bytes(raw)
        elif info.compression == 'deflate':
            try:
                got = zlib.decompress(raw)
            except zlib.error as e:
                raise ValueError(f'block {blocks[j]} does not inflate: {e}') from e
        else:
            size, status = C.c_int64(), C.c_int32()
            check(lib.satcv_lzw_decode_host(bytes(raw), len(raw), dst.ctypes.data, block_bytes, C.byref(size), C.byref(status)))
            if status.value or size.value < want[j]:
                _refuse_block(blocks[j], status.value if status.value else 1, raw)
            return
        if len(got) < want[j]:
            raise ValueError(f'block {blocks[j]} holds {len(got)} bytes, {want[j]} are needed')
        dst[:min(len(got), stride)] = np.frombuffer(got, np.uint8)[:stride]
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1))) as ex:
        list(ex.map(one, range(len(blocks))))


def _untile_host(info, blocks, raw, stride, window, bands, layout):
    """NumPy counterpart of satcv_raster_untile for device=False"""
    H, W = info.shape
    bh, bw = info.block_shape
    dt = np.dtype(DTYPES[info.dtype][0])
    across, down = -(-W // bw), -(-H // bh)
    cb = info.bands if info.planar == 1 else 1
    row0, col0, h, w = window
    out = np.zeros((h, w, len(bands)), dt)
    for j, t in enumerate(blocks):
        plane, t2 = (t // (across * down), t % (across * down)) if info.planar == 2 else (0, t)
        by, bx = t2 // across, t2 % across
        blk = raw[j * stride:j * stride + bh * bw * cb * dt.itemsize].view(dt).reshape(bh, bw, cb)
        if info.predictor:
            blk = np.cumsum(blk.view('u%d' % dt.itemsize), axis=1, dtype=np.uint64).astype('u%d' % dt.itemsize).view(dt)
        y0, x0 = max(by * bh, row0), max(bx * bw, col0)
        y1, x1 = min(by * bh + bh, row0 + h), min(bx * bw + bw, col0 + w)
        part = blk[y0 - by * bh:y1 - by * bh, x0 - bx * bw:x1 - bx * bw]
        for k, b in enumerate(bands):
            if info.planar == 1:
                out[y0 - row0:y1 - row0, x0 - col0:x1 - col0, k] = part[..., b]
            elif b == plane:
                out[y0 - row0:y1 - row0, x0 - col0:x1 - col0, k] = part[..., 0]
    return out if layout == 'hwc' else np.ascontiguousarray(out.transpose(2, 0, 1))


def _torch_dtype(name):
    import torch
    if name == 'uint16':
        return torch.uint16 if hasattr(torch, 'uint16') else torch.int16      # (bytes only, where this torch has no uint16)
    return getattr(torch, name)


def default_decode(info):
    """where `read_cog(decode=None)` decodes LZW blocks: the choice tools/cog_read_probe.py measured per input class ("Reading
    GeoTIFFs")"""
    return 'host'


def read_cog(path, window=None, level=0, bands=None, layout='hwc', device=True, decode=None, out=None):
    """Read a GeoTIFF / COG onto the device: -> `Raster` (array, transform, crs, nodata, dtype).

    window: (row0, col0, h, w) in pixels of the level that is read, None: all of it; only the blocks it touches are read from the file.
    level: 0 the image, k its k-th overview (the IFDs marked as overviews, in file order).  bands: indices of the bands to keep, in the
    order given; None: all.  layout: 'hwc' -> (h, w, C), 'chw' -> (C, h, w).  The array is in the file's own kind (uint8, uint16,
    int16, int32, float32): a CUDA tensor, or a NumPy array with device=False.  The transform is that of the window at that level.
    decode: where LZW blocks are decoded -- 'device' (satcv_lzw_decode_tiles: the compressed bytes go up, one wavefront decodes a block),
    'host' (satcv_lzw_decode_host in at most 16 threads, the raw blocks go up), None: `default_decode`.  Deflate blocks are always
    inflated on the host (zlib), uncompressed blocks go up as they are.  Either way the blocks travel in one pinned buffer and one
    copy, and one satcv_raster_untile launch undoes predictor 2 and scatters them into the window.
    out: a contiguous CUDA tensor of the result's shape and kind to write into (a slot of a stack), returned as `.array`.
    ValueError: what `read_info` refuses, a window outside the image, and a block that does not decode (its index and status)."""
    import ctypes as C
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    if decode not in (None, 'host', 'device'):
        raise ValueError(f"decode must be 'host', 'device' or None, got {decode!r}")
    infos = read_info(path)
    levels = _levels(infos)
    if isinstance(level, bool) or int(level) != level or not 0 <= level < len(levels):
        raise ValueError(f'level {level!r}: the file has levels 0 ... {len(levels) - 1}')
    info = levels[int(level)]
    window, bands, blocks = _plan_read(info, window, bands)
    row0, col0, h, w = window
    if info.compression != 'lzw':
        decode = 'host'
    elif decode is None:
        decode = default_decode(info) if device else 'host'
    if decode == 'device' and not device:
        raise ValueError("decode='device' leaves the raster on the device: it needs device=True")
    if out is not None and not device:
        raise ValueError('out is a CUDA tensor: it needs device=True')
    dt = np.dtype(DTYPES[info.dtype][0])
    bh, bw = info.block_shape
    cb = info.bands if info.planar == 1 else 1
    block_bytes = bh * bw * cb * dt.itemsize
    stride = (block_bytes + 15) // 16 * 16
    n = len(blocks)
    transform = _window_transform(levels[0].transform, levels[0].shape, info.shape, row0, col0)
    result = lambda arr: Raster(arr, transform, levels[0].crs, info.nodata if info.nodata is not None else levels[0].nodata, info.dtype)
    offs, cnts = info.offsets[blocks], info.counts[blocks]
    if not device:
        with open(path, 'rb') as f:
            slices = []
            for o, c in zip(offs, cnts):
                f.seek(int(o))
                slices.append(f.read(int(c)))
        raw = np.zeros(n * stride, np.uint8)
        _decode_host(info, blocks, slices, raw, stride)
        return result(_untile_host(info, blocks, raw, stride, window, bands, layout))
    import torch
    from . import ops
    from ._lib import UntileDesc, check, lib
    from .prediction_tools import _device_empty
    shape = (h, w, len(bands)) if layout == 'hwc' else (len(bands), h, w)
    td = _torch_dtype(info.dtype)
    if out is None:
        out = _device_empty(shape, td, 'the raster')
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == shape and out.element_size() == dt.itemsize
              and out.dtype.is_floating_point == (dt.kind == 'f')):
        raise ValueError(f'out must be a contiguous CUDA tensor of shape {shape} and kind {info.dtype}')
    # one pinned buffer: offsets (int64), sizes (int32) and block indices (int32) of the n blocks, then the payload
    head = 16 * n
    payload = int(cnts.sum()) if decode == 'device' else n * stride
    pinned = torch.empty(head + max(payload, 16), dtype=torch.uint8, pin_memory=True)
    buf = pinned.numpy()
    rel = np.concatenate([[0], np.cumsum(cnts)[:-1]]).astype(np.int64) if decode == 'device' else np.arange(n, dtype=np.int64) * stride
    buf[:8 * n].view(np.int64)[:] = rel
    buf[8 * n:12 * n].view(np.int32)[:] = cnts if decode == 'device' else block_bytes
    buf[12 * n:16 * n].view(np.int32)[:] = blocks
    with open(path, 'rb') as f:
        if decode == 'device':
            for o, c, r in zip(offs, cnts, rel):
                f.seek(int(o))
                f.readinto(memoryview(buf[head + int(r):head + int(r) + int(c)]))
        else:
            slices = []
            for o, c in zip(offs, cnts):
                f.seek(int(o))
                slices.append(f.read(int(c)))
    if decode != 'device':
        buf[head:head + payload] = 0
        _decode_host(info, blocks, slices, buf[head:head + payload], stride)
    _mark('read')
    dev = pinned.to('cuda', non_blocking=True)                 # the one host-to-device copy
    _mark('upload')
    st = ops.stream_ptr()
    base = dev.data_ptr()
    if decode == 'device':
        decoded = _device_empty((n * stride,), torch.uint8, 'the decoded blocks')
        flags = _device_empty((2 * n,), torch.int32, 'the block statuses')
        check(lib.satcv_lzw_decode_tiles(base + head, payload, base, base + 8 * n, n, block_bytes, decoded.data_ptr(), stride, flags.data_ptr(),
                                         flags.data_ptr() + 4 * n, st))
        src = decoded.data_ptr()
    else:
        src = base + head
    _mark('decode')
    d = UntileDesc(src=src, src_stride=stride, blocks=base + 12 * n, nblocks=n, bh=bh, bw=bw, across=-(-info.shape[1] // bw),
                   per_plane=-(-info.shape[1] // bw) * -(-info.shape[0] // bh), spp=info.bands, planar=info.planar, kind=DTYPES[info.dtype][1],
                   predictor=2 if info.predictor else 0, row0=row0, col0=col0, h=h, w_=w, dst=out.data_ptr(), layout=0 if layout == 'hwc' else 1,
                   ld=len(bands), coff=0)
    for b in range(16):
        d.band_map[b] = bands.index(b) if b in bands else -1
    check(lib.satcv_raster_untile(C.byref(d), st))
    _mark('untile')
    if decode == 'device':
        got = flags.cpu().numpy()                              # the one host synchronisation: statuses and decoded lengths
        want = np.asarray(_expected_bytes(info, blocks))
        bad = np.nonzero((got[:n] != 0) | (got[n:] < want))[0]
        if bad.size:
            j = int(bad[0])
            r, c = int(rel[j]), int(cnts[j])
            _refuse_block(blocks[j], int(got[j]) if got[j] else 1, buf[head + r:head + r + c])
    else:
        torch.cuda.current_stream().synchronize()              # the pinned buffer is released only after the copy
    _mark('status')
    return result(out)


def read_stack(paths, window=None, bands=None):
    """The files of a time series as one resident stack: -> (stack, transform, crs, nodata), stack a (T, C, H, W) CUDA tensor in the
    files' kind -- what `pc_tools.median_composite`, `ee_tools.mask` and `pc_tools.predict_change` take.  Every file is decoded straight
    into its slot (`read_cog(..., layout='chw', out=stack[t])`).  The files must agree on shape, kind, transform and CRS: ValueError
    names the first that differs."""
    from .prediction_tools import _device_empty
    paths = list(paths)
    if not paths:
        raise ValueError('read_stack needs at least one file')
    first = read_info(paths[0])[0]
    for p in paths[1:]:
        i = read_info(p)[0]
        for what in ('shape', 'bands', 'dtype', 'transform', 'epsg'):
            if getattr(i, what) != getattr(first, what):
                raise ValueError(f'{p} differs from {paths[0]} in {what}: {getattr(i, what)!r} against {getattr(first, what)!r}')
    (row0, col0, h, w), bands, _ = _plan_read(first, window, bands)
    stack = _device_empty((len(paths), len(bands), h, w), _torch_dtype(first.dtype), 'the time stack')
    for t, p in enumerate(paths):
        r = read_cog(p, (row0, col0, h, w), 0, bands, 'chw', True, None, stack[t])
    return stack, r.transform, r.crs, r.nodata


# ---------------------------------------------------------------------------------------------------------------------------------
# Alignment: rasters of one CRS brought onto one pixel grid, on the device.
#
#     grids on the host (Grid, union_grid, warp_window) -> the window of the file the grid needs (read_cog) -> satcv_raster_warp
#       (nearest / bilinear / cubic / average, nodata-aware, into a new raster, a slot of a stack or a channel range of a scene)
#
# What the reference takes from stackstac.stack(epsg=, resolution=), gdal.BuildVRT / rioxarray's merge_arrays and reproject_match
# (utils/pc_tools.py:152-186, 251-282, 368-431).  The resampling rules are this library's own (include/satcv.h, "Raster alignment").
# Refused by name: rotated or sheared transforms, two different EPSG codes (unless reproject=True: the last section), a raster without a transform.
WARP_RESAMPLING = {'nearest': 0, 'bilinear': 1, 'cubic': 2, 'average': 3}
_WARP_MARGIN = {'nearest': 0, 'bilinear': 1, 'cubic': 2}
MAX_AVERAGE_SCALE = 64


def _check_transform(transform, what):
    if transform is None:
        raise ValueError(f'{what} has no transform: it cannot be placed on a grid')
    t = tuple(float(v) for v in transform)
    if len(t) != 6:
        raise ValueError(f'transform is six numbers (a, b, c, d, e, f), got {len(t)} for {what}')
    if t[1] != 0 or t[3] != 0:
        raise ValueError(f'{what} has a rotated or sheared transform (b = {t[1]}, d = {t[3]}): only scale and shift are resampled')
    if not (np.isfinite(t).all() and t[0] != 0 and t[4] != 0):
        raise ValueError(f'{what} has a transform with a zero or non-finite pixel size: {t}')
    return t


def _epsg_of(crs):
    return None if crs is None else parse_crs(crs)[0]


def _common_epsg(codes, what='the sources'):
    """the one EPSG code of `codes` (None entries say nothing): ValueError for two different ones"""
    known = sorted({c for c in codes if c is not None})
    if len(known) > 1:
        raise ValueError(f'{what} are in EPSG:{known[0]} and EPSG:{known[1]}: reprojection between coordinate systems is not done')
    return known[0] if known else None


class Grid(tuple):
    """A pixel grid: transform (six numbers in Affine order, b == d == 0), shape (H, W), crs ('EPSG:n' or None).  An immutable value;
    `bounds` is (left, bottom, right, top), `resolution` (|a|, |e|)."""
    __slots__ = ()

    def __new__(cls, transform, shape, crs=None):
        t = _check_transform(transform, 'a grid')
        if len(tuple(shape)) != 2 or any(isinstance(v, bool) or int(v) != v or int(v) < 1 for v in shape):
            raise ValueError(f'a grid has a shape (H, W) of positive integers, got {shape!r}')
        epsg = _epsg_of(crs)
        return tuple.__new__(cls, (t, (int(shape[0]), int(shape[1])), None if epsg is None else f'EPSG:{epsg}'))

    transform = property(lambda self: self[0])
    shape = property(lambda self: self[1])
    crs = property(lambda self: self[2])

    @property
    def epsg(self):
        return _epsg_of(self[2])

    @property
    def resolution(self):
        return abs(self[0][0]), abs(self[0][4])

    @property
    def bounds(self):
        a, _, c, _, e, f = self[0]
        H, W = self[1]
        xs, ys = (c, c + W * a), (f, f + H * e)
        return min(xs), min(ys), max(xs), max(ys)

    def __repr__(self):
        return f'Grid(transform={self[0]!r}, shape={self[1]!r}, crs={self[2]!r})'


def _as_grid(source):
    """a path, a LevelInfo or a Grid as a Grid"""
    if isinstance(source, Grid):
        return source
    if isinstance(source, LevelInfo):
        _check_transform(source.transform, f'IFD {source.index}')
        return Grid(source.transform, source.shape, source.crs)
    info = read_info(source)[0]
    _check_transform(info.transform, str(source))
    return Grid(info.transform, info.shape, info.crs)


def union_grid(sources, resolution=None, bounds=None, crs=None, reproject=False):
    """The north-up grid that holds every source: -> Grid.  sources: paths, `LevelInfo`s or `Grid`s.  resolution: a number or (x, y);
    None: the finest among the sources, per axis.  bounds: (left, bottom, right, top); None: the union of the sources' bounds.  The
    bounds are snapped outward to multiples of the resolution (stackstac's snap_bounds), so grids made from overlapping sets of files
    share their pixel edges.  ValueError for rotated sources, sources without a transform, and two different EPSG codes.
    reproject=True takes sources of several EPSG codes (`crs.crs_params` names the supported ones): the grid is in `crs`, without one in
    the code of the first source that has one; a source of another code enters with `transform_bounds` of its bounds and with its pixel
    size measured in the target CRS at its centre (`measured_pixel_size`)."""
    grids = [_as_grid(s) for s in sources]
    if reproject:
        known = [g.epsg for g in grids if g.epsg is not None]
        epsg = _epsg_of(crs) if crs is not None else (known[0] if known else None)
        grids = [g if g.epsg in (None, epsg) else _foreign_extent(g, epsg) for g in grids]
    else:
        epsg = _common_epsg([g.epsg for g in grids] + [_epsg_of(crs)])
    if resolution is None:
        if not grids:
            raise ValueError('union_grid needs sources or a resolution')
        rx, ry = min(g.resolution[0] for g in grids), min(g.resolution[1] for g in grids)
    else:
        rx, ry = (float(resolution),) * 2 if np.ndim(resolution) == 0 else (float(v) for v in resolution)
    if not (np.isfinite([rx, ry]).all() and rx > 0 and ry > 0):
        raise ValueError(f'resolution must be positive, got {resolution!r}')
    if bounds is None:
        if not grids:
            raise ValueError('union_grid needs sources or bounds')
        b = [g.bounds for g in grids]
        bounds = min(v[0] for v in b), min(v[1] for v in b), max(v[2] for v in b), max(v[3] for v in b)
    left, bottom, right, top = (float(v) for v in bounds)
    if not (np.isfinite([left, bottom, right, top]).all() and left < right and bottom < top):
        raise ValueError(f'bounds are (left, bottom, right, top) with left < right and bottom < top, got {bounds!r}')
    left, right = np.floor(left / rx) * rx, np.ceil(right / rx) * rx
    bottom, top = np.floor(bottom / ry) * ry, np.ceil(top / ry) * ry
    return Grid((rx, 0.0, float(left), 0.0, -ry, float(top)), (int(round((top - bottom) / ry)), int(round((right - left) / rx))),
                None if epsg is None else f'EPSG:{epsg}')


def warp_coefficients(src_transform, dst_transform):
    """(su, ou, sv, ov) of satcv_raster_warp: destination pixel coordinates (j + 0.5, i + 0.5) -> source pixel coordinates
    u = su * (j + 0.5) + ou, v = sv * (i + 0.5) + ov"""
    a_s, _, c_s, _, e_s, f_s = _check_transform(src_transform, 'the source')
    a_d, _, c_d, _, e_d, f_d = _check_transform(dst_transform, 'the destination grid')
    return a_d / a_s, (c_d - c_s) / a_s, e_d / e_s, (f_d - f_s) / e_s


def _check_method(resampling, su, sv):
    if resampling not in WARP_RESAMPLING:
        raise ValueError(f'resampling must be one of {sorted(WARP_RESAMPLING)}, got {resampling!r}')
    if resampling == 'average' and max(abs(su), abs(sv)) > MAX_AVERAGE_SCALE:
        raise ValueError(f"resampling='average' over a footprint of {abs(sv):.4g} x {abs(su):.4g} source pixels (at most {MAX_AVERAGE_SCALE} per axis): "
                         "read an overview of the source instead (level='auto')")


def warp_window(src_transform, src_shape, grid, resampling='nearest'):
    """The window (row0, col0, h, w) of a source raster that `grid` needs under `resampling`, or None when the grid misses the raster:
    the pixels under the grid's sample points and 0 (nearest), 1 (bilinear) or 2 (cubic) more on every side, for 'average' the pixels
    the grid's footprint touches; clipped to the raster."""
    su, ou, sv, ov = warp_coefficients(src_transform, grid.transform)
    _check_method(resampling, su, sv)
    out = []
    for s, o, n_dst, n_src in ((sv, ov, grid.shape[0], src_shape[0]), (su, ou, grid.shape[1], src_shape[1])):
        if resampling == 'average':
            ends = (s * 0.0 + o, s * float(n_dst) + o)
            lo, hi = int(np.floor(min(ends))), int(np.ceil(max(ends))) - 1
        else:
            ends = (s * 0.5 + o, s * (n_dst - 0.5) + o)
            m = _WARP_MARGIN[resampling]
            lo, hi = int(np.floor(min(ends))) - m, int(np.floor(max(ends))) + m
        lo, hi = max(lo, 0), min(hi, int(n_src) - 1)
        if lo > hi:
            return None
        out.append((lo, hi - lo + 1))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def auto_level(level_transforms, grid, src_crs=None):
    """level='auto' of `read_warped`: the index of the coarsest level whose pixels are no larger than the grid's on either axis (level 0
    when none is); level_transforms: the transform of every level, the image first.  src_crs: the files' CRS when it is not the grid's --
    a level's pixel size is then measured in the grid's CRS at the grid's centre (`measured_pixel_size`)."""
    rx, ry = grid.resolution
    best, size = 0, -1.0
    foreign = src_crs is not None and grid.epsg is not None and _epsg_of(src_crs) != grid.epsg
    if foreign:
        a, _, c, _, e, f = grid.transform
        centre = (c + 0.5 * grid.shape[1] * a, f + 0.5 * grid.shape[0] * e)
    for k, t in enumerate(level_transforms):
        px, py = measured_pixel_size(t, src_crs, grid.crs, centre) if foreign else (abs(t[0]), abs(t[4]))
        if px <= rx * (1 + 1e-9) and py <= ry * (1 + 1e-9) and px * py > size:
            best, size = k, px * py
    return best


def _fill(t, dtype, value):
    """every sample of the CUDA tensor `t` (a view too) becomes `value` of kind `dtype` (uint16 may be stored as int16)"""
    import torch
    if dtype == 'float32':
        t.fill_(float(value))
    else:
        nt = np.dtype(DTYPES[dtype][0])
        store = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[nt.itemsize]
        t.view(store).fill_(int(np.array(value, nt).view({1: np.uint8, 2: np.int16, 4: np.int32}[nt.itemsize])))
    return t


def _invalid_value(dtype, nodata):
    return nodata if nodata is not None else (float('nan') if dtype == 'float32' else 0)


def _chw_or_hwc(layout):
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    return 0 if layout == 'hwc' else 1


def _warp_source(src, src_layout, src_dtype):
    """a resident source as (pointer of band 0 of pixel 0 of the ld-wide raster, kind name, h, w, c, ld, coff, two-dimensional)"""
    import torch
    if not (isinstance(src, torch.Tensor) and src.is_cuda):
        raise ValueError('warp takes a resident raster: a CUDA tensor')
    if src.dtype == torch.float64:
        raise ValueError('a resident raster is uint8, uint16, int16, int32 or float32, got torch.float64')
    if _chw_or_hwc(src_layout) == 0:
        t, kind, h, w, c, ld, coff = _inspect(src)
        ptr = t.data_ptr() - coff * t.element_size()
    else:
        if src.dim() not in (2, 3) or 0 in src.shape or not src.is_contiguous():
            raise ValueError(f"a 'chw' source is a contiguous, non-empty (C, H, W) or (H, W) CUDA tensor, got shape {tuple(src.shape)}")
        if src.dtype not in _tensor_kinds():
            raise ValueError(f'a resident raster is uint8, uint16, int16, int32 or float32, got {src.dtype}')
        kind = _tensor_kinds()[src.dtype]
        c, h, w = ((1,) + tuple(src.shape))[-3:]
        ld, coff, ptr = c, 0, src.data_ptr()
        if c > 16:
            raise ValueError(f'{c} bands: a raster has at most 16')
    name = _NAME_OF_KIND[kind]
    if src_dtype is not None:
        if src_dtype not in DTYPES or np.dtype(DTYPES[src_dtype][0]).itemsize != src.element_size() or (src_dtype == 'float32') != (name == 'float32'):
            raise ValueError(f'src_dtype {src_dtype!r} does not describe a tensor of {src.dtype}')
        name = src_dtype
    return ptr, name, int(h), int(w), int(c), int(ld), int(coff), src.dim() == 2


def warp(src, src_transform, grid, resampling='nearest', src_nodata=None, nodata=None, dtype=None, src_layout='hwc', layout='hwc', out=None,
         channel_offset=0, keep=False, src_origin=(0, 0), src_dtype=None):
    """A resident raster resampled onto `grid` (same CRS), on the device: -> CUDA tensor of grid.shape.

    src: a CUDA tensor -- (H, W) or (H, W, C) for src_layout 'hwc' (contiguous, or a channel slice of a contiguous (H, W, ld) tensor),
    (H, W) or a contiguous (C, H, W) for 'chw'; C <= 16; uint8, uint16, int16, int32 or float32 (src_dtype='uint16' names the kind of
    an int16 tensor that stores uint16 bytes).  src_transform: the Affine transform of the grid `src` is a window of; src_origin:
    (row, col) of src[0, 0] on that grid -- a window warped with its origin equals the whole raster warped, bit for bit.
    grid: the destination `Grid`.  resampling: 'nearest', 'bilinear', 'cubic' (Catmull-Rom) or 'average' (area-weighted; at most 64
    source pixels per destination pixel and axis) -- the rules of satcv_raster_warp in include/satcv.h, which are this library's own.
    src_nodata: samples equal to it are invalid, as NaN is.  nodata: what an invalid result becomes; None: src_nodata, and without
    that NaN (float32) or 0.  dtype: None keeps the source's kind, 'float32' converts.  keep=True leaves the destination untouched where
    the result is invalid (the mosaic rule: later sources lie on top only where they have data).
    out: the tensor to write into, contiguous: (H, W, ld) for layout 'hwc', (ld, H, W) for 'chw' (a slot stack[t] of a (T, C, H, W)
    stack), or (H, W) -- bands go to channels channel_offset .. channel_offset + C - 1, no other channel is touched; returned as given.
    Without `out` the result is a new (H, W, C) / (C, H, W) tensor ((H, W) for a two-dimensional source).
    ValueError: rotated transforms, an unknown method, 'average' beyond 64 pixels, shapes or kinds that do not fit; MemoryError names a
    destination that does not fit in device memory."""
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    su, ou, sv, ov = warp_coefficients(src_transform, grid.transform)
    _check_method(resampling, su, sv)
    return _resample(src, (su, ou, sv, ov), None, grid, resampling, src_nodata, nodata, dtype, src_layout, layout, out, channel_offset, keep, src_origin, src_dtype)


def _resample(src, coeff, rmap, grid, resampling, src_nodata, nodata, dtype, src_layout, layout, out, channel_offset, keep, src_origin, src_dtype):
    """the launch `warp` and `reproject` share: the descriptor of satcv_raster_warp, with the coefficients `coeff` (rmap None) or with a
    `ReprojectMap` for satcv_raster_reproject"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import WarpDesc, check, lib
    from .prediction_tools import _device_empty
    su, ou, sv, ov = coeff
    ptr, name, sh, sw, c, sld, scoff, flat = _warp_source(src, src_layout, src_dtype)
    dname = name if dtype is None else dtype
    if dname not in (name, 'float32'):
        raise ValueError(f'dtype must be None, {name!r} (the source) or \'float32\', got {dtype!r}')
    dl = _chw_or_hwc(layout)
    H, W = grid.shape
    if out is None:
        shape = (H, W) if flat else ((H, W, c) if dl == 0 else (c, H, W))
        out = _device_empty(shape, _torch_dtype(dname), 'the warped raster')
        dld, dcoff = c, 0
    else:
        nt = np.dtype(DTYPES[dname][0])
        want = '(H, W, ld)' if dl == 0 else '(ld, H, W)'
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dim() in (2, 3)):
            raise ValueError(f'out must be a contiguous CUDA tensor of shape {want} or (H, W)')
        hw = tuple(out.shape) if out.dim() == 2 else (tuple(out.shape[:2]) if dl == 0 else tuple(out.shape[1:]))
        dld = 1 if out.dim() == 2 else int(out.shape[2] if dl == 0 else out.shape[0])
        if hw != (H, W):
            raise ValueError(f'out is {hw[0]} x {hw[1]}, the grid {H} x {W}')
        if dtype is None and out.dtype == torch.float32:
            dname, nt = 'float32', np.dtype(np.float32)
        if out.element_size() != nt.itemsize or out.dtype.is_floating_point != (nt.kind == 'f') or out.dtype == torch.float64:
            raise ValueError(f'out is {out.dtype}, the result {dname}')
        dcoff = int(channel_offset)
        if dcoff < 0 or dcoff + c > dld:
            raise ValueError(f'channels {dcoff} ... {dcoff + c - 1} do not fit the {dld} of out')
    if nodata is None:
        nodata = src_nodata
    d = WarpDesc(src=ptr, src_kind=DTYPES[name][1], src_layout=_chw_or_hwc(src_layout), sh=sh, sw=sw, src_ld=sld, src_coff=scoff,
                 src_row0=int(src_origin[0]), src_col0=int(src_origin[1]), dst=out.data_ptr(), dst_kind=DTYPES[dname][1], dst_layout=dl, dh=H, dw=W,
                 dst_ld=dld, dst_coff=dcoff, dst_row0=0, dst_col0=0, c=c, su=su, ou=ou, sv=sv, ov=ov, resampling=WARP_RESAMPLING[resampling],
                 has_src_nodata=int(src_nodata is not None), src_nodata=float(src_nodata if src_nodata is not None else 0.0),
                 has_dst_nodata=int(nodata is not None), dst_nodata=float(nodata if nodata is not None else 0.0), keep=int(bool(keep)))
    if rmap is None:
        check(lib.satcv_raster_warp(C.byref(d), ops.stream_ptr()))
        _mark('warp')
    else:
        check(lib.satcv_raster_reproject(C.byref(d), C.byref(rmap), ops.stream_ptr()))
        _mark('reproject')
    return out


def _file_levels(path, grid, reproject=False):
    """the levels of a file that can be placed on `grid`: -> (levels, their transforms); ValueError for a file without a transform, a
    rotated one, or one in another CRS (with reproject: in a CRS `crs.crs_params` does not know)"""
    levels = _levels(read_info(path))
    base = levels[0]
    _check_transform(base.transform, str(path))
    if reproject and None not in (base.epsg, grid.epsg) and base.epsg != grid.epsg:
        from .crs import crs_params
        for code in (base.epsg, grid.epsg):                    # (a ValueError that names the supported set)
            crs_params(code)
    else:
        _common_epsg([base.epsg, grid.epsg], f'{path} and the grid')
    return levels, [_window_transform(base.transform, base.shape, lv.shape, 0, 0) for lv in levels]


def read_warped(path, grid, bands=None, resampling='nearest', level=0, layout='hwc', out=None, keep=False, nodata=None, dtype=None,
                channel_offset=0, decode=None, reproject=False):
    """A GeoTIFF / COG read onto `grid`: -> `Raster` on the grid (array, the grid's transform and CRS, nodata, dtype).

    Only the window of the file that the grid needs is read (`warp_window`: the samples under the grid and 0 / 1 / 2 more for nearest /
    bilinear / cubic, the footprint for average), then `warp` resamples it with the window's origin, so the result equals the whole
    file warped.  A grid that misses the file reads nothing: the result is all nodata (untouched with keep).
    bands, decode: as for `read_cog`.  level: 0 the image (the default: results do not depend on how the overviews were made), k its
    k-th overview, 'auto' the coarsest level whose pixels are no larger than the grid's on either axis (`auto_level`).
    resampling, layout, out, channel_offset, keep, dtype: as for `warp`.  nodata: what invalid results become; None: the file's nodata,
    without one NaN (float32) or 0.  ValueError: a file without a transform, a rotated one, one in another EPSG code than the grid's
    ("reprojection between coordinate systems is not done"), and what `read_cog` and `warp` refuse.
    reproject=True reads a file of another EPSG code instead of refusing it: the window is `reproject_window`'s (the source pixels
    under the grid's boundary, the method's margin and one pixel more), the resampling `reproject`'s -- the same rules with the pixel's
    coordinates taken through both projections; 'average' is a ValueError there, and level='auto' measures the file's pixels in the
    grid's CRS at the grid's centre."""
    from .prediction_tools import _device_empty
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    levels, transforms = _file_levels(path, grid, reproject)
    foreign = reproject and None not in (levels[0].epsg, grid.epsg) and levels[0].epsg != grid.epsg
    if foreign:
        _check_reproject_method(resampling)
    if level == 'auto':
        level = auto_level(transforms, grid, levels[0].crs if foreign else None)
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level < len(levels):
        raise ValueError(f"level {level!r}: the file has levels 0 ... {len(levels) - 1} (or 'auto')")
    info, lt = levels[int(level)], transforms[int(level)]
    src_nodata = info.nodata if info.nodata is not None else levels[0].nodata
    if nodata is None:
        nodata = src_nodata
    dname = info.dtype if dtype is None else dtype
    crs = grid.crs if grid.crs is not None else levels[0].crs
    window = reproject_window(lt, info.shape, levels[0].crs, grid, resampling) if foreign else warp_window(lt, info.shape, grid, resampling)
    if window is None:
        _, nb, _ = _plan_read(info, None, bands)
        c = len(nb)
        if out is None:
            H, W = grid.shape
            out = _device_empty((H, W, c) if _chw_or_hwc(layout) == 0 else (c, H, W), _torch_dtype(dname), 'the warped raster')
            _fill(out, dname, _invalid_value(dname, nodata))
        elif not keep:
            if out.dtype.is_floating_point:
                dname = 'float32'
            part = out if out.dim() == 2 else (out[..., channel_offset:channel_offset + c] if layout == 'hwc' else out[channel_offset:channel_offset + c])
            _fill(part, dname, _invalid_value(dname, nodata))
        return Raster(out, grid.transform, crs, nodata, dname)
    r = read_cog(path, window, int(level), bands, 'hwc', True, decode)
    if foreign:
        arr = _reproject_raster(r.array, lt, levels[0].crs, grid, resampling, src_nodata, nodata, dtype, 'hwc', layout, out, channel_offset, keep, window[:2], info.dtype)
    else:
        arr = warp(r.array, lt, grid, resampling, src_nodata, nodata, dtype, 'hwc', layout, out, channel_offset, keep, window[:2], info.dtype)
    return Raster(arr, grid.transform, crs, nodata, 'float32' if arr.dtype.is_floating_point else info.dtype)


def _same_kind(paths, bands):
    """(dtype, number of bands read, nodata) the files share; ValueError names the first that differs in kind or band count"""
    first = read_info(paths[0])[0]
    n = len(_plan_read(first, None, bands)[1])
    for p in paths[1:]:
        i = read_info(p)[0]
        if i.dtype != first.dtype or (bands is None and i.bands != first.bands):
            raise ValueError(f'{p} differs from {paths[0]} in kind or bands: {i.dtype} x {i.bands} against {first.dtype} x {first.bands}')
    return first.dtype, n, first.nodata


def read_mosaic(paths, grid=None, bands=None, resampling='nearest', level=0, layout='hwc', first=False, nodata=None, dtype=None, out=None,
                channel_offset=0, decode=None, reproject=False):
    """Files of one CRS mosaicked onto one grid: -> `Raster`.  grid: None is `union_grid(paths)`.  The destination is filled with
    nodata, then every file is read onto it with keep=True, in order: a later file lies on top wherever it has valid data
    (gdal.BuildVRT's order); first=True goes through the files in reverse, so the first file wins (rioxarray's merge_arrays).
    nodata: None is the first file's, without one NaN (float32) or 0.  The other arguments as for `read_warped`; with reproject=True the
    files may be in several EPSG codes (the two-UTM-zone case), grid=None is then `union_grid(paths, reproject=True)`."""
    from .prediction_tools import _device_empty
    paths = list(paths)
    if not paths:
        raise ValueError('read_mosaic needs at least one file')
    if grid is None:
        grid = union_grid(paths, reproject=reproject)
    for p in paths:
        _file_levels(p, grid, reproject)                       # every refusal before anything is allocated
    name, c, file_nodata = _same_kind(paths, bands)
    if nodata is None:
        nodata = file_nodata
    dname = name if dtype is None else dtype
    H, W = grid.shape
    if out is None:
        out = _device_empty((H, W, c) if _chw_or_hwc(layout) == 0 else (c, H, W), _torch_dtype(dname), 'the mosaic')
        part = out
    else:
        part = out if out.dim() == 2 else (out[..., channel_offset:channel_offset + c] if layout == 'hwc' else out[channel_offset:channel_offset + c])
        if out.dtype.is_floating_point:
            dname = 'float32'
    _fill(part, dname, _invalid_value(dname, nodata))
    for p in (reversed(paths) if first else paths):
        r = read_warped(p, grid, bands, resampling, level, layout, out, True, nodata, dtype, channel_offset, decode, reproject)
    return Raster(out, grid.transform, r.crs, nodata, dname)


def read_aligned_stack(items, grid=None, resolution=None, bands=None, resampling='nearest', level=0, reproject=False):
    """The acquisitions of a time series on ONE grid as a resident stack: -> (stack, transform, crs, nodata), the contract of
    `read_stack` -- stack a (T, C, H, W) CUDA tensor in the files' kind -- for files that need not share a grid: other footprints,
    other resolutions (the 20 m bands beside the 10 m ones), one CRS.  items: per acquisition a path, or a list of paths mosaicked
    into the slot (`read_mosaic`).  grid: None is `union_grid` of every file at `resolution` (None: the finest).  Every file is
    resampled straight into its slot.  With files that already share the grid, nearest gives `read_stack`'s result bit for bit.
    reproject=True: the files may be in several EPSG codes (`read_warped`); the grid built here is `union_grid(..., reproject=True)`."""
    import os
    from .prediction_tools import _device_empty
    items = [[it] if isinstance(it, (str, os.PathLike)) else list(it) for it in items]
    flat = [p for it in items for p in it]
    if not flat or any(not it for it in items):
        raise ValueError('read_aligned_stack needs at least one file per acquisition')
    if grid is None:
        grid = union_grid(flat, resolution=resolution, reproject=reproject)
    elif resolution is not None:
        raise ValueError('resolution describes the grid that is built when none is given')
    for p in flat:
        _file_levels(p, grid, reproject)
    name, c, nodata = _same_kind(flat, bands)
    H, W = grid.shape
    stack = _device_empty((len(items), c, H, W), _torch_dtype(name), 'the time stack')
    for t, it in enumerate(items):
        if len(it) == 1:
            r = read_warped(it[0], grid, bands, resampling, level, 'chw', stack[t], False, nodata, reproject=reproject)
        else:
            r = read_mosaic(it, grid, bands, resampling, level, 'chw', False, nodata, None, stack[t], reproject=reproject)
    return stack, grid.transform, r.crs, nodata


# ---------------------------------------------------------------------------------------------------------------------------------
# Reprojection: rasters of several coordinate systems brought onto one grid, on the device.
#
#     EPSG table on the host (crs.py) -> points through satcv_crs_transform (bounds, windows, pixel sizes: the CPU loop of the same
#       csrc/crs_core.hpp the kernels use) -> satcv_raster_reproject (the warp's rules, u and v through both projections per pixel)
#
# What the reference takes from gdal.Warp (utils/pc_tools.py:152-186: NAIP tiles in two UTM zones), stackstac.stack(epsg=) and
# rasterio's transform_bounds (utils/prediction_tools.py:560-600).  The projection rules are csrc/crs_core.hpp's; WGS84 and NAD83
# coordinates are taken as the same point (no datum shift, at most 1-2 m).  Every default of the functions above is unchanged:
# reprojection is opt-in (reproject=True) or goes through the names below.
def _check_reproject_method(resampling):
    if resampling not in WARP_RESAMPLING:
        raise ValueError(f'resampling must be one of {sorted(WARP_RESAMPLING)}, got {resampling!r}')
    if resampling == 'average':
        raise ValueError("resampling='average' between two coordinate systems is not done (a pixel's footprint is no axis-parallel rectangle): "
                         "read an overview with level='auto' and resample it with 'bilinear'")


def transform_points(xs, ys, src_crs, dst_crs, device=False):
    """Points of `src_crs` in `dst_crs`: -> (xs, ys) of the same shape, float64.  Geographic coordinates are x = longitude, y = latitude
    in degrees.  A point outside a projection's domain (csrc/crs_core.hpp: |lat| > 90, more than 30 degrees off a UTM zone's central
    meridian, beyond the square world of EPSG:3857, not finite) comes back as NaN.  device=False: array-likes in, NumPy arrays out, the
    loop runs on the CPU; device=True: CUDA float64 tensors in and out, one thread per point.  No datum shift between WGS84 and NAD83
    (at most 1-2 m).  ValueError for a code `crs.crs_params` does not know."""
    import ctypes as C
    from ._lib import check, lib
    from .crs import crs_struct
    a, b = crs_struct(src_crs), crs_struct(dst_crs)
    if device:
        import torch
        from . import ops
        if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 for t in (xs, ys)) or xs.shape != ys.shape:
            raise ValueError('device=True takes two CUDA float64 tensors of one shape')
        xs, ys = xs.contiguous(), ys.contiguous()
        xo, yo = torch.empty_like(xs), torch.empty_like(ys)
        check(lib.satcv_crs_transform(C.byref(a), C.byref(b), xs.data_ptr(), ys.data_ptr(), xo.data_ptr(), yo.data_ptr(), None, xs.numel(), 1, ops.stream_ptr()))
        return xo, yo
    xs, ys = np.ascontiguousarray(xs, np.float64), np.ascontiguousarray(ys, np.float64)
    if xs.shape != ys.shape:
        raise ValueError(f'xs and ys differ in shape: {xs.shape} against {ys.shape}')
    xo, yo = np.empty_like(xs), np.empty_like(ys)
    check(lib.satcv_crs_transform(C.byref(a), C.byref(b), xs.ctypes.data, ys.ctypes.data, xo.ctypes.data, yo.ctypes.data, None, xs.size, 0, None))
    return xo, yo


def transform_bounds(src_crs, dst_crs, left, bottom, right, top, densify_pts=21):
    """rasterio's `transform_bounds`: the box (left, bottom, right, top) of `dst_crs` that holds the box of `src_crs`.  Every edge gets
    `densify_pts` points between its corners (an edge that is straight in one projection bulges in another), all are transformed, and
    the result is the minimum and maximum over the points inside the projections' domains.  ValueError when none is."""
    if isinstance(densify_pts, bool) or int(densify_pts) != densify_pts or densify_pts < 0:
        raise ValueError(f'densify_pts must be an integer >= 0, got {densify_pts!r}')
    t = np.linspace(0.0, 1.0, int(densify_pts) + 2)
    ex, ey = left + (right - left) * t, bottom + (top - bottom) * t
    xs = np.concatenate([ex, ex, np.full_like(t, left), np.full_like(t, right)])
    ys = np.concatenate([np.full_like(t, bottom), np.full_like(t, top), ey, ey])
    xo, yo = transform_points(xs, ys, src_crs, dst_crs)
    ok = ~np.isnan(xo)
    if not ok.any():
        raise ValueError(f'no point of the bounds {(left, bottom, right, top)} of {src_crs} lies inside the domain of {dst_crs}')
    return float(xo[ok].min()), float(yo[ok].min()), float(xo[ok].max()), float(yo[ok].max())


def measured_pixel_size(src_transform, src_crs, dst_crs, centre):
    """(px, py): the size of a pixel of `src_transform` (of `src_crs`) in units of `dst_crs`, at the point `centre` = (x, y) of
    `dst_crs`: the point is taken to `src_crs`, it and its two one-pixel neighbours (one column on, one row on) are taken back, and the
    two distances are the sizes.  ValueError when one of the three lies outside a projection's domain."""
    a, _, _, _, e, _ = _check_transform(src_transform, 'the source')
    cx, cy = transform_points([centre[0]], [centre[1]], dst_crs, src_crs)
    xs, ys = transform_points([cx[0], cx[0] + a, cx[0]], [cy[0], cy[0], cy[0] + e], src_crs, dst_crs)
    if np.isnan(xs).any():
        raise ValueError(f'the point {tuple(centre)} of {dst_crs} and its neighbours do not lie inside the domain of {src_crs}')
    return float(np.hypot(xs[1] - xs[0], ys[1] - ys[0])), float(np.hypot(xs[2] - xs[0], ys[2] - ys[0]))


class _Extent:
    """bounds and resolution of a source in another CRS (what `union_grid` needs of a Grid)"""
    __slots__ = ('bounds', 'resolution', 'epsg')

    def __init__(self, bounds, resolution, epsg):
        self.bounds, self.resolution, self.epsg = bounds, resolution, epsg


def _foreign_extent(g, epsg):
    dst = f'EPSG:{epsg}'
    bounds = transform_bounds(g.crs, dst, *g.bounds)
    a, _, c, _, e, f = g.transform
    cx, cy = transform_points([c + 0.5 * g.shape[1] * a], [f + 0.5 * g.shape[0] * e], g.crs, dst)
    if np.isnan(cx[0]):
        raise ValueError(f'the centre of a source in {g.crs} lies outside the domain of {dst}')
    return _Extent(bounds, measured_pixel_size(g.transform, g.crs, dst, (cx[0], cy[0])), epsg)


def reproject_grid(source, dst_crs, resolution=None, bounds=None):
    """A north-up grid of `dst_crs` that holds `source` (a path, a `LevelInfo` or a `Grid` with a CRS): -> Grid.  bounds: None is
    `transform_bounds` of the source's bounds.  resolution: a number or (x, y); None keeps the number of pixels along the diagonal --
    the length of the destination bounds' diagonal over sqrt(H^2 + W^2), square pixels.  The bounds are snapped outward to multiples of
    the resolution, as `union_grid` does.  This rule is the library's own (it is the one GDAL documents for its suggested warp output,
    but GDAL's `calculate_default_transform` was not run against it)."""
    g = _as_grid(source)
    if g.crs is None:
        raise ValueError('the source carries no EPSG code: it cannot be reprojected')
    if bounds is None:
        bounds = transform_bounds(g.crs, dst_crs, *g.bounds)
    if resolution is None:
        left, bottom, right, top = (float(v) for v in bounds)
        resolution = float(np.hypot(right - left, top - bottom) / np.hypot(g.shape[0], g.shape[1]))
    return union_grid([], resolution=resolution, bounds=bounds, crs=dst_crs)


def _reproject_map(grid, src_crs, src_transform):
    from ._lib import ReprojectMap
    from .crs import crs_struct
    if grid.crs is None or src_crs is None:
        raise ValueError('reprojection needs the EPSG codes of the grid and of the source')
    a_d, _, c_d, _, e_d, f_d = grid.transform
    m = ReprojectMap(dst_crs=crs_struct(grid.crs), dst_a=a_d, dst_c=c_d, dst_e=e_d, dst_f=f_d, src_crs=crs_struct(src_crs), has_src_transform=0)
    if src_transform is not None:
        a_s, _, c_s, _, e_s, f_s = _check_transform(src_transform, 'the source')
        m.has_src_transform, m.src_a, m.src_c, m.src_e, m.src_f = 1, a_s, c_s, e_s, f_s
    return m


def pixel_coords(grid, crs=None, transform=None):
    """Per pixel of `grid` the coordinates of its centre in another system: -> a (2, H, W) float64 CUDA tensor (satcv_grid_coords).
    crs: the other CRS (None: the grid's own); with crs=4326 the result is the longitude [0] and latitude [1] of every pixel.
    transform: an Affine transform in that CRS -- the result is then in its pixel coordinates, column u [0] and row v [1], the very
    numbers `reproject` samples at; None: CRS units.  NaN where a pixel lies outside a projection's domain."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    m = _reproject_map(grid, grid.crs if crs is None else crs, transform)
    H, W = grid.shape
    out = _device_empty((2, H, W), torch.float64, 'the coordinate field')
    check(lib.satcv_grid_coords(C.byref(m), H, W, 0, 0, out[0].data_ptr(), out[1].data_ptr(), ops.stream_ptr()))
    return out


def reproject(src, src_transform, src_crs, grid, resampling='nearest', src_nodata=None, nodata=None, dtype=None, src_layout='hwc', layout='hwc',
              out=None, channel_offset=0, keep=False, src_origin=(0, 0), src_dtype=None):
    """A resident raster of `src_crs` resampled onto `grid` of another CRS, on the device: -> CUDA tensor of grid.shape.  Every argument
    but src_crs is `warp`'s, and so are the rules: per destination pixel the centre's coordinates go through the grid's projection
    back to longitude / latitude and through the source's projection forward (csrc/crs_core.hpp; no datum shift between WGS84 and
    NAD83, at most 1-2 m), then 'nearest', 'bilinear' or 'cubic' sample as `warp` does; a pixel outside a projection's domain is
    invalid.  With equal EPSG codes (or a missing one) this IS `warp`.  'average' across two codes is a ValueError: read an overview
    (level='auto') and use 'bilinear'."""
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    if src_crs is None or grid.crs is None or _epsg_of(src_crs) == grid.epsg:
        return warp(src, src_transform, grid, resampling, src_nodata, nodata, dtype, src_layout, layout, out, channel_offset, keep, src_origin, src_dtype)
    _check_reproject_method(resampling)
    m = _reproject_map(grid, src_crs, src_transform)
    return _resample(src, (0.0, 0.0, 0.0, 0.0), m, grid, resampling, src_nodata, nodata, dtype, src_layout, layout, out, channel_offset, keep, src_origin, src_dtype)


_reproject_raster = reproject      # (the readers have a keyword of that name)


def reproject_window(src_transform, src_shape, src_crs, grid, resampling='nearest'):
    """`warp_window` across two coordinate systems: the window (row0, col0, h, w) of a source raster of `src_crs` that `grid` needs, or
    None when the grid misses the raster.  The centres of ALL boundary pixels of the grid are transformed (the map between two
    projections is a homeomorphism: the extremes of u and v over the grid lie on its boundary); the window runs from floor(min) to
    floor(max), widened by the method's margin (0 / 1 / 2) and by one pixel more -- the host's and the device's libm may differ in the
    last bits -- and clipped to the raster.  When some boundary pixel lies outside a projection's domain the extremes are unknown: the
    window is the whole raster; when every one does: None."""
    _check_reproject_method(resampling)
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    a_s, _, c_s, _, e_s, f_s = _check_transform(src_transform, 'the source')
    a_d, _, c_d, _, e_d, f_d = grid.transform
    H, W = grid.shape
    jj = np.concatenate([np.arange(W), np.arange(W), np.zeros(H), np.full(H, W - 1)]).astype(np.float64)
    ii = np.concatenate([np.zeros(W), np.full(W, H - 1), np.arange(H), np.arange(H)]).astype(np.float64)
    xs, ys = transform_points(a_d * (jj + 0.5) + c_d, e_d * (ii + 0.5) + f_d, grid.crs, src_crs)
    ok = ~np.isnan(xs)
    if not ok.any():
        return None
    if not ok.all():
        return 0, 0, int(src_shape[0]), int(src_shape[1])
    u, v = (xs - c_s) / a_s, (ys - f_s) / e_s
    m = _WARP_MARGIN[resampling] + 1
    out = []
    for w_, n_src in ((v, src_shape[0]), (u, src_shape[1])):
        lo, hi = int(np.floor(w_.min())) - m, int(np.floor(w_.max())) + m
        lo, hi = max(lo, 0), min(hi, int(n_src) - 1)
        if lo > hi:
            return None
        out.append((lo, hi - lo + 1))
    return out[0][0], out[1][0], out[0][1], out[1][1]
