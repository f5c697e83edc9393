"""The writers of the reference's utils/raster_tools.py (:367-461 `numpy_to_raster`, `arrays_to_cog`) without rasterio and GDAL: a map
that lies on the device is written as a Cloud-Optimized GeoTIFF -- tiled, with overviews, COMPRESS=LZW, nodata = 255 -- from there.
The second part of the file is the way back (`read_cog`, `read_stack`): what the reference asks of rasterio's `open().read(window=)`
and rioxarray's `open_rasterio` (utils/pc_tools.py:131-186, 328-386).  The third aligns rasters that do not share a pixel grid
(`union_grid`, `warp`, `read_warped`, `read_mosaic`, `read_aligned_stack`): stackstac's, BuildVRT's and reproject_match's part; the end
of the file takes points, bounds and rasters between coordinate systems (`transform_points`, `transform_bounds`, `reproject_grid`,
`pixel_coords`, `reproject`, and `reproject=True` of the readers): PROJ's part behind gdal.Warp and stackstac.stack(epsg=).

    map (host array or CUDA tensor) -> satcv_raster_convert (dtype, nodata) -> satcv_raster_overview (the pyramid, level by level)
      -> satcv_raster_tiles (tile-major layout, predictor 2) -> satcv_lzw_tiles (every tile of every level in one launch)
      -> satcv_bytes_compact -> one device-to-host copy of the file's tile payload -> header + IFDs + payload on disk

The container (tag tables, `build_container`, `read_info`, `LevelInfo`, a level's window and block plan) is host code without torch in
`tiff_container`, whose names are imported here; this file holds what touches the device.  Three private types carry it: `_View`, a raster on
the device (every descriptor is filled from one); `_Mapping`, where a grid's pixels lie on a source (one CRS or two: method check, source window,
pixel size, launch arguments); `_File`, a file whose container is parsed once per public call.  The overview resampling rules are defined here
(include/satcv.h, satcv_raster_overview), not GDAL's, whose COG default is cubic.  Out of scope: BigTIFF, the float predictor 3, `arrays_to_cog`'s
window-by-window assembly from .npy files (its body writes to an undefined `src`), cloud destinations, the chip and window helpers of utils/raster_tools.py.
"""
import ctypes as C
import os
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from functools import cached_property

import numpy as np
import torch

from . import ops
from ._lib import RasterDesc, RasterizeDesc, ReprojectMap, UntileDesc, WarpDesc, check, lib
from .crs import crs_params, crs_struct
from .polygons import (convert, convert_poly_coords, edge_table, geometry_rings, get_centroid, make_jittered_window, make_window,      # noqa: F401
                       rings_bounds, to_pixels, win_jitter)
from .prediction_tools import _device_empty, _to_device
from .tiff_container import (DTYPES, LevelInfo, _COMPRESSION, _expected_bytes, _levels, _plan_read, _window_transform,      # noqa: F401
                             build_container, overview_shapes, parse_crs, read_info, tile_grid, write_tiles)

_RESAMPLING = {'nearest': 0, 'average': 1, 'mode': 2}


# ----------------------------------------------------------------------------------------------------------------- arguments
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


def _chw_or_hwc(layout):
    if layout not in ('hwc', 'chw'):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    return 0 if layout == 'hwc' else 1


def lzw_encode(data):
    """TIFF LZW of a bytes-like object on the CPU (satcv_lzw_encode_host, the coder the device runs per tile)"""
    data = bytes(data)
    cap = 2 * len(data) + 16
    dst = C.create_string_buffer(cap)
    size = C.c_int64()
    check(lib.satcv_lzw_encode_host(data, len(data), dst, cap, C.byref(size)))
    return dst.raw[:size.value]


def _pool():
    """the thread pool of the host codecs (zlib and the host LZW decoder release the interpreter lock): at most 16 threads"""
    return ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1)))


# ----------------------------------------------------------------------------------------------------------------- a raster on the device
# kind names: of a torch dtype and of a NumPy dtype (float64 is converted to float32 before a kernel reads it)
_TENSOR_KINDS = {getattr(torch, k): v for k, v in {**{k: k for k in DTYPES}, 'float64': 'float32'}.items() if hasattr(torch, k)}
_ARRAY_KINDS = {**{np.dtype(v[0]): k for k, v in DTYPES.items()}, np.dtype(np.float64): 'float32'}
_TORCH_OF = {'uint8': 'uint8', 'uint16': 'int16', 'int16': 'int16', 'int32': 'int32', 'float32': 'float32'}      # storage of a kind (bytes only)


def _torch_dtype(name):
    if name == 'uint16':
        return torch.uint16 if hasattr(torch, 'uint16') else torch.int16      # (bytes only, where this torch has no uint16)
    return getattr(torch, name)


class _View(namedtuple('_View', 'owner ptr kind h w c ld coff layout flat')):
    """A raster where it lies: owner (the tensor that holds the samples; for the writer, before `on_device`, it may be a host array),
    ptr (the address of channel 0 of pixel 0 of the ld-wide raster), kind (name), h, w, c, ld (the channel count of the owner), coff
    (the first of the c channels), layout (0 'hwc', 1 'chw'), flat (the owner is (H, W)).  `_desc`, WarpDesc and UntileDesc are filled from it."""
    __slots__ = ()

    def on_device(self):
        """the view with its samples resident: a host array goes up once, float64 becomes float32 first (a host array on the host)"""
        obj = self.owner
        if isinstance(obj, torch.Tensor):
            if obj.dtype != torch.float64:
                return self
            obj = obj.to(torch.float32).contiguous()
            return self._replace(owner=obj, ptr=obj.data_ptr(), ld=self.c, coff=0)
        t = _to_device(obj.astype(np.float32) if obj.dtype == np.float64 else obj, 'the map')
        return self._replace(owner=t, ptr=t.data_ptr())


def _packed_view(t, kind, shape):                              # a contiguous raster of `shape` (h, w, c) and `kind` in the tensor `t`
    return _View(owner=t, ptr=t.data_ptr(), kind=kind, h=shape[0], w=shape[1], c=shape[2], ld=shape[2], coff=0, layout=0, flat=False)


def _source_view(arr, layout='hwc', src_dtype=None, writer=False):
    """What a source is, without touching the device: -> `_View`.  A CUDA tensor is read where it lies: (H, W[, C]) for 'hwc', contiguous or a channel slice
    of a contiguous (H, W, ld) tensor, or a contiguous (C, H, W) / (H, W) for 'chw'; src_dtype names the kind whose bytes it stores.  writer=True: host arrays and float64 too."""
    resident = isinstance(arr, torch.Tensor) and arr.is_cuda
    if not writer and not resident:
        raise ValueError('warp takes a resident raster: a CUDA tensor')
    if not writer and arr.dtype == torch.float64:
        raise ValueError('a resident raster is uint8, uint16, int16, int32 or float32, got torch.float64')
    lay = _chw_or_hwc(layout)
    kinds = _TENSOR_KINDS if resident else _ARRAY_KINDS
    if lay == 1:
        if arr.dim() not in (2, 3) or 0 in arr.shape or not arr.is_contiguous():
            raise ValueError(f"a 'chw' source is a contiguous, non-empty (C, H, W) or (H, W) CUDA tensor, got shape {tuple(arr.shape)}")
        if arr.dtype not in kinds:
            raise ValueError(f'a resident raster is uint8, uint16, int16, int32 or float32, got {arr.dtype}')
        c, h, w = ((1,) + tuple(arr.shape))[-3:]
        if c > 16:
            raise ValueError(f'{c} bands: a raster has at most 16')
        ld, coff, ptr = c, 0, arr.data_ptr()
    else:
        if not resident:
            arr = np.asarray(arr.numpy() if isinstance(arr, torch.Tensor) else arr)
        if arr.dtype not in kinds:
            raise ValueError(f'a map is uint8, uint16, int16, int32, float32 or float64, got {arr.dtype}')
        shape = tuple(arr.shape)
        if len(shape) not in (2, 3) or 0 in shape:
            raise ValueError(f'expected a non-empty (H, W) or (H, W, C) map, got shape {shape}')
        h, w, c = shape[0], shape[1], (shape[2] if len(shape) == 3 else 1)
        if c > 16:
            raise ValueError(f'{c} bands: a map has at most 16')
        ld, coff, ptr = c, 0, None
        if resident:
            ld = int(arr.stride(1)) if w > 1 else (int(arr.stride(0)) if h > 1 else c)
            if not (ld >= c and (w == 1 or arr.stride(1) == ld) and (h == 1 or arr.stride(0) == w * ld) and (arr.dim() == 2 or c == 1 or arr.stride(2) == 1)):
                raise ValueError(f'a tensor map is contiguous (H, W[, C]) or a channel slice t[..., a:b] of a contiguous (H, W, ld) tensor; '
                                 f'got shape {shape} with strides {tuple(arr.stride())}')
            coff = int(arr.storage_offset()) % ld
            coff = 0 if coff + c > ld else coff               # (a view that starts inside a row of its base: the descriptor reads from its first sample)
            ptr = arr.data_ptr() - coff * arr.element_size()
    name = kinds[arr.dtype]
    if src_dtype is not None:
        if src_dtype not in DTYPES or np.dtype(DTYPES[src_dtype][0]).itemsize != arr.element_size() or (src_dtype == 'float32') != (name == 'float32'):
            raise ValueError(f'src_dtype {src_dtype!r} does not describe a tensor of {arr.dtype}')
        name = src_dtype
    return _View(owner=arr, ptr=ptr, kind=name, h=int(h), w=int(w), c=int(c), ld=int(ld), coff=int(coff), layout=lay, flat=len(arr.shape) == 2)


def _dest_view(shape, c, kind, dtype, layout, out=None, channel_offset=0, flat=False):
    """Where a result of `c` channels on a grid of `shape` goes: -> `_View`.  kind: the source's; dtype: None keeps it, 'float32' converts.
    Without `out` a new (H, W, c) / (c, H, W) tensor ((H, W) for `flat`); with it the channels channel_offset ... of that tensor, checked
    against grid, layout and kind."""
    dname = kind if dtype is None else dtype
    if dname not in (kind, 'float32'):
        raise ValueError(f'dtype must be None, {kind!r} (the source) or \'float32\', got {dtype!r}')
    lay = _chw_or_hwc(layout)
    (H, W), ld, coff = shape, c, 0
    if out is None:
        out = _device_empty((H, W) if flat else ((H, W, c) if lay == 0 else (c, H, W)), _torch_dtype(dname), 'the warped raster')
    else:
        nt = np.dtype(DTYPES[dname][0])
        want = '(H, W, ld)' if lay == 0 else '(ld, H, W)'
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dim() in (2, 3)):
            raise ValueError(f'out must be a contiguous CUDA tensor of shape {want} or (H, W)')
        hw = tuple(out.shape) if out.dim() == 2 else (tuple(out.shape[:2]) if lay == 0 else tuple(out.shape[1:]))
        ld, coff, flat = (1 if out.dim() == 2 else int(out.shape[2] if lay == 0 else out.shape[0])), int(channel_offset), out.dim() == 2
        if hw != (H, W):
            raise ValueError(f'out is {hw[0]} x {hw[1]}, the grid {H} x {W}')
        if dtype is None and out.dtype == torch.float32:
            dname, nt = 'float32', np.dtype(np.float32)
        if out.element_size() != nt.itemsize or out.dtype.is_floating_point != (nt.kind == 'f') or out.dtype == torch.float64:
            raise ValueError(f'out is {out.dtype}, the result {dname}')
        if coff < 0 or coff + c > ld:
            raise ValueError(f'channels {coff} ... {coff + c - 1} do not fit the {ld} of out')
    return _View(owner=out, ptr=out.data_ptr(), kind=dname, h=H, w=W, c=c, ld=ld, coff=coff, layout=lay, flat=flat)


def _filled(shape, c, kind, nodata, layout, out, channel_offset, what, fill=True):
    """The destination of a reader that has nothing to resample into it (yet): -> (tensor, kind name).  Without `out` a new (H, W, c) / (c, H, W)
    tensor of `kind`, named `what` in a MemoryError; with it `out` as given -- nothing about it is refused here, `warp` does that once a file is
    read -- whose kind is float32 if it is a floating tensor.  Unless `fill` is False for a given `out`, every sample of the channels
    channel_offset ... channel_offset + c - 1 becomes nodata, without one NaN (float32) or 0."""
    chans = slice(channel_offset, channel_offset + c)
    if out is None:
        part = out = _device_empty(shape + (c,) if _chw_or_hwc(layout) == 0 else (c,) + shape, _torch_dtype(kind), what)
    elif not fill:
        return out, kind
    else:
        kind = 'float32' if out.dtype.is_floating_point else kind
        part = out if out.dim() == 2 else (out[..., chans] if layout == 'hwc' else out[chans])
    if kind == 'float32':
        part.fill_(float(nodata if nodata is not None else 'nan'))
    else:                                                     # (by bytes: uint16 may be stored as int16)
        nt = np.dtype(DTYPES[kind][0])
        store, bits = {1: (torch.uint8, np.uint8), 2: (torch.int16, np.int16), 4: (torch.int32, np.int32)}[nt.itemsize]
        part.view(store).fill_(int(np.array(nodata or 0, nt).view(bits)))
    return out, kind


_stage_hook = None       # tools/cog_probe.py and tools/cog_read_probe.py set a callable: it receives a stage's name once the stage's launches are issued


def _mark(stage):
    if _stage_hook is not None:
        _stage_hook(stage)


def _desc(src, dst, dst_kind, scale=0.0, nodata=None, resampling=0, blocksize=0, predictor=0):
    """satcv_raster_desc: the `_View` src read into the tensor `dst` of kind `dst_kind`"""
    return RasterDesc(src=src.ptr, src_kind=DTYPES[src.kind][1], h=src.h, w_=src.w, c=src.c, ld=src.ld, coff=src.coff, dst=dst.data_ptr(),
                      dst_kind=DTYPES[dst_kind][1], scale=float(scale or 0.0), has_nodata=int(nodata is not None),
                      nodata=float(nodata if nodata is not None else 0.0), resampling=resampling, blocksize=blocksize, predictor=int(bool(predictor)))


def to_float32(tensor, dtype, what='the float32 copy', as_raster=False):
    """An integer raster or stack on the device cast to float32 there: -> a new CUDA tensor of the same shape (satcv_raster_convert,
    exact for 8- and 16-bit samples and for 32-bit ones within +-2^24).  tensor: contiguous, of any rank; dtype: the name of its kind
    ('uint16' for an int16 tensor that stores uint16 bytes); what: names the copy in a MemoryError.  The kernel is told rows x last
    axis x one channel, so the tensor holds fewer than 2^31 samples; as_raster=True describes an (H, W, C) tensor, C <= 16, as that
    raster, and the limit is 2^31 pixels (a whole scene: `prediction_tools.predict_raster`)."""
    f32 = _device_empty(tuple(tensor.shape), torch.float32, what)
    shape = tuple(tensor.shape) if as_raster else (tensor.numel() // int(tensor.shape[-1]), int(tensor.shape[-1]), 1)
    check(lib.satcv_raster_convert(C.byref(_desc(_packed_view(tensor, dtype, shape), f32, 'float32')), ops.stream_ptr()))
    return f32


# ----------------------------------------------------------------------------------------------------------------- the writer
def _device_pyramid(view, dtype, shapes, nodata=None, scale=None, resampling='nearest'):
    """The converted map and its overviews as packed views (h, w, C), full resolution first.  A map that already is a contiguous
    raster of `dtype` is read where it lies."""
    view = view.on_device()
    _mark('upload')
    td = getattr(torch, _TORCH_OF[dtype])
    st = ops.stream_ptr()
    if not (dtype == view.kind and view.ld == view.c and view.coff == 0 and scale is None):
        base = _device_empty((view.h, view.w, view.c), td, 'the converted map')
        check(lib.satcv_raster_convert(C.byref(_desc(view, base, dtype, scale=scale, nodata=nodata)), st))
        view = _packed_view(base, dtype, (view.h, view.w, view.c))
    _mark('convert')
    levels = [view]
    for oh, ow in shapes[1:]:
        nxt = _device_empty((oh, ow, view.c), td, 'an overview')
        check(lib.satcv_raster_overview(C.byref(_desc(levels[-1], nxt, dtype, nodata=nodata, resampling=_RESAMPLING[resampling])), st))
        levels.append(_packed_view(nxt, dtype, (oh, ow, view.c)))
    _mark('pyramid')
    return levels


def device_pyramid(arr, dtype=None, nodata=255, scale=None, blocksize=512, overviews='auto', resampling='nearest'):
    """The first two stages of `write_cog` on their own: the map converted to `dtype` and its overviews, as device tensors [(h, w, C)],
    full resolution first.  Arguments as for `write_cog`."""
    view, dtype, shapes, _ = _plan(arr, dtype, nodata=nodata, scale=scale, blocksize=blocksize, overviews=overviews, resampling=resampling)
    return [lv.owner for lv in _device_pyramid(view, dtype, shapes, nodata=nodata, scale=scale, resampling=resampling)]


def _plan(arr, dtype, nodata, scale, blocksize, overviews, resampling, compress=None, predictor=False, transform=(0,) * 6):
    """every check of `write_cog` that needs no device: -> (`_View` of the map, dtype name, [(h, w)] of the levels, full resolution
    first, the transform as six floats)"""
    view = _source_view(arr, writer=True)
    dtype = view.kind if dtype is None else dtype
    transform = _check_options(dtype, nodata, compress, predictor, blocksize=blocksize, resampling=resampling, transform=transform)
    if scale is not None and view.kind != 'float32':
        raise ValueError('scale is for float32 sources only')
    tile_bytes = int(blocksize) ** 2 * view.c * np.dtype(DTYPES[dtype][0]).itemsize
    if tile_bytes >= 1 << 30:
        raise ValueError(f'a tile of {tile_bytes} bytes: tiles stay below 2^30 bytes, lower blocksize')
    return view, dtype, [(view.h, view.w)] + overview_shapes(view.h, view.w, int(blocksize), overviews), transform


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
    parse_crs(crs)
    view, dtype, shapes, transform = _plan(arr, dtype, nodata=nodata, scale=scale, blocksize=blocksize, overviews=overviews, resampling=resampling,
                                           compress=compress, predictor=predictor, transform=transform)
    blocksize, C_ = int(blocksize), view.c
    tile_bytes = blocksize * blocksize * C_ * np.dtype(DTYPES[dtype][0]).itemsize
    levels = _device_pyramid(view, dtype, shapes, nodata=nodata, scale=scale, resampling=resampling)
    container = dict(compress=compress, predictor=predictor, nodata=nodata, transform=transform, crs=crs)
    ntiles = [int(np.prod(tile_grid(h, w, blocksize))) for h, w in shapes]
    n = sum(ntiles)
    st = ops.stream_ptr()
    # every level's tiles in one buffer, in file order: the smallest overview first
    tiles = _device_empty((n, tile_bytes), torch.uint8, 'the tile buffer')
    first = {}
    at = 0
    for k in reversed(range(len(levels))):
        first[k] = at
        d = _desc(levels[k], tiles, dtype, nodata=nodata, blocksize=blocksize, predictor=predictor)
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
        head, offsets, total = build_container(shapes, dtype, C_, blocksize, byte_counts=per_level, **container)
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
    if compress is None:
        blobs = [raw[i].tobytes() for i in range(n)]
    else:
        with _pool() as ex:                                    # (zlib level 6)
            blobs = list(ex.map(lambda i: zlib.compress(raw[i].data, 6), range(n)))
    _mark('deflate')
    per_level = [blobs[first[k]:first[k] + ntiles[k]] for k in range(len(levels))]
    write_tiles(out_file, shapes, per_level, dtype, bands=C_, blocksize=blocksize, **container)
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
#     container parsed on the host (read_info, once per file and call: _File) -> the blocks the window touches, read into ONE pinned
#       buffer behind their offsets, sizes and indices -> one host-to-device copy -> satcv_lzw_decode_tiles (one wavefront per block)
#       -> satcv_raster_untile (predictor 2, window, band subset, destination layout) -> a device tensor in the file's own kind
#
# Deflate blocks are inflated on the host (zlib, at most 16 threads) and go up raw; uncompressed blocks go up as they are; decode='host'
# does the same for LZW with satcv_lzw_decode_host.  What is read and what is refused: tiff_container.
STATUS_NAMES = {0: 'ok', 1: 'truncated input', 2: 'bad code', 3: 'overlong'}       # satcv_lzw_decode_tiles


class Raster:
    """What `read_cog` returns: array (a CUDA tensor, or a NumPy array with device=False), transform (Affine order, of the window and
    level that were read), crs ('EPSG:n' or None), nodata, dtype (name of the file's kind)."""
    __slots__ = ('array', 'transform', 'crs', 'nodata', 'dtype')

    def __init__(self, array, transform, crs, nodata, dtype):
        self.array, self.transform, self.crs, self.nodata, self.dtype = array, transform, crs, nodata, dtype


class _File:
    """A file whose container is parsed on first use and once: `levels` (the image and its overview chain) and their `transforms`.  The readers
    make one per path at the top of a public call and hand it down in the path's place."""

    def __init__(self, path):
        self.path = path

    @cached_property
    def levels(self):
        return _levels(read_info(self.path))

    @cached_property
    def transforms(self):
        base = self.levels[0]
        return [_window_transform(base.transform, base.shape, lv.shape, row0=0, col0=0) for lv in self.levels]


def _files(paths):                                             # [_File] of paths (a record passes), one record per distinct path
    known = {}
    return [p if isinstance(p, _File) else known.setdefault(p, _File(p)) for p in paths]


def level_window(info, window=None):
    """The checked window of a `LevelInfo` and where it lies: -> ((row0, col0, h, w), its transform in Affine order, None for a level
    without one).  window: None is the whole level; ValueError as `read_cog` raises it for a window outside the image."""
    window = _plan_read(info, window, None)[0]
    return window, _window_transform(info.transform, info.shape, info.shape, row0=window[0], col0=window[1])


def lzw_decode(stream, cap):
    """TIFF LZW of a bytes-like object decoded on the CPU (satcv_lzw_decode_host): -> (status, bytes), at most `cap` bytes"""
    stream = bytes(stream)
    dst = C.create_string_buffer(max(int(cap), 1))
    size, status = C.c_int64(), C.c_int32()
    check(lib.satcv_lzw_decode_host(stream, len(stream), dst, int(cap), C.byref(size), C.byref(status)))
    return status.value, dst.raw[:size.value]


def _refuse_block(t, status, stream):
    first = (int.from_bytes(bytes(stream[:2]), 'big') >> 7) if len(stream) >= 2 else 256
    hint = '' if first == 256 else ("; the stream does not open with a Clear code (its first 9 bits, MSB-first, are %d): this may be the LSB-first "
                                    "'old-style' LZW, which is not supported" % first)
    raise ValueError(f'block {t} does not decode: status {status} ({STATUS_NAMES.get(status, "?")})' + hint)


def _read_blocks(path, info, blocks, into=None, rel=None):
    """the bytes of the planned blocks from the file: a list of byte strings, or -- with `into` -- block j read into into[rel[j]:]"""
    slices = []
    with open(path, 'rb') as f:
        for j, (o, c) in enumerate(zip(info.offsets[blocks], info.counts[blocks])):
            f.seek(int(o))
            if into is None:
                slices.append(f.read(int(c)))
            else:
                f.readinto(memoryview(into[int(rel[j]):int(rel[j]) + int(c)]))
    return slices


def _decode_host(info, blocks, slices, into, stride):
    """the blocks decoded on the host into `into` (a uint8 array), block j at j * stride; at most 16 threads"""
    want = _expected_bytes(info, blocks)

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
            check(lib.satcv_lzw_decode_host(bytes(raw), len(raw), dst.ctypes.data, info.block_bytes, C.byref(size), C.byref(status)))
            if status.value or size.value < want[j]:
                _refuse_block(blocks[j], status.value if status.value else 1, raw)
            return
        if len(got) < want[j]:
            raise ValueError(f'block {blocks[j]} holds {len(got)} bytes, {want[j]} are needed')
        dst[:min(len(got), stride)] = np.frombuffer(got, np.uint8)[:stride]
    with _pool() as ex:
        list(ex.map(one, range(len(blocks))))


def _untile_host(info, blocks, raw, stride, window, bands, layout):
    """NumPy counterpart of satcv_raster_untile for device=False"""
    bh, bw = info.block_shape
    dt = np.dtype(DTYPES[info.dtype][0])
    across, per_plane = info.across, info.across * info.down
    row0, col0, h, w = window
    out = np.zeros((h, w, len(bands)), dt)
    for j, t in enumerate(blocks):
        plane, t2 = (t // per_plane, t % per_plane) if info.planar == 2 else (0, t)
        by, bx = t2 // across, t2 % across
        blk = raw[j * stride:j * stride + info.block_bytes].view(dt).reshape(bh, bw, info.block_samples)
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


def default_decode(info):
    """where `read_cog(decode=None)` decodes LZW blocks: the choice tools/cog_read_probe.py measured per input class ("Reading
    GeoTIFFs")"""
    return 'host'


def _plan_cog(f, window, level, bands, layout, device, decode, out):
    """every check of `read_cog` that needs no device: -> (LevelInfo, (row0, col0, h, w), band list, block indices, where LZW is decoded, array -> `Raster`)"""
    _chw_or_hwc(layout)
    if decode not in (None, 'host', 'device'):
        raise ValueError(f"decode must be 'host', 'device' or None, got {decode!r}")
    levels = f.levels
    if isinstance(level, bool) or int(level) != level or not 0 <= level < len(levels):
        raise ValueError(f'level {level!r}: the file has levels 0 ... {len(levels) - 1}')
    info = levels[int(level)]
    window, bands, blocks = _plan_read(info, window, bands)
    if info.compression != 'lzw':
        decode = 'host'
    elif decode is None:
        decode = default_decode(info) if device else 'host'
    if decode == 'device' and not device:
        raise ValueError("decode='device' leaves the raster on the device: it needs device=True")
    if out is not None and not device:
        raise ValueError('out is a CUDA tensor: it needs device=True')
    transform = _window_transform(levels[0].transform, levels[0].shape, info.shape, row0=window[0], col0=window[1])
    nodata = info.nodata if info.nodata is not None else levels[0].nodata
    return info, window, bands, blocks, decode, lambda arr: Raster(arr, transform, levels[0].crs, nodata=nodata, dtype=info.dtype)


def _untile_device(path, info, blocks, window, bands, layout, decode, out):
    """the device half of `read_cog`: the destination (new, or `out`, which must fit exactly), the blocks in one pinned buffer, one copy, the decode and untile launches"""
    (row0, col0, h, w), c, dt = window, len(bands), np.dtype(DTYPES[info.dtype][0])
    shape = (h, w, c) if layout == 'hwc' else (c, h, w)
    if out is None:
        out = _device_empty(shape, _torch_dtype(info.dtype), 'the raster')
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == shape and out.element_size() == dt.itemsize
              and out.dtype.is_floating_point == (dt.kind == 'f')):
        raise ValueError(f'out must be a contiguous CUDA tensor of shape {shape} and kind {info.dtype}')
    dst = _packed_view(out, info.dtype, (h, w, c))._replace(layout=_chw_or_hwc(layout))
    n, block_bytes, cnts = len(blocks), info.block_bytes, info.counts[blocks]
    stride = (block_bytes + 15) // 16 * 16
    # one pinned buffer: offsets (int64), sizes (int32) and block indices (int32) of the n blocks, then the payload
    head = 16 * n
    payload = int(cnts.sum()) if decode == 'device' else n * stride
    pinned = torch.empty(head + max(payload, 16), dtype=torch.uint8, pin_memory=True)
    buf = pinned.numpy()
    rel = np.concatenate([[0], np.cumsum(cnts)[:-1]]).astype(np.int64) if decode == 'device' else np.arange(n, dtype=np.int64) * stride
    buf[:8 * n].view(np.int64)[:] = rel
    buf[8 * n:12 * n].view(np.int32)[:] = cnts if decode == 'device' else block_bytes
    buf[12 * n:16 * n].view(np.int32)[:] = blocks
    if decode == 'device':
        _read_blocks(path, info, blocks, into=buf[head:], rel=rel)
    else:
        slices = _read_blocks(path, info, blocks)
        buf[head:head + payload] = 0
        _decode_host(info, blocks, slices, into=buf[head:head + payload], stride=stride)
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
    d = UntileDesc(src=src, src_stride=stride, blocks=base + 12 * n, nblocks=n, bh=info.block_shape[0], bw=info.block_shape[1], across=info.across,
                   per_plane=info.across * info.down, spp=info.bands, planar=info.planar, kind=DTYPES[info.dtype][1],
                   predictor=2 if info.predictor else 0, row0=row0, col0=col0, h=dst.h, w_=dst.w, dst=dst.ptr, layout=dst.layout,
                   ld=dst.ld, coff=dst.coff)
    for b in range(16):
        d.band_map[b] = bands.index(b) if b in bands else -1
    check(lib.satcv_raster_untile(C.byref(d), st))
    _mark('untile')
    if decode == 'device':
        got = flags.cpu().numpy()                              # the one host synchronisation: statuses and decoded lengths
        bad = np.nonzero((got[:n] != 0) | (got[n:] < np.asarray(_expected_bytes(info, blocks))))[0]
        if bad.size:
            j = int(bad[0])
            r, c = int(rel[j]), int(cnts[j])
            _refuse_block(blocks[j], int(got[j]) if got[j] else 1, buf[head + r:head + r + c])
    else:
        torch.cuda.current_stream().synchronize()              # the pinned buffer is released only after the copy
    _mark('status')
    return dst.owner


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
    ValueError: what `read_info` refuses, a window outside the image, and a block that does not decode (its index and status).
    Inside the package `path` may be a `_File`, a file that is already parsed: `read_warped` and `read_stack` come in through this name."""
    f = path if isinstance(path, _File) else _File(path)
    info, window, bands, blocks, decode, result = _plan_cog(f, window, level, bands, layout=layout, device=device, decode=decode, out=out)
    if not device:
        stride = (info.block_bytes + 15) // 16 * 16
        raw = np.zeros(len(blocks) * stride, np.uint8)
        _decode_host(info, blocks, _read_blocks(f.path, info, blocks), into=raw, stride=stride)
        return result(_untile_host(info, blocks, raw, stride, window=window, bands=bands, layout=layout))
    return result(_untile_device(f.path, info, blocks, window, bands=bands, layout=layout, decode=decode, out=out))


def read_stack(paths, window=None, bands=None):
    """The files of a time series as one resident stack: -> (stack, transform, crs, nodata), stack a (T, C, H, W) CUDA tensor in the
    files' kind -- what `pc_tools.median_composite`, `ee_tools.mask` and `pc_tools.predict_change` take.  Every file is decoded straight
    into its slot (`read_cog(..., layout='chw', out=stack[t])`).  The files must agree on shape, kind, transform and CRS: ValueError
    names the first that differs."""
    files = _files(paths)
    if not files:
        raise ValueError('read_stack needs at least one file')
    first = files[0].levels[0]
    for f in files[1:]:
        for what in ('shape', 'bands', 'dtype', 'transform', 'epsg'):
            if getattr(f.levels[0], what) != getattr(first, what):
                raise ValueError(f'{f.path} differs from {files[0].path} in {what}: {getattr(f.levels[0], what)!r} against {getattr(first, what)!r}')
    window, bands, _ = _plan_read(first, window, bands)
    stack = _device_empty((len(files), len(bands), window[2], window[3]), _torch_dtype(first.dtype), 'the time stack')
    for t, f in enumerate(files):
        r = read_cog(f, window, 0, bands, layout='chw', out=stack[t])
    return stack, r.transform, r.crs, r.nodata


# ---------------------------------------------------------------------------------------------------------------------------------
# Alignment: rasters brought onto one pixel grid, on the device.
#
#     grids on the host (Grid, union_grid) -> where the grid lies on a source (_Mapping: one CRS or two) -> the window of the file the
#       grid needs (read_cog) -> satcv_raster_warp / satcv_raster_reproject (nearest / bilinear / cubic / average, nodata-aware, into a
#       new raster, a slot of a stack or a channel range of a scene)
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
    epsg = property(lambda self: _epsg_of(self[2]))
    resolution = property(lambda self: (abs(self[0][0]), abs(self[0][4])))

    @property
    def bounds(self):
        a, _, c, _, e, f = self[0]
        H, W = self[1]
        xs, ys = (c, c + W * a), (f, f + H * e)
        return min(xs), min(ys), max(xs), max(ys)

    def __repr__(self):
        return f'Grid(transform={self[0]!r}, shape={self[1]!r}, crs={self[2]!r})'


def _a_grid(grid):
    if not isinstance(grid, Grid):
        raise ValueError(f'grid must be a Grid, got {type(grid).__name__}')
    return grid


def _as_grid(source, what=None):
    """a path, a LevelInfo (of the file `what`) or a Grid as a Grid"""
    if isinstance(source, Grid):
        return source
    if not isinstance(source, LevelInfo):
        source, what = read_info(source)[0], str(source)
    _check_transform(source.transform, what or f'IFD {source.index}')
    return Grid(source.transform, source.shape, source.crs)


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


class _Mapping:
    """Where the pixels of a destination `Grid` lie on a source raster of `transform` and `src_crs`.  Construction decides how: foreign
    -- every pixel goes through both projections, `reproject`'s rules -- when reprojection is allowed and the two sides name different EPSG
    codes; otherwise the two share a CRS (or one names none) and the map is affine, `warp`'s rules.  `foreign=` states the decision instead
    (another level of the same file; `reproject_window`, which always goes through the projections).  With `what`, the name of the two sides,
    construction also raises what the readers refuse about the codes before a file is read: two different ones, and with reproject=True a
    code `crs.crs_params` does not know.  The methods answer everything that depends on the decision."""
    def __init__(self, transform, src_crs, grid, reproject=False, foreign=None, what=None):
        if foreign is None:
            foreign = bool(reproject) and None not in (src_crs, grid.crs) and _epsg_of(src_crs) != grid.epsg
        self.transform, self.src_crs, self.grid, self.foreign = transform, src_crs, grid, foreign
        if what is not None and foreign:
            for code in (_epsg_of(src_crs), grid.epsg):
                crs_params(code)
        elif what is not None:
            _common_epsg([_epsg_of(src_crs), grid.epsg], what)

    def at(self, transform):                                   # (the same mapping for another level of the source's file)
        return _Mapping(transform, self.src_crs, self.grid, foreign=self.foreign)

    @cached_property
    def launch(self):
        """((su, ou, sv, ov) of satcv_raster_warp, None), or (zeros, the `ReprojectMap` of satcv_raster_reproject); the transforms are checked once"""
        if self.foreign:
            return (0.0, 0.0, 0.0, 0.0), _reproject_map(self.grid, self.src_crs, self.transform)
        return warp_coefficients(self.transform, self.grid.transform), None

    def check_method(self, resampling):
        """ValueError for an unknown method, for 'average' over more than 64 source pixels and for 'average' across two CRSs"""
        # (the coefficients first: what `warp_coefficients` refuses about the transforms comes before what is refused about the method)
        su, _, sv, _ = (0.0,) * 4 if self.foreign else self.launch[0]
        if resampling not in WARP_RESAMPLING:
            raise ValueError(f'resampling must be one of {sorted(WARP_RESAMPLING)}, got {resampling!r}')
        if resampling == 'average' and self.foreign:
            raise ValueError("resampling='average' between two coordinate systems is not done (a pixel's footprint is no axis-parallel rectangle): "
                             "read an overview with level='auto' and resample it with 'bilinear'")
        if resampling == 'average' and max(abs(su), abs(sv)) > MAX_AVERAGE_SCALE:
            raise ValueError(f"resampling='average' over a footprint of {abs(sv):.4g} x {abs(su):.4g} source pixels (at most {MAX_AVERAGE_SCALE} per axis): "
                             "read an overview of the source instead (level='auto')")

    def window(self, src_shape, resampling):
        """`warp_window` or `reproject_window`: one rule each for the pixels the grid needs, one clip to the raster"""
        self.check_method(resampling)
        spans = self._foreign_spans(src_shape, resampling) if self.foreign else self._affine_spans(resampling)
        out = []
        for (lo, hi), n_src in zip(spans or (), src_shape):
            lo, hi = max(lo, 0), min(hi, int(n_src) - 1)
            if lo > hi:
                return None
            out.append((lo, hi - lo + 1))
        return (out[0][0], out[1][0], out[0][1], out[1][1]) if out else None

    def _affine_spans(self, resampling):
        """per axis (rows, columns) the first and last source pixel: under the grid's sample points plus the margin; 'average': the footprint"""
        (su, ou, sv, ov), spans = self.launch[0], []
        for s, o, n_dst in ((sv, ov, self.grid.shape[0]), (su, ou, self.grid.shape[1])):
            if resampling == 'average':
                ends = (s * 0.0 + o, s * float(n_dst) + o)
                spans.append((int(np.floor(min(ends))), int(np.ceil(max(ends))) - 1))
            else:
                ends, m = (s * 0.5 + o, s * (n_dst - 0.5) + o), _WARP_MARGIN[resampling]
                spans.append((int(np.floor(min(ends))) - m, int(np.floor(max(ends))) + m))
        return spans

    def _foreign_spans(self, src_shape, resampling):
        """the same from the centres of all boundary pixels of the grid, one pixel more; the whole raster when some lie outside a domain, None when all do"""
        grid = _a_grid(self.grid)
        a_s, _, c_s, _, e_s, f_s = _check_transform(self.transform, 'the source')
        a_d, _, c_d, _, e_d, f_d = grid.transform
        H, W = grid.shape
        jj = np.concatenate([np.arange(W), np.arange(W), np.zeros(H), np.full(H, W - 1)]).astype(np.float64)
        ii = np.concatenate([np.zeros(W), np.full(W, H - 1), np.arange(H), np.arange(H)]).astype(np.float64)
        xs, ys = transform_points(a_d * (jj + 0.5) + c_d, e_d * (ii + 0.5) + f_d, grid.crs, self.src_crs)
        ok = ~np.isnan(xs)
        if not ok.any():
            return None
        if not ok.all():
            return [(0, int(n) - 1) for n in src_shape[:2]]
        m = _WARP_MARGIN[resampling] + 1
        return [(int(np.floor(p.min())) - m, int(np.floor(p.max())) + m) for p in ((ys - f_s) / e_s, (xs - c_s) / a_s)]

    def pixel_size(self):
        """(px, py) of a source pixel in the grid's units; across two CRSs measured at the grid's centre (`measured_pixel_size`)"""
        if not self.foreign:
            return abs(self.transform[0]), abs(self.transform[4])
        a, _, c, _, e, f = self.grid.transform
        return measured_pixel_size(self.transform, self.src_crs, self.grid.crs, (c + 0.5 * self.grid.shape[1] * a, f + 0.5 * self.grid.shape[0] * e))


def warp_window(src_transform, src_shape, grid, resampling='nearest'):
    """The window (row0, col0, h, w) of a source raster that `grid` needs under `resampling`, or None when the grid misses the raster:
    the pixels under the grid's sample points and 0 (nearest), 1 (bilinear) or 2 (cubic) more on every side, for 'average' the pixels
    the grid's footprint touches; clipped to the raster."""
    return _Mapping(src_transform, None, grid).window(src_shape, resampling)


def auto_level(level_transforms, grid, src_crs=None):
    """level='auto' of `read_warped`: the index of the coarsest level whose pixels are no larger than the grid's on either axis (level 0
    when none is); level_transforms: the transform of every level, the image first.  src_crs: the files' CRS when it is not the grid's --
    a level's pixel size is then measured in the grid's CRS at the grid's centre (`measured_pixel_size`)."""
    m, (rx, ry) = _Mapping(None, src_crs, grid, reproject=True), grid.resolution
    best, size = 0, -1.0
    for k, t in enumerate(level_transforms):
        px, py = m.at(t).pixel_size()
        if px <= rx * (1 + 1e-9) and py <= ry * (1 + 1e-9) and px * py > size:
            best, size = k, px * py
    return best


def _resample(m, src, resampling, src_nodata=None, nodata=None, dtype=None, src_layout='hwc', layout='hwc', out=None, channel_offset=0, keep=False,
              src_origin=(0, 0), src_dtype=None):
    """The launch `warp`, `reproject` and `read_warped` share: the resident raster `src` onto the grid of the `_Mapping` m, by satcv_raster_warp or,
    where the mapping is foreign, satcv_raster_reproject.  Every refusal comes before the destination is allocated."""
    m.check_method(resampling)
    (su, ou, sv, ov), rmap = m.launch
    src = _source_view(src, src_layout, src_dtype)
    dst = _dest_view(m.grid.shape, src.c, src.kind, dtype, layout=layout, out=out, channel_offset=channel_offset, flat=src.flat)
    if nodata is None:
        nodata = src_nodata
    d = WarpDesc(src=src.ptr, src_kind=DTYPES[src.kind][1], src_layout=src.layout, sh=src.h, sw=src.w, src_ld=src.ld, src_coff=src.coff,
                 src_row0=int(src_origin[0]), src_col0=int(src_origin[1]), dst=dst.ptr, dst_kind=DTYPES[dst.kind][1], dst_layout=dst.layout, dh=dst.h, dw=dst.w,
                 dst_ld=dst.ld, dst_coff=dst.coff, dst_row0=0, dst_col0=0, c=src.c, su=su, ou=ou, sv=sv, ov=ov, resampling=WARP_RESAMPLING[resampling],
                 has_src_nodata=int(src_nodata is not None), src_nodata=float(src_nodata if src_nodata is not None else 0.0),
                 has_dst_nodata=int(nodata is not None), dst_nodata=float(nodata if nodata is not None else 0.0), keep=int(bool(keep)))
    if rmap is None:
        check(lib.satcv_raster_warp(C.byref(d), ops.stream_ptr()))
        _mark('warp')
    else:
        check(lib.satcv_raster_reproject(C.byref(d), C.byref(rmap), ops.stream_ptr()))
        _mark('reproject')
    return dst.owner


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
    return _resample(_Mapping(src_transform, None, _a_grid(grid)), src, resampling, src_nodata=src_nodata, nodata=nodata, dtype=dtype, src_layout=src_layout,
                     layout=layout, out=out, channel_offset=channel_offset, keep=keep, src_origin=src_origin, src_dtype=src_dtype)


def _file_mapping(f, grid, reproject=False):
    """the `_Mapping` of a file's image onto `grid`; ValueError for a file without a transform, a rotated one, or one in another CRS"""
    _check_transform(f.levels[0].transform, str(f.path))
    return _Mapping(f.transforms[0], f.levels[0].crs, grid, reproject=reproject, what=f'{f.path} and the grid')


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
    grid's CRS at the grid's centre.
    Inside the package `path` may be a `_File`, a file that is already parsed (`read_mosaic`, `read_aligned_stack`)."""
    f = _files([path])[0]
    m = _file_mapping(f, _a_grid(grid), reproject)
    if m.foreign:
        m.check_method(resampling)                             # (across two CRSs the method is refused before the level, with one CRS after it)
    levels, transforms = f.levels, f.transforms
    if level == 'auto':
        level = auto_level(transforms, grid, f.levels[0].crs)
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)) or not 0 <= level < len(levels):
        raise ValueError(f"level {level!r}: the file has levels 0 ... {len(levels) - 1} (or 'auto')")
    info, m = levels[int(level)], m.at(transforms[int(level)])
    src_nodata = info.nodata if info.nodata is not None else levels[0].nodata
    if nodata is None:
        nodata = src_nodata
    crs = grid.crs if grid.crs is not None else levels[0].crs
    window = m.window(info.shape, resampling)
    if window is None:
        c = len(_plan_read(info, None, bands)[1])
        arr, dname = _filled(grid.shape, c, info.dtype if dtype is None else dtype, nodata, layout=layout, out=out, channel_offset=channel_offset,
                             what='the warped raster', fill=not keep)
        return Raster(arr, grid.transform, crs, nodata=nodata, dtype=dname)
    r = read_cog(f, window, int(level), bands, decode=decode)
    arr = _resample(m, r.array, resampling, src_nodata=src_nodata, nodata=nodata, dtype=dtype, layout=layout, out=out, channel_offset=channel_offset,
                    keep=keep, src_origin=window[:2], src_dtype=info.dtype)
    return Raster(arr, grid.transform, crs, nodata=nodata, dtype='float32' if arr.dtype.is_floating_point else info.dtype)


def _same_kind(files, bands):
    """(dtype, number of bands read, nodata) the files share; ValueError names the first that differs in kind or band count"""
    first = files[0].levels[0]
    n = len(_plan_read(first, None, bands)[1])
    for f in files[1:]:
        i = f.levels[0]
        if i.dtype != first.dtype or (bands is None and i.bands != first.bands):
            raise ValueError(f'{f.path} differs from {files[0].path} in kind or bands: {i.dtype} x {i.bands} against {first.dtype} x {first.bands}')
    return first.dtype, n, first.nodata


def _footprint_x(f, grid):
    """the x of the centre of a file's footprint in the grid's CRS"""
    g = _as_grid(f.levels[0], str(f.path))
    left, bottom, right, top = g.bounds
    x, y = 0.5 * (left + right), 0.5 * (bottom + top)
    if g.epsg is not None and grid.epsg is not None and g.epsg != grid.epsg:
        xs, _ = transform_points([x], [y], g.crs, grid.crs)
        x = float(xs[0])
    return x


def _read_mosaic_equalized(files, grid, bands, resampling, level, layout, first, nodata, dtype, out, channel_offset, decode, reproject, name, c):
    """`read_mosaic(equalize=True)`: one slot per file, the chain of `calibration.equalize_collection` west to east, then every slot
    painted into the filled destination by satcv_calib_apply with keep.  Every refusal comes before the slots are allocated."""
    from . import calibration
    if name not in calibration.KINDS:
        raise ValueError(f'equalize=True bins uint8, uint16 and int16 files, got {name} (float32 needs a binning rule whose rounding can be pinned)')
    if nodata is None:
        raise ValueError('equalize=True needs a nodata value (the files\' or nodata=): it is what tells where a file has data on the grid')
    dst = _dest_view(grid.shape, c, name, dtype, layout=layout, out=out, channel_offset=channel_offset) if out is not None else None
    if (dst.kind if dst is not None else (dtype or name)) != name:
        raise ValueError(f'equalize=True writes the files\' kind {name}: a float32 destination is not served')
    xs = [_footprint_x(f, grid) for f in files]
    order = sorted(range(len(files)), key=lambda i: xs[i])       # (stable: ties keep the order of the paths)
    slots = _device_empty((len(files), c) + grid.shape, _torch_dtype(name), 'the slots of the equalized mosaic')
    for s, f in enumerate(files):
        r = read_warped(f, grid, bands, resampling, level=level, layout='chw', out=slots[s], nodata=nodata, decode=decode, reproject=reproject)
    calibration._chain(slots, name, nodata, order)
    _mark('equalize')
    out, dname = _filled(grid.shape, c, name, nodata, layout=layout, out=out, channel_offset=channel_offset, what='the mosaic')
    lay = _chw_or_hwc(layout)
    ld = c if dst is None else dst.ld
    # the identity table, by bytes: bin k holds the value k - bias (a uint16 value as the int16 with its bytes)
    k = torch.arange(calibration.BINS[name], device='cuda', dtype=torch.int32) - calibration.BIAS[name]
    identity = k.to(torch.uint8) if name == 'uint8' else ((k + 32768) % 65536 - 32768).to(torch.int16)
    identity = identity.repeat(c, 1).contiguous()
    for s in (reversed(range(len(files))) if first else range(len(files))):
        calibration._apply(slots[s], name, identity, out, nodata, layout=lay, ld=ld, coff=channel_offset, keep=True)
    _mark('paint')
    return Raster(out, grid.transform, r.crs, nodata=nodata, dtype=dname)


def read_mosaic(paths, grid=None, bands=None, resampling='nearest', level=0, layout='hwc', first=False, nodata=None, dtype=None, out=None,
                channel_offset=0, decode=None, reproject=False, equalize=False):
    """Files of one CRS mosaicked onto one grid: -> `Raster`.  grid: None is `union_grid(paths)`.  The destination is filled with
    nodata, then every file is read onto it with keep=True, in order: a later file lies on top wherever it has valid data
    (gdal.BuildVRT's order); first=True goes through the files in reverse, so the first file wins (rioxarray's merge_arrays).
    nodata: None is the first file's, without one NaN (float32) or 0.  The other arguments as for `read_warped`; with reproject=True the
    files may be in several EPSG codes (the two-UTM-zone case), grid=None is then `union_grid(paths, reproject=True)`.
    equalize=True removes the radiometric seam between the files (utils/calibration.py's equalize_collection): every file is warped into a
    slot of its own (S x C x H x W samples are resident), the slots are histogram-matched west to east -- by the x of each file's
    footprint centre in the grid's CRS, ties in path order; `calibration.equalize_collection` -- and painted in the order `first`
    prescribes.  For uint8, uint16 and int16 files with a nodata value; float32 and int32 files are refused.
    Inside the package the paths may be `_File`s, files that are already parsed (`read_aligned_stack`)."""
    files = _files(paths)
    if not files:
        raise ValueError('read_mosaic needs at least one file')
    if grid is None:
        grid = union_grid([_as_grid(f.levels[0], str(f.path)) for f in files], reproject=reproject)
    for f in files:
        _file_mapping(f, grid, reproject)                      # every refusal before anything is allocated
    name, c, file_nodata = _same_kind(files, bands)
    if nodata is None:
        nodata = file_nodata
    if equalize:
        return _read_mosaic_equalized(files, grid, bands, resampling, level, layout, first, nodata, dtype, out, channel_offset, decode, reproject, name, c)
    out, dname = _filled(grid.shape, c, name if dtype is None else dtype, nodata, layout=layout, out=out, channel_offset=channel_offset, what='the mosaic')
    for f in (reversed(files) if first else files):
        r = read_warped(f, grid, bands, resampling, level=level, layout=layout, out=out, keep=True, nodata=nodata, dtype=dtype,
                        channel_offset=channel_offset, decode=decode, reproject=reproject)
    return Raster(out, grid.transform, r.crs, nodata=nodata, dtype=dname)


def read_aligned_stack(items, grid=None, resolution=None, bands=None, resampling='nearest', level=0, reproject=False, equalize=False):
    """The acquisitions of a time series on ONE grid as a resident stack: -> (stack, transform, crs, nodata), the contract of
    `read_stack` -- stack a (T, C, H, W) CUDA tensor in the files' kind -- for files that need not share a grid: other footprints,
    other resolutions (the 20 m bands beside the 10 m ones), one CRS.  items: per acquisition a path, or a list of paths mosaicked
    into the slot (`read_mosaic`).  grid: None is `union_grid` of every file at `resolution` (None: the finest).  Every file is
    resampled straight into its slot.  With files that already share the grid, nearest gives `read_stack`'s result bit for bit.
    reproject=True: the files may be in several EPSG codes (`read_warped`); the grid built here is `union_grid(..., reproject=True)`.
    equalize=True: the items that are lists of paths are mosaicked with `read_mosaic(equalize=True)`."""
    items = [[it] if isinstance(it, (str, os.PathLike)) else list(it) for it in items]
    flat = _files([p for it in items for p in it])
    if not flat or any(not it for it in items):
        raise ValueError('read_aligned_stack needs at least one file per acquisition')
    if grid is None:
        grid = union_grid([_as_grid(f.levels[0], str(f.path)) for f in flat], resolution=resolution, reproject=reproject)
    elif resolution is not None:
        raise ValueError('resolution describes the grid that is built when none is given')
    for f in flat:
        _file_mapping(f, grid, reproject)
    name, c, nodata = _same_kind(flat, bands)
    stack = _device_empty((len(items), c) + grid.shape, _torch_dtype(name), 'the time stack')
    record = iter(flat)                                        # (the records of the items, in order)
    for t, it in enumerate(items):
        files = [next(record) for _ in it]
        slot = dict(level=level, layout='chw', out=stack[t], nodata=nodata, reproject=reproject)
        if len(files) == 1:
            r = read_warped(files[0], grid, bands, resampling, **slot)
        else:
            r = read_mosaic(files, grid, bands, resampling, equalize=equalize, **slot)
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
def transform_points(xs, ys, src_crs, dst_crs, device=False):
    """Points of `src_crs` in `dst_crs`: -> (xs, ys) of the same shape, float64.  Geographic coordinates are x = longitude, y = latitude
    in degrees.  A point outside a projection's domain (csrc/crs_core.hpp: |lat| > 90, more than 30 degrees off a UTM zone's central
    meridian, beyond the square world of EPSG:3857, not finite) comes back as NaN.  device=False: array-likes in, NumPy arrays out, the
    loop runs on the CPU; device=True: CUDA float64 tensors in and out, one thread per point.  No datum shift between WGS84 and NAD83
    (at most 1-2 m).  ValueError for a code `crs.crs_params` does not know."""
    a, b = crs_struct(src_crs), crs_struct(dst_crs)
    if device:
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


_Extent = namedtuple('_Extent', 'bounds resolution epsg')      # of a source in another CRS: what `union_grid` needs of a Grid


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
    m = _reproject_map(_a_grid(grid), grid.crs if crs is None else crs, transform)
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
    m = _Mapping(src_transform, src_crs, _a_grid(grid), reproject=True)      # (without `what`: the method is refused first, then a code, by the launch)
    return _resample(m, src, resampling, src_nodata=src_nodata, nodata=nodata, dtype=dtype, src_layout=src_layout, layout=layout, out=out,
                     channel_offset=channel_offset, keep=keep, src_origin=src_origin, src_dtype=src_dtype)


def reproject_window(src_transform, src_shape, src_crs, grid, resampling='nearest'):
    """`warp_window` across two coordinate systems: the window (row0, col0, h, w) of a source raster of `src_crs` that `grid` needs, or
    None when the grid misses the raster.  The centres of ALL boundary pixels of the grid are transformed (the map between two
    projections is a homeomorphism: the extremes of u and v over the grid lie on its boundary); the window runs from floor(min) to
    floor(max), widened by the method's margin (0 / 1 / 2) and by one pixel more -- the host's and the device's libm may differ in the
    last bits -- and clipped to the raster.  When some boundary pixel lies outside a projection's domain the extremes are unknown: the
    window is the whole raster; when every one does: None."""
    return _Mapping(src_transform, src_crs, grid, foreign=True).window(src_shape, resampling)


# ----------------------------------------------------------------------------------------------------------------- polygons on a grid
# `rio.clip([aoi], crs)` of utils/pc_tools.py:595-606 (commented out at :384, :439, :493): polygons become a mask or a burned label
# raster on the device (csrc/rasterize.hip), and one mask serves every plane of a raster or a stack.  The rule -- pixel centres,
# all_touched=False, even-odd -- is this library's own (include/satcv.h, "Polygon rasterization"; tests/rasterize_oracle.py).  Host code
# (GeoJSON, the edge table, the window helpers of utils/raster_tools.py:70-331) is in `polygons`.  Out of scope, each a ValueError:
# all_touched=True, lines and points, rotated grids, densifying edges before a change of CRS (only vertices are transformed, as
# rio.clip does).
def _rings_on(rings, grid, geom_crs):
    """`geometry_rings` output with the vertices in the CRS of `grid`: only vertices are transformed"""
    src, dst = _epsg_of(geom_crs), grid.epsg
    if src is None or dst is None or src == dst:
        return rings
    out = []
    for g in rings:
        out.append([])
        for r in g:
            xs, ys = transform_points(r[:, 0], r[:, 1], f'EPSG:{src}', f'EPSG:{dst}')
            out[-1].append(np.stack([xs, ys], axis=1))
    return out


def geometry_bounds(geoms, geom_crs=None, crs=None):
    """(left, bottom, right, top) of the geometries; when `geom_crs` and `crs` name different codes, `transform_bounds` of that box in `crs`"""
    b = rings_bounds(geometry_rings(geoms))
    src, dst = _epsg_of(geom_crs), _epsg_of(crs)
    if src is None or dst is None or src == dst:
        return b
    return transform_bounds(f'EPSG:{src}', f'EPSG:{dst}', *b)


def aoi_grid(geoms, resolution, crs, geom_crs='EPSG:4326'):
    """The north-up grid of `crs` at `resolution` that holds the geometries (given in `geom_crs`): `union_grid` of their bounds, snapped
    outward to multiples of the resolution."""
    return union_grid([], resolution=resolution, bounds=geometry_bounds(geoms, geom_crs=geom_crs, crs=crs), crs=crs)


def _burn(geoms_px, shape, mode, invert, values, fill, dst, keep, device):
    """one satcv_rasterize call: geometries in pixel coordinates into the `_View` dst (device) or the host array view (ptr) it describes"""
    table, row_start = edge_table(geoms_px, shape)
    vals = None if mode == 0 else np.ascontiguousarray(values, DTYPES[dst.kind][0])
    d = RasterizeDesc(edges=table.ctypes.data if len(table) else None, n_items=len(table), row_start=row_start.ctypes.data, h=shape[0], w_=shape[1], n_geoms=len(geoms_px),
                      mode=mode, invert=int(bool(invert)), values=vals.ctypes.data if vals is not None and vals.size else None, fill=float(fill), dst=dst.ptr,
                      dst_kind=DTYPES[dst.kind][1], dst_layout=dst.layout, dst_ld=dst.ld, dst_coff=dst.coff, keep=int(bool(keep)), on_device=int(bool(device)))
    ws = None
    if device:
        need = C.c_int64()
        check(lib.satcv_rasterize_workspace(len(table), shape[0], int(row_start[-1]), len(geoms_px), C.byref(need)))
        ws = _device_empty((max(int(need.value), 16),), torch.uint8, 'the rasterization workspace')
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    ops.rasterize(d)
    return ws


def _shapes(shapes, values):
    """-> ([geometry (list of rings)], [value per geometry]) of `rasterize`'s shapes / values"""
    if isinstance(shapes, dict) or hasattr(shapes, '__geo_interface__'):
        shapes = [shapes]
    shapes = list(shapes)
    if values is not None:
        values = list(np.atleast_1d(values))
        if len(values) != len(shapes):
            raise ValueError(f'{len(values)} values for {len(shapes)} shapes')
    geoms, vals = [], []
    for k, s in enumerate(shapes):
        v = 1 if values is None else values[k]
        if isinstance(s, (tuple, list)) and len(s) == 2 and np.ndim(s[1]) == 0 and not isinstance(s[1], (dict, str)) and not hasattr(s[1], '__geo_interface__'):
            if values is not None:
                raise ValueError('values are given twice: as (geometry, value) pairs and as values=')
            s, v = s
        g = geometry_rings(s)
        geoms += g
        vals += [v] * len(g)
    return geoms, vals


def rasterize(shapes, grid, values=None, fill=0, dtype='uint8', geom_crs=None, out=None, channel_offset=0, layout='hwc', keep=False, device=True,
              all_touched=False):
    """Polygons burned into a raster on `grid`: a pixel whose centre lies inside a geometry (even-odd over its rings; the rule of
    include/satcv.h, this library's own) takes that geometry's value -- of the LAST one in list order that covers it -- every other
    pixel `fill`, or with keep=True what `out` held (without `out` there is nothing to keep: `fill`).  shapes: geometries (`geometry_rings` says which) or (geometry, value) pairs;
    values: one per shape instead of pairs; neither: 1.  geom_crs: the CRS of the vertices when it is not the grid's -- only vertices are
    transformed (`transform_points`), edges are not densified.  dtype: 'uint8', 'uint16', 'int16', 'int32' or 'float32'.
    device=True: -> a CUDA tensor (H, W), or `out` ((H, W), (H, W, ld) for layout 'hwc', (ld, H, W) for 'chw'; channel channel_offset is
    written, no other).  device=False: the same rule on the CPU -> a NumPy array (H, W); `out` then is a C-contiguous array of the same forms.
    ValueError: all_touched=True, lines and points, a non-finite vertex, an unknown dtype or layout; a row with more than 4096 crossings is
    refused by the library (SatcvError) before anything is launched."""
    if all_touched:
        raise ValueError('all_touched=True is not implemented: the rule is the pixel-centre rule')
    grid = _a_grid(grid)
    if dtype not in DTYPES:
        raise ValueError(f'dtype {dtype!r}: one of {sorted(DTYPES)}')
    geoms, vals = _shapes(shapes, values)
    px = to_pixels(_rings_on(geoms, grid, geom_crs), grid.transform)
    keep = bool(keep) and out is not None                     # (a new raster holds nothing to keep: every uncovered pixel is `fill`)
    if device:
        dst = _dest_view(grid.shape, 1, dtype, None, layout, out=out, channel_offset=channel_offset, flat=True)
        if dst.kind != dtype:
            raise ValueError(f'out is {dst.owner.dtype}, the result {dtype}')
    else:
        dst = _host_dest(grid.shape, dtype, layout, out, channel_offset)
    _burn(px, grid.shape, 1, False, vals, fill, dst, keep, device)
    return dst.owner


def _host_dest(shape, dtype, layout, out, channel_offset):
    nt = np.dtype(DTYPES[dtype][0])
    lay = _chw_or_hwc(layout)
    if out is None:
        out = np.empty(shape, nt)
    if not (isinstance(out, np.ndarray) and out.flags.c_contiguous and out.dtype == nt and out.ndim in (2, 3)):
        raise ValueError(f'out must be a C-contiguous NumPy array of {nt}, (H, W), (H, W, ld) or (ld, H, W)')
    hw = out.shape if out.ndim == 2 else (out.shape[:2] if lay == 0 else out.shape[1:])
    ld = 1 if out.ndim == 2 else int(out.shape[2] if lay == 0 else out.shape[0])
    if tuple(hw) != tuple(shape):
        raise ValueError(f'out is {hw[0]} x {hw[1]}, the grid {shape[0]} x {shape[1]}')
    if not 0 <= int(channel_offset) < ld:
        raise ValueError(f'channel {channel_offset} does not fit the {ld} of out')
    return _View(owner=out, ptr=out.ctypes.data, kind=dtype, h=shape[0], w=shape[1], c=1, ld=ld, coff=int(channel_offset), layout=lay, flat=out.ndim == 2)


def _mask_of(rings, grid, invert=False, device=True):
    px = to_pixels(rings, grid.transform)
    if device:
        dst = _dest_view(grid.shape, 1, 'uint8', None, 'hwc', flat=True)
    else:
        dst = _host_dest(grid.shape, 'uint8', 'hwc', None, 0)
    _burn(px, grid.shape, 0, invert, None, 0, dst, False, device)
    return dst.owner


def geometry_mask(geoms, grid, invert=False, geom_crs=None, device=True, all_touched=False):
    """The geometries as a uint8 (H, W) mask on `grid`, on the device: 1 INSIDE a geometry and 0 outside (their union) -- the opposite of
    rasterio's `geometry_mask`, whose default is True outside; invert=True gives 0 inside and 1 outside.  This is the form
    `calibration.*(region=)` and `clip` take.  device=False: a NumPy array from the host loop.  Rule and refusals: `rasterize`."""
    if all_touched:
        raise ValueError('all_touched=True is not implemented: the rule is the pixel-centre rule')
    grid = _a_grid(grid)
    return _mask_of(_rings_on(geometry_rings(geoms), grid, geom_crs), grid, invert, device)


def mask_apply(arr, mask, nodata=None, invert=False, layout='hwc', inplace=False, src_dtype=None):
    """Samples of `arr` where `mask` is 0 (invert=True: is not 0) become nodata -- None: NaN for float32, 0 for integers; every other
    sample is kept.  arr: a contiguous CUDA tensor, (H, W) or (H, W, C) for layout 'hwc', (C, H, W) or a (T, C, H, W) stack for 'chw';
    mask: a uint8 or bool (H, W) CUDA tensor.  inplace=True writes into `arr` (only the samples outside are touched) and returns it;
    otherwise a new tensor.  One streaming launch (satcv_raster_mask_apply)."""
    if not (isinstance(arr, torch.Tensor) and arr.is_cuda and arr.is_contiguous() and arr.dtype in _TENSOR_KINDS and arr.dtype != torch.float64):
        raise ValueError('mask_apply takes a contiguous CUDA tensor of uint8, uint16, int16, int32 or float32')
    lay = _chw_or_hwc(layout)
    if lay == 0:
        if arr.dim() not in (2, 3):
            raise ValueError(f"an 'hwc' raster is (H, W) or (H, W, C), got shape {tuple(arr.shape)}")
        h, w, ld = int(arr.shape[0]), int(arr.shape[1]), int(arr.shape[2]) if arr.dim() == 3 else 1
    else:
        if arr.dim() not in (2, 3, 4):
            raise ValueError(f"a 'chw' raster is (H, W), (C, H, W) or a (T, C, H, W) stack, got shape {tuple(arr.shape)}")
        h, w = int(arr.shape[-2]), int(arr.shape[-1])
        ld = int(np.prod(arr.shape[:-2], dtype=np.int64)) if arr.dim() > 2 else 1
    if 0 in arr.shape:
        raise ValueError(f'an empty raster: shape {tuple(arr.shape)}')
    if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    if not (isinstance(mask, torch.Tensor) and mask.is_cuda and mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w)):
        raise ValueError(f'mask is a uint8 or bool (H, W) = {(h, w)} CUDA tensor')
    kind = _TENSOR_KINDS[arr.dtype] if src_dtype is None else src_dtype
    mask = mask.contiguous()
    dst = arr if inplace else _device_empty(tuple(arr.shape), arr.dtype, 'the masked raster')
    ops.raster_mask_apply(mask, arr, dst, DTYPES[kind][1], lay, h, w, ld, 0, ld, nodata, invert)
    return dst


def clip(arr, grid, geoms, geom_crs=None, nodata=None, crop=True, layout='hwc', inplace=False):
    """`rio.clip([aoi], crs)` on the device: -> (raster, Grid).  Samples of `arr` (on `grid`; forms as `mask_apply`) whose pixel centre
    lies outside every geometry become nodata (None: NaN for float32, 0 for integers): `geometry_mask`, then `mask_apply`.  crop=True
    returns the view of the geometries' pixel bounding box (clipped to the grid) and that window's Grid; ValueError when the
    geometries miss the grid.  inplace=True masks `arr` itself."""
    grid = _a_grid(grid)
    rings = _rings_on(geometry_rings(geoms), grid, geom_crs)
    mask = _mask_of(rings, grid)
    out = mask_apply(arr, mask, nodata=nodata, layout=layout, inplace=inplace)
    if not crop:
        return out, grid
    H, W = grid.shape
    px = np.concatenate([r for g in to_pixels(rings, grid.transform) for r in g])
    if not np.isfinite(px).all():
        raise ValueError('a vertex lies outside the domain of the grid\'s projection')
    c0, c1 = int(max(np.floor(px[:, 0].min()), 0)), int(min(np.ceil(px[:, 0].max()), W))
    r0, r1 = int(max(np.floor(px[:, 1].min()), 0)), int(min(np.ceil(px[:, 1].max()), H))
    if c0 >= c1 or r0 >= r1:
        raise ValueError('the geometries do not intersect the grid')
    view = out[r0:r1, c0:c1] if _chw_or_hwc(layout) == 0 else out[..., r0:r1, c0:c1]
    return view, Grid(_window_transform(grid.transform, grid.shape, grid.shape, r0, c0), (r1 - r0, c1 - c0), grid.crs)
