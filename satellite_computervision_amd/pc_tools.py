"""Compute half of the reference's utils/pc_tools.py on arrays instead of xarray objects: what `run_local` (:620-668) does between
"the acquisitions are in memory" and the returned change map.

    stack (time, band, y, x) -> nodata 0 -> NaN (:376) -> harmonize_to_old (:284-326) -> median over time (:642-643)
      -> normalize_dataArray over bands (:90-107) -> [before bands, after bands] (:650) -> chips -> model -> stitched map

The first four arrows are ONE kernel (satcv_median_composite, csrc/composite.hip) on a stack that is uploaded once; its output is the
(H, W, C) float32 scene the device-resident prediction loop of prediction_tools reads in place.  Acquisition (STAC search, rioxarray)
stays with the caller; files on differing grids are aligned by `predict_change_files` (raster_tools.read_aligned_stack, what
stackstac.stack(resolution=) does for the reference; reproject=True for several coordinate systems), and its aoi= / `predict_change`'s
region= clip to a polygon, the reference's rio.clip([aoi], crs) (:595-606; raster_tools.geometry_mask, mask_apply).

The composites the reference's models were trained on were masked per acquisition first (utils/ee_tools.py: basicQA :159, maskTOA
:288, maskSR :270, mask :257).  `median_composite(clear=...)` / `predict_change(quality=...)` take those masks from `ee_tools` as bit-planes
on the device (satcv_median_composite_masked): a sample is valid iff it is > 0 and its clear bit is set.
"""
from datetime import datetime

import numpy as np


def harmonize_offsets(times, cutoff=datetime(2022, 1, 25), offset=1000):
    """Per-acquisition offsets of `harmonize_to_old` (utils/pc_tools.py:284-326) as a (t,) float32 array: `offset` for an acquisition
    at or after `cutoff` (the "new" processing baseline, what `data.sel(time=slice(cutoff, None))` selects), 0 before it.

    times: `datetime.datetime` / `numpy.datetime64` values (a list or an array).  The reference harmonises the bands of its list
    B01 ... B12, B8A -- every Sentinel-2 reflectance band -- so here the offset of an acquisition applies to all bands of the stack."""
    t = np.asarray(list(times), dtype='datetime64[us]')
    return np.where(t >= np.datetime64(cutoff, 'us'), np.float32(offset), np.float32(0)).astype(np.float32)


def trim_array(arr, size):
    """`trim_dataArray` (utils/pc_tools.py:109-129) on the last two axes (y, x): drop the remainder so both are divisible by `size`."""
    sl = [slice(None)] * (arr.ndim - 2)
    for n in arr.shape[-2:]:
        remainder = n % size
        sl.append(slice(-remainder) if remainder else slice(None))
    return arr[tuple(sl)]


def _stack_to_device(stack):
    """-> (CUDA tensor (T, C, H, W) contiguous, element kind of satcv_composite_desc)"""
    import torch
    from .prediction_tools import _to_device
    if isinstance(stack, torch.Tensor):
        if not stack.is_cuda:
            stack = stack.numpy()
        else:
            if stack.dtype == torch.float64:
                stack = stack.to(torch.float32)
            kinds = {torch.int16: 3, torch.float32: 2}
            if hasattr(torch, 'uint16'):
                kinds[torch.uint16] = 1
            if stack.dtype not in kinds:
                raise ValueError(f'a stack is uint16, int16, float32 or float64, got {stack.dtype}')
            return stack.contiguous(), kinds[stack.dtype]
    stack = np.asarray(stack)
    if stack.dtype == np.float64:
        stack = stack.astype(np.float32)      # documented deviation: lossless for integer-valued imagery
    kinds = {np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3}
    if stack.dtype not in kinds:
        raise ValueError(f'a stack is uint16, int16, float32 or float64, got {stack.dtype}')
    return _to_device(stack, 'the time stack'), kinds[stack.dtype]


def _band_selection(bands, band_names, nplanes):
    """`bands` (indices, or names together with `band_names`) -> plane indices; None: every plane in order"""
    if bands is None:
        return list(range(nplanes))
    bands = list(bands)
    if not bands:
        raise ValueError('an empty band selection')
    if all(isinstance(b, (int, np.integer)) for b in bands):
        idx = [int(b) for b in bands]
    else:
        if band_names is None:
            raise ValueError('bands given by name need band_names, the names of the planes of the stack')
        from .ee_tools import canonical_band
        names = [canonical_band(b) for b in band_names]
        if len(names) != nplanes:
            raise ValueError(f'{nplanes} planes need {nplanes} band_names, got {len(names)}')
        missing = [b for b in bands if canonical_band(b) not in names]
        if missing:
            raise ValueError(f'bands {missing} are not among band_names {list(band_names)}')
        idx = [names.index(canonical_band(b)) for b in bands]
    if any(i < 0 or i >= nplanes for i in idx):
        raise ValueError(f'band selection {idx} outside the {nplanes} planes of the stack')
    if len(idx) > 16:
        raise ValueError(f'{len(idx)} bands: the composite kernel takes at most 16')
    return idx


def _offsets_to_device(T, times, offsets):
    from .prediction_tools import _to_device
    if times is not None and offsets is not None:
        raise ValueError('give times or offsets, not both')
    if times is not None:
        offsets = harmonize_offsets(times)
    if offsets is None:
        return None
    offsets = np.ascontiguousarray(offsets, np.float32)
    if offsets.shape != (T,):
        raise ValueError(f'{T} acquisitions need {T} offsets / times, got shape {offsets.shape}')
    return _to_device(offsets, 'the offset table') if offsets.any() else None


def _composite(src, kind, off_dev, fill, out, channel_offset, clear=None, idx=None):
    """the launch of `median_composite` on a resident stack (src, kind); clear: a ClearMask or None, idx: plane indices or None.
    With neither it is satcv_median_composite, otherwise satcv_median_composite_masked."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import CompositeDesc, CompositeMaskedDesc, check, lib
    from .prediction_tools import _device_empty
    T, cs, H, W = (int(v) for v in src.shape)
    nb = cs if idx is None else len(idx)
    median = _device_empty((H, W, nb), torch.float32, 'the median composite')
    if out is None:
        if channel_offset:
            raise ValueError('channel_offset needs out')
        out = _device_empty((H, W, nb), torch.float32, 'the normalised composite')
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 3 and out.is_contiguous()
              and tuple(out.shape[:2]) == (H, W)):
        raise ValueError(f'out must be a contiguous float32 CUDA tensor ({H}, {W}, ld)')
    d = CompositeDesc(src=src.data_ptr(), src_kind=kind, t=T, c=nb, h=H, w_=W, offsets=off_dev.data_ptr() if off_dev is not None else None,
                      median=median.data_ptr(), ld_med=nb, coff_med=0, norm=out.data_ptr(), ld_norm=out.shape[2], coff_norm=int(channel_offset),
                      use_fill=int(fill is not None), fill=float(fill or 0.0))
    if clear is None and idx is None:
        check(lib.satcv_median_composite(C.byref(d), ops.stream_ptr()))
    else:
        if clear is not None and clear.shape != (T, H, W):
            raise ValueError(f'the clear mask is for a stack {clear.shape}, the stack is {(T, H, W)}')
        table = list(idx if idx is not None else range(cs)) + [0] * 16
        md = CompositeMaskedDesc(base=d, clear=clear.words.data_ptr() if clear is not None else None, cs=cs, band_idx=(C.c_int32 * 16)(*table[:16]))
        check(lib.satcv_median_composite_masked(C.byref(md), ops.stream_ptr()))
    # `src`, `off_dev` and the mask may be released on return: the caching allocator hands their memory to later work of this same stream only
    return median, out[..., channel_offset:channel_offset + nb]


def median_composite(stack, times=None, offsets=None, fill=None, out=None, channel_offset=0, clear=None, bands=None, band_names=None):
    """Median composite of a time stack and its per-pixel normalisation over bands, on the device: `(median, norm)`, float32 CUDA
    tensors (H, W, C).

    stack: (T, C, H, W), the layout stackstac delivers -- a host array of uint16 / int16 / float32 / float64, or a CUDA tensor of
    those kinds.  It is uploaded once; float64 is converted to float32 first (lossless for integer-valued imagery; the reference
    computes in float64).  Values <= 0 and NaN are nodata (:376).
    times: the acquisition times -> `harmonize_offsets(times)`; or offsets: (T,) values given directly (0 = none).  Neither: no
    harmonisation.  16-bit stacks take offsets rounded to integers.
    fill: replaces NaN in `norm` (only there); None = the reference, NaN propagates.
    out, channel_offset: write `norm` into channels [channel_offset, channel_offset + C) of an existing contiguous float32 CUDA tensor
    (H, W, ld) -- with ld = 2 C the before / after composites of `run_local` land in one scene without a concatenation pass (:650);
    the returned `norm` is that slice.
    clear: an `ee_tools.ClearMask` of the stack (basicQA / maskTOA / maskSR / mask): a sample takes part iff it is > 0 and clear.
    bands: the planes that make the composite, by index, or by name together with band_names (the names of the stack's planes) --
    a 14-plane stack with its QA60 plane yields a 4-band composite without a copy; C above is then len(bands).
    With neither `clear` nor `bands` the launch is the unmasked kernel's, unchanged.
    Nothing here synchronises with the host.  T <= 256, C <= 16; a stack that does not fit in device memory raises MemoryError."""
    from ._lib import COMPOSITE_MAX_T
    if getattr(stack, 'ndim', 0) != 4:
        raise ValueError(f'expected a (T, C, H, W) stack, got shape {tuple(getattr(stack, "shape", ()))}')
    T, nb, H, W = (int(v) for v in stack.shape)
    if T > COMPOSITE_MAX_T:
        raise ValueError(f'{T} acquisitions: the composite kernel takes at most {COMPOSITE_MAX_T}')
    idx = _band_selection(bands, band_names, nb) if bands is not None else None
    if clear is not None and not hasattr(clear, 'words'):
        raise ValueError('clear is an ee_tools.ClearMask')
    off_dev = _offsets_to_device(T, times, offsets)
    src, kind = _stack_to_device(stack)
    return _composite(src, kind, off_dev, fill, out, channel_offset, clear, idx)


def predict_change(before, after, m, before_times=None, after_times=None, buff=128, kernel=256, batch_size=16, channel=0,
                   cover='reference', fill=None, quality=None, band_names=None, bands=None, out_file=None, transform=None, crs=None,
                   cog_options=None, region=None):
    """`run_local` (utils/pc_tools.py:620-668) from the two time stacks on: `(output, bef_median, aft_median)` -- the change map
    (H, W) float32 and the two median composites (H, W, C) float32 as host arrays (the reference's return without the geotransform).

    before, after: (T, C, H, W) stacks of equal C, H, W (see `median_composite`); before_times / after_times: their acquisition times
    for the harmonisation, or None.  A single-input model gets the reference's one scene [before bands, after bands] (:650); a
    two-input model (make_siamese_unet) gets the pair in its own input order (a = after / T2, b = before / T1, as `predict_chips`
    documents).  buff, kernel, batch_size, channel, cover: as `prediction_tools.predict_scene`.  fill: see `median_composite`; with
    None a pixel without a valid sample sends NaN into every chip that contains it, as in the reference.
    quality: masks both stacks before their composites, as the reference's training composites were (utils/ee_tools.py) -- 'toa'
    (maskTOA :288), 'sr' (maskSR :270), 'mask' (mask :257), any rule set `ee_tools.rule_set` takes (these need band_names, the names of
    the planes), or a pair of `ee_tools.ClearMask`s (before, after).  bands: the planes the model sees, see `median_composite`; the
    returned medians are the masked composites of those bands.
    out_file: also write the change map as a Cloud-Optimized GeoTIFF (`raster_tools.write_cog`, float32 unless cog_options says
    otherwise) straight from the device map, where the reference hands its array to numpy_to_raster; needs transform (a, b, c, d, e, f)
    and crs ('EPSG:n' or an int).  cog_options: a dict of further `write_cog` arguments (dtype, scale, nodata, compress, ...).  The
    return value is unchanged.
    region: a uint8 or bool (H, W) mask, 1 inside (`raster_tools.geometry_mask` of an area of interest; a host array goes up once):
    the `rio.clip([aoi], crs)` of :595-606.  Both stacks are clipped before their composites -- a sample outside becomes 0 (NaN for
    float32), nodata by the rule above, so it drops out of the median -- and the change map is NaN outside the region before it is
    returned and written.  The caller's stacks are not modified.  None: the launches and results are exactly those without it.
    The composites stay on the device from the composite kernel to the stitch; the three returned arrays are the only copies back."""
    import torch
    from . import prediction_tools as pt
    from .prediction_tools import _device_empty
    if out_file is not None:
        from . import raster_tools as rt
        if transform is None or crs is None:
            raise ValueError('out_file needs transform and crs')
        rt.parse_crs(crs)
        if len(tuple(transform)) != 6:
            raise ValueError(f'transform is six numbers (a, b, c, d, e, f), got {len(tuple(transform))}')
    elif transform is not None or crs is not None or cog_options:
        raise ValueError('transform, crs and cog_options describe out_file, which is not given')
    if getattr(before, 'ndim', 0) != 4 or getattr(after, 'ndim', 0) != 4 or tuple(before.shape[1:]) != tuple(after.shape[1:]):
        raise ValueError(f'before and after must be (T, C, H, W) stacks of equal C, H, W, got {tuple(before.shape)} and {tuple(after.shape)}')
    cs, H, W = (int(v) for v in before.shape[1:])
    idx = _band_selection(bands, band_names, cs) if bands is not None else None
    nb = cs if idx is None else len(idx)
    masks = (None, None)
    rules = table = None
    if quality is not None:
        from . import ee_tools as ee
        if isinstance(quality, (tuple, list)) and len(quality) == 2 and all(hasattr(q, 'words') for q in quality):
            masks = tuple(quality)
        else:
            rules = ee.rule_set(quality)
            if band_names is None:
                raise ValueError('quality rules need band_names, the names of the planes of the stacks')
            if len(band_names) != cs:
                raise ValueError(f'{cs} planes need {cs} band_names, got {len(band_names)}')
            table = ee.band_table(band_names)
            ee._require(table, rules, band_names)
    if region is not None:
        from . import raster_tools as rt
        from .calibration import _mask
        region = _mask(region, (H, W))
    two_inputs = len(getattr(m, 'inputs', ())) > 1
    scene = None if two_inputs else _device_empty((H, W, 2 * nb), torch.float32, 'the two-date scene')
    medians, norms = [], []
    for k, (stack, times, clear) in enumerate(((before, before_times, masks[0]), (after, after_times, masks[1]))):
        off_dev = _offsets_to_device(int(stack.shape[0]), times, None)
        src, kind = _stack_to_device(stack)                  # uploaded once: the mask kernel and the composite read the same copy
        if region is not None:                               # (in place on the copy made here; a resident stack of the caller's is left as it is)
            src = rt.mask_apply(src, region, layout='chw', inplace=src is not stack)
        if rules is not None:
            clear = ee._quality(src, kind, table, rules, off_dev, clear=True)[0]
        median, norm = _composite(src, kind, off_dev, fill, scene, 0 if two_inputs else k * nb, clear, idx)
        medians.append(median)
        norms.append(norm)
        del src, clear                                       # one stack resident at a time, as before
    bef_median, aft_median = medians
    if two_inputs:
        scene = (norms[1], norms[0])
    if out_file is None and region is None:
        output = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=batch_size, channel=channel, cover=cover)
    else:
        dev_map = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=batch_size, channel=channel, cover=cover, device=True)
        if region is not None:
            rt.mask_apply(dev_map, region, inplace=True)
        if out_file is not None:
            rt.write_cog(dev_map, out_file, transform, crs, **dict(cog_options or {}))
        output = dev_map.cpu().numpy()
    return output, bef_median.cpu().numpy(), aft_median.cpu().numpy()


def predict_change_files(before_items, after_items, m, grid=None, resolution=None, out_file=None, file_bands=None, resampling='nearest',
                         reproject=False, aoi=None, aoi_crs='EPSG:4326', **predict_change_kwargs):
    """`predict_change` from files that need not share a pixel grid: both periods are read as aligned stacks on ONE grid
    (`raster_tools.read_aligned_stack` -- what the reference gets from stackstac.stack(epsg=, resolution=)) and handed to
    `predict_change` with that grid's georeference; returns what `predict_change` returns.

    before_items, after_items: per acquisition a path or a list of paths mosaicked into one acquisition; one CRS throughout.  grid: the
    common `raster_tools.Grid`; None: `union_grid` of every file of both periods at `resolution` (None: the finest).  file_bands: the
    bands read from every file (None: all); resampling: as for `raster_tools.warp`.  out_file: the change map as a Cloud-Optimized
    GeoTIFF with the grid's transform and CRS.  predict_change_kwargs: every other argument of `predict_change` (times, kernel, buff,
    quality, bands, fill, cog_options, ...); transform and crs come from the grid.
    reproject=True: the files may be in several EPSG codes (a series that straddles a UTM zone boundary): they are reprojected onto the
    grid (`raster_tools.read_warped(reproject=True)`); the grid built here is in the code of the first file.
    aoi: an area of interest, a GeoJSON-like polygon in aoi_crs (`raster_tools.geometry_rings` says which forms): the `aoi` of `run_local`
    and its `rio.clip([aoi], crs)` (:595-606).  With no `grid` the grid is `raster_tools.aoi_grid` of the polygon in the files' CRS, at
    `resolution` or the files' finest; the polygon's mask on the grid is `predict_change`'s region: both stacks are clipped before the
    composites and the change map is NaN outside.  None: everything is as without it."""
    import os
    from . import raster_tools as rt
    for k in ('transform', 'crs', 'region'):
        if k in predict_change_kwargs:
            raise ValueError(f'{k} comes from the common grid: it is not an argument of predict_change_files')
    if grid is None:
        flat = [p for it in list(before_items) + list(after_items) for p in ([it] if isinstance(it, (str, os.PathLike)) else it)]
        grid = rt.union_grid(flat, resolution=resolution, reproject=reproject)
        if aoi is not None:
            if grid.crs is None:
                raise ValueError('the files carry no EPSG code: an aoi cannot be placed on them')
            grid = rt.aoi_grid(aoi, grid.resolution, grid.crs, geom_crs=aoi_crs)
    elif resolution is not None:
        raise ValueError('resolution describes the grid that is built when none is given')
    if aoi is not None:
        predict_change_kwargs['region'] = rt.geometry_mask(aoi, grid, geom_crs=aoi_crs)
    before = rt.read_aligned_stack(before_items, grid, bands=file_bands, resampling=resampling, reproject=reproject)
    after = rt.read_aligned_stack(after_items, grid, bands=file_bands, resampling=resampling, reproject=reproject)
    if out_file is not None:
        if grid.crs is None and before[2] is None:
            raise ValueError('the files carry no EPSG code: out_file cannot be georeferenced')
        predict_change_kwargs.update(out_file=out_file, transform=grid.transform, crs=grid.crs or before[2])
    return predict_change(before[0], after[0], m, **predict_change_kwargs)
