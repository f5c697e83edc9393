"""Compute half of the reference's utils/pc_tools.py on arrays instead of xarray objects: what `run_local` (:620-668) does between
"the acquisitions are in memory" and the returned change map.

    stack (time, band, y, x) -> nodata 0 -> NaN (:376) -> harmonize_to_old (:284-326) -> median over time (:642-643)
      -> normalize_dataArray over bands (:90-107) -> [before bands, after bands] (:650) -> chips -> model -> stitched map

The first four arrows are ONE kernel (satcv_median_composite, csrc/composite.hip) on a stack that is uploaded once; its output is the
(H, W, C) float32 scene the device-resident prediction loop of prediction_tools reads in place.  Acquisition (STAC search, stackstac,
rioxarray), reprojection and clipping stay with the caller.
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


def median_composite(stack, times=None, offsets=None, fill=None, out=None, channel_offset=0):
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
    Nothing here synchronises with the host.  T <= 256, C <= 16; a stack that does not fit in device memory raises MemoryError."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import COMPOSITE_MAX_T, CompositeDesc, check, lib
    from .prediction_tools import _device_empty, _to_device
    if getattr(stack, 'ndim', 0) != 4:
        raise ValueError(f'expected a (T, C, H, W) stack, got shape {tuple(getattr(stack, "shape", ()))}')
    T, nb, H, W = (int(v) for v in stack.shape)
    if T > COMPOSITE_MAX_T:
        raise ValueError(f'{T} acquisitions: the composite kernel takes at most {COMPOSITE_MAX_T}')
    if times is not None and offsets is not None:
        raise ValueError('give times or offsets, not both')
    if times is not None:
        offsets = harmonize_offsets(times)
    off_dev = None
    if offsets is not None:
        offsets = np.ascontiguousarray(offsets, np.float32)
        if offsets.shape != (T,):
            raise ValueError(f'{T} acquisitions need {T} offsets / times, got shape {offsets.shape}')
        if offsets.any():
            off_dev = _to_device(offsets, 'the offset table')
    src, kind = _stack_to_device(stack)
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
    check(lib.satcv_median_composite(C.byref(d), ops.stream_ptr()))
    # `src` and `off_dev` may be released on return: the caching allocator hands their memory to later work of this same stream only
    return median, out[..., channel_offset:channel_offset + nb]


def predict_change(before, after, m, before_times=None, after_times=None, buff=128, kernel=256, batch_size=16, channel=0,
                   cover='reference', fill=None):
    """`run_local` (utils/pc_tools.py:620-668) from the two time stacks on: `(output, bef_median, aft_median)` -- the change map
    (H, W) float32 and the two median composites (H, W, C) float32 as host arrays (the reference's return without the geotransform).

    before, after: (T, C, H, W) stacks of equal C, H, W (see `median_composite`); before_times / after_times: their acquisition times
    for the harmonisation, or None.  A single-input model gets the reference's one scene [before bands, after bands] (:650); a
    two-input model (make_siamese_unet) gets the pair in its own input order (a = after / T2, b = before / T1, as `predict_chips`
    documents).  buff, kernel, batch_size, channel, cover: as `prediction_tools.predict_scene`.  fill: see `median_composite`; with
    None a pixel without a valid sample sends NaN into every chip that contains it, as in the reference.
    The composites stay on the device from the composite kernel to the stitch; the three returned arrays are the only copies back."""
    import torch
    from . import prediction_tools as pt
    from .prediction_tools import _device_empty
    if getattr(before, 'ndim', 0) != 4 or getattr(after, 'ndim', 0) != 4 or tuple(before.shape[1:]) != tuple(after.shape[1:]):
        raise ValueError(f'before and after must be (T, C, H, W) stacks of equal C, H, W, got {tuple(before.shape)} and {tuple(after.shape)}')
    nb, H, W = (int(v) for v in before.shape[1:])
    if len(getattr(m, 'inputs', ())) > 1:
        bef_median, bef_norm = median_composite(before, times=before_times, fill=fill)
        aft_median, aft_norm = median_composite(after, times=after_times, fill=fill)
        scene = (aft_norm, bef_norm)
    else:
        scene = _device_empty((H, W, 2 * nb), torch.float32, 'the two-date scene')
        bef_median, _ = median_composite(before, times=before_times, fill=fill, out=scene, channel_offset=0)
        aft_median, _ = median_composite(after, times=after_times, fill=fill, out=scene, channel_offset=nb)
    output = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=batch_size, channel=channel, cover=cover)
    return output, bef_median.cpu().numpy(), aft_median.cpu().numpy()
