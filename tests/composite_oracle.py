"""NumPy float64 restatement of the compute half of `run_local` (utils/pc_tools.py:620-668) for the composite tests:

    np.where(x > 0, x, nan)                                   :376   (stackstac nodata 0 -> NaN, as `x > 0`)
    np.where(off > 0, np.clip(x, off, None) - off, x)         :284-326  harmonize_to_old
    np.nanmedian(axis=0)                                      :642-643  DataArray.median(dim='time'), skipna
    (m - nanmean) / (nanstd + 1e-6) over bands                :90-107   normalize_dataArray

xarray cannot be imported here, so the reference's own bodies are not executed; what xarray dispatches to (bottleneck / NumPy
nan-reductions) is pinned by tests/golden/composite_reference.npz (make_composite_fixtures.py)."""
import warnings

import numpy as np


def composite(stack, offsets=None):
    """stack (T, C, H, W) of any real dtype, offsets (T,) or None -> (median (H, W, C), norm (H, W, C)), float64.

    A float32 stack is rounded to float32 right after the subtraction of the offset (the kernel holds samples as float32: the
    documented deviation, nil for integer-valued imagery); everything else is float64."""
    x = np.asarray(stack).astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        x = np.where(x > 0, x, np.nan)
        if offsets is not None:
            off = np.asarray(offsets, np.float64).reshape(-1, 1, 1, 1)
            x = np.where(off > 0, np.clip(x, off, None) - off, x)
            if np.asarray(stack).dtype == np.float32:
                x = x.astype(np.float32).astype(np.float64)
        med = np.nanmedian(x, axis=0)                         # (C, H, W)
        mean = np.nanmean(med, axis=0)
        sd = np.nanstd(med, axis=0)
        norm = (med - mean) / (sd + 0.000001)
    return np.ascontiguousarray(med.transpose(1, 2, 0)), np.ascontiguousarray(norm.transpose(1, 2, 0))


def norm_bound(med, c):
    """Absolute part of the `norm` tolerance, per pixel (H, W, 1): 8 c 2^-53 max|median| / (sd + 1e-6) -- the double-precision rounding of
    `median - mean` amplified by the division; it only matters where sd ~ 0."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        sd = np.nanstd(med, axis=2, keepdims=True)
        big = np.nanmax(np.abs(med), axis=2, keepdims=True)
    return np.nan_to_num(8.0 * c * 2.0 ** -53 * big / (sd + 1e-6), nan=0.0)


def ulp_distance(a, b):
    """distance in float32 units in the last place between two float32 arrays (finite values; NaN positions must be masked by the caller)"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))
