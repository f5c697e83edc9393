"""Pin what xarray dispatches `DataArray.median / mean / std(skipna=True)` to, for tests/composite_oracle.py.

xarray itself cannot be imported in the build container, but its nan-reductions go to bottleneck when that is installed (NumPy's
nan-functions otherwise), and the side interpreter has bottleneck 1.3.2 with numpy 1.26:
    /opt/conda/bin/python3.9 tests/golden/make_composite_fixtures.py
Writes tests/golden/composite_reference.npz: small seeded stacks (t, c, h, w) after the nodata rule and the harmonisation (float64
with NaN), `bottleneck.nanmedian(axis=0)` of each, and `bottleneck.nanmean / nanstd` over the band axis of that median.  The
restatement in tests/composite_oracle.py must reproduce all three exactly (tests/test_composite_cpu.py)."""
import os

import bottleneck as bn
import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
rng = np.random.default_rng(20220125)

out = {}
for name, (t, c, h, w), dtype in [('a', (5, 4, 9, 11), np.uint16), ('b', (12, 4, 8, 8), np.uint16), ('c', (6, 13, 5, 7), np.int16),
                                 ('d', (7, 3, 6, 6), np.float32)]:
    if dtype == np.float32:
        raw = (rng.random((t, c, h, w)) * 4000).astype(np.float32)
    elif dtype == np.int16:
        raw = rng.integers(-50, 6000, (t, c, h, w)).astype(np.int16)
    else:
        raw = rng.integers(1, 12000, (t, c, h, w)).astype(np.uint16)
    raw[rng.random(raw.shape) < 0.3] = 0
    raw[:, :, 0, 0] = 0                                       # a pixel with no valid sample
    raw[:, 1, 1, 1] = 0                                       # one band of a pixel without a valid sample
    offsets = np.where(np.arange(t) >= t // 2, 1000.0, 0.0)
    x = raw.astype(np.float64)
    x = np.where(x > 0, x, np.nan)
    off = offsets.reshape(-1, 1, 1, 1)
    x = np.where(off > 0, np.clip(x, off, None) - off, x)
    if dtype == np.float32:
        x = x.astype(np.float32).astype(np.float64)
    med = bn.nanmedian(x, axis=0)
    out[f'{name}_raw'] = raw
    out[f'{name}_offsets'] = offsets
    out[f'{name}_median'] = med
    out[f'{name}_mean'] = bn.nanmean(med, axis=0)
    out[f'{name}_std'] = bn.nanstd(med, axis=0)
out['versions'] = np.array([f'bottleneck {bn.__version__}', f'numpy {np.__version__}'])
np.savez_compressed(os.path.join(OUT, 'composite_reference.npz'), **out)
print({k: getattr(v, 'shape', None) for k, v in out.items()})
