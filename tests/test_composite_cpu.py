"""CPU checks of the median-composite feature: the host checks of satcv_median_composite (rejected before any launch), the ctypes mirror
of satcv_composite_desc against the header, harmonize_offsets / trim_array, and the NumPy restatement (tests/composite_oracle.py)
against what xarray's reductions dispatch to (bottleneck, tests/golden/composite_reference.npz)."""
import ctypes
import os
import subprocess
import sys
from datetime import datetime

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def _desc(L, **kw):
    """a descriptor every check accepts (the pointers are never followed: each case below breaks one field)"""
    base = dict(src=0x1000, src_kind=1, t=6, c=4, h=8, w_=8, offsets=None, median=0x2000, ld_med=4, coff_med=0,
                norm=0x3000, ld_norm=8, coff_norm=4, use_fill=0, fill=0.0)
    base.update(kw)
    return L.CompositeDesc(**base)


@pytest.mark.parametrize('change,message', [
    (dict(src=None), b'null pointer'),
    (dict(median=None, norm=None), b'both outputs are null'),
    (dict(t=0), b'sizes must be positive'),
    (dict(c=0), b'sizes must be positive'),
    (dict(h=-3), b'sizes must be positive'),
    (dict(w_=0), b'sizes must be positive'),
    (dict(c=17, ld_med=17, ld_norm=34), b'at most 16'),
    (dict(src_kind=0), b'src_kind 0'),
    (dict(src_kind=4), b'src_kind 4'),
    (dict(ld_med=3), b'coff_med + c <= ld_med'),
    (dict(coff_med=-1), b'coff_med + c <= ld_med'),
    (dict(coff_norm=5), b'coff_norm + c <= ld_norm'),
    (dict(t=257), b'at most 256'),
    (dict(h=65536, w_=32768), b'beyond 2^31 pixels'),
])
def test_host_checks_reject_before_any_launch(change, message):
    from satellite_computervision_amd import _lib as L
    d = _desc(L, **change)
    rc = L.lib.satcv_median_composite(ctypes.byref(d), None)
    assert rc == -1
    assert message in L.lib.satcv_last_error(), L.lib.satcv_last_error()
    with pytest.raises(L.SatcvError):
        L.check(rc)


def test_null_descriptor_is_rejected():
    from satellite_computervision_amd import _lib as L
    assert L.lib.satcv_median_composite(None, None) == -1 and b'null pointer' in L.lib.satcv_last_error()


def test_time_limit_of_the_binding_is_the_header_s():
    import re
    from satellite_computervision_amd import _lib as L
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    assert int(re.search(r'#define SATCV_COMPOSITE_MAX_T (\d+)', hdr).group(1)) == L.COMPOSITE_MAX_T >= 256


def test_composite_descriptor_layout_matches_the_header(tmp_path):
    from satellite_computervision_amd import _lib as L
    cname, cls = 'satcv_composite_desc', L.CompositeDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f'{cname}.{f}']) == getattr(cls, f).offset, f


def test_harmonize_offsets_on_both_sides_of_and_on_the_cutoff():
    from satellite_computervision_amd import pc_tools as pc
    times = [datetime(2021, 6, 1), datetime(2022, 1, 24, 23, 59, 59), datetime(2022, 1, 25), datetime(2022, 1, 25, 0, 0, 1), datetime(2023, 3, 3)]
    want = np.array([0, 0, 1000, 1000, 1000], np.float32)
    got = pc.harmonize_offsets(times)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(pc.harmonize_offsets(np.array(times, dtype='datetime64[ns]')), want)
    assert np.array_equal(pc.harmonize_offsets([np.datetime64('2022-01-24'), np.datetime64('2022-01-25')]), [0, 1000])
    assert np.array_equal(pc.harmonize_offsets(times, cutoff=datetime(2023, 1, 1), offset=5), [0, 0, 0, 0, 5])
    assert pc.harmonize_offsets([]).shape == (0,)


def test_trim_array_drops_the_remainder_of_the_last_two_axes():
    from satellite_computervision_amd import pc_tools as pc
    a = np.arange(2 * 3 * 37 * 53).reshape(2, 3, 37, 53)
    got = pc.trim_array(a, 8)
    assert got.shape == (2, 3, 32, 48) and np.array_equal(got, a[:, :, :32, :48])
    assert pc.trim_array(a[0, 0], 37).shape == (37, 37)
    assert pc.trim_array(np.zeros((64, 128)), 32).shape == (64, 128)            # nothing to drop


def test_python_surface_refuses_bad_arguments_without_a_device():
    from satellite_computervision_amd import pc_tools as pc
    with pytest.raises(ValueError, match='T, C, H, W'):
        pc.median_composite(np.zeros((4, 8, 8), np.uint16))
    with pytest.raises(ValueError, match='at most 256'):
        pc.median_composite(np.zeros((257, 1, 2, 2), np.uint16))
    with pytest.raises(ValueError, match='not both'):
        pc.median_composite(np.zeros((2, 1, 2, 2), np.uint16), times=[datetime(2022, 1, 1)] * 2, offsets=[0, 0])
    with pytest.raises(ValueError, match='2 offsets'):
        pc.median_composite(np.zeros((2, 1, 2, 2), np.uint16), offsets=[0, 0, 0])
    with pytest.raises(ValueError, match='equal C, H, W'):
        pc.predict_change(np.zeros((2, 4, 8, 8), np.uint16), np.zeros((2, 4, 8, 9), np.uint16), None)


def test_restatement_reproduces_the_bottleneck_fixture():
    """exactly: bottleneck.nanmedian equals np.nanmedian bit for bit, and on data of this size nanmean / nanstd do too"""
    import composite_oracle as O
    z = np.load(os.path.join(GOLD, 'composite_reference.npz'))
    for name in 'abcd':
        raw, offsets = z[f'{name}_raw'], z[f'{name}_offsets']
        med, norm = O.composite(raw, offsets)
        want = z[f'{name}_median'].transpose(1, 2, 0)
        assert np.array_equal(np.isnan(med), np.isnan(want))
        assert np.array_equal(med[~np.isnan(med)], want[~np.isnan(want)])
        mean, sd = z[f'{name}_mean'][..., None], z[f'{name}_std'][..., None]
        want_norm = (want - mean) / (sd + 0.000001)
        assert np.array_equal(np.isnan(norm), np.isnan(want_norm))
        ok = ~np.isnan(norm)
        assert np.array_equal(norm[ok], want_norm[ok])
        assert np.isnan(med[0, 0]).all() and np.isnan(med[1, 1, 1]) and not np.isnan(med[1, 1, 0])      # the fixture has both NaN cases
