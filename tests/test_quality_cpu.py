"""CPU checks of the quality-mask feature: the exact (integer) and the literal (float64) restatements of utils/ee_tools.py agree off
the thresholds (tests/quality_oracle.py), the seeded generator is a real mixture, the host checks of satcv_quality_mask and
satcv_median_composite_masked (rejected before any launch), the ctypes mirrors of both descriptors against the header, and the host
logic of ee_tools (band names, rule sets)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CASES = [(np.uint16, 8, 37, 53, 'BANDS9'), (np.int16, 17, 4, 10, 'BANDS14'), (np.float32, 5, 3, 1301, 'BANDS14')]


@pytest.mark.parametrize('dtype,t,H,W,which', CASES, ids=lambda v: getattr(v, '__name__', str(v)))
def test_exact_and_literal_forms_agree_off_the_thresholds(dtype, t, H, W, which):
    import quality_oracle as Q
    bands = getattr(Q, which)
    stack, offsets = Q.make_stack(7 + t, dtype, t, H, W, bands)
    for offs in (offsets, None):
        score, on = Q.cloud_score_exact(stack, bands, offs, with_flag=True)
        lit = Q.cloud_score_float(stack, bands, offs)
        assert np.array_equal(score == 255, lit == 255)
        assert np.array_equal(score[~on], lit[~on]), int((score[~on] != lit[~on]).sum())
        assert np.all(np.abs(score[on].astype(int) - lit[on].astype(int)) <= 1)        # on a threshold the float form may truncate one lower
        water, won = Q.water_decision_exact(stack, bands, offs, with_flag=True)
        ws = Q.water_score_float(stack, bands, offs)
        with np.errstate(invalid='ignore'):
            lit_water = ws > 0.25                                                      # mask :264 keeps `<= 0.25`
        assert np.array_equal(water[~won], lit_water[~won]), int((water[~won] != lit_water[~won]).sum())
        ok = ~np.isnan(ws)
        assert ws[ok].min() >= 0 and ws[ok].max() <= 1
    if H * W >= Q.PLANTED_PIXELS:                                                      # the planted thresholds are among the flagged samples
        score, on = Q.cloud_score_exact(stack, bands, offsets, with_flag=True)
        flat_on, flat = on.reshape(t, -1), score.reshape(t, -1)
        for k in range(6):
            assert flat_on[:, Q.P_TERM0 + 2 * k].all() and np.all(flat[:, Q.P_TERM0 + 2 * k] == 16)
            assert np.all(flat[:, Q.P_TERM0 + 2 * k + 1] == 15)


@pytest.mark.parametrize('dtype,t,H,W,which', CASES, ids=lambda v: getattr(v, '__name__', str(v)))
def test_generator_is_a_mixture(dtype, t, H, W, which):
    """a condition on the inputs: a mask of all ones or of all zeros cannot pass the comparisons that use this generator"""
    import quality_oracle as Q
    bands = getattr(Q, which)
    stack, offsets = Q.make_stack(7 + t, dtype, t, H, W, bands)
    valid = Q.cloud_score_exact(stack, bands, offsets) != 255
    cloud_clear = Q.clear_exact(stack, bands, Q.CLOUD, offsets)
    water = Q.water_decision_exact(stack, bands, offsets)
    presets = ['toa', 'mask'] + (['sr'] if 'SCL' in bands else [])
    shares = {p: Q.clear_exact(stack, bands, Q.PRESETS[p], offsets).mean() for p in presets}
    print(f'valid {valid.mean():.3f}, cloud-clear of valid {cloud_clear[valid].mean():.3f}, water {water.mean():.3f}, clear shares {shares}')
    assert 0.2 <= cloud_clear.mean() <= 0.9
    for p, share in shares.items():
        assert 0.2 <= share <= 0.9, (p, share)
    assert water.mean() > 0


def test_planted_pixels_are_what_they_claim():
    import quality_oracle as Q
    t, H, W = 5, 4, 10
    stack, offsets = Q.make_stack(3, np.uint16, t, H, W, Q.BANDS14)
    flat = lambda a: a.reshape(t, -1)
    for rule in (Q.QA60, Q.CLOUD, Q.SHADOW, Q.WATER, Q.SCL, Q.PRESETS['toa'], Q.PRESETS['sr'], Q.PRESETS['mask']):
        c = flat(Q.clear_exact(stack, Q.BANDS14, rule, offsets))
        assert not c[:, Q.P_NONE].any() and c[:, Q.P_ALL].all(), rule
        assert c[:, Q.P_ONE].sum() == 1 and c[t - 1, Q.P_ONE] and c[:, Q.P_TWO].sum() == 2, rule
    qa = flat(Q.clear_exact(stack, Q.BANDS14, Q.QA60, offsets))
    assert not qa[:, Q.P_QA10].any() and not qa[:, Q.P_QA11].any() and qa[:, Q.P_SCL0].all()
    assert not flat(Q.clear_exact(stack, Q.BANDS14, Q.SCL, offsets))[:, Q.P_SCL0].any()
    score = flat(Q.cloud_score_exact(stack, Q.BANDS14, offsets))
    assert np.all(score[:, Q.P_NODATA_BAND] == 255) and np.all(score[:, Q.P_ALL] == 0)
    assert not flat(Q.clear_exact(stack, Q.BANDS14, Q.SHADOW, offsets))[:, Q.P_NODATA_BAND].any()
    med, _ = Q.masked_composite(stack, Q.clear_exact(stack, Q.BANDS14, Q.PRESETS['toa'], offsets), offsets, [Q.BANDS14.index(b) for b in ('B2', 'B3', 'B4', 'B8')])
    med = med.reshape(-1, 4)
    assert np.isnan(med[Q.P_NONE]).all() and np.array_equal(med[Q.P_ALL], [800, 900, 1000, 3000]) and np.array_equal(med[Q.P_TWO], [700, 900, 1000, 3000])
    assert np.array_equal(Q.pack_bits(np.ones((33, 1, 2), bool)).ravel(), [0xffffffff, 0xffffffff, 1, 1])


# ---------------------------------------------------------------------------------------------------------------- host checks
def _qdesc(L, **kw):
    """a descriptor every check accepts (the pointers are never followed: each case below breaks one field)"""
    base = dict(src=0x1000, src_kind=1, t=6, cs=9, h=8, w_=8, offsets=None, band=(ctypes.c_int32 * 10)(0, 1, 2, 3, 4, 5, 6, 7, 8, -1),
                rules=3, cloud_max=15, shadow_min=900.0, clear=0x2000, cloud_score=None, water_score=None)
    base.update(kw)
    return L.QualityDesc(**base)


def _bands(*v):
    return (ctypes.c_int32 * 10)(*v)


@pytest.mark.parametrize('change,message', [
    (dict(src=None), b'null pointer'),
    (dict(clear=None), b'every output is null'),
    (dict(t=0), b'sizes must be positive'),
    (dict(cs=0), b'sizes must be positive'),
    (dict(h=-1), b'sizes must be positive'),
    (dict(cs=17), b'at most 16'),
    (dict(src_kind=0), b'src_kind 0'),
    (dict(src_kind=4), b'src_kind 4'),
    (dict(t=257), b'at most 256'),
    (dict(h=65536, w_=32768), b'beyond 2^31 pixels'),
    (dict(rules=32), b'unknown bits'),
    (dict(rules=16), b'role SCL is absent'),                                            # a rule without its role
    (dict(rules=1, band=_bands(0, 1, 2, 3, 4, 5, 6, 7, -1, -1)), b'role QA60 is absent'),
    (dict(rules=2, band=_bands(0, 1, 2, 3, 4, -1, 6, 7, 8, -1)), b'role B10 is absent'),
    (dict(rules=4, band=_bands(0, 1, 2, 3, 4, 5, -1, 7, 8, -1)), b'role B11 is absent'),
    (dict(rules=8, band=_bands(0, 1, 2, 3, 4, 5, 6, -1, 8, -1)), b'role B12 is absent'),
    (dict(rules=1, water_score=0x3000, band=_bands(0, 1, 2, 3, 4, 5, 6, -1, 8, -1)), b'role B12 is absent'),     # an output without its role
    (dict(rules=1, cloud_score=0x3000, band=_bands(-1, 1, 2, 3, 4, 5, 6, 7, 8, -1)), b'role B1 is absent'),
    (dict(band=_bands(0, 1, 2, 3, 4, 5, 6, 7, 9, -1)), b'role QA60 at plane 9 out of range'),
])
def test_quality_host_checks_reject_before_any_launch(change, message):
    from satellite_computervision_amd import _lib as L
    d = _qdesc(L, **change)
    rc = L.lib.satcv_quality_mask(ctypes.byref(d), None)
    assert rc == -1
    assert message in L.lib.satcv_last_error(), L.lib.satcv_last_error()
    with pytest.raises(L.SatcvError):
        L.check(rc)


def _mdesc(L, base=None, **kw):
    b = dict(src=0x1000, src_kind=1, t=6, c=4, h=8, w_=8, offsets=None, median=0x2000, ld_med=4, coff_med=0,
             norm=0x3000, ld_norm=8, coff_norm=4, use_fill=0, fill=0.0)
    b.update(base or {})
    m = dict(clear=0x4000, cs=14, band_idx=(ctypes.c_int32 * 16)(1, 2, 3, 7))
    m.update(kw)
    return L.CompositeMaskedDesc(base=L.CompositeDesc(**b), **m)


@pytest.mark.parametrize('base,change,message', [
    (dict(src=None), {}, b'null pointer'),
    (dict(median=None, norm=None), {}, b'both outputs are null'),
    (dict(t=0), {}, b'sizes must be positive'),
    (dict(c=17, ld_med=17, ld_norm=34), {}, b'at most 16'),
    (dict(src_kind=4), {}, b'src_kind 4'),
    (dict(ld_med=3), {}, b'coff_med + c <= ld_med'),
    (dict(coff_norm=5), {}, b'coff_norm + c <= ld_norm'),
    (dict(t=257), {}, b'at most 256'),
    (dict(h=65536, w_=32768), {}, b'beyond 2^31 pixels'),
    ({}, dict(cs=17), b'cs = 17'),
    ({}, dict(cs=0), b'cs = 0'),
    ({}, dict(band_idx=(ctypes.c_int32 * 16)(1, 2, 3, 14)), b'band_idx[3] = 14 out of range'),
    ({}, dict(band_idx=(ctypes.c_int32 * 16)(-1, 2, 3, 4)), b'band_idx[0] = -1 out of range'),
    ({}, dict(cs=3), b'band_idx[2] = 3 out of range'),
])
def test_masked_composite_host_checks_reject_before_any_launch(base, change, message):
    from satellite_computervision_amd import _lib as L
    d = _mdesc(L, base, **change)
    rc = L.lib.satcv_median_composite_masked(ctypes.byref(d), None)
    assert rc == -1
    assert message in L.lib.satcv_last_error(), L.lib.satcv_last_error()
    assert b'median_composite_masked' in L.lib.satcv_last_error()


def test_null_descriptors_are_rejected():
    from satellite_computervision_amd import _lib as L
    assert L.lib.satcv_quality_mask(None, None) == -1 and b'null pointer' in L.lib.satcv_last_error()
    assert L.lib.satcv_median_composite_masked(None, None) == -1 and b'null pointer' in L.lib.satcv_last_error()


@pytest.mark.parametrize('cname,clsname', [('satcv_quality_desc', 'QualityDesc'), ('satcv_composite_masked_desc', 'CompositeMaskedDesc')])
def test_descriptor_layouts_match_the_header(tmp_path, cname, clsname):
    import re
    from satellite_computervision_amd import _lib as L
    cls = getattr(L, clsname)
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
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    bits = {k: int(v) for k, v in re.findall(r'#define SATCV_Q_(QA60|CLOUD|SHADOW|WATER|SCL) (\d+)', hdr)}
    assert bits == dict(QA60=L.Q_QA60, CLOUD=L.Q_CLOUD, SHADOW=L.Q_SHADOW, WATER=L.Q_WATER, SCL=L.Q_SCL) == dict(QA60=1, CLOUD=2, SHADOW=4, WATER=8, SCL=16)
    assert int(re.search(r'#define SATCV_Q_ROLES (\d+)', hdr).group(1)) == len(L.Q_ROLES) == 10


# ---------------------------------------------------------------------------------------------------------------- ee_tools host logic
def test_band_names_and_rule_sets():
    import quality_oracle as Q
    from satellite_computervision_amd import ee_tools as ee
    assert ee.ROLES == ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60', 'SCL')
    s2 = ['B01', 'B02', 'B03', 'B04', 'B05', 'B06', 'B07', 'B08', 'B8A', 'B09', 'B10', 'B11', 'B12', 'QA60']
    assert ee.band_table(s2) == [0, 1, 2, 3, 7, 10, 11, 12, 13, -1]
    assert ee.band_table(['B1', 'B2', 'B3', 'B4', 'B5', 'B6', 'B7', 'B8', 'B8A', 'B9', 'B10', 'B11', 'B12', 'QA60']) == ee.band_table(s2)
    assert ee.band_table(Q.BANDS14) == [Q.BANDS14.index(r) for r in ee.ROLES]
    assert ee.band_table(['b8a', 'scl']) == [-1] * 9 + [1]                              # B8A is not B8
    with pytest.raises(ValueError, match='repeat'):
        ee.band_table(['B01', 'B1'])
    assert ee.rule_set('toa') == ee.QA60 | ee.CLOUD == 3
    assert ee.rule_set('sr') == ee.QA60 | ee.SCL == 17
    assert ee.rule_set('mask') == ee.QA60 | ee.CLOUD | ee.SHADOW | ee.WATER == 15
    assert ee.rule_set(['cloud', 'water']) == 10 and ee.rule_set(4) == 4 and ee.rule_set('shadow') == 4
    for bad in ('clouds', 0, 32, []):
        with pytest.raises(ValueError):
            ee.rule_set(bad)
    assert (ee.PRESETS, (ee.QA60, ee.CLOUD, ee.SHADOW, ee.WATER, ee.SCL)) == (Q.PRESETS, (Q.QA60, Q.CLOUD, Q.SHADOW, Q.WATER, Q.SCL))


def test_python_surface_refuses_bad_arguments_without_a_device():
    from satellite_computervision_amd import ee_tools as ee, pc_tools as pc
    z = np.zeros((2, 9, 2, 2), np.uint16)
    with pytest.raises(ValueError, match='T, C, H, W'):
        ee.maskTOA(z[0], ['B1'])
    with pytest.raises(ValueError, match='9 band names'):
        ee.maskTOA(z, ['B1', 'B2'])
    with pytest.raises(ValueError, match='rule scl reads SCL'):
        ee.maskSR(z, ['B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60'])
    with pytest.raises(ValueError, match='rule cloud reads B10'):
        ee.sentinelCloudScore(z, ['B1', 'B2', 'B3', 'B4', 'B8', 'B9', 'B11', 'B12', 'QA60'])
    with pytest.raises(ValueError, match='not both'):
        ee.basicQA(z, ['B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60'], offsets=[0, 0], times=[np.datetime64('2022-01-01')] * 2)
    with pytest.raises(ValueError, match='need band_names'):
        pc.median_composite(z, bands=['B2'])
    with pytest.raises(ValueError, match='not among band_names'):
        pc.median_composite(z, bands=['B5'], band_names=['B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60'])
    with pytest.raises(ValueError, match='outside the 9 planes'):
        pc.median_composite(z, bands=[0, 9])
    with pytest.raises(ValueError, match='ClearMask'):
        pc.median_composite(z, clear=np.ones((2, 2, 2), bool))
    with pytest.raises(ValueError, match='need band_names'):
        pc.predict_change(z, z, None, quality='toa')
    with pytest.raises(ValueError, match='rule scl reads SCL'):
        pc.predict_change(z, z, None, quality='sr', band_names=['B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60'])


def test_array_helpers():
    from satellite_computervision_amd import ee_tools as ee
    x = np.array([0.1, 0.3, 0.5])
    assert np.allclose(ee.rescale(x, 'img', [0.1, 0.5]), [0, 0.5, 1]) and np.allclose(ee.rescale(x, lambda v: v * 2, [0.2, 1.0]), [0, 0.5, 1])
    s = np.full((2, 3, 1, 1), 5000, np.uint16)
    toa = ee.sentinel2toa(s, ['B02', 'QA60', 'B11'])
    assert toa.dtype == np.float64 and np.array_equal(toa[:, 0], np.full((2, 1, 1), 0.5)) and np.array_equal(toa[:, 1], np.full((2, 1, 1), 5000.0))
