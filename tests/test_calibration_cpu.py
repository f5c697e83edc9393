"""CPU checks of the calibration rules: the NumPy oracle (tests/calibration_oracle.py) against answers that are known without it --
recovery under a strictly increasing map, monotone tables, the identity on an empty region and on self-matching, the nearest-rank
percentile against a sort, int16 ordering across zero, the chain against pairwise matching by hand -- and what the Python layer and
the C ABI refuse before they touch the device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import calibration_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(name, c=2, h=23, w=31, seed=0, lo=None, hi=None):
    rng = np.random.default_rng(seed)
    info = np.iinfo(name)
    lo = info.min // 4 if lo is None else lo
    hi = info.max // 4 if hi is None else hi
    return rng.integers(lo, hi, size=(c, h, w)).astype(name)


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
def test_a_strictly_increasing_map_is_undone_exactly(name):
    img1 = _scene(name, seed=1)
    f = lambda v: (v.astype(np.int64) * 2 + 7 - (60 if name == 'int16' else 0)).astype(name)      # strictly increasing, inside the kind
    img2 = f(img1)
    assert np.array_equal(co.equalize(img1, img2), img1)
    # ... and on a region only: bit for bit on the region
    mask = np.random.default_rng(2).random(img1.shape[1:]) < 0.5
    got = co.equalize(img1, img2, mask=mask)
    assert np.array_equal(got[:, mask], img1[:, mask])


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
def test_tables_are_monotone_and_land_on_occupied_bins(name):
    img1, img2 = _scene(name, seed=3), _scene(name, seed=4)
    region = co.overlap(img1, img2)
    h1, h2 = co.histogram(img1, region), co.histogram(img2, region)
    lut, counts = co.match_lut(h1, h2, name)
    assert np.all(np.diff(lut.astype(np.int64), axis=1) >= 0)
    assert np.array_equal(counts, np.full((2, 2), region.sum()))
    for b in range(2):
        assert np.all(h1[b][lut[b].astype(np.int64) + co.BIAS[name]] > 0)      # every entry, also below image 2's smallest occupied bin
        first2 = np.nonzero(h2[b])[0][0]                        # n1 == n2 here: below it the answer is image 1's smallest occupied bin
        assert np.all(lut[b, :first2].astype(np.int64) + co.BIAS[name] == np.nonzero(h1[b])[0][0])


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
def test_an_empty_region_gives_the_identity(name):
    img1, img2 = _scene(name, seed=5), _scene(name, seed=6)
    empty = np.zeros(img1.shape[1:], np.uint8)
    lut, counts = co.match_lut(co.histogram(img1, empty), co.histogram(img2, empty), name)
    assert np.array_equal(lut.astype(np.int64), np.tile(np.arange(co.BINS[name]) - co.BIAS[name], (2, 1))) and not counts.any()
    assert np.array_equal(co.equalize(img1, img2, mask=empty), img2)
    table, upper = co.scale_lut(co.histogram(img1, empty), name, 99)
    assert np.isnan(table).all() and np.array_equal(upper, [-1, -1])
    # one side empty only: nodata everywhere in image 1
    gone = np.zeros_like(img1)
    assert np.array_equal(co.equalize(gone, np.maximum(img2, 1), nodata=0), np.maximum(img2, 1))


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
def test_matching_an_image_to_itself_is_the_identity_on_its_values(name):
    img = _scene(name, seed=7)
    assert np.array_equal(co.equalize(img, img), img)
    h = co.histogram(img, np.ones(img.shape[1:], np.uint8))
    lut, _ = co.match_lut(h, h, name)
    for b in range(2):
        occ = np.nonzero(h[b])[0]
        assert np.array_equal(lut[b, occ].astype(np.int64) + co.BIAS[name], occ)


@pytest.mark.parametrize('name', ['uint8', 'uint16', 'int16'])
@pytest.mark.parametrize('p', [1, 50, 99, 100])
def test_the_percentile_is_the_nearest_rank_of_a_sort(name, p):
    img = _scene(name, c=1, seed=8, lo=1 if name != 'int16' else None)
    _, upper = co.scale_lut(co.histogram(img, np.ones(img.shape[1:], np.uint8)), name, p)
    s = np.sort(img.ravel())
    n = s.size
    assert upper[0] == s[-(-p * n // 100) - 1]                  # the ceil(p n / 100)-th smallest
    if upper[0] > 0:
        got = co.clamp_and_scale(img, p)
        want = (np.minimum(img, upper[0]).astype(np.float64) / float(upper[0])).astype(np.float32)
        assert np.array_equal(got, want) and got.max() == 1.0


def test_scale_of_invalid_samples_and_of_a_zero_percentile():
    img = np.array([[[0, 5, 10, 20]]], np.uint16)
    got = co.clamp_and_scale(img, 50, nodata=0)
    assert np.isnan(got[0, 0, 0]) and np.array_equal(got[0, 0, 1:], np.array([0.5, 1.0, 1.0], np.float32))
    zeros = np.zeros((1, 2, 2), np.uint8)
    table, upper = co.scale_lut(co.histogram(zeros, np.ones((2, 2))), 'uint8', 99)
    assert upper[0] == 0 and np.isnan(table).all()


def test_int16_bins_are_ordered_across_zero():
    img1 = np.array([[[-32768, -300, -1, 0, 1, 300, 32767]]], np.int16)
    img2 = np.array([[[-5, -4, -3, -2, -1, 0, 1]]], np.int16)
    assert np.array_equal(co.equalize(img1, img2), img1)         # rank for rank, negative values first
    h = co.histogram(img1, np.ones((1, 7)))
    assert np.array_equal(np.nonzero(h[0])[0], [0, 32468, 32767, 32768, 32769, 33068, 65535])


def test_nodata_outside_the_kind_matches_nothing():
    img = np.array([[[0, 1, 2]]], np.int16)
    assert co.overlap(img, None, nodata=65535).all() and co.overlap(img, None, nodata=0.5).all()
    assert np.array_equal(co.overlap(img, None, nodata=0), [[0, 1, 1]])


def test_a_chain_of_three_scenes_is_pairwise_matching_in_order():
    rng = np.random.default_rng(11)
    base = rng.integers(100, 4000, size=(2, 20, 30)).astype(np.uint16)
    stack = np.stack([base, (base * 1.3 + 50).astype(np.uint16), (base * 0.7 + 11).astype(np.uint16)])
    stack[0, :, :, 20:] = 0
    stack[1, :, :, :8] = 0
    stack[2, :, :, :15] = 0
    got = co.equalize_collection(stack, nodata=0)
    e1 = co.equalize(stack[0], stack[1], nodata=0)
    e2 = co.equalize(e1, stack[2], nodata=0)
    assert np.array_equal(got, np.stack([stack[0], e1, e2]))
    assert np.array_equal(got == 0, stack == 0)                  # validity is preserved: no table value is nodata
    # another order: the chain starts at scene 2
    rev = co.equalize_collection(stack, nodata=0, order=[2, 1, 0])
    r1 = co.equalize(stack[2], stack[1], nodata=0)
    assert np.array_equal(rev, np.stack([co.equalize(r1, stack[0], nodata=0), r1, stack[2]]))
    # the seam: where scenes 0 and 1 overlap, the equalized scene 1 has scene 0's distribution
    both = (stack[0] != 0).all(axis=0) & (stack[1] != 0).all(axis=0)
    assert np.array_equal(np.sort(e1[0][both]), np.sort(stack[0][0][both]))


# ---------------------------------------------------------------------------------------------------------------- the host layer
def test_descriptor_layout_matches_the_header(tmp_path):
    from satellite_computervision_amd import _lib as L
    cname, cls = 'satcv_calib_apply_desc', L.CalibApplyDesc
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
    for sym in ('overlap', 'histogram', 'match_lut', 'scale_lut', 'apply'):
        assert f'satcv_calib_{sym}' in L.EXPORTED_SYMBOLS


def test_the_c_abi_refuses_null_pointers_without_a_device():
    from satellite_computervision_amd import _lib as L
    calls = [lambda: L.lib.satcv_calib_overlap(None, None, 1, 1, 4, 4, 0, 0.0, None, None, None),
             lambda: L.lib.satcv_calib_histogram(None, 1, 1, 4, 4, None, None, 0, None),
             lambda: L.lib.satcv_calib_match_lut(None, None, 1, 1, None, None, None),
             lambda: L.lib.satcv_calib_scale_lut(None, 1, 1, 99, None, None, None),
             lambda: L.lib.satcv_calib_apply(None, None)]
    for call in calls:
        assert call() == -1 and b'null pointer' in L.lib.satcv_last_error()


def test_the_python_layer_refuses_before_it_touches_the_device():
    from satellite_computervision_amd import calibration as cal
    u16 = np.zeros((2, 4, 4), np.uint16)
    for bad in (np.zeros((2, 4, 4), np.float32), np.zeros((2, 4, 4), np.int32), np.zeros((2, 4, 4), np.float64)):
        for call in (lambda: cal.get_overlap(bad), lambda: cal.make_FC(bad), lambda: cal.equalize(bad, bad), lambda: cal.clamp_and_scale(bad),
                     lambda: cal.equalize_collection(bad[None])):
            with pytest.raises(ValueError, match='uint8, uint16 and int16'):
                call()
    for p in (0, 101, -1, 99.0, True, None):
        with pytest.raises(ValueError, match='percentile'):
            cal.clamp_and_scale(u16, p=p)
    for shape in ((4, 4), (17, 4, 4), (1, 2, 4, 4), (0, 4, 4)):
        with pytest.raises(ValueError, match='raster'):
            cal.get_overlap(np.zeros(shape, np.uint16))
    with pytest.raises(ValueError, match='a stack'):
        cal.equalize_collection(u16)
    for order in ([0, 0, 1], [0, 1], [1, 2, 3]):
        with pytest.raises(ValueError, match='permutation'):
            cal.equalize_collection(np.zeros((3, 1, 4, 4), np.uint16), order=order)
    with pytest.raises(ValueError, match='does not describe'):
        cal.get_overlap(np.zeros((1, 4, 4), np.uint8), dtype='uint16')
    with pytest.raises(ValueError, match='float32 and int32 are refused'):
        cal.get_overlap(u16, dtype='float32')
    assert cal.kind_name(np.dtype(np.int16), 'uint16') == 'uint16' and cal.KINDS == {'uint8': 0, 'uint16': 1, 'int16': 3}


def test_hist_to_fc_on_a_host_histogram():
    from satellite_computervision_amd import calibration as cal
    img = np.array([[[3, 3, 9, 200]]], np.uint8)
    h = co.histogram(img, np.ones((1, 4)))
    dn, prob = cal.hist_to_FC(h, 0)
    assert np.array_equal(dn, [3, 9, 200]) and np.array_equal(prob, [0.5, 0.75, 1.0]) and prob.dtype == np.float64
    h16 = co.histogram(np.array([[[-2, 5]]], np.int16), np.ones((1, 2)))
    dn, prob = cal.hist_to_FC(h16, 0, dtype='int16')
    assert np.array_equal(dn, [-2, 5]) and np.array_equal(prob, [0.5, 1.0])
    dn, prob = cal.hist_to_FC(np.zeros((1, 256), np.uint32), 0)
    assert dn.size == 0 and prob.size == 0
    with pytest.raises(ValueError):
        cal.hist_to_FC(h, 0, dtype='int16')
