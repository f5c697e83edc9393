"""Host side of the device-resident scene prediction (prediction_tools.predict_chips_device / predict_scene / callback_predictions): the
full-cover grid and the reflect rule, the greedy split of overlapping centres into disjoint scatter launches, the ValueError paths that
must be reached before any device call, the callback_predictions placement rule, and the C ABI of the two new entry points (descriptor
layouts, argument validation).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirror(i, n):
    """the gather kernel's coordinate rule: np.pad(mode='reflect'), then clamped"""
    if i < 0:
        i = -i
    elif i >= n:
        i = 2 * (n - 1) - i
    return min(max(i, 0), n - 1)


@pytest.mark.parametrize('kernel,buff', [(32, 16), (64, 32), (256, 128)])
def test_full_cover_grid_covers_every_pixel_once(kernel, buff):
    from satellite_computervision_amd import prediction_tools as pt
    sizes = [kernel + buff, kernel + buff + 1, 2 * kernel + 1, 3 * kernel + 1, 3 * kernel - 1, 3 * kernel, 5 * kernel + 7]
    assert any(h % kernel == 1 for h in sizes) and sizes[0] == kernel + buff
    for H, W in zip(sizes, reversed(sizes)):
        count = np.zeros((H, W), np.int64)
        idx = pt.full_cover_indices((H, W, 4), kernel)
        for y, x in idx:
            count[y:y + kernel, x:x + kernel] += 1           # NumPy clips the slice like the scatter clips the centre
        assert count.min() == 1 and count.max() == 1, (H, W)
        assert pt._disjoint_runs(idx, kernel, kernel) == [(0, len(idx))]
        # the mirrored window coordinates stay inside the scene and are those of np.pad(mode='reflect')
        off = buff // 2
        side = kernel + buff
        line = np.arange(H)
        padded = np.pad(line, (off, kernel + off), mode='reflect')
        for y in range(0, H, kernel):
            got = [_mirror(y - off + r, H) for r in range(side)]
            assert min(got) >= 0 and max(got) < H
            assert np.array_equal(line[got], padded[y:y + side]), (H, y)


def test_disjoint_runs_split_overlaps_greedily_in_list_order():
    from satellite_computervision_amd import prediction_tools as pt
    k = 32
    grid = [(y, x) for y in range(0, 96, k) for x in range(0, 128, k)]
    assert pt._disjoint_runs(grid, k, k) == [(0, len(grid))]                   # a disjoint list stays one launch
    assert pt._disjoint_runs([], k, k) == []
    idx = [(0, 0), (0, 32), (16, 16), (64, 64), (64, 64), (200, 0), (0, 31)]
    runs = pt._disjoint_runs(idx, k, k)
    assert runs == [(0, 2), (2, 4), (4, 7)]
    assert [i for a, b in runs for i in range(a, b)] == list(range(len(idx)))   # order kept, nothing dropped
    rng = np.random.default_rng(0)
    idx = [(int(y), int(x)) for y, x in rng.integers(0, 150, (60, 2))]
    runs = pt._disjoint_runs(idx, k, 20)                                        # non-square rectangles (callback_predictions' crop)
    assert [i for a, b in runs for i in range(a, b)] == list(range(60))
    for a, b in runs:
        cover = np.zeros((200, 200), np.int64)
        for y, x in idx[a:b]:
            cover[y:y + k, x:x + 20] += 1
        assert cover.max() == 1
        if b < 60:                                                              # greedy: the next chip did overlap this run
            y, x = idx[b]
            assert cover[y:y + k, x:x + 20].max() == 1


class _Stub:
    """a model that must never be asked to predict"""
    outputs = ['probs']
    inputs = ['x']

    def predict_on_device(self, x):
        raise AssertionError('device call before the arguments were checked')

    predict = predict_on_device


def test_value_errors_are_raised_before_any_device_call():
    from satellite_computervision_amd import prediction_tools as pt
    m = _Stub()
    arr = np.zeros((100, 120, 4), np.float32)
    t = np.ones((100, 120))
    assert pt.predict_chips_device(arr, [], t, m, 32, 16) is t and np.array_equal(t, np.ones((100, 120)))      # empty list: untouched
    for bad in [(4, 40), (40, 4), (-8, 40), (100 - 32 - 8 + 1, 8), (8, 120 - 32 - 8 + 1)]:
        with pytest.raises(ValueError, match='leaves the'):
            pt.predict_chips_device(arr, [(8, 8), bad], t, m, 32, 16)
    with pytest.raises(ValueError, match='pair'):
        pt.predict_chips_device((arr, arr, arr), [(8, 8)], t, m, 32, 16)
    with pytest.raises(ValueError, match='co-registered'):
        pt.predict_chips_device((arr, arr[:50]), [(8, 8)], t, m, 32, 16)
    with pytest.raises(ValueError, match='batch_size'):
        pt.predict_chips_device(arr, [(8, 8)], t, m, 32, 16, batch_size=0)
    assert np.array_equal(t, np.ones((100, 120)))
    with pytest.raises(ValueError, match="cover='full' needs"):
        pt.predict_scene(np.zeros((47, 120, 4), np.float32), m, 32, 16, cover='full')
    with pytest.raises(ValueError, match="cover='full' needs"):
        pt.predict_scene(np.zeros((120, 47, 4), np.float32), m, 32, 16, cover='full')
    with pytest.raises(ValueError, match='cover must be'):
        pt.predict_scene(arr, m, 32, 16, cover='everything')
    with pytest.raises(ValueError, match='classes=True'):
        pt.predict_scene(arr, m, 32, 16, classes=True)                          # single-output model
    with pytest.raises(ValueError, match='does not fill one mosaic row'):
        pt._patch_grid(2, 3, (48, 48), [32, 32], [16, 16])
    with pytest.raises(ValueError, match='empty crop'):
        pt._patch_grid(6, 3, (8, 48), [32, 32], [16, 16])


class _PatchStub:
    """predict() of a model whose patch i is the constant i + 1 in channel 1 plus a position ramp, -1 in channel 0"""

    def __init__(self, n, h, w):
        ramp = np.arange(h)[:, None] * 1000.0 + np.arange(w)[None, :]
        self.out = np.stack([np.full((n, h, w), -1.0), (np.arange(n)[:, None, None] + 1) * 1e6 + ramp[None]], axis=-1).astype(np.float64)

    def predict(self, x, steps=None, verbose=0):
        return [self.out[:steps], np.zeros(self.out.shape[:3], np.int32)[:steps]]


def _reference_mosaic(predictions, patches, cols, kernel_shape, kernel_buffer):
    """what utils/prediction_tools.py:245-291 assembles, restated with NumPy: channel 1 of every patch cropped to rows
    [kernel_buffer[1] // 2, kernel_shape[1] + kernel_buffer[0] // 2) and columns [kernel_buffer[0] // 2, kernel_shape[0] + kernel_buffer[1] // 2),
    `cols` crops side by side per mosaic row, complete rows only"""
    if isinstance(predictions, list):
        predictions = predictions[0]
    xb, yb = kernel_buffer[0] // 2, kernel_buffer[1] // 2
    crops = [p[yb:kernel_shape[1] + xb, xb:kernel_shape[0] + yb, 1] for p in predictions]
    return np.concatenate([np.concatenate(crops[r * cols:(r + 1) * cols], axis=1) for r in range(patches // cols)], axis=0)


@pytest.mark.parametrize('patches,cols,patch,kshape,kbuf', [
    (6, 3, (48, 48), [32, 32], [16, 16]),
    (6, 3, (56, 48), [32, 40], [16, 16]),             # non-square kernel
    (8, 2, (48, 48), [32, 32], [16, 8]),              # non-square buffer: the crop is 36 x 28
    (7, 3, (48, 48), [32, 32], [8, 16]),              # trailing partial row is dropped
    (4, 2, (40, 40), [32, 32], [16, 16]),             # stop beyond the patch: clipped like a NumPy slice
])
def test_callback_predictions_placement_rule(patches, cols, patch, kshape, kbuf):
    from satellite_computervision_amd import prediction_tools as pt
    stub = _PatchStub(patches, *patch)
    want = _reference_mosaic(stub.predict(None, steps=patches), patches, cols, kshape, kbuf)
    crop, origins, hw = pt._patch_grid(patches, cols, patch, kshape, kbuf)
    assert len(origins) == (patches // cols) * cols and hw == want.shape
    got = np.full(hw, np.nan)
    for i, (y, x) in enumerate(origins):                     # what the scatter kernel does with this table
        got[y:y + crop[2], x:x + crop[3]] = stub.out[i, crop[0]:crop[0] + crop[2], crop[1]:crop[1] + crop[3], 1]
    assert np.array_equal(got, want)
    assert pt._disjoint_runs(origins, crop[2], crop[3]) == [(0, len(origins))]


def test_scene_descriptor_layouts_match_the_header(tmp_path):
    from satellite_computervision_amd import _lib
    pairs = {'satcv_scene_gather_desc': _lib.SceneGatherDesc, 'satcv_scene_scatter_desc': _lib.SceneScatterDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(cls, fname).offset, f'{cname}.{fname}'


def test_scene_entry_points_validate_their_arguments_without_gpu():
    """every bad descriptor is refused on the host with a message; nothing is launched (the pointers are never dereferenced)"""
    from satellite_computervision_amd import _lib
    lib = _lib.lib
    P = 4096                                                  # a non-null stand-in: validation fails before any use

    def gather(**kw):
        f = dict(src=P, src_kind=1, h=100, w_=90, c=4, rescale=0.0, origins=P, total=8, first=0, n=8, off=8, side=48, dst=P, ldc=4, coff=0)
        f.update(kw)
        return lib.satcv_scene_gather(ctypes.byref(_lib.SceneGatherDesc(**f)), None), lib.satcv_last_error()

    def scatter(**kw):
        f = dict(src=P, src_kind=2, n=8, sh=48, sw=48, lds=2, c0=0, nc=1, crop_y=8, crop_x=8, crop_h=32, crop_w=32, origins=P, total=8, first=0,
                 dst=P, dst_kind=2, h=100, w_=90, ldd=1, doff=0, accumulate=1)
        f.update(kw)
        return lib.satcv_scene_scatter(ctypes.byref(_lib.SceneScatterDesc(**f)), None), lib.satcv_last_error()

    assert lib.satcv_scene_gather(None, None) == -1 and lib.satcv_scene_scatter(None, None) == -1
    for kw, msg in [(dict(src=None), b'null'), (dict(origins=None), b'null'), (dict(dst=None), b'null'), (dict(h=0), b'positive'),
                    (dict(side=0), b'positive'), (dict(n=0), b'positive'), (dict(off=-1), b'positive'), (dict(src_kind=4), b'src_kind'),
                    (dict(src_kind=-1), b'src_kind'), (dict(ldc=4, coff=1), b'coff + c <= ldc'), (dict(coff=-1), b'coff + c <= ldc'),
                    (dict(first=1), b'origin table'), (dict(first=-1), b'origin table'), (dict(n=2 ** 20, total=2 ** 20, side=4096), b'2^31')]:
        rc, err = gather(**kw)
        assert rc == -1 and msg in err, (kw, err)
    for kw, msg in [(dict(src=None), b'null'), (dict(origins=None), b'null'), (dict(dst=None), b'null'), (dict(nc=0), b'positive'),
                    (dict(ldd=0), b'positive'), (dict(crop_y=20), b'crop outside'), (dict(crop_w=41), b'crop outside'), (dict(crop_x=-1), b'crop outside'),
                    (dict(c0=1, nc=2), b'c0 + nc <= lds'), (dict(doff=1), b'doff + nc <= ldd'), (dict(src_kind=0), b'src_kind'),
                    (dict(dst_kind=1), b'dst_kind'), (dict(dst_kind=0), b'u8 map'), (dict(src_kind=5, dst_kind=0), b'u8 map'),
                    (dict(first=4), b'origin table')]:
        rc, err = scatter(**kw)
        assert rc == -1 and msg in err, (kw, err)
    with pytest.raises(_lib.SatcvError):
        _lib.check(scatter(nc=0)[0])
