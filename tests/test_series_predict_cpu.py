"""Host side of scene prediction for the ConvLSTM2D time-series models (prediction_tools.predict_series_scene): every ValueError is
raised before anything touches the device, and the C ABI of satcv_series_gather (descriptor layout, argument validation).  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, C, H, W, KERNEL, BUFF = 3, 6, 56, 40, 16, 8


class _Stub:
    """a time-series model that must never be asked to predict"""
    n_time, n_channels = T, C

    def predict_on_device(self, *a, **k):
        raise AssertionError('device call before the arguments were checked')

    predict = predict_on_device


def _ae_stub():
    from satellite_computervision_amd import lstm_tools as lt

    class _AEStub(lt.LSTMAutoencoder):
        """an autoencoder by type only: nothing is built, nothing can run"""
        n_time, n_channels = T, C

        def __init__(self):
            pass

        def predict_on_device(self, *a, **k):
            raise AssertionError('device call before the arguments were checked')

        predict = predict_on_device
    return _AEStub()


def test_value_errors_are_raised_before_any_device_call():
    from satellite_computervision_amd import prediction_tools as pt
    m = _Stub()
    stack = np.zeros((T, C, H, W), np.int16)
    kw = dict(kernel=KERNEL, buff=BUFF, batch_size=4)
    for bad in (np.zeros((C, H, W), np.int16), np.zeros((1, T, C, H, W), np.int16), np.zeros((H, W), np.float32)):
        with pytest.raises(ValueError, match=r'\(T, C, H, W\)'):                 # wrong rank
            pt.predict_series_scene(bad, m, **kw)
    with pytest.raises(ValueError, match='acquisitions'):                       # T too small
        pt.predict_series_scene(stack[:T - 1], m, **kw)
    with pytest.raises(ValueError, match='bands'):                              # band mismatch, both ways
        pt.predict_series_scene(stack[:, :C - 2], m, **kw)
    with pytest.raises(ValueError, match='bands'):
        pt.predict_series_scene(np.zeros((T, C + 1, H, W), np.int16), m, **kw)
    with pytest.raises(ValueError, match='cover must be'):
        pt.predict_series_scene(stack, m, cover='everything', **kw)
    for small in (stack[:, :, :KERNEL + BUFF - 1], stack[:, :, :, :KERNEL + BUFF - 1]):
        with pytest.raises(ValueError, match="cover='full' needs"):
            pt.predict_series_scene(small, m, cover='full', **kw)
    with pytest.raises(ValueError, match='batch_size'):
        pt.predict_series_scene(stack, m, kernel=KERNEL, buff=BUFF, batch_size=0)
    with pytest.raises(ValueError, match='maxval'):
        pt.predict_series_scene(stack, m, maxval=0, **kw)
    with pytest.raises(ValueError, match='harmonics'):                          # harmonics given to a model without a second input
        pt.predict_series_scene(stack, m, harmonics=(0.5, 0.5), **kw)


def test_autoencoder_value_errors_are_raised_before_any_device_call():
    from satellite_computervision_amd import prediction_tools as pt
    ae = _ae_stub()
    stack = np.zeros((T + 2, C, H, W), np.float32)
    kw = dict(kernel=KERNEL, buff=BUFF, batch_size=4)
    with pytest.raises(ValueError, match='needs harmonics'):                    # harmonics missing
        pt.predict_series_scene(stack, ae, **kw)
    with pytest.raises(ValueError, match='pair'):
        pt.predict_series_scene(stack, ae, harmonics=(0.1, 0.2, 0.3), **kw)
    with pytest.raises(ValueError, match='classes=True'):                       # an autoencoder has no class output
        pt.predict_series_scene(stack, ae, harmonics=(0.0, 1.0), classes=True, **kw)
    with pytest.raises(ValueError, match='cover must be'):
        pt.predict_series_scene(stack, ae, harmonics=(0.0, 1.0), cover='all', **kw)


def test_predict_scene_still_refuses_a_time_stack():
    from satellite_computervision_amd import prediction_tools as pt
    with pytest.raises(ValueError, match=r'\(H, W, C\)'):
        pt.predict_scene(np.zeros((T, C, H, W), np.float32), _Stub(), KERNEL, BUFF)


def test_series_descriptor_layout_matches_the_header(tmp_path):
    from satellite_computervision_amd import _lib
    cname, cls = 'satcv_series_gather_desc', _lib.SeriesGatherDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "satcv.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f'{cname}.{fname}']) == getattr(cls, fname).offset, fname
    assert 'satcv_series_gather' in _lib.EXPORTED_SYMBOLS


def test_series_gather_validates_its_arguments_without_gpu():
    """every bad descriptor is refused on the host with a message; nothing is launched (the pointers are never dereferenced)"""
    from satellite_computervision_amd import _lib
    lib = _lib.lib
    P = 4096                                                  # a non-null, 16-byte aligned stand-in: validation fails before any use

    def gather(**kw):
        f = dict(src=P, src_kind=3, t=5, c=6, h=56, w_=40, steps=3, maxval=10000.0, origins=P, total=8, first=0, n=8, off=4, side=24, dst=P,
                 dtype=_lib.BF16, cpad=16)
        f.update(kw)
        return lib.satcv_series_gather(ctypes.byref(_lib.SeriesGatherDesc(**f)), None), lib.satcv_last_error()

    assert lib.satcv_series_gather(None, None) == -1
    for kw, msg in [(dict(src=None), b'null'), (dict(origins=None), b'null'), (dict(dst=None), b'null'), (dict(h=0), b'positive'), (dict(c=0), b'positive'),
                    (dict(side=0), b'positive'), (dict(n=0), b'positive'), (dict(off=-1), b'positive'), (dict(src_kind=0), b'src_kind'),
                    (dict(src_kind=4), b'src_kind'), (dict(src_kind=5), b'src_kind'), (dict(steps=0), b'steps'), (dict(steps=6), b'steps'),
                    (dict(maxval=0.0), b'maxval'), (dict(maxval=float('nan')), b'maxval'), (dict(dtype=_lib.FP8), b'dtype'), (dict(dtype=7), b'dtype'),
                    (dict(cpad=12), b'cpad'), (dict(cpad=0), b'cpad'), (dict(c=17), b'cpad'), (dict(dst=P + 8), b'aligned'),
                    (dict(first=1), b'origin table'), (dict(first=-1), b'origin table'), (dict(n=2 ** 20, total=2 ** 20, side=4096), b'2^31'),
                    (dict(h=2 ** 16, w_=2 ** 16), b'2^31')]:
        rc, err = gather(**kw)
        assert rc == -1 and msg in err, (kw, err)
    with pytest.raises(_lib.SatcvError):
        _lib.check(gather(steps=0)[0])
