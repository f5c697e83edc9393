"""Host side of the Siamese inference path: the pair-store fields of satcv_conv_desc and two-date chip prediction with a stub model."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_conv_desc_pair_fields_follow_tile_policy():
    from satellite_computervision_amd._lib import ConvDesc
    names = [f[0] for f in ConvDesc._fields_]
    assert names[-4:] == ['tile_policy', 'pair_n', 'pair_c0', 'pair_c1']
    tp = ConvDesc.tile_policy.offset
    assert (ConvDesc.pair_n.offset, ConvDesc.pair_c0.offset, ConvDesc.pair_c1.offset) == (tp + 4, tp + 8, tp + 12)
    assert C.sizeof(ConvDesc) >= tp + 16
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    body = hdr[hdr.index('typedef struct satcv_conv_desc'):hdr.index('} satcv_conv_desc;')]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    assert re.search(r'int32_t tile_policy;\s*int32_t pair_n, pair_c0, pair_c1;\s*$', body)


def test_make_conv_desc_pair():
    from satellite_computervision_amd import ops
    d = ops.make_conv_desc(x0=None, c0=16, w=None, y=None, ldy=64, n=4, h=8, w_=8, cout=32, cout_pad=32, dtype=0, pair=(2, 32, 0))
    assert (d.pair_n, d.pair_c0, d.pair_c1) == (2, 32, 0)
    d = ops.make_conv_desc(x0=None, c0=16, w=None, y=None, ldy=64, n=4, h=8, w_=8, cout=32, cout_pad=32, dtype=0)
    assert (d.pair_n, d.pair_c0, d.pair_c1) == (0, 0, 0)


class _Stub:
    """records the batches it is asked for; 'probabilities' are a fixed function of both chips"""

    def __init__(self):
        self.calls = []

    def predict(self, x, batch_size=None, verbose=0):
        self.calls.append(x)
        a, b = x
        p = (a.sum(-1, keepdims=True) - 2 * b.sum(-1, keepdims=True)).astype(np.float32)
        return [p, (p > 0).astype(np.int32)]


def test_predict_chips_two_dates_with_stub():
    from satellite_computervision_amd import prediction_tools as pt
    rng = np.random.default_rng(0)
    a, b = rng.random((150, 170, 3)).astype(np.float32), rng.random((150, 170, 3)).astype(np.float32)
    kernel, buff = 32, 16
    idx = pt.generate_chip_indices(a, buff, kernel)
    m = _Stub()
    got = pt.predict_chips((a, b), idx, np.zeros((150, 170), np.float32), m, kernel=kernel, buff=buff, batch_size=4)
    assert len(m.calls) == -(-len(idx) // 4)
    hb = buff // 2
    k = 0
    ref = np.zeros((150, 170), np.float32)
    for call in m.calls:
        ca, cb = call
        assert ca.shape == cb.shape and ca.shape[1:] == (kernel + buff, kernel + buff, 3)
        for j in range(ca.shape[0]):
            y, x = idx[k]
            assert np.array_equal(ca[j], a[y - hb:y + kernel + hb, x - hb:x + kernel + hb])
            assert np.array_equal(cb[j], b[y - hb:y + kernel + hb, x - hb:x + kernel + hb])
            cen_a = a[y:y + kernel, x:x + kernel].sum(-1)
            cen_b = b[y:y + kernel, x:x + kernel].sum(-1)
            ref[y:y + kernel, x:x + kernel] += (cen_a - 2 * cen_b).astype(np.float32)
            k += 1
    assert k == len(idx)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5)


def test_predict_chips_two_dates_shape_mismatch():
    from satellite_computervision_amd import prediction_tools as pt
    a, b = np.zeros((100, 100, 3), np.float32), np.zeros((100, 96, 3), np.float32)
    with pytest.raises(ValueError):
        pt.predict_chips((a, b), [(16, 16)], np.zeros((100, 100), np.float32), _Stub(), kernel=32, buff=16)
    with pytest.raises(ValueError):
        pt.predict_chips_sharded((a, b), [(16, 16)], np.zeros((100, 100), np.float32), _Stub(), kernel=32, buff=16)
