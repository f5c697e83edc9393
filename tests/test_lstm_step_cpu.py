"""CPU side of the fused ConvLSTM2D step (csrc/convlstm_step.hip, lstm_infer.py): the gate-interleaved channel order, the declarations
of the new entry points, and the corner share of every seeded input set tests/test_lstm_step_gpu.py uses (float64 reference alone)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import lstm_kernels_oracle as O  # noqa: E402
import lstm_step_cases as SC  # noqa: E402


def _gate_order():
    from satellite_computervision_amd import lstm_infer
    return lstm_infer.gate_order


@pytest.mark.parametrize('F', [16, 32, 64])
def test_gate_order_is_a_permutation_with_the_documented_layout(F):
    perm = _gate_order()(F)
    assert perm.shape == (4 * F,) and np.array_equal(np.sort(perm), np.arange(4 * F))
    G = min(F, 32)
    for blk in range(F // G):
        for gate in range(4):
            for j in (0, G - 1):
                assert perm[blk * 4 * G + gate * G + j] == gate * F + blk * G + j
    # the four gates of a filter sit G positions apart inside one block of 4 G: 32 MFMA columns apart for F >= 32
    inv = np.argsort(perm)
    for f in (0, F - 1):
        pos = inv[[g * F + f for g in range(4)]]
        assert np.array_equal(np.diff(pos), [G, G, G]) and pos[0] // (4 * G) == pos[3] // (4 * G)
    assert np.array_equal(_gate_order()(F, group=F), _gate_order()(F, F))
    with pytest.raises(ValueError):
        _gate_order()(F, group=F + 1)


@pytest.mark.parametrize('F', [16, 32, 64])
def test_permuted_kernel_unpermuted_output_is_the_natural_convolution(F):
    rng = np.random.default_rng(F)
    x = rng.standard_normal((2, 5, 7, F))
    k = rng.standard_normal((3, 3, F, 4 * F))
    b = rng.standard_normal(4 * F)
    perm = _gate_order()(F)
    nat = SC.conv3x3_same64(x, k) + b
    per = SC.conv3x3_same64(x, k[..., perm]) + b[perm]
    assert np.array_equal(per, nat) == (F <= 32)          # (one block of F <= 32 filters: the natural order already is the interleaved one)
    assert np.array_equal(per[..., np.argsort(perm)], nat)


def test_header_declares_and_lib_binds_the_new_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'satcv.h')).read()
    assert re.search(r'int\s+satcv_convlstm_step_fwd\s*\(\s*const\s+satcv_lstm_step_desc\s*\*', hdr)
    assert re.search(r'int\s+satcv_convlstm_step_supported\s*\(', hdr)
    assert 'typedef struct satcv_lstm_step_desc' in hdr and 'utils/model_tools.py:685-720' in hdr
    from satellite_computervision_amd import _lib
    assert hasattr(_lib.lib, 'satcv_convlstm_step_fwd') and hasattr(_lib.lib, 'satcv_convlstm_step_supported')
    fields = [f[0] for f in _lib.LstmStepDesc._fields_]
    body = hdr[hdr.index('typedef struct satcv_lstm_step_desc'):hdr.index('} satcv_lstm_step_desc;')]
    declared = re.findall(r'(\w+)\s*[;,]', body)
    assert fields == declared, (fields, declared)
    for F in (8, 16, 32, 48, 64, 128):
        assert _lib.lib.satcv_convlstm_step_supported(F, _lib.BF16) == (1 if F in (16, 32, 64) else 0)


def test_the_case_list_covers_what_the_gpu_file_promises():
    cs = SC.CASES
    assert len(set(cs)) == len(cs)
    assert {c[0] for c in cs} == {'f32', 'bf16'} and {c[3] for c in cs} == {16, 32, 64}
    for kind in ('f32', 'bf16'):
        for F in (16, 64):
            mine = [c for c in cs if c[0] == kind and c[3] == F]
            assert {(c[4], c[5]) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            assert any(c[6] for c in mine) and any((c[1], c[2]) == SC.RAGGED for c in mine) and any((c[1], c[2]) == SC.SMALL for c in mine)
    h, w = SC.RAGGED
    assert h > 2 * SC.TILE_H and h % SC.TILE_H and w > 2 * SC.TILE_W and w % SC.TILE_W
    assert SC.SMALL[0] < SC.TILE_H and SC.SMALL[1] < SC.TILE_W


@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_id)
def test_corner_share_of_every_gpu_input_set_is_below_one_per_cent(case):
    kind, h, w, F, rec, act, t0, pad = case
    ref = SC.reference(case)
    share = ref['corner'].mean()
    inside = (np.abs(ref['z']) < 2.5).mean()
    print(f'[fig] {SC.case_id(case)}: corner share {share:.4%}, |z| < 2.5 for {inside:.2%}, std z {ref["z"].std():.3f}')
    assert share < 0.01
    assert 0.5 < ref['z'].std() < 2.0 and inside > 0.95        # z of order 1, mostly inside the linear arm
    assert np.isfinite(ref['h64']).all() and np.ptp(ref['h64']) > 0
