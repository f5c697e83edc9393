"""bench.py's own contract: a plain run times exactly --steps steps and prints the headline line only; --dump-outputs writes what the
last timed step computed (same arguments -> same inputs -> same arrays); --full adds the per-class, repeated-region and roofline figures.
Each run is a fresh subprocess at a small batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--batch', '8'] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    outs, dumps = [], []
    for i in range(2):
        d = tmp_path / f'dump{i}'
        outs.append(_bench('--steps', '3', '--warmup', '2', '--dump-outputs', str(d)))
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    out = outs[0]
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in out, k
    assert out['steps'] == 3 and out['warmup'] == 2 and out['unit'] == 'tiles/s' and out['higher_is_better'] is True and out['dtype'] == 'bf16'
    assert abs(out['value'] - 8 * 3 / (out['ms_per_step'] * 3 / 1000)) / out['value'] < 1e-3
    assert 'roofline' not in out and 'cpu_baseline' not in out and 'kernel_ms_per_step' not in out['extra']
    a, b = dumps
    assert sorted(a) == ['loss.npy', 'weights.npy'], sorted(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert np.isfinite(a['loss.npy']).all() and np.isfinite(a['weights.npy']).all()
    assert a['loss.npy'][0] == np.float32(out['extra']['loss_last'])
    # training is bit-reproducible: identical arguments give identical weights.  The loss is a sum of per-workgroup partials whose
    # order is not fixed, so it agrees to float32 rounding
    assert np.array_equal(a['weights.npy'], b['weights.npy'])
    np.testing.assert_allclose(a['loss.npy'], b['loss.npy'], rtol=1e-5)


@pytest.mark.gpu
def test_full_bench_line_keeps_the_extra_figures():
    out = _bench('--steps', '2', '--warmup', '1', '--full', '--repeats', '2', '--no-infer', '--no-cpu-baseline')
    assert out['steps'] == 2 and out['value'] > 0
    assert out['extra']['region_ms_per_step']['repeats'] == 2
    assert out['roofline']['achieved'] > 0 and out['extra']['box_probe']['conv3x3_1024_512_16x16_us'] > 0
    assert set(out['extra']['kernel_ms_per_step']) == {'conv3x3_igemm_fwd_dgrad', 'conv1x1_convT_gemm', 'conv_wgrad', 'conv3x3_fused_dgrad_wgrad'}
