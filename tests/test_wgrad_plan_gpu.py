"""Weight-gradient kernels of csrc/conv_wgrad.hip, one test per entry of tests/wgrad_cases.py: every template instantiation the planner
can choose, at a whole-tile, a ragged and a several-images-per-tile shape, and every cross-cutting feature on each kernel template.

Per case
  * the plan query (satcv_conv2d_wgrad_plan_info) says the intended instantiation is the one about to run;
  * Gaussian data, pre-rounded to the storage type, against the float64 oracle (oracle.keras_ops.conv2d_same_bwd /
    conv2d_transpose_ks_bwd) under the rule of tests/test_ops_gpu.py: close() with k = 5 (fp32) / 0.5 (bf16), twice that where the
    loader's affine rounds the staged tile;
  * integer-lattice data, BIT-EXACT: x, dy and the accumulate base are integers in [-4, 4], the affine's scale is from {1, 2, -1, 0.5} and
    its shift an integer, so every product and every partial sum is an integer (a half-integer with the 0.5 scale) far below 2^24
    (asserted from the shape, wgrad_cases.lattice_bound) -- fp32 sums of such numbers are exact in ANY order, whatever the slab count,
    the slab-sum kernel and defer_reduce.  dW must equal the exact reference with np.array_equal.  The zero tolerance is derived, not
    measured.  Stored channels beyond cin / cout carry nonzero lattice values and the workspace is filled with NaN before every launch,
    so that a leak of padding or of an unwritten slab shows;
  * two runs are torch.equal (fixed summation order).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import wgrad_cases as W  # noqa: E402
from oracle import keras_ops as K  # noqa: E402
from test_ops_gpu import close  # noqa: E402  (the one tolerance rule of the op tests)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ops():
    from satellite_computervision_amd import ops as _ops
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _ops


@pytest.fixture
def case_options(request):
    """the in-process options of the case, restored afterwards (as force_db of tests/test_ops_gpu.py does)"""
    with W.options(request.param['opts']):
        yield request.param


def tdtype(c):
    return torch.bfloat16 if c['dtype'] == W.BF16 else torch.float32


def make_data(c, rng, lattice):
    """float64 arrays exactly representable in the storage type: x (n, h, w, c0 + c1), dy (n, hf, wf, lddy), scale / shift (c0 + c1) or None,
    accumulate base (dW's shape) or None"""
    td, f = tdtype(c), max(c['f'], 1)
    cs = c['c0'] + c['c1']
    xs, ds = (c['n'], c['h'], c['w'], cs), (c['n'], c['h'] * f, c['w'] * f, c['lddy'])
    wshape = (f, f, c['cout'], c['cin']) if c['f'] else (c['k'], c['k'], c['cin'], c['cout'])
    if lattice:
        x, dy = rng.integers(-4, 5, xs).astype(np.float64), rng.integers(-4, 5, ds).astype(np.float64)
        sc = rng.choice([1.0, 2.0, -1.0, 0.5], cs) if c['affine'] else None
        sh = rng.integers(-3, 4, cs).astype(np.float64) if c['affine'] else None
        base = rng.integers(-4, 5, wshape).astype(np.float64) if c['accumulate'] else None
    else:
        r = lambda s: torch.tensor(rng.standard_normal(s), dtype=torch.float32).to(td).to(torch.float64).numpy()
        x, dy = r(xs), r(ds)
        sc = rng.standard_normal(cs).astype(np.float32).astype(np.float64) if c['affine'] else None
        sh = rng.standard_normal(cs).astype(np.float32).astype(np.float64) if c['affine'] else None
        base = rng.standard_normal(wshape).astype(np.float32).astype(np.float64) if c['accumulate'] else None
    return x, dy, sc, sh, base


def reference(c, x, dy, sc, sh, base):
    """float64 dW in the layout the library writes.  On lattice data every intermediate is a multiple of 1/2 below 2^53: exact."""
    td, cin, cout = tdtype(c), c['cin'], c['cout']
    a = x[..., :cin]
    if sc is not None:
        a = np.maximum(a * sc[:cin] + sh[:cin], 0)
        if td == torch.bfloat16:                      # the staged tile is stored in bf16 (the lattice values are representable: no change)
            a = torch.tensor(a, dtype=torch.float32).to(td).double().numpy()
    g = np.ascontiguousarray(dy[..., :cout])
    if c['f']:
        dk = K.conv2d_transpose_ks_bwd(a, np.zeros((c['f'], c['f'], cout, cin)), g)[1]
    else:
        dk = K.conv2d_same_bwd(a, np.zeros((c['k'], c['k'], cin, cout)), g, c['dil'])[1]
    return dk + base if base is not None else dk


def run(ops, c, x, dy, sc, sh, base):
    """one satcv_conv2d_wgrad of the case (plus the deferred slab sum where the case defers it); returns dW as a device tensor"""
    from satellite_computervision_amd._lib import lib, check, ReduceJob
    td, dev = tdtype(c), torch.device('cuda')
    up = lambda a: torch.tensor(a, dtype=torch.float32).to(td).to(dev).contiguous()
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()
    x0 = up(x[..., :c['c0']])
    x1 = up(x[..., c['c0']:]) if c['c1'] else None
    dyd = up(dy)
    scd, shd = (f32(sc), f32(sh)) if sc is not None else (None, None)
    f = c['f']
    wshape = (f, f, c['cout'], c['cin']) if f else (c['k'], c['k'], c['cin'], c['cout'])
    dw = f32(base) if base is not None else torch.full(wshape, float('nan'), dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    ptrs = dict(x0=p(x0), x1=p(x1), dy=p(dyd), dw=p(dw), in_scale=p(scd), in_shift=p(shd))
    d = W.make_desc(c, ptrs)
    nb = lib.satcv_conv2d_wgrad_workspace(C.byref(d))
    assert nb > 0, lib.satcv_last_error()
    ws = torch.full((nb // 4,), float('nan'), dtype=torch.float32, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nb
    got = W.plan_info(d)                               # with the real pointers: the form about to run
    assert got['key'] == c['key'] and bool(got['per_tap']) == c['per_tap'], (c['name'], got)
    check(lib.satcv_conv2d_wgrad(C.byref(d), ops.stream_ptr()))
    if c['defer_reduce']:
        job = ReduceJob()
        check(lib.satcv_conv2d_wgrad_reduce_job(C.byref(d), C.byref(job)))
        assert job.nslab == got['nsplit'] and job.kpad == got['kpad'] and job.npad == got['npad']
        total = int(lib.satcv_reduce_job_items(C.byref(job)))
        jd = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(dev)
        pd = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.satcv_reduce_slabs_batched(jd.data_ptr(), pd.data_ptr(), 1, total, ops.stream_ptr()))
    torch.cuda.synchronize()
    return dw, got


def check_case(ops, c):
    """every check of one case; returns the record line of profiles/wgrad_plan_parity.txt"""
    td = tdtype(c)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c['name'])) % 2**31
    # Gaussian parity
    data = make_data(c, np.random.default_rng(seed), lattice=False)
    dw, got = run(ops, c, *data)
    k = (5.0 if td == torch.float32 else 0.5) * (2.0 if c['affine'] else 1.0)
    err, tol = close(dw.double().cpu().numpy(), reference(c, *data), td, f"wgrad {c['name']}", k=k)
    dw2, _ = run(ops, c, *data)
    assert torch.equal(dw, dw2), f"{c['name']}: two runs differ"
    # integer lattice, bit-exact
    assert W.lattice_bound(c) < 2 ** 24 and 16 * c['n'] * c['h'] * c['w'] * (2 if c['affine'] else 1) < 2 ** 24
    data = make_data(c, np.random.default_rng(seed + 1), lattice=True)
    ref = reference(c, *data)
    assert np.array_equal(ref * 2, np.rint(ref * 2)) and np.abs(ref).max() * 2 <= W.lattice_bound(c)       # the reference is on the lattice
    dw, _ = run(ops, c, *data)
    g = dw.double().cpu().numpy()
    nbad = int((g != ref).sum())
    line = (f"WGRAD-PARITY {c['name']:42s} {'/'.join(str(v) for v in c['key']):34s} nsplit {got['nsplit']:3d} {got['reduce']:8s}"
            f"{' per-tap' if got['per_tap'] else ''} gauss {err:.2e} < {tol:.1e}  lattice {'exact' if nbad == 0 else 'NOT EXACT (%d of %d)' % (nbad, g.size)}")
    print(line)
    assert np.array_equal(g, ref), f"{c['name']}: {nbad} of {g.size} elements differ from the exact reference, max |diff| {np.nanmax(np.abs(g - ref))}"
    dw2, _ = run(ops, c, *data)
    assert torch.equal(dw, dw2), f"{c['name']}: two lattice runs differ"
    return line


@pytest.mark.parametrize('case_options', W.CASES, ids=[c['name'] for c in W.CASES], indirect=True)
def test_wgrad_case(ops, case_options):
    check_case(ops, case_options)


def child_main():
    """the startup-only cases, in a process started with their environment"""
    from satellite_computervision_amd import ops as _ops
    lines = []
    for c in W.STARTUP_CASES:
        with W.options(c['opts']):
            lines.append(check_case(_ops, c))
    print('CHILD-OK ' + json.dumps(lines))


def test_startup_option_cases_in_a_fresh_process():
    """wgrad_dma, wgrad_pix256 and wgrad_wgs are read once, when the library loads: their cases share ONE child process."""
    code = f'import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_wgrad_plan_gpu as T; T.child_main()'
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **W.startup_env(W.STARTUP_OPTS)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith('CHILD-OK '), r.stdout[-2000:]
    lines = json.loads(last[len('CHILD-OK '):])
    assert len(lines) == len(W.STARTUP_CASES)
    print('\n'.join(lines))


def test_bench_table_is_what_the_engine_builds(ops, monkeypatch):
    """wgrad_cases.BENCH_LAUNCHES against the satcv_wgrad_desc structures engine.py builds for bench.py's workload (get_unet_model(2, 4),
    256 x 256, batch 64, bf16): the same launches in the same order -- shape, sources, taps / transposed factor, loader affine, accumulate,
    whole_chip -- and, with the engine's own pointers, the pinned kernel form, slab count and slab sum."""
    from satellite_computervision_amd import model_tools as mt
    made = []
    orig = ops.make_wgrad_desc

    def record(**kw):
        d = orig(**kw)
        made.append(d)
        return d
    monkeypatch.setattr(ops, 'make_wgrad_desc', record)
    mt.reset_uids()
    mt.set_seed(0)
    old, model = mt._DEFAULT_DTYPE, None
    mt.set_compute_dtype('bfloat16')
    try:
        model = mt.get_unet_model(2, 4)
        model.compile(optimizer=mt.Adam(9e-4), loss=lambda yt, yp: mt.weighted_categorical_crossentropy(yt, yp, [1.0, 20.0]))
        model._head_plan(W.BENCH_N, 256, 256, True)
        assert len(made) == len(W.BENCH_LAUNCHES) == 14, [(d.h, d.w_, d.c0, d.c1, d.cout) for d in made]
        for d, c in zip(made, W.BENCH_LAUNCHES):
            got = (d.n, d.h, d.w_, d.c0, d.c1, d.cin, d.cout, d.kh, d.kw, d.dil, d.f if d.mode_dy else 0, bool(d.in_scale), d.accumulate, d.whole_chip,
                   d.lddy, d.dtype)
            want = (c['n'], c['h'], c['w'], c['c0'], c['c1'], c['cin'], c['cout'], c['k'], c['k'], c['dil'], c['f'], c['affine'], int(c['accumulate']),
                    int(c['whole_chip']), c['lddy'], ops.BF16)
            assert got == want, (c['name'], got, want)
            g = W.plan_info(d)
            assert (g['key'], g['nsplit'], g['reduce']) == (c['key'], c['nsplit'], c['reduce']), (c['name'], g)
    finally:
        mt.set_compute_dtype(old)
        del model
        torch.cuda.empty_cache()
