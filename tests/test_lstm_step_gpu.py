"""Op-level parity of satcv_convlstm_step_fwd (csrc/convlstm_step.hip) through the C ABI against the float64 oracle of
tests/lstm_step_cases.py: two images (a halo leaking across the image boundary would show: h_prev is nonzero everywhere), a 5 x 7 plane
(smaller than the 8 x 16 tile) and a 19 x 37 one (3 x 3 tiles, ragged both ways), F = 16 and 64 and one case of 32 per storage type, both
storage types, both recurrent activations, the linear and the tanh cell, the t = 0 form (NULL h_prev / c_prev), leading dimensions wider
than needed with NaN / sentinel padding channels and a sentinel row behind every output, and the refusals.

Bounds (none tuned on the device): c and float32 h within close_tol(kind) of the output scale; bf16 h within the fp32 bound plus one
bf16 rounding of the float64 value (lstm_kernels_oracle.storage_bound, the rule tests/test_lstm_kernels_gpu.py states).  Elements with a
hard-sigmoid gate on a corner are set aside, under the 1 % cap tests/test_lstm_step_cpu.py holds.  Worst errors print as `[fig]` lines."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import lstm_kernels_oracle as O  # noqa: E402
import lstm_step_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
CODE = {'f32': 0, 'bf16': 1}
RAW = {4: torch.int32, 2: torch.int16}
SENT = -777.0


class _Env:
    def __getattr__(self, name):
        from satellite_computervision_amd import _lib, ops, lstm_infer
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
        self.lib, self.check, self.ops, self.Desc, self.gate_order = _lib.lib, _lib.check, ops, _lib.LstmStepDesc, lstm_infer.gate_order
        return self.__dict__[name]


E = _Env()


def dev(x64, kind):
    return torch.tensor(np.asarray(x64), dtype=torch.float32).to(TD[kind]).cuda().contiguous()


def host(t):
    return t.detach().cpu().to(torch.float64).numpy()


def raw(t):
    return t.detach().contiguous().view(RAW[t.element_size()]).cpu().numpy()


def wide(x64, kind, ld, fill):
    buf = np.full((x64.shape[0], ld), fill, np.float64)
    buf[:, :x64.shape[1]] = x64
    return dev(buf, kind)


def guarded(rows, ld, kind, extra=1):
    """sentinel-filled (rows + extra, ld) output buffer: the kernel owns channels [0, c) of the first `rows` rows"""
    return dev(np.full((rows + extra, ld), SENT), kind)


def only_wrote(t, before, rows, c):
    now = raw(t)
    return np.array_equal(now[rows:], before[rows:]) and np.array_equal(now[:rows, c:], before[:rows, c:])


def fig(what, err, tol):
    print(f'[fig] {what}: {err:.3e} (bound {tol:.1e})')


def build_call(case):
    """device buffers and the descriptor of one case -> (desc, dict of tensors kept alive)"""
    kind, h, w, F, rec, act, t0, pad = case
    inp = SC.inputs(case)
    npix = SC.N_IMG * h * w
    perm = E.gate_order(F)
    ldx, ldh, ldhp = 4 * F + pad, F + pad, F + 2 * pad
    keep = dict(xg=wide(inp['xg'][:, perm], kind, ldx, np.nan), c_out=guarded(npix, F, 'f32'), h_out=guarded(npix, ldh, kind))
    d = E.Desc()
    if not t0:
        keep['h_prev'] = wide(inp['h_prev'].reshape(npix, F), kind, ldhp, np.nan)
        keep['c_prev'] = dev(inp['c_prev'], 'f32')
        # the stored kernel, output channels permuted, packed as ops.pack_weights packs any forward kernel (the values are storage-exact)
        wk = torch.tensor(inp['wr'][..., perm], dtype=torch.float32).cuda().contiguous()
        keep['w'], _ = E.ops.pack_weights(wk, F, CODE[kind], want_dgrad=False)
        d.h_prev, d.ldh_prev, d.w, d.c_prev = keep['h_prev'].data_ptr(), ldhp, keep['w'].data_ptr(), keep['c_prev'].data_ptr()
    d.xg, d.ldx = keep['xg'].data_ptr(), ldx
    d.c_out, d.h_out, d.ldh = keep['c_out'].data_ptr(), keep['h_out'].data_ptr(), ldh
    d.n, d.h, d.w_, d.filters, d.rec_act, d.act, d.dtype = SC.N_IMG, h, w, F, rec, act, CODE[kind]
    return d, keep


@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_id)
def test_step_against_the_float64_oracle(case):
    kind, h, w, F, rec, act, t0, pad = case
    npix = SC.N_IMG * h * w
    ref = SC.reference(case)
    d, keep = build_call(case)
    before = {k: raw(keep[k]) for k in ('c_out', 'h_out')}
    E.check(E.lib.satcv_convlstm_step_fwd(C.byref(d), E.ops.stream_ptr()))
    torch.cuda.synchronize()
    assert only_wrote(keep['c_out'], before['c_out'], npix, F), 'c_out: something outside the owned region changed'
    assert only_wrote(keep['h_out'], before['h_out'], npix, F), 'h_out: something outside the owned region changed'
    ok = ~ref['corner']
    assert ok.mean() > 0.99
    c_got, h_got = host(keep['c_out'])[:npix], host(keep['h_out'])[:npix, :F]
    name = SC.case_id(case)
    # c (float32): close_tol(kind) relative to the output scale
    cscale = max(np.abs(ref['c64']).max(), 1e-6)
    cerr = (np.abs(c_got - ref['c64']) * ok).max() / cscale
    fig(f'{name} c', cerr, O.close_tol(kind))
    assert cerr < O.close_tol(kind)
    if kind == 'f32':
        hscale = max(np.abs(ref['h64']).max(), 1e-6)
        herr = (np.abs(h_got - ref['h64']) * ok).max() / hscale
        fig(f'{name} h', herr, O.close_tol('f32'))
        assert herr < O.close_tol('f32')
    else:
        frac = np.where(ok, np.abs(h_got - ref['h64']) / O.storage_bound(ref['h64'], 'bf16'), 0.0)
        fig(f'{name} h (fraction of fp32 bound + one bf16 rounding)', float(frac.max()), 1.0)
        assert frac.max() <= 1.0, f'{frac.max():.3f} of the bound at {np.unravel_index(frac.argmax(), frac.shape)}'
    # the elements set aside are still finite and close in the loose sense (a corner moves a gate by one rounding, not more)
    assert np.isfinite(c_got).all() and np.isfinite(h_got).all()


REFUSE_CASE = ('bf16', 5, 7, 16, 0, 0, False, 8)


def _refused(mutate, what):
    assert REFUSE_CASE in SC.CASES
    d, keep = build_call(REFUSE_CASE)
    outs = [(keep[k], raw(keep[k])) for k in ('c_out', 'h_out')]
    mutate(d, keep)
    rc = E.lib.satcv_convlstm_step_fwd(C.byref(d), E.ops.stream_ptr())
    torch.cuda.synchronize()
    msg = E.lib.satcv_last_error().decode()
    assert rc != 0, f'{what}: the call should have been refused'
    assert 'convlstm_step_fwd' in msg, msg
    for t, b in outs:
        assert np.array_equal(raw(t), b), f'{what}: a refused call wrote to an output'
    return msg


def test_refuses_aliased_buffers():
    def h_alias(d, keep):
        d.h_out, d.ldh = d.h_prev, d.ldh_prev
    assert 'h_out aliases h_prev' in _refused(h_alias, 'h alias')

    def h_overlap(d, keep):                        # a partial overlap is an alias too
        d.h_out, d.ldh = d.h_prev + 64, d.ldh_prev
    assert 'h_out aliases h_prev' in _refused(h_overlap, 'h overlap')

    def c_alias(d, keep):
        d.c_out = d.c_prev
    assert 'c_out aliases c_prev' in _refused(c_alias, 'c alias')


@pytest.mark.parametrize('field,value', [('ldx', 4 * 16 - 8), ('ldh', 8), ('ldh_prev', 8), ('ldx', 4 * 16 + 4)])
def test_refuses_bad_leading_dimensions(field, value):
    def mut(d, keep):
        setattr(d, field, value)
    assert 'leading dimension' in _refused(mut, field)


@pytest.mark.parametrize('F', [8, 24, 48, 128])
def test_refuses_filter_counts_it_was_not_built_for(F):
    def mut(d, keep):
        d.filters = F
    assert 'filters' in _refused(mut, f'F = {F}')


def test_refuses_bad_dtype_and_null_outputs():
    def dt(d, keep):
        d.dtype = 5
    _refused(dt, 'dtype')

    def nul(d, keep):
        d.c_out = None
    _refused(nul, 'null c_out')
