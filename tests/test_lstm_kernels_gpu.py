"""Op-level parity of the ConvLSTM cell and small dense-head kernels (csrc/convlstm.hip) through the C ABI against the float64
restatements of tests/lstm_kernels_oracle.py: every filter count the entry points take, both recurrent activations, the linear and the
tanh cell, the t = 0 forms (NULL hg / c_prev / dc_next), one and two dh sources, leading dimensions wider than needed, work past the
launch caps, all three kernels of the dense backward, nearest resizes that upsample and downsample by integer and non-integer ratios
(including 14 -> 23 and 26 -> 11, where the float32 index map of the kernel and exact integer arithmetic differ), and the argument
checks (error code, satcv_last_error naming the entry point, outputs untouched).  Every output sits in a buffer padded with a sentinel.

Bounds (none tuned on the device): bit-exact where the kernel copies or selects; the op-level close() bounds of tests/test_ops_gpu.py
(2e-5 fp32, 1.2e-2 bf16, relative to the output scale); for a float32 result stored as bf16 the fp32 bound plus ONE bf16 rounding of
the float64 value; for float sums in any order the derived (n - 1) 2^-24 sum|terms|.  Elements whose float64 value sits on a corner
(hard sigmoid at 0 / 1, ReLU at 0 / max_value, softmax ties) are set aside, under a 1 % cap that tests/test_lstm_kernels_cpu.py holds
for the reference alone.  Every toleranced check prints its worst error as a `[fig]` line (pytest -rP)."""
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

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
CODE = {'f32': 0, 'bf16': 1}
RAW = {4: torch.int32, 2: torch.int16, 8: torch.int64}
KINDS = ['f32', 'bf16']
FILTERS = [8, 16, 64, 256]
SENT = -777.0


class _Env:
    def __getattr__(self, name):
        from satellite_computervision_amd import _lib, ops
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
        self.lib, self.check, self.st = _lib.lib, _lib.check, ops.stream_ptr()
        self.GatesDesc, self.DenseDesc = _lib.LstmGatesDesc, _lib.DenseDesc
        return self.__dict__[name]


E = _Env()


def sync():
    torch.cuda.synchronize()


def dev(x64, kind):
    return torch.tensor(np.asarray(x64), dtype=torch.float32).to(TD[kind]).cuda().contiguous()


def f32dev(x):
    return torch.tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous()


def host(t):
    return t.detach().cpu().to(torch.float64).numpy()


def raw(t):
    return t.detach().contiguous().view(RAW[t.element_size()]).cpu().numpy()


def wide(x64, kind, ld, fill):
    """(rows, c) -> device (rows, ld) of the storage type holding x at channels [0, c) and `fill` in the others"""
    buf = np.full((x64.shape[0], ld), fill, np.float64)
    buf[:, :x64.shape[1]] = x64
    return dev(buf, kind)


def guarded(rows, ld, kind, extra=1):
    """sentinel-filled (rows + extra, ld) output buffer: the kernel owns channels [0, c) of the first `rows` rows"""
    return dev(np.full((rows + extra, ld), SENT), kind)


def only_wrote(t, before, rows, c):
    """nothing outside [0, rows) x [0, c) changed"""
    now = raw(t)
    return np.array_equal(now[rows:], before[rows:]) and np.array_equal(now[:rows, c:], before[:rows, c:])


def fig(what, err, tol):
    print(f'[fig] {what}: {err:.3e} (bound {tol:.1e})')


def close(got, ref, kind, what):
    err, _ = O.close_err(got, ref)
    tol = O.close_tol(kind)
    fig(what, err, tol)
    assert err < tol, f'{what}: rel-to-max err {err:.3e} >= {tol:.1e}'


def within(got, ref, bound, what, keep=None):
    """|got - ref| <= bound element-wise (over the elements of `keep`); prints the worst fraction of the bound"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    frac = err / np.maximum(bound, 1e-300)
    if keep is not None:
        frac = np.where(keep, frac, 0.0)
    fig(what + ' (fraction of the derived bound)', float(frac.max()), 1.0)
    assert frac.max() <= 1.0, f'{what}: {frac.max():.3f} of the bound at {np.unravel_index(frac.argmax(), frac.shape)}'


def refused(rc, name, outs):
    """error code, the message names the entry point, no output changed.  outs: [(tensor, raw before)]"""
    assert rc != 0, 'the call should have been refused'
    assert name in E.lib.satcv_last_error().decode(), E.lib.satcv_last_error().decode()
    sync()
    for t, before in outs:
        assert np.array_equal(raw(t), before), 'a refused call wrote to an output'


# ---------------------------------------------------------------------------- ingest
INGEST_SHAPES = [(2, 3, 5, 7, 3, 16), (1, 1, 4, 4, 8, 8), (3, 2, 3, 3, 13, 32), (2, 3, 300, 301, 3, 8)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', INGEST_SHAPES)
def test_ingest_seq(kind, shape):
    b, t, h, w, c, cpad = shape
    if h == 300:
        assert b * t * h * w * (cpad // 8) > O.LSTM_CAP_ITEMS                     # a second trip of the grid-stride loop
    src = np.random.default_rng(sum(shape)).standard_normal((b, t, h, w, c)).astype(np.float32)
    rows = t * b * h * w
    out = guarded(rows, cpad, kind)
    before = raw(out)
    srcd = f32dev(src)
    E.check(E.lib.satcv_ingest_seq(srcd.data_ptr(), out.data_ptr(), b, t, h, w, c, cpad, CODE[kind], E.st))
    sync()
    assert np.array_equal(host(out)[:rows], O.ingest_seq(src, cpad, kind).reshape(rows, cpad)), f'ingest_seq {kind} {shape}'
    assert not raw(out)[:rows, c:].any(), 'pad channels are exactly zero'
    assert only_wrote(out, before, rows, cpad)


def test_ingest_seq_refuses_bad_arguments():
    src, out = f32dev(np.ones((2 * 4 * 4 * 13,))), guarded(32, 16, 'f32')
    before = raw(out)
    for c, cpad, dt in ((13, 8, 0), (13, 12, 0), (0, 16, 0), (13, 16, 5)):
        refused(E.lib.satcv_ingest_seq(src.data_ptr(), out.data_ptr(), 1, 2, 4, 4, c, cpad, dt, E.st), 'ingest_seq', [(out, before)])


# ------------------------------------------------------------------------- gates fwd
def gates_fwd_call(kind, inp, f, rec_kind, act_kind, pad, with_gates, with_stats, launches=1, mutate=None):
    """-> dict of device outputs and their `before` images; pad: extra channels of every leading dimension"""
    npix = inp['xg'].shape[0]
    ldx, ldh_g, ldh, sld = 4 * f + pad, 4 * f + 2 * pad, f + pad, f + pad
    xg = wide(inp['xg'], kind, ldx, np.nan)
    hg = wide(inp['hg'], kind, ldh_g, np.nan) if inp['hg'] is not None else None
    cp = f32dev(inp['c_prev']) if inp['c_prev'] is not None else None
    c_out, h_out, gates = guarded(npix, f, 'f32'), guarded(npix, ldh, kind), guarded(npix, 4 * f, kind)
    stats = torch.zeros((O.STAT_ROWS, 2, sld), dtype=torch.float64, device='cuda')
    stats[:, :, f:] = SENT
    d = E.GatesDesc()
    d.xg, d.ldx = xg.data_ptr(), ldx
    d.hg, d.ldh_g = (hg.data_ptr(), ldh_g) if hg is not None else (None, 0)
    d.c_prev = cp.data_ptr() if cp is not None else None
    d.c_out, d.h_out, d.ldh = c_out.data_ptr(), h_out.data_ptr(), ldh
    d.gates_out = gates.data_ptr() if with_gates else None
    if with_stats:
        d.stats, d.stats_ld = stats.data_ptr(), sld
    d.npix, d.filters, d.rec_act, d.act, d.dtype = npix, f, rec_kind, act_kind, CODE[kind]
    outs = [(t, raw(t)) for t in (c_out, h_out, gates, stats)]
    if mutate is not None:
        mutate(d)
        return E.lib.satcv_convlstm_gates_fwd(C.byref(d), E.st), outs
    for _ in range(launches):
        E.check(E.lib.satcv_convlstm_gates_fwd(C.byref(d), E.st))
    sync()
    assert only_wrote(c_out, outs[0][1], npix, f) and only_wrote(h_out, outs[1][1], npix, f), 'gates_fwd wrote outside c / h'
    assert only_wrote(gates, outs[2][1], npix if with_gates else 0, 4 * f), 'gates_fwd wrote outside gates_out'
    assert (stats[:, :, f:] == SENT).all().item() and (with_stats or not stats[:, :, :f].any().item()), 'gates_fwd wrote outside its statistics'
    return dict(c=host(c_out)[:npix], h=host(h_out)[:npix, :f], gates=host(gates)[:npix], stats=stats[:, :, :f].sum(0).cpu().numpy(),
                c_dev=c_out, gates_dev=gates)


def check_gates_fwd(kind, npix, f, rec_kind, act_kind, forms):
    for t0, pad, with_gates, with_stats in forms:
        inp = O.cell_inputs(kind, npix, f, seed=f + npix + rec_kind, t0=t0)
        ref = O.gates_fwd(inp['xg'], inp['hg'], inp['c_prev'], rec_kind, act_kind, kind)
        got = gates_fwd_call(kind, inp, f, rec_kind, act_kind, pad, with_gates, with_stats, launches=2 if with_stats else 1)
        tag = f'gates_fwd {kind} npix={npix} F={f} rec={rec_kind} act={act_kind} t0={t0} pad={pad}'
        assert not np.isnan(got['c']).any() and not np.isnan(got['h']).any(), 'NaN: a read outside the input slices'
        close(got['c'], ref['c64'], 'f32', tag + ' c')
        within(got['h'], ref['h64'], O.storage_bound(ref['h64'], kind), tag + ' h')
        if with_gates:
            within(got['gates'], ref['gates64'], O.storage_bound(ref['gates64'], kind), tag + ' gates')
        if with_stats:                                        # of the stored h THE KERNEL wrote; two launches accumulate
            hk = got['h']
            for row, v in ((0, hk), (1, hk * hk)):
                within(got['stats'][row], 2.0 * v.sum(0), 2.0 * O.stat_bound(v) + 1e-300, tag + f' stats row {row}')


FWD_FORMS = [(False, 8, True, True), (True, 0, False, False), (False, 0, True, False)]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('f', FILTERS)
@pytest.mark.parametrize('rec_kind', [0, 1])
@pytest.mark.parametrize('act_kind', [0, 1])
def test_gates_fwd(kind, f, rec_kind, act_kind):
    check_gates_fwd(kind, 3 * 5 * 7, f, rec_kind, act_kind, FWD_FORMS)


@pytest.mark.parametrize('kind', KINDS)
def test_gates_fwd_past_the_launch_cap(kind):
    npix, f = 66001, 64
    assert npix * f // 8 > O.LSTM_CAP_ITEMS
    check_gates_fwd(kind, npix, f, 0, 1, FWD_FORMS[:1])


def test_gates_fwd_refuses_bad_arguments():
    inp = O.cell_inputs('f32', 16, 64, seed=1)

    def setter(**kw):
        return lambda d: [setattr(d, k, v) for k, v in kw.items()]
    for m in (setter(filters=24), setter(filters=512), setter(ldx=4 * 64 - 8), setter(stats_ld=56), setter(dtype=2), setter(ldh=56)):
        rc, outs = gates_fwd_call('f32', inp, 64, 0, 0, 8, True, True, mutate=m)
        refused(rc, 'lstm_gates_fwd', outs)


# ------------------------------------------------------------------------- gates bwd
def gates_bwd_call(kind, f, gates, c, c_prev, dc_next, dh_a, dh_b, rec_kind, act_kind, pad, mutate=None, gates_dev=None, c_dev=None):
    npix = gates.shape[0] if gates is not None else gates_dev.shape[0] - 1
    lda, ldb, lddz = f + pad, f + 2 * pad, 4 * f + pad
    keep = [wide(dh_a, kind, lda, np.nan) if dh_a is not None else None, wide(dh_b, kind, ldb, np.nan) if dh_b is not None else None,
            dev(gates, kind) if gates_dev is None else gates_dev, f32dev(c) if c_dev is None else c_dev,
            f32dev(c_prev) if c_prev is not None else None, f32dev(dc_next) if dc_next is not None else None]
    dz, dcp = guarded(npix, lddz, kind), guarded(npix, f, 'f32')
    d = E.GatesDesc()
    if keep[0] is not None:
        d.dh_a, d.lddh_a = keep[0].data_ptr(), lda
    if keep[1] is not None:
        d.dh_b, d.lddh_b = keep[1].data_ptr(), ldb
    d.gates_out, d.c_out = keep[2].data_ptr(), keep[3].data_ptr()
    d.c_prev = keep[4].data_ptr() if keep[4] is not None else None
    d.dc_next = keep[5].data_ptr() if keep[5] is not None else None
    d.dz_out, d.lddz, d.dc_prev_out = dz.data_ptr(), lddz, dcp.data_ptr()
    d.npix, d.filters, d.rec_act, d.act, d.dtype = npix, f, rec_kind, act_kind, CODE[kind]
    outs = [(dz, raw(dz)), (dcp, raw(dcp))]
    if mutate is not None:
        mutate(d)
        return E.lib.satcv_convlstm_gates_bwd(C.byref(d), E.st), outs
    E.check(E.lib.satcv_convlstm_gates_bwd(C.byref(d), E.st))
    sync()
    assert only_wrote(dz, outs[0][1], npix, 4 * f) and only_wrote(dcp, outs[1][1], npix, f), 'gates_bwd wrote outside dz / dc_prev'
    return host(dz)[:npix, :4 * f], host(dcp)[:npix]


BWD_FORMS = [('ab', False, 8), ('a', True, 0), ('b', False, 0)]         # (dh sources, t0: c_prev and dc_next NULL, pad)


def check_gates_bwd(kind, npix, f, rec_kind, act_kind, forms):
    for which, t0, pad in forms:
        inp = O.cell_inputs(kind, npix, f, seed=2 * f + npix + act_kind, t0=t0)
        fw = O.gates_fwd(inp['xg'], inp['hg'], inp['c_prev'], rec_kind, act_kind, kind)         # realistic STORED gates, exact 0 / 1 among them
        dh_a, dh_b = (inp['dh_a'] if 'a' in which else None), (inp['dh_b'] if 'b' in which else None)
        dcn = None if t0 else inp['dc_next']
        dz_ref, dcp_ref = O.gates_bwd(dh_a, dh_b, dcn, fw['gates'], inp['c_prev'], fw['c'], rec_kind, act_kind)
        dz, dcp = gates_bwd_call(kind, f, fw['gates'], fw['c'], inp['c_prev'], dcn, dh_a, dh_b, rec_kind, act_kind, pad)
        tag = f'gates_bwd {kind} npix={npix} F={f} rec={rec_kind} act={act_kind} dh={which} t0={t0}'
        assert not np.isnan(dz).any() and not np.isnan(dcp).any(), 'NaN: a read outside the input slices'
        within(dz, dz_ref, O.storage_bound(dz_ref, kind), tag + ' dz')
        close(dcp, dcp_ref, 'f32', tag + ' dc_prev')
        if rec_kind == 0:
            assert (fw['gates'][:, :2 * f] == 0).any() and (fw['gates'][:, :2 * f] == 1).any(), 'the clipped arms must occur'


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('f', FILTERS)
@pytest.mark.parametrize('rec_kind', [0, 1])
@pytest.mark.parametrize('act_kind', [0, 1])
def test_gates_bwd(kind, f, rec_kind, act_kind):
    check_gates_bwd(kind, 3 * 5 * 7, f, rec_kind, act_kind, BWD_FORMS)


@pytest.mark.parametrize('kind', KINDS)
def test_gates_bwd_past_the_launch_cap(kind):
    check_gates_bwd(kind, 66001, 64, 0, 1, BWD_FORMS[:1])


@pytest.mark.parametrize('kind', KINDS)
def test_gates_bwd_hard_sigmoid_slope_at_the_ends(kind):
    """hand-placed stored gates: exactly 0 and 1 (slope 0), their nearest neighbours inside (0, 1) in the storage type (slope 0.2), -0 and the
    neighbour above 1 (slope 0).  Launch 1: dh = 0, dc_next = c_prev = g = 1 -> di = slope(i), df = slope(f); launch 2: dh = c = 1 ->
    do = slope(o); each exactly 0 or the stored float32(0.2)."""
    if kind == 'f32':
        tiny, below, above = float(np.nextafter(np.float32(0), np.float32(1))), float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2)))
    else:
        tiny, below, above = 2.0 ** -133, 1.0 - 2.0 ** -8, 1.0 + 2.0 ** -7
    vals = np.array([0.0, -0.0, tiny, 0.5, below, 1.0, above])
    expect = np.array([0.0, 0.0, 0.2, 0.2, 0.2, 0.0, 0.0])
    f, npix = 8, len(vals)
    slope = O.to_storage(np.full(1, 0.2, np.float32), kind)[0]
    col = np.repeat(vals[:, None], f, 1)
    one, zero = np.ones((npix, f)), np.zeros((npix, f))
    gates = np.concatenate([col, col, one, col], -1)
    gd = dev(gates, kind)
    assert np.array_equal(host(gd), gates), 'the hand-placed gate values survive the trip to the device'
    dz, _ = gates_bwd_call(kind, f, gates, one, one, one, zero, None, 0, 0, 0)
    want = np.repeat((expect / 0.2 * slope)[:, None], f, 1)
    assert np.array_equal(dz[:, :f], want) and np.array_equal(dz[:, f:2 * f], want), f'slopes of i / f from the stored value: {dz[:, 0]} {dz[:, f]}'
    dz, _ = gates_bwd_call(kind, f, gates, one, one, None, None, one, 0, 0, 0)
    assert np.array_equal(dz[:, 3 * f:], want), f'slope of o from the stored value: {dz[:, 3 * f]}'


def test_gates_bwd_refuses_bad_arguments():
    inp = O.cell_inputs('f32', 16, 64, seed=1)
    fw = O.gates_fwd(inp['xg'], inp['hg'], inp['c_prev'], 0, 0, 'f32')

    def setter(**kw):
        return lambda d: [setattr(d, k, v) for k, v in kw.items()]
    for m in (setter(lddh_a=56), setter(lddh_b=56), setter(filters=512), setter(filters=24), setter(lddz=4 * 64 - 8), setter(dtype=2),
              setter(dh_a=None, dh_b=None)):
        rc, outs = gates_bwd_call('f32', 64, fw['gates'], fw['c'], inp['c_prev'], inp['dc_next'], inp['dh_a'], inp['dh_b'], 0, 0, 8, mutate=m)
        refused(rc, 'lstm_gates_bwd', outs)


# -------------------------------------------------------------------- composed cell
@pytest.mark.parametrize('case', O.COMPOSED, ids=lambda c: c[0])
def test_cell_forward_then_backward_against_the_float64_cell(case):
    """gates_fwd, then gates_bwd on what it stored, against the float64 cell differentiated from its pre-activations.  The kernel takes
    the hard-sigmoid slope from the STORED gate; the elements where that can differ from the pre-activation rule (the float64 value within
    one storage rounding of 0 or 1) are set aside.  bf16: a dz element is a product with at most two rounded gates and is rounded once
    more when stored -- three bf16 roundings of 2^-8 each, 1.17e-2, inside the 1.2e-2 op-level bound."""
    kind, npix, f, rec_kind, act_kind, seed = case
    inp = O.cell_inputs(kind, npix, f, seed)
    z = inp['xg'] + inp['hg']
    fwd = gates_fwd_call(kind, inp, f, rec_kind, act_kind, 0, True, False)
    dz, dcp = gates_bwd_call(kind, f, None, None, inp['c_prev'], inp['dc_next'], inp['dh_a'], inp['dh_b'], rec_kind, act_kind, 8,
                             gates_dev=fwd['gates_dev'], c_dev=fwd['c_dev'])
    dz_ref, dcp_ref = O.gates_bwd_from_z(inp['dh_a'] + inp['dh_b'], inp['dc_next'], z, inp['c_prev'], rec_kind, act_kind)
    amb = O.composed_ambiguous(z, kind)
    fig(f'composed cell {case}: share of dz elements set aside', float(amb.mean()), 0.01)
    assert amb.mean() < 0.01
    tol = O.close_tol(kind) * max(np.abs(dz_ref).max(), 1e-6)
    within(dz, dz_ref, np.full(dz.shape, tol), f'composed cell {case} dz', keep=~amb)
    close(dcp, dcp_ref, kind, f'composed cell {case} dc_prev')


# ----------------------------------------------------------------------- dense heads
def dense_desc(srcs, meta, w, b, cout, act, mx, h, w_):
    """-> (desc, keep-alive list).  Sources go to the device with NaN in the channels [cin, ld)"""
    d, keep = E.DenseDesc(), []
    d.nsrc = len(srcs)
    for i, (s, (kind, ld)) in enumerate(zip(srcs, meta)):
        cin = s.x.shape[-1]
        xd = wide(s.x.reshape(-1, cin), kind, ld, np.nan)
        keep.append(xd)
        ds = d.src[i]
        ds.x, ds.ld, ds.cin, ds.dtype = xd.data_ptr(), ld, cin, CODE[kind]
        if s.scale is not None:
            scd, shd = f32dev(s.scale), f32dev(s.shift)
            keep += [scd, shd]
            ds.in_scale, ds.in_shift, ds.in_relu = scd.data_ptr(), shd.data_ptr(), 1 if s.relu else 0
        if s.resized:
            ds.hs, ds.ws = s.x.shape[1], s.x.shape[2]
    wd, bd = f32dev(w), f32dev(b)
    keep += [wd, bd]
    d.w, d.b, d.cout, d.activation, d.max_value = wd.data_ptr(), bd.data_ptr(), cout, act, mx
    d.h, d.w_, d.npix = h, w_, srcs[0].x.shape[0] * h * w_
    return d, keep


def dense_fwd_call(d, with_extras):
    npix, k = d.npix, d.cout
    out, z = guarded(npix, k, 'f32'), guarded(npix, k, 'f32')
    cls = torch.full((npix + 8,), -5, dtype=torch.int32, device='cuda')
    before = [raw(out), raw(z)]
    d.out = out.data_ptr()
    d.z_out, d.classes = (z.data_ptr(), cls.data_ptr()) if with_extras else (None, None)
    E.check(E.lib.satcv_dense_small_fwd(C.byref(d), E.st))
    sync()
    assert only_wrote(out, before[0], npix, k) and only_wrote(z, before[1], npix if with_extras else 0, k), 'dense_small_fwd wrote outside out / z_out'
    wrote_cls = with_extras and d.activation == 0
    assert (cls[npix:] == -5).all().item() and (wrote_cls or (cls == -5).all().item())
    return host(out)[:npix], host(z)[:npix], cls[:npix].cpu().numpy(), out


@pytest.mark.parametrize('case,pair,nimg,seed', list(O.dense_gpu_cases()), ids=lambda v: v[0] if isinstance(v, tuple) and isinstance(v[0], str) else str(v))
def test_dense_small_fwd(case, pair, nimg, seed):
    name, cout, act, mx, specs = case
    h, w_ = pair[2], pair[3]
    srcs, meta, w, b = O.dense_inputs(case, pair, nimg, seed)
    z_ref, out_ref, cls_ref, margin = O.dense_fwd(srcs, w, b, act, mx, h, w_, 'tf32')
    d, keep = dense_desc(srcs, meta, w, b, cout, act, mx, h, w_)
    out, z, cls, _ = dense_fwd_call(d, True)
    tag = f'dense_small_fwd {name} cout={cout} {pair}'
    assert not np.isnan(out).any(), 'NaN: a read outside a source slice'
    close(z, z_ref, 'f32', tag + ' z')
    close(out, out_ref, 'f32', tag + ' out')
    if act == 0:
        sure = margin > O.close_tol('f32')
        fig(tag + ' share of pixels left out of the class comparison', 1.0 - sure.mean(), 0.01)
        assert 1.0 - sure.mean() < 0.01 and np.array_equal(cls[sure], cls_ref[sure])
    out2, _, _, _ = dense_fwd_call(d, False)
    assert np.array_equal(out2, out), 'z_out / classes change the output'
    if any(s.resized for s in srcs) and not (O.nn_forms_agree(pair[0], pair[2]) and O.nn_forms_agree(pair[1], pair[3])):
        wrong = O.dense_fwd(srcs, w, b, act, mx, h, w_, 'exact')[0]             # this test fails for a kernel that follows the exact index map
        assert O.close_err(wrong, z_ref)[0] > 10 * O.close_tol('f32')


def test_dense_small_fwd_argmax_of_equal_logits_is_the_first():
    s = O.Src(np.zeros((1, 3, 5, 8)))
    d, keep = dense_desc([s], [('f32', 8)], np.zeros((8, 4)), np.array([0.0, 1.0, 1.0, -1.0]), 4, 0, 0.0, 3, 5)
    _, _, cls, _ = dense_fwd_call(d, True)
    assert (cls == 1).all()


def check_dense_bwd(tag, srcs, meta, w, b, cout, act, mx, h, w_, dx_kinds, seed, with_dz=True):
    """dx_kinds: per source 'f32' / 'bf16' / None (no data gradient)"""
    rng = np.random.default_rng(seed)
    d, keep = dense_desc(srcs, meta, w, b, cout, act, mx, h, w_)
    npix, rows = d.npix, w.shape[0]
    dout = (rng.standard_normal((npix, cout))).astype(np.float32).astype(np.float64)
    out_dev = None
    if act == 3:                                                      # the mask comes from the forward output the KERNEL stored
        _, _, _, out_dev = dense_fwd_call(d, False)
        d.out = out_dev.data_ptr()
    pre_w, pre_b = rng.standard_normal((rows, cout)).astype(np.float32), rng.standard_normal(cout).astype(np.float32)
    dw, db = guarded(rows, cout, 'f32'), guarded(1, cout, 'f32')
    dw[:rows] = f32dev(pre_w)
    db[:1] = f32dev(pre_b[None])
    dz = guarded(npix, cout, 'f32')
    doutd = f32dev(dout)
    outs = [(dw, raw(dw)), (db, raw(db)), (dz, raw(dz))]
    dxs = []
    for i, (s, kind) in enumerate(zip(srcs, dx_kinds)):
        if kind is None:
            dxs.append(None)
            continue
        cin, n_src = s.x.shape[-1], int(np.prod(s.x.shape[:3]))
        t = guarded(n_src, cin + 8, kind)
        d.src[i].dx, d.src[i].lddx, d.src[i].dx_dtype = t.data_ptr(), cin + 8, CODE[kind]
        dxs.append((t, raw(t), n_src, cin))
    d.dout, d.dw, d.db = doutd.data_ptr(), dw.data_ptr(), db.data_ptr()
    d.dz_out = dz.data_ptr() if with_dz else None
    E.check(E.lib.satcv_dense_small_bwd(C.byref(d), E.st))
    sync()
    assert only_wrote(dw, outs[0][1], rows, cout) and only_wrote(db, outs[1][1], 1, cout) and only_wrote(dz, outs[2][1], npix if with_dz else 0, cout)
    z_ref, out_ref, _, _ = O.dense_fwd(srcs, w, b, act, mx, h, w_)
    dz_given = None
    if act == 3:
        amb = O.relu_ambiguous(z_ref, mx, O.close_tol('f32') * max(np.abs(z_ref).max(), 1e-6))
        fig(tag + ' share of outputs at a ReLU corner', float(amb.mean()), 0.01)
        assert amb.mean() < 0.01
        assert (z_ref <= 0).any() and (mx <= 0 or (z_ref >= mx).any()), 'both arms of the ReLU must occur'
        dz_given = dout * O.relu_mask(out_ref, mx)
        if with_dz and amb.any():                                     # at a corner either side is right: follow the kernel there
            dzk = host(dz)[:npix]
            assert ((dzk[amb] == 0) | (dzk[amb] == dout[amb])).all()
            dz_given[amb] = dzk[amb]
        elif amb.any():
            pytest.fail('a ReLU corner without dz_out: choose another seed')
    ref = O.dense_bwd(srcs, w, dout, out_ref, act, mx, h, w_, 'tf32', dz=dz_given)
    if with_dz:
        assert np.array_equal(host(dz)[:npix], ref['dz']), tag + ' dz_out'
    within(host(dw)[:rows] - pre_w, ref['dw'], O.sum_bound(npix, ref['dw_abs'], pre_w) + 1e-300, tag + ' dW')
    within(host(db)[0] - pre_b, ref['db'], O.sum_bound(npix, ref['db_abs'], pre_b) + 1e-300, tag + ' db')
    for i, e in enumerate(dxs):
        if e is None:
            continue
        t, before, n_src, cin = e
        assert only_wrote(t, before, n_src, cin), tag + f' dx of source {i} written outside its slice'
        close(host(t)[:n_src, :cin], ref['dx'][i].reshape(n_src, cin), dx_kinds[i], tag + f' dx[{i}] {dx_kinds[i]}')
    return d, keep


def plain_sources(rng, nimg, h, w_, specs):
    """specs: (cin, ld, kind, affine, relu)"""
    srcs, meta = [], []
    for cin, ld, kind, affine, relu in specs:
        x = O.to_storage(rng.standard_normal((nimg, h, w_, cin)).astype(np.float32), kind)
        sc, sh = (rng.uniform(0.5, 1.5, cin).astype(np.float32), (rng.standard_normal(cin) * 0.5).astype(np.float32)) if affine else (None, None)
        srcs.append(O.Src(x, sc, sh, relu))
        meta.append((kind, ld))
    return srcs, meta


def weights(rng, rows, cout, act):
    return (rng.standard_normal((rows, cout)) / np.sqrt(rows)).astype(np.float32), (rng.standard_normal(cout) * 0.5 + (1.0 if act == 3 else 0.0)).astype(np.float32)


@pytest.mark.parametrize('act,mx', [(2, 0.0), (3, 2.0), (3, 0.0)])
@pytest.mark.parametrize('dxk', KINDS)
def test_dense_small_bwd_lane_kernel_three_rows(act, mx, dxk):
    rng = np.random.default_rng(31)
    srcs, meta = plain_sources(rng, 2, 9, 11, [(3, 8, dxk, True, True)])
    w, b = weights(rng, 3, 3, act)
    check_dense_bwd(f'dense_small_bwd lane rows=3 act={act} max={mx} dx={dxk}', srcs, meta, w, b, 3, act, mx, 9, 11, [dxk], 32, with_dz=not (dxk == 'bf16' and act == 2))


@pytest.mark.parametrize('cout', [1, 16])
def test_dense_small_bwd_lane_kernel_past_its_block_cap(cout):
    """rows = 127: two pixel lanes of 128 threads, 32 pixels per workgroup, 1024 workgroups at the most -- 40200 pixels take a second trip"""
    rng = np.random.default_rng(33)
    nimg, h, w_ = 2, 100, 201
    assert nimg * h * w_ > O.DENSE_LANE_CAP_BLOCKS * 32
    srcs, meta = plain_sources(rng, nimg, h, w_, [(64, 72, 'bf16', True, True), (63, 64, 'f32', False, False)])
    w, b = weights(rng, 127, cout, 3)
    check_dense_bwd(f'dense_small_bwd lane rows=127 cout={cout}', srcs, meta, w, b, cout, 3, 2.0, h, w_, ['bf16', 'f32'], 34)


@pytest.mark.parametrize('act,mx', [(2, 0.0), (3, 2.0)])
def test_dense_small_bwd_wide_kernel(act, mx):
    rng = np.random.default_rng(35)
    srcs, meta = plain_sources(rng, 2, 9, 11, [(192, 200, 'bf16', True, True), (96, 96, 'f32', False, False)])
    w, b = weights(rng, 288, 3, act)
    check_dense_bwd(f'dense_small_bwd wide rows=288 act={act}', srcs, meta, w, b, 3, act, mx, 9, 11, ['bf16', 'f32'], 36)


@pytest.mark.parametrize('pair', O.RESIZE_PAIRS, ids=str)
@pytest.mark.parametrize('dxk', KINDS)
@pytest.mark.parametrize('act,mx', [(2, 0.0), (3, 2.0)])
def test_dense_small_bwd_gather_kernel(pair, dxk, act, mx):
    case = ('gather', 3, act, mx, [(8, 8, 'bf16', True, True, True), (5, 8, 'f32', False, False, False)])
    srcs, meta, w, b = O.dense_inputs(case, pair, 2, seed=40 + sum(pair))
    check_dense_bwd(f'dense_small_bwd gather {pair} act={act} dx={dxk}', srcs, meta, w, b, 3, act, mx, pair[2], pair[3], [dxk, None if dxk == 'bf16' else 'f32'], 41)
    if not O.nn_forms_agree(pair[0], pair[2]):
        dout = np.ones((2 * pair[2] * pair[3], 3))
        a, e = (O.dense_bwd(srcs, w, dout, None, 2, 0.0, pair[2], pair[3], form)['dx'][0] for form in ('tf32', 'exact'))
        assert O.close_err(e, a)[0] > 10 * O.close_tol(dxk)                      # a gather over the exact index map would fail above


def test_dense_small_bwd_both_sources_resized():
    case = ('gather2', 16, 2, 0.0, [(8, 16, 'f32', False, False, True), (5, 8, 'bf16', True, False, True)])
    srcs, meta, w, b = O.dense_inputs(case, (7, 7, 5, 5), 3, seed=50)
    check_dense_bwd('dense_small_bwd two resized sources', srcs, meta, w, b, 16, 2, 0.0, 5, 5, ['f32', 'bf16'], 51)


# ------------------------------------------------------------- refused dense calls
def _set(path, value):
    def m(d):
        obj = d
        for p in path[:-1]:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        setattr(obj, path[-1], value)
    return m


FWD_REFUSALS = {
    'in_scale without in_shift': _set(('src', 0, 'in_shift'), None),
    'in_shift without in_scale': _set(('src', 0, 'in_scale'), None),
    'activation 4': _set(('activation',), 4),
    'activation -1': _set(('activation',), -1),
}
BWD_REFUSALS = {
    'source x NULL': _set(('src', 1, 'x'), None),
    'cin 0': _set(('src', 0, 'cin'), 0),
    'ld < cin': _set(('src', 0, 'ld'), 4),
    'source dtype': _set(('src', 1, 'dtype'), 7),
    'hs without ws': _set(('src', 0, 'ws'), 0),
    'ws without hs': _set(('src', 1, 'ws'), 3),
    'h 0': _set(('h',), 0),
    'w 0': _set(('w_',), 0),
    'npix not whole images': _set(('npix',), 2 * 8 * 8 - 1),
    'lddx < cin': _set(('src', 1, 'lddx'), 4),
    'dx dtype': _set(('src', 0, 'dx_dtype'), 7),
    'in_scale without in_shift': _set(('src', 0, 'in_shift'), None),
    'activation 0': _set(('activation',), 0),
}


def refusal_setup():
    case = ('refuse', 3, 3, 2.0, [(8, 8, 'bf16', True, True, True), (5, 8, 'f32', False, False, False)])
    srcs, meta, w, b = O.dense_inputs(case, (4, 4, 8, 8), 2, seed=60)
    return dense_desc(srcs, meta, w, b, 3, 3, 2.0, 8, 8)


@pytest.mark.parametrize('what', list(FWD_REFUSALS))
def test_dense_small_fwd_refuses(what):
    d, keep = refusal_setup()
    out, z = guarded(d.npix, 3, 'f32'), guarded(d.npix, 3, 'f32')
    d.out, d.z_out = out.data_ptr(), z.data_ptr()
    outs = [(out, raw(out)), (z, raw(z))]
    FWD_REFUSALS[what](d)
    refused(E.lib.satcv_dense_small_fwd(C.byref(d), E.st), 'dense_small_fwd', outs)


@pytest.mark.parametrize('what', list(BWD_REFUSALS))
def test_dense_small_bwd_refuses(what):
    d, keep = refusal_setup()
    npix = d.npix
    out, dout = f32dev(np.ones((npix, 3))), f32dev(np.ones((npix, 3)))
    dw, db, dz = guarded(13, 3, 'f32'), guarded(1, 3, 'f32'), guarded(npix, 3, 'f32')
    dx0, dx1 = guarded(2 * 4 * 4, 8, 'bf16'), guarded(npix, 8, 'f32')
    d.out, d.dout, d.dw, d.db, d.dz_out = out.data_ptr(), dout.data_ptr(), dw.data_ptr(), db.data_ptr(), dz.data_ptr()
    d.src[0].dx, d.src[0].lddx, d.src[0].dx_dtype = dx0.data_ptr(), 8, CODE['bf16']
    d.src[1].dx, d.src[1].lddx, d.src[1].dx_dtype = dx1.data_ptr(), 8, CODE['f32']
    outs = [(t, raw(t)) for t in (dw, db, dz, dx0, dx1)]
    BWD_REFUSALS[what](d)
    refused(E.lib.satcv_dense_small_bwd(C.byref(d), E.st), 'dense_small_bwd', outs)
