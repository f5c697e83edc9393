"""Op-level parity of the element-wise glue kernels (csrc/elementwise.hip) through the C ABI against the float64 restatements of
tests/elementwise_oracle.py: every kernel at a small shape, a ragged one (n = 3, odd h and w) and one past the launch cap of the
grid-stride loops (256 * SATCV_EW_PER_CU workgroups), channel counts whose group count is not a power of two, channel slices of wider
tensors guarded by sentinels / NaN, the in-place forms the engine uses, and the argument checks (error code, output untouched).

Bounds (none tuned on the device): bit-exact where the kernel selects, performs one float32 operation or sums integers; the derived
bounds (npix - 1) 2^-24 sum|v| and binomial 5 sigma; otherwise the op-level close() bounds of tests/test_ops_gpu.py (2e-5 fp32,
1.2e-2 bf16, relative to the output scale).  Every toleranced check prints its worst error as a `[fig]` line (pytest -rP)."""
import ctypes as C
import math
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
import elementwise_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16, 'fp8': torch.float8_e4m3fn}
CODE = {'f32': 0, 'bf16': 1, 'fp8': 2}
ES = {'f32': 4, 'bf16': 2, 'fp8': 1}
RAW = {'f32': torch.int32, 'bf16': torch.int16, 'fp8': torch.uint8}
KINDS2, KINDS3 = ['f32', 'bf16'], ['f32', 'bf16', 'fp8']
SENT = -777.0
CAP = O.grid_cap_threads()                   # work items of the largest launch at the documented default
NONPOW2_C = [8, 24, 40, 72, 1000, 2048]


class _Env:
    def __getattr__(self, name):
        from satellite_computervision_amd import _lib, ops
        assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
        self.lib, self.check, self.HeadDesc, self.st = _lib.lib, _lib.check, _lib.HeadDesc, ops.stream_ptr()
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
    return t.detach().contiguous().view(RAW[{4: 'f32', 2: 'bf16', 1: 'fp8'}[t.element_size()]]).cpu().numpy()


def rnd(rng, shape, kind, scale=1.0):
    return O.to_storage((rng.standard_normal(shape) * scale).astype(np.float32), kind)


def wide(x64, kind, ld, off, fill):
    """(npix, c) -> device (npix, ld) of the storage type holding x at channels [off, off + c) and `fill` elsewhere"""
    buf = np.full((x64.shape[0], ld), fill, np.float64)
    buf[:, off:off + x64.shape[1]] = x64
    return dev(buf, kind)


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def outside_untouched(t, before_raw, off, c):
    now = raw(t)
    keep = np.ones(now.shape[-1], bool)
    keep[off:off + c] = False
    return np.array_equal(now[..., keep], before_raw[..., keep])


def fig(what, err, tol):
    print(f'[fig] {what}: {err:.3e} (bound {tol:.1e})')


def close(got, ref, kind, what):
    err, _ = O.close_err(got, ref)
    tol = O.close_tol(kind)
    fig(what, err, tol)
    assert err < tol, f'{what}: rel-to-max err {err:.3e} >= {tol:.1e}'


def refused(rc, out=None, before=None):
    assert rc != 0, 'the call should have been refused'
    if out is not None:
        sync()
        assert np.array_equal(raw(out), before), 'a refused call wrote to its output'


def rows_past_cap(groups_per_row, extra=3):
    """rows such that rows * groups_per_row work items take at least two full trips of the stride loop, plus a ragged tail"""
    return -(-2 * CAP // groups_per_row) + extra


# ------------------------------------------------------------------------- maxpool
POOL_WINDOWS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (3, 2, 0), (1, 2, 0)]
POOL_MAPS = [(2, 8, 8, 8), (3, 7, 9, 8), (3, 2, 2, 8), (1, 3, 3, 24), (2, 16, 17, 40)]


def check_maxpool(kind, win, shape, seed=0):
    k, s, pad = win
    n, h, w, c = shape
    ho, wo = O.pool_out(h, k, s, pad), O.pool_out(w, k, s, pad)
    rng = np.random.default_rng(seed)
    neg = O.to_storage((-0.5 - np.abs(rnd(rng, shape, kind))).astype(np.float32), kind)
    for x in (rnd(rng, shape, kind), neg):                                        # the second: zero padding would win at every border
        xd = dev(x, kind)
        if ho < 1 or wo < 1:
            out = dev(np.full((n, 1, 1, c), 5.0), kind)
            refused(E.lib.satcv_maxpool(xd.data_ptr(), out.data_ptr(), n, h, w, c, k, s, pad, CODE[kind], E.st), out, raw(out))
            continue
        out = dev(np.full((n, ho, wo, c), 5.0), kind)
        E.check(E.lib.satcv_maxpool(xd.data_ptr(), out.data_ptr(), n, h, w, c, k, s, pad, CODE[kind], E.st))
        sync()
        assert np.array_equal(host(out), O.maxpool(x, k, s, pad)), f'maxpool {kind} {win} {shape}'


@pytest.mark.parametrize('kind', KINDS3)
@pytest.mark.parametrize('win', POOL_WINDOWS)
@pytest.mark.parametrize('shape', POOL_MAPS)
def test_maxpool(kind, win, shape):
    check_maxpool(kind, win, shape)


@pytest.mark.parametrize('kind', KINDS3)
def test_maxpool_past_the_launch_cap(kind):
    c, (k, s, pad) = 24, (3, 2, 1)
    ho = math.isqrt(rows_past_cap(c // 8)) + 1
    h = 2 * ho - 1                                                               # odd map, ho * ho * c / 8 >= 2 * cap
    assert O.pool_out(h, k, s, pad) == ho and ho * ho * (c // 8) >= 2 * CAP
    check_maxpool(kind, (k, s, pad), (1, h, h, c))


def test_maxpool_refuses_bad_arguments():
    x = dev(np.ones((1, 4, 4, 12)), 'f32')
    out = dev(np.full((1, 4, 4, 12), 5.0), 'f32')
    before = raw(out)
    refused(E.lib.satcv_maxpool(x.data_ptr(), out.data_ptr(), 1, 4, 4, 12, 2, 2, 0, 0, E.st), out, before)         # c % 8
    refused(E.lib.satcv_maxpool(x.data_ptr(), out.data_ptr(), 1, 2, 2, 8, 3, 2, 0, 0, E.st), out, before)          # empty output
    refused(E.lib.satcv_maxpool(x.data_ptr(), out.data_ptr(), 1, 4, 4, 8, 2, 2, 0, 7, E.st), out, before)          # dtype


# ------------------------------------------------------------------------- add_act
def _f32_then_storage(a32, kind):
    return torch.tensor(a32).to(TD[kind]).to(torch.float64).numpy()


def check_add_act(kind, npix, c, seed=0, combos=None):
    rng = np.random.default_rng(seed + c)
    y, res = rnd(rng, (npix, c), kind), rnd(rng, (npix, c), kind)
    coef = [rng.uniform(0.5, 1.5, c).astype(np.float32) if i % 2 == 0 else rng.standard_normal(c).astype(np.float32) for i in range(4)]
    cd = [f32dev(v) for v in coef]
    yd, rd = dev(y, kind), dev(res, kind)
    for ya, ra, relu in combos or [(a, b, r) for a in (0, 1) for b in (0, 1) for r in (0, 1)]:
        out = dev(np.full((npix, c), SENT), kind)
        E.check(E.lib.satcv_add_act(yd.data_ptr(), ptr(cd[0]) if ya else None, ptr(cd[1]) if ya else None, rd.data_ptr(), ptr(cd[2]) if ra else None,
                                    ptr(cd[3]) if ra else None, relu, out.data_ptr(), npix, c, CODE[kind], E.st))
        sync()
        if not ya and not ra:              # one rounded float32 add, then the storage rounding
            u = y.astype(np.float32) + res.astype(np.float32)
            ref = _f32_then_storage(np.maximum(u, np.float32(0)) if relu else u, kind)
            assert np.array_equal(host(out), ref), f'add_act plain {kind} npix={npix} c={c} relu={relu}'
        else:
            ref = O.add_act(y, coef[0] if ya else None, coef[1] if ya else None, res, coef[2] if ra else None, coef[3] if ra else None, relu)
            close(host(out), ref, kind, f'add_act {kind} npix={npix} c={c} affine=({ya},{ra}) relu={relu}')
    # the engine's backward fan-in: out == y, no affine
    first = yd.clone()
    E.check(E.lib.satcv_add_act(first.data_ptr(), None, None, rd.data_ptr(), None, None, 0, first.data_ptr(), npix, c, CODE[kind], E.st))
    sync()
    assert np.array_equal(host(first), _f32_then_storage(y.astype(np.float32) + res.astype(np.float32), kind)), 'add_act in place'


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('npix,c', [(64, 8), (3 * 7 * 5, 24), (1031, 40), (517, 72), (301, 1000), (97, 2048), (1, 2048), (1, 24)])
def test_add_act(kind, npix, c):
    check_add_act(kind, npix, c)


@pytest.mark.parametrize('kind', KINDS2)
def test_add_act_past_the_launch_cap(kind):
    assert CAP % 5 != 0                                                          # c = 40: idle threads on the capped grid
    check_add_act(kind, rows_past_cap(5), 40, combos=[(0, 0, 0), (1, 1, 1), (1, 0, 1)])


def test_add_act_refuses_bad_arguments():
    y = dev(np.ones((4, 2056)), 'f32')
    out = dev(np.full((4, 2056), SENT), 'f32')
    before = raw(out)
    for c in (12, 2056, 0):
        refused(E.lib.satcv_add_act(y.data_ptr(), None, None, y.data_ptr(), None, None, 0, out.data_ptr(), 4, c, 0, E.st), out, before)
    refused(E.lib.satcv_add_act(y.data_ptr(), None, None, y.data_ptr(), None, None, 0, out.data_ptr(), 4, 8, 2, E.st), out, before)     # fp8 not taken


# ------------------------------------------------------------------------ relu_bwd
def check_relu_bwd(kind, count, seed=0):
    rng = np.random.default_rng(seed)
    act = rnd(rng, (count,), kind)
    tiny = float(np.float32(1e-40)) if kind == 'f32' else 2.0 ** -130              # denormal in either storage type
    special = np.array([0.0, -0.0, tiny, -tiny, -1.0, 1.0, -0.0, 0.0])
    act[:8] = special
    act[-8:] = special[::-1]
    g = rnd(rng, (count,), kind)
    g[1] = -3.0
    ad, gd = dev(act, kind), dev(g, kind)
    assert np.array_equal(host(ad)[:8], special)                                  # the denormals survive the trip to the device
    E.check(E.lib.satcv_relu_bwd(ad.data_ptr(), gd.data_ptr(), count, CODE[kind], E.st))
    sync()
    assert np.array_equal(raw(gd), raw(dev(O.relu_bwd(act, g), kind))), f'relu_bwd {kind} count={count}'


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('count', [8 * 2, 8 * 255, 8 * (256 * 3 + 1), 3 * 7 * 5 * 24])
def test_relu_bwd(kind, count):
    check_relu_bwd(kind, count)


@pytest.mark.parametrize('kind', KINDS2)
def test_relu_bwd_past_the_launch_cap(kind):
    check_relu_bwd(kind, 8 * (2 * CAP + 5))


def test_relu_bwd_refuses_bad_arguments():
    a, g = dev(np.ones(64), 'f32'), dev(np.full(64, SENT), 'f32')
    before = raw(g)
    refused(E.lib.satcv_relu_bwd(a.data_ptr(), g.data_ptr(), 60, 0, E.st), g, before)
    refused(E.lib.satcv_relu_bwd(a.data_ptr(), g.data_ptr(), 0, 0, E.st), g, before)
    refused(E.lib.satcv_relu_bwd(a.data_ptr(), g.data_ptr(), 64, 2, E.st), g, before)


# ----------------------------------------------------------------------- bias_grad
def run_bias_grad(dyd, off, ld, npix, c, kind, dbias0, partials):
    """-> (dbias float32 array, guard ok).  partials: False = atomics, True = the reproducible form with a guarded workspace"""
    db = f32dev(dbias0)
    ws, nws = None, 0
    if partials:
        nb = E.lib.satcv_bias_grad_workspace(npix, c)
        assert nb > 0 and nb % 4 == 0
        nws = nb // 4
        ws = torch.full((nws + 256,), SENT, dtype=torch.float32, device='cuda')
    E.check(E.lib.satcv_bias_grad(ptr(dyd, off), ld, npix, c, CODE[kind], db.data_ptr(), ws.data_ptr() if partials else None, E.st))
    sync()
    if partials:
        assert (ws[nws:] == SENT).all().item(), 'bias_grad wrote past satcv_bias_grad_workspace bytes'
    return db.cpu().numpy()


def check_bias_grad_exact(kind, npix, c, seed=0):
    """small integers: every partial sum is an integer below 2^24, the result is exact in any order"""
    assert 8 * npix + 16 < 2 ** 24
    rng = np.random.default_rng(seed + npix + c)
    dy = rng.integers(-8, 9, (npix, c)).astype(np.float64)
    pre = (np.arange(c) % 17 - 8).astype(np.float64)                              # dbias is accumulated into
    ref = (O.bias_grad(dy) + pre).astype(np.float32)
    plain, sliced = dev(dy, kind), wide(dy, kind, c + 16, 8, np.nan)
    for partials in (False, True):
        for dyd, off, ld in ((plain, 0, c), (sliced, 8, c + 16)):
            got = run_bias_grad(dyd, off, ld, npix, c, kind, pre, partials)
            assert np.array_equal(got, ref), f'bias_grad {kind} npix={npix} c={c} partials={partials} ld={ld}: {np.abs(got - ref).max()} off'


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('c', NONPOW2_C)
@pytest.mark.parametrize('npix', [1, 257, 3 * 7 * 5, 1031])
def test_bias_grad_integer_sums_are_exact(kind, c, npix):
    check_bias_grad_exact(kind, npix, c)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('c', [40, 72, 8])
def test_bias_grad_past_the_launch_cap(kind, c):
    """c = 40, 72: five / nine groups do not divide the capped launch's thread count, so the idle-thread branch runs on a capped grid"""
    assert c == 8 or CAP % (c // 8) != 0
    check_bias_grad_exact(kind, rows_past_cap(c // 8), c)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('npix,c', [(1031, 40), (20011, 24), (4099, 1000)])
def test_bias_grad_random_values(kind, npix, c):
    rng = np.random.default_rng(npix)
    dy = rnd(rng, (npix, c), kind)
    dyd = dev(dy, kind)
    ref, bound = O.bias_grad(dy), O.bias_grad_bound(dy)
    zero = np.zeros(c)
    a = run_bias_grad(dyd, 0, c, npix, c, kind, zero, False)
    p1 = run_bias_grad(dyd, 0, c, npix, c, kind, zero, True)
    p2 = run_bias_grad(dyd, 0, c, npix, c, kind, zero, True)
    assert np.array_equal(p1.view(np.int32), p2.view(np.int32)), 'the partials form is not bit-reproducible'
    for name, got in (('atomics', a), ('partials', p1)):
        err = np.abs(got.astype(np.float64) - ref)
        worst = (err / bound).max()
        fig(f'bias_grad {name} {kind} npix={npix} c={c} (fraction of the derived bound)', worst, 1.0)
        assert (err <= bound).all(), f'bias_grad {name}: {worst:.3f} of the bound'


def test_bias_grad_refuses_bad_arguments():
    dy = dev(np.ones((4, 2056)), 'f32')
    db = f32dev(np.full(2056, SENT))
    before = raw(db)
    for c, ld in ((12, 12), (2056, 2056), (16, 8)):
        refused(E.lib.satcv_bias_grad(dy.data_ptr(), ld, 4, c, 0, db.data_ptr(), None, E.st), db, before)
    assert E.lib.satcv_bias_grad_workspace(4, 12) == 0 and E.lib.satcv_bias_grad_workspace(0, 8) == 0


# ------------------------------------------------------------------- upsample_head
def check_upsample_head(case, with_classes=True):
    n, h, w, ncls, f, act, thresh = case
    lg = O.upsample_logits(case)
    p_ref, c_ref, margin = O.upsample_head(lg.astype(np.float64), f, act, thresh)
    probs = torch.full(p_ref.shape, SENT, dtype=torch.float32, device='cuda')
    classes = torch.full(c_ref.shape, -5, dtype=torch.int32, device='cuda')
    lgd = f32dev(lg)
    E.check(E.lib.satcv_upsample_head(lgd.data_ptr(), n, h, w, ncls, f, act, thresh, probs.data_ptr(), classes.data_ptr() if with_classes else None, E.st))
    sync()
    close(host(probs), p_ref, 'f32', f'upsample_head probs {case}')
    if not with_classes:
        assert (classes == -5).all().item()
        return host(probs)
    bound = O.close_tol('f32') * max(np.abs(p_ref).max(), 1e-6)
    sure = margin > bound
    left_out = 1.0 - sure.mean()
    fig(f'upsample_head share of pixels left out of the class comparison {case}', left_out, 0.01)
    assert left_out <= 0.01
    assert np.array_equal(classes.cpu().numpy()[sure], c_ref[sure]), f'upsample_head classes {case}'
    return host(probs)


@pytest.mark.parametrize('case', O.upsample_cases())
def test_upsample_head(case):
    check_upsample_head(case)


def test_upsample_head_without_classes_and_ties():
    for case in (O.upsample_cases()[1], O.upsample_cases()[8]):
        assert np.array_equal(check_upsample_head(case, with_classes=False), check_upsample_head(case))
    lg = np.random.default_rng(0).standard_normal((2, 3, 5, 4)).astype(np.float32)
    lg[..., 0] -= 10.0
    lg[..., 2] = lg[..., 1] = np.maximum(lg[..., 1], lg[..., 3]) + 1.0              # classes 1 and 2 tie for the maximum everywhere
    probs = torch.empty((2, 9, 15, 4), dtype=torch.float32, device='cuda')
    classes = torch.full((2, 9, 15), -5, dtype=torch.int32, device='cuda')
    lgd = f32dev(lg)
    E.check(E.lib.satcv_upsample_head(lgd.data_ptr(), 2, 3, 5, 4, 3, 0, 0.5, probs.data_ptr(), classes.data_ptr(), E.st))
    sync()
    assert (classes == 1).all().item(), 'two equal logits give the lower index'


def test_upsample_head_refuses_bad_arguments():
    lg = f32dev(np.zeros((1, 2, 2, 9)))
    probs = torch.full((1, 4, 4, 9), SENT, dtype=torch.float32, device='cuda')
    before = raw(probs)
    refused(E.lib.satcv_upsample_head(lg.data_ptr(), 1, 2, 2, 9, 2, 0, 0.5, probs.data_ptr(), None, E.st), probs, before)
    refused(E.lib.satcv_upsample_head(lg.data_ptr(), 1, 2, 2, 2, 0, 0, 0.5, probs.data_ptr(), None, E.st), probs, before)
    refused(E.lib.satcv_upsample_head(lg.data_ptr(), 1, 0, 2, 2, 2, 0, 0.5, probs.data_ptr(), None, E.st), probs, before)


# -------------------------------------------------------------------- dropout_mask
N_DRAWS = 2 ** 22


def gen_mask(seed, offset, rate, count):
    m = torch.full((count + 64,), SENT, dtype=torch.float32, device='cuda')
    E.check(E.lib.satcv_dropout_mask(seed, offset, rate, count, m.data_ptr(), E.st))
    sync()
    assert (m[count:] == SENT).all().item()
    return m[:count].cpu().numpy()


@pytest.mark.parametrize('rate', [0.1, 0.25, 0.5, 0.9])
def test_dropout_mask_values_share_and_correlation(rate):
    assert N_DRAWS >= 2 * CAP
    m = gen_mask(1234, 0, rate, N_DRAWS)
    keep = O.dropout_keep_value(rate)
    kept = m != 0
    assert np.array_equal(m[kept].view(np.int32), np.full(int(kept.sum()), keep).view(np.int32)) and not m[~kept].view(np.int32).any()
    p = 1.0 - float(np.float32(rate))
    dev_ = abs(kept.mean() - p)
    fig(f'dropout_mask kept share, rate {rate}', dev_, O.five_sigma(rate, N_DRAWS))
    assert dev_ <= O.five_sigma(rate, N_DRAWS)
    # lag correlation: under independence "both kept" is Bernoulli(p^2); overlapping pairs (i, i + L), (i + L, i + 2 L) share one draw,
    # covariance p^3 - p^4, so the variance of the mean over N pairs is (p^2 (1 - p^2) + 2 (p^3 - p^4)) / N
    for lag in (1, 24, 256, CAP):                       # neighbours, a mask row (ldm = 24), a workgroup, one trip of the grid
        both = (kept[:-lag] & kept[lag:]).mean()
        bound = 5.0 * math.sqrt((p * p * (1 - p * p) + 2 * (p ** 3 - p ** 4)) / (N_DRAWS - lag))
        fig(f'dropout_mask lag-{lag} pair share, rate {rate}', abs(both - p * p), bound)
        assert abs(both - p * p) <= bound, f'lag {lag}'


def test_dropout_mask_stream_is_counter_based():
    k = CAP + 37                                           # the shift crosses the launch cap
    base = gen_mask(99, 0, 0.25, N_DRAWS)
    assert np.array_equal(gen_mask(99, k, 0.25, N_DRAWS - k), base[k:])
    assert np.array_equal(gen_mask(99, 1 << 40, 0.25, 4096), gen_mask(99, 1 << 40, 0.25, 4096))
    assert np.array_equal(gen_mask(99, 0, 0.25, N_DRAWS), base)
    other = gen_mask(100, 0, 0.25, N_DRAWS)
    agree = ((other != 0) == (base != 0)).mean()            # two independent streams agree on p^2 + (1 - p)^2 of the draws
    assert abs(agree - (0.75 ** 2 + 0.25 ** 2)) <= 5.0 * math.sqrt(0.625 * 0.375 / N_DRAWS)
    assert (gen_mask(7, 0, 0.0, 3 * 7 * 5 * 24) == 1.0).all()
    assert gen_mask(7, 5, 0.5, 1).shape == (1,)


def test_dropout_mask_refuses_bad_arguments():
    m = torch.full((64,), SENT, dtype=torch.float32, device='cuda')
    before = raw(m)
    for rate in (1.0, -0.1, 1.5):
        refused(E.lib.satcv_dropout_mask(1, 0, rate, 64, m.data_ptr(), E.st), m, before)
    refused(E.lib.satcv_dropout_mask(1, 0, 0.5, 0, m.data_ptr(), E.st), m, before)


# ------------------------------------------------------------------- dropout_apply
def check_dropout_apply(kind, n, hw, c, mode, fused, seed=0):
    rng = np.random.default_rng(seed + c + mode)
    npix = n * hw
    x = rnd(rng, (npix, c), kind)
    rows = n if mode == 0 else npix
    mask = ((rng.random((rows, c)) >= 0.3) * np.float64(O.dropout_keep_value(0.3)))
    sc, sh = (rng.uniform(0.5, 1.5, c).astype(np.float32), rng.standard_normal(c).astype(np.float32)) if fused else (None, None)
    scd, shd = (f32dev(sc), f32dev(sh)) if fused else (None, None)
    ldx, ldm, ldo = c + 16, c + 8, c + 24
    xd = wide(x, kind, ldx, 8, np.nan)
    md = wide(mask, 'f32', ldm, 8, np.nan)
    out = dev(np.full((npix, ldo), SENT), kind)
    before = raw(out)
    E.check(E.lib.satcv_dropout_apply(ptr(xd, 8), ldx, ptr(scd) if fused else None, ptr(shd) if fused else None, 1, ptr(md, 8), ldm, mode,
                                      ptr(out, 16), ldo, n, hw, c, CODE[kind], E.st))
    sync()
    assert outside_untouched(out, before, 16, c), 'dropout_apply wrote outside its channel slice'
    got = host(out)[:, 16:16 + c]
    if fused:
        close(got, O.dropout_apply(x, mask, mode, hw, sc, sh, True), kind, f'dropout_apply fused {kind} n={n} hw={hw} c={c} mode={mode}')
    else:                                   # one float32 multiply, then the storage rounding
        m32 = (mask[np.arange(npix) // hw] if mode == 0 else mask).astype(np.float32)
        assert np.array_equal(got, _f32_then_storage(x.astype(np.float32) * m32, kind)), f'dropout_apply {kind} n={n} hw={hw} c={c} mode={mode}'
        # the engine's backward: g * mask in place, ld == c
        gd, mc = dev(x, kind), f32dev(mask)
        E.check(E.lib.satcv_dropout_apply(gd.data_ptr(), c, None, None, 0, mc.data_ptr(), c, mode, gd.data_ptr(), c, n, hw, c, CODE[kind], E.st))
        sync()
        assert np.array_equal(host(gd), got), 'dropout_apply in place'


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('n,hw,c', [(2, 16, 8), (3, 7 * 9, 24), (3, 7 * 9, 40), (1, 1, 72)])
def test_dropout_apply(kind, mode, fused, n, hw, c):
    check_dropout_apply(kind, n, hw, c, mode, fused)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('mode', [0, 1])
def test_dropout_apply_past_the_launch_cap(kind, mode):
    check_dropout_apply(kind, 5, -(-rows_past_cap(3) // 5), 24, mode, False)


def test_dropout_apply_refuses_bad_arguments():
    x = dev(np.ones((8, 32)), 'f32')
    m = f32dev(np.ones((8, 32)))
    out = dev(np.full((8, 32), SENT), 'f32')
    before = raw(out)
    for c, ldx, ldm, ldo, mode in ((12, 12, 12, 12, 1), (16, 16, 8, 16, 1), (16, 8, 16, 16, 1), (16, 16, 16, 8, 1), (16, 16, 16, 16, 2)):
        refused(E.lib.satcv_dropout_apply(x.data_ptr(), ldx, None, None, 0, m.data_ptr(), ldm, mode, out.data_ptr(), ldo, 2, 4, c, 0, E.st), out, before)


# ------------------------------------------------------------------ affine_requant
def check_affine_requant(pair, npix, c, relu, seed=None):
    kin, kout = pair
    x, sc, sh = O.requant_inputs(npix, c, kin, seed=npix + c + relu if seed is None else seed)
    ldx, ldo = c + 16, c + 24
    xd = wide(x, kin, ldx, 8, np.nan)
    out = torch.full((npix, ldo), 0x55, dtype=torch.uint8, device='cuda').view(TD[kout]) if kout == 'fp8' else dev(np.full((npix, ldo), SENT), kout)
    before = raw(out)
    scd, shd = f32dev(sc), f32dev(sh)
    E.check(E.lib.satcv_affine_requant(ptr(xd, 8), ldx, scd.data_ptr(), shd.data_ptr(), relu, ptr(out, 16), ldo, npix, c, CODE[kin], CODE[kout], E.st))
    sync()
    assert outside_untouched(out, before, 16, c), 'affine_requant wrote outside its channel slice'
    got = host(out)[:, 16:16 + c]
    assert not np.isnan(got).any(), 'NaN in the output (a read outside the input slice, or an unsaturated conversion)'
    if kout == 'fp8':
        val, lo, hi, amb = O.affine_requant_fp8(x, sc, sh, relu)
        fig(f'affine_requant {pair} npix={npix} c={c} relu={relu} share near a rounding boundary', amb.mean(), 0.01)
        assert amb.mean() <= 0.01
        ok = (got == val) | (amb & ((got == lo) | (got == hi)))
        assert ok.all(), f'affine_requant {pair}: {(~ok).sum()} of {ok.size} e4m3 values differ, first {got[~ok][:4]} vs {val[~ok][:4]}'
        assert np.abs(got).max() == O.E4M3_MAX                                      # saturated, not NaN
    else:
        close(got, O.affine(x, sc, sh, bool(relu)), kout, f'affine_requant {pair} npix={npix} c={c} relu={relu}')


@pytest.mark.parametrize('pair', O.REQUANT_PAIRS)
@pytest.mark.parametrize('npix,c', O.REQUANT_SHAPES)
@pytest.mark.parametrize('relu', [0, 1])
def test_affine_requant(pair, npix, c, relu):
    check_affine_requant(pair, npix, c, relu)


@pytest.mark.parametrize('pair', O.REQUANT_PAIRS)
def test_affine_requant_past_the_launch_cap(pair):
    assert 4099 * 2048 // 8 >= 2 * CAP
    check_affine_requant(pair, 4099, 2048, 1)                                       # the CPU file holds this seed under the 1 % cap


def test_affine_requant_refuses_bad_arguments():
    x = dev(np.ones((8, 32)), 'f32')
    s = f32dev(np.ones(32))
    out = dev(np.full((8, 32), SENT), 'f32')
    before = raw(out)
    for kin, kout in (('bf16', 'f32'), ('f32', 'bf16'), ('fp8', 'f32')):
        refused(E.lib.satcv_affine_requant(x.data_ptr(), 32, s.data_ptr(), s.data_ptr(), 0, out.data_ptr(), 32, 8, 16, CODE[kin], CODE[kout], E.st), out, before)
    for c, ldx, ldo in ((12, 12, 12), (16, 8, 16), (16, 16, 8)):
        refused(E.lib.satcv_affine_requant(x.data_ptr(), ldx, s.data_ptr(), s.data_ptr(), 0, out.data_ptr(), ldo, 8, c, 0, 0, E.st), out, before)


# -------------------------------------------------------------- ingest_nhwc_scaled
def check_ingest_scaled(kind, npix, c, mul=37.5):
    rng = np.random.default_rng(npix + c)
    src = rng.random((npix, c)).astype(np.float32)
    out = torch.full((npix, 16), 0x55, dtype=torch.uint8, device='cuda').view(TD[kind]) if kind == 'fp8' else dev(np.full((npix, 16), SENT), kind)
    srcd = f32dev(src)
    E.check(E.lib.satcv_ingest_nhwc_scaled(srcd.data_ptr(), out.data_ptr(), npix, c, 16, mul, CODE[kind], E.st))
    sync()
    ref = O.to_storage(O.ingest_scaled_f32(src, 16, mul), kind)                     # the multiplier first, then the storage rounding
    assert np.array_equal(host(out), ref), f'ingest_nhwc_scaled {kind} npix={npix} c={c}'
    assert not raw(out)[:, c:].any(), 'pad channels are exactly zero'


@pytest.mark.parametrize('kind', KINDS3)
@pytest.mark.parametrize('c', [4, 13])
@pytest.mark.parametrize('npix', [16, 3 * 7 * 5])
def test_ingest_nhwc_scaled(kind, c, npix):
    check_ingest_scaled(kind, npix, c)


@pytest.mark.parametrize('kind', KINDS3)
def test_ingest_nhwc_scaled_past_the_launch_cap(kind):
    check_ingest_scaled(kind, rows_past_cap(2), 13)


def test_ingest_nhwc_scaled_refuses_bad_arguments():
    src = f32dev(np.ones((8, 13)))
    out = dev(np.full((8, 16), SENT), 'f32')
    before = raw(out)
    for c, cpad in ((13, 12), (13, 8), (0, 16)):
        refused(E.lib.satcv_ingest_nhwc_scaled(src.data_ptr(), out.data_ptr(), 8, c, cpad, 2.0, 0, E.st), out, before)


# ------------------------------------------------------------------------ head_bwd
def run_head_bwd(kind, xd, ld, off, cin, ncls, scd, shd, wd, dld, npix, form):
    """form 'atomics' | 'partials' -> (dx, dw, db) as float64 / float32 host arrays"""
    dx = dev(np.full((npix, cin + 16), SENT), kind)
    before = raw(dx)
    dw, db = torch.zeros((cin, ncls), dtype=torch.float32, device='cuda'), torch.zeros(ncls, dtype=torch.float32, device='cuda')
    d = E.HeadDesc()
    d.x, d.ldx, d.cin = ptr(xd, off), ld, cin
    d.in_scale, d.in_shift = (scd.data_ptr(), shd.data_ptr()) if scd is not None else (None, None)
    d.w, d.ncls, d.dlogits = wd.data_ptr(), ncls, dld.data_ptr()
    d.dx, d.lddx, d.dw, d.db = ptr(dx, 8), cin + 16, dw.data_ptr(), db.data_ptr()
    d.npix, d.dtype = npix, CODE[kind]
    nb = E.lib.satcv_head_bwd_workspace(C.byref(d))
    if form == 'partials':
        assert nb > 0 and nb % 4 == 0
        ws = torch.full((nb // 4 + 256,), SENT, dtype=torch.float32, device='cuda')
        d.partials = ws.data_ptr()
        E.check(E.lib.satcv_head_bwd(C.byref(d), E.st))
        E.check(E.lib.satcv_head_bwd_finalize(C.byref(d), E.st))
        sync()
        assert (ws[nb // 4:] == SENT).all().item(), 'head_bwd wrote past satcv_head_bwd_workspace bytes'
    else:
        E.check(E.lib.satcv_head_bwd(C.byref(d), E.st))
        sync()
    assert outside_untouched(dx, before, 8, cin), 'head_bwd wrote dx outside its channel slice'
    return host(dx)[:, 8:8 + cin], dw.cpu().numpy(), db.cpu().numpy(), nb


def check_head_bwd(kind, cin, ncls, npix, affine, fast=True):
    rng = np.random.default_rng(cin + ncls + npix)
    # ---- integer-valued inputs: dW, db (and dx) are exact in any order, in both forms
    assert 16 * npix < 2 ** 24
    xi = rng.integers(-4, 5, (npix, cin)).astype(np.float64)
    wi = rng.integers(-2, 3, (cin, ncls)).astype(np.float64)
    dli = rng.integers(-4, 5, (npix, ncls)).astype(np.float64)
    dxr, dwr, dbr = O.head_bwd(xi, None, None, wi, dli)
    xd, wd, dld = wide(xi, kind, cin + 8, 8, np.nan), f32dev(wi), f32dev(dli)
    for form in (('atomics', 'partials') if fast else ('atomics',)):
        dx, dw, db, nb = run_head_bwd(kind, xd, cin + 8, 8, cin, ncls, None, None, wd, dld, npix, form)
        assert (nb > 0) == fast
        assert np.array_equal(dw, dwr.astype(np.float32)) and np.array_equal(db, dbr.astype(np.float32)) and np.array_equal(dx, dxr), f'head_bwd integers {form}'
    # ---- random values against float64 (autograd-pinned restatement) and the two forms against each other
    x, w, dl = rnd(rng, (npix, cin), kind), rng.standard_normal((cin, ncls)).astype(np.float32), (rng.standard_normal((npix, ncls)) / npix).astype(np.float32)
    sc, sh = (rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.standard_normal(cin).astype(np.float32)) if affine else (None, None)
    dxr, dwr, dbr = O.head_bwd(x, sc, sh, w, dl.astype(np.float64))
    xd, wd, dld = dev(x, kind), f32dev(w), f32dev(dl)
    scd, shd = (f32dev(sc), f32dev(sh)) if affine else (None, None)
    res = {}
    for form in (('atomics', 'partials', 'partials') if fast else ('atomics',)):
        dx, dw, db, _ = run_head_bwd(kind, xd, cin, 0, cin, ncls, scd, shd, wd, dld, npix, form)
        tag = f'head_bwd {form} {kind} cin={cin} ncls={ncls} npix={npix} affine={affine}'
        close(dx, dxr, kind, tag + ' dx')
        close(dw, dwr, 'f32', tag + ' dW')
        close(db, dbr, 'f32', tag + ' db')
        if form in res and form == 'partials':
            assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(res[form][1:], (dw, db))), 'partials form not bit-reproducible'
        res[form] = (dx, dw, db)
    if fast:
        close(res['partials'][1], res['atomics'][1].astype(np.float64), 'f32', 'head_bwd partials vs atomics dW')
        close(res['partials'][2], res['atomics'][2].astype(np.float64), 'f32', 'head_bwd partials vs atomics db')
        assert np.array_equal(res['partials'][0], res['atomics'][0])


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('cin,ncls', [(16, 1), (16, 2), (32, 3), (32, 4), (64, 2)])
@pytest.mark.parametrize('npix,affine', [(64, False), (3 * 7 * 5, True), (1031, True)])
def test_head_bwd_partials(kind, cin, ncls, npix, affine):
    check_head_bwd(kind, cin, ncls, npix, affine)


@pytest.mark.parametrize('kind', KINDS2)
def test_head_bwd_partials_past_the_launch_cap(kind):
    check_head_bwd(kind, 16, 2, rows_past_cap(2), True)


@pytest.mark.parametrize('kind', KINDS2)
@pytest.mark.parametrize('cin,ncls', [(24, 2), (32, 5), (128, 2)])
def test_head_bwd_outside_the_register_resident_kernel(kind, cin, ncls):
    """satcv_head_bwd_workspace returns 0, the call is still correct (atomics), and `partials` is refused"""
    check_head_bwd(kind, cin, ncls, 3 * 7 * 5, True, fast=False)
    d = E.HeadDesc()
    x, w, dl = dev(np.ones((8, cin)), kind), f32dev(np.ones((cin, ncls))), f32dev(np.ones((8, ncls)))
    dw = torch.full((cin, ncls), SENT, dtype=torch.float32, device='cuda')
    d.x, d.ldx, d.cin, d.w, d.ncls, d.dlogits, d.dw, d.npix, d.dtype, d.partials = x.data_ptr(), cin, cin, w.data_ptr(), ncls, dl.data_ptr(), dw.data_ptr(), 8, CODE[kind], dw.data_ptr()
    before = raw(dw)
    refused(E.lib.satcv_head_bwd(C.byref(d), E.st), dw, before)
    refused(E.lib.satcv_head_bwd_finalize(C.byref(d), E.st), dw, before)


# ------------------------------------------------------------------ adam_step_part
def check_adam_parts(n, cuts, with_mul, steps=3):
    """three launches over [cuts[1], n), [0, cuts[0]), [cuts[0], cuts[1]) -- only the last bumps -- against one satcv_adam_step"""
    rng = np.random.default_rng(n)
    p0, g = f32dev(rng.standard_normal(n)), f32dev(rng.standard_normal(n))
    mul = f32dev(rng.choice([0.0, 0.5, 1.0, 2.0], n)) if with_mul else None
    a, b = cuts
    outs = []
    for parts in (None, ((b, n, 0), (0, a, 0), (a, b, 1))):
        p, m, v = p0.clone(), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
        state = torch.tensor([1e-2, 0.0, 0.5, 0.0], dtype=torch.float32, device='cuda')
        for _ in range(steps):
            if parts is None:
                E.check(E.lib.satcv_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, 0.9, 0.999, 1e-7, state.data_ptr(), ptr(mul) if with_mul else None, E.st))
            else:
                for lo, hi, bump in parts:
                    E.check(E.lib.satcv_adam_step_part(ptr(p, lo), ptr(g, lo), ptr(m, lo), ptr(v, lo), hi - lo, 0.9, 0.999, 1e-7, state.data_ptr(),
                                                       ptr(mul, lo) if with_mul else None, bump, E.st))
        sync()
        assert state[1].item() == float(steps)
        outs.append((p, m, v, state))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(outs[0][0], p0)


@pytest.mark.parametrize('with_mul', [False, True])
def test_adam_step_part(with_mul):
    """odd length, cut after an odd number of 16-byte vectors (the argument check asks for 16-byte aligned sub-ranges: an odd ELEMENT
    offset is refused, below)"""
    check_adam_parts(4 * 1000 + 3, (4 * 33, 4 * 333), with_mul)
    check_adam_parts(4 * 3 + 1, (4, 8), with_mul)
    n = 4 * (2 * 4096 * O.EW_BLOCK) + 4 * 7 + 3                                    # past this kernel's own cap of 4096 workgroups of float4 items
    check_adam_parts(n, (4 * 100001, 4 * 1000003), with_mul, steps=2)


def test_adam_step_part_refuses_bad_arguments():
    n = 64
    p, g, m, v = (f32dev(np.full(n, 1.0 + i)) for i in range(4))
    state = torch.tensor([1e-2, 0.0, 1.0, 0.0], dtype=torch.float32, device='cuda')
    keep = [raw(t) for t in (p, m, v, state)]
    assert E.lib.satcv_adam_step_part(ptr(p, 1), ptr(g, 1), ptr(m, 1), ptr(v, 1), 8, 0.9, 0.999, 1e-7, state.data_ptr(), None, 1, E.st) != 0
    assert E.lib.satcv_adam_step_part(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 0.9, 0.999, 1e-7, state.data_ptr(), None, 1, E.st) != 0
    sync()
    assert all(np.array_equal(raw(t), k) for t, k in zip((p, m, v, state), keep))


# ----------------------------------------------------------------------- confusion
def check_confusion(ncls, npix, one_class=False):
    rng = np.random.default_rng(ncls + npix)
    cls = np.full(npix, ncls - 1) if one_class else rng.integers(0, ncls, npix)
    lab = np.full(npix, ncls // 2) if one_class else rng.integers(0, ncls, npix)
    y = np.eye(ncls, dtype=np.float32)[lab]
    pre = rng.integers(0, 2 ** 40, (ncls, ncls))                                   # the matrix is accumulated into, in 64 bits
    conf = torch.tensor(pre, dtype=torch.int64, device='cuda')
    cd, yd = torch.tensor(cls, dtype=torch.int32, device='cuda'), f32dev(y)
    E.check(E.lib.satcv_confusion(cd.data_ptr(), yd.data_ptr(), ncls, npix, conf.data_ptr(), E.st))
    sync()
    assert np.array_equal(conf.cpu().numpy(), pre + O.confusion(cls, y, ncls)), f'confusion ncls={ncls} npix={npix}'


@pytest.mark.parametrize('ncls', range(1, 9))
def test_confusion(ncls):
    check_confusion(ncls, 3 * 7 * 5)
    check_confusion(ncls, 1)
    check_confusion(ncls, 1031, one_class=True)
    check_confusion(ncls, 2 * 512 * O.EW_BLOCK + 77)                               # past this kernel's own cap of 512 workgroups


def test_confusion_refuses_bad_arguments():
    conf = torch.full((81,), 5, dtype=torch.int64, device='cuda')
    cls, y = torch.zeros(8, dtype=torch.int32, device='cuda'), f32dev(np.ones((8, 9)))
    for ncls, npix in ((9, 8), (0, 8), (2, 0)):
        assert E.lib.satcv_confusion(cls.data_ptr(), y.data_ptr(), ncls, npix, conf.data_ptr(), E.st) != 0
    sync()
    assert (conf == 5).all().item()


# ------------------------------------------------- a smaller launch cap (one child)
def run_small_grid_child():
    """every kernel on a mid-sized tensor with SATCV_EW_PER_CU=1: 256 workgroups, so these sizes take two or more trips"""
    cap = O.grid_cap_threads(1)
    assert os.environ.get('SATCV_EW_PER_CU') == '1'
    assert E.lib.satcv_bias_grad_workspace(10 ** 6, 8) == 256 * 8 * 4, 'the launch cap did not follow SATCV_EW_PER_CU'
    rows = -(-2 * cap // 3) + 3                                                     # c = 24: three groups per pixel
    side = math.isqrt(rows) + 1
    for kind in KINDS3:
        check_maxpool(kind, (3, 2, 1), (1, 2 * side - 1, 2 * side - 1, 24))
        check_ingest_scaled(kind, cap + 3, 13)
    for kind in KINDS2:
        check_add_act(kind, rows, 24, combos=[(0, 0, 1), (1, 1, 1)])
        check_relu_bwd(kind, 8 * (2 * cap + 5))
        check_bias_grad_exact(kind, rows, 24)
        check_dropout_apply(kind, 3, -(-rows // 3), 24, 0, False)
        check_dropout_apply(kind, 3, -(-rows // 3), 24, 1, True)
        check_head_bwd(kind, 16, 2, cap + 3, True)
    for pair in O.REQUANT_PAIRS:
        check_affine_requant(pair, rows, 24, 1, seed=5)
    check_upsample_head((1, 37, 60, 2, 16, 0, 0.5))
    k = cap + 37
    assert np.array_equal(gen_mask(3, k, 0.5, 2 ** 20 - k), gen_mask(3, 0, 0.5, 2 ** 20)[k:])
    check_adam_parts(4 * 1000 + 3, (4 * 33, 4 * 333), True)
    check_confusion(3, 2 * cap + 77)
    print('small-grid child ok')


def test_all_kernels_with_one_workgroup_per_cu():
    """SATCV_EW_PER_CU is read once per process: a fresh child, its own time limit, exit status checked, nothing started after it"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_elementwise_gpu as T; T.run_small_grid_child()' % (ROOT, HERE)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SATCV_EW_PER_CU='1'), capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'small-grid child ok'
