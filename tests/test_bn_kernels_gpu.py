"""Op-level parity of the BatchNorm kernel family (csrc/elementwise.hip: satcv_bn_relu_pool[_amax], satcv_bn_bwd_reduce / _apply,
satcv_bn_finalize_train, satcv_bn_bwd_finalize[2], satcv_bn_affine_infer[_batched]) through the C ABI against the float64 restatements
of tests/bn_oracle.py, over the case tables of that module: every kernel instantiation and launcher branch on lattice inputs (every
float32 operation exact: the outputs are compared bit for bit, the sums exactly wherever the oracle's exactness condition holds) and
on random inputs (derived bounds; outputs under the ambiguity rule of bn_oracle.ambiguous are accepted on either branch).

Bounds (none tuned on the device), u = 2^-24:
  act / pooled, f32:   2 u (|scale y| + |shift|)  -- one product, one sum (or one fma);  bf16: the oracle's bits
  dy:                  8 u |scale| (|g| + |c1| + |xhat c2|)  (+ half a bf16 unit of the reference) -- either association rounds six times at most
  sums of n terms:     (n - 1) u sum|term| per channel (elementwise_oracle.bias_grad_bound), plus what the terms themselves may be off by
  finalize kernels:    k u relative per value, k counted beside each check; rsqrtf / sqrtf and what multiplies them 4 units more
Every toleranced check prints its error as a fraction of the bound in a `[fig]` line (pytest -rP)."""
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
import bn_oracle as B  # noqa: E402
import test_elementwise_gpu as G  # noqa: E402  (device arrays, `wide`, `outside_untouched`, `refused`, `[fig]` lines)

pytestmark = pytest.mark.gpu

U = B.U24
SENT = G.SENT
PAD = 8                                       # columns on either side of a tensor inside its wider buffer
E = G.E


def desc_type():
    from satellite_computervision_amd import _lib
    return _lib.BnBwdDesc


def frac(what, err, bound):
    """worst error / bound over the compared outputs, printed and asserted"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return
    r = np.where(err <= bound, err / np.maximum(bound, 1e-300), np.inf)
    worst = float(r.max())
    G.fig(f'{what} (fraction of the derived bound)', worst, 1.0)
    assert worst <= 1.0, f'{what}: error {err.max():.3e} past its bound at {int((r > 1).sum())} of {r.size} outputs'


class Buf:
    """a (rows, c) tensor of the storage type, alone or at channel offset PAD inside a (rows, c + 2 PAD) buffer filled with `fill`"""

    def __init__(self, x2, kind, widen, fill=SENT, ld=None):
        x2 = np.asarray(x2, np.float64)
        self.c, self.off = x2.shape[1], PAD if widen else 0
        self.ld = ld or (self.c + 2 * PAD if widen else self.c)
        self.t = G.wide(x2, kind, self.ld, self.off, fill) if self.ld != self.c else G.dev(x2, kind)
        self.p = G.ptr(self.t, self.off)
        self.before = G.raw(self.t)

    def get(self, c=None):
        return G.host(self.t)[:, self.off:self.off + (c or self.c)]

    def untouched_outside(self, c=None):
        return G.outside_untouched(self.t, self.before, self.off, c or self.c)


def out_buf(rows, c, kind, widen, ld=None):
    return Buf(np.full((max(rows, 1), c), SENT), kind, widen, ld=ld)


GUARD = 2 * 2048          # doubles behind the replica rows: a reduction that runs over more channels than the slice owns lands here


class Rows:
    """[32][2][ld] float64 replica rows at column offset PAD of a wider buffer, the columns of the slice pre-filled with nonzero values
    (the kernels add to them), the others and a guard region behind the last row with a sentinel"""

    def __init__(self, c, widen, prefill=True):
        self.c, self.off = c, PAD if widen else 0
        self.ld = c + 2 * PAD if widen else c
        base = np.full((B.STAT_ROWS, 2, self.ld), SENT)
        r, w, ch = np.meshgrid(np.arange(B.STAT_ROWS), np.arange(2), np.arange(c), indexing='ij')
        base[:, :, self.off:self.off + c] = ((r * 3 + w + ch) % 7 - 3) * 0.25 if prefill else 0.0
        self.base = base
        self.flat = torch.tensor(np.concatenate([base.reshape(-1), np.full(GUARD, SENT)]), dtype=torch.float64).cuda()
        self.p = self.flat.data_ptr() + self.off * 8

    def now(self):
        v = self.flat.cpu().numpy()
        assert (v[self.base.size:] == SENT).all(), 'written behind the last replica row'
        return v[:self.base.size].reshape(self.base.shape)

    def added(self):
        """(2, c): what the kernel added, summed over the replica rows; the columns outside the slice must hold their sentinel"""
        now = self.now()
        keep = np.ones(self.ld, bool)
        keep[self.off:self.off + self.c] = False
        assert np.array_equal(now[:, :, keep], self.base[:, :, keep]), 'a column outside the statistics slice was written'
        s = slice(self.off, self.off + self.c)
        return (now[:, :, s] - self.base[:, :, s]).sum(0)

    def slice_now(self):
        return self.now()[:, :, self.off:self.off + self.c]


def check_sum(what, got, ref, terms, regime, slack=0.0, per_term=0.0):
    """a per-channel sum of the rows of `terms` ((..., c)): exact on lattice inputs where the oracle's condition holds, otherwise within
    (n - 1) u sum|term| + per_term u sum|term| + slack per channel"""
    t = np.abs(np.asarray(terms, np.float64).reshape(-1, terms.shape[-1]))
    if regime == 'lattice' and B.sum_is_exact(terms):
        assert np.array_equal(got, ref), f'{what}: not exact at channels {np.nonzero(got != ref)[0][:8]}'
        return
    bound = (max(t.shape[0] - 1, 0) + per_term) * U * t.sum(0) + slack + 1e-300
    frac(what, np.abs(got - ref), bound)


# ------------------------------------------------------------------ bn_relu_pool, bn_relu_pool_amax
def check_pool(case, kind, regime, key=None):
    shape, f, amax, actmode, with_pooled, with_stats = case
    n, h, w, c = shape
    hp, wp = h // f, w // f
    npix, npool = n * h * w, n * hp * wp
    d = B.make_inputs(shape, f, kind, regime, key or B.case_id(case))
    y, sc, sh = d['y'], d['scale'], d['shift']
    what = f'bn_relu_pool {B.case_id(case)} {kind} {regime}'
    yd, scd, shd = G.dev(y.reshape(-1, c), kind), G.f32dev(sc), G.f32dev(sh)
    act = None if actmode == 'no' else out_buf(npix, c, kind, actmode == 'wide')
    pooled = out_buf(npool, c, kind, False) if with_pooled else None
    am = torch.full((max(npool, 1), c), 0xEE, dtype=torch.uint8).cuda() if amax else None
    rows = Rows(c, actmode == 'wide') if with_stats else None
    args = [yd.data_ptr(), scd.data_ptr(), shd.data_ptr(), act.p if act else None, act.ld if act else 0, pooled.p if pooled else None]
    tail = [rows.p if rows else None, rows.ld if rows else 0, n, h, w, c, f, G.CODE[kind], E.st]
    if amax:
        E.check(E.lib.satcv_bn_relu_pool_amax(*args, am.data_ptr(), *tail))
    else:
        E.check(E.lib.satcv_bn_relu_pool(*args, *tail))
    G.sync()
    ref_act = B.act_of(y, sc, sh, kind)
    a64 = np.maximum(B.pre_act(y, sc, sh), 0.0)
    amb = B.ambiguous(y, sc, sh, kind, f)
    loose = amb['sign'] | amb['rnd']
    ebound = 2 * U * (np.abs(y * sc) + np.abs(sh))                        # one product and one sum, or one fma
    if act:
        got = act.get().reshape(shape)
        assert act.untouched_outside(), f'{what}: act wrote outside its channels'
        if regime == 'lattice':
            assert np.array_equal(got, ref_act), f'{what}: act'
        elif kind == 'f32':
            frac(f'{what} act', np.abs(got - a64)[~loose], ebound[~loose])
        else:
            ok = (got == ref_act) | amb['sign'] | (amb['rnd'] & (np.abs(got - ref_act) <= B.bf16_ulp(ref_act)))
            assert ok.all(), f'{what}: act differs at {int((~ok).sum())} outputs outside the ambiguity rule'
    if pooled:
        gp = pooled.get()
        if npool == 0:
            assert np.array_equal(G.raw(pooled.t), pooled.before), f'{what}: pooled written although no whole window exists'
        else:
            gp = gp.reshape(n, hp, wp, c)
            ref_pool = B.maxpool(ref_act, f)
            if regime == 'lattice':
                assert np.array_equal(gp, ref_pool), f'{what}: pooled'
            else:
                clean = ~B.windows(loose, f).any(3)
                if kind == 'f32':
                    frac(f'{what} pooled', np.abs(gp - B.maxpool(a64, f))[clean], B.windows(ebound, f).max(3)[clean])
                else:
                    assert np.array_equal(gp[clean], ref_pool[clean]), f'{what}: pooled'
            if act:      # relations on the kernel's own outputs
                assert np.array_equal(gp, B.maxpool(got, f)), f'{what}: pooled is not the max-pool of the stored act'
    if amax:
        ga = am.cpu().numpy()
        if npool == 0:
            assert (ga == 0xEE).all()
        else:
            ga = ga.reshape(n, hp, wp, c)
            if regime == 'lattice':
                assert np.array_equal(ga, B.first_argmax(ref_act, f)), f'{what}: amax'
            else:
                clean = ~(B.windows(loose, f).any(3) | amb['tie'])
                assert np.array_equal(ga[clean], B.first_argmax(ref_act, f)[clean]), f'{what}: amax'
            if act:
                assert np.array_equal(ga, B.first_argmax(got, f)), f'{what}: amax is not the first maximum of the stored act'
    if rows:
        s = rows.added()
        r1, r2 = B.act_stats(ref_act)
        delta = np.where(amb['rnd'], B.bf16_ulp(ref_act), 0.0) + np.where(amb['sign'], amb['b'], 0.0) + (ebound if kind == 'f32' else 0.0)
        delta = delta if regime == 'random' else np.zeros_like(delta)
        flat = lambda v: v.reshape(-1, c).sum(0)                           # noqa: E731
        check_sum(f'{what} sum', s[0], r1, ref_act, regime, slack=flat(delta))
        # the squares: one more rounding per term
        check_sum(f'{what} sum of squares', s[1], r2, ref_act * ref_act, regime, slack=flat(2 * ref_act * delta + delta * delta), per_term=1)


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('kind', B.KINDS)
@pytest.mark.parametrize('case', B.pool_cases(), ids=B.case_id)
def test_bn_relu_pool(case, kind, regime):
    check_pool(case, kind, regime)


# ---------------------------------------------------------------------- bn_bwd_reduce, bn_bwd_apply
class BwdSetup:
    """device tensors and the descriptor of one case; `widen`: every tensor inside a wider buffer (NaN around the inputs)"""

    def __init__(self, case, kind, regime, key=None):
        self.case, self.kind, self.regime = case, kind, regime
        shape, f = case['shape'], case['f']
        n, h, w, c = shape
        self.shape, self.c, self.npix = shape, c, n * h * w
        split, widen = case['split'], case['wide']
        self.d = d = B.make_inputs(shape, f, kind, regime, key or B.case_id(case), B.skip_channels(case))
        nan = float('nan')
        y2 = d['y'].reshape(-1, c)
        self.y0 = Buf(y2[:, :split] if split else y2, kind, widen, nan)
        self.y1 = Buf(y2[:, split:], kind, widen, nan) if split else None
        self.da = Buf(d['da'].reshape(-1, c), kind, widen, nan) if case['da'] else None
        self.dp = Buf(d['dpool'].reshape(-1, c) if d['dpool'].size else np.zeros((1, c)), kind, widen, nan) if case['dpool'] else None
        self.vec = {k: G.f32dev(d[k]) for k in ('scale', 'shift', 'mean', 'rstd')}
        self.coef = G.f32dev(np.concatenate([d['c1'], d['c2']]))                    # [c1 | c2] over the whole c
        D = desc_type()
        self.desc = D(da=self.da.p if self.da else None, ldda=self.da.ld if self.da else 0, dpool=self.dp.p if self.dp else None,
                      lddp=self.dp.ld if self.dp else 0, f=f, yraw=self.y0.p, ldy=self.y0.ld, scale=self.vec['scale'].data_ptr(),
                      shift=self.vec['shift'].data_ptr(), mean=self.vec['mean'].data_ptr(), rstd=self.vec['rstd'].data_ptr(), n=n, h=h, w_=w, c=c,
                      dtype=G.CODE[kind], linear=case['linear'], c_split=split)
        if split:
            self.desc.yraw1, self.desc.ldy1 = self.y1.p, self.y1.ld
        self.g = B.bwd_g(d['y'], d['scale'], d['shift'], d['da'] if case['da'] else None, d['dpool'] if case['dpool'] else None, f, kind, case['linear'])
        self.xh = B.xhat_of(d['y'], d['mean'], d['rstd'])
        self.what = f'{B.case_id(case)} {kind} {regime}'
        # what the ambiguity rule lets differ (random inputs): the mask of a pixel, the routing inside a window
        self.px_loose = np.zeros(shape, bool)
        self.slack1 = self.slack2 = np.zeros(c)
        if regime == 'random':
            amb = B.ambiguous(d['y'], d['scale'], d['shift'], kind, f if case['dpool'] else 1)
            sign = amb['sign'] & (not case['linear'])
            routed = moved = np.zeros(shape)
            if case['dpool']:
                first = B.first_argmax(B.act_of(d['y'], d['scale'], d['shift'], kind), f)
                routed = np.abs(B.unpool(d['dpool'], first, f, shape))
                moved = B.unpool(np.abs(d['dpool']) * amb['tie'], first, f, shape)          # |dpool| of a window whose arg-max may differ, once
                self.px_loose = B.spread_windows(amb['tie'], f, shape)
            self.px_loose = self.px_loose | sign
            lost = np.where(sign, (np.abs(d['da']) if case['da'] else 0.0) + routed, 0.0)    # a pixel whose mask may flip: its whole gradient
            self.slack1 = (lost + moved).reshape(-1, c).sum(0)
            self.slack2 = (lost * np.abs(self.xh)).reshape(-1, c).sum(0) + 2 * moved.reshape(-1, c).sum(0) * np.abs(self.xh).max((0, 1, 2))


def check_reduce(S):
    case, c = S.case, S.c
    rows = Rows(c, case['wide'])
    S.desc.sums, S.desc.sums_ld = rows.p, rows.ld
    E.check(E.lib.satcv_bn_bwd_reduce(S.desc, E.st))
    G.sync()
    s = rows.added()
    r1, r2 = B.bwd_sums(S.g, S.d['y'], S.d['mean'], S.d['rstd'])
    check_sum(f'bn_bwd_reduce {S.what} sum g', s[0], r1, S.g, S.regime, slack=S.slack1)
    # g * xhat: y - mean, times rstd, times g -- three roundings per term, four allowed
    check_sum(f'bn_bwd_reduce {S.what} sum g xhat', s[1], r2, S.g * S.xh, S.regime, slack=S.slack2, per_term=4)
    S.desc.sums, S.desc.sums_ld = None, 0


def check_apply(S):
    case, kind, c, npix, d = S.case, S.kind, S.c, S.npix, S.d
    split, widen = case['split'], case['wide']
    c0 = split or c
    # dy1 == NULL: dy is as wide as the whole concatenation, its channels >= c_split must keep their sentinel
    dy0 = out_buf(npix, c0, kind, widen, ld=(c + (2 * PAD if widen else 0)) if split and not case['dy1'] else None)
    dy1 = out_buf(npix, c - split, kind, widen) if split and case['dy1'] else None
    S.desc.coef, S.desc.dy, S.desc.lddy_out = S.coef.data_ptr(), dy0.p, dy0.ld
    if dy1:
        S.desc.dy1, S.desc.lddy1 = dy1.p, dy1.ld
    pre = ((np.arange(c) % 5) - 2) * 0.5
    dbias = G.f32dev(pre) if case['dbias'] else None
    S.desc.dbias = dbias.data_ptr() if case['dbias'] else None
    sk = Rows(split, widen) if case['sk'] else None
    if sk:
        S.desc.sk_sums, S.desc.sk_sums_ld = sk.p, sk.ld
    E.check(E.lib.satcv_bn_bwd_apply(S.desc, E.st))
    G.sync()
    t = B.bwd_dy(S.g, d['y'], d['scale'], d['mean'], d['rstd'], d['c1'], d['c2']).reshape(-1, c)
    ref = B.store(t, kind)
    assert dy0.untouched_outside(c0) and (dy1 is None or dy1.untouched_outside()), f'bn_bwd_apply {S.what}: wrote outside the dy channels'
    got = np.concatenate([dy0.get(c0)] + ([dy1.get()] if dy1 else []), 1)
    cc = got.shape[1]                                                              # (dy1 == NULL: only the first source's channels exist)
    if S.regime == 'lattice':
        assert np.array_equal(got, ref[:, :cc]), f'bn_bwd_apply {S.what}: dy differs at {int((got != ref[:, :cc]).sum())} outputs'
    else:
        g2, xh2 = S.g.reshape(-1, c), S.xh.reshape(-1, c)
        bound = 8 * U * np.abs(d['scale']) * (np.abs(g2) + np.abs(d['c1']) + np.abs(xh2 * d['c2'])) + (B.bf16_ulp(t) / 2 if kind == 'bf16' else 0.0)
        keep = ~S.px_loose.reshape(-1, c)[:, :cc]
        frac(f'bn_bwd_apply {S.what} dy', np.abs(got - t[:, :cc])[keep], bound[:, :cc][keep])
    if dbias is not None:
        gb = G.host(dbias)
        if S.regime == 'lattice' and B.sum_is_exact(ref):
            assert np.array_equal(gb, pre + ref.sum(0)), f'bn_bwd_apply {S.what}: dbias'
        else:   # a relation on the kernel's own dy: npix + 1 terms with the value the vector held
            frac(f'bn_bwd_apply {S.what} dbias', np.abs(gb - (pre + got.sum(0))), npix * U * (np.abs(got).sum(0) + np.abs(pre)) + 1e-300)
    if sk:
        s = sk.added()
        a0 = d['y'].reshape(-1, c)[:, :split]
        if S.regime == 'lattice':
            r1, r2 = B.skip_sums(ref[:, :split], a0)
        else:
            r1, r2 = B.skip_sums(got[:, :split], a0)                              # relation on the kernel's own dy
        check_sum(f'bn_bwd_apply {S.what} sk sum dy [a > 0]', s[0], r1, ref[:, :split] * (a0 > 0), S.regime)
        check_sum(f'bn_bwd_apply {S.what} sk sum dy a', s[1], r2, ref[:, :split] * a0, S.regime, per_term=1)
        S.desc.sk_sums, S.desc.sk_sums_ld = None, 0
    S.desc.coef = S.desc.dy = S.desc.dy1 = S.desc.dbias = None


def check_bwd(case, kind, regime, reduce=True, apply=True, key=None):
    S = BwdSetup(case, kind, regime, key)
    if reduce:
        check_reduce(S)
    if apply:
        check_apply(S)


@pytest.mark.parametrize('regime', B.REGIMES)
@pytest.mark.parametrize('kind', B.KINDS)
@pytest.mark.parametrize('case', B.bwd_cases(), ids=B.case_id)
def test_bn_bwd(case, kind, regime):
    check_bwd(case, kind, regime)


# ----------------------------------------------------------------------------- past the launch cap
@pytest.mark.parametrize('kind,regime', [('f32', 'lattice'), ('bf16', 'lattice'), ('f32', 'random'), ('bf16', 'random')])
@pytest.mark.parametrize('case', B.cap_cases(), ids=B.case_id)
def test_bn_bwd_past_the_launch_cap(case, kind, regime):
    assert case['shape'][2] >= 2 * G.CAP
    check_bwd(case, kind, regime, reduce=not (case['dbias'] or case['sk']))


@pytest.mark.parametrize('kind,regime', [('f32', 'lattice'), ('bf16', 'random')])
def test_bn_bwd_apply_one_full_unrolled_trip_and_a_tail_of_one(kind, regime):
    case = B.unrolled_tail_case()
    assert case['shape'][2] == 4 * G.CAP + 1
    check_bwd(case, kind, regime, reduce=False)


@pytest.mark.parametrize('kind,regime', [('f32', 'lattice'), ('bf16', 'lattice'), ('f32', 'random'), ('bf16', 'random')])
def test_bn_relu_pool_past_the_launch_cap(kind, regime):
    check_pool(((1, 1, G.rows_past_cap(1), 8), 1, 0, 'yes', 0, 1), kind, regime)


# ------------------------------------------------------------------------------- child processes
def run_small_grid_child():
    """SATCV_EW_PER_CU=1: 256 workgroups.  The 2x2 pool path, the one-pass pooled reduce (its grid sized for 8 items per thread) and the
    pooled apply past the cap at c = 24, and the four-pixel apply loop with a full trip and a tail of one"""
    cap = B.grid_cap_threads(1)
    assert os.environ.get('SATCV_EW_PER_CU') == '1'
    assert E.lib.satcv_bias_grad_workspace(10 ** 6, 8) == 256 * 8 * 4, 'the launch cap did not follow SATCV_EW_PER_CU'
    side = 2 * (int(np.sqrt(2 * cap / 3)) + 2)                                     # windows * 3 groups >= 2 cap
    assert (side // 2) ** 2 * 3 >= 2 * cap
    big = 2 * (int(np.sqrt(8 * cap / 3)) + 2)                                      # windows * 3 groups / 8 > cap
    assert (big // 2) ** 2 * 3 > 8 * cap
    for kind, regime in [('f32', 'lattice'), ('bf16', 'random')]:
        check_pool(((1, side, side, 24), 2, 1, 'yes', 1, 1), kind, regime)
        check_pool(((1, side, side, 24), 2, 0, 'wide', 1, 1), kind, regime)
        check_bwd(B.bwd_case((1, side, side, 24), f=2, dpool=1, dbias=1), kind, regime, reduce=False)
        check_bwd(B.bwd_case((1, big, big, 24) if regime == 'lattice' else (1, side, side, 24), f=2, dpool=1), kind, regime, apply=False)
        for case in (B.cap_cases(1) if regime == 'lattice' else []) + [B.unrolled_tail_case(1), dict(B.unrolled_tail_case(1), dbias=1)]:
            check_bwd(case, kind, regime)
        t = B.unrolled_tail_case(1)['shape'][2]
        check_bwd(B.bwd_case((1, 1, t, 16), split=8, sk=1), kind, regime, reduce=False)
    print('small-grid child ok')


def run_round3_apply_child():
    """SATCV_BN_APPLY=0 SATCV_BN_REV=0: the round-3 apply loop in forward pixel order on every apply case of the table -- on lattice inputs
    against the very oracle values the default process is held to, bit for bit: the switch selects the same function"""
    from satellite_computervision_amd import _lib
    for env, key in (('SATCV_BN_APPLY', b'bn_apply'), ('SATCV_BN_REV', b'bn_rev')):
        v = G.C.c_int32(-1)
        assert os.environ.get(env) == '0' and _lib.lib.satcv_get_option(key, G.C.byref(v)) == 0 and v.value == 0, env
    for case in B.bwd_cases() + B.cap_cases():
        for kind in B.KINDS:
            for regime in B.REGIMES:
                if case['shape'][2] > 10 ** 5 and (kind, regime) not in (('f32', 'lattice'), ('bf16', 'random')):
                    continue
                check_bwd(case, kind, regime, reduce=False)
    print('round-3 apply child ok')


def _child(fn, env, timeout):
    """a fresh process with its own time limit, exit status checked, nothing started after it"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_bn_kernels_gpu as T; T.%s()' % (ROOT, HERE, fn)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    figs = [ln for ln in r.stdout.splitlines() if ln.startswith('[fig]')]
    print('\n'.join(sorted(figs, key=lambda ln: -float(ln.rsplit(': ', 1)[1].split(' ')[0]))[:40]))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.strip().splitlines()[-1]


def test_bn_kernels_with_one_workgroup_per_cu():
    assert _child('run_small_grid_child', {'SATCV_EW_PER_CU': '1'}, 300) == 'small-grid child ok'


def test_bn_apply_round3_loop_in_forward_order_is_the_same_function():
    assert _child('run_round3_apply_child', {'SATCV_BN_APPLY': '0', 'SATCV_BN_REV': '0'}, 300) == 'round-3 apply child ok'


# ------------------------------------------------------------------------------ finalize kernels
def rel(what, got, ref, k, mag=None):
    """|got - ref| <= k u mag per value (mag: the magnitude the roundings act on; |ref| unless the formula cancels)"""
    mag = np.abs(ref) if mag is None else mag
    frac(what, np.abs(np.asarray(got, np.float64) - ref), k * U * mag + 1e-300)


def f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


@pytest.mark.parametrize('case', B.FINALIZE_CASES, ids=lambda t: 'c%d-pad%d-u%d-b%d-n%g-mv%d' % t)
def test_bn_finalize_train(case):
    c, pad, updates, bessel, count, moving = case
    eps, mom = 1e-3, 0.99
    rng = np.random.default_rng(c * 7 + updates)
    rows = B.stat_rows_of(count, c, c + updates)
    ld = c + pad
    buf = np.full((B.STAT_ROWS, 2, ld), SENT)
    buf[:, :, :c] = rows
    rt = torch.tensor(buf, dtype=torch.float64).cuda()
    gamma, beta, mm0, mv0 = f32(rng.uniform(0.5, 1.5, c)), f32(rng.standard_normal(c)), f32(rng.standard_normal(c)), f32(rng.uniform(0.5, 2.0, c))
    gd, bd, mmd, mvd = (G.f32dev(v) for v in (gamma, beta, mm0, mv0))
    outs = [G.f32dev(np.full(c + 3, SENT)) for _ in range(4)]
    E.check(E.lib.satcv_bn_finalize_train(rt.data_ptr(), ld, c, count, gd.data_ptr(), bd.data_ptr(), eps, mom, updates, bessel,
                                          mmd.data_ptr() if moving else None, mvd.data_ptr() if moving else None, *[o.data_ptr() for o in outs], E.st))
    G.sync()
    ref = B.finalize_train(rows[:, 0].sum(0), rows[:, 1].sum(0), count, gamma, beta, eps, f32(mom), updates, bessel, mm0, mv0)
    scale, shift, mean, rstd = (G.host(o) for o in outs)
    assert all((v[c:] == SENT).all() for v in (scale, shift, mean, rstd)), 'wrote past channel c'
    now = rt.cpu().numpy()
    assert (now[:, :, :c] == 0).all() and (now[:, :, c:] == SENT).all(), 'rows: zero below c, untouched from c on'
    what = 'bn_finalize_train c=%d pad=%d updates=%d bessel=%d count=%g' % case[:5]
    rel(f'{what} mean', mean[:c], ref['mean'], 1)                                   # k = 1: the conversion of the double quotient
    # var: 1 (conversion); + eps: 1; rsqrtf: 4 -- relative to var + eps the first two weigh half each through the root: k = 6 is a ceiling
    rel(f'{what} rstd', rstd[:c], ref['rstd'], 6)
    rel(f'{what} scale', scale[:c], ref['scale'], 7)                                # rstd (6) and one product
    # shift = beta - mean * scale: mean (1), scale (7), product (1) on |mean scale|; the difference (1) on the result
    rel(f'{what} shift', shift[:c], ref['shift'], 10, np.abs(beta) + np.abs(ref['mean'] * ref['scale']))
    if moving:
        # per update: 1 - momentum (1), two products (2), one sum (1) on |moving| + |batch|; the batch value itself: mean 1; variance 1 (+ 3
        # for the Bessel factor: a difference, a quotient, a product)
        rel(f'{what} moving mean', G.host(mmd), ref['mm'], 4 * updates + 1, np.abs(mm0) + np.abs(ref['mean']))
        rel(f'{what} moving variance', G.host(mvd), ref['mv'], 4 * updates + 4, np.abs(mv0) + np.abs(ref['vv']))
    if count == 1.0:
        assert (rstd[:c] == rstd[0]).all() and abs(rstd[0] - 1 / np.sqrt(eps)) <= 6 * U / np.sqrt(eps), 'one sample: the variance is clamped at 0'


@pytest.mark.parametrize('two', [0, 1], ids=['finalize', 'finalize2'])
@pytest.mark.parametrize('c,pad', [(1, 0), (5, 3), (13, 0), (32, 8), (1000, 24)])
def test_bn_bwd_finalize(c, pad, two):
    count = 189.0
    rng = np.random.default_rng(c + two)
    ld = c + pad
    sc, sh, mu, rs = f32(rng.standard_normal(c)), f32(rng.standard_normal(c)), f32(rng.standard_normal(c)), f32(rng.uniform(0.5, 2.0, c))
    sc[c // 2] = 0.0                                                                # a zero scale channel: its activated rows convert to 0
    vd = [G.f32dev(v) for v in (sc, sh, mu, rs)]
    for accumulate, with_dg, with_db, with_raw in [(0, 1, 1, 1), (1, 1, 1, 1), (0, 0, 1, 1), (1, 1, 0, 1), (0, 1, 1, 0), (1, 0, 0, 0)]:
        if not two and not with_raw:
            continue
        raw_rows, act_rows = B.random_rows(c, c + accumulate), B.random_rows(c, c + 17 + accumulate)

        def place(r):
            buf = np.full((B.STAT_ROWS, 2, ld), SENT)
            buf[:, :, :c] = r
            return torch.tensor(buf, dtype=torch.float64).cuda()
        rt, at = place(raw_rows), place(act_rows)
        dg0, db0 = f32(rng.standard_normal(c) * 30), f32(rng.standard_normal(c) * 30)
        dg, db, coef = G.f32dev(dg0), G.f32dev(db0), G.f32dev(np.full(2 * c + 3, SENT))
        if two:
            E.check(E.lib.satcv_bn_bwd_finalize2(rt.data_ptr() if with_raw else None, ld, at.data_ptr(), ld, c, count, *[v.data_ptr() for v in vd],
                                                 dg.data_ptr() if with_dg else None, db.data_ptr() if with_db else None, coef.data_ptr(), accumulate, E.st))
            ref = B.bwd_finalize2(raw_rows[:, 0].sum(0) if with_raw else None, raw_rows[:, 1].sum(0) if with_raw else None, act_rows[:, 0].sum(0),
                                  act_rows[:, 1].sum(0), count, sc, sh, mu, rs, dg0, db0, accumulate)
        else:
            E.check(E.lib.satcv_bn_bwd_finalize(rt.data_ptr(), ld, c, count, dg.data_ptr() if with_dg else None, db.data_ptr() if with_db else None,
                                                coef.data_ptr(), accumulate, E.st))
            ref = B.bwd_finalize(raw_rows[:, 0].sum(0), raw_rows[:, 1].sum(0), count, dg0, db0, accumulate)
        G.sync()
        what = f'bn_bwd_finalize{2 if two else ""} c={c} pad={pad} acc={accumulate} dgamma={with_dg} dbeta={with_db} raw={with_raw}'
        for t, used in ((rt, with_raw or not two), (at, two)):
            now = t.cpu().numpy()
            if used:
                assert (now[:, :, :c] == 0).all() and (now[:, :, c:] == SENT).all(), f'{what}: rows zero below c, untouched from c on'
        # the sums are formed in double and converted once (k = 1); accumulate adds once more, on |old| + |sum|
        s1, s2 = ref['c1'] * count, ref['c2'] * count
        k = 2 if accumulate else 1
        # finalize2 forms (sum g a - (shift + scale mean) sum g) rstd / scale in double: 8 units of 2^-53 on the magnitude of its terms
        tiny = 0.0
        if two:
            a1, a2 = np.abs(act_rows[:, 0]).sum(0), np.abs(act_rows[:, 1]).sum(0)
            tiny = 8 * 2.0 ** -53 * np.where(sc != 0, (a2 + (np.abs(sh) + np.abs(sc * mu)) * a1) * np.abs(rs / np.where(sc != 0, sc, 1.0)), 0.0)
        if with_db:
            rel(f'{what} dbeta', G.host(db), ref['dbeta'], k, np.abs(db0) * accumulate + np.abs(s1))
        else:
            assert np.array_equal(G.host(db), db0)
        if with_dg:
            rel(f'{what} dgamma', G.host(dg), ref['dgamma'], k, np.abs(dg0) * accumulate + np.abs(s2) + tiny / U)
        else:
            assert np.array_equal(G.host(dg), dg0)
        cf = G.host(coef)
        assert (cf[2 * c:] == SENT).all()
        rel(f'{what} c1', cf[:c], ref['c1'], 2)                                     # conversion and quotient
        rel(f'{what} c2', cf[c:2 * c], ref['c2'], 2, np.abs(ref['c2']) + tiny / U / count)


def test_bn_bwd_finalize_of_lattice_sums_is_exact():
    """the reduce pass of a lattice case, then the finalize: dgamma, dbeta exactly the oracle's sums, coef their correctly rounded quotients"""
    case = B.bwd_case((3, 7, 9, 40), f=2, dpool=1)
    for kind in B.KINDS:
        S = BwdSetup(case, kind, 'lattice')
        rows = Rows(S.c, False, prefill=False)
        S.desc.sums, S.desc.sums_ld = rows.p, rows.ld
        E.check(E.lib.satcv_bn_bwd_reduce(S.desc, E.st))
        dg, db, coef = (G.f32dev(np.zeros(n)) for n in (S.c, S.c, 2 * S.c))
        E.check(E.lib.satcv_bn_bwd_finalize(rows.p, rows.ld, S.c, float(S.npix), dg.data_ptr(), db.data_ptr(), coef.data_ptr(), 0, E.st))
        G.sync()
        r1, r2 = B.bwd_sums(S.g, S.d['y'], S.d['mean'], S.d['rstd'])
        assert B.sum_is_exact(S.g) and B.sum_is_exact(S.g * S.xh)
        assert np.array_equal(G.host(db), r1) and np.array_equal(G.host(dg), r2)
        want = np.concatenate([r1, r2]).astype(np.float32) / np.float32(S.npix)     # IEEE float32 division, as the device's
        assert np.array_equal(G.host(coef), want.astype(np.float64))
        assert (rows.slice_now() == 0).all()


@pytest.mark.parametrize('batched', [0, 1])
def test_bn_affine_infer(batched):
    eps = 1e-3
    rng = np.random.default_rng(11 + batched)
    jobs, table, keep = [], [], []
    for i, c in enumerate((5, 256, 1000)):                                          # 5 and 1000: no multiple of either block size
        v = dict(gamma=f32(rng.standard_normal(c)), beta=f32(rng.standard_normal(c)), mm=f32(rng.standard_normal(c)), mv=f32(rng.uniform(0.05, 3.0, c)),
                 bias=f32(rng.standard_normal(c)))
        dv = {k: G.f32dev(x) for k, x in v.items()}
        out = {k: G.f32dev(np.full(c + 3, SENT)) for k in ('scale', 'shift', 'bias_eff')}
        keep.append((dv, out))
        mode = ['none', 'bias', 'nobias'][i]                                        # bias_eff: not written, with conv_bias, with conv_bias == NULL
        jobs.append((c, v, out, mode))
        table.append([dv['gamma'].data_ptr(), dv['beta'].data_ptr(), dv['mm'].data_ptr(), dv['mv'].data_ptr(), out['scale'].data_ptr(), out['shift'].data_ptr(), c,
                      dv['bias'].data_ptr() if mode == 'bias' else 0, out['bias_eff'].data_ptr() if mode != 'none' else 0])
    if batched:
        tab = torch.tensor(table, dtype=torch.int64).cuda()
        E.check(E.lib.satcv_bn_affine_infer_batched(tab.data_ptr(), len(table), eps, E.st))
    else:
        for row in table:
            E.check(E.lib.satcv_bn_affine_infer(row[0], row[1], row[2], row[3], eps, row[6], row[4], row[5], E.st))
    G.sync()
    for c, v, out, mode in jobs:
        ref = B.affine_infer(v['gamma'], v['beta'], v['mm'], v['mv'], eps, v['bias'] if mode == 'bias' else None)
        sc, sh, be = (G.host(out[k]) for k in ('scale', 'shift', 'bias_eff'))
        assert (sc[c:] == SENT).all() and (sh[c:] == SENT).all() and (be[c:] == SENT).all()
        what = f'bn_affine_infer batched={batched} c={c}'
        rel(f'{what} scale', sc[:c], ref['scale'], 7)                               # + eps (1), sqrtf (1 + 4), the quotient (1)
        rel(f'{what} shift', sh[:c], ref['shift'], 9, np.abs(v['beta']) + np.abs(v['mm'] * ref['scale']))      # scale (7), product (1); the difference (1)
        if batched and mode != 'none':
            # shift (9 on its terms), conv_bias * scale (7 + 1), the sum (1)
            mag = np.abs(v['beta']) + np.abs(v['mm'] * ref['scale']) + (np.abs(v['bias'] * ref['scale']) if mode == 'bias' else 0.0)
            rel(f'{what} bias_eff ({mode})', be[:c], ref['bias_eff'], 10, mag)
            if mode == 'nobias':
                assert np.array_equal(be[:c], sh[:c])
        else:
            assert (be == SENT).all()


# -------------------------------------------------------------------------------------- refusals
def test_bn_relu_pool_refuses_bad_arguments():
    y = G.dev(np.ones((16, 2056)), 'f32')
    v = G.f32dev(np.ones(2056))
    act, pooled = G.dev(np.full((16, 2056), SENT), 'f32'), G.dev(np.full((16, 2056), SENT), 'f32')
    am = torch.full((16, 2056), 0xEE, dtype=torch.uint8).cuda()
    rows = torch.full((B.STAT_ROWS, 2, 8), SENT, dtype=torch.float64).cuda()
    before = [G.raw(act), G.raw(pooled), am.cpu().numpy(), rows.cpu().numpy()]

    def untouched():
        G.sync()
        assert np.array_equal(G.raw(act), before[0]) and np.array_equal(G.raw(pooled), before[1]) and np.array_equal(am.cpu().numpy(), before[2])
        assert np.array_equal(rows.cpu().numpy(), before[3])

    def pool(c=8, f=2, dtype=0, stats_ld=8, stats=True, n=1, h=4, w=4):
        return E.lib.satcv_bn_relu_pool(y.data_ptr(), v.data_ptr(), v.data_ptr(), act.data_ptr(), 0, pooled.data_ptr(), rows.data_ptr() if stats else None, stats_ld,
                                        n, h, w, c, f, dtype, E.st)

    def pool_amax(c=8, f=2, dtype=0, pooled_=True, amax_=True, h=4, w=4):
        return E.lib.satcv_bn_relu_pool_amax(y.data_ptr(), v.data_ptr(), v.data_ptr(), act.data_ptr(), 0, pooled.data_ptr() if pooled_ else None,
                                             am.data_ptr() if amax_ else None, None, 0, 1, h, w, c, f, dtype, E.st)
    for rc in (pool(c=12), pool(c=2056, stats=False), pool(dtype=2), pool(f=0), pool(f=-1), pool(c=16, stats_ld=8), pool(n=0),
               pool_amax(c=12), pool_amax(c=2056), pool_amax(dtype=2), pool_amax(f=0), pool_amax(f=16, h=16, w=16), pool_amax(pooled_=False), pool_amax(amax_=False)):
        G.refused(rc)
        untouched()
    assert pool_amax(f=15, h=16, w=1) == 0                                          # 225 positions fit the byte
    G.sync()


def test_bn_bwd_refuses_bad_arguments():
    c, npix = 16, 16
    D = desc_type()
    y, da = G.dev(np.ones((npix, 2056)), 'f32'), G.dev(np.ones((npix, 2056)), 'f32')
    dy = G.dev(np.full((npix, 2056), SENT), 'f32')
    v = G.f32dev(np.ones(2 * 2056))
    rows = torch.full((B.STAT_ROWS, 2, c), SENT, dtype=torch.float64).cuda()
    dbias = G.f32dev(np.full(2056, SENT))
    before = [G.raw(dy), rows.cpu().numpy(), G.raw(dbias)]

    def base(**kw):
        d = D(da=da.data_ptr(), ldda=2056, f=2, yraw=y.data_ptr(), ldy=2056, scale=v.data_ptr(), shift=v.data_ptr(), mean=v.data_ptr(), rstd=v.data_ptr(),
              n=1, h=4, w_=4, c=c, dtype=0, sums=rows.data_ptr(), sums_ld=c, coef=v.data_ptr(), dy=dy.data_ptr(), lddy_out=2056)
        for k, x in kw.items():
            setattr(d, k, x)
        return d
    two = dict(c_split=8, yraw1=y.data_ptr(), ldy1=2056, dy1=dy.data_ptr(), lddy1=2056)
    both = [dict(c=12), dict(c=2056), dict(dtype=2), dict(da=None), dict(dpool=da.data_ptr(), lddp=2056, f=0), dict(two, c_split=4), dict(two, c_split=16),
            dict(two, c_split=24), dict(two, dpool=da.data_ptr(), lddp=2056), dict(two, dbias=dbias.data_ptr()), dict(two, yraw1=None), dict(n=0), dict(yraw=None)]
    apply_only = [dict(sk_sums=rows.data_ptr(), sk_sums_ld=c), dict(two, sk_sums=rows.data_ptr(), sk_sums_ld=4), dict(coef=None), dict(dy=None)]
    reduce_only = [dict(sums=None), dict(sums_ld=8)]
    for kw in both + reduce_only:
        G.refused(E.lib.satcv_bn_bwd_reduce(base(**kw), E.st))
    for kw in both + apply_only:
        G.refused(E.lib.satcv_bn_bwd_apply(base(**kw), E.st))
    G.sync()
    assert np.array_equal(G.raw(dy), before[0]) and np.array_equal(rows.cpu().numpy(), before[1]) and np.array_equal(G.raw(dbias), before[2])


def test_bn_finalize_and_affine_refuse_bad_arguments():
    c = 8
    rows = torch.full((B.STAT_ROWS, 2, c), 3.0, dtype=torch.float64).cuda()
    v = G.f32dev(np.ones(c))
    out = G.f32dev(np.full(2 * c, SENT))
    before = [rows.cpu().numpy(), G.raw(out)]
    p, o, r = v.data_ptr(), out.data_ptr(), rows.data_ptr()
    lib = E.lib
    calls = [lib.satcv_bn_finalize_train(r, 4, c, 16.0, p, p, 1e-3, 0.99, 1, 0, None, None, o, o, o, o, E.st),                 # stats_ld < c
             lib.satcv_bn_finalize_train(r, c, c, 0.0, p, p, 1e-3, 0.99, 1, 0, None, None, o, o, o, o, E.st),                 # count <= 0
             lib.satcv_bn_finalize_train(r, c, c, -1.0, p, p, 1e-3, 0.99, 1, 0, None, None, o, o, o, o, E.st),
             lib.satcv_bn_finalize_train(r, c, 0, 16.0, p, p, 1e-3, 0.99, 1, 0, None, None, o, o, o, o, E.st),
             lib.satcv_bn_bwd_finalize(r, 4, c, 16.0, o, o, o, 0, E.st), lib.satcv_bn_bwd_finalize(r, c, c, 0.0, o, o, o, 0, E.st),
             lib.satcv_bn_bwd_finalize(r, c, c, 16.0, o, o, None, 0, E.st), lib.satcv_bn_bwd_finalize(None, c, c, 16.0, o, o, o, 0, E.st),
             lib.satcv_bn_bwd_finalize2(r, 4, r, c, c, 16.0, p, p, p, p, o, o, o, 0, E.st), lib.satcv_bn_bwd_finalize2(r, c, r, 4, c, 16.0, p, p, p, p, o, o, o, 0, E.st),
             lib.satcv_bn_bwd_finalize2(r, c, None, c, c, 16.0, p, p, p, p, o, o, o, 0, E.st), lib.satcv_bn_bwd_finalize2(None, 0, r, c, c, 0.0, p, p, p, p, o, o, o, 0, E.st),
             lib.satcv_bn_affine_infer(p, p, p, p, 1e-3, 0, o, o, E.st), lib.satcv_bn_affine_infer(p, p, p, None, 1e-3, c, o, o, E.st),
             lib.satcv_bn_affine_infer_batched(r, 0, 1e-3, E.st), lib.satcv_bn_affine_infer_batched(r, -1, 1e-3, E.st),     # njobs <= 0
             lib.satcv_bn_affine_infer_batched(None, 1, 1e-3, E.st)]
    for rc in calls:
        G.refused(rc)
    G.sync()
    assert np.array_equal(rows.cpu().numpy(), before[0]) and np.array_equal(G.raw(out), before[1])
