"""NumPy float64 restatements of the BatchNorm kernel family of csrc/elementwise.hip (satcv_bn_relu_pool[_amax], satcv_bn_bwd_reduce /
_apply, satcv_bn_finalize_train, satcv_bn_bwd_finalize[2], satcv_bn_affine_infer[_batched]), written from the formulas of include/satcv.h
(helper module, no tests in it), the two input regimes and the case tables that tests/test_bn_kernels_cpu.py and
tests/test_bn_kernels_gpu.py both iterate over.

Lattice inputs: small dyadic values on which every float32 operation of either association of the formulas (mul then add, or fma; the
c1 / c2 form or the k1 = scale c1, k2 = scale rstd c2 form) is exact, so the stored outputs are the same bits whatever the kernel's
order -- the checks are equalities.  Random inputs: normal values, the checks are derived bounds, and `ambiguous` marks the outputs
whose value hangs on a decision (ReLU mask, bf16 rounding, arg-max) that a float32 rounding of a = scale y + shift can flip.

All tensors are NHWC float64 arrays whose values the storage type under test holds exactly."""
import numpy as np

from elementwise_oracle import bf16_round, grid_cap_threads, to_storage  # noqa: F401  (one definition of the storage rounding)

U24 = 2.0 ** -24
STAT_ROWS = 32
KINDS = ['f32', 'bf16']
REGIMES = ['lattice', 'random']


def store(x64, kind):
    """float64 -> float32 -> storage type, as float64"""
    return to_storage(np.asarray(x64, np.float64).astype(np.float32), kind)


def bf16_ulp(x64):
    """spacing of bfloat16 at |x| (8 significant bits)"""
    ax = np.maximum(np.abs(np.asarray(x64, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(ax)) - 7)


# --------------------------------------------------------------------------------------- forward
def pre_act(y, scale, shift):
    return y * scale + shift


def act_of(y, scale, shift, kind):
    """act = store(relu(scale * y + shift))"""
    return store(np.maximum(pre_act(y, scale, shift), 0.0), kind)


def windows(x, f):
    """(n, h, w, c) -> (n, h // f, w // f, f * f, c): the whole ('valid') windows, positions in row-major order i * f + j"""
    n, h, w, c = x.shape
    hp, wp = h // f, w // f
    return x[:, :hp * f, :wp * f].reshape(n, hp, f, wp, f, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, hp, wp, f * f, c)


def maxpool(act, f):
    n, h, w, c = act.shape
    return windows(act, f).max(3) if h >= f and w >= f else np.zeros((n, h // f, w // f, c))


def first_argmax(act, f):
    """position i * f + j of the first maximum of every whole window (np.argmax returns the first)"""
    n, h, w, c = act.shape
    return windows(act, f).argmax(3).astype(np.uint8) if h >= f and w >= f else np.zeros((n, h // f, w // f, c), np.uint8)


def act_stats(act):
    a = act.reshape(-1, act.shape[-1])
    return a.sum(0), (a * a).sum(0)


def unpool(dpool, amax, f, shape):
    """dpool routed to the arg-max position of its window, zero elsewhere (and in the border a partial window covers)"""
    n, h, w, c = shape
    hp, wp = h // f, w // f
    out = np.zeros(shape)
    if hp == 0 or wp == 0:
        return out
    onehot = np.arange(f * f).reshape(1, 1, 1, f * f, 1) == amax[:, :, :, None, :]
    r = (onehot * dpool[:, :, :, None, :]).reshape(n, hp, wp, f, f, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, hp * f, wp * f, c)
    out[:, :hp * f, :wp * f] = r
    return out


# -------------------------------------------------------------------------------------- backward
def bwd_g(y, scale, shift, da, dpool, f, kind, linear=False):
    """g = (da + unpool(dpool by the first arg-max of the stored act)) * [scale * y + shift > 0 or linear]"""
    g = np.zeros(y.shape) if da is None else da.copy()
    if dpool is not None:
        g = g + unpool(dpool, first_argmax(act_of(y, scale, shift, kind), f), f, y.shape)
    return g if linear else g * (pre_act(y, scale, shift) > 0)


def xhat_of(y, mean, rstd):
    return (y - mean) * rstd


def bwd_sums(g, y, mean, rstd):
    """sum g, sum g * xhat per channel"""
    c = y.shape[-1]
    return g.reshape(-1, c).sum(0), (g * xhat_of(y, mean, rstd)).reshape(-1, c).sum(0)


def bwd_dy(g, y, scale, mean, rstd, c1, c2):
    """scale * (g - c1 - xhat * c2), unrounded"""
    return scale * (g - c1 - xhat_of(y, mean, rstd) * c2)


def skip_sums(dy0, a0):
    """the activated-form sums over the skip channels: sum dy [a > 0], sum dy * a"""
    c = a0.shape[-1]
    return (dy0 * (a0 > 0)).reshape(-1, c).sum(0), (dy0 * a0).reshape(-1, c).sum(0)


# -------------------------------------------------------------------------------------- finalize
def finalize_train(s1, s2, count, gamma, beta, eps, momentum, updates, bessel, mm=None, mv=None):
    mean = s1 / count
    var = np.maximum(s2 / count - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * rstd
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale)
    if mm is not None:
        vv = var * (count / max(count - 1.0, 1.0)) if bessel else var
        a, b = np.asarray(mm, np.float64).copy(), np.asarray(mv, np.float64).copy()
        for _ in range(updates):
            a, b = a * momentum + mean * (1.0 - momentum), b * momentum + vv * (1.0 - momentum)
        out.update(mm=a, mv=b, vv=vv)
    return out


def bwd_finalize(s1, s2, count, dgamma0=None, dbeta0=None, accumulate=0):
    return dict(dbeta=s1 + (dbeta0 if accumulate else 0.0), dgamma=s2 + (dgamma0 if accumulate else 0.0), c1=s1 / count, c2=s2 / count)


def act_to_raw_sum(a1, a2, scale, shift, mean, rstd):
    """sum g xhat from the activated-form sums: (sum g a - (shift + scale mean) sum g) rstd / scale, 0 where scale == 0"""
    safe = np.where(scale != 0, scale, 1.0)
    return np.where(scale != 0, (a2 - (shift + scale * mean) * a1) * (rstd / safe), 0.0)


def bwd_finalize2(d1, d2, a1, a2, count, scale, shift, mean, rstd, dgamma0=None, dbeta0=None, accumulate=0):
    d1 = 0.0 if d1 is None else d1
    d2 = 0.0 if d2 is None else d2
    return bwd_finalize(d1 + a1, d2 + act_to_raw_sum(a1, a2, scale, shift, mean, rstd), count, dgamma0, dbeta0, accumulate)


def affine_infer(gamma, beta, mm, mv, eps, conv_bias=None):
    scale = gamma / np.sqrt(mv + eps)
    shift = beta - mm * scale
    return dict(scale=scale, shift=shift, bias_eff=shift + (0.0 if conv_bias is None else conv_bias * scale))


# ---------------------------------------------------------------------------------------- inputs
def _seed(*key):
    """a seed per case: from the case's own description, stable across processes"""
    s = 0
    for ch in repr(key).encode():
        s = (s * 131 + ch) % (2 ** 31 - 1)
    return s


# random cases whose first seed put more than 1e-3 of their outputs under the ambiguity rule (tests/test_bn_kernels_cpu.py holds every
# case to that cap): the seed was replaced, the cap was not
RESEED = {('3x7x9x8-f2-act_wide-stats', 'bf16'): 1, ('2x8x8x24-f2-amax-act_wide', 'bf16'): 1, ('2x8x8x40-f2-act_yes-nopooled-stats', 'bf16'): 1,
          ('2x8x8x72-f3-amax-act_yes-stats', 'bf16'): 1, ('3x7x9x72-f4-amax-act_wide-stats', 'bf16'): 1, ('1x2x3x72-f1-split48', 'bf16'): 1,
          ('1x2x3x72-f1-sk-wide-split48', 'bf16'): 1, ('3x7x9x40-f3-noda-dpool-dbias', 'bf16'): 1}


def _lat(rng, shape, k, den):
    return rng.integers(-k, k + 1, shape).astype(np.float64) / den


def make_inputs(shape, f, kind, regime, key, skip_c=0):
    """dict of y, da, dpool (both always made), scale, shift, mean, rstd, c1, c2.  skip_c > 0: the first skip_c channels of y are an
    ACTIVATED tensor (>= 0, about half zeros), as the skip source of the two-source form with sk_sums is."""
    n, h, w, c = shape
    rng = np.random.default_rng(_seed(shape, f, kind, regime, key, RESEED.get((key, kind), 0) if regime == 'random' else 0))
    pshape = (n, h // f, w // f, c)
    if regime == 'lattice':
        y = _lat(rng, shape, 16, 4)
        scale = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], c)
        scale[rng.permutation(c)[:3]] = [0.0, -1.0, -0.5]                  # a zero and negative ones in every case
        d = dict(y=y, scale=scale, rstd=rng.choice([0.5, 1.0, 2.0], c), shift=_lat(rng, c, 8, 4), mean=_lat(rng, c, 4, 4),
                 da=_lat(rng, shape, 8, 4), dpool=_lat(rng, pshape, 8, 4), c1=_lat(rng, c, 4, 8), c2=_lat(rng, c, 4, 8))
    else:
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)       # noqa: E731
        d = dict(y=store(rng.standard_normal(shape) * 1.5 + 0.3, kind), scale=f32(rng.standard_normal(c)), shift=f32(rng.standard_normal(c)),
                 mean=f32(rng.standard_normal(c) * 0.5 + 0.3), rstd=f32(rng.uniform(0.5, 2.0, c)),
                 da=store(rng.standard_normal(shape), kind), dpool=store(rng.standard_normal(pshape), kind),
                 c1=f32(rng.standard_normal(c) * 0.1), c2=f32(rng.standard_normal(c) * 0.1))
    if skip_c:
        d['y'][..., :skip_c] = np.maximum(d['y'][..., :skip_c], 0.0)
    return d


# ------------------------------------------------------------------------ exactness of a lattice case
def _is_f32(x):
    x = np.asarray(x, np.float64)
    return bool(np.all(x.astype(np.float32).astype(np.float64) == x))


def assert_lattice_exact(d, kind, f, linear=False, pooled=True):
    """every intermediate of either association of the forward and backward formulas is a float32 value (24 bits), the inputs and the
    activation are values of the storage type: float64 arithmetic on them is then exactly what float32 computes, whatever the order"""
    y, sc, sh, mu, rs, c1, c2 = (d[k] for k in ('y', 'scale', 'shift', 'mean', 'rstd', 'c1', 'c2'))
    for name in ('y', 'da', 'dpool'):
        assert np.array_equal(store(d[name], kind), d[name]), f'{name} is not a {kind} value'
    a = pre_act(y, sc, sh)
    act = np.maximum(a, 0.0)
    assert np.array_equal(store(act, kind), act), 'act does not fit the storage type'
    g = bwd_g(y, sc, sh, d['da'], d['dpool'] if pooled else None, f, kind, linear)
    ymu = y - mu
    xh = ymu * rs
    k1, k2 = sc * c1, sc * rs * c2
    inter = [y * sc, a, act * act, ymu, xh, g, g * xh, xh * c2, g - c1, g - c1 - xh * c2, bwd_dy(g, y, sc, mu, rs, c1, c2),      # c1 / c2 form
             k1, sc * rs, k2, sc * g, sc * g - k1, k2 * ymu, sc * g - k1 - k2 * ymu]                                              # k1 / k2 form
    assert all(_is_f32(v) for v in inter), 'an intermediate needs more than 24 bits'
    assert np.array_equal(inter[10], inter[-1]), 'the two forms differ on lattice inputs'
    return True


def denominator(x):
    """smallest power of two d with x * d integral (x dyadic)"""
    d = 1.0
    while not np.all(np.asarray(x) * d == np.round(np.asarray(x) * d)):
        d *= 2.0
        assert d <= 2.0 ** 30
    return d


def sum_is_exact(terms):
    """worst case npix * max|term| * denominator < 2^24: every partial sum of the terms, in any order, is a float32 value"""
    t = np.asarray(terms, np.float64)
    npix = t.size // t.shape[-1]
    return bool(npix * np.abs(t).max(initial=0.0) * denominator(t) < 2.0 ** 24)


# ------------------------------------------------------------------------------------- ambiguity
def ambiguous(y, scale, shift, kind, f=1):
    """outputs whose value depends on a decision that the float32 rounding of a = scale * y + shift can flip, with
    b = 4 * 2^-24 (|scale y| + |shift|):  sign: |a| <= b (ReLU mask);  rnd: a within b of the midpoint of two neighbouring storage values
    (bf16 rounding of act);  tie: (n, h // f, w // f, c) windows whose two largest distinct values differ by <= 2 b, or that hold a
    rounding-ambiguous value within two bf16 units of their maximum (arg-max and pooled-gradient routing)."""
    a = pre_act(y, scale, shift)
    b = 4 * U24 * (np.abs(y * scale) + np.abs(shift) * np.ones_like(y))
    sign = (np.abs(a) <= b) & (b > 0)                                                  # (b == 0: a is 0 + 0, exact)
    rnd = np.zeros(a.shape, bool)
    if kind == 'bf16':
        lo = (np.abs(a).astype(np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)   # truncated to bf16
        mid = lo + bf16_ulp(np.maximum(lo, 2.0 ** -126)) / 2
        rnd = (a > 0) & (np.abs(np.abs(a) - mid) <= b)
    n, h, w, c = y.shape
    tie = np.zeros((n, h // f, w // f, c), bool)
    if f > 1 and h >= f and w >= f:
        act = act_of(y, scale, shift, kind)
        wa, wb, wr = windows(act, f), windows(b, f), windows(rnd, f)
        top = wa.max(3, keepdims=True)
        second = np.where(wa < top, wa, -np.inf).max(3, keepdims=True)                # the largest value below the maximum
        tie = ((top - second) <= 2 * wb.max(3, keepdims=True))[:, :, :, 0]
        tie |= (wr & (wa >= top - 2 * bf16_ulp(top))).any(3)
    return dict(sign=sign, rnd=rnd, tie=tie, b=b)


def spread_windows(tie, f, shape):
    """window flags -> per-pixel flags of the pixels those windows cover"""
    n, h, w, c = shape
    out = np.zeros(shape, bool)
    hp, wp = h // f, w // f
    if hp and wp:
        out[:, :hp * f, :wp * f] = np.repeat(np.repeat(tie, f, 1), f, 2)
    return out


def ambiguous_share(shape, f, kind, key, skip_c=0):
    """share of the compared element-wise outputs (act, pooled, dy) of a random case that the ambiguity rule excludes"""
    d = make_inputs(shape, f, kind, 'random', key, skip_c)
    am = ambiguous(d['y'], d['scale'], d['shift'], kind, f)
    px = am['sign'] | am['rnd'] | spread_windows(am['tie'], f, shape)
    return (px.sum() + am['tie'].sum()) / max(px.size + am['tie'].size, 1)


# ------------------------------------------------------------------------------------ case tables
def _past_cap_pixels(per_cu=6):
    """c = 8 (one channel group per pixel): two full trips of a stride loop at the launch cap, plus a ragged tail"""
    return 2 * grid_cap_threads(per_cu) + 3


def pool_cases():
    """(shape, f, amax, act in {'yes', 'no', 'wide'}, pooled, stats).  f == 2 with even h and w: the compile-time 2x2 path."""
    cases = []
    for c in (8, 24):
        for amax in (0, 1):
            cases += [((2, 8, 8, c), 2, amax, 'yes', 1, 1), ((2, 8, 8, c), 2, amax, 'wide', 1, 0), ((3, 7, 9, c), 2, amax, 'wide', 1, 1)]
    cases += [((2, 8, 8, 8), 2, 0, 'no', 1, 1), ((2, 8, 8, 40), 2, 0, 'yes', 0, 1), ((2, 8, 8, 8), 2, 1, 'no', 1, 0)]
    for f in (1, 2, 3, 4):
        cases += [((3, 7, 9, 40), f, f % 2, 'yes', 1, 1), ((3, 7, 9, 72), f, 1 - f % 2, 'wide', 1, 1 - f % 2), ((2, 8, 8, 72), f, f % 2, 'yes', 1, 1)]
    cases += [((3, 7, 9, 8), 3, 0, 'no', 1, 0), ((3, 7, 9, 8), 1, 0, 'yes', 0, 0), ((3, 8, 9, 24), 2, 1, 'yes', 1, 1), ((3, 7, 8, 24), 2, 0, 'yes', 1, 1)]
    for c in (1000, 2048):
        cases += [((1, 1, 1, c), 1, 0, 'yes', 0, 1), ((1, 1, 1, c), 2, 0, 'yes', 1, 1), ((1, 2, 3, c), 2, 1, 'wide', 1, 1), ((1, 2, 3, c), 3, 0, 'yes', 1, 0),
                  ((1, 2, 2, c), 2, 1, 'yes', 1, 1)]
    return cases


def bwd_case(shape, f=1, da=1, dpool=0, linear=0, split=0, dy1=1, sk=0, dbias=0, wide=0):
    return dict(shape=shape, f=f, da=da, dpool=dpool, linear=linear, split=split, dy1=dy1, sk=sk, dbias=dbias, wide=wide)


def bwd_cases():
    """every form of satcv_bn_bwd_reduce / satcv_bn_bwd_apply.  The reduce pass ignores dy1, sk and dbias (one reduce per distinct rest)."""
    B = bwd_case
    cases = []
    # dense: pixel counts 128, 189 (ragged), 1, 3, 4, 5, 6; group counts that do not divide the workgroup; wide channel counts on tiny maps
    for shape in [(2, 8, 8, 8), (3, 7, 9, 24), (3, 7, 9, 40), (2, 8, 8, 72), (1, 1, 1, 8), (1, 1, 3, 8), (1, 2, 2, 8), (1, 1, 5, 24), (1, 2, 3, 1000),
                  (1, 1, 1, 1000), (1, 2, 3, 2048), (1, 1, 1, 2048)]:
        cases += [B(shape), B(shape, dbias=1, wide=1)]
    cases += [B((3, 7, 9, 24), linear=1), B((2, 8, 8, 8), linear=1, wide=1, dbias=1)]
    # two sources, unequal halves
    for shape, split in [((3, 7, 9, 64), 16), ((2, 8, 8, 40), 32), ((1, 1, 1, 1000), 8), ((1, 2, 3, 72), 48), ((1, 1, 5, 24), 16)]:
        for wide in (0, 1):
            cases += [B(shape, split=split, wide=wide), B(shape, split=split, dy1=0, wide=wide), B(shape, split=split, sk=1, wide=wide),
                      B(shape, split=split, sk=1, dy1=0, wide=wide)]
    # pooled: the one-pass 2x2 reduce (even map, da), the generic loop (odd map, f = 3), dpool alone, partial windows, dbias, linear
    cases += [B((2, 8, 8, 24), f=2, dpool=1), B((2, 8, 8, 8), f=2, dpool=1, wide=1, dbias=1), B((3, 7, 9, 40), f=2, dpool=1), B((3, 7, 9, 24), f=3, dpool=1, wide=1),
              B((3, 7, 9, 72), f=3, dpool=1, dbias=1), B((2, 8, 8, 8), f=2, da=0, dpool=1), B((3, 7, 9, 24), f=2, da=0, dpool=1, wide=1),
              B((3, 7, 9, 40), f=3, da=0, dpool=1, dbias=1), B((2, 8, 8, 72), f=4, da=0, dpool=1), B((3, 7, 9, 24), f=2, dpool=1, linear=1),
              B((1, 2, 3, 1000), f=2, dpool=1), B((1, 1, 1, 2048), f=2, dpool=1, dbias=1), B((1, 2, 2, 1000), f=2, dpool=1, wide=1), B((2, 8, 8, 8), f=1, dpool=1)]
    return cases


def cap_cases(per_cu=6):
    """past the launch cap: dense reduce, dense apply (plain, dbias, sk_sums) on c = 8 (the two-source ones on 8 + 8)"""
    p = _past_cap_pixels(per_cu)
    B = bwd_case
    return [B((1, 1, p, 8)), B((1, 1, p, 8), dbias=1), B((1, 1, p, 16), split=8, sk=1), B((1, 1, p, 16), split=8, sk=1, dy1=0)]


def unrolled_tail_case(per_cu=6):
    """4 * per + 1 pixels at c = 8 (per = the whole capped grid): one FULL trip of the four-pixel loop, then a tail of one pixel"""
    return bwd_case((1, 1, 4 * grid_cap_threads(per_cu) + 1, 8))


def case_id(case):
    if isinstance(case, dict):
        tags = ['x'.join(map(str, case['shape'])), f"f{case['f']}"]
        tags += [] if case['da'] else ['noda']
        tags += [k for k in ('dpool', 'linear', 'sk', 'dbias', 'wide') if case[k]]
        tags += [f"split{case['split']}"] + ([] if case['dy1'] else ['nody1']) if case['split'] else []
        return '-'.join(tags)
    shape, f, amax, act, pooled, stats = case
    return 'x'.join(map(str, shape)) + f'-f{f}' + ('-amax' if amax else '') + f'-act_{act}' + ('' if pooled else '-nopooled') + ('-stats' if stats else '')


def skip_channels(case):
    return case['split'] if case['sk'] else 0


FINALIZE_CASES = [(c, pad, updates, bessel, count, moving) for c, pad in [(1, 0), (5, 3), (13, 0), (32, 8), (1000, 24)]
                  for updates, bessel, count, moving in [(0, 0, 189.0, 1), (1, 1, 189.0, 1), (2, 0, 4096.0, 1), (1, 1, 1.0, 1), (2, 1, 128.0, 0)]]


def stat_rows_of(count, c, seed):
    """[32][2][c] float64 sum / sum-of-squares rows of `count` samples per channel dealt over the 32 replica rows (channel 0: constant
    data, variance 0 up to rounding -- the clamp)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((int(count), c)) * rng.uniform(0.2, 3.0, c) + rng.standard_normal(c) * 2.0
    x[:, 0] = 1.25
    rows = np.zeros((STAT_ROWS, 2, c))
    for r in range(STAT_ROWS):
        rows[r, 0], rows[r, 1] = x[r::STAT_ROWS].sum(0), (x[r::STAT_ROWS] ** 2).sum(0)
    return rows


def random_rows(c, seed, scale=50.0):
    """[32][2][c] float64 rows of backward sums, every row holding a part"""
    return np.random.default_rng(seed).standard_normal((STAT_ROWS, 2, c)) * scale
