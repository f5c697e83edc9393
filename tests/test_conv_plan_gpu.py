"""Forward / data-gradient convolution kernels behind satcv_conv2d_igemm, one test per entry of tests/conv_cases.py: every template instantiation the
dispatcher can choose, at a whole-tile, a ragged and a several-images-per-tile shape, and the features each kernel family accepts.

Per case
  * the plan query (satcv_conv2d_igemm_plan_info, with the real pointers and the device's CU count) says the intended instantiation is the one
    about to run; the launch counters of the persistent kernels move by one where they exist; satcv_conv2d_igemm_pipelined agrees;
  * Gaussian data, pre-rounded to the storage type, against the float64 oracle (oracle.keras_ops; float64 torch for strides, and a float64
    per-tap matrix product on the device for the few large shapes) under close() of tests/test_ops_gpu.py with the k of the existing test of
    the same feature: 1, or 2 with the loader's affine / a stride;
  * integer-lattice data, BIT-EXACT: x, w, bias, the accumulate base and the raw outputs v of the fused sums are small integers, the loader
    scale and the output multiplier are from {1, 2, -1, 0.5} with integer shifts, bst_mean is an integer and bst_rstd from {0.5, 1, 2}.  The
    amplitudes are chosen per case so that every accumulator stays below 2^24 in units of the grid (lattice(), asserted from the shape): the fp32
    accumulation is then exact in any order, any K split and any atomic order, and the stored output must equal the exact reference rounded ONCE
    to the storage type, round to nearest even (what torch's .to(bfloat16) does), with np.array_equal.  accumulate rounds twice by definition
    (satcv.h: the result is rounded to the storage type, then added): the pipelined kernels do so for both modes; the generic kernel adds the
    unrounded result for accumulate = 1 (one rounding fewer -- a documented difference).  Under a second asserted bound
    (pixels x max |y| < 2^24) the statistics' sum row, the fused sum g and sum g xhat and the pooled output are exact as well; the sum of squares
    is exact where pixels x max |y|^2 < 2^24 and keeps the existing tolerance elsewhere.  The zero tolerance is derived, not measured;
  * y and pool_y are filled with NaN before each launch, and so is the split-K workspace (the library keeps it per stream: the same launch on NaN
    input runs first); stored input channels beyond the real cin carry non-zero lattice values, as do their scale / shift entries (padded-cin
    cases); stored channels beyond cout must come back untouched, and y has a sentinel image row before and after it;
  * two runs are torch.equal.

The e4m3 storage types (SATCV_FP8, and the block-scaled SATCV_FP8X with its 16-byte items and K = 64 fragments) run the same checks; x, y and pool_y
are float8_e4m3fn and the dtype code comes from the case.  What differs, and why:
  * rounding once to e4m3 is clamp to +-448, then float64 -> float32 -> float8_e4m3fn: the hardware conversion saturates, torch's gives NaN above 464;
  * lattice: x and w are integers of [-4, 4], exact in e4m3; every case has the output multiplier s m_c, m_c from {1, 2, -1, 0.5} and s the largest
    power of two with 2 s K amax aw + 4 <= 448 (lattice()): no element saturates and every fp32 operation of the epilogue is exact, so the stored
    bytes must decode to the float64 reference rounded once -- tolerance zero, derived.  Two cases (conv_cases.E4M3_SATURATING) raise s until 2 - 30 %
    of the reference exceeds 448: the kernel must store +-448 there;
  * three mantissa bits hide small errors, so each lattice case first shows, on the reference alone, that zeroing ONE input channel at ONE tap changes
    at least 5 % of the stored elements (lattice_case(); tests/test_conv_plan_cpu.py asserts the same without a device);
  * Gaussian data: products of e4m3 values are exact in fp32 and the fp32 sum, multiplier and bias err far below half an e4m3 step, so every element
    must lie within ONE e4m3 step of the once-rounded reference (the neighbour near a tie) and none is NaN; the share of elements that are not
    bit-identical goes into the record line, as a record;
  * the sentinel rows hold a fixed byte and are compared as uint8 (777 is no e4m3 value).
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
import conv_cases as W  # noqa: E402
from oracle import keras_ops as K  # noqa: E402
from test_ops_gpu import close  # noqa: E402  (the one tolerance rule of the op tests)

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
GPU_CASES = [c for c in W.CASES if c['gpu']]


@pytest.fixture(scope='module')
def ops():
    from satellite_computervision_amd import ops as _ops
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _ops


@pytest.fixture
def case_options(request):
    with W.options(request.param['opts']):
        yield request.param


E4M3 = torch.float8_e4m3fn
E4M3_MAX = 448.0
SENTINEL_BYTE = 0x5A        # 777 is no e4m3 value: the sentinel rows of an e4m3 buffer hold this byte and are compared as uint8


def tdtype(c):
    """the torch type of x, y and pool_y (both e4m3 storage types are float8_e4m3fn: the dtype CODE comes from the case, dcode())"""
    return {W.BF16: torch.bfloat16, W.F32: torch.float32, W.FP8: E4M3, W.FP8X: E4M3}[c['dtype']]


def dcode(ops, c):
    return {W.F32: ops.F32, W.BF16: ops.BF16, W.FP8: ops.FP8, W.FP8X: ops.FP8X}[c['dtype']]


def is8(c):
    return c['dtype'] in (W.FP8, W.FP8X)


def rne(a, td):
    """float64 array rounded once to the storage type, round to nearest even.  e4m3: the hardware conversion SATURATES at +-448 (common.hpp),
    torch's gives NaN above 464 -- clamped first"""
    t = torch.tensor(a, dtype=torch.float64)
    if td == E4M3:
        t = t.clamp(-E4M3_MAX, E4M3_MAX)
    return t.to(torch.float32).to(td).to(torch.float32).to(torch.float64).numpy()


def host64(t):
    """device tensor -> float64 array (e4m3 goes through float32: exact)"""
    return t.float().double().cpu().numpy()


def spacing8(v):
    """distance between neighbouring e4m3 values at |v|: 2^(floor(log2 |v|) - 3), the subnormal step 2^-9 at least"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -20)))
    return np.maximum(2.0 ** (e - 3), 2.0 ** -9)


def geometry(c):
    """(input shape, kernel shape, output shape, K, pixels of the output)"""
    n, h, w, f, cs, co = c['n'], c['h'], c['w'], c['f'], c['c0'] + c['c1'], c['cout']
    if c['mode'] == 'convt':
        return (n, h, w, cs), (f, f, co, cs), (n, h * f, w * f), cs, n * h * w * f * f
    if c['mode'] == 'convt_dgrad':
        return (n, h * f, w * f, cs), (f, f, cs, co), (n, h, w), f * f * cs, n * h * w
    s = c['stride']
    # (cin: the REAL input channels; the stored cs - cin others carry data too, and zero weights)
    return (n, (h - 1) * s + 1, (w - 1) * s + 1, cs), (c['k'], c['k'], c['cin'], co), (n, h, w), c['k'] * c['k'] * c['cin'], n * h * w


def lattice(c):
    """amplitudes (ax, aw) of the lattice data and what is exact with them.  unit: the grid is 1, or 1/2 with the affine's / multiplier's 0.5;
    amax: largest |activation| in units; the accumulator bound K amax aw must stay below 2^24 (asserted); ymax bounds |y| in units (multiplier
    at most 2, bias at most 4, base at most 4).  The largest amplitudes for which the statistics' sum is exact too are taken."""
    _, _, _, kk, npix = geometry(c)
    if is8(c):
        # e4m3: x and w are integers of [-4, 4] (exact in e4m3, and so is every staged loader value, at most 11 in steps of 1/2).  The
        # multiplier is s m_c with m_c from {1, 2, -1, 0.5} and s the largest power of two with 2 s K amax aw + 4 <= 448: no element
        # saturates, and every fp32 operation of the epilogue is exact (all values are integers below 2^24 in units of s / 4, or s / 8
        # with the affine's halves)
        assert c['out_scale'] and not (c['stats'] or c['accumulate'] or c['bst'])
        ax = aw = 4
        amax = (2 * ax + 3) if c['affine'] else ax
        bound = kk * amax * aw
        s = 2.0 ** np.floor(np.log2((E4M3_MAX - 4) / (2 * bound)))
        assert 2 * s * bound + 4 <= E4M3_MAX < 4 * s * bound + 4, (c['name'], s)
        unit = (2 if c['affine'] else 1) * 2 / s
        acc, ymax = bound * (2 if c['affine'] else 1), (2 * s * bound + 4) * unit
        assert acc < 2 ** 24 and ymax < 2 ** 24, (c['name'], acc, ymax)
        return dict(ax=ax, aw=aw, unit=unit, ymax=ymax, s=s, sum_exact=False, sq_exact=False, bst_exact=False)
    unit = (2 if c['affine'] else 1) * (2 if c['out_scale'] else 1)
    for ax, aw in ((4, 4), (2, 2), (2, 1), (1, 1)):
        amax = (2 * ax + 3) if c['affine'] else ax
        acc = kk * amax * aw * (2 if c['affine'] else 1)
        ymax = acc * (4 if c['out_scale'] else 1) + 8 * unit          # (multiplier at most 2, and its 0.5 halves the grid)
        if npix * ymax < 2 ** 24:
            break
    assert acc < 2 ** 24 and ymax < 2 ** 24, (c['name'], acc, ymax)
    return dict(ax=ax, aw=aw, unit=unit, ymax=ymax, sum_exact=npix * ymax < 2 ** 24, sq_exact=npix * ymax * ymax < 2 ** 24,
                bst_exact=npix * ymax * 32 < 2 ** 24)


def make_data(c, rng, lat):
    """float64 arrays exactly representable in the storage type"""
    td = tdtype(c)
    xs, ks, ys, _, _ = geometry(c)
    cs, co = c['c0'] + c['c1'], c['cout']
    d = {}
    if lat:
        L = lattice(c)
        ri = lambda lo, hi, s: rng.integers(lo, hi + 1, s).astype(np.float64)
        d['x'], d['kern'] = ri(-L['ax'], L['ax'], xs), ri(-L['aw'], L['aw'], ks)
        d['bias'] = ri(-4, 4, co)
        d['sc'], d['sh'] = rng.choice([1.0, 2.0, -1.0, 0.5], cs), ri(-3, 3, cs)
        d['osc'] = rng.choice([1.0, 2.0, -1.0, 0.5], co)
        d['base'] = ri(-4, 4, ys + (co,))
        d['v'] = ri(-4, 4, ys + (co,))
        d['bsc'], d['bsh'] = rng.choice([1.0, 2.0, -1.0, 0.5], co), ri(-3, 3, co)
        d['bmu'], d['brs'] = ri(-4, 4, co), rng.choice([0.5, 1.0, 2.0], co)
        if is8(c):
            d['osc'] = d['osc'] * L['s']
    else:
        r = lambda s, k=1.0: torch.tensor(rng.standard_normal(s) * k, dtype=torch.float32).to(td).to(torch.float64).numpy()
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        d['x'], d['kern'] = r(xs), r(ks, 0.2)
        d['bias'] = f32(rng.standard_normal(co))
        d['sc'], d['sh'] = f32(1 + 0.2 * rng.standard_normal(cs)), f32(0.2 * rng.standard_normal(cs))
        d['osc'] = f32(rng.uniform(0.5, 1.5, co))
        d['base'], d['v'] = r(ys + (co,)), r(ys + (co,), 1.5)
        d['bsc'], d['bsh'] = f32(rng.standard_normal(co)), f32(0.5 * rng.standard_normal(co))
        d['bmu'], d['brs'] = f32(0.3 * rng.standard_normal(co)), f32(0.5 + rng.random(co))
    return d


def conv_ref(c, a, kern):
    """float64 result of the bare convolution (no bias)"""
    xs, ks, ys, kk, npix = geometry(c)
    if c['mode'] == 'convt':
        return K.conv2d_transpose_ks(a, kern, None)
    if c['mode'] == 'convt_dgrad':
        return K.conv2d_transpose_ks_bwd(np.zeros(ys + (c['cout'],)), kern, a)[0]
    if c['stride'] == 1 and npix * kk * c['cout'] <= 4e8:
        return K.conv2d_same(a, kern, None, c['dil'])
    # strides, and the few large shapes: float64 per-tap matrix products of the shifted input (on the device; exact for lattice data like any
    # float64 evaluation, since every partial sum is an integer multiple of the grid far below 2^53)
    dev = torch.device('cuda')
    x, w = torch.tensor(a, device=dev), torch.tensor(kern, device=dev)
    k, dil, s = c['k'], c['dil'], c['stride']
    pad = dil * (k - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, pad, pad, pad, pad))
    n, h, w_ = ys
    y = torch.zeros(ys + (c['cout'],), dtype=torch.float64, device=dev)
    for i in range(k):
        for j in range(k):
            y += xp[:, i * dil:i * dil + (h - 1) * s + 1:s, j * dil:j * dil + (w_ - 1) * s + 1:s, :] @ w[i, j]
    return y.cpu().numpy()


def reference(c, d, family):
    """float64: the stored output (the whole y buffer's valid part), the statistics rows, the pooled output"""
    td, co = tdtype(c), c['cout']
    a = d['x']
    if c['affine']:
        a = rne(np.maximum(a * d['sc'] + d['sh'], 0), td)        # the staged tile is stored in the storage type
    v = conv_ref(c, a[..., :c['cin']] if c['mode'] == 'conv' else a, d['kern'])
    if c['out_scale']:
        v = v * d['osc']
    if c['bias']:
        v = v + d['bias']
    if c['out_relu']:
        v = np.maximum(v, 0)
    tv = rne(v, td)
    out = dict(raw=v)
    if c['accumulate'] == 1:
        tv = rne(d['base'] + (v if family == 'generic' else tv), td)
    elif c['accumulate'] == 2:
        tv = rne(np.maximum(d['base'] + tv, 0), td)
    out['y'] = tv
    ax = (0, 1, 2)
    if c['bst']:
        mask = (d['v'] * d['bsc'] + d['bsh'] > 0) if c['bst_relu'] else np.ones_like(tv, bool)
        g = np.where(mask, tv, 0.0)
        out['s1'], out['s2'] = g.sum(ax), (g * ((d['v'] - d['bmu']) * d['brs'])).sum(ax)
    elif c['stats']:
        out['s1'], out['s2'] = tv.sum(ax), (tv * tv).sum(ax)
    if c['pool_f']:
        out['pool'] = K.maxpool(tv, c['pool_f'])
    return out


def probe_tap(c):
    """the tap whose weights the sensitivity condition zeroes: the last one, in raster order, that reads real data at a quarter of the output
    pixels or more.  An undilated kernel's last tap always does; a strongly dilated kernel's reads mostly padding (dilation 6 on a 16 x 8 map: 15 %
    of the pixels; the centre-tap cases: none), and the centre tap always qualifies"""
    k, dil, h, w = c['k'], c['dil'], c['h'], c['w']
    for t in range(k * k - 1, -1, -1):
        i, j = divmod(t, k)
        if 4 * max(h - abs(i - k // 2) * dil, 0) * max(w - abs(j - k // 2) * dil, 0) >= h * w:
            return i, j


def lattice_case(c, seed, fam):
    """(data, reference, lattice(), notes) of the bit-exact run of a case.  For the e4m3 types, asserted here on the reference alone
      * sensitivity: three mantissa bits hide small errors, so zeroing the weights of the last real input channel at probe_tap() (a transposed
        conv: at every tap, each of which writes its own quarter of the output) must change at least 5 % of the stored reference elements;
      * the cases of conv_cases.E4M3_SATURATING: the multiplier is raised by the smallest power of two for which at least 2 % of the
        reference elements exceed 448 before the clamp; the share must lie between 2 % and 30 %."""
    L = lattice(c)
    d = make_data(c, np.random.default_rng(seed), True)
    notes = []
    if is8(c) and c['name'] in W.E4M3_SATURATING:
        osc, p = d['osc'], 1
        while True:
            p *= 2
            assert p <= 64, c['name']
            d['osc'] = osc * p
            share = float((np.abs(reference(c, d, fam)['raw']) > E4M3_MAX).mean())
            if share >= 0.02:
                break
        assert 0.02 <= share <= 0.30, (c['name'], p, share)
        L['ymax'] *= p
        notes.append(f'saturated {100 * share:.1f}%')
    ref = reference(c, d, fam)
    if is8(c):
        kern = d['kern'].copy()
        if c['mode'] == 'convt':
            kern[:, :, :, -1] = 0
        else:
            i, j = probe_tap(c)
            kern[i, j, c['cin'] - 1, :] = 0
        share = float((reference(c, dict(d, kern=kern), fam)['y'] != ref['y']).mean())
        assert share >= 0.05, f"{c['name']}: zeroing one input channel at one tap changes {100 * share:.1f} % of the stored reference"
        notes.append(f'sens {100 * share:.1f}%')
    return d, ref, L, notes


def counters():
    from satellite_computervision_amd._lib import lib, check
    v, o = C.c_int32(), {}
    for k in ('igemm_thin_launches', 'thin_roles_launches', 'm16p_launches'):
        check(lib.satcv_get_option(k.encode(), C.byref(v)))
        o[k] = v.value
    return o


def run(ops, c, d):
    """one satcv_conv2d_igemm of the case; returns dict(y, stats, pool, plan) of device tensors and the plan"""
    from satellite_computervision_amd._lib import lib, check
    td, dev = tdtype(c), torch.device('cuda')
    code = dcode(ops, c)            # (ops.DTYPE_CODE cannot tell the two e4m3 types apart)
    up = lambda a: torch.tensor(a, dtype=torch.float32).to(td).to(dev).contiguous()
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()
    _, _, ys, _, _ = geometry(c)
    cs, co, ldy = c['c0'] + c['c1'], c['cout'], c['ldy']
    keep = []
    x0 = up(d['x'][..., :c['c0']])
    x1 = up(d['x'][..., c['c0']:]) if c['c1'] else None
    if c['mode'] == 'conv':
        wimg, _ = ops.pack_weights(f32(d['kern']), cs, code, want_dgrad=False)
    elif c['mode'] == 'convt':
        wimg, _ = ops.pack_weights(f32(d['kern']), cs, code, transposed=True, want_dgrad=False)
    else:
        _, wimg = ops.pack_weights(f32(d['kern']), co, code, transposed=True)
    # y with one sentinel image row before and after; pair store: (pair_n, h, w, ldy)
    ny = ys[0] // 2 if c['pair'] else ys[0]
    rows = ny * ys[1]
    nans = lambda shape: torch.full(shape, float('nan'), dtype=torch.float32, device=dev).to(td)
    ybuf = nans((rows + 2, ys[2], ldy))
    if td == E4M3:
        ybuf.view(torch.uint8)[0], ybuf.view(torch.uint8)[-1] = SENTINEL_BYTE, SENTINEL_BYTE
        sentinels_intact = lambda: bool((ybuf.view(torch.uint8)[0] == SENTINEL_BYTE).all()) and bool((ybuf.view(torch.uint8)[-1] == SENTINEL_BYTE).all())
    else:
        ybuf[0], ybuf[-1] = SENTINEL, SENTINEL
        sentinels_intact = lambda: bool((ybuf[0] == SENTINEL).all()) and bool((ybuf[-1] == SENTINEL).all())
    if c['accumulate']:
        ybuf[1:-1, :, :co] = up(d['base']).reshape(rows, ys[2], co)
    y = ybuf[1:-1]
    p = dict(x0=x0.data_ptr(), x1=x1.data_ptr() if x1 is not None else None, w=wimg.data_ptr(), y=y.data_ptr())
    for name, arr in (('in_scale', d['sc']), ('in_shift', d['sh'])) if c['affine'] else ():
        keep.append(f32(arr)); p[name] = keep[-1].data_ptr()
    if c['bias']:
        keep.append(f32(d['bias'])); p['bias'] = keep[-1].data_ptr()
    if c['out_scale']:
        keep.append(f32(d['osc'])); p['out_scale'] = keep[-1].data_ptr()
    stats = ops.new_stats(c['stats_ld'], dev) if c['stats'] else None
    if stats is not None:
        p['stats'] = stats.data_ptr()
    pool = None
    if c['pool_f']:
        pool = nans((ys[0], ys[1] // c['pool_f'], ys[2] // c['pool_f'], co))
        p['pool_y'] = pool.data_ptr()
    if c['bst']:
        half = co // c['bst']
        keep.append(up(d['v'][..., :half])); p['bst_y'] = keep[-1].data_ptr()
        if c['bst'] == 2:
            keep.append(up(d['v'][..., half:])); p['bst_y1'] = keep[-1].data_ptr()
        for name, key in (('bst_scale', 'bsc'), ('bst_shift', 'bsh'), ('bst_mean', 'bmu'), ('bst_rstd', 'brs')):
            keep.append(f32(d[key])); p[name] = keep[-1].data_ptr()
    desc = W.make_desc(c, p)
    got = W.check_plan(c, desc, ncu=0)                 # with the real pointers and the device's CU count: the form about to run
    if c['dtype'] == W.BF16 and not (c['out_scale'] or c['pool_f'] or c['bst'] or c['pair']):        # (plain store: see test_conv_plan_cpu.py on the rest)
        assert lib.satcv_conv2d_igemm_pipelined(C.byref(desc)) == (got['family'] != 'generic'), (c['name'], got['family'])
    if got['sk']:
        # split-K: the fp32 slabs live in a workspace the library keeps per stream.  Poison it first -- the same launch on NaN input writes NaN
        # into every slab element a launch of this geometry writes -- so that no element the finish kernel sums can hold what an earlier,
        # identical run left there (the cases run twice); an element no launch writes holds other data and shows as a wrong value
        pd = type(desc).from_buffer_copy(desc)
        keep.append(torch.full_like(x0, float('nan')))
        pd.x0 = keep[-1].data_ptr()
        keep.append(torch.empty_like(ybuf))
        pd.y = keep[-1][1:-1].data_ptr()
        if stats is not None:
            keep.append(torch.zeros_like(stats))
            pd.stats = keep[-1].data_ptr()
        assert W.plan_info(pd, 0)['key'] == got['key']
        check(lib.satcv_conv2d_igemm(C.byref(pd), ops.stream_ptr()))
        assert bool(torch.isnan(keep[-2 if stats is not None else -1][1:-1][..., :co].float()).all()), f"{c['name']}: the poisoning launch left finite outputs"
    before = counters()
    check(lib.satcv_conv2d_igemm(C.byref(desc), ops.stream_ptr()))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing more may run on this device in this session
        pytest.exit(f"{c['name']}: the device reported {e}", returncode=3)
    after = counters()
    fam = got['family']
    want = dict(igemm_thin_launches=int(fam in ('ws', 'tr')), thin_roles_launches=int(fam == 'tr'), m16p_launches=int(fam == 'm16p'))
    assert {k: after[k] - before[k] for k in want} == want, (c['name'], fam, before, after)
    assert sentinels_intact(), f"{c['name']}: a sentinel row around y was overwritten"
    return dict(y=y.reshape((ny,) + ys[1:] + (ldy,)), stats=stats, pool=pool, plan=got, keep=keep)


def stored(c, r):
    """float64 (n, ho, wo, cout) of what the launch stored, the pair store undone; asserts that channels beyond cout were left alone"""
    y = host64(r['y'])
    co, ldy = c['cout'], c['ldy']
    if c['pair']:
        assert np.isnan(y[..., co:ldy // 2]).all() and np.isnan(y[..., ldy // 2 + co:]).all(), f"{c['name']}: the pair store wrote outside its channels"
        return np.concatenate([y[..., :co], y[..., ldy // 2:ldy // 2 + co]], 0)
    assert np.isnan(y[..., co:]).all(), f"{c['name']}: stored channels beyond cout were overwritten"
    return y[..., :co]


def case_seed(c):
    """seed of a case's Gaussian data; the lattice data takes the next one"""
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c['name'])) % 2**31


def check_case(ops, c):
    """every check of one case; returns the record line of profiles/conv_plan_parity.txt"""
    td = tdtype(c)
    seed = case_seed(c)
    npix = geometry(c)[4]
    # ---- Gaussian parity
    d = make_data(c, np.random.default_rng(seed), False)
    r = run(ops, c, d)
    fam = r['plan']['family']
    ref = reference(c, d, fam)
    got = stored(c, r)
    assert not np.isnan(got).any(), f"{c['name']}: {int(np.isnan(got).sum())} output elements were never written"
    if is8(c):
        # e4m3 inputs: every product is exact in fp32, and the fp32 sum, multiplier and bias add errors far below half an e4m3 step -- the stored
        # value is the once-rounded reference or, near a tie, its neighbour.  The share of not bit-identical elements is a record, not a threshold
        off = np.abs(got - ref['y']) > spacing8(ref['y'])
        assert not off.any(), f"{c['name']}: {int(off.sum())} of {got.size} elements are more than one e4m3 step from the once-rounded reference, max |diff| {np.abs(got - ref['y']).max()}"
        gauss = f"gauss one step, {100 * float((got != ref['y']).mean()):.2f}% not identical"
    else:
        err, tol = close(got, ref['y'], td, f"conv {c['name']}", k=2.0 if (c['affine'] or c['stride'] > 1) else 1.0)
        gauss = f'gauss {err:.2e} < {tol:.1e}'
    if c['stats']:
        s = r['stats'].sum(0).double().cpu().numpy()[:, :c['cout']]
        if c['bst']:            # sums of the STORED gradient (the rule of test_16x16x32_tile_fused_bn_backward_sums)
            mask = (d['v'] * d['bsc'] + d['bsh'] > 0) if c['bst_relu'] else np.ones_like(got, bool)
            gg, xh = np.where(mask, got, 0.0), (d['v'] - d['bmu']) * d['brs']
            t = 2e-4 * np.sqrt(npix) * max(1.0, float(np.abs(got).max()))
            np.testing.assert_allclose(s[0], gg.sum((0, 1, 2)), rtol=1e-4, atol=t, err_msg=f"sum g {c['name']}")
            np.testing.assert_allclose(s[1], (gg * xh).sum((0, 1, 2)), rtol=1e-4, atol=t * float(np.abs(xh).max()), err_msg=f"sum g xhat {c['name']}")
        else:                   # statistics of the STORED values (the rule of test_conv2d_fwd)
            np.testing.assert_allclose(s[0], got.sum((0, 1, 2)), rtol=2e-4, atol=2e-3 * np.sqrt(npix), err_msg=f"sum {c['name']}")
            np.testing.assert_allclose(s[1], (got ** 2).sum((0, 1, 2)), rtol=2e-4, err_msg=f"sum of squares {c['name']}")
    if c['pool_f']:
        assert np.array_equal(host64(r['pool']), K.maxpool(got, c['pool_f'])), f"{c['name']}: pooled output is not the max of the stored one"
    # ---- integer lattice, bit-exact (e4m3: with the sensitivity and saturation conditions of lattice_case)
    d, ref, L, notes = lattice_case(c, seed + 1, fam)
    assert np.abs(ref['raw']).max() * L['unit'] <= L['ymax'] and np.array_equal(ref['raw'] * L['unit'], np.rint(ref['raw'] * L['unit']))      # on the lattice
    r = run(ops, c, d)
    got = stored(c, r)
    nbad = int((got != ref['y']).sum())
    if is8(c):
        over = np.abs(ref['raw']) > E4M3_MAX
        assert over.any() == (c['name'] in W.E4M3_SATURATING), c['name']
    if c['stats']:
        s = r['stats'].sum(0).double().cpu().numpy()[:, :c['cout']]
        exact1 = L['bst_exact'] if c['bst'] else L['sum_exact']
        exact2 = L['bst_exact'] if c['bst'] else L['sq_exact']
        if nbad == 0:
            if exact1:
                assert np.array_equal(s[0], ref['s1']), f"{c['name']}: sum row differs from the exact one by up to {np.abs(s[0] - ref['s1']).max()}"
            else:
                np.testing.assert_allclose(s[0], ref['s1'], rtol=2e-4, atol=2e-3 * np.sqrt(npix) * L['ymax'])
            if exact2:
                assert np.array_equal(s[1], ref['s2']), f"{c['name']}: second row differs from the exact one by up to {np.abs(s[1] - ref['s2']).max()}"
            else:
                np.testing.assert_allclose(s[1], ref['s2'], rtol=2e-4, atol=2e-4 * np.abs(ref['s2']).max() + 1e-30)
        notes.append(f"sums {'exact' if exact1 else 'tol'}/{'exact' if exact2 else 'tol'}")
    if c['pool_f'] and nbad == 0:
        assert np.array_equal(host64(r['pool']), ref['pool']), f"{c['name']}: pooled output differs"
    line = (f"CONV-PARITY {c['name']:46s} {'/'.join(str(v) for v in c['key']):44s} wg {r['plan']['workgroups']:5d} {gauss}  "
            f"lattice {'exact' if nbad == 0 else 'NOT EXACT (%d of %d)' % (nbad, got.size)}{' ' + ' '.join(notes) if notes else ''}")
    print(line)
    if is8(c):
        assert np.array_equal(got[over], np.sign(ref['raw'][over]) * E4M3_MAX), f"{c['name']}: elements beyond 448 were not stored as +-448"
    assert nbad == 0, f"{c['name']}: {nbad} of {got.size} elements differ from the exact reference, max |diff| {np.nanmax(np.abs(got - ref['y']))}"
    r2 = run(ops, c, d)
    assert torch.equal(torch.nan_to_num(r['y'].float(), nan=-1.0), torch.nan_to_num(r2['y'].float(), nan=-1.0)), f"{c['name']}: two lattice runs differ"
    return line


@pytest.mark.parametrize('case_options', GPU_CASES, ids=[c['name'] for c in GPU_CASES], indirect=True)
def test_conv_case(ops, case_options):
    check_case(ops, case_options)


def child_main(i):
    """the cases of one startup-option set, in a process started with its environment"""
    from satellite_computervision_amd import ops as _ops
    lines = []
    for c in W.STARTUP_SETS[i]['cases']:
        if c['gpu']:
            with W.options(c['opts']):
                lines.append(check_case(_ops, c))
    print('CHILD-OK ' + json.dumps(lines))


@pytest.mark.parametrize('i', range(len(W.STARTUP_SETS)))
def test_startup_option_cases_in_a_fresh_process(i):
    """startup-only switches are read once, when the library loads: the cases of a set share ONE child process."""
    s = W.STARTUP_SETS[i]
    code = f'import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]; import test_conv_plan_gpu as T; T.child_main({i})'
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **W.startup_env(s['opts'])), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith('CHILD-OK '), r.stdout[-2000:]
    lines = json.loads(last[len('CHILD-OK '):])
    assert len(lines) == sum(1 for c in s['cases'] if c['gpu'])
    print('\n'.join(lines))


def test_bench_table_is_what_the_engine_builds(ops, monkeypatch):
    """conv_cases.BENCH_LAUNCHES against the satcv_conv_desc structures engine.py builds for bench.py's workload (get_unet_model(2, 4), 256 x 256,
    batch 64, bf16, training plan): the same launches in the same order, field by field, and, with the engine's own pointers and the device's CU
    count, the pinned kernel form and workgroup count (pinned at 256 CUs: compared where the device has 256)."""
    from satellite_computervision_amd import model_tools as mt, _lib
    made = []
    orig = ops.make_conv_desc

    def record(**kw):
        d = orig(**kw)
        if sys._getframe(1).f_code.co_name == '_conv_step':       # (the engine's dry-run probes build descriptors too: launches only)
            made.append(d)
        return d
    monkeypatch.setattr(ops, 'make_conv_desc', record)
    mt.reset_uids()
    mt.set_seed(0)
    old, model = mt._DEFAULT_DTYPE, None
    mt.set_compute_dtype('bfloat16')
    try:
        model = mt.get_unet_model(2, 4)
        model.compile(optimizer=mt.Adam(9e-4), loss=lambda yt, yp: mt.weighted_categorical_crossentropy(yt, yp, [1.0, 20.0]))
        model._head_plan(W.BENCH_N, 256, 256, True)
        assert len(made) == len(W.BENCH_LAUNCHES) == 35, [(d.h, d.w_, d.c0, d.c1, d.cout) for d in made]
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        ptrs = ('x0', 'x1', 'in_scale', 'in_shift', 'w', 'bias', 'y', 'stats', 'out_scale', 'pool_y', 'bst_y', 'bst_y1', 'bst_scale', 'bst_shift', 'bst_mean', 'bst_rstd')
        for d, c in zip(made, W.BENCH_LAUNCHES):
            want = W.make_desc(c)
            for k, _ in _lib.ConvDesc._fields_:
                a, b = getattr(d, k), getattr(want, k)
                assert (bool(a) == bool(b)) if k in ptrs else (a == b), (c['name'], k, a, b)
            g = W.plan_info(d, 0)
            assert g['key'] == c['key'], (c['name'], g)
            if cus == W.NCU:        # (the table pins the workgroup counts of a 256-CU device)
                assert g['workgroups'] == c['workgroups'], (c['name'], g)
    finally:
        mt.set_compute_dtype(old)
        del model
        torch.cuda.empty_cache()
