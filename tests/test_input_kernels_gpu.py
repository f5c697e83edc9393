"""Op-level parity of the kernels that bring data and weights into the model -- csrc/input_pipeline.hip (satcv_tile_channel_mean,
satcv_tile_ingest, satcv_label_onehot) and, of csrc/elementwise.hip, satcv_ingest_chw and satcv_pack_weights / _batched /
satcv_pack_job_items -- through the C ABI, each call with its own descriptor, against the NumPy restatements of
tests/input_kernels_oracle.py (pinned by tests/test_input_kernels_cpu.py).

Every output lies inside a wider device buffer: NaN bits (0xFF bytes) where the kernel may write and beside its channel slice, a sentinel
byte run in front of and behind it; nothing but the owned region may change.  Source elements outside the trimmed window are NaN in the
float kinds (huge values for the mean kernel, which would skip a NaN).

Bounds (none tuned on the device):
  tile_ingest          the float32 bits of the oracle (NaN payloads aside), mask channel included; uniform draws exactly draw_uniform;
                       normal draws within 2^-22 |ref| + 2^-60 of draw_normal (one float32 rounding plus the last places of the double
                       log, cos and sqrt, margin of four), at most 1e-3 of them differing from the oracle's float32 at all
  tile_channel_mean    (cnt + 1) 2^-53 sum|v| / cnt; exact where the double sum is (integer planes, rescale 0 or a power of two)
  mean -> ingest       (|contra| + |bright|) times the mean's bound plus one rounding of the output (2^-24 |ref|)
  label_onehot, ingest_chw, pack_weights, pack_weights_batched     bit for bit
Every toleranced check prints its error as a fraction of its bound in a `[fig]` line (pytest -rP); run as a script, the file writes the
line closest to its bound per test and kind of check to profiles/input_kernels_parity.txt."""
import ctypes as C
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
import input_kernels_oracle as I  # noqa: E402
import test_elementwise_gpu as G  # noqa: E402  (the library handle `E`, the stream, `sync`)

pytestmark = pytest.mark.gpu

E = G.E
O = I.O
GB = 4096                                      # guard bytes on either side of every output
GUARD_BYTE, NAN_BYTE = 0xA5, 0xFF
ES = {'f32': 4, 'bf16': 2, 'fp8': 1}
BITS = {'f32': np.uint32, 'bf16': np.uint16, 'fp8': np.uint8}
CODE = {'f32': 0, 'bf16': 1, 'fp8': 2, 'fp8x': 3}
NANBITS = np.uint32(0xFFFFFFFF)


def fig(check, detail, err, bound):
    frac = float(err) / float(bound) if bound > 0 else (0.0 if err == 0 else np.inf)
    print(f'[fig] {check} | {detail}: {frac:.3e} of its bound')
    return frac


def last_error():
    return E.lib.satcv_last_error().decode()


class Guarded:
    """`nbytes` of device memory holding NaN bits between two runs of a sentinel byte"""

    def __init__(self, nbytes, fill=NAN_BYTE):
        self.n = int(nbytes)
        host = np.full(self.n + 2 * GB, fill, np.uint8)
        host[:GB] = GUARD_BYTE
        host[GB + self.n:] = GUARD_BYTE
        self.before = host
        self.t = torch.from_numpy(host.copy()).cuda()
        self.p = self.t.data_ptr() + GB

    def body(self, dtype=np.uint8):
        G.sync()
        now = self.t.cpu().numpy()
        assert (now[:GB] == GUARD_BYTE).all(), 'written in front of the buffer'
        assert (now[GB + self.n:] == GUARD_BYTE).all(), 'written behind the buffer'
        return now[GB:GB + self.n].view(dtype)

    def unchanged(self):
        G.sync()
        return np.array_equal(self.t.cpu().numpy(), self.before)


def window_poisoned(planes, h, w, value):
    """the planes with every element outside the trimmed window replaced (float kinds): nothing may read it"""
    if planes.dtype.kind != 'f':
        return planes
    p = np.full_like(planes, value)
    ty, tx = (planes.shape[-2] - h) // 2, (planes.shape[-1] - w) // 2
    p[..., ty:ty + h, tx:tx + w] = planes[..., ty:ty + h, tx:tx + w]
    return p


def dev_planes(planes):
    return torch.from_numpy(np.ascontiguousarray(planes)).cuda()


def tile_desc(src, planes, h, w, **kw):
    from satellite_computervision_amd import _lib
    n, c, hin, win = planes.shape
    d = _lib.TileDesc(src=src.data_ptr(), src_kind=I.kind_of(planes), n=n, c=c, hin=hin, win=win, h=h, w_=w, rescale=0.0, nan_mask=0, replace=1, seed=0,
                      ch_mean=None, contra_mul=1.0, bright_mul=1.0, flip_v=0, flip_h=0, rot=0, dst=None, ldc=0, coff=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def run_ingest(planes, h, w, rescale=0.0, nan_mask=0, replace=1, seed=0, ch_mean=None, contra=1.0, bright=1.0, morph=(0, 0, 0), ldc=None, coff=0,
               ch_mean_dev=None):
    """-> the (n, ho, wo, c[+1]) float32 the kernel wrote; asserts that nothing else in the guarded (n, ho, wo, ldc) buffer changed"""
    n, c = planes.shape[:2]
    cw = c + (1 if nan_mask else 0)
    ldc = ldc or cw
    ho, wo = (w, h) if morph[2] % 2 else (h, w)
    src = dev_planes(window_poisoned(planes, h, w, np.nan))
    out = Guarded(n * ho * wo * ldc * 4)
    mean = ch_mean_dev if ch_mean_dev is not None else (torch.tensor(np.asarray(ch_mean, np.float64).reshape(-1)).cuda() if ch_mean is not None else None)
    d = tile_desc(src, planes, h, w, rescale=float(rescale), nan_mask=nan_mask, replace=replace, seed=seed, ch_mean=mean.data_ptr() if mean is not None else None,
                  contra_mul=float(contra), bright_mul=float(bright), flip_v=morph[0], flip_h=morph[1], rot=morph[2], dst=out.p, ldc=ldc, coff=coff)
    E.check(E.lib.satcv_tile_ingest(C.byref(d), E.st))
    body = out.body(np.uint32).reshape(n, ho, wo, ldc)
    keep = np.ones(ldc, bool)
    keep[coff:coff + cw] = False
    assert (body[..., keep] == NANBITS).all(), 'tile_ingest wrote outside its channel slice'
    return np.ascontiguousarray(body[..., coff:coff + cw]).view(np.float32)


def same_f32(got, ref):
    """the float32 bits agree; a NaN matches any NaN (payloads are not part of the contract)"""
    if got.shape != ref.shape:
        return False
    gn, rn = np.isnan(got), np.isnan(ref)
    g, r = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(ref, np.float32).view(np.uint32)
    return np.array_equal(gn, rn) and np.array_equal(g[~gn], r[~rn])


def oracle_ingest(planes, h, w, morph=(0, 0, 0), **kw):
    return I.tile_ingest(planes, h, w, flip_v=morph[0], flip_h=morph[1], rot=morph[2], **kw)


def check_ingest(what, planes, h, w, morph=(0, 0, 0), ldc=None, coff=0, **kw):
    """one launch against the oracle: bit for bit outside the normal draws, the draws within their bound"""
    got = run_ingest(planes, h, w, morph=morph, ldc=ldc, coff=coff, **kw)
    okw = {k: v for k, v in kw.items()}
    ref = oracle_ingest(planes, h, w, morph, **okw)
    nan_mask, replace = kw.get('nan_mask', 0), kw.get('replace', 1)
    if nan_mask == 1 and replace:
        c = planes.shape[1]
        rep = I.tile_replaced(planes, h, w, kw.get('rescale', 0.0), 1, 1, *morph)
        ref64 = oracle_ingest(planes, h, w, morph, as64=True, **okw)[..., :c]
        assert same_f32(got[..., c], ref[..., c]), f'{what}: mask channel'
        assert same_f32(got[..., :c][~rep], ref[..., :c][~rep]), f'{what}: an element that holds no draw'
        if rep.any():
            err = np.abs(got[..., :c][rep].astype(np.float64) - ref64[rep])
            bound = 2.0 ** -22 * np.abs(ref64[rep]) + 2.0 ** -60
            worst = float((err / bound).max())
            fig('normal draws', what, worst, 1.0)
            assert worst <= 1.0, f'{what}: a normal draw off by {worst:.2f} of its bound'
            differ = int((got[..., :c][rep] != ref[..., :c][rep]).sum())
            assert differ <= 1e-3 * rep.sum(), f'{what}: {differ} of {int(rep.sum())} normal draws differ from the float32 of the oracle'
    else:
        assert same_f32(got, ref), f'{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} of {got.size} outputs differ'
    return got


def tile_cases():
    return [(hw, src) for hw, even, odd in I.TILE_SHAPES for src in (even, odd)]


# ------------------------------------------------------------------------------ tile_ingest
@pytest.mark.parametrize('kind', I.KIND_NAMES)
def test_tile_ingest_every_kind_size_and_trim(kind):
    """rescale, centre trim (even and odd differences), every mask mode, on three tiles of which two are not square; n = 3"""
    i = 0
    for (h, w), (hin, win) in tile_cases():
        for c in (1, 3, 4):
            for rescale in (I.RESCALE[kind], 0.0):
                what = f'{kind} {h}x{w} of {hin}x{win} c={c} rescale={rescale:g}'
                m = I.MORPHS[i % 16]
                i += 5
                planes = I.make_planes(kind, (3, c, hin, win), seed=c + hin, nan_frac=0.02, low_frac=0.03, rescale=rescale, mode=1)
                check_ingest(what, planes, h, w, m, rescale=rescale)
                check_ingest(what + ' mode 1', planes, h, w, m, rescale=rescale, nan_mask=1, replace=1, seed=17 + i)
                check_ingest(what + ' mode 1 keep', planes, h, w, rescale=rescale, nan_mask=1, replace=0)
                p2 = I.make_planes(kind, (3, c, hin, win), seed=c + win, nan_frac=0.03, low_frac=0.04, rescale=rescale, mode=2)
                check_ingest(what + ' mode 2', p2, h, w, m, rescale=rescale, nan_mask=2, seed=2 ** 63 + i)


@pytest.mark.parametrize('kind', ['f32', 'i16'])
def test_tile_ingest_all_morphs_of_a_non_square_tile_in_a_wider_tensor(kind):
    """5 x 7 of 8 x 12 at channel offset 2 of c + 5 channels.  The draws are keyed on the SOURCE index: the output under each morph is the
    morph of the unmorphed output, replaced values included, bit for bit"""
    c, (h, w) = 4, (5, 7)
    rescale = 0.0 if kind == 'i16' else I.RESCALE[kind]                                # -15000 fits the type only unscaled
    planes = I.make_planes(kind, (3, c, 8, 12), seed=4, nan_frac=0.1, low_frac=0.1, rescale=rescale, mode=1)
    for mode, seed in ((0, 0), (1, 99), (2, 5)):
        kw = dict(rescale=rescale, nan_mask=mode, seed=seed)
        base = check_ingest(f'{kind} mode {mode} unmorphed', planes, h, w, ldc=c + 5, coff=2, **kw)
        if mode == 1:
            assert base[..., c].any() and not base[..., c].all()
        for m in I.MORPHS:
            got = check_ingest(f'{kind} mode {mode} morph {m}', planes, h, w, m, ldc=c + 5, coff=2, **kw)
            assert got.shape == ((3, w, h, base.shape[-1]) if m[2] % 2 else base.shape)
            assert same_f32(got, I.morph(base, *m)) and np.array_equal(got.view(np.uint32), I.morph(base, *m).view(np.uint32)), (mode, m)


@pytest.mark.parametrize('kind', ['f32', 'f64', 'i16', 'i32'])
@pytest.mark.parametrize('replace', [1, 0])
def test_tile_ingest_mode_1_accumulates_its_flags_over_the_channels(kind, replace):
    """a flag in the first, a middle and the last of five channels: that channel and every later one of the pixel is replaced"""
    c, (h, w) = 5, (6, 9)
    rescale = 0.0 if kind == 'i16' else I.RESCALE[kind]
    planes = I.make_planes(kind, (2, c, 9, 12), seed=8, rescale=rescale)
    low = np.asarray(-5000.0 * (rescale or 1.0) * 2).astype(planes.dtype)
    planes[0, 0, 3, 4] = low
    planes[0, 2, 4, 5] = np.nan if kind in ('f32', 'f64') else low
    planes[1, 4, 5, 6] = low
    planes[1, 2, 0, 0] = low                                                          # trimmed away: flags nothing
    got = check_ingest(f'{kind} replace={replace}', planes, h, w, rescale=rescale, nan_mask=1, replace=replace, seed=3)
    ref0 = oracle_ingest(planes, h, w, rescale=rescale)
    changed = (got[..., :c].view(np.uint32) != ref0.view(np.uint32)) & ~(np.isnan(got[..., :c]) & np.isnan(ref0))
    expect = np.zeros(changed.shape, bool)
    if replace:
        expect[0, 2, 3, 0:], expect[0, 3, 4, 2:], expect[1, 4, 5, 4:] = True, True, True     # window offset (1, 1)
    assert np.array_equal(changed, expect) and got[..., c].sum() == (3 if replace else 0)


@pytest.mark.parametrize('case', I.threshold_cases(), ids=str)
def test_tile_ingest_thresholds_at_equality(case):
    """exactly -5000 (mode 1) or -1 (mode 2) after the rescale is valid; the predecessor is flagged"""
    kind, rescale, mode = case
    p, _ = I.threshold_planes(kind, rescale, mode)
    got = check_ingest(f'{kind} rescale={rescale:g} mode {mode}', p, 4, 6, rescale=rescale, nan_mask=mode, replace=1, seed=1)
    flagged = got[0, ..., 3] == (1.0 if mode == 1 else 0.0)
    assert not flagged[0, 0] and flagged[0, 3] and not flagged[0, 4]
    if not rescale:
        assert flagged[0, 1] and not flagged[0, 2]


@pytest.mark.parametrize('kind', ['f32', 'f64'])
def test_tile_ingest_mode_2_replaces_nans_with_the_uniform_draws(kind):
    c, (h, w) = 3, (12, 20)
    planes = I.make_planes(kind, (3, c, 15, 25), seed=6, nan_frac=0.2, low_frac=0.05, rescale=10000.0, mode=2)
    for seed in (0, 12345, 2 ** 64 - 1):
        got = check_ingest(f'{kind} seed {seed}', planes, h, w, rescale=10000.0, nan_mask=2, seed=seed)
        rep = I.tile_replaced(planes, h, w, 10000.0, 2)
        idx = np.arange(planes.size, dtype=np.uint64).reshape(planes.shape)
        u = np.moveaxis(I._trim(I.draw_uniform(seed, idx), h, w), 1, 3)
        assert rep.sum() > 100 and np.array_equal(got[..., :c][rep], u[rep].astype(np.float32))          # exactly draw_uniform
        assert np.array_equal(got[..., c] == 0, (rep | (got[..., :c] < -1)).any(-1))


AWKWARD_MEANS = [np.pi * 1e-3, 1.0 / 3.0, -7.7e5, 1e-310, 0.1 + 2.0 ** -50, 16777217.0, -0.0, 2.0 ** -140, 1.7e38, np.nan, 1e-45, 123456.789]


@pytest.mark.parametrize('kind', I.KIND_NAMES)
def test_tile_ingest_colour_about_a_given_mean(kind):
    """(v - mu) contra + mu bright as separate operations, in float32 for float32 planes and in double otherwise, for doubles that no mean
    kernel would produce as well as for true means"""
    rng = np.random.default_rng(3)
    (h, w), (hin, win), c, n = (12, 20), (15, 25), 4, 3
    for rescale in (I.RESCALE[kind], 0.0):
        planes = I.make_planes(kind, (n, c, hin, win), seed=9, nan_frac=0.01, rescale=rescale)
        true = I.tile_channel_mean(planes, h, w, rescale)[0]
        for mu, (contra, bright), m in ((np.array(AWKWARD_MEANS).reshape(n, c), (0.97, 1.04), (1, 0, 3)), (true, (1.05, 0.95), (0, 1, 1)),
                                        (true * (1 + rng.standard_normal((n, c)) * 1e-9), (1.0 / 3.0, 0.1), (0, 0, 0))):
            with np.errstate(all='ignore'):
                check_ingest(f'{kind} rescale={rescale:g} colour {contra:g} {bright:g}', planes, h, w, m, rescale=rescale, ch_mean=mu, contra=contra, bright=bright,
                             ldc=c + 5, coff=2)
    planes = I.make_planes(kind, (n, c, hin, win), seed=10, nan_frac=0.1, rescale=10000.0, mode=2)
    mu = I.tile_channel_mean(planes, h, w, 10000.0, nan_mask=2, seed=77)[0]
    check_ingest(f'{kind} mode 2 with colour', planes, h, w, (1, 1, 2), rescale=10000.0, nan_mask=2, seed=77, ch_mean=mu, contra=1.02, bright=0.99)


# ------------------------------------------------------------------------ tile_channel_mean
def run_mean(planes, h, w, rescale=0.0, nan_mask=0, seed=0, poison=True):
    n, c = planes.shape[:2]
    huge = {np.dtype('float32'): 3e38, np.dtype('float64'): 1e300}.get(planes.dtype, 0)
    src = dev_planes(window_poisoned(planes, h, w, huge) if poison else planes)
    out = Guarded(n * c * 8)
    d = tile_desc(src, planes, h, w, rescale=float(rescale), nan_mask=nan_mask, seed=seed)
    E.check(E.lib.satcv_tile_channel_mean(C.byref(d), out.p, E.st))
    return out.body(np.float64).reshape(n, c).copy(), (src, d)


def check_mean(what, planes, h, w, rescale=0.0, nan_mask=0, seed=0, exact=False):
    got, _ = run_mean(planes, h, w, rescale, nan_mask, seed)
    ref, cnt, sabs = I.tile_channel_mean(planes, h, w, rescale, nan_mask, seed)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f'{what}: NaN means'
    ok = ~np.isnan(ref)
    if exact:
        assert np.array_equal(got[ok], ref[ok]), f'{what}: an exact sum came out inexact'
        return got
    err, bound = np.abs(got - ref)[ok], I.mean_bound(cnt, sabs)[ok]
    worst = float(np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    fig('channel mean', what, worst, 1.0)
    assert worst <= 1.0, f'{what}: {worst:.2f} of the bound'
    return got


@pytest.mark.parametrize('kind', I.KIND_NAMES)
def test_tile_channel_mean(kind):
    """windows with fewer pixels than threads, one pixel per thread and many; a channel with some NaNs, an all-NaN channel"""
    for h, w in I.MEAN_WINDOWS:
        for rescale, hin, win in ((I.RESCALE[kind], h + 3, w + 2), (0.0, h, w + 1)):
            planes = I.make_planes(kind, (2, 3, hin, win), seed=h + 1, nan_frac=0.05, rescale=rescale)
            if kind in ('f32', 'f64'):
                planes[1, 1] = np.nan
            got = check_mean(f'{kind} {h}x{w} rescale={rescale:g}', planes, h, w, rescale)
            assert np.isnan(got[1, 1]) == (kind in ('f32', 'f64')) and np.isfinite(got[0]).all()


@pytest.mark.parametrize('kind', I.EXACT_MEAN_KINDS)
def test_tile_channel_mean_is_exact_where_the_sum_is(kind):
    for h, w in I.MEAN_WINDOWS:
        planes = I.exact_mean_planes(kind, (2, 2, h + 3, w + 2), h)
        for rescale in I.EXACT_MEAN_RESCALES:
            check_mean(f'{kind} {h}x{w} rescale={rescale:g}', planes, h, w, rescale, exact=True)


@pytest.mark.parametrize('kind', ['f32', 'f64'])
def test_tile_channel_mean_in_mode_2_includes_the_draws_the_ingest_writes(kind):
    (h, w), seed = (16, 16), 31
    planes = I.make_planes(kind, (2, 3, 19, 21), seed=2, nan_frac=0.3, rescale=10000.0, mode=2)
    planes[1, 2] = np.nan                                                              # a channel of draws alone
    got = check_mean(f'{kind} mode 2', planes, h, w, 10000.0, nan_mask=2, seed=seed)
    assert 0.3 < got[1, 2] < 0.7
    out = check_ingest(f'{kind} mode 2', planes, h, w, rescale=10000.0, nan_mask=2, seed=seed)
    assert abs(out[1, ..., 2].astype(np.float64).mean() - got[1, 2]) <= 2.0 ** -24                # the float32 of the very values it averaged


@pytest.mark.parametrize('kind', ['u16', 'f64'])
def test_mean_then_ingest_as_the_generator_chains_them(kind):
    (h, w), (hin, win), c, n = (12, 20), (15, 25), 4, 3
    rescale, contra, bright = I.RESCALE[kind], 0.96, 1.03
    planes = I.make_planes(kind, (n, c, hin, win), seed=12, nan_frac=0.02, rescale=rescale)
    src = dev_planes(planes)
    mean = torch.full((n * c,), -777.0, dtype=torch.float64).cuda()
    d = tile_desc(src, planes, h, w, rescale=rescale)
    E.check(E.lib.satcv_tile_channel_mean(C.byref(d), mean.data_ptr(), E.st))
    got = run_ingest(planes, h, w, rescale=rescale, ch_mean_dev=mean, contra=contra, bright=bright, morph=(1, 0, 1)).astype(np.float64)
    mu, cnt, sabs = I.tile_channel_mean(planes, h, w, rescale)
    ref = oracle_ingest(planes, h, w, (1, 0, 1), rescale=rescale, ch_mean=mu, contra=contra, bright=bright, as64=True)
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(got), ~ok)
    bound = (abs(contra) + abs(bright)) * I.mean_bound(cnt, sabs)[:, None, None, :] + 2.0 ** -24 * np.abs(ref)
    worst = float((np.abs(got - ref)[ok] / bound[ok]).max())
    fig('mean -> ingest', kind, worst, 1.0)
    assert worst <= 1.0


# ----------------------------------------------------------------------------- label_onehot
def run_labels(lc, h, w, ncls, lut=None, lu=None, lu_lut=None, morph=(0, 0, 0), ldc=None, coff=0):
    n, _, hin, win = lc.shape
    ldc = ldc or ncls
    ho, wo = (w, h) if morph[2] % 2 else (h, w)
    lcd = dev_planes(window_poisoned(lc, h, w, np.nan))
    lud = dev_planes(window_poisoned(lu, h, w, 82.0)) if lu is not None else None
    lutd = torch.tensor(np.asarray(lut), dtype=torch.int32).cuda() if lut is not None else None
    lulutd = torch.tensor(np.asarray(lu_lut), dtype=torch.int32).cuda() if lu_lut is not None else None
    out = Guarded(n * ho * wo * ldc * 4)
    E.check(E.lib.satcv_label_onehot(lcd.data_ptr(), I.kind_of(lc), lutd.data_ptr() if lutd is not None else None, lud.data_ptr() if lud is not None else None,
                                     I.kind_of(lu) if lu is not None else 0, lulutd.data_ptr() if lulutd is not None else None, n, hin, win, h, w, ncls,
                                     morph[0], morph[1], morph[2], out.p, ldc, coff, E.st))
    body = out.body(np.uint32).reshape(n, ho, wo, ldc)
    keep = np.ones(ldc, bool)
    keep[coff:coff + ncls] = False
    assert (body[..., keep] == NANBITS).all(), 'label_onehot wrote outside its channel slice'
    return np.ascontiguousarray(body[..., coff:coff + ncls]).view(np.float32)


def luts():
    lut = np.full(256, -1, np.int64)
    for x, y in [(12, 3), (11, 3), (10, 3), (9, 8), (255, 0), (3, 12), (2, 1), (7, -1)]:
        lut[x] = y
    lu_lut = np.full(256, -1, np.int64)
    lu_lut[82], lu_lut[84], lu_lut[0], lu_lut[255] = 9, 1, 2, -1
    return lut, lu_lut


@pytest.mark.parametrize('kind', I.LABEL_KINDS)
def test_label_onehot(kind):
    """every label kind with values at and past each limit (>= 256, < 0, >= ncls, fractional, NaN and +-inf in the float kinds: zero rows),
    with and without either table, land use of a float and an integer kind (82.5 and values >= 256 match nothing), ncls 1, 2 and 8"""
    lut, lu_lut = luts()
    i = 0
    for (h, w), (hin, win) in tile_cases():
        lc = I.label_planes(kind, (3, 1, hin, win), hin)
        for lu_kind in (None, 'f32', 'i16'):
            lu = I.landuse_planes(lu_kind, lc.shape, win) if lu_kind else None
            for ncls in (1, 2, 8):
                for use_lut in (lut, None):
                    m = I.MORPHS[i % 16]
                    i += 3
                    got = run_labels(lc, h, w, ncls, use_lut, lu, lu_lut if lu is not None else None, m)
                    ref = I.label_onehot(lc, use_lut, lu, lu_lut if lu is not None else None, h, w, ncls, m)
                    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (kind, h, w, hin, win, lu_kind, ncls, use_lut is not None, m)


@pytest.mark.parametrize('kind', ['f32', 'f64'])
def test_label_onehot_truncates_and_gives_zero_rows_for_labels_that_are_no_integer(kind):
    """2.7 -> 2, -0.5 -> 0; NaN, +-inf and values outside the int64 range are no class; a non-integral land-use value matches nothing"""
    dt = np.float32 if kind == 'f32' else np.float64
    lc = np.array([2.7, -0.5, np.nan, np.inf, -np.inf, 300.0, 1.0, 7.0, 1e30, -1e30, 9.3e18, 255.9], dt).reshape(1, 1, 3, 4)
    lu = np.array([82.5, 82.0, 82.0, 0.0, 0.0, 0.0, 338.0, 82.0, np.nan, np.inf, 256.0, 81.999], dt).reshape(1, 1, 3, 4)
    lut = np.full(256, -1, np.int64)
    lut[2], lut[7], lut[255] = 5, -1, 4
    lu_lut = np.full(256, -1, np.int64)
    lu_lut[82] = 3
    got = run_labels(lc, 3, 4, 8, lut).reshape(12, 8)
    assert got.argmax(1).tolist() == [5, 0, 0, 0, 0, 0, 1, 7, 0, 0, 0, 4] and got.sum(1).tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1]
    got = run_labels(lc, 3, 4, 8, lut, lu, lu_lut).reshape(12, 8)
    assert got.argmax(1).tolist() == [5, 3, 3, 0, 0, 0, 1, 3, 0, 0, 0, 4] and got.sum(1).tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1]
    assert np.array_equal(got, I.label_onehot(lc, lut, lu, lu_lut, 3, 4, 8, (0, 0, 0)).reshape(12, 8))


@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_label_onehot_all_morphs_of_a_non_square_tile_in_a_wider_tensor(kind):
    lut, lu_lut = luts()
    (h, w), ncls = (5, 7), 8
    lc = I.label_planes(kind, (3, 1, 8, 12), 1)
    lu = I.landuse_planes('f32', lc.shape, 2)
    base = run_labels(lc, h, w, ncls, lut, lu, lu_lut, ldc=ncls + 5, coff=2)
    for m in I.MORPHS:
        got = run_labels(lc, h, w, ncls, lut, lu, lu_lut, m, ldc=ncls + 5, coff=2)
        assert np.array_equal(got, I.label_onehot(lc, lut, lu, lu_lut, h, w, ncls, m)) and np.array_equal(got, I.morph(base, *m)), m


# ------------------------------------------------------------- past the cap of grid_for (65,536 workgroups)
SIDE = 4100                                     # 16.81 M pixels against 16.78 M threads: some threads take a second trip


def test_tile_ingest_past_the_launch_cap():
    assert SIDE * SIDE > I.GRID_FOR_CAP
    planes = np.random.default_rng(0).integers(0, 256, (1, 1, SIDE, SIDE)).astype(np.uint8)
    got = run_ingest(planes, SIDE, SIDE, rescale=255.0)
    ref = I.tile_ingest(planes, SIDE, SIDE, 255.0)
    for rows in (slice(0, 300), slice(SIDE - 300, SIDE)):
        assert np.array_equal(got[0, rows].view(np.uint32), ref[0, rows].view(np.uint32))
    assert np.array_equal(got, ref)


def test_label_onehot_past_the_launch_cap():
    lc = np.random.default_rng(1).integers(0, 3, (1, 1, SIDE, SIDE)).astype(np.uint8)
    lut = np.full(256, -1, np.int64)
    lut[2] = 0
    got = run_labels(lc, SIDE, SIDE, 1, lut)
    ref = I.label_onehot(lc, lut, None, None, SIDE, SIDE, 1, (0, 0, 0))
    for rows in (slice(0, 300), slice(SIDE - 300, SIDE)):
        assert np.array_equal(got[0, rows].view(np.uint32), ref[0, rows].view(np.uint32))
    assert np.array_equal(got, ref) and 0.6 < ref.mean() < 0.7


# ------------------------------------------------------------------------------- ingest_chw
def check_chw(src, kind, n, c, h, w, cpad, seed=0):
    planes, scale = I.chw_planes(src, (n, c, h, w), seed)
    out, pd = Guarded(n * h * w * cpad * ES[kind]), dev_planes(planes)
    E.check(E.lib.satcv_ingest_chw(pd.data_ptr(), I.kind_of(planes), scale, out.p, n, c, h, w, cpad, CODE[kind], E.st))
    got = out.body(BITS[kind]).reshape(n, h, w, cpad)
    ref = I.storage_bits(I.ingest_chw(planes, scale, cpad, kind), kind)
    assert np.array_equal(got, ref), f'ingest_chw {src} -> {kind} c={c} cpad={cpad}: {int((got != ref).sum())} of {ref.size} differ'
    assert not got[..., c:].any()                                                   # +0 in the pad channels


def chw_past_cap(per_cu=O.EW_PER_CU_DEFAULT):
    """(n, c, h, w, cpad): n h w cpad / 8 takes two full trips at the launch cap and a ragged tail"""
    cap = O.grid_cap_threads(per_cu)
    side = int(np.sqrt(2 * cap / 3)) + 2
    assert 3 * side * (side - 2) > 2 * cap
    return 3, 5, side, side - 2, 8


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('src', I.CHW_SOURCES)
def test_ingest_chw(src, kind):
    """one float32 multiply and one storage rounding; u16 through the unsigned view (values >= 32768 present)"""
    for c, cpad in I.CHW_CASES:
        check_chw(src, kind, 3, c, 5, 7, cpad)


@pytest.mark.parametrize('kind', ['f32', 'bf16'])
@pytest.mark.parametrize('src', I.CHW_SOURCES)
def test_ingest_chw_past_the_launch_cap(src, kind):
    n, c, h, w, cpad = chw_past_cap()
    assert n * h * w * cpad // 8 > 393216
    check_chw(src, kind, n, c, h, w, cpad, seed=1)


# ----------------------------------------------------------------------------- pack_weights
def image_bits(k, mode, cin_pad, kind, el=8):
    return I.storage_bits(I.pack_image(k, mode, cin_pad, el, kind), kind)


def check_pack(shape, transposed, kind, seed=0):
    """both destinations in one call and each alone (the other NULL), NaN-filled, a sentinel right behind ops.packed_sizes elements"""
    from satellite_computervision_amd import ops
    kh, kw, a, b, cin_pad = shape
    cin, cout = (b, a) if transposed else (a, b)
    k = I.pack_kernel_values((kh, kw, a, b), seed + a * b)
    kd = torch.tensor(k).cuda()
    ef, ed, _, _ = ops.packed_sizes(kh, kw, cin, cout, cin_pad, bool(transposed))
    modes = (2, 3) if transposed else (0, 1)
    refs = [image_bits(k, m, cin_pad, kind) for m in modes]
    assert (refs[0].size, refs[1].size) == (ef, ed), 'ops.packed_sizes disagrees with the header'
    owned = [I.pack_owned(k, m, cin_pad) for m in modes]
    what = f'pack_weights {shape} transposed={transposed} {kind}'
    for want_f, want_d in ((1, 1), (1, 0), (0, 1)):
        fwd, dg = Guarded(ef * ES[kind]), Guarded(ed * ES[kind])
        E.check(E.lib.satcv_pack_weights(kd.data_ptr(), fwd.p if want_f else None, dg.p if want_d else None, kh, kw, cin, cout, cin_pad, transposed, CODE[kind], E.st))
        for want, buf, ref, own, name in ((want_f, fwd, refs[0], owned[0], 'fwd'), (want_d, dg, refs[1], owned[1], 'dgrad')):
            if not want:
                assert buf.unchanged(), f'{what}: the {name} image was written although its destination was NULL'
                continue
            got = buf.body(BITS[kind])
            assert not got[~own].any(), f'{what}: {name} padding is not +0 at {int((got[~own] != 0).sum())} elements'
            assert np.array_equal(got, ref), f'{what}: {name} image differs at {int((got != ref).sum())} of {ref.size} elements'


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp8'])
@pytest.mark.parametrize('shape', I.PACK_PLAIN, ids=str)
def test_pack_weights_conv(shape, kind):
    check_pack(shape, 0, kind)


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp8'])
@pytest.mark.parametrize('shape', I.PACK_TRANSPOSED, ids=str)
def test_pack_weights_transposed(shape, kind):
    check_pack(shape, 1, kind)


def check_pack_fp8x(case):
    from satellite_computervision_amd import ops
    kh, kw, a, b, cin_pad, transposed = case
    cin, cout = (b, a) if transposed else (a, b)
    k = I.pack_kernel_values((kh, kw, a, b), 7 + a * b)
    ef = ops.packed_sizes(kh, kw, cin, cout, cin_pad, bool(transposed))[0]
    ref = image_bits(k, 2 if transposed else 0, cin_pad, 'fp8', el=16)
    own = I.pack_owned(k, 2 if transposed else 0, cin_pad, el=16)
    fwd, kd = Guarded(ef), torch.tensor(k).cuda()
    assert ref.size == ef
    E.check(E.lib.satcv_pack_weights(kd.data_ptr(), fwd.p, None, kh, kw, cin, cout, cin_pad, transposed, CODE['fp8x'], E.st))
    got = fwd.body(np.uint8)
    assert not got[~own].any() and np.array_equal(got, ref), f'pack_weights fp8x {case}: {int((got != ref).sum())} of {ref.size} differ'
    if cin_pad > 8:
        assert not np.array_equal(ref, image_bits(k, 2 if transposed else 0, cin_pad, 'fp8', el=8))      # the 16-element image is another image


@pytest.mark.parametrize('case', I.PACK_FP8X, ids=str)
def test_pack_weights_fp8x_sixteen_element_granules(case):
    check_pack_fp8x(case)


# --------------------------------------------------------------------- pack_weights_batched
def check_batched(jobs, kind):
    """every image of one launch against pack_image; the destinations are consecutive slices of one guarded buffer"""
    from satellite_computervision_amd import _lib, ops
    srcs, cjobs, refs, offs, tot = {}, [], [], [], 0
    for job in jobs:
        kh, kw, cin, cout, cp, mode = job
        shape = I.job_kernel_shape(job)
        if shape not in srcs:
            k = I.pack_kernel_values(shape, 11 + len(srcs))
            srcs[shape] = (k, torch.tensor(k).cuda())
        refs.append(image_bits(srcs[shape][0], mode, cp, kind))
        offs.append(tot)
        tot += refs[-1].size * ES[kind]
    out = Guarded(tot)
    for job, off in zip(jobs, offs):
        kh, kw, cin, cout, cp, mode = job
        _, kpad, npad = I.pack_dims(mode, kh * kw, cin, cout, cp)
        cjobs.append(_lib.PackJob(src=srcs[I.job_kernel_shape(job)][1].data_ptr(), dst=out.p + off, mode=mode, taps=kh * kw, cin=cin, cout=cout, kpad=kpad, npad=npad))
    for cj, job in zip(cjobs, jobs):
        real = I.job_real_items(job)
        assert E.lib.satcv_pack_job_items(C.byref(cj)) == I.rup(real, 256), f'pack_job_items {job}'
    tab = ops.job_table(cjobs, E.lib.satcv_pack_job_items, 'cuda')
    assert tab['total'] == sum(I.rup(I.job_real_items(j), 256) for j in jobs)
    E.check(E.lib.satcv_pack_weights_batched(tab['jobs'].data_ptr(), tab['prefix'].data_ptr(), tab['n'], tab['total'], CODE[kind], E.st))
    body = out.body()
    for job, off, ref in zip(jobs, offs, refs):
        got = body[off:off + ref.size * ES[kind]].view(BITS[kind])
        assert np.array_equal(got, ref), f'pack_weights_batched {kind} job {job}: {int((got != ref).sum())} of {ref.size} elements differ'


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp8'])
def test_pack_weights_batched(kind):
    """the whole table in one launch: 589,824 items of the two 512-channel images alone, past the default cap, so a workgroup's later trips
    fall into other jobs; the remapped data-gradient path (kpad % 32 == 0) and the plain one against the same oracle"""
    jobs = I.batched_jobs()
    assert sum(I.rup(I.job_real_items(j), 256) for j in jobs) > G.CAP
    check_batched(jobs, kind)


@pytest.mark.parametrize('kind', ['f32', 'bf16', 'fp8'])
def test_pack_weights_batched_single_jobs(kind):
    """njobs = 1: a job whose item count is a multiple of 256, one 64 over a multiple, a remapped one, a transposed one"""
    singles = [(3, 3, 64, 64, 64, 1), (3, 3, 64, 64, 64, 0), (3, 3, 13, 24, 16, 1), (3, 3, 13, 24, 16, 0), (1, 1, 32, 2, 32, 0), (2, 2, 32, 64, 32, 3), (3, 3, 48, 48, 48, 1)]
    real = [I.job_real_items(j) for j in singles]
    assert any(r % 256 == 0 for r in real) and any(r % 256 == 64 for r in real)
    for job in singles:
        check_batched([job], kind)


def test_pack_weights_batched_remapped_and_plain_paths_agree_with_the_per_layer_packer():
    """the same kernel through satcv_pack_weights (no remap) and as a batched mode-1 job on the remapped path: the same bytes"""
    from satellite_computervision_amd import _lib, ops
    k = I.pack_kernel_values((3, 3, 32, 64), 5)
    kd = torch.tensor(k).cuda()
    ed = ops.packed_sizes(3, 3, 32, 64, 32, False)[1]
    for kind in ('f32', 'bf16', 'fp8'):
        a, b = Guarded(ed * ES[kind]), Guarded(ed * ES[kind])
        E.check(E.lib.satcv_pack_weights(kd.data_ptr(), None, a.p, 3, 3, 32, 64, 32, 0, CODE[kind], E.st))
        job = _lib.PackJob(src=kd.data_ptr(), dst=b.p, mode=1, taps=9, cin=32, cout=64, kpad=64, npad=32)
        tab = ops.job_table([job], E.lib.satcv_pack_job_items, 'cuda')
        E.check(E.lib.satcv_pack_weights_batched(tab['jobs'].data_ptr(), tab['prefix'].data_ptr(), 1, tab['total'], CODE[kind], E.st))
        assert np.array_equal(a.body(), b.body()) and np.array_equal(a.body(BITS[kind]), image_bits(k, 1, 32, kind))


# ------------------------------------------------------------------------------- refusals
def refused(rc, names, outs):
    assert rc != 0, 'the call should have been refused'
    msg = last_error()
    assert any(nm in msg for nm in ([names] if isinstance(names, str) else names)), f'the error message does not name its entry point: {msg!r}'
    for o in outs:
        assert o.unchanged(), 'a refused call wrote to its output'


def test_tile_kernels_refuse_bad_arguments():
    planes = I.make_planes('f32', (2, 3, 8, 10), 0)
    src = dev_planes(planes)
    out, mean_out = Guarded(2 * 5 * 7 * 8 * 4), Guarded(6 * 8)
    mean = torch.zeros(6, dtype=torch.float64).cuda()

    def base(**kw):
        d = tile_desc(src, planes, 5, 7, dst=out.p, ldc=8, coff=2)
        for key, v in kw.items():
            setattr(d, key, v)
        return d
    ok8, ok5 = Guarded(2 * 5 * 7 * 8 * 4), Guarded(2 * 5 * 7 * 5 * 4)
    E.check(E.lib.satcv_tile_ingest(C.byref(base(dst=ok8.p)), E.st))                                  # the base descriptor itself is accepted
    bad_dims = [dict(src=None), dict(n=0), dict(n=-1), dict(c=0), dict(h=0), dict(w_=0), dict(w_=-3), dict(hin=4), dict(win=6), dict(src_kind=7), dict(src_kind=-1),
                dict(rot=4), dict(rot=-1)]
    ingest_only = [dict(dst=None), dict(nan_mask=3), dict(nan_mask=-1), dict(nan_mask=1, ch_mean=mean.data_ptr()), dict(ldc=4), dict(nan_mask=1, ldc=5, coff=2),
                   dict(coff=-1), dict(coff=-2, ldc=1), dict(nan_mask=2, coff=-1)]
    for kw in bad_dims + ingest_only:
        refused(E.lib.satcv_tile_ingest(C.byref(base(**kw)), E.st), 'tile_ingest', [out])
    refused(E.lib.satcv_tile_ingest(None, E.st), 'tile_ingest', [out])
    for kw in bad_dims:
        refused(E.lib.satcv_tile_channel_mean(C.byref(base(**kw)), mean_out.p, E.st), 'tile_channel_mean', [mean_out])
    refused(E.lib.satcv_tile_channel_mean(C.byref(base()), None, E.st), 'tile_channel_mean', [mean_out])
    refused(E.lib.satcv_tile_channel_mean(None, mean_out.p, E.st), 'tile_channel_mean', [mean_out])
    assert E.lib.satcv_tile_ingest(C.byref(base(ldc=5, dst=ok5.p)), E.st) == 0                          # ldc exactly coff + c
    ok8.body(), ok5.body()


def test_label_onehot_refuses_bad_arguments():
    lc = dev_planes(np.ones((2, 1, 8, 10), np.uint8))
    lu = dev_planes(np.ones((2, 1, 8, 10), np.float32))
    lut = torch.zeros(256, dtype=torch.int32).cuda()
    out = Guarded(2 * 5 * 7 * 8 * 4)

    def call(lc_=lc.data_ptr(), lc_kind=0, lu_=None, lu_kind=0, lu_lut=None, n=2, hin=8, win=10, h=5, w=7, ncls=4, rot=0, dst=out.p, ldc=8, coff=2):
        return E.lib.satcv_label_onehot(lc_, lc_kind, lut.data_ptr(), lu_, lu_kind, lu_lut, n, hin, win, h, w, ncls, 0, 0, rot, dst, ldc, coff, E.st)
    bad = [dict(lc_=None), dict(dst=None), dict(n=0), dict(h=0), dict(w=0), dict(w=-1), dict(hin=4), dict(win=6), dict(ncls=0), dict(ldc=5), dict(coff=-1),
           dict(coff=-4, ldc=1), dict(lc_kind=7), dict(lc_kind=-1), dict(lu_=lu.data_ptr(), lu_kind=7, lu_lut=lut.data_ptr()),
           dict(lu_=lu.data_ptr(), lu_kind=-1, lu_lut=lut.data_ptr()), dict(lu_=lu.data_ptr(), lu_kind=2, lu_lut=None), dict(rot=4), dict(rot=-1)]
    for kw in bad:
        refused(call(**kw), 'label_onehot', [out])
    ok6 = Guarded(2 * 5 * 7 * 6 * 4)
    assert call(ldc=6, dst=ok6.p) == 0                                                                # ldc exactly coff + ncls
    ok6.body()


def test_ingest_chw_refuses_bad_arguments():
    src = dev_planes(np.ones((2, 3, 5, 7), np.float32))
    out = Guarded(2 * 5 * 7 * 8 * 4)

    def call(src_=src.data_ptr(), kind=2, dst=out.p, n=2, c=3, h=5, w=7, cpad=8, dtype=0):
        return E.lib.satcv_ingest_chw(src_, kind, 1.0, dst, n, c, h, w, cpad, dtype, E.st)
    for kw in [dict(src_=None), dict(dst=None), dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(h=-5, w=-7), dict(c=9), dict(cpad=12), dict(cpad=0), dict(kind=3),
               dict(kind=-1), dict(dtype=2), dict(dtype=7), dict(dtype=-1)]:
        refused(call(**kw), 'ingest_chw', [out])
    assert call() == 0
    out.body()


def test_pack_weights_refuse_bad_arguments():
    from satellite_computervision_amd import _lib
    k = torch.ones(3 * 3 * 20 * 32).cuda()
    fwd, dg = Guarded(9 * 32 * 32 * 4), Guarded(9 * 32 * 32 * 4)

    def call(src=k.data_ptr(), f=fwd.p, d=dg.p, kh=3, kw=3, cin=20, cout=32, cin_pad=32, transposed=0, dtype=0):
        return E.lib.satcv_pack_weights(src, f, d, kh, kw, cin, cout, cin_pad, transposed, dtype, E.st)
    for kw in [dict(src=None), dict(cin=0), dict(cout=0), dict(cout=-32), dict(kh=0), dict(kw=0), dict(kh=-3, kw=-3), dict(cin_pad=16), dict(cin_pad=24), dict(cin_pad=40),
               dict(dtype=3), dict(dtype=3, f=None), dict(dtype=3, f=None, d=None), dict(dtype=7), dict(dtype=4), dict(dtype=-1)]:
        refused(call(**kw), 'pack_weights', [fwd, dg])

    def job(**kw):
        j = _lib.PackJob(src=k.data_ptr(), dst=fwd.p, mode=0, taps=9, cin=20, cout=32, kpad=32, npad=32)
        for key, v in kw.items():
            setattr(j, key, v)
        return j
    assert E.lib.satcv_pack_job_items(C.byref(job())) == I.rup(9 * 4 * 32, 256)
    for kw in [dict(taps=0), dict(taps=-9), dict(cin=0), dict(cout=0), dict(cout=-1), dict(kpad=0), dict(kpad=20), dict(npad=0), dict(mode=4), dict(mode=-1)]:
        assert E.lib.satcv_pack_job_items(C.byref(job(**kw))) == -1, kw
    assert E.lib.satcv_pack_job_items(None) == -1
    jobs = torch.zeros(64, dtype=torch.uint8).cuda()
    prefix = torch.zeros(1, dtype=torch.int64).cuda()
    for args in [(None, prefix.data_ptr(), 1, 1280, 0), (jobs.data_ptr(), None, 1, 1280, 0), (jobs.data_ptr(), prefix.data_ptr(), 0, 1280, 0),
                 (jobs.data_ptr(), prefix.data_ptr(), -1, 1280, 0), (jobs.data_ptr(), prefix.data_ptr(), 1, 0, 0), (jobs.data_ptr(), prefix.data_ptr(), 1, 1152 + 64, 0),
                 (jobs.data_ptr(), prefix.data_ptr(), 1, 1280, 3), (jobs.data_ptr(), prefix.data_ptr(), 1, 1280, 7)]:
        refused(E.lib.satcv_pack_weights_batched(*args, E.st), 'pack_weights_batched', [fwd, dg])
    G.sync()


# ------------------------------------------------------------------------------- child process
def run_small_grid_child():
    """SATCV_EW_PER_CU=1 (256 workgroups): the ingest_chw cases, the pack_weights cases and the batched table with a 3x3x256x256 job in the
    place of the 512 one; every pack image of more than 65,536 items now takes several trips"""
    assert os.environ.get('SATCV_EW_PER_CU') == '1'
    assert E.lib.satcv_bias_grad_workspace(10 ** 6, 8) == 256 * 8 * 4, 'the launch cap did not follow SATCV_EW_PER_CU'
    n, c, h, w, cpad = chw_past_cap(1)
    for kind in ('f32', 'bf16'):
        for src in I.CHW_SOURCES:
            for cc, cp in I.CHW_CASES:
                check_chw(src, kind, 3, cc, 5, 7, cp)
            check_chw(src, kind, n, c, h, w, cpad, seed=1)
    for kind in ('f32', 'bf16', 'fp8'):
        for shape in I.PACK_PLAIN:
            check_pack(shape, 0, kind)
        for shape in I.PACK_TRANSPOSED:
            check_pack(shape, 1, kind)
        jobs = I.batched_jobs(256)
        assert sum(I.rup(I.job_real_items(j), 256) for j in jobs) > 2 * O.grid_cap_threads(1)
        check_batched(jobs, kind)
    for case in I.PACK_FP8X:
        check_pack_fp8x(case)
    print('small-grid child ok')


def test_input_kernels_with_one_workgroup_per_cu():
    """SATCV_EW_PER_CU is read once per process: a fresh child, its own time limit, exit status checked, nothing started after it"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import test_input_kernels_gpu as T; T.run_small_grid_child()' % (ROOT, HERE)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, SATCV_EW_PER_CU='1'), capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1] == 'small-grid child ok'


if __name__ == '__main__':      # the record: the `[fig]` line closest to its bound per test and kind of check
    import contextlib
    import io
    import re
    _buf = io.StringIO()
    with contextlib.redirect_stdout(_buf):
        _rc = pytest.main([os.path.abspath(__file__), '-m', 'gpu', '-q', '-rP', '-p', 'no:cacheprovider'])
    _worst, _test = {}, '?'
    for _ln in _buf.getvalue().splitlines():
        _m = re.match(r'_+ (test_\w+)', _ln)
        if _m:
            _test = _m.group(1)
        if _ln.startswith('[fig] '):
            _check, _rest = _ln[6:].split(' | ', 1)
            _frac = float(_rest.rsplit(': ', 1)[1].split(' ')[0])
            if _frac >= _worst.get((_test, _check), (-1.0, ''))[0]:
                _worst[(_test, _check)] = (_frac, _ln)
    _tail = [ln for ln in _buf.getvalue().splitlines() if ' passed' in ln or ' failed' in ln][-1:]
    with open(os.path.join(ROOT, 'profiles', 'input_kernels_parity.txt'), 'w') as _f:
        _f.write('# tests/test_input_kernels_gpu.py: per test and kind of check, the outcome closest to its bound (fraction of the bound)\n')
        for (_t, _c), (_fr, _ln) in sorted(_worst.items()):
            _f.write(f'{_t}: {_ln}\n')
        _f.write('# every other check of the file is an equality of bits\n# ' + ' '.join(_tail) + '\n')
    print(_buf.getvalue()[-3000:])
    sys.exit(int(_rc))
