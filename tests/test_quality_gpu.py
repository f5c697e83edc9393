"""Quality masks and the masked composite on the GPU: satcv_quality_mask against the exact integer restatement of utils/ee_tools.py
(tests/quality_oracle.py) -- clear bits for each rule alone and for the presets, the cloud score, the water score --, and
satcv_median_composite_masked against the composite oracle, against the existing kernel on a host-zeroed stack, and against the
existing entry point without a mask; the Python surface (ee_tools, median_composite(clear=, bands=), predict_change(quality=)).

Tolerances (derived, not measured): clear bits and cloud scores are exact.  water_score is a double evaluation rounded once to fp32 on
values in [0, 1]: the rounding errs by at most 2^-24 = 6e-8, and 1e-6 absolute leaves room for the order of operations against the
literal float64 form.  The masked composite is held to the bounds of test_composite_gpu: `median` bit-equal to the oracle rounded to
float32, `norm` within 2 float32 ulp or within 8 c 2^-53 max|median| / (sd + 1e-6) absolute where that is larger."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

KIND = {np.uint16: 1, np.float32: 2, np.int16: 3}
DEPTHS = [1, 2, 5, 8, 17, 32, 33, 70]                        # every network size, both parities, one and several mask words
SHAPES = [(37, 53), (3, 1301), (4, 10), (1, 1)]              # odd pixel counts for the two-pixel lanes, a row wider than a workgroup's span,
                                                             # a small even map, and the one-pixel map (general path, one pixel per lane)
CASES = [(dtype, t) for dtype in (np.uint16, np.int16, np.float32) for t in DEPTHS]
IDS = [f'{d.__name__}-{t}' for d, t in CASES]


@pytest.fixture(scope='module')
def env():
    import composite_oracle as O
    import quality_oracle as Q
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, pc_tools as pc, ee_tools as ee, _lib
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pt=pt, pc=pc, ee=ee, L=_lib, O=O, Q=Q)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bands_of(env, dtype, t):
    Q = env['Q']
    return Q.BANDS14 if (t + KIND[dtype]) % 2 else Q.BANDS9


def _quality(env, stack, bands, rules, offsets, clear=True, cloud=False, water=False):
    """one launch -> (words uint32 | None, cloud uint8 | None, water float32 | None) on the host; outputs start from sentinels"""
    L, ops, ee = env['L'], env['ops'], env['ee']
    t, cs, H, W = stack.shape
    src = _dev(stack)
    off = _dev(offsets) if offsets is not None else None
    words = torch.full(((t + 31) // 32, H, W), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    cl = torch.full((t, H, W), 199, dtype=torch.uint8, device='cuda')
    wa = torch.full((t, H, W), -777.0, dtype=torch.float32, device='cuda')
    d = L.QualityDesc(src=src.data_ptr(), src_kind=KIND[stack.dtype.type], t=t, cs=cs, h=H, w_=W, offsets=off.data_ptr() if off is not None else None,
                      band=(C.c_int32 * 10)(*ee.band_table(bands)), rules=rules, cloud_max=15, shadow_min=900.0,
                      clear=words.data_ptr() if clear else None, cloud_score=cl.data_ptr() if cloud else None, water_score=wa.data_ptr() if water else None)
    L.check(L.lib.satcv_quality_mask(C.byref(d), ops.stream_ptr()))
    words, cl, wa = words.cpu().numpy().view(np.uint32), cl.cpu().numpy(), wa.cpu().numpy()
    assert clear or np.all(words == 0x5a5a5a5a)
    assert cloud or np.all(cl == 199)
    assert water or np.all(wa == -777.0)
    return (words if clear else None), (cl if cloud else None), (wa if water else None)


def _assert_planted(Q, passes, score, t, bands):
    """the planted cases are present in the oracle's output: a missing one is an error of the test"""
    flat = lambda a: a.reshape(t, -1)
    toa = flat(Q.combine(passes, Q.PRESETS['toa']))
    assert not toa[:, Q.P_NONE].any() and toa[:, Q.P_ALL].all() and toa[:, Q.P_ONE].sum() == 1 and toa[:, Q.P_TWO].sum() == min(2, t)
    s, cloud = flat(score), flat(passes[Q.CLOUD])
    for k in range(6):
        assert np.all(s[:, Q.P_TERM0 + 2 * k] == 16) and not cloud[:, Q.P_TERM0 + 2 * k].any(), k
        assert np.all(s[:, Q.P_TERM0 + 2 * k + 1] == 15) and cloud[:, Q.P_TERM0 + 2 * k + 1].all(), k
    qa = flat(passes[Q.QA60])
    assert not qa[:, Q.P_QA10].any() and not qa[:, Q.P_QA11].any() and qa[:, Q.P_SCL0].all()
    if 'SCL' in bands:
        assert not flat(passes[Q.SCL])[:, Q.P_SCL0].any() and flat(passes[Q.SCL])[:, Q.P_QA10].all()
    assert np.all(s[:, Q.P_NODATA_BAND] == 255) and not flat(passes[Q.SHADOW])[:, Q.P_NODATA_BAND].any() and qa[:, Q.P_NODATA_BAND].all()


# ---------------------------------------------------------------------------------------------------------------- 1. the mask kernel
@pytest.mark.parametrize('dtype,t', CASES, ids=IDS)
def test_mask_kernel_equals_the_exact_form(env, dtype, t):
    Q = env['Q']
    bands = _bands_of(env, dtype, t)
    worst = 0.0
    for H, W in SHAPES:
        stack, offsets = Q.make_stack(100 * t + KIND[dtype], dtype, t, H, W, bands)
        for offs in ((offsets, None) if (H, W) == (37, 53) else (offsets,)):
            what = f'{dtype.__name__} t={t} {H}x{W} {len(bands)} planes offsets={offs is not None}'
            passes = Q.rule_passes(stack, bands, offs)
            score = Q.cloud_score_exact(stack, bands, offs)
            if H * W >= Q.PLANTED_PIXELS and offs is not None:
                _assert_planted(Q, passes, score, t, bands)
            rule_sets = [r for r in (Q.QA60, Q.CLOUD, Q.SHADOW, Q.WATER, Q.SCL) if r in passes] + [v for k, v in Q.PRESETS.items() if k != 'sr' or Q.SCL in passes]
            for rules in rule_sets:
                want = Q.pack_bits(Q.combine(passes, rules))
                # the 'mask' preset also writes both scores in the same launch
                both = rules == Q.PRESETS['mask']
                words, cl, wa = _quality(env, stack, bands, rules, offs, cloud=both, water=both)
                assert np.array_equal(words, want), (what, rules, int((words != want).sum()))         # unused high bits included
                if both:
                    assert np.array_equal(cl, score), (what, int((cl != score).sum()))
                    lit = Q.water_score_float(stack, bands, offs)
                    assert np.array_equal(np.isnan(wa), np.isnan(lit)), what
                    ok = ~np.isnan(lit)
                    if ok.any():
                        worst = max(worst, float(np.abs(wa[ok] - lit[ok]).max()))
                        assert wa[ok].min() >= 0 and wa[ok].max() <= 1
            # the scores alone: no rule, no clear output, only their planes are read
            _, cl, _ = _quality(env, stack, bands, 0, offs, clear=False, cloud=True)
            assert np.array_equal(cl, score), what
    print(f'{dtype.__name__} t={t}: water_score max |err| vs the literal float64 form {worst:.3e}')
    assert worst <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 2. the masked composite
def _check(O, got_med, got_norm, want_med, want_norm, c, what):
    """(as in test_composite_gpu) every pixel and band takes part: NaN patterns equal, median bit-equal, norm within the derived bounds"""
    wm, wn = want_med.astype(np.float32), want_norm.astype(np.float32)
    assert np.array_equal(np.isnan(got_med), np.isnan(wm)), what
    assert np.array_equal(np.isnan(got_norm), np.isnan(wn)), what
    ok = ~np.isnan(wm)
    assert np.array_equal(got_med[ok].view(np.uint32), wm[ok].view(np.uint32)), (what, np.abs(got_med[ok] - wm[ok]).max())
    ok = ~np.isnan(wn)
    ulp = O.ulp_distance(np.where(ok, got_norm, 0), np.where(ok, wn, 0))
    err = np.abs(np.where(ok, got_norm.astype(np.float64) - want_norm, 0))
    bound = np.broadcast_to(O.norm_bound(want_med, c), err.shape)
    print(f'{what}: norm max ulp {ulp.max()}, max |err| {err.max():.3e}, pixels on the absolute bound {int(((ulp > 2) & (err <= bound)).sum())}')
    assert np.all((ulp <= 2) | (err <= bound)), (what, ulp.max(), err.max())


def _bit_equal(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint32), b[~np.isnan(b)].view(np.uint32))


def _composite(env, stack, offsets, ld_med, coff_med, ld_norm, coff_norm, fill=None, masked=False, words=None, idx=None):
    """the existing entry point, or (masked) the new one with `words` (uint32 bit-planes or None) and the band table `idx`"""
    L, ops = env['L'], env['ops']
    t, cs, H, W = stack.shape
    c = len(idx) if idx is not None else cs
    src = _dev(stack)
    off = _dev(offsets) if offsets is not None else None
    med = torch.full((H, W, ld_med), -777.0, dtype=torch.float32, device='cuda')
    nrm = torch.full((H, W, ld_norm), -777.0, dtype=torch.float32, device='cuda')
    d = L.CompositeDesc(src=src.data_ptr(), src_kind=KIND[stack.dtype.type], t=t, c=c, h=H, w_=W, offsets=off.data_ptr() if off is not None else None,
                        median=med.data_ptr(), ld_med=ld_med, coff_med=coff_med, norm=nrm.data_ptr(), ld_norm=ld_norm, coff_norm=coff_norm,
                        use_fill=int(fill is not None), fill=float(fill or 0.0))
    if masked:
        w = _dev(words) if words is not None else None
        table = list(idx if idx is not None else range(cs)) + [0] * 16
        md = L.CompositeMaskedDesc(base=d, clear=w.data_ptr() if w is not None else None, cs=cs, band_idx=(C.c_int32 * 16)(*table[:16]))
        L.check(L.lib.satcv_median_composite_masked(C.byref(md), ops.stream_ptr()))
    else:
        L.check(L.lib.satcv_median_composite(C.byref(d), ops.stream_ptr()))
    return med.cpu().numpy(), nrm.cpu().numpy()


@pytest.mark.parametrize('dtype,t', CASES, ids=IDS)
def test_masked_composite_equals_the_oracle_and_the_existing_kernel(env, dtype, t):
    O, Q = env['O'], env['Q']
    bands = _bands_of(env, dtype, t)
    idx = [bands.index(b) for b in ('B2', 'B3', 'B4', 'B8')]
    c = 4
    for H, W in SHAPES:
        stack, offsets = Q.make_stack(100 * t + KIND[dtype], dtype, t, H, W, bands)
        clear = Q.clear_exact(stack, bands, Q.PRESETS['toa'], offsets)
        words = Q.pack_bits(clear)
        if H * W >= Q.PLANTED_PIXELS:
            n = clear.reshape(t, -1).sum(axis=0)
            assert n[Q.P_NONE] == 0 and n[Q.P_ALL] == t and n[Q.P_ONE] == 1 and n[Q.P_TWO] == min(2, t)
        what = f'{dtype.__name__} t={t} {H}x{W} {len(bands)} planes'
        want_med, want_norm = Q.masked_composite(stack, clear, offsets, idx)
        if H * W >= Q.PLANTED_PIXELS:
            assert np.isnan(want_med.reshape(-1, c)[Q.P_NONE]).all() and not np.isnan(want_med.reshape(-1, c)[Q.P_ALL]).any()
        zeroed = Q.zero_unclear(stack, clear, idx)
        # tight outputs (16-byte stores)
        med, nrm = _composite(env, stack, offsets, c, 0, c, 0, masked=True, words=words, idx=idx)
        _check(O, med, nrm, want_med, want_norm, c, what)
        ymed, ynrm = _composite(env, zeroed, offsets, c, 0, c, 0)                        # the existing kernel as the yardstick
        assert _bit_equal(med, ymed) and _bit_equal(nrm, ynrm), what
        # wide outputs at a channel offset (scalar stores), fill: the sentinel outside the channel range survives
        med, nrm = _composite(env, stack, offsets, c + 3, 2, 2 * c + 1, c, fill=0.0, masked=True, words=words, idx=idx)
        ymed, ynrm = _composite(env, zeroed, offsets, c + 3, 2, 2 * c + 1, c, fill=0.0)
        assert np.array_equal(med, ymed, equal_nan=True) and np.array_equal(nrm, ynrm) and not np.isnan(nrm).any(), what
        assert np.all(np.delete(med, np.s_[2:2 + c], axis=-1) == -777.0) and np.all(np.delete(nrm, np.s_[c:2 * c], axis=-1) == -777.0)
        assert _bit_equal(med[..., 2:2 + c], want_med.astype(np.float32)), what


@pytest.mark.parametrize('dtype,t', [(np.uint16, 5), (np.uint16, 32), (np.int16, 12), (np.int16, 33), (np.float32, 8), (np.float32, 70)],
                         ids=lambda v: getattr(v, '__name__', str(v)))
def test_without_a_mask_the_new_entry_point_is_the_existing_one(env, dtype, t):
    """clear = NULL and the identity band table: bit-equal to satcv_median_composite on the same stack, every plane taking part"""
    Q = env['Q']
    for H, W in SHAPES:
        stack, offsets = Q.make_stack(9 * t, dtype, t, H, W, Q.BANDS9)
        if dtype == np.float32:
            stack = np.where(np.isnan(stack), np.float32(0), stack)                       # (every plane is a band here, the codes too)
        c = 9
        for args in ((c, 0, c, 0, None), (c + 3, 2, 2 * c + 1, c, None), (c + 3, 2, 2 * c + 1, c, 0.0), (12, 0, 12, 0, 0.0)):
            a = _composite(env, stack, offsets, *args[:4], fill=args[4])
            b = _composite(env, stack, offsets, *args[:4], fill=args[4], masked=True)
            assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True), (H, W, args)
            assert np.all(np.delete(a[0], np.s_[args[1]:args[1] + c], axis=-1) == -777.0) and np.all(np.delete(a[1], np.s_[args[3]:args[3] + c], axis=-1) == -777.0)


def test_band_selection_equals_a_stack_built_from_those_planes(env):
    Q = env['Q']
    for dtype, t in ((np.uint16, 8), (np.float32, 17), (np.int16, 33)):
        for H, W in SHAPES[:3]:
            stack, offsets = Q.make_stack(5 * t, dtype, t, H, W, Q.BANDS14)
            idx = [1, 2, 3, 7]
            sub = np.ascontiguousarray(stack[:, idx])
            if dtype == np.float32:
                stack, sub = np.nan_to_num(stack, nan=0.0), np.nan_to_num(sub, nan=0.0)
            want = _composite(env, sub, offsets, 4, 0, 4, 0)
            got = _composite(env, stack, offsets, 4, 0, 4, 0, masked=True, idx=idx)
            assert _bit_equal(got[0], want[0]) and _bit_equal(got[1], want[1]), (dtype, t, H, W)
            # ... and under a mask
            clear = Q.clear_exact(stack, Q.BANDS14, Q.PRESETS['sr'], offsets)
            want = _composite(env, Q.zero_unclear(stack, clear, idx), offsets, 4, 0, 4, 0)
            got = _composite(env, stack, offsets, 4, 0, 4, 0, masked=True, words=Q.pack_bits(clear), idx=idx)
            assert _bit_equal(got[0], want[0]) and _bit_equal(got[1], want[1]), (dtype, t, H, W)
            assert not _bit_equal(got[0], _composite(env, sub, offsets, 4, 0, 4, 0)[0])   # the mask takes part


# ---------------------------------------------------------------------------------------------------------------- 3. the Python surface
def test_ee_tools_functions_equal_the_oracle(env):
    ee, pc, Q, O = env['ee'], env['pc'], env['Q'], env['O']
    t, H, W = 33, 37, 53
    stack, offsets = Q.make_stack(77, np.uint16, t, H, W, Q.BANDS14)
    names = [b.replace('B1', 'B01') if b == 'B1' else b.replace('B8', 'B08') if b == 'B8' else b for b in Q.BANDS14]      # B01 / B08 spellings
    passes = Q.rule_passes(stack, Q.BANDS14, offsets)
    for fn, rules in ((ee.basicQA, Q.QA60), (ee.maskTOA, Q.PRESETS['toa']), (ee.maskSR, Q.PRESETS['sr']), (ee.mask, Q.PRESETS['mask'])):
        m = fn(stack, names, offsets=offsets)
        assert isinstance(m, ee.ClearMask) and m.T == t and m.shape == (t, H, W) and m.words.is_cuda
        want = Q.combine(passes, rules)
        assert np.array_equal(m.numpy(), want) and np.array_equal(m.count(), want.sum(axis=0)), fn.__name__
    m = ee.mask(stack, names, offsets=offsets, rules=['cloud', 'shadow'])
    assert np.array_equal(m.numpy(), Q.combine(passes, Q.CLOUD | Q.SHADOW))
    cs = ee.sentinelCloudScore(stack, names, offsets=offsets)
    assert cs.is_cuda and cs.dtype == torch.uint8 and np.array_equal(cs.cpu().numpy(), Q.cloud_score_exact(stack, Q.BANDS14, offsets))
    ws = ee.waterScore(stack, names, offsets=offsets)
    lit = Q.water_score_float(stack, Q.BANDS14, offsets)
    assert ws.dtype == torch.float32 and np.array_equal(np.isnan(ws.cpu().numpy()), np.isnan(lit))
    assert np.nanmax(np.abs(ws.cpu().numpy() - lit)) <= 1e-6
    # a resident int16 tensor, harmonisation from times
    from datetime import datetime
    st16, _ = Q.make_stack(78, np.int16, 6, H, W, Q.BANDS9)
    times = [datetime(2022, 1, 22 + d) for d in range(6)]
    offs = pc.harmonize_offsets(times)
    m = ee.maskTOA(torch.from_numpy(st16).cuda(), Q.BANDS9, times=times)
    want = Q.clear_exact(st16, Q.BANDS9, Q.PRESETS['toa'], offs)
    assert np.array_equal(m.numpy(), want)
    # median_composite(clear=, bands=): by name and by index, against the oracle
    sel = ['B02', 'B03', 'B04', 'B08']
    idx = [Q.BANDS9.index(b) for b in ('B2', 'B3', 'B4', 'B8')]
    med, nrm = pc.median_composite(st16, times=times, clear=m, bands=sel, band_names=Q.BANDS9)
    med2, nrm2 = pc.median_composite(st16, offsets=offs, clear=m, bands=idx)
    assert med.shape == (H, W, 4) and torch.equal(med.isnan(), med2.isnan()) and torch.equal(med.nan_to_num(-1.0), med2.nan_to_num(-1.0))
    wm, wn = Q.masked_composite(st16, want, offs, idx)
    _check(O, med.cpu().numpy(), nrm.cpu().numpy(), wm, wn, 4, 'median_composite(clear=, bands=)')
    with pytest.raises(ValueError, match='clear mask is for a stack'):
        pc.median_composite(stack, clear=m)


def _randomise(m, seed):
    rng = np.random.default_rng(seed + 13)
    w = {}
    for ps in m.param_specs:
        if ps.kind == 'kernel':
            w[ps.name] = (rng.standard_normal(ps.shape) * np.sqrt(2.0 / np.prod(ps.shape[:3]))).astype(np.float32)
        elif ps.kind == 'moving_var':
            w[ps.name] = (0.5 + rng.random(ps.shape)).astype(np.float32)
        elif ps.kind == 'gamma':
            w[ps.name] = (1 + 0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
        else:
            w[ps.name] = (0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
    m.set_weights_dict(w)


def _unet8(mt):
    mt.reset_uids(); mt.set_seed(6)
    m = mt.get_unet_model(2, 8, filters=[32, 64], factors=[2, 2])
    m.compute_dtype = 'bfloat16'
    _randomise(m, 6)
    return m


def test_predict_change_with_quality_masks(env, monkeypatch):
    ee, pc, pt, mt, Q = env['ee'], env['pc'], env['pt'], env['mt'], env['Q']
    H = W = 152
    before, boff = Q.make_stack(61, np.uint16, 5, H, W, Q.BANDS9)
    after, aoff = Q.make_stack(62, np.uint16, 4, H, W, Q.BANDS9)
    from datetime import datetime
    bt = [datetime(2022, 1, 22 + d) for d in range(5)]                                   # the later halves fall after the cutoff, as make_stack's offsets
    at = [datetime(2022, 1, 23 + d) for d in range(4)]
    assert np.array_equal(pc.harmonize_offsets(bt), boff) and np.array_equal(pc.harmonize_offsets(at), aoff)
    sel = ['B2', 'B3', 'B4', 'B8']
    m = _unet8(mt)
    kw = dict(before_times=bt, after_times=at, buff=16, kernel=32, batch_size=4, fill=0.0, band_names=Q.BANDS9, bands=sel)
    warm = pc.predict_change(before, after, m, quality='toa', **kw)                      # plan construction may synchronise
    # the same scene from two median_composite(clear=...) calls through predict_scene
    scene = torch.empty((H, W, 8), dtype=torch.float32, device='cuda')
    bm, _ = pc.median_composite(before, times=bt, fill=0.0, out=scene, channel_offset=0, clear=ee.maskTOA(before, Q.BANDS9, times=bt), bands=sel, band_names=Q.BANDS9)
    am, _ = pc.median_composite(after, times=at, fill=0.0, out=scene, channel_offset=4, clear=ee.maskTOA(after, Q.BANDS9, times=at), bands=sel, band_names=Q.BANDS9)
    want = pt.predict_scene(scene, m, kernel=32, buff=16, batch_size=4)
    assert warm[0].shape == (H, W) and warm[0].max() > 0 and np.array_equal(warm[0], want)
    assert np.array_equal(warm[1], bm.cpu().numpy(), equal_nan=True) and np.array_equal(warm[2], am.cpu().numpy(), equal_nan=True)
    # the returned medians are the masked ones: the oracle's
    idx = [Q.BANDS9.index(b) for b in sel]
    wbm, _ = Q.masked_composite(before, Q.clear_exact(before, Q.BANDS9, Q.PRESETS['toa'], boff), boff, idx)
    assert _bit_equal(warm[1], wbm.astype(np.float32))
    # a pair of ClearMasks is the same thing
    pair = pc.predict_change(before, after, m, quality=(ee.maskTOA(before, Q.BANDS9, times=bt), ee.maskTOA(after, Q.BANDS9, times=at)), **kw)
    assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(pair, warm))
    # it differs from the unmasked prediction on the same stacks
    plain = pc.predict_change(before, after, m, **kw)
    assert not np.array_equal(plain[0], warm[0]) and not np.array_equal(plain[1], warm[1], equal_nan=True)
    # at most one host synchronisation
    count = {'n': 0}
    real_sync, real_stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

    def counted_sync(*a, **k):
        count['n'] += 1
        return real_sync(*a, **k)

    def counted_stream_sync(self):
        count['n'] += 1
        return real_stream_sync(self)
    monkeypatch.setattr(torch.cuda, 'synchronize', counted_sync)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', counted_stream_sync)
    mask = ee.mask(before, Q.BANDS9, times=bt)
    ee.sentinelCloudScore(before, Q.BANDS9, times=bt), ee.waterScore(before, Q.BANDS9, times=bt)
    pc.median_composite(before, times=bt, clear=mask, bands=sel, band_names=Q.BANDS9)
    assert count['n'] == 0, count
    got = pc.predict_change(before, after, m, quality='toa', **kw)
    assert count['n'] <= 1, count
    for g, w in zip(got, warm):
        assert np.array_equal(g, w, equal_nan=True)
