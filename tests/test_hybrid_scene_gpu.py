"""Scene prediction for the two-resolution models on the GPU.

1. satcv_dense_scene_fwd against two yardsticks: bit-equal to satcv_dense_small_fwd + satcv_scene_scatter into an identically prefilled
   map, and within the op-level float32 bound of tests/lstm_kernels_oracle.py's float64 restatement, cropped and placed in NumPy.
   3 chips of 12 x 10, crop 6 x 4 at (3, 2), launched as chips [1, 4) of a 5-entry origin table; the last window overhangs the map's
   bottom-right corner.  Sources with 16-byte rows (the wide loads) and without (one load per channel), and the 64 + 16 channel bf16
   pair of the hierarchical fusion.
2. Every refusal names the entry point and leaves the maps untouched.
3. predict_hybrid_scene against the host loop of tests/hybrid_scene_cases.py (np.array_equal): hybrid model in bf16 and float32, both
   covers, one channel and all, the class map, resident inputs, the three heads of the hierarchical model.
4. HybridInferPlan: unfused == eager; fused == a host loop over the same plan; replay; refresh after set_weights_dict; refusals.
5. The errors of predict_hybrid_scene that need a model."""
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
import hybrid_scene_cases as HC  # noqa: E402
import lstm_kernels_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {'f32': torch.float32, 'bf16': torch.bfloat16}
CODE = {'f32': 0, 'bf16': 1}


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, lstm_tools as lt, lstm_infer as li, _lib
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return dict(ops=ops, mt=mt, pt=pt, lt=lt, li=li, L=_lib, st=ops.stream_ptr())


def f32dev(x):
    return torch.tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous()


def bits(t):
    t = t.detach().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()]).cpu().numpy()


# ------------------------------------------------------------------------------------------------ 1. the kernel
NCHIP, CH, CW = 3, 12, 10
CROP = (3, 2, 6, 4)                                          # crop_y, crop_x, crop_h, crop_w
MAP_H, MAP_W = 20, 17
ORIGINS = [(5, 5), (1, 2), (9, 3), (16, 14), (0, 9)]         # chips [1, 4) are launched; (16, 14) + (6, 4) overhangs the 20 x 17 map
FIRST = 1
PREFILL, CLS_PREFILL = 7.25, 200
RESIZED_FROM = (5, 4)                                        # grid of the resized sources: 5 x 4 -> 12 x 10, no integer ratio


def kernel_cases():
    """the forward cases of tests/lstm_kernels_oracle.py (one and two sources, one resized, bf16 and f32, pending BatchNorm + ReLU, cout
    1, 3 and 16, every activation; all with 16-byte pixel rows) plus rows that are NOT 16-byte multiples (one load per channel) and the
    hierarchical fusion's 64-channel bf16 source next to a 16-channel one"""
    cases = list(O.dense_cases())
    cases.append(('narrow-softmax', 3, 0, 0.0, [(5, 7, 'bf16', True, True, True), (6, 7, 'f32', False, False, False)]))
    cases.append(('narrow-relu', 16, 3, 2.0, [(13, 13, 'f32', True, False, False)]))
    cases.append(('hier-fuse', 3, 0, 0.0, [(64, 64, 'bf16', True, True, True), (16, 16, 'bf16', True, True, False)]))
    cases.append(('wide-tail', 4, 0, 0.0, [(11, 16, 'bf16', True, True, False), (6, 8, 'f32', True, True, True)]))
    return cases


def dense_desc(env, case, seed):
    """-> (DenseDesc without outputs, keep-alive list, oracle inputs).  Sources go to the device with NaN in the channels [cin, ld)"""
    name, cout, act, mx, specs = case
    srcs, meta, w, b = O.dense_inputs(case, RESIZED_FROM + (CH, CW), NCHIP, seed)
    d, keep = env['L'].DenseDesc(), []
    d.nsrc = len(srcs)
    for i, (s, (kind, ld)) in enumerate(zip(srcs, meta)):
        cin = s.x.shape[-1]
        buf = np.full((s.x.size // cin, ld), np.nan)
        buf[:, :cin] = s.x.reshape(-1, cin)
        xd = torch.tensor(buf, dtype=torch.float32).to(TD[kind]).cuda().contiguous()
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
    d.h, d.w_, d.npix = CH, CW, NCHIP * CH * CW
    return d, keep, (srcs, w, b)


def scene_desc(env, d, org, fmap, cmap, c0, nc, ldm):
    L = env['L']
    return L.DenseSceneDesc(head=d, crop_y=CROP[0], crop_x=CROP[1], crop_h=CROP[2], crop_w=CROP[3], origins=org.data_ptr(), total=len(ORIGINS),
                            first=FIRST, map=fmap.data_ptr(), map_h=MAP_H, map_w=MAP_W, ldm=ldm, c0=c0, nc=nc,
                            class_map=cmap.data_ptr() if cmap is not None else None)


def maps(ldm):
    return (torch.full((MAP_H, MAP_W, ldm), PREFILL, dtype=torch.float32, device='cuda'),
            torch.full((MAP_H, MAP_W), CLS_PREFILL, dtype=torch.uint8, device='cuda'))


def pair_of_launches(env, d, org, c0, nc, ldm, want_cls):
    """yardstick (a): satcv_dense_small_fwd into a chip tensor, then satcv_scene_scatter of the crop (and of the classes)"""
    L = env['L']
    out = torch.empty(NCHIP, CH, CW, d.cout, dtype=torch.float32, device='cuda')
    cls = torch.empty(NCHIP, CH, CW, dtype=torch.int32, device='cuda')
    d.out, d.classes = out.data_ptr(), cls.data_ptr() if want_cls else None
    L.check(L.lib.satcv_dense_small_fwd(C.byref(d), env['st']))
    d.out, d.classes = None, None
    fmap, cmap = maps(ldm)
    common = dict(n=NCHIP, sh=CH, sw=CW, crop_y=CROP[0], crop_x=CROP[1], crop_h=CROP[2], crop_w=CROP[3], origins=org.data_ptr(), total=len(ORIGINS),
                  first=FIRST, h=MAP_H, w_=MAP_W, accumulate=0)
    s = L.SceneScatterDesc(src=out.data_ptr(), src_kind=2, lds=d.cout, c0=c0, nc=nc, dst=fmap.data_ptr(), dst_kind=2, ldd=ldm, doff=0, **common)
    L.check(L.lib.satcv_scene_scatter(C.byref(s), env['st']))
    if want_cls:
        s = L.SceneScatterDesc(src=cls.data_ptr(), src_kind=5, lds=1, c0=0, nc=1, dst=cmap.data_ptr(), dst_kind=0, ldd=1, doff=0, **common)
        L.check(L.lib.satcv_scene_scatter(C.byref(s), env['st']))
    return fmap, cmap


def placed(values, fill, dtype):
    """NumPy placement: values (NCHIP, CH, CW[, k]) cropped and put at ORIGINS[FIRST:], clipped to the map -> (map, written mask)"""
    cy, cx, ch, cw = CROP
    tail = values.shape[3:]
    out = np.full((MAP_H, MAP_W) + tail, fill, dtype)
    mask = np.zeros((MAP_H, MAP_W), bool)
    for k in range(NCHIP):
        y, x = ORIGINS[FIRST + k]
        hh, ww = min(ch, MAP_H - y), min(cw, MAP_W - x)
        out[y:y + hh, x:x + ww] = values[k, cy:cy + hh, cx:cx + ww]
        assert not mask[y:y + hh, x:x + ww].any()             # the contract: disjoint windows
        mask[y:y + hh, x:x + ww] = True
    return out, mask


@pytest.mark.parametrize('case', kernel_cases(), ids=lambda c: c[0])
def test_dense_scene_fwd_against_both_yardsticks(env, case):
    L = env['L']
    name, cout, act, mx, specs = case
    d, keep, (srcs, w, b) = dense_desc(env, case, seed=300 + len(name) + cout)
    org = torch.tensor(np.asarray(ORIGINS, np.int32)).cuda()
    want_cls = act == 0
    ldm = cout + 1                                           # a map pixel wider than the channels written
    fmap, cmap = maps(ldm)
    sd = scene_desc(env, d, org, fmap, cmap if want_cls else None, 0, cout, ldm)
    L.check(L.lib.satcv_dense_scene_fwd(C.byref(sd), env['st']))
    torch.cuda.synchronize()
    got, got_cls = fmap.cpu().numpy(), cmap.cpu().numpy()
    # (a) bit-equal to the pair of launches it replaces
    ref_map, ref_cls = pair_of_launches(env, d, org, 0, cout, ldm, want_cls)
    torch.cuda.synchronize()
    assert np.array_equal(bits(fmap), bits(ref_map)), 'differs from dense_small_fwd + scene_scatter'
    assert np.array_equal(got_cls, ref_cls.cpu().numpy())
    # (b) the float64 restatement, cropped and placed
    z, out_ref, cls_ref, margin = O.dense_fwd(srcs, w, b, act, mx, CH, CW, 'tf32')
    want, mask = placed(out_ref.reshape(NCHIP, CH, CW, cout), np.nan, np.float64)
    assert mask.sum() == 2 * 24 + 4 * 3                       # two whole windows and the clipped corner
    assert not np.isnan(got).any(), 'NaN: a read outside a source slice'
    err, scale = O.close_err(got[mask][:, :cout], want[mask])
    print(f'[fig] dense_scene_fwd {name} cout={cout}: {err:.3e} (bound {O.close_tol("f32"):.1e})')
    assert err < O.close_tol('f32')
    if want_cls:
        wcls, _ = placed(cls_ref.reshape(NCHIP, CH, CW), CLS_PREFILL, np.int64)
        sure, _ = placed((margin > O.close_tol('f32')).reshape(NCHIP, CH, CW), False, bool)
        assert sure[mask].mean() > 0.9 and np.array_equal(got_cls[sure], wcls[sure])
    # (c) everything outside the placed windows -- and the spare channel -- keeps its prefill bits
    pre = np.float32(PREFILL).view(np.int32)
    assert (bits(fmap)[~mask] == pre).all() and (bits(fmap)[..., cout:] == pre).all()
    assert (got_cls[~mask] == CLS_PREFILL).all() and (want_cls or (got_cls == CLS_PREFILL).all())
    # (d) c0 = 1, nc = 1: only that channel, at map channel 0
    if cout >= 3:
        fmap1, _ = maps(2)
        sd = scene_desc(env, d, org, fmap1, None, 1, 1, 2)
        L.check(L.lib.satcv_dense_scene_fwd(C.byref(sd), env['st']))
        torch.cuda.synchronize()
        b1 = bits(fmap1)
        assert np.array_equal(b1[..., 0][mask], bits(fmap)[..., 1][mask]) and (b1[..., 0][~mask] == pre).all() and (b1[..., 1] == pre).all()
        ref1, _ = pair_of_launches(env, d, org, 1, 1, 2, False)
        assert np.array_equal(b1, bits(ref1))


def test_dense_scene_fwd_argmax_of_equal_logits_is_the_first(env):
    L = env['L']
    case = ('ties', 4, 0, 0.0, [(8, 8, 'f32', False, False, False)])
    d, keep, _ = dense_desc(env, case, seed=1)
    wd, bd = f32dev(np.zeros((8, 4))), f32dev([0.0, 1.0, 1.0, -1.0])
    d.w, d.b = wd.data_ptr(), bd.data_ptr()
    org = torch.tensor(np.asarray(ORIGINS, np.int32)).cuda()
    fmap, cmap = maps(4)
    L.check(L.lib.satcv_dense_scene_fwd(C.byref(scene_desc(env, d, org, fmap, cmap, 0, 4, 4)), env['st']))
    _, mask = placed(np.zeros((NCHIP, CH, CW)), 0, np.int64)
    got = cmap.cpu().numpy()
    assert (got[mask] == 1).all() and (got[~mask] == CLS_PREFILL).all()


# ------------------------------------------------------------------------------------------------ 2. refusals
def _sd(field, value):
    return lambda sd: setattr(sd, field, value)


def _head(path, value):
    def m(sd):
        obj = sd.head
        for p in path[:-1]:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        setattr(obj, path[-1], value)
    return m


SOME_PTR = 4096                                               # never dereferenced: the call is refused first
REFUSALS = {
    'NULL map': _sd('map', None),
    'NULL origins': _sd('origins', None),
    'c0 + nc > cout': _sd('c0', 2),
    'nc > ldm': _sd('ldm', 2),
    'nc 0': _sd('nc', 0),
    'crop below the chip': _sd('crop_h', CH - CROP[0] + 1),
    'crop right of the chip': _sd('crop_x', CW - CROP[3] + 1),
    'negative crop origin': _sd('crop_y', -1),
    'class_map with a ReLU head': _head(('activation',), 3),
    'first + n > total': _sd('first', len(ORIGINS) - NCHIP + 1),
    'negative first': _sd('first', -1),
    'head.out': _head(('out',), SOME_PTR),
    'head.classes': _head(('classes',), SOME_PTR),
    'head.z_out': _head(('z_out',), SOME_PTR),
    'head.dw': _head(('dw',), SOME_PTR),
    'head.src[0].dx': _head(('src', 0, 'dx'), SOME_PTR),
    'activation 4': _head(('activation',), 4),
    'NULL source': _head(('src', 1, 'x'), None),
    'ld < cin': _head(('src', 0, 'ld'), 4),
    'source dtype': _head(('src', 1, 'dtype'), 7),
    'hs without ws': _head(('src', 0, 'ws'), 0),
    'in_scale without in_shift': _head(('src', 0, 'in_shift'), None),
    'h 0': _head(('h',), 0),
    'npix not whole chips': _head(('npix',), NCHIP * CH * CW - 1),
    'nsrc 3': _head(('nsrc',), 3),
    'cout 17': _head(('cout',), 17),
}


@pytest.mark.parametrize('what', list(REFUSALS))
def test_dense_scene_fwd_refuses(env, what):
    L = env['L']
    case = ('refuse', 3, 0, 0.0, [(8, 8, 'bf16', True, True, True), (5, 8, 'f32', False, False, False)])
    d, keep, _ = dense_desc(env, case, seed=60)
    org = torch.tensor(np.asarray(ORIGINS, np.int32)).cuda()
    fmap, cmap = maps(3)
    sd = scene_desc(env, d, org, fmap, cmap, 0, 3, 3)
    before = (bits(fmap), bits(cmap))
    REFUSALS[what](sd)
    rc = L.lib.satcv_dense_scene_fwd(C.byref(sd), env['st'])
    assert rc != 0, 'the call should have been refused'
    assert 'dense_scene_fwd' in L.lib.satcv_last_error().decode(), L.lib.satcv_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(bits(fmap), before[0]) and np.array_equal(bits(cmap), before[1]), 'a refused call wrote to a map'


# ------------------------------------------------------------------------------------------------ 3. scenes against the host loop
HY = HC.HYBRID
KW = dict(kernel=HY['kernel'], buff=HY['buff'], batch_size=HY['batch'], rescale=HC.RESCALE, maxval=HC.MAXVAL)
GEO = {k: HY[k] for k in ('r', 'off', 'side', 'side_lo', 'off_lo')}


@pytest.fixture(scope='module')
def hybrid(env):
    """per storage type: the model and, per cover, the scene, the stack and the host loop's (H, W, 3) map (computed once, shared)"""
    res = {}
    for dtype in ('bfloat16', 'float32'):
        m = HC.hybrid_model(env['lt'], env['mt'], dtype)
        entry = dict(m=m)
        for cover in ('reference', 'full'):
            scene, stack = HC.hybrid_scene(cover)
            want, mask = HC.host_loop(scene, stack, lambda hi, lo: m.predict([hi, lo]), GEO, HY['kernel'], HY['buff'], cover, HY['batch'], HY['T'],
                                      rescale=HC.RESCALE)
            assert np.ptp(want[mask]) > 0 and (cover == 'reference' or mask.all())
            entry[cover] = dict(scene=scene, stack=stack, want=want, mask=mask)
        res[dtype] = entry
    return res


@pytest.mark.parametrize('cover', ['reference', 'full'])
@pytest.mark.parametrize('dtype', ['bfloat16', 'float32'])
def test_hybrid_scene_equals_the_host_loop(env, hybrid, dtype, cover):
    pt, m, c = env['pt'], hybrid[dtype]['m'], hybrid[dtype][cover]
    got = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=None, cover=cover, **KW)
    assert got.shape == c['want'].shape and got.dtype == np.float32 and np.ptp(c['want']) > 0
    assert np.array_equal(got, c['want'])
    one = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=1, cover=cover, **KW)
    assert one.shape == c['want'].shape[:2] and np.array_equal(one, c['want'][..., 1]) and np.ptp(one) > 0
    if cover == 'reference':                                  # the border the reference cover leaves out
        assert not c['mask'].all() and (got[~c['mask']] == 0).all()


@pytest.mark.parametrize('cover', ['reference', 'full'])
def test_hybrid_scene_class_map(env, hybrid, cover):
    pt, m, c = env['pt'], hybrid['bfloat16']['m'], hybrid['bfloat16'][cover]
    probs, cls = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=-1, cover=cover, classes=True, **KW)
    assert np.array_equal(probs, c['want'][..., 2])
    want = np.where(c['mask'], c['want'].argmax(-1), 255).astype(np.uint8)      # (np.argmax: the first index on ties, as the kernel)
    assert cls.dtype == np.uint8 and cls.shape == want.shape and np.array_equal(cls, want)
    if cover == 'reference':
        assert (cls[~c['mask']] == 255).all() and (~c['mask']).any()


def test_hybrid_scene_from_resident_tensors(env, hybrid):
    pt, m, c = env['pt'], hybrid['bfloat16']['m'], hybrid['bfloat16']['full']
    scene = torch.from_numpy((c['scene'].astype(np.float64) / HC.RESCALE).astype(np.float32)).cuda()
    stack = torch.from_numpy(c['stack']).cuda()
    assert stack.dtype == torch.int16 and stack.shape[0] > HY['T']
    kw = dict(KW, rescale=None)
    got = pt.predict_hybrid_scene(scene, stack, m, channel=None, cover='full', **kw)
    assert np.array_equal(got, c['want'])


@pytest.fixture(scope='module')
def hier(env):
    m = HC.hierarchical_model(env['lt'], env['mt'], 'bfloat16')
    scene, stack = HC.hier_scene()
    g = HC.HIER
    geo = {k: g[k] for k in ('r', 'off', 'side', 'side_lo', 'off_lo')}
    # one pass: the three heads of every batch side by side along the channel axis, split again afterwards
    counts = [m.sub.cout, m.acnn.cout, m.fuse.cout]
    both, mask = HC.host_loop(scene, stack, lambda hi, lo: np.concatenate(m.predict([hi, lo]), -1), geo, g['kernel'], g['buff'], 'reference', g['batch'],
                              g['T'], rescale=None)
    assert both.shape[-1] == sum(counts)
    want = dict(zip(m.output_names, np.split(both, np.cumsum(counts)[:-1], -1)))
    return dict(m=m, scene=scene, stack=stack, want=want, mask=mask)


@pytest.mark.parametrize('output', ['sub_probs', 'acnn_probs', 'lstm_probs'])
def test_hierarchical_scene_equals_the_host_loop(env, hier, output):
    pt, g, m = env['pt'], HC.HIER, hier['m']
    kw = dict(kernel=g['kernel'], buff=g['buff'], batch_size=g['batch'], maxval=HC.MAXVAL)
    want = hier['want'][output]
    got = pt.predict_hybrid_scene(hier['scene'], hier['stack'], m, channel=None, output=output, **kw)
    assert got.shape == want.shape and np.ptp(want) > 0 and np.array_equal(got, want)
    assert (got[~hier['mask']] == 0).all() and (~hier['mask']).any()
    if output == 'lstm_probs':                                # the default head, with its class map
        probs, cls = pt.predict_hybrid_scene(hier['scene'], hier['stack'], m, channel=0, classes=True, **kw)
        assert np.array_equal(probs, want[..., 0])
        assert np.array_equal(cls, np.where(hier['mask'], want.argmax(-1), 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ 4. the plan
@pytest.mark.parametrize('cover', ['reference', 'full'])
def test_scene_with_an_unfused_plan_equals_the_eager_path(env, hybrid, cover):
    pt, m, c = env['pt'], hybrid['bfloat16']['m'], hybrid['bfloat16'][cover]
    got = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=None, cover=cover, plan=True, **KW)
    assert np.array_equal(got, c['want'])                     # (the eager path equals the host loop: the test above)
    plan = m.scene_plan(HY['batch'], HY['side'], HY['side_lo'])
    assert plan.fused_layers == ()
    got, cls = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=None, cover=cover, classes=True, plan=plan, **KW)
    assert np.array_equal(got, c['want']) and np.array_equal(cls, np.where(c['mask'], c['want'].argmax(-1), 255).astype(np.uint8))


def _plan_host_loop(env, plan, m, c, cover):
    """the host loop with the SAME plan in place of m.predict (a short last batch as a prefix)"""
    lt = env['lt']

    def predict(hi, lo):
        xt, _ = lt._ingest_seq(torch.from_numpy(lo).cuda(), 16, m.dtype_code)
        return plan.run(torch.from_numpy(hi).cuda(), xt).cpu().numpy()
    return HC.host_loop(c['scene'], c['stack'], predict, GEO, HY['kernel'], HY['buff'], cover, HY['batch'], HY['T'], rescale=HC.RESCALE)[0]


@pytest.mark.parametrize('cover', ['reference', 'full'])
def test_scene_with_a_fused_plan_equals_a_host_loop_over_the_same_plan(env, hybrid, cover):
    pt, m, c = env['pt'], hybrid['bfloat16']['m'], hybrid['bfloat16'][cover]
    plan = m.scene_plan(HY['batch'], HY['side'], HY['side_lo'], fused=True)
    assert plan.fused_layers == ('conv_lstm', 'dilated_conv_lstm')
    want = _plan_host_loop(env, plan, m, c, cover)
    got = pt.predict_hybrid_scene(c['scene'], c['stack'], m, channel=None, cover=cover, plan=plan, **KW)
    assert np.ptp(want) > 0 and np.array_equal(got, want)


def test_plan_replays_by_the_third_batch_and_follows_the_weights(env, hybrid, monkeypatch):
    pt, lt, c = env['pt'], env['lt'], hybrid['bfloat16']['full']
    monkeypatch.setenv('SATCV_LSTM_GRAPH', '1')
    m = HC.hybrid_model(env['lt'], env['mt'], 'bfloat16')   # (a model of its own: its weights change below)
    plan = m.scene_plan(HY['batch'], HY['side'], HY['side_lo'], fused=True)
    xu = torch.zeros(HY['batch'], HY['side'], HY['side'], HY['C'], device='cuda')
    xt = torch.zeros(HY['T'] * HY['batch'], HY['side_lo'], HY['side_lo'], 16, dtype=torch.bfloat16, device='cuda')
    plan.run(xu, xt)
    assert not plan.replaying
    plan.run(xu, xt)
    assert plan.replaying                                     # captured by the second batch, so the third replays
    kw = dict(channel=None, cover='full', **KW)
    first = pt.predict_hybrid_scene(c['scene'], c['stack'], m, plan=plan, **kw)
    HC.randomise(m, 99, scale=2.0)                            # set_weights_dict with changed weights
    fresh = pt.predict_hybrid_scene(c['scene'], c['stack'], m, plan=m.scene_plan(HY['batch'], HY['side'], HY['side_lo'], fused=True), **kw)
    got = pt.predict_hybrid_scene(c['scene'], c['stack'], m, plan=plan, **kw)
    assert plan.replaying and np.array_equal(got, fresh) and not np.array_equal(got, first)


def test_plan_refusals(env, hybrid, hier):
    pt, m, c = env['pt'], hybrid['bfloat16']['m'], hybrid['bfloat16']['reference']
    other = hybrid['float32']['m']
    with pytest.raises(ValueError, match='HybridInferPlan'):  # a plan of another model
        pt.predict_hybrid_scene(c['scene'], c['stack'], m, cover='reference', plan=other.scene_plan(HY['batch'], HY['side'], HY['side_lo']), **KW)
    with pytest.raises(ValueError, match='HybridInferPlan'):  # a plan of another shape
        pt.predict_hybrid_scene(c['scene'], c['stack'], m, cover='reference', plan=m.scene_plan(HY['batch'] + 1, HY['side'], HY['side_lo']), **KW)
    g = HC.HIER
    with pytest.raises(NotImplementedError):
        pt.predict_hybrid_scene(hier['scene'], hier['stack'], hier['m'], kernel=g['kernel'], buff=g['buff'], batch_size=g['batch'], plan=True)
    with pytest.raises(NotImplementedError):
        env['li'].HybridInferPlan(hier['m'], 4, 16, 8)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_that_need_a_model(env, hybrid):
    pt, lt, m, c = env['pt'], env['lt'], hybrid['bfloat16']['m'], hybrid['bfloat16']['reference']
    scene, stack = c['scene'], c['stack']
    kw = dict(KW, cover='reference')
    with pytest.raises(ValueError, match='HybridModel'):
        pt.predict_hybrid_scene(scene, stack, lt.get_lstm_model(6, 3, 3), **kw)
    with pytest.raises(ValueError, match='fine bands'):
        pt.predict_hybrid_scene(scene[..., :3], stack, m, **kw)
    with pytest.raises(ValueError, match='coarse bands'):
        pt.predict_hybrid_scene(scene, stack[:, :5], m, **kw)
    with pytest.raises(ValueError, match='acquisitions'):
        pt.predict_hybrid_scene(scene, stack[:2], m, **kw)
    with pytest.raises(ValueError, match='ratio'):
        pt.predict_hybrid_scene(scene, stack[..., :19], m, **kw)
    with pytest.raises(ValueError, match='kernel'):
        pt.predict_hybrid_scene(scene, stack, m, **dict(kw, kernel=20))
    with pytest.raises(ValueError, match='side'):              # r = 2, side = 4 + 2 * 2 = 8: no multiple of the pooling product 6
        pt.predict_hybrid_scene(np.zeros((120, 120, 4), np.float32), np.zeros((3, 6, 60, 60), np.float32), m, kernel=4, buff=4, batch_size=4)
    with pytest.raises(ValueError, match='output'):
        pt.predict_hybrid_scene(scene, stack, m, output='lstm_probs', **kw)
    with pytest.raises(IndexError):
        pt.predict_hybrid_scene(scene, stack, m, **dict(kw, channel=3))
    with pytest.raises(ValueError, match='maxval'):
        pt.predict_hybrid_scene(scene, stack, m, **dict(kw, maxval=0))
    act = m.fusion.activation
    try:                                                      # a head without a class output
        m.fusion.activation = m.fusion.ACT['relu']
        with pytest.raises(ValueError, match='classes=True'):
            pt.predict_hybrid_scene(scene, stack, m, classes=True, **kw)
    finally:
        m.fusion.activation = act
    # a scene too small for one reference chip: the prefilled maps
    probs, cls = pt.predict_hybrid_scene(scene[:48, :48], stack[:, :, :8, :8], m, classes=True, **kw)
    assert probs.shape == (48, 48) and not probs.any() and cls.dtype == np.uint8 and (cls == 255).all()
    # predict_on_device: the inputs as the gathers leave them
    with pytest.raises(ValueError, match='float32 CUDA'):
        m.predict_on_device([torch.zeros(1, 48, 48, 5, device='cuda'), torch.zeros(3, 8, 8, 16, dtype=torch.bfloat16, device='cuda')], shape=(1, 3, 8, 8))
    with pytest.raises(ValueError, match='float32 CUDA'):
        m.predict_on_device([np.zeros((1, 48, 48, 4), np.float32), torch.zeros(3, 8, 8, 16, device='cuda')], shape=(1, 3, 8, 8))
    with pytest.raises(ValueError, match='numbers of chips'):
        m.predict_on_device([torch.zeros(2, 48, 48, 4, device='cuda'), torch.zeros(3, 8, 8, 16, dtype=torch.bfloat16, device='cuda')], shape=(1, 3, 8, 8))


def test_predict_on_device_equals_predict(env, hybrid, hier):
    """the model entry points alone: the whole chip tensor, bit-equal to predict on the same host values"""
    lt = env['lt']
    m, c = hybrid['bfloat16']['m'], hybrid['bfloat16']['reference']
    hi, lo = HC.cut_chips(c['scene'], c['stack'], HC.origins(c['scene'].shape[:2], HY['kernel'], HY['buff'], 'reference')[:3], GEO, HY['T'], HC.RESCALE, HC.MAXVAL)
    want = m.predict([hi, lo])
    xt, shape = lt._ingest_seq(torch.from_numpy(lo).cuda(), 16, m.dtype_code)
    probs, cls = m.predict_on_device([torch.from_numpy(hi).cuda(), xt], shape=shape, want_classes=True)
    assert np.array_equal(probs.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), want.argmax(-1))
    assert np.array_equal(m.predict_on_device([torch.from_numpy(hi).cuda(), torch.from_numpy(lo).cuda()]).cpu().numpy(), want)
    g, hm = HC.HIER, hier['m']
    geo = {k: g[k] for k in ('r', 'off', 'side', 'side_lo', 'off_lo')}
    hi, lo = HC.cut_chips(hier['scene'], hier['stack'], HC.origins(hier['scene'].shape[:2], g['kernel'], g['buff'], 'reference')[:3], geo, g['T'], None, HC.MAXVAL)
    want = hm.predict([hi, lo])
    xt, shape = lt._ingest_seq(torch.from_numpy(lo).cuda(), 16, hm.dtype_code)
    for i, name in enumerate(hm.output_names):
        got = hm.predict_on_device([torch.from_numpy(hi).cuda(), xt], shape=shape, output=name)
        assert np.array_equal(got.cpu().numpy(), want[i]) and np.ptp(want[i]) > 0
