"""Folded bf16 / fp8 inference of the Siamese change-detection U-Net (make_siamese_unet, utils/model_tools.py:576-663) and two-date
chip prediction.  The pair store of the conv epilogue (satcv_conv_desc pair_n: the two dates of a shared layer as one launch whose
store remaps into concat([x_b, x_a])) is checked bit-exactly against two plain launches into the same channel slices; the plans
against the float64 PyTorch restatement (oracle/torch_unet.siamese_forward)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

FILTERS, FACTORS = [32, 64], [2, 2]


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, fp8_infer
    from satellite_computervision_amd._lib import lib, check, FP8, FP8X, BF16
    return dict(ops=ops, mt=mt, fi=fp8_infer, lib=lib, check=check, FP8=FP8, FP8X=FP8X, BF16=BF16)


@pytest.fixture
def no_thin_roles(env):
    """the staging / matrix wave-role kernel has no pair store: compare the weights-stationary kernel's paired and plain launches"""
    lib, check = env['lib'], env['check']
    old = C.c_int(0)
    check(lib.satcv_get_option(b'thin_roles', C.byref(old)))
    check(lib.satcv_set_option(b'thin_roles', 0))
    yield
    check(lib.satcv_set_option(b'thin_roles', old.value))


# (storage, n per date, h, w, cin, cout, k, dil, fused pool)
PAIR_CASES = [
    ('bf16', 2, 64, 64, 32, 32, 3, 1, False), ('bf16', 2, 64, 64, 32, 32, 3, 1, True), ('bf16', 2, 64, 64, 16, 32, 3, 1, True),
    ('fp8', 2, 64, 64, 32, 32, 3, 1, False), ('fp8', 2, 64, 64, 32, 32, 3, 1, True),
    ('bf16', 3, 16, 16, 128, 256, 3, 1, False), ('bf16', 3, 8, 8, 128, 256, 3, 1, True), ('fp8', 3, 16, 16, 128, 256, 3, 1, False),
    ('fp8', 3, 8, 8, 128, 256, 3, 1, False), ('fp8x', 3, 16, 16, 128, 256, 3, 1, False), ('fp8x', 3, 8, 8, 128, 256, 3, 1, True),
    ('bf16', 3, 8, 8, 512, 256, 1, 1, False), ('fp8', 3, 8, 8, 512, 256, 1, 1, False), ('fp8x', 3, 8, 8, 512, 256, 1, 1, False),
    ('bf16', 2, 16, 16, 128, 128, 3, 3, False), ('bf16', 2, 16, 16, 128, 128, 3, 6, False),
    ('fp8', 2, 16, 16, 128, 128, 3, 3, False), ('fp8', 2, 16, 16, 128, 128, 3, 6, False),
]


@pytest.mark.parametrize('case', PAIR_CASES)
def test_pair_store_matches_two_plain_launches(env, no_thin_roles, case):
    """one launch of 2n images with the pair store == one launch per date at n images storing into the same channel slices, bit for bit;
    channels outside the two slices keep their sentinel.  The fused max-pool is not remapped (2n pooled images)."""
    ops, lib, check = env['ops'], env['lib'], env['check']
    store, pn, h, w, cin, cout, k, dil, pool = case
    dt = {'bf16': env['BF16'], 'fp8': env['FP8'], 'fp8x': env['FP8X']}[store]
    tdt = torch.bfloat16 if store == 'bf16' else torch.float8_e4m3fn
    esz = 2 if store == 'bf16' else 1
    rng = np.random.default_rng(hash(case) % 2 ** 31)
    n = 2 * pn
    x = torch.tensor(rng.integers(-3, 4, (n, h, w, cin)), dtype=torch.float32).to(tdt).cuda()
    kern = torch.tensor(rng.integers(-2, 3, (k, k, cin, cout)), dtype=torch.float32)
    wp, _ = ops.pack_weights(kern.cuda(), cin, dt, want_dgrad=False)
    osc = torch.tensor(2.0 ** rng.integers(-7, -4, cout), dtype=torch.float32).cuda()
    bias = torch.tensor(rng.integers(-4, 5, cout), dtype=torch.float32).cuda()
    ldy = 2 * cout + 32                                  # the two date slices and a spare slice at the end
    sentinel = 0x3c if store == 'bf16' else 0x21

    def alloc(*shape):
        return torch.full(shape, sentinel, dtype=torch.uint8, device='cuda')
    y_pair, y_two = alloc(pn, h, w, ldy * esz), alloc(pn, h, w, ldy * esz)
    f = 2 if pool else 0
    p_pair = alloc(n, h // 2, w // 2, cout * esz) if pool else None
    p_two = alloc(n, h // 2, w // 2, cout * esz) if pool else None
    base = dict(c0=cin, w=wp.data_ptr(), bias=bias.data_ptr(), out_scale=osc.data_ptr(), h=h, w_=w, cout=cout, cout_pad=ops.rup(cout, 32),
                kh=k, kw=k, dil=dil, dtype=dt, out_relu=1)
    offs = (cout, 0)                                     # concat([x_b, x_a]): date a behind date b
    pk = dict(pool_y=p_pair.data_ptr(), pool_ld=cout, pool_f=f) if pool else {}
    d = ops.make_conv_desc(x0=x.data_ptr(), n=n, y=y_pair.data_ptr(), ldy=ldy, pair=(pn, offs[0], offs[1]), **base, **pk)
    assert lib.satcv_conv2d_igemm_pipelined(C.byref(d)) == 1
    check(lib.satcv_conv2d_igemm(C.byref(d), ops.stream_ptr()))
    xb = x.view(torch.uint8) if x.dtype != torch.bfloat16 else x
    for dd in (0, 1):
        pk = dict(pool_y=p_two.data_ptr() + dd * pn * (h // 2) * (w // 2) * cout * esz, pool_ld=cout, pool_f=f) if pool else {}
        d1 = ops.make_conv_desc(x0=xb[dd * pn:].data_ptr(), n=pn, y=y_two.data_ptr() + offs[dd] * esz, ldy=ldy, **base, **pk)
        check(lib.satcv_conv2d_igemm(C.byref(d1), ops.stream_ptr()))
    torch.cuda.synchronize()
    # exactly representable data: the stored values are the float64 result rounded once to the storage type, whichever kernel ran
    xf = x.float().cpu().double().permute(0, 3, 1, 2)
    acc = torch.nn.functional.conv2d(xf, kern.permute(3, 2, 0, 1).double(), padding=dil * (k - 1) // 2, dilation=dil).permute(0, 2, 3, 1)
    ref = (acc * osc.cpu().double() + bias.cpu().double()).clamp_min(0)
    ref = (ref.clamp_max(448) if store != 'bf16' else ref).float().to(tdt).view(torch.uint8).reshape(n, h, w, cout * esz)
    yv = y_pair.cpu().reshape(pn, h, w, ldy * esz)
    assert torch.equal(yv[..., offs[0] * esz:(offs[0] + cout) * esz], ref[:pn]), 'date a'
    assert torch.equal(yv[..., offs[1] * esz:(offs[1] + cout) * esz], ref[pn:]), 'date b'
    assert torch.equal(y_pair, y_two)
    assert bool((y_pair[..., 2 * cout * esz:] == sentinel).all()), 'channels outside the two slices were written'
    assert not bool((y_pair[..., :2 * cout * esz] == sentinel).all())
    if pool:
        assert torch.equal(p_pair, p_two)


def test_pair_store_refused_where_only_a_non_pairing_kernel_could_run(env):
    """a pair-store descriptor that no pipelined kernel takes (a y that breaks the 16-byte store alignment) is an error, not a plain store"""
    ops, lib, check, BF16 = env['ops'], env['lib'], env['check'], env['BF16']
    pn, h, w, cin, cout = 2, 32, 32, 32, 32
    x = torch.ones(2 * pn, h, w, cin, dtype=torch.bfloat16, device='cuda')
    wp, _ = ops.pack_weights(torch.ones(3, 3, cin, cout, device='cuda'), cin, BF16, want_dgrad=False)
    y = torch.zeros(pn * h * w * 2 * cout + 8, dtype=torch.bfloat16, device='cuda')
    d = ops.make_conv_desc(x0=x.data_ptr(), c0=cin, w=wp.data_ptr(), y=y.data_ptr() + 2, ldy=2 * cout, n=2 * pn, h=h, w_=w, cout=cout, cout_pad=cout,
                           dtype=BF16, pair=(pn, cout, 0))
    assert lib.satcv_conv2d_igemm_pipelined(C.byref(d)) == 0
    assert lib.satcv_conv2d_igemm(C.byref(d), ops.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert not bool(y.any())
    bad = ops.make_conv_desc(x0=x.data_ptr(), c0=cin, w=wp.data_ptr(), y=y.data_ptr(), ldy=2 * cout, n=2 * pn + 1, h=h, w_=w, cout=cout, cout_pad=cout,
                             dtype=BF16, pair=(pn, cout, 0))
    assert lib.satcv_conv2d_igemm(C.byref(bad), ops.stream_ptr()) != 0
    bad = ops.make_conv_desc(x0=x.data_ptr(), c0=cin, w=wp.data_ptr(), y=y.data_ptr(), ldy=2 * cout, n=2 * pn, h=h, w_=w, cout=cout, cout_pad=cout,
                             dtype=BF16, pair=(pn, cout + 8, 0))
    assert lib.satcv_conv2d_igemm(C.byref(bad), ops.stream_ptr()) != 0


def _siamese(mt, seed=4, thresh=0.4, dtype='bfloat16'):
    """a [32, 64] Siamese U-Net with non-trivial weights and BatchNorm statistics, and the float64 oracle of its current parameters"""
    from oracle import torch_unet as TU
    mt.reset_uids(); mt.set_seed(seed)
    m = mt.make_siamese_unet(4, FILTERS, FACTORS, class_thresh=thresh)
    m.compute_dtype = dtype
    conv_of = {'enc0': 'conv2d', 'enc1': 'conv2d_2', 'aspp.cba': 'conv2d_4', 'aspp.cba3': 'conv2d_6', 'aspp.cba3_3': 'conv2d_7', 'aspp.cba3_6': 'conv2d_8',
               'aspp.cba3_12': 'conv2d_9', 'dec1.conv1': 'conv2d_10', 'dec1.conv2': 'conv2d_11', 'dec0.conv1': 'conv2d_12', 'dec0.conv2': 'conv2d_13'}
    ref_of = {'probs/kernel': 'probs.kernel', 'probs/bias': 'probs.bias', 'conv2d_transpose/kernel': 'dec1.up.kernel', 'conv2d_transpose/bias': 'dec1.up.bias',
              'conv2d_transpose_1/kernel': 'dec0.up.kernel', 'conv2d_transpose_1/bias': 'dec0.up.bias'}
    for rn, cn in conv_of.items():
        ref_of[cn + '/kernel'] = rn + '.kernel'; ref_of[cn + '/bias'] = rn + '.bias'
        idx = cn.split('_')[1] if '_' in cn else '0'
        idx = {'10': '11', '11': '12', '12': '14', '13': '15'}.get(idx, idx)
        bn = 'batch_normalization' if idx == '0' else f'batch_normalization_{idx}'
        for s_ in ('gamma', 'beta', 'moving_mean', 'moving_var'):
            ref_of[f'{bn}/{s_}'] = f'{rn}.bn.{s_}'
    for bn, rn in (('batch_normalization_10', 'dec1.bn0'), ('batch_normalization_13', 'dec0.bn0')):
        for s_ in ('gamma', 'beta', 'moving_mean', 'moving_var'):
            ref_of[f'{bn}/{s_}'] = f'{rn}.{s_}'
    assert set(ref_of) == {ps.name for ps in m.param_specs}
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

    def oracle(xa, xb):
        tp = TU.params_to_torch({ref_of[k]: v for k, v in m.get_weights_dict().items()}, torch.float64, requires_grad=False)
        with torch.no_grad():
            return TU.siamese_forward(tp, torch.tensor(xa, dtype=torch.float64), torch.tensor(xb, dtype=torch.float64), FILTERS, FACTORS).numpy()
    return m, oracle


def _run(env, m, plan, xa, xb):
    m._stage_x(plan, [xa, xb])
    plan.run_forward(env['ops'].stream_ptr())
    torch.cuda.synchronize()
    return [plan.outputs[t.id].cpu().numpy() for t in m.outputs]


@pytest.mark.parametrize('store', ['bf16', 'fp8'])
def test_paired_plan_equals_unpaired_plan(env, store):
    """Fp8Plan(pair=True): shared encoder levels and the ASPP squeeze as one 2n launch with the pair store; pair=False: one launch per
    date into the same slices -- identical probabilities and classes"""
    mt, fi = env['mt'], env['fi']
    m, _ = _siamese(mt)
    rng = np.random.default_rng(2)
    xa, xb = rng.random((3, 64, 64, 4)).astype(np.float32), rng.random((3, 64, 64, 4)).astype(np.float32)
    q = fi.calibrate(m, [xa, xb]) if store == 'fp8' else None
    sdt = env['FP8'] if store == 'fp8' else env['BF16']
    out_p = _run(env, m, fi.Fp8Plan(m, 3, 64, 64, q, store=sdt, pair=True), xa, xb)
    out_u = _run(env, m, fi.Fp8Plan(m, 3, 64, 64, q, store=sdt, pair=False), xa, xb)
    assert out_p[0].shape == (3, 64, 64, 1) and out_p[1].shape == (3, 64, 64, 1)
    assert np.array_equal(out_p[0], out_u[0]) and np.array_equal(out_p[1], out_u[1])


def test_folded_bf16_siamese_matches_oracle(env):
    mt = env['mt']
    m, oracle = _siamese(mt)
    rng = np.random.default_rng(3)
    xa, xb = rng.random((3, 64, 96, 4)).astype(np.float32), rng.random((3, 64, 96, 4)).astype(np.float32)
    p_ref = oracle(xa, xb)
    p_reg, _ = m.predict([xa, xb])
    m.enable_folded_inference()
    p_fold, c_fold = m.predict([xa, xb])
    assert isinstance(m._infer_plan(3, 64, 96), env['fi'].Fp8Plan)
    m.disable_folded_inference()
    assert np.abs(p_fold - p_ref).max() < 0.05, (np.abs(p_fold - p_ref).max(), np.abs(p_reg - p_ref).max())
    assert np.abs(p_fold - p_ref).mean() <= 1.5 * np.abs(p_reg - p_ref).mean() + 1e-4
    ok = np.abs(p_ref - 0.4) > 0.1
    assert np.array_equal(c_fold[ok], (p_ref > 0.4).astype(np.int32)[ok])


def test_fp8_siamese_change_iou(env):
    """a Siamese U-Net trained on a synthetic change task (change where the band sum moved by more than a threshold between the dates):
    fp8 mask vs the float64 oracle's, both scored against ground truth -- the tolerances of the U-Net's fp8 test"""
    mt = env['mt']
    m, oracle = _siamese(mt, seed=5, thresh=0.5, dtype='float32')
    rng = np.random.default_rng(11)

    def make(n):
        def scene():
            lo = torch.tensor(rng.random((n, 4, 8, 8)), dtype=torch.float32)
            return torch.nn.functional.interpolate(lo, size=(64, 64), mode='bilinear', align_corners=False).permute(0, 2, 3, 1).numpy()
        xb = scene()
        xa = xb + (rng.random((n, 1, 1, 1)) < 0.5) * (scene() - xb)      # half of the pairs changed
        xa = (xa + 0.03 * rng.standard_normal(xa.shape)).astype(np.float32)
        xb = (xb + 0.03 * rng.standard_normal(xb.shape)).astype(np.float32)
        return xa, xb, (np.abs(xa.sum(-1) - xb.sum(-1)) > 0.4).astype(np.float32)[..., None]
    xa, xb, lab = make(32)
    m.compile(optimizer=mt.Adam(2e-3), loss=lambda yt, yp: mt.weighted_bce(yt, yp, 1.0))
    for _ in range(60):
        for s in range(0, 32, 8):
            m.train_on_batch([xa[s:s + 8], xb[s:s + 8]], lab[s:s + 8])
    ta, tb, labt = make(8)
    p_ref = oracle(ta, tb)
    c_ref = (p_ref > 0.5).astype(np.int32)

    def iou(a, b):
        return np.logical_and(a == 1, b == 1).sum() / max(np.logical_or(a == 1, b == 1).sum(), 1)
    iou_ref = iou(c_ref, labt)
    assert iou_ref > 0.6, iou_ref
    m.enable_fp8_inference([xa[:8], xb[:8]])
    p8, c8 = m.predict([ta, tb])
    assert isinstance(m._infer_plan(8, 64, 64), env['fi'].Fp8Plan)
    m.disable_fp8_inference()
    agree = (c8 == c_ref).mean()
    margin = np.abs(p_ref - 0.5) > 0.25
    print(f'fp8 vs oracle: pixel agreement {agree:.4f}, IoU {iou(c8, labt):.4f} vs {iou_ref:.4f}')
    assert (c8[margin] == c_ref[margin]).mean() >= 0.995
    assert agree >= 0.985 and abs(iou(c8, labt) - iou_ref) <= 5e-3, (agree, iou(c8, labt), iou_ref)


def test_siamese_default_plan_and_state(env):
    mt, fi = env['mt'], env['fi']
    m, _ = _siamese(mt)
    rng = np.random.default_rng(5)
    xa, xb = rng.random((2, 32, 32, 4)).astype(np.float32), rng.random((2, 32, 32, 4)).astype(np.float32)
    p_reg, _ = m.predict([xa, xb])
    assert not isinstance(m._infer_plan(2, 32, 32), fi.Fp8Plan)          # the default stays the regular plan
    m.enable_folded_inference()
    p1, _ = m.predict([xa, xb])
    w = m.get_weights_dict()
    w2 = {k: (v * 0.5 if k.endswith('/kernel') and k != 'probs/kernel' else v) for k, v in w.items()}
    m.set_weights_dict(w2)
    p2, _ = m.predict([xa, xb])
    m.disable_folded_inference()
    p2_reg, _ = m.predict([xa, xb])
    assert np.abs(p1 - p_reg).max() < 0.05 and np.abs(p2 - p2_reg).max() < 0.05 and np.abs(p2 - p1).max() > 0.05
    m.set_weights_dict(w)
    m.compile(optimizer=mt.Adam(1e-2), loss=lambda yt, yp: mt.weighted_bce(yt, yp, 1.0))
    m.enable_folded_inference()
    p3, _ = m.predict([xa, xb])
    m.train_on_batch([xa, xb], (rng.random((2, 32, 32, 1)) < 0.5).astype(np.float32))
    p4, _ = m.predict([xa, xb])
    m.disable_folded_inference()
    p4_reg, _ = m.predict([xa, xb])
    assert np.abs(p4 - p4_reg).max() < 0.05 and np.abs(p4 - p3).max() > 0
    xs = rng.random((1, 34, 34, 4)).astype(np.float32)
    with pytest.raises(ValueError):
        m.predict([xs, xs])
    m.enable_folded_inference()
    with pytest.raises(ValueError):
        m.predict([xs, xs])
    m.disable_folded_inference()


@pytest.mark.parametrize('folded', [False, True])
def test_two_date_predict_chips(env, folded):
    from satellite_computervision_amd import prediction_tools as pt
    mt = env['mt']
    m, _ = _siamese(mt)
    if folded:
        m.enable_folded_inference()
    rng = np.random.default_rng(9)
    a, b = rng.random((200, 232, 4)).astype(np.float32), rng.random((200, 232, 4)).astype(np.float32)
    kernel, buff = 32, 32
    idx = pt.generate_chip_indices(a, buff, kernel)
    got = pt.predict_chips((a, b), idx, np.zeros((200, 232), np.float32), m, kernel=kernel, buff=buff, batch_size=5)
    ref = np.zeros((200, 232), np.float32)
    for y, x in idx:
        ca = a[None, y - buff // 2:y + kernel + buff // 2, x - buff // 2:x + kernel + buff // 2]
        cb = b[None, y - buff // 2:y + kernel + buff // 2, x - buff // 2:x + kernel + buff // 2]
        p, _ = m.predict([ca, cb])
        ref[y:y + kernel, x:x + kernel] += p[0, buff // 2:kernel + buff // 2, buff // 2:kernel + buff // 2, 0]
    if folded:
        m.disable_folded_inference()
    assert len(idx) > 5 and np.array_equal(got, ref)
