"""The float64 restatements of tests/bn_oracle.py are right, and the conditions that the GPU file's checks rest on hold -- no GPU.

The oracle is pinned to two independent implementations: the Keras-semantics operations of oracle/keras_ops.py and float64 torch autograd
of max_pool2d(relu(batch_norm(y))) on the CPU, both at 1e-12 relative.  For every lattice case the GPU file runs the exactness
assertions pass (that is what licenses its bit-for-bit checks); for every random case the ambiguity rule excludes at most 1e-3 of the
compared outputs (a condition on the seeds, not a tolerance: a seed that exceeds it is replaced, the cap stays)."""
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
import bn_oracle as B  # noqa: E402
from oracle import keras_ops as K  # noqa: E402

REL = 1e-12
AMBIGUOUS_CAP = 1e-3


def rel_close(got, ref, what):
    err = np.abs(np.asarray(got) - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= REL, f'{what}: {err:.3e}'


def batch_case(shape, seed, ties):
    """y, gamma, beta and upstream gradients; ties: activations on a coarse grid (many equal maxima), else all distinct"""
    rng = np.random.default_rng(seed)
    y = np.round(rng.standard_normal(shape) * 2) / 2 if ties else rng.standard_normal(shape)
    c = shape[-1]
    return y, rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c), rng.standard_normal(c) * 0.3


@pytest.mark.parametrize('f', [1, 2, 3])
@pytest.mark.parametrize('shape', [(2, 8, 8, 8), (3, 7, 9, 5)])
def test_oracle_against_keras_ops(shape, f):
    eps = 1e-3
    y, gamma, beta = batch_case(shape, 1, ties=True)
    count = y.size / shape[-1]
    rng = np.random.default_rng(2)
    s1, s2 = B.act_stats(y)
    fin = B.finalize_train(s1, s2, count, gamma, beta, eps, 0.99, 1, 0, np.zeros(shape[-1]), np.ones(shape[-1]))
    bn, mean, var = K.batchnorm_train(y, gamma, beta, eps)
    rel_close(fin['mean'], mean, 'mean')
    rel_close(fin['var'], var, 'var')
    rel_close(B.pre_act(y, fin['scale'], fin['shift']), bn, 'scale * y + shift')
    mm, mv = K.bn_update_moving(np.zeros(shape[-1]), np.ones(shape[-1]), mean, var, 0.99, count, False)
    rel_close(fin['mm'], mm, 'moving mean')
    rel_close(fin['mv'], mv, 'moving variance')
    act = np.maximum(bn, 0.0)
    rel_close(B.maxpool(act, f), K.maxpool(act, f), 'maxpool')
    n, h, w, c = shape
    da, dpool = rng.standard_normal(shape), rng.standard_normal((n, h // f, w // f, c))
    # the routing and the mask on the float64 activation (bwd_g itself, which stores the activation, follows on float32 values)
    assert np.array_equal(B.unpool(dpool, B.first_argmax(act, f), f, shape), K.maxpool_bwd(act, f, dpool))
    g = (da + B.unpool(dpool, B.first_argmax(act, f), f, shape)) * (bn > 0)
    rel_close(g, K.relu_bwd(act, da + K.maxpool_bwd(act, f, dpool)), 'g')
    d1, d2 = B.bwd_sums(g, y, fin['mean'], fin['rstd'])
    dx, dgamma, dbeta = K.batchnorm_train_bwd(y, gamma, mean, var, g, eps)
    fb = B.bwd_finalize(d1, d2, count)
    rel_close(fb['dbeta'], dbeta, 'dbeta')
    rel_close(fb['dgamma'], dgamma, 'dgamma')
    rel_close(B.bwd_dy(g, y, fin['scale'], fin['mean'], fin['rstd'], fb['c1'], fb['c2']), dx, 'dy')
    # bwd_g itself (float32 storage of values that are float32: the lattice of the tie case)
    y32 = B.store(y, 'f32')
    sc, sh = np.asarray(fin['scale'], np.float32).astype(np.float64), np.asarray(fin['shift'], np.float32).astype(np.float64)
    a32 = B.act_of(y32, sc, sh, 'f32')
    ref = K.relu_bwd(B.pre_act(y32, sc, sh), da + K.maxpool_bwd(a32, f, dpool))
    assert np.array_equal(B.bwd_g(y32, sc, sh, da, dpool, f, 'f32'), ref)


@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('f', [2, 3])
def test_oracle_against_torch_autograd(f, ties):
    """ties=False: every window has one maximum, torch's routing and the first-maximum rule agree, so dy agrees.  ties=True: only what does
    not depend on the routing is compared (the forward values)."""
    shape, eps = (3, 7, 9, 6), 1e-3
    y, gamma, beta = batch_case(shape, 3, ties)
    n, h, w, c = shape
    rng = np.random.default_rng(4)
    da, dpool = rng.standard_normal(shape), rng.standard_normal((n, h // f, w // f, c))
    yt = torch.tensor(y.transpose(0, 3, 1, 2), dtype=torch.float64, requires_grad=True)
    bn = torch.nn.functional.batch_norm(yt, None, None, torch.tensor(gamma), torch.tensor(beta), training=True, eps=eps)
    act = torch.relu(bn)
    pooled = torch.nn.functional.max_pool2d(act, f)
    loss = (act * torch.tensor(da.transpose(0, 3, 1, 2))).sum() + (pooled * torch.tensor(dpool.transpose(0, 3, 1, 2))).sum()
    loss.backward()
    count = n * h * w
    s1, s2 = B.act_stats(y)
    fin = B.finalize_train(s1, s2, count, gamma, beta, eps, 0.99, 0, 0)
    a = B.pre_act(y, fin['scale'], fin['shift'])
    rel_close(np.maximum(a, 0.0), act.detach().numpy().transpose(0, 2, 3, 1), 'act')
    rel_close(B.maxpool(np.maximum(a, 0.0), f), pooled.detach().numpy().transpose(0, 2, 3, 1), 'pooled')
    if ties:
        return
    g = (da + B.unpool(dpool, B.first_argmax(np.maximum(a, 0.0), f), f, shape)) * (a > 0)
    d1, d2 = B.bwd_sums(g, y, fin['mean'], fin['rstd'])
    fb = B.bwd_finalize(d1, d2, count)
    dy = B.bwd_dy(g, y, fin['scale'], fin['mean'], fin['rstd'], fb['c1'], fb['c2'])
    rel_close(dy, yt.grad.numpy().transpose(0, 2, 3, 1), 'dy')


def test_finalize2_equals_the_raw_form_sums():
    """the activated-form sums (sum g [a > 0], sum g a) convert to sum g xhat of the masked gradient"""
    shape = (3, 7, 9, 16)
    d = B.make_inputs(shape, 1, 'f32', 'random', 'finalize2')
    y, sc, sh, mu, rs = d['y'], d['scale'], d['shift'], d['mean'], d['rstd']
    # scale y + shift = (scale / rstd) xhat + (shift + scale mean) for any scale, shift, mean, rstd: wherever the mask is 1,
    # xhat = (a - shift - scale mean) rstd / scale
    a = np.maximum(B.pre_act(y, sc, sh), 0.0)
    g = d['da'] * (a > 0)
    raw1, raw2 = B.bwd_sums(g, y, mu, rs)
    a1, a2 = B.skip_sums(d['da'], a)
    conv = B.act_to_raw_sum(a1, a2, sc, sh, mu, rs)
    assert np.abs(a1 - raw1).max() <= REL * np.abs(raw1).max()
    assert np.abs(conv - raw2).max() <= 1e-10 * np.abs(raw2).max()    # (the division by scale: |scale| down to 1e-2 here)
    fb = B.bwd_finalize2(raw1, raw2, a1, a2, 189.0, sc, sh, mu, rs)
    rel_close(fb['dbeta'], 2 * raw1, 'raw + activated rows')
    assert np.abs(fb['dgamma'] - 2 * raw2).max() <= 1e-10 * np.abs(raw2).max()
    zero = sc.copy()
    zero[3] = 0.0
    assert B.act_to_raw_sum(a1, a2, zero, sh, mu, rs)[3] == 0.0


def test_affine_infer_against_keras_ops():
    rng = np.random.default_rng(5)
    c = 13
    gamma, beta, mm, mv, bias = rng.standard_normal(c), rng.standard_normal(c), rng.standard_normal(c), rng.uniform(0.1, 2.0, c), rng.standard_normal(c)
    x = rng.standard_normal((2, 3, 3, c))
    aff = B.affine_infer(gamma, beta, mm, mv, 1e-3, bias)
    rel_close(x * aff['scale'] + aff['shift'], K.batchnorm_infer(x, gamma, beta, mm, mv, 1e-3), 'inference affine')
    rel_close(x * aff['scale'] + aff['bias_eff'], K.batchnorm_infer(x + bias, gamma, beta, mm, mv, 1e-3), 'bias_eff')


def test_ambiguous_marks_what_rounding_can_flip():
    y = np.zeros((1, 2, 2, 8))
    sc, sh = np.ones(8), np.zeros(8)
    y[0, 0, 0, 0] = 2.0 ** -30                    # a within b of zero? b = 4 * 2^-24 * |y|: no -- a == y exactly, not ambiguous
    y[0, 0, 1, 1] = 1.0 + 2.0 ** -8               # the midpoint of two bf16 values
    y[0, :, :, 2] = [[1.0, 1.0 + 2.0 ** -23], [0.0, 0.0]]        # two distinct f32 maxima closer than 2 b
    am32, am16 = B.ambiguous(y, sc, sh, 'f32', 2), B.ambiguous(y, sc, sh, 'bf16', 2)
    assert not am32['sign'].any() and not am32['rnd'].any()
    assert am16['rnd'][0, 0, 1, 1] and am16['rnd'].sum() == 1
    assert am32['tie'][0, 0, 0, 2] and am32['tie'].sum() == 1
    sh2 = np.full(8, -1.0)
    y2 = np.full((1, 1, 1, 8), 1.0 + 2.0 ** -23)  # a = 2^-23 against b = 4 * 2^-24 * 2
    assert B.ambiguous(y2, sc, sh2, 'f32', 1)['sign'].all()


# --------------------------------------------------------- the conditions of the GPU file's checks, case by case
@pytest.mark.parametrize('kind', B.KINDS)
def test_lattice_cases_are_exact(kind):
    small = 0
    for case in B.pool_cases():
        shape, f = case[0], case[1]
        d = B.make_inputs(shape, f, kind, 'lattice', B.case_id(case))
        assert B.assert_lattice_exact(d, kind, f)
        act = B.act_of(d['y'], d['scale'], d['shift'], kind)
        assert B.sum_is_exact(act) and B.sum_is_exact(act * act), B.case_id(case)
        assert abs((act == 0).mean() - 0.5) < 0.2 or act.size < 4096, 'about half of the activations are zero'
        small += 1
    for case in B.bwd_cases():
        shape, f = case['shape'], case['f']
        d = B.make_inputs(shape, f, kind, 'lattice', B.case_id(case), B.skip_channels(case))
        assert B.assert_lattice_exact(d, kind, f, case['linear'], case['dpool'])
        g = B.bwd_g(d['y'], d['scale'], d['shift'], d['da'] if case['da'] else None, d['dpool'] if case['dpool'] else None, f, kind, case['linear'])
        dy = B.store(B.bwd_dy(g, d['y'], d['scale'], d['mean'], d['rstd'], d['c1'], d['c2']), kind)
        sums = [g, g * B.xhat_of(d['y'], d['mean'], d['rstd']), dy]
        if case['sk']:
            sums.append(dy[..., :case['split']] * d['y'][..., :case['split']])
        assert all(B.sum_is_exact(s) for s in sums), B.case_id(case)
        small += 1
    assert small > 100
    # the lattice of every case holds a zero and a negative scale
    assert (d['scale'] == 0).any() and (d['scale'] < 0).any()
    # past the launch cap the element-wise outputs are still exact; the sums need not be (the GPU file then uses the random-input bound)
    case = B.cap_cases()[0]
    d = B.make_inputs((1, 1, 4099, 8), 1, kind, 'lattice', B.case_id(case))
    assert B.assert_lattice_exact(d, kind, 1)


@pytest.mark.parametrize('kind', B.KINDS)
def test_random_cases_keep_the_ambiguous_share_under_the_cap(kind):
    worst = 0.0
    for case in B.pool_cases():
        share = B.ambiguous_share(case[0], case[1], kind, B.case_id(case))
        assert share <= AMBIGUOUS_CAP, (B.case_id(case), share)
        worst = max(worst, share)
    for case in B.bwd_cases():
        share = B.ambiguous_share(case['shape'], case['f'], kind, B.case_id(case), B.skip_channels(case))
        assert share <= AMBIGUOUS_CAP, (B.case_id(case), share)
        worst = max(worst, share)
    print(f'[fig] worst ambiguous share {kind}: {worst:.3e} (cap {AMBIGUOUS_CAP:.0e})')


def test_case_tables_reach_every_form():
    """reading aid for the dispatch in satcv_bn_relu_pool*, satcv_bn_bwd_reduce and satcv_bn_bwd_apply"""
    P, W = B.pool_cases(), B.bwd_cases()
    even2 = [c for c in P if c[1] == 2 and c[0][1] % 2 == 0 and c[0][2] % 2 == 0]
    odd2 = [c for c in P if c[1] == 2 and (c[0][1] % 2 or c[0][2] % 2)]
    for group in (even2, odd2, [c for c in P if c[1] not in (1, 2)]):
        assert {c[2] for c in group} == {0, 1}                                              # with and without the arg-max bytes
    assert {c[1] for c in P} == {1, 2, 3, 4} and {c[3] for c in P} == {'yes', 'no', 'wide'} and {c[5] for c in P} == {0, 1}
    assert any(not c[4] for c in P)
    assert {c[0][3] for c in P} >= {8, 24, 40, 72, 1000, 2048}
    has = lambda **kw: any(all(c[k] == v for k, v in kw.items()) for c in W)                # noqa: E731
    assert has(f=2, dpool=1, da=1, shape=(2, 8, 8, 24)) and has(f=2, dpool=1, da=1, shape=(3, 7, 9, 40)) and has(f=3, dpool=1, da=1)
    assert has(da=0, dpool=1, f=2) and has(da=0, dpool=1, f=3) and has(linear=1, dpool=0) and has(linear=1, dpool=1)
    assert has(dbias=1, dpool=0) and has(dbias=1, dpool=1)
    for sk in (0, 1):
        for dy1 in (0, 1):
            for wide in (0, 1):
                assert has(split=16, sk=sk, dy1=dy1, wide=wide) and has(split=32, sk=sk, dy1=dy1, wide=wide)
    assert {c['shape'][3] for c in W} >= {8, 24, 40, 72, 1000, 2048}
    assert {int(np.prod(c['shape'][:3])) for c in W if not c['dpool']} >= {1, 3, 4, 5, 189}
