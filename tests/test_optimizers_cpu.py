"""CPU checks of the optimizer family: tests/optimizers_oracle.py against what can pin it without TensorFlow (torch.optim.SGD, torch's
clip_grad_norm_, a second RMSprop restatement), the callbacks of model_tools on scripted metric sequences against the oracle's decision
logic, and the host-side refusals.  Nothing here touches a GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import optimizers_oracle as O  # noqa: E402


@pytest.fixture(scope='module')
def mt():
    from satellite_computervision_amd import model_tools
    return model_tools


# ------------------------------------------------------------------ SGD vs torch.optim.SGD
@pytest.mark.parametrize('momentum, nesterov', [(0.0, False), (0.9, False), (0.9, True)])
def test_oracle_sgd_equals_torch_sgd(momentum, nesterov):
    """Keras keeps v = momentum v - lr g, torch buf = momentum buf + g: at a constant rate v = -lr buf, and both move the parameter by
    the same amount (nesterov: Keras momentum v - lr g = -lr (g + momentum buf), torch's nesterov form).  Twenty float64 steps.
    Bound: each step adds a few roundings of 2^-53 relative to |p| + the update (values are O(1)); 20 steps x ~8 roundings x 1.1e-16
    < 2e-14, asserted as atol 1e-13 with no relative part."""
    rng = np.random.default_rng(5)
    n, lr = 257, 0.05
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) for _ in range(20)]
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([tp], lr=lr, momentum=momentum, nesterov=nesterov)
    p, slots = p0.copy(), {}
    for g in grads:
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p = O.sgd_step(p, g, slots, lr, momentum, nesterov)
    err = np.abs(p - tp.detach().numpy()).max()
    print(f'[fig] sgd momentum={momentum} nesterov={nesterov}: max|oracle - torch| = {err:.3e}')
    assert err <= 1e-13
    if momentum:
        buf = opt.state[tp]['momentum_buffer'].numpy()
        assert np.abs(slots['v'] + lr * buf).max() <= 1e-13          # the substitution itself
    else:
        assert 'v' not in slots


# ------------------------------------------------------------------ global_clipnorm vs torch.nn.utils.clip_grad_norm_
def test_oracle_global_clipnorm_equals_torch_clip_grad_norm():
    """torch scales by c / (norm + 1e-6), clamped to 1; the oracle by c / norm.  For an active clip the two results differ by the factor
    norm / (norm + 1e-6): relative difference 1e-6 / (norm + 1e-6) < 1e-6 / norm.  The inputs below have norm ~ sqrt(4001) * 3 ~ 190
    and ~ sqrt(4001) ~ 63, so the bound is 1e-6 / norm per element relative (5.3e-9 and 1.6e-8), plus float64 rounding (1e-15).  An
    inactive clip (c above the norm) returns the gradient unchanged from both, exactly."""
    rng = np.random.default_rng(6)
    for scale, c in ((3.0, 1.0), (1.0, 10.0), (1.0, 1e4)):
        shapes = [(1000,), (37, 81), (4,)]
        gs = [scale * rng.standard_normal(s) for s in shapes]
        flat = np.concatenate([g.ravel() for g in gs])
        ps = [torch.zeros(s, dtype=torch.float64, requires_grad=True) for s in shapes]
        for pt, g in zip(ps, gs):
            pt.grad = torch.tensor(g)
        tn = float(torch.nn.utils.clip_grad_norm_(ps, c))
        got, n = O.clip_global_norm(flat, c)
        ref = np.concatenate([pt.grad.numpy().ravel() for pt in ps])
        assert abs(n - tn) <= 1e-12 * n
        if n <= c:
            assert np.array_equal(got, flat) and np.array_equal(ref, flat)
            continue
        bound = 1e-6 / n + 1e-15
        rel = np.abs(got - ref).max() / np.abs(ref).max()
        print(f'[fig] clipnorm c={c} norm={n:.3f}: rel diff {rel:.3e} (bound {bound:.3e})')
        assert np.all(np.abs(got - ref) <= bound * np.abs(got) + 1e-300)
        assert abs(O.global_norm(got) - c) <= 1e-12 * c


def test_oracle_clip_value_and_non_finite_norm():
    g = np.array([-3.0, -0.5, 0.0, 0.25, 7.0])
    assert np.array_equal(O.clip_value(g, 0.5), [-0.5, -0.5, 0.0, 0.25, 0.5])
    bad = np.array([1.0, np.inf, -2.0])
    out, n = O.clip_global_norm(bad, 1.0)
    assert np.isinf(n) and np.array_equal(out, bad)


# ------------------------------------------------------------------ RMSprop vs an independent restatement
def _rmsprop_second(p, grads, lr, rho, momentum, eps, centered):
    """written from the ApplyRMSProp / ApplyCenteredRMSProp documentation element by element, in plain Python floats"""
    p = [float(x) for x in p]
    ms, mg, mom = [0.0] * len(p), [0.0] * len(p), [0.0] * len(p)
    for g in grads:
        for i, gi in enumerate(g):
            gi = float(gi)
            ms[i] = ms[i] + (gi * gi - ms[i]) * (1.0 - rho)          # TensorFlow's incremental form of rho ms + (1 - rho) g^2
            if centered:
                mg[i] = mg[i] + (gi - mg[i]) * (1.0 - rho)
            denom = (ms[i] - (mg[i] * mg[i] if centered else 0.0) + eps) ** 0.5
            mom[i] = momentum * mom[i] + lr * gi / denom
            p[i] -= mom[i]
    return np.array(p)


@pytest.mark.parametrize('centered', [False, True])
@pytest.mark.parametrize('momentum', [0.0, 0.8])
def test_oracle_rmsprop_equals_second_restatement(momentum, centered):
    """(torch.optim.RMSprop adds epsilon OUTSIDE the root, so it cannot pin this rule.)  Both restatements are float64; the two
    algebraic forms of the moving averages differ by rounding only: 12 steps of O(1) values, asserted to 1e-12."""
    rng = np.random.default_rng(8)
    p0 = rng.standard_normal(33)
    grads = [rng.standard_normal(33) * (1 + k) for k in range(12)]
    p, slots = p0.copy(), {}
    for g in grads:
        p = O.rmsprop_step(p, g, slots, 2e-3, 0.9, momentum, 1e-7, centered)
    ref = _rmsprop_second(p0, grads, 2e-3, 0.9, momentum, 1e-7, centered)
    assert np.abs(p - ref).max() <= 1e-12
    assert ('mg' in slots) == centered and ('mom' in slots) == (momentum > 0)


def test_oracle_adam_first_step_closed_form():
    """step 1 from zero moments: m = (1 - b1) g, v = (1 - b2) g^2, so the update is lr g / (|g| + eps / sqrt(1 - b2)) in closed form"""
    g = np.array([1e-3, -5.0, 2.0])
    p = O.adam_step(np.zeros(3), g, {}, 1e-2)
    np.testing.assert_allclose(p, -1e-2 * g / (np.abs(g) + 1e-7 / np.sqrt(1 - 0.999)), rtol=1e-12)


# ------------------------------------------------------------------ callbacks on scripted metric sequences
def _fake_model(mt, opt):
    m = types.SimpleNamespace(optimizer=opt, stop_training=False, weights={'w': np.zeros(2)})
    m.get_weights_dict = lambda: {k: v.copy() for k, v in m.weights.items()}
    m.set_weights_dict = lambda d: m.weights.update({k: np.array(v) for k, v in d.items()})
    return m


def _drive(mt, cb, model, name, values, on_epoch=None):
    """run a callback over the scripted values as fit() does; -> the `lr` logged per epoch"""
    cb.model = model
    mt.run_callbacks([cb], 'on_train_begin')
    lrs = []
    for epoch, v in enumerate(values):
        mt.run_callbacks([cb], 'on_epoch_begin', epoch)
        if on_epoch:
            on_epoch(epoch)
        logs = {name: v}
        cb.on_epoch_end(epoch, logs)
        lrs.append(logs.get('lr'))
        if model.stop_training:
            break
    return lrs


def test_reduce_lr_on_plateau_plateau_cooldown_and_min_lr(mt):
    vals = [1.0, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.9, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    kw = dict(factor=0.1, patience=2, min_delta=1e-3, cooldown=2, min_lr=5e-4)
    opt = mt.SGD(0.1)
    cb = mt.ReduceLROnPlateau(monitor='val_loss', mode='min', **kw)
    lrs = _drive(mt, cb, _fake_model(mt, opt), 'val_loss', vals)
    want, final = O.reduce_lr_on_plateau(vals, 0.1, mode='min', **kw)
    assert lrs == pytest.approx(want, rel=1e-12)
    assert float(opt.learning_rate) == pytest.approx(final, rel=1e-12)
    # spelled out: two flat epochs -> 0.01 after epoch 3; two cooldown epochs, two more flat ones -> 0.001 after epoch 7; ... -> the floor
    assert want[:4] == [0.1, 0.1, 0.1, 0.1] and want[4] == pytest.approx(0.01) and want[8] == pytest.approx(0.001)
    assert min(want + [final]) == pytest.approx(5e-4) and final == pytest.approx(5e-4)


def test_reduce_lr_on_plateau_mode_max(mt):
    vals = [0.5, 0.6, 0.6, 0.6, 0.7, 0.65, 0.65]
    opt = mt.Adam(1e-3)
    cb = mt.ReduceLROnPlateau(monitor='val_accuracy', factor=0.5, patience=2, min_delta=0.0, mode='auto')
    assert cb.mode == 'max'
    lrs = _drive(mt, cb, _fake_model(mt, opt), 'val_accuracy', vals)
    want, final = O.reduce_lr_on_plateau(vals, 1e-3, factor=0.5, patience=2, min_delta=0.0, mode='max')
    assert lrs == pytest.approx(want, rel=1e-12) and float(opt.learning_rate) == pytest.approx(final, rel=1e-12)
    assert want == pytest.approx([1e-3, 1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 5e-4]) and final == pytest.approx(2.5e-4)
    with pytest.raises(ValueError):
        mt.ReduceLROnPlateau(factor=1.0)


@pytest.mark.parametrize('mode, vals', [('min', [1.0, 0.8, 0.7, 0.75, 0.72, 0.71, 0.6]), ('max', [0.1, 0.3, 0.5, 0.45, 0.5, 0.49, 0.9])])
def test_early_stopping_stops_and_restores(mt, mode, vals):
    model = _fake_model(mt, mt.SGD(0.1))
    cb = mt.EarlyStopping(monitor='score', min_delta=0.0, patience=3, mode=mode, restore_best_weights=True)

    def train(epoch):
        model.weights['w'] = np.array([float(epoch), -float(epoch)])       # "the parameters of epoch e"
    ran = _drive(mt, cb, model, 'score', vals, on_epoch=train)
    stop, best = O.early_stopping(vals, 0.0, 3, mode)
    assert (stop, best) == (5, 2)
    assert model.stop_training and cb.stopped_epoch == stop and len(ran) == stop + 1 and cb.best_epoch == best
    assert np.array_equal(model.weights['w'], [float(best), -float(best)])
    # without restore the last epoch's parameters stay
    model2 = _fake_model(mt, mt.SGD(0.1))
    cb2 = mt.EarlyStopping(monitor='score', patience=3, mode=mode)

    def train2(epoch):
        model2.weights['w'] = np.array([float(epoch), -float(epoch)])
    _drive(mt, cb2, model2, 'score', vals, on_epoch=train2)
    assert np.array_equal(model2.weights['w'], [float(stop), -float(stop)])


def test_early_stopping_min_delta(mt):
    vals = [1.0, 0.95, 0.93, 0.92, 0.5]
    stop, best = O.early_stopping(vals, 0.1, 2, 'min')
    assert (stop, best) == (2, 0)
    model = _fake_model(mt, mt.SGD(0.1))
    ran = _drive(mt, mt.EarlyStopping(monitor='loss', min_delta=0.1, patience=2), model, 'loss', vals)
    assert len(ran) == 3 and model.stop_training


def test_learning_rate_scheduler(mt):
    opt = mt.RMSprop(1e-2)
    sched = lambda epoch, lr: lr * (0.5 if epoch % 2 else 1.0)      # noqa: E731
    lrs = _drive(mt, mt.LearningRateScheduler(sched), _fake_model(mt, opt), 'loss', [1.0] * 5)
    assert lrs == pytest.approx(O.scheduled_rates(sched, 1e-2, 5), rel=1e-12)
    opt1 = mt.SGD(1.0)
    assert _drive(mt, mt.LearningRateScheduler(lambda epoch: 0.1 / (epoch + 1)), _fake_model(mt, opt1), 'loss', [1.0] * 3) == pytest.approx([0.1, 0.05, 0.1 / 3])
    with pytest.raises(ValueError):
        _drive(mt, mt.LearningRateScheduler(lambda epoch, lr: 'fast'), _fake_model(mt, mt.SGD()), 'loss', [1.0])


# ------------------------------------------------------------------ host-side surface and refusals
def test_optimizer_arguments_and_refusals(mt):
    assert float(mt.SGD().learning_rate) == 0.01 and mt.SGD().momentum == 0.0 and mt.SGD().slot_names == ()
    assert mt.SGD(lr=0.3, momentum=0.9, nesterov=True).slot_names == ('v',) and float(mt.SGD(lr=0.3).lr) == 0.3
    r = mt.RMSprop()
    assert (float(r.learning_rate), r.rho, r.momentum, r.epsilon, r.centered) == (1e-3, 0.9, 0.0, 1e-7, False) and r.slot_names == ('ms',)
    assert mt.RMSprop(centered=True, momentum=0.5).slot_names == ('ms', 'mg', 'mom')
    a = mt.Adam()
    assert (float(a.learning_rate), a.beta_1, a.beta_2, a.epsilon, a.clipvalue, a.global_clipnorm) == (1e-3, 0.9, 0.999, 1e-7, None, None)
    o = mt.SGD(0.1)
    o.learning_rate = 0.05
    assert float(o.lr) == 0.05 and o.learning_rate.numpy() == np.float32(0.05)
    o.lr.assign(0.02)
    assert float(o.learning_rate) == 0.02
    for cls in (mt.Adam, mt.SGD, mt.RMSprop):
        assert cls(clipvalue=0.5).clipvalue == 0.5 and cls(global_clipnorm=2.0).global_clipnorm == 2.0
        with pytest.raises(ValueError, match='at most one'):
            cls(clipvalue=0.5, global_clipnorm=1.0)
        with pytest.raises(ValueError, match='global_clipnorm'):
            cls(clipnorm=1.0)
        with pytest.raises(ValueError):
            cls(clipvalue=-1.0)
    with pytest.raises(TypeError):
        mt.SGD(decay=1e-4)
    with pytest.raises(ValueError):
        mt.SGD(momentum=1.5)


def test_compile_refuses_unknown_optimizers(mt):
    class LooksLikeAdam:                      # carries the three names the old step read: it used to train as Adam
        beta_1, beta_2, epsilon, _lr = 0.9, 0.999, 1e-7, 1e-3

    mt.reset_uids()
    m = mt.get_unet_model(2, 4, [16], [2])
    loss = lambda yt, yp: mt.weighted_bce(yt, yp, 2.0)      # noqa: E731
    with pytest.raises(TypeError, match='Adam.*SGD.*RMSprop'):
        m.compile(optimizer=LooksLikeAdam(), loss=loss)
    with pytest.raises(ValueError):
        m.compile(optimizer='adagrad', loss=loss)
    for name, cls in (('adam', mt.Adam), ('sgd', mt.SGD), ('rmsprop', mt.RMSprop), ('SGD', mt.SGD)):
        m.compile(optimizer=name, loss=loss)
        assert type(m.optimizer) is cls
    opt = mt.RMSprop(centered=True)
    m.compile(optimizer=opt, loss=loss)
    assert m.optimizer is opt
    assert mt.resolve_optimizer(opt) is opt
