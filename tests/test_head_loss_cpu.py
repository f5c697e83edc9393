"""tests/head_loss_oracle.py without a device: its gradients against torch autograd in float64 for every loss x activation pair the GPU
file runs, the conditions of its input builders for every seed and shape used there (no probability in a band where float32 and float64
may disagree about a clip; at most 1 % of the pixels set aside by the argmax / threshold margin masks -- shown here for the reference
alone, so the GPU file leaves nothing out on the strength of what a kernel returned), and the reach of its case tables."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_loss_oracle as H  # noqa: E402


def _t(a):
    return torch.tensor(np.asarray(a, np.float64))


def _act(z, activation):
    return torch.softmax(z, -1) if activation == H.SOFTMAX else (torch.sigmoid(z) if activation == H.SIGMOID else z)


def _inputs(activation, shape, seed, positive):
    """logits whose activation is a valid argument of the loss: a linear head feeds the point-wise losses probabilities"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(shape) * 1.5
    if activation == H.LINEAR and positive:
        z = rng.uniform(0.05, 0.95, shape)
    return z


@pytest.mark.parametrize('activation', H.ACTIVATIONS)
@pytest.mark.parametrize('ncls', H.POINTWISE_NCLS)
@pytest.mark.parametrize('kind', [H.CCE, H.BCE])
def test_pointwise_gradients_are_torch_autograd(kind, ncls, activation):
    npix, gs = 3 * 7 * 9, 128.0
    z = _inputs(activation, (npix, ncls), 10 * ncls + activation, True)
    t = H.targets_random(ncls, npix, 3).astype(np.float64)
    wts = H.CCE_WEIGHTS(ncls) if kind == H.CCE else H.BCE_WEIGHTS
    zt = _t(z).requires_grad_()
    p = _act(zt, activation)
    if kind == H.CCE:
        o = p / p.sum(-1, keepdim=True)
        lt = -(_t(wts) * _t(t) * torch.log(torch.clamp(o, H.CCE_LO, H.CCE_HI))).sum(-1).mean()
    else:
        yp = torch.clamp(p, H.BCE_LO, H.BCE_HI)
        lt = (_t(t) * -torch.log(yp) * float(wts[0]) + (1 - _t(t)) * -torch.log(1 - yp)).mean()
    (lt * gs).backward()
    r = H.pointwise_loss(kind, p.detach().numpy(), t, wts, activation, gs)
    np.testing.assert_allclose(r['loss'], lt.item(), rtol=1e-12)
    np.testing.assert_allclose(r['dlogits'], zt.grad.numpy(), atol=1e-12 * gs)
    assert r['nterms'] > 0 and r['abs_sum'] >= abs(r['loss']) * (1 - 1e-12)


@pytest.mark.parametrize('run', H.global_runs())
def test_global_gradients_are_torch_autograd(run):
    kind, activation, mode, ncls = run
    nimg, ppi, gs, eps = 3, 7 * 9, 128.0, 1e-6
    _, t = H.global_inputs(kind, activation, ncls, nimg, ppi)
    t = t.astype(np.float64)
    zt = _t(_inputs(activation, (nimg, ppi, ncls), 7 * ncls + kind, False)).requires_grad_()
    p, tt = _act(zt, activation), _t(t)
    gw = H.DICE_WEIGHTS(ncls) if mode == 'global' else None
    if kind == H.DICE:
        if gw is not None:
            wk = _t(gw.astype(np.float64)).reshape(1, ncls)
        else:
            cnt = tt.sum(1)
            wk = torch.where(cnt > 0, 1.0 / cnt ** 2, torch.full_like(cnt, float(np.float32(eps))))
        lt = (1 - 2 * (wk * (tt * p).sum(1)).sum(-1) / (wk * (tt + p).sum(1)).sum(-1)).mean()
    elif kind == H.IOU:
        lt = 1 - (tt * p).sum() / (tt + (1 - tt) * p).sum()
    else:
        fin = torch.isfinite(tt)
        lt = (torch.where(fin, p - torch.where(fin, tt, torch.zeros_like(tt)), torch.zeros_like(p)) ** 2).sum() / fin.sum()
    (lt * gs).backward()
    r = H.global_loss(kind, p.detach().numpy(), t, activation, gs, gw, eps)
    np.testing.assert_allclose(r['loss'], lt.item(), rtol=1e-12)
    np.testing.assert_allclose(r['dlogits'], zt.grad.numpy(), atol=1e-12 * gs)
    assert 0 < r['loss_bound'] < 1e-3 * max(1.0, abs(r['loss']))
    if kind == H.DICE and mode == 'counts':
        assert (t[1].sum(0) == 0).any(), 'a class is absent from image 1'


def test_head_reference_is_a_torch_conv_head():
    for activation in H.ACTIVATIONS:
        for bn in (False, True):
            x, w, b, sc, sh = H.head_inputs(3, 24, 'bf16')
            x = x[:64]
            a = torch.relu(_t(x) * _t(sc) + _t(sh)) if bn else _t(x)
            z = a @ _t(w) + _t(b)
            p, cls = H.head_fwd(x, w, b, sc if bn else None, sh if bn else None, activation, 0.3)
            np.testing.assert_allclose(p, _act(z, activation).numpy(), rtol=1e-12, atol=1e-300)
            if activation == H.SOFTMAX:
                assert np.array_equal(cls, z.argmax(-1).numpy())
            elif activation == H.SIGMOID:
                assert np.array_equal(cls, (torch.sigmoid(z) > float(np.float32(0.3))).numpy().astype(np.int32))
            else:
                assert cls is None
    # ties: the lowest index
    w = np.ones((8, 4), np.float32)
    p, cls = H.head_fwd(np.ones((5, 8)), w, np.zeros(4, np.float32), None, None, H.SOFTMAX)
    assert (cls == 0).all() and (p == 0.25).all()


def test_case_tables_reach_every_head_form():
    fast = [(1, 16), (2, 16), (1, 32), (2, 32), (3, 32), (4, 32), (1, 64), (2, 64)]          # by hand from head_fast_launch
    assert sorted(H.HEAD_FAST_FORMS) == sorted(fast) and len(set(H.HEAD_FORMS)) == len(H.HEAD_FORMS)
    generic = [f for f in H.HEAD_FORMS if f not in fast]
    assert len(generic) >= 3 and set(generic) == {(8, 32), (5, 64), (2, 8), (3, 24), (1, 128)}
    assert all(1 <= n <= H.HEAD_NCMAX and c % 8 == 0 for n, c in H.HEAD_FORMS)
    assert max(n for n, _ in H.HEAD_FORMS) == H.HEAD_NCMAX and any(c not in (16, 32, 64) for _, c in generic)
    assert H.HEAD_KINDS == ['f32', 'bf16', 'fp8']
    big = H.head_shapes()[-1]
    assert big > 2 * H.capped_stride() and big > 2 * H.HEAD_FAST_STRIDE and big % H.EW_BLOCK != 0
    assert all(s % H.HEAD_UNIQUE_ROWS != 0 for s in (H.capped_stride(), H.HEAD_FAST_STRIDE))
    assert H.pointwise_shapes()[-1] > 2 * max(H.pointwise_strides())
    assert all(ppi > 2 * H.GLOBAL_STRIDE for n, ppi in H.global_shapes()[-1:]) and H.global_shapes()[-1][0] == 2
    picks = H.probe_picks(H.pointwise_shapes()[-1], H.pointwise_strides())
    n = H.pointwise_shapes()[-1]
    assert picks == sorted({0, H.LOSS_GENERAL_STRIDE - 1, H.LOSS_GENERAL_STRIDE, H.capped_stride() - 1, H.capped_stride(), n - 3, n - 2, n - 1})
    t = H.probe_targets(n, picks, 3)
    assert t.sum() == len(picks) and (t[picks].sum(-1) == 1).all()


@pytest.mark.parametrize('kind', H.HEAD_KINDS)
@pytest.mark.parametrize('form', H.HEAD_FORMS)
def test_head_margin_masks_leave_out_at_most_one_per_cent(form, kind):
    ncls, cin = form
    x, w, b, sc, sh = H.head_inputs(ncls, cin, kind)
    for bn in (False, True):
        args = (x, w, b, sc if bn else None, sh if bn else None)
        rows = [min(n, H.HEAD_UNIQUE_ROWS) for n in H.head_shapes()]                # the GPU file's shapes are the first rows / all rows, repeated
        p, _ = H.head_fwd(*args, H.SOFTMAX)
        sure = H.argmax_margin_mask(p, H.head_fwd_bound(*args, H.SOFTMAX))
        assert all(1.0 - sure[:n].mean() <= 0.01 for n in rows)
        for thresh in (0.5, 0.3):
            p, _ = H.head_fwd(*args, H.SIGMOID, thresh)
            sure = H.thresh_margin_mask(p, H.head_fwd_bound(*args, H.SIGMOID, thresh), thresh).all(-1)
            assert all(1.0 - sure[:n].mean() <= 0.01 for n in rows)
        for activation in H.ACTIVATIONS:
            bound, (ref, _) = H.head_fwd_bound(*args, activation), H.head_fwd(*args, activation)
            assert bound.shape == ref.shape and (bound > 0).all() and bound.max() < 1e-3           # a bound, not a licence


@pytest.mark.parametrize('ncls', H.POINTWISE_NCLS)
@pytest.mark.parametrize('kind', [H.CCE, H.BCE])
def test_probability_builders_keep_clear_of_the_ambiguous_bands(kind, ncls):
    amb = H.cce_ambiguous if kind == H.CCE else H.bce_ambiguous
    for npix in H.pointwise_shapes():
        seed = H.pointwise_seed(kind, ncls, npix)
        for p in (H.probs_random(ncls, npix, seed, kind), H.probs_saturated(ncls, npix, seed, kind)):      # the second asserts its branches itself
            assert p.dtype == np.float32 and p.shape == (npix, ncls) and np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all()
            assert not amb(p).any()
        if kind == H.BCE:                                       # the rows a softmax head hands the loss
            p = H.probs_random(ncls, npix, seed, kind, rows_sum_to_one=True)
            assert not amb(p).any() and np.abs(p.sum(-1, dtype=np.float64) - 1).max() < 1e-6
        p = H.probs_saturated(ncls, npix, seed, kind)[:5].astype(np.float64)                                # the first five pixels hold every mode
        inside = H.cce_inside(p)[0] if kind == H.CCE else H.bce_inside(p)
        assert (ncls == 1 and kind == H.CCE) or (inside.any() and not inside.all())
    # the bands themselves
    assert H.cce_ambiguous(np.array([[1e-7, 1.0]])).any() and not H.cce_ambiguous(np.array([[0.0, 1.0], [3e-9, 1.0], [1e-6, 1.0]])).any()
    assert H.bce_ambiguous(np.array([np.float32(1e-5), 1 - 1e-5])).all() and not H.bce_ambiguous(np.array([0.0, 1.0, 0.5, 8e-7, np.float32(1 - 8e-7)])).any()


def test_clip_constant_shifts():
    """what clipping at 1e-7f, 1 - 2^-23, 0.00001f and 0.99999f instead of the decimal constants moves a clipped logarithm by"""
    assert float(np.float32(1) - np.float32(1e-7)) == 1 - 2.0 ** -23
    assert 1.8e-8 < -H.CCE_SHIFT_HI < 2e-8 and abs(H.CCE_SHIFT_LO) < 2e-8
    assert 1.3e-3 < H.BCE_SHIFT['hi', 'q'] < 1.4e-3 and max(abs(H.BCE_SHIFT[k]) for k in (('lo', 'p'), ('lo', 'q'), ('hi', 'p'))) < 1e-7
    # loss + clip_shift is the loss clipped at those constants: one clipped element of each sort
    p, t = np.array([[1.0], [0.0], [0.5]]), np.array([[0.0], [1.0], [1.0]])
    r = H.pointwise_loss(H.BCE, p, t, H.BCE_WEIGHTS, H.SIGMOID)
    lo32, hi32 = np.float64(np.float32(H.BCE_LO)), np.float64(np.float32(H.BCE_HI))
    want = (-np.log(np.float64(np.float32(1) - np.float32(H.BCE_HI))) - 5.0 * np.log(lo32) - 5.0 * np.log(0.5)) / 3
    np.testing.assert_allclose(r['loss'] + r['clip_shift'], want, rtol=1e-14)
    r = H.pointwise_loss(H.CCE, np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([[1.0, 0.0], [1.0, 0.0]]), [2.0, 3.0], H.SOFTMAX)
    want = (-2.0 * np.log(1 - 2.0 ** -23) - 2.0 * np.log(np.float64(np.float32(1e-7)))) / 2
    np.testing.assert_allclose(r['loss'] + r['clip_shift'], want, rtol=1e-14)
