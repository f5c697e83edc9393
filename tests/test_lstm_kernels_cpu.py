"""The float64 restatements of tests/lstm_kernels_oracle.py against independent implementations that every machine has (torch float64
autograd on the CPU, oracle/convlstm.py), and the conditions tests/test_lstm_kernels_gpu.py relies on: on which size pairs the exact
and the float32 nearest index maps agree, and that every "share set aside" (hard-sigmoid values within one storage rounding of 0 or 1,
softmax ties, ReLU outputs at 0 or max_value) stays under its 1 % cap for the float64 reference alone, for the seeds and shapes the
GPU file uses."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import lstm_kernels_oracle as O  # noqa: E402
from oracle import convlstm as CL  # noqa: E402

REC = {0: 'hard_sigmoid', 1: 'sigmoid'}
ACT = {0: None, 1: 'tanh'}


# ------------------------------------------------------------------------------ cell
def torch_cell(z, c_prev, rec_kind, act_kind):
    f = z.shape[-1] // 4
    zi, zf, zg, zo = z[:, :f], z[:, f:2 * f], z[:, 2 * f:3 * f], z[:, 3 * f:]
    ra = (lambda v: torch.clamp(0.2 * v + 0.5, 0.0, 1.0)) if rec_kind == 0 else torch.sigmoid
    act = torch.tanh if act_kind else (lambda v: v)
    i, fg, o, g = ra(zi), ra(zf), ra(zo), act(zg)
    c = i * g if c_prev is None else fg * c_prev + i * g
    return c, o * act(c), torch.cat([i, fg, g, o], -1)


@pytest.mark.parametrize('rec_kind', [0, 1])
@pytest.mark.parametrize('act_kind', [0, 1])
@pytest.mark.parametrize('t0', [False, True])
def test_cell_restatement_is_torch_autograd(rec_kind, act_kind, t0):
    npix, f = 3 * 5 * 7, 16
    inp = O.cell_inputs('f32', npix, f, seed=3, t0=t0)
    z = inp['xg'] if t0 else inp['xg'] + inp['hg']
    fw = O.gates_fwd(inp['xg'], inp['hg'], inp['c_prev'], rec_kind, act_kind, 'f32')
    zt = torch.tensor(z, requires_grad=True)
    cpt = None if t0 else torch.tensor(inp['c_prev'], requires_grad=True)
    c, h, gates = torch_cell(zt, cpt, rec_kind, act_kind)
    assert np.abs(fw['c64'] - c.detach().numpy()).max() < 1e-13 and np.abs(fw['h64'] - h.detach().numpy()).max() < 1e-13
    assert np.abs(fw['gates64'] - gates.detach().numpy()).max() < 1e-13
    dh, dcn = inp['dh_a'] + inp['dh_b'], inp['dc_next']
    ((h * torch.tensor(dh)).sum() + (c * torch.tensor(dcn)).sum()).backward()
    # no |z| equals 2.5 here, so the value rule on UNROUNDED float64 gates and the pre-activation rule are the same function
    for dz, dcp in (O.gates_bwd(inp['dh_a'], inp['dh_b'], dcn, fw['gates64'], inp['c_prev'], fw['c64'], rec_kind, act_kind),
                    O.gates_bwd_from_z(dh, dcn, z, inp['c_prev'], rec_kind, act_kind)):
        assert np.abs(dz - zt.grad.numpy()).max() < 1e-13
        if not t0:
            assert np.abs(dcp - cpt.grad.numpy()).max() < 1e-13
    # one dh source, no dc_next
    dz1, _ = O.gates_bwd(None, inp['dh_b'], None, fw['gates64'], inp['c_prev'], fw['c64'], rec_kind, act_kind)
    zt.grad = None
    c, h, _ = torch_cell(zt, cpt, rec_kind, act_kind)
    (h * torch.tensor(inp['dh_b'])).sum().backward()
    assert np.abs(dz1 - zt.grad.numpy()).max() < 1e-13


def test_cell_restatement_is_the_model_oracle():
    z = np.random.default_rng(0).standard_normal((50, 8)) * 3.0
    for k in (0, 1):
        assert np.array_equal(O.rec_act(z, k), CL.rec_act_fwd(z, REC[k]))
        assert np.allclose(O.rec_act_grad_from_z(z, k), CL.rec_act_bwd(z, CL.rec_act_fwd(z, REC[k]), REC[k]), rtol=0, atol=1e-15)
        assert np.array_equal(O.cell_act(z, k), CL.act_fwd(z, ACT[k]))
    y = np.array([0.0, 1.0, np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0), 0.5, -0.0])
    assert np.array_equal(O.rec_act_grad_from_value(y, 0), [0.0, 0.0, 0.2, 0.2, 0.2, 0.0])


def test_storage_rounding_and_stats_of_the_stored_h():
    inp = O.cell_inputs('bf16', 33, 8, seed=5)
    fw = O.gates_fwd(inp['xg'], inp['hg'], inp['c_prev'], 0, 0, 'bf16')
    hb = torch.tensor(fw['h64']).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(fw['h'], hb) and np.array_equal(fw['s1'], hb.sum(0)) and np.array_equal(fw['s2'], (hb * hb).sum(0))
    assert (np.abs(fw['h'] - fw['h64']) <= O.bf16_half_ulp(fw['h64']) + 1e-7 * np.abs(fw['h64'])).all()       # (float32 on the way)
    assert np.array_equal(O.bf16_half_ulp(np.array([0.0, 1.0, 1.99, 2.0, -0.75])), [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9])
    src = np.arange(2 * 3 * 2 * 2 * 3, dtype=np.float32).reshape(2, 3, 2, 2, 3)
    out = O.ingest_seq(src, 8, 'f32')
    assert out.shape == (3, 2, 2, 2, 8) and not out[..., 3:].any() and np.array_equal(out[1, 0, :, :, :3], src[0, 1])


@pytest.mark.parametrize('case', O.COMPOSED)
def test_composed_share_near_a_hard_sigmoid_corner(case):
    kind, npix, f, rec_kind, act_kind, seed = case
    inp = O.cell_inputs(kind, npix, f, seed)
    z = inp['xg'] + inp['hg']
    assert np.abs(z).max() < 16.0                                   # the range F32_GATE_MARGIN was derived for
    amb = O.composed_ambiguous(z, kind)
    share = float(amb.mean())
    print(f'[fig] composed cell {case}: share of dz elements set aside {share:.3e} (cap 1.0e-02)')
    assert share < 0.01
    clipped = np.mean(np.abs(z) >= 2.5)
    assert 0.1 < clipped < 0.6, 'both arms and the slope of the hard sigmoid must be well represented'


# --------------------------------------------------------------------------- nearest
def test_nearest_forms_on_the_pairs_the_gpu_file_uses():
    agree = {p: O.nn_forms_agree(*p) for p in O.size_pairs()}
    print('[fig] nearest index, exact == float32 per (in, out):', agree)
    split = [p for p, a in agree.items() if not a]
    assert set(split) == set(O.SPLIT_PAIRS) and len(split) >= 2
    assert any(i < o for i, o in split) and any(i > o for i, o in split)
    assert any(i < o for i, o in agree if agree[(i, o)]) and any(i > o for i, o in agree if agree[(i, o)])
    for n_in, n_out in O.size_pairs():
        for form in ('exact', 'tf32'):
            idx = O.nn_index(n_in, n_out, form)
            assert idx.min() >= 0 and idx.max() <= n_in - 1 and (np.diff(idx) >= 0).all()
    # a source finer than the output leaves source pixels with an empty pre-image
    assert len(set(O.nn_index(26, 11, 'tf32'))) == 11 and len(set(O.nn_index(8, 4, 'tf32'))) == 4


def test_nearest_forms_split_on_22_pairs_up_to_48():
    split = [(i, o) for i in range(1, 49) for o in range(1, 49) if not O.nn_forms_agree(i, o)]
    assert len(split) == 22 and {(14, 23), (26, 11), (30, 29), (6, 37), (2, 41)} <= set(split)
    assert (8, 48) not in split


def test_model_oracle_resize_follows_the_float32_form():
    rng = np.random.default_rng(1)
    for hs, ws, h, w in O.RESIZE_PAIRS + [(8, 8, 48, 48)]:
        x = rng.standard_normal((2, hs, ws, 3))
        up, (iy, ix) = CL.resize_nearest(x, h, w)
        assert np.array_equal(iy, O.nn_index(hs, h, 'tf32')) and np.array_equal(ix, O.nn_index(ws, w, 'tf32'))
        assert np.array_equal(up, O.dense_concat([O.Src(x, resized=True)], h, w))
        g = rng.standard_normal(up.shape)
        s = O.Src(x, resized=True)
        ref = O.dense_bwd([s], np.eye(3), g.reshape(-1, 3), None, 2, 0.0, h, w)['dx'][0]
        assert np.allclose(ref, CL.resize_nearest_bwd(g, (iy, ix), hs, ws), rtol=0, atol=1e-14)


def test_nearest_is_tf_image_resize():
    """tf.image.resize(..., 'nearest') at 14 -> 23 and 26 -> 11, where the exact and the float32 index maps differ.  Without TensorFlow
    this is skipped: the float32 reading rests on recollection of TF's source (ResizeNearestNeighbor with half_pixel_centers computes
    (i + 0.5f) * (in / (float) out) and floorf in float32), not on a run of it."""
    tf = pytest.importorskip('tensorflow', reason="TensorFlow is not installed: the float32 reading rests on recollection of TF's source "
                             '(ResizeNearestNeighbor with half_pixel_centers computes (i + 0.5f) * (in / (float) out) and floorf in float32), not on a run of it')
    for n_in, n_out in O.SPLIT_PAIRS:
        x = np.arange(n_in, dtype=np.float32).reshape(1, n_in, 1, 1)
        got = tf.image.resize(x, [n_out, 1], method='nearest').numpy().reshape(-1).astype(np.int64)
        assert np.array_equal(got, O.nn_index(n_in, n_out, 'tf32')) and not np.array_equal(got, O.nn_index(n_in, n_out, 'exact'))


# ----------------------------------------------------------------------- dense heads
def torch_dense(srcs, w, b, h, w_):
    """F.conv2d 1x1 on the concatenation of F.interpolate(mode='nearest-exact') of the activated sources; -> z (npix, cout), leaf tensors"""
    leaves, cols = [], []
    for s in srcs:
        a = torch.tensor(s.activated(), requires_grad=True)
        leaves.append(a)
        t = a.permute(0, 3, 1, 2)
        cols.append(F.interpolate(t, size=(h, w_), mode='nearest-exact') if s.resized else t)
    wt = torch.tensor(np.asarray(w, np.float64), requires_grad=True)
    bt = torch.tensor(np.asarray(b, np.float64), requires_grad=True)
    z = F.conv2d(torch.cat(cols, 1), wt.t()[:, :, None, None], bt)
    return z.permute(0, 2, 3, 1).reshape(-1, wt.shape[1]), leaves, wt, bt


AGREEING = [p for p in O.RESIZE_PAIRS if O.nn_forms_agree(p[0], p[2]) and O.nn_forms_agree(p[1], p[3])]


@pytest.mark.parametrize('case', O.dense_cases(), ids=lambda c: c[0])
def test_dense_restatement_is_torch_autograd(case):
    name, cout, act, mx, specs = case
    assert len(AGREEING) == 4
    for pair in AGREEING:
        hs, ws, h, w_ = pair
        srcs, _, w, b = O.dense_inputs(case, pair, 2, seed=7)
        z, out, cls, margin = O.dense_fwd(srcs, w, b, act, mx, h, w_)
        zt, leaves, wt, bt = torch_dense(srcs, w, b, h, w_)
        assert np.abs(z - zt.detach().numpy()).max() < 1e-12
        ref_out = {0: lambda v: torch.softmax(v, -1), 1: torch.sigmoid, 2: lambda v: v,
                   3: lambda v: torch.clamp(v, 0.0, mx) if mx > 0 else torch.relu(v)}[act](zt)
        assert np.abs(out - ref_out.detach().numpy()).max() < 1e-12
        sure = margin > 1e-9
        assert np.array_equal(cls[sure], ref_out.argmax(-1).numpy()[sure])
        if act in (2, 3):
            dout = np.random.default_rng(8).standard_normal(out.shape)
            (ref_out * torch.tensor(dout)).sum().backward()
            r = O.dense_bwd(srcs, w, dout, out, act, mx, h, w_)
            assert np.abs(r['dw'] - wt.grad.numpy()).max() < 1e-11 and np.abs(r['db'] - bt.grad.numpy()).max() < 1e-11
            for dx, leaf in zip(r['dx'], leaves):
                assert dx.shape == tuple(leaf.shape) and np.abs(dx - leaf.grad.numpy()).max() < 1e-12
            assert (r['dw_abs'] >= np.abs(r['dw']) - 1e-12).all()


def test_dense_argmax_takes_the_first_maximum_and_empty_pre_images_get_zero():
    s = O.Src(np.zeros((1, 2, 2, 3)))
    _, out, cls, margin = O.dense_fwd([s], np.zeros((3, 4)), np.array([0.0, 1.0, 1.0, -1.0]), 0, 0.0, 2, 2)
    assert (cls == 1).all() and (margin == 0).all()
    s = O.Src(np.ones((1, 8, 8, 2)), resized=True)
    dx = O.dense_bwd([s], np.ones((2, 1)), np.ones((16, 1)), None, 2, 0.0, 4, 4)['dx'][0]
    assert (dx == 0).sum() == 2 * (64 - 16) and dx.sum() == 2 * 16


def test_dense_shares_set_aside():
    worst_tie, worst_relu = 0.0, 0.0
    for case, pair, nimg, seed in O.dense_gpu_cases():
        name, cout, act, mx, specs = case
        srcs, _, w, b = O.dense_inputs(case, pair, nimg, seed)
        z, out, cls, margin = O.dense_fwd(srcs, w, b, act, mx, pair[2], pair[3])
        tol = O.close_tol('f32') * max(np.abs(z).max(), 1e-6)
        if act == 0 and cout > 1:
            tie = float((margin <= O.close_tol('f32')).mean())
            worst_tie = max(worst_tie, tie)
            assert tie < 0.01, f'{name} {pair}: {tie:.3%} softmax ties'
        if act == 3:
            amb = float(O.relu_ambiguous(z, mx, tol).mean())
            worst_relu = max(worst_relu, amb)
            assert amb < 0.01, f'{name} {pair}: {amb:.3%} of the outputs at a ReLU corner'
            assert (z <= 0).any() and (mx <= 0 or (z >= mx).any()), 'both arms of the ReLU must occur'
    print(f'[fig] dense heads: worst share of softmax ties {worst_tie:.3e}, of ReLU corners {worst_relu:.3e} (cap 1.0e-02)')
