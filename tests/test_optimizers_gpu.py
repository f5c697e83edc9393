"""The optimizer family on the GPU: satcv_sgd_step / satcv_rmsprop_step / satcv_grad_clip through the C ABI against the float64
restatements of tests/optimizers_oracle.py, then through the Keras surface (compile / train_on_batch / fit with SGD, RMSprop, gradient
clipping and the learning-rate callbacks) for both model families.

Bounds (none tuned on the device): op-level parity uses the bound of tests/test_ops_gpu.py::test_adam_keras_formulation (rtol 1e-5,
atol 1e-6: the same kind of fp32 arithmetic); the U-Net trajectories use the bounds of
tests/test_model_gpu.py::test_training_trajectory_matches_oracle_over_steps (losses rtol 5e-3, ||got - ref|| < 0.5 ||update|| per
tensor, same exclusions); the captured-graph comparisons use those of the replay tests of tests/test_lstm_gpu.py (losses rtol 5e-3,
weights 3e-3); everything else is bit-exact.  Toleranced checks print their worst figure as a `[fig]` line (pytest -rP)."""
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
import optimizers_oracle as O  # noqa: E402
from oracle import losses as OL  # noqa: E402
from oracle.unet import UNetOracle  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-6          # tests/test_ops_gpu.py::test_adam_keras_formulation


@pytest.fixture(scope='module')
def mt():
    from satellite_computervision_amd import model_tools
    assert torch.cuda.is_available()
    return model_tools


@pytest.fixture(scope='module')
def ops():
    from satellite_computervision_amd import ops
    assert torch.cuda.is_available()
    return ops


@pytest.fixture(scope='module')
def lt():
    from satellite_computervision_amd import lstm_tools
    assert torch.cuda.is_available()
    return lstm_tools


def f32dev(x):
    return torch.tensor(np.asarray(x), dtype=torch.float32).cuda().contiguous()


def back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().astype(np.float64)


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def close(got, ref, what):
    err = np.abs(got - ref) - RTOL * np.abs(ref)
    print(f'[fig] {what}: max(|got - ref| - rtol |ref|) = {err.max():.3e} (atol {ATOL:.0e})')
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)


SIZES = [1003, 4 * 257, 5, 3]          # not a multiple of the vector width, a multiple, smaller than two vectors, smaller than one
BIG = 4096 * 256 * 4 + 7               # past the launch cap of the grid-stride loop (4096 workgroups of 256 lanes x 4 elements)


def _case(rng, n, with_mask):
    p, g = f32(rng.standard_normal(n)), f32(rng.standard_normal(n))
    mask = (rng.random(n) < 0.7).astype(np.float32) if with_mask else None
    return p, g, mask


# ------------------------------------------------------------------ op-level parity
@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('momentum, nesterov', [(0.0, False), (0.9, False), (0.9, True)])
def test_sgd_step_parity(ops, momentum, nesterov, with_mask):
    rng = np.random.default_rng(11)
    for n in SIZES + ([BIG] if (nesterov and with_mask) else []):
        p, g, mask = _case(rng, n, with_mask)
        pd = f32dev(p)
        vd = torch.zeros(n, device='cuda') if momentum else None
        md = f32dev(mask) if with_mask else None
        state = torch.tensor([0.05, 0.0, 1.0, 0.0], device='cuda')
        pr, slots = p.copy(), {}
        for t in range(1, 4):
            gt = f32(g * t)
            ops.sgd_step(pd, f32dev(gt), vd, state, momentum, nesterov, lr_mul=md)
            if with_mask:
                pr = O.masked(O.sgd_step, pr, gt, slots, mask, 0.05, momentum, nesterov)
            else:
                pr = O.sgd_step(pr, gt, slots, 0.05, momentum, nesterov)
        close(back(pd), pr, f'sgd n={n} momentum={momentum} nesterov={nesterov} mask={with_mask}: p')
        if momentum:
            close(back(vd), slots['v'], f'sgd n={n}: v')
        if with_mask:
            assert np.array_equal(back(pd)[mask == 0], p[mask == 0]), 'masked elements moved'
            if momentum:
                assert not back(vd)[mask == 0].any(), 'masked slots were written'
        assert state[1].item() == 0.0           # no bias correction: the step counter is Adam's


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('centered', [False, True])
@pytest.mark.parametrize('momentum', [0.0, 0.8])
def test_rmsprop_step_parity(ops, momentum, centered, with_mask):
    rng = np.random.default_rng(12)
    for n in SIZES + ([BIG] if (centered and momentum and with_mask) else []):
        p, g, mask = _case(rng, n, with_mask)
        pd, msd = f32dev(p), torch.zeros(n, device='cuda')
        mgd = torch.zeros(n, device='cuda') if centered else None
        mod = torch.zeros(n, device='cuda') if momentum else None
        md = f32dev(mask) if with_mask else None
        state = torch.tensor([2e-3, 0.0, 1.0, 0.0], device='cuda')
        pr, slots = p.copy(), {}
        for t in range(1, 4):
            gt = f32(g * t)
            ops.rmsprop_step(pd, f32dev(gt), msd, mgd, mod, state, 0.9, momentum, 1e-7, lr_mul=md)
            args = (2e-3, 0.9, momentum, 1e-7, centered)
            pr = O.masked(O.rmsprop_step, pr, gt, slots, mask, *args) if with_mask else O.rmsprop_step(pr, gt, slots, *args)
        tag = f'rmsprop n={n} momentum={momentum} centered={centered} mask={with_mask}'
        close(back(pd), pr, tag + ': p')
        close(back(msd), slots['ms'], tag + ': ms')
        if centered:
            close(back(mgd), slots['mg'], tag + ': mg')
        if momentum:
            close(back(mod), slots['mom'], tag + ': mom')
        if with_mask:
            assert np.array_equal(back(pd)[mask == 0], p[mask == 0]) and not back(msd)[mask == 0].any()


def test_update_kernels_read_rate_and_gradient_scale_from_the_state_buffer(ops):
    """lr = state[0] and grad_scale = state[2] (1 / world under data parallelism) are device values: changing them changes the next launch"""
    rng = np.random.default_rng(13)
    n = 1003
    p, g, _ = _case(rng, n, False)
    pd, vd = f32dev(p), torch.zeros(n, device='cuda')
    state = torch.tensor([0.05, 0.0, 1.0, 0.0], device='cuda')
    pr, slots = p.copy(), {}
    for lr, gs in ((0.05, 1.0), (0.005, 0.25)):
        state[0:1].fill_(lr); state[2:3].fill_(gs)
        ops.sgd_step(pd, f32dev(g), vd, state, 0.9, True)
        pr = O.sgd_step(pr, g * gs, slots, lr, 0.9, True)
    close(back(pd), pr, 'sgd with a changed rate and gradient scale')
    pd, msd = f32dev(p), torch.zeros(n, device='cuda')
    pr, slots = p.copy(), {}
    for lr, gs in ((2e-3, 1.0), (2e-4, 0.5)):
        state[0:1].fill_(lr); state[2:3].fill_(gs)
        ops.rmsprop_step(pd, f32dev(g), msd, None, None, state)
        pr = O.rmsprop_step(pr, g * gs, slots, lr)
    close(back(pd), pr, 'rmsprop with a changed rate and gradient scale')


@pytest.mark.parametrize('n', SIZES + [BIG])
def test_grad_clip_parity(ops, n):
    rng = np.random.default_rng(14)
    g = f32(rng.standard_normal(n))
    # clipvalue: a selection, so bit-exact; with a gradient scale the bound applies to g * scale
    gd = f32dev(g)
    ops.grad_clip(gd, ops.CLIP_VALUE, 0.5)
    assert np.array_equal(back(gd), O.clip_value(g, 0.5))
    gd = f32dev(g)
    ops.grad_clip(gd, ops.CLIP_VALUE, 0.5, state=torch.tensor([1e-3, 0.0, 0.25, 0.0], device='cuda'))
    assert np.array_equal(back(gd) * 0.25, O.clip_value(g * 0.25, 0.5))
    # global norm, active and with a gradient scale
    norm = O.global_norm(g)
    for c, gs in ((0.5 * norm, 1.0), (0.1 * norm, 0.5)):
        gd = f32dev(g)
        ws = ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, float(np.float32(c)), state=torch.tensor([1e-3, 0.0, gs, 0.0], device='cuda'))
        ref, _ = O.clip_global_norm(g * gs, float(np.float32(c)))
        close(back(gd) * gs, ref, f'global_clipnorm n={n} c={c:.3f} grad_scale={gs}')
        assert abs(np.sqrt(back(ws)[1024]) - norm) <= 2.0 ** -24 * norm
    # NaN in: clipvalue keeps it, the global norm is NaN and the gradient stays as it is
    bad = g.copy(); bad[n // 2] = np.nan
    gd = f32dev(bad)
    ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, 1e-3)
    assert np.array_equal(back(gd), bad, equal_nan=True)
    bad[0] = np.inf; bad[n // 2] = 1.0
    gd = f32dev(bad)
    ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, 1e-3)
    assert np.array_equal(back(gd), f32(bad))


def test_new_entry_points_refuse_bad_arguments(ops):
    from satellite_computervision_amd._lib import lib
    st = ops.stream_ptr()
    p, g, v = (torch.zeros(16, device='cuda') for _ in range(3))
    state = torch.tensor([0.1, 0.0, 1.0, 0.0], device='cuda')
    ws = ops.grad_clip_workspace(16, 'cuda')
    assert lib.satcv_grad_clip_workspace(16) == 1025 * 8 and lib.satcv_grad_clip_workspace(0) == 0
    P, G, V, S = p.data_ptr(), g.data_ptr(), v.data_ptr(), state.data_ptr()
    assert lib.satcv_sgd_step(P, G, None, 16, 0.9, 0, S, None, st) != 0            # momentum without its slot
    assert lib.satcv_sgd_step(P, G, V, 16, 0.0, 0, S, None, st) != 0               # a slot without momentum
    assert lib.satcv_sgd_step(P, G, None, 16, 0.0, 1, S, None, st) != 0            # nesterov without momentum
    assert lib.satcv_sgd_step(P + 4, G, None, 8, 0.0, 0, S, None, st) != 0         # misaligned
    assert lib.satcv_sgd_step(P, G, None, 0, 0.0, 0, S, None, st) != 0
    assert lib.satcv_rmsprop_step(P, G, None, None, None, 16, 0.9, 0.0, 1e-7, S, None, st) != 0
    assert lib.satcv_rmsprop_step(P, G, V, None, None, 16, 0.9, 0.5, 1e-7, S, None, st) != 0
    assert lib.satcv_grad_clip(G, 16, 1, 1.0, S, None, st) != 0                    # global norm without a workspace
    assert lib.satcv_grad_clip(G, 16, 2, 1.0, S, ws.data_ptr(), st) != 0           # unknown mode
    assert lib.satcv_grad_clip(G, 16, 0, 0.0, S, None, st) != 0                    # c must be positive
    torch.cuda.synchronize()
    assert not p.any() and not g.any() and not v.any()


# ------------------------------------------------------------------ global norm: reproducibility
def test_global_norm_is_bit_reproducible_across_runs_and_streams(ops):
    """a few million elements: the squared norm (double) and the clipped gradient are the same BITS on every run and on every stream --
    the partition and the order of the sum depend on n alone -- and the norm agrees with float64 NumPy to fp32 rounding of its value."""
    rng = np.random.default_rng(15)
    n = 3_000_001
    g = rng.standard_normal(n).astype(np.float32)
    ref = O.global_norm(g)
    c = float(np.float32(0.37 * ref))
    results = []
    streams = [None, None, torch.cuda.Stream(), torch.cuda.Stream(priority=-1)]
    for s in streams:
        gd = torch.from_numpy(g).cuda()
        torch.cuda.synchronize()
        if s is None:
            ws = ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, c)
        else:
            with torch.cuda.stream(s):
                ws = ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, c)
        torch.cuda.synchronize()
        results.append((ws.cpu().numpy().copy(), gd.cpu().numpy().copy()))
    for ws, out in results[1:]:
        assert np.array_equal(ws.view(np.uint64), results[0][0].view(np.uint64)), 'partials / norm differ between runs or streams'
        assert np.array_equal(out.view(np.uint32), results[0][1].view(np.uint32)), 'clipped gradient differs between runs or streams'
    norm = float(np.sqrt(results[0][0][1024]))
    print(f'[fig] global norm of {n} elements: device {norm!r} float64 {ref!r} rel {abs(norm - ref) / ref:.3e}')
    assert abs(norm - ref) <= 2.0 ** -24 * ref
    close(results[0][1].astype(np.float64), O.clip_global_norm(g, c)[0], 'clipped gradient of a few million elements')


def test_global_norm_below_the_threshold_returns_the_gradient_bit_identical(ops):
    rng = np.random.default_rng(16)
    for n in (1003, 3_000_001):
        g = rng.standard_normal(n).astype(np.float32)
        for c in (1.0001 * O.global_norm(g), 1e6):
            gd = torch.from_numpy(g).cuda()
            ops.grad_clip(gd, ops.CLIP_GLOBAL_NORM, float(c))
            torch.cuda.synchronize()
            assert np.array_equal(gd.cpu().numpy().view(np.uint32), g.view(np.uint32))


# ------------------------------------------------------------------ U-Net models
LOSS_W = [1.0, 2.0]


def build_pair(mt, filters=(32, 64), factors=(2, 2), seed=9):
    """the same fp32-representable weights in the float64 oracle and the device model (as tests/test_model_gpu.py does)"""
    o = UNetOracle(2, 4, list(filters), list(factors), dtype=np.float64, seed=seed)
    rng = np.random.default_rng(seed + 1)
    for n, _, kind in o.specs:
        if kind in ('gamma', 'beta', 'bias', 'mm'):
            o.params[n] = o.params[n] + 0.2 * rng.standard_normal(o.params[n].shape)
        if kind == 'mv':
            o.params[n] = o.params[n] * (0.5 + rng.random(o.params[n].shape))
    for n in o.params:
        o.params[n] = o.params[n].astype(np.float32).astype(np.float64)
    mt.reset_uids()
    m = mt.get_unet_model(2, 4, list(filters), list(factors))
    m.compute_dtype = 'float32'
    names = mt.structural_names(m)
    m.set_weights_dict({names[k]: v for k, v in o.params.items()})
    return o, m, names


def batch():
    rng = np.random.default_rng(33)
    x = rng.random((4, 32, 32, 4)).astype(np.float32)
    lab = (x[..., 0] + x[..., 2] > 1.0).astype(np.int64)
    return x, np.eye(2)[lab].astype(np.float32)


def unet_loss(mt):
    return lambda yt, yp: mt.weighted_categorical_crossentropy(yt, yp, LOSS_W)


def make_opts(mt):
    return {'sgd': lambda: mt.SGD(0.05, momentum=0.9, nesterov=True),
            'sgd_plain_clipvalue': lambda: mt.SGD(0.05, clipvalue=1e-2),
            'rmsprop': lambda: mt.RMSprop(2e-3, centered=True, global_clipnorm=1.0),
            'rmsprop_momentum': lambda: mt.RMSprop(1e-3, momentum=0.5),
            'adam_clipnorm': lambda: mt.Adam(2e-3, global_clipnorm=1.0)}


CLIP_C = 1.0        # the oracle's gradient norms over the five RMSprop steps below are 1.59, 0.81, 0.89, 0.54, 0.46: step 1 is clipped, the others are not


@pytest.mark.parametrize('which', ['sgd', 'rmsprop'])
def test_unet_trajectory_matches_oracle(mt, which):
    """five fp32 steps with SGD(momentum=0.9, nesterov=True) and with RMSprop(centered=True, global_clipnorm=c) against the oracle/ U-Net
    backward + the optimizer oracle doing the same five steps; bounds and exclusions of test_training_trajectory_matches_oracle_over_steps"""
    o, m, names = build_pair(mt)
    x, t = batch()
    if which == 'sgd':
        m.compile(optimizer=mt.SGD(0.05, momentum=0.9, nesterov=True), loss=unet_loss(mt))
        step = lambda p, g, s: O.sgd_step(p, g, s, 0.05, 0.9, True)                       # noqa: E731
    else:
        m.compile(optimizer=mt.RMSprop(2e-3, centered=True, global_clipnorm=CLIP_C), loss=unet_loss(mt))
        step = lambda p, g, s: O.rmsprop_step(p, g, s, 2e-3, 0.9, 0.0, 1e-7, True)        # noqa: E731
    p_start = {k: v.copy() for k, v in o.params.items()}
    slots = {k: {} for k in o.trainable}
    dev_losses, ref_losses, norms = [], [], []
    for _ in range(5):
        pr, _ = o.forward(x, training=True)
        loss_ref, dprobs, _ = OL.weighted_categorical_crossentropy(t.astype(np.float64), pr, LOSS_W)
        g = o.backward(dprobs)
        if which == 'rmsprop':
            flat = np.concatenate([g[k].ravel() for k in o.trainable])
            _, nrm = O.clip_global_norm(flat, CLIP_C)
            norms.append(nrm)
            scale = CLIP_C / nrm if nrm > CLIP_C else 1.0
            g = {k: g[k] * scale for k in o.trainable}
        for k in o.trainable:
            o.params[k] = step(o.params[k], g[k], slots[k])
        ref_losses.append(float(loss_ref))
        dev_losses.append(m.train_on_batch(x, t))
    print(f'[fig] {which}: losses device {dev_losses} oracle {ref_losses} norms {norms}')
    if which == 'rmsprop':
        assert any(n > 1.05 * CLIP_C for n in norms) and any(n < 0.95 * CLIP_C for n in norms), norms      # clipping active and inactive
    np.testing.assert_allclose(dev_losses, ref_losses, rtol=5e-3)
    assert ref_losses[-1] < ref_losses[0]
    w = m.get_weights_dict()
    for k in o.params:
        if k.endswith('.bias') and not k.startswith('probs'):
            continue
        if k.endswith('moving_mean') or k.endswith('moving_var'):
            continue
        ref, got = o.params[k], w[names[k]].astype(np.float64)
        upd = np.linalg.norm(ref - p_start[k])
        assert np.linalg.norm(got - ref) < 0.5 * max(upd, 1e-9), f'{k}: {np.linalg.norm(got - ref):.3e} vs update {upd:.3e}'


@pytest.mark.parametrize('which', ['sgd', 'sgd_plain_clipvalue', 'rmsprop', 'rmsprop_momentum', 'adam_clipnorm'])
def test_two_identical_runs_end_in_identical_bits(mt, which):
    x, t = batch()
    runs = []
    for _ in range(2):
        _, m, _ = build_pair(mt)
        m.compile(optimizer=make_opts(mt)[which](), loss=unet_loss(mt))
        for _ in range(4):
            m.train_on_batch(x, t)
        rt = m.runtime
        torch.cuda.synchronize()
        slots = {k: v.cpu().numpy().copy() for k, v in rt.opt_slots(m.optimizer).items()}
        assert set(slots) == set(m.optimizer.slot_names)
        runs.append((m.get_weights_dict(), slots))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k].view(np.uint32), runs[1][0][k].view(np.uint32)), k
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k].view(np.uint32), runs[1][1][k].view(np.uint32)), k


@pytest.mark.parametrize('which', ['sgd', 'rmsprop', 'rmsprop_momentum', 'adam_clipnorm'])
def test_frozen_layer_keeps_its_weights_bit_for_bit(mt, which):
    _, m, _ = build_pair(mt)
    x, t = batch()
    m.compile(optimizer=make_opts(mt)[which](), loss=unet_loss(mt))
    frozen = [l for l in m.layers if any(p.name.endswith('/kernel') for p in l.specs)][1]
    frozen.trainable = False
    w0 = m.get_weights_dict()
    for _ in range(3):
        m.train_on_batch(x, t)
    w1 = m.get_weights_dict()
    mine = {p.name for p in frozen.specs}
    for k in w0:
        same = np.array_equal(w0[k].view(np.uint32), w1[k].view(np.uint32))
        if k in mine:
            assert same, f'frozen {k} moved'
    moved = [k for k in w0 if k.endswith('/kernel') and k not in mine and not np.array_equal(w0[k], w1[k])]
    assert len(moved) == sum(1 for k in w0 if k.endswith('/kernel')) - 1, 'the other layers must train'
    for k, v in m.runtime.opt_slots(m.optimizer).items():
        off = m.runtime.offsets[frozen.kernel_name]
        assert not v[off:off + 16].any(), f'slot {k} of the frozen layer was written'


def test_recompiling_with_another_optimizer_resets_the_slots(mt):
    _, m, _ = build_pair(mt)
    x, t = batch()
    m.compile(optimizer=mt.Adam(1e-3), loss=unet_loss(mt))
    m.train_on_batch(x, t)
    rt = m.runtime
    assert rt.slot_kind == 'adam' and set(rt.slots) == {'m', 'v'} and rt.adam_state[1].item() == 1.0
    m.compile(optimizer=mt.SGD(0.01, momentum=0.9), loss=unet_loss(mt))
    assert rt.slot_kind != 'adam' and 'm' not in rt.slots and rt.adam_state[1].item() == 0.0
    m.train_on_batch(x, t)
    assert set(rt.slots) == {'v'} and rt.slots['v'].any() and rt.slot_kind != 'adam' and 'm' not in rt.slots
    v1 = rt.slots['v'].clone()
    m.compile(optimizer=mt.SGD(0.01, momentum=0.9), loss=unet_loss(mt))         # a NEW optimizer object: fresh slots, as in Keras
    assert not rt.slots
    m.compile(optimizer=mt.RMSprop(centered=True), loss=unet_loss(mt))
    m.train_on_batch(x, t)
    assert set(rt.slots) == {'ms', 'mg'} and not torch.equal(rt.slots['ms'], v1)
    m.compile(optimizer='sgd', loss=unet_loss(mt))
    m.train_on_batch(x, t)
    assert not rt.slots, 'plain SGD owns no slot'


@pytest.mark.parametrize('ext', ['npz', 'h5'])
def test_saved_model_carries_the_new_slots(mt, tmp_path, ext):
    """Model.save stores the Adam moments; the SGD / RMSprop slots follow the same rule and come back bit for bit"""
    _, m, _ = build_pair(mt)
    x, t = batch()
    m.compile(optimizer=mt.RMSprop(1e-3, momentum=0.5, centered=True), loss=unet_loss(mt))
    for _ in range(2):
        m.train_on_batch(x, t)
    path = str(tmp_path / f'model.{ext}')
    m.save(path)
    mt.set_compute_dtype('float32')          # (a loaded model builds its runtime at once, in the default compute type)
    try:
        m2 = mt.load_model(path)
    finally:
        mt.set_compute_dtype('bfloat16')
    keys = {'ms', 'mg', 'mom'}
    if ext == 'npz':
        with np.load(path) as z:
            assert {f'__rmsprop_{k}__' for k in keys} | {'__opt_kind__', '__opt_state__'} <= set(z.files) and str(z['__opt_kind__']) == 'rmsprop'
    else:
        from satellite_computervision_amd import hdf5_io
        with hdf5_io.File(path) as f:
            assert all(f'optimizer_weights/satcv_rmsprop/{k}:0' in f for k in keys | {'state'})
    assert m2.runtime.slot_kind == 'rmsprop' and set(m2.runtime.slots) == keys
    for k, v in m.runtime.slots.items():
        assert torch.equal(v.cpu(), m2.runtime.slots[k].cpu()), k
    m2.compile(optimizer=mt.RMSprop(1e-3, momentum=0.5, centered=True), loss=unet_loss(mt))
    a, b = m.train_on_batch(x, t), m2.train_on_batch(x, t)
    assert a == pytest.approx(b, rel=1e-6)          # (the loss scalar is a sum whose last bit is not part of the reproducibility contract; the parameters are)
    w, w2 = m.get_weights_dict(), m2.get_weights_dict()
    for k in w:
        assert np.array_equal(w[k].view(np.uint32), w2[k].view(np.uint32)), k
    if ext == 'h5':                          # the SGD momentum slot under its own group of the same file layout
        m.compile(optimizer=mt.SGD(0.01, momentum=0.9), loss=unet_loss(mt))
        m.train_on_batch(x, t)
        m.save(path)
        with hdf5_io.File(path) as f:
            assert 'optimizer_weights/satcv_sgd/v:0' in f and 'optimizer_weights/satcv_sgd/state:0' in f and 'optimizer_weights/satcv_rmsprop/ms:0' not in f
        mt.set_compute_dtype('float32')
        try:
            m3 = mt.load_model(path)
        finally:
            mt.set_compute_dtype('bfloat16')
        assert m3.runtime.slot_kind == 'sgd' and set(m3.runtime.slots) == {'v'} and torch.equal(m3.runtime.slots['v'].cpu(), m.runtime.slots['v'].cpu())


# ------------------------------------------------------------------ the C-ABI calls of a step
NEW_SYMBOLS = ('satcv_sgd_step', 'satcv_rmsprop_step', 'satcv_grad_clip', 'satcv_grad_clip_workspace')


def record_calls(monkeypatch):
    """wrap every entry point of the library: the list of C-ABI calls a piece of Python issues, in order"""
    from satellite_computervision_amd import _lib
    calls = []

    def wrap(name, fn):
        def call(*a):
            calls.append(name)
            return fn(*a)
        return call
    for name in _lib.EXPORTED_SYMBOLS:
        monkeypatch.setattr(_lib.lib, name, wrap(name, getattr(_lib.lib, name)))
    return calls


def test_adam_step_issues_the_same_calls_as_before(mt, monkeypatch):
    """compile(optimizer=mt.Adam()) / 'adam': the step ends in satcv_adam_step and the operand repack, and nothing of the new surface runs"""
    x, t = batch()
    for opt in (lambda: mt.Adam(), lambda: 'adam'):
        _, m, _ = build_pair(mt)
        m.compile(optimizer=opt(), loss=unet_loss(mt))
        m.train_on_batch(x, t)                     # (plans are built on the first step)
        with monkeypatch.context() as mp:
            calls = record_calls(mp)
            m.train_on_batch(x, t)
        assert not [c for c in calls if c in NEW_SYMBOLS], calls
        assert calls.count('satcv_adam_step') == 1 and 'satcv_adam_step_part' not in calls
        assert calls[-2:] == ['satcv_adam_step', 'satcv_pack_weights_batched'], calls[-4:]


def test_clip_comes_before_the_step(mt, monkeypatch):
    x, t = batch()
    for opt, step in ((mt.SGD(0.01, global_clipnorm=1.0), 'satcv_sgd_step'), (mt.RMSprop(clipvalue=0.1), 'satcv_rmsprop_step'),
                      (mt.Adam(global_clipnorm=1.0), 'satcv_adam_step')):
        _, m, _ = build_pair(mt)
        m.compile(optimizer=opt, loss=unet_loss(mt))
        m.train_on_batch(x, t)
        with monkeypatch.context() as mp:
            calls = record_calls(mp)
            m.train_on_batch(x, t)
        assert calls[-3:] == ['satcv_grad_clip', step, 'satcv_pack_weights_batched'], calls[-4:]


# ------------------------------------------------------------------ callbacks in fit (U-Net family)
class Script:
    """puts a scripted metric into the epoch logs and keeps the parameters of every epoch"""

    def __init__(self, values):
        self.values, self.model, self.weights = values, None, []

    def on_epoch_end(self, epoch, logs):
        logs['script'] = self.values[epoch]
        self.weights.append(self.model.get_weights_dict())


def test_fit_runs_the_three_callbacks(mt):
    _, m, _ = build_pair(mt)
    x, t = batch()
    m.compile(optimizer=mt.SGD(0.05, momentum=0.9), loss=unet_loss(mt))
    values = [1.0, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1]
    script = Script(values)
    sched = mt.LearningRateScheduler(lambda epoch, lr: lr * 0.5 if epoch == 1 else lr)
    plateau = mt.ReduceLROnPlateau(monitor='script', factor=0.1, patience=2, min_delta=0.0, cooldown=0, min_lr=1e-4, mode='min')
    stop = mt.EarlyStopping(monitor='script', min_delta=0.0, patience=4, mode='min', restore_best_weights=True)
    h = m.fit(x, t, batch_size=2, epochs=8, verbose=0, shuffle=False, callbacks=[script, sched, plateau, stop])
    want_stop, want_best = O.early_stopping(values, 0.0, 4, 'min')
    assert (want_stop, want_best) == (5, 1)
    assert h.epoch == list(range(want_stop + 1)) and m.stop_training
    # rates: 0.05; halved by the scheduler from epoch 1; the plateau (epochs 2, 3 without improvement) cuts it after epoch 3
    want_lr, _ = O.reduce_lr_on_plateau(values[1:want_stop + 1], 0.025, factor=0.1, patience=2, min_delta=0.0, min_lr=1e-4, mode='min')
    assert h.history['lr'] == pytest.approx([0.05] + want_lr, rel=1e-12)
    assert h.history['lr'] == pytest.approx([0.05, 0.025, 0.025, 0.025, 0.0025, 0.0025], rel=1e-12)
    assert h.history['script'] == values[:want_stop + 1] and len(h.history['loss']) == want_stop + 1
    assert m.runtime.adam_state[0].item() == np.float32(float(m.optimizer.learning_rate))      # the value is in the device state buffer
    w = m.get_weights_dict()
    for k, v in script.weights[want_best].items():
        assert np.array_equal(v.view(np.uint32), w[k].view(np.uint32)), f'{k}: not the best epoch\'s parameters'
    assert any(not np.array_equal(script.weights[-1][k], w[k]) for k in w)


# ------------------------------------------------------------------ ConvLSTM family
def lstm_run(lt, mt, flag, opt, xs, ys, lrs=None):
    os.environ['SATCV_LSTM_GRAPH'] = flag
    try:
        mt.reset_uids(); mt.set_seed(7)
        m = lt.get_lstm_model(4, 3, 3, optim=opt, loss=mt.mse_4d)
        losses = []
        for i, (x, y) in enumerate(zip(xs, ys)):
            if lrs is not None:
                m.optimizer.learning_rate = lrs[i]
            losses.append(m.train_on_batch(x, y))
        return m, losses
    finally:
        os.environ.pop('SATCV_LSTM_GRAPH', None)


@pytest.mark.parametrize('which', ['sgd', 'rmsprop_clip'])
def test_lstm_model_trains_with_the_new_optimizers_and_replay_equals_the_tape(lt, mt, which):
    mt.set_compute_dtype('float32')
    try:
        rng = np.random.default_rng(23)
        xs = [rng.random((4, 3, 16, 16, 4)).astype(np.float32) for _ in range(8)]
        ys = [rng.random((4, 16, 16, 3)).astype(np.float32) for _ in range(8)]
        mk = (lambda: mt.SGD(0.02, momentum=0.9)) if which == 'sgd' else (lambda: mt.RMSprop(1e-3, centered=True, global_clipnorm=0.5))
        me, le = lstm_run(lt, mt, '0', mk(), xs, ys)
        mg, lg = lstm_run(lt, mt, '1', mk(), xs, ys)
        assert any('g' in st for st in mg._graphs.values()), 'no step was captured'
        assert set(mg.P.slots) == set(mg.optimizer.slot_names) and mg.P.slot_kind != 'adam' and 'm' not in mg.P.slots, 'the Adam moments are not allocated for another optimizer'
        print(f'[fig] lstm {which}: eager {le} replay {lg}')
        np.testing.assert_allclose(lg, le, rtol=5e-3)
        assert le[-1] < le[0] and lg[-1] < lg[0]
        we, wg = me.get_weights_dict(), mg.get_weights_dict()
        for k in we:
            assert np.abs(we[k] - wg[k]).max() < 3e-3, (k, np.abs(we[k] - wg[k]).max())
    finally:
        mt.set_compute_dtype('bfloat16')


def test_lstm_rate_change_through_reduce_lr_on_plateau_reaches_the_replayed_graph(lt, mt):
    """fit() with ReduceLROnPlateau on a captured step: the rates of the epochs are 0.1, 0.1, 0.01, 0.001 (the monitor never improves by
    min_delta), and the replayed graph -- captured in epoch 1 at rate 0.1 -- must train like an eager tape that is given those rates step by
    step, and unlike one that keeps the first rate."""
    mt.set_compute_dtype('float32')
    try:
        rng = np.random.default_rng(29)
        x = rng.random((16, 3, 16, 16, 4)).astype(np.float32)
        y = rng.random((16, 16, 16, 3)).astype(np.float32)
        os.environ['SATCV_LSTM_GRAPH'] = '1'
        try:
            mt.reset_uids(); mt.set_seed(7)
            m = lt.get_lstm_model(4, 3, 3, optim=mt.SGD(0.1), loss=mt.mse_4d)
            cb = mt.ReduceLROnPlateau(monitor='loss', factor=0.1, patience=1, min_delta=100.0, mode='min')
            h = m.fit(x, y, batch_size=4, epochs=4, callbacks=[cb])
        finally:
            os.environ.pop('SATCV_LSTM_GRAPH', None)
        assert any('g' in st for st in m._graphs.values()), 'no step was captured'
        want, final = O.reduce_lr_on_plateau(h.history['loss'], 0.1, factor=0.1, patience=1, min_delta=100.0, mode='min')
        assert h.history['lr'] == pytest.approx(want, rel=1e-12) and want == pytest.approx([0.1, 0.1, 0.01, 0.001])
        assert m.P.adam_state[0].item() == np.float32(final)
        xs, ys = [x[i:i + 4] for i in range(0, 16, 4)] * 4, [y[i:i + 4] for i in range(0, 16, 4)] * 4
        per_step = [r for r in want for _ in range(4)]
        me, _ = lstm_run(lt, mt, '0', mt.SGD(0.1), xs, ys, lrs=per_step)
        mc, _ = lstm_run(lt, mt, '0', mt.SGD(0.1), xs, ys)
        w, we, wc = m.get_weights_dict(), me.get_weights_dict(), mc.get_weights_dict()
        same = max(np.abs(w[k] - we[k]).max() for k in w)
        other = max(np.abs(w[k] - wc[k]).max() for k in w)
        print(f'[fig] replay vs eager with the same rates {same:.3e}; vs eager at the constant first rate {other:.3e}')
        assert same < 3e-3
        assert other > 10 * same, 'the replayed graph did not pick up the reduced rate'
    finally:
        mt.set_compute_dtype('bfloat16')


def test_lstm_fit_stops_early_and_restores(lt, mt):
    mt.set_compute_dtype('float32')
    try:
        rng = np.random.default_rng(31)
        x = rng.random((8, 3, 16, 16, 4)).astype(np.float32)
        y = rng.random((8, 16, 16, 3)).astype(np.float32)
        mt.reset_uids(); mt.set_seed(7)
        m = lt.get_lstm_model(4, 3, 3, optim='rmsprop', loss=mt.mse_4d)
        assert type(m.optimizer) is mt.RMSprop
        values = [0.3, 0.2, 0.25, 0.26, 0.1]
        script = Script(values)
        h = m.fit(x, y, batch_size=4, epochs=5, callbacks=[script, mt.EarlyStopping(monitor='script', patience=2, restore_best_weights=True)])
        assert h.epoch == [0, 1, 2, 3] and m.stop_training and h.history['script'] == values[:4]
        w = m.get_weights_dict()
        for k, v in script.weights[1].items():
            assert np.array_equal(v.view(np.uint32), w[k].view(np.uint32)), k
        with pytest.raises(TypeError, match='SGD'):
            m.compile(optimizer=object(), loss=mt.mse_4d)
    finally:
        mt.set_compute_dtype('bfloat16')


def test_hybrid_model_refuses_global_clipnorm_and_trains_with_clipvalue(lt, mt):
    with pytest.raises(NotImplementedError, match='global_clipnorm'):
        lt.get_hybrid_model((48, 48, 4), (3, 8, 8, 6), 3, filters=[32, 64], factors=[3, 2], compile_model=True, optim=mt.SGD(0.01, global_clipnorm=1.0),
                            loss=lambda yt, yp: mt.weighted_categorical_crossentropy(yt, yp, [1.0] * 3))
    mt.reset_uids(); mt.set_seed(5)
    m = lt.get_hybrid_model((48, 48, 4), (3, 8, 8, 6), 3, filters=[32, 64], factors=[3, 2], compile_model=True,
                            optim=mt.SGD(0.05, momentum=0.9, clipvalue=0.05), loss=lambda yt, yp: mt.weighted_categorical_crossentropy(yt, yp, [1.0] * 3))
    rng = np.random.default_rng(3)
    xu, xl = rng.random((2, 48, 48, 4)).astype(np.float32), rng.random((2, 3, 8, 8, 6)).astype(np.float32)
    y = np.eye(3, dtype=np.float32)[rng.integers(0, 3, (2, 48, 48))]
    losses = [m.train_on_batch([xu, xl], y) for _ in range(6)]
    assert np.all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert set(m.P.slots) == {'v'} and set(m.unet.runtime.slots) == {'v'} and m.unet.runtime.slot_kind != 'adam' and 'm' not in m.unet.runtime.slots
