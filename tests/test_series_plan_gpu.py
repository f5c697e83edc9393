"""lstm_infer.SeriesInferPlan on the GPU, model level: get_lstm_model(6, 3, 3) and a small get_lstm_autoencoder at B = 3, 16 x 16.

  * fused=False issues the tape's launches: torch.equal to predict_on_device (both storage types, the class tensor, the autoencoder);
  * a captured plan replays what it ran eagerly: two different inputs through one captured plan, each torch.equal to an eager plan;
  * the fused plan against predict_on_device in float32 within 1e-4 of the output scale, and in bf16 BOTH paths against
    oracle/convlstm.py within 2e-2 -- the two model-level forward bounds of tests/test_lstm_gpu.py (its inference comparison);
  * the contract structurally: under the call recorder of tools/plan_manifest.py the convolution / gate / add / head launches of
    predict_on_device and of an unfused plan's first run are the same list, field for field;
  * a filter count the step kernel refuses (LSTMLayers(..., filters=8)) takes the fallback, torch.equal to the tape;
  * predict_series_scene(plan=...) on an int16 (3, 6, 80, 112) stack, kernel 16, buff 16, batch_size 4 (short last batch), both covers.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import convlstm as CL  # noqa: E402
from plan_cases import randomise as _randomise  # noqa: E402  (non-trivial BatchNorm statistics and biases; the kernels keep their initialisers)

pytestmark = pytest.mark.gpu

NB, NCLS, T, B, H, W = 6, 3, 3, 3, 16, 16
F32_BOUND, BF16_BOUND = 1e-4, 2e-2          # tests/test_lstm_gpu.py, test_get_lstm_model_training_step_matches_oracle: rel(pred, pred_ref)


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, lstm_tools as lt, lstm_infer as li
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pt=pt, lt=lt, li=li)


def rel(got, ref):
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


def _lstm(env, dtype, activation='relu', seed=7):
    env['mt'].set_seed(seed)
    m = env['lt'].get_lstm_model(NB, NCLS, T, activation=activation)
    m.compute_dtype = dtype
    return _randomise(m, seed)


def _autoencoder(env, dtype, seed=9):
    env['mt'].set_seed(seed)
    m = env['lt'].get_lstm_autoencoder(2, 2, 1)          # 2 bands, 2 steps (one recurrent step runs), 1 output band
    m.compute_dtype = dtype
    return _randomise(m, seed)


def _ingested(env, m, seed, b=B):
    x = np.random.default_rng(seed).random((b, m.n_time, H, W, m.n_channels)).astype(np.float32)
    xt, shape = env['lt']._ingest_seq(torch.from_numpy(x).cuda(), env['ops'].rup(m.n_channels, 16), m.dtype_code)
    return x, xt, shape


# ------------------------------------------------------------------------------------------------ 1. unfused == tape
@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_unfused_plan_equals_predict_on_device(env, dtype):
    m = _lstm(env, dtype)
    _, xt, shape = _ingested(env, m, 1)
    want = m.predict_on_device(xt, shape=shape)
    plan = m.inference_plan(shape, fused=False)
    assert plan.fused_layers == ()
    for _ in range(3):                                   # eager, capture + replay, replay
        got = plan.run(xt)
        assert got.dtype == torch.float32 and torch.equal(got, want)
    assert want.abs().max() > 0
    with pytest.raises(ValueError, match='softmax'):
        plan.run(xt, want_classes=True)


def test_unfused_plan_returns_the_class_tensor_of_a_softmax_head(env):
    m = _lstm(env, 'bfloat16', activation='softmax', seed=11)
    _, xt, shape = _ingested(env, m, 2)
    want, wcls = m.predict_on_device(xt, shape=shape, want_classes=True)
    plan = m.inference_plan(shape, fused=False)
    for _ in range(2):
        got, cls = plan.run(xt, want_classes=True)
        assert torch.equal(got, want) and cls.dtype == torch.int32 and torch.equal(cls, wcls)
    assert torch.equal(plan.run(xt), want)


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_unfused_plan_of_the_autoencoder_equals_predict_on_device(env, dtype):
    m = _autoencoder(env, dtype)
    _, xt, shape = _ingested(env, m, 3)
    sincos = torch.from_numpy(np.random.default_rng(4).standard_normal((B, H, W, 2)).astype(np.float32)).cuda()
    want = m.predict_on_device([xt, sincos], shape=shape)
    plan = m.inference_plan(shape, fused=False)
    for _ in range(3):
        assert torch.equal(plan.run([xt, sincos]), want)
    assert want.abs().max() > 0

def _launch_list(calls):
    """the launches the tape and an unfused plan must share, with every non-pointer field; the prologue (weight packing, the BatchNorm
    affine) legitimately differs: the tape packs through the model's parameter store, the plan into its own images"""
    names = ('satcv_conv2d_igemm', 'satcv_convlstm_gates_fwd', 'satcv_add_act', 'satcv_dense_small_fwd')
    return [(name, structs, scalars) for name, _, structs, scalars in calls if name in names]


@pytest.mark.parametrize('kind', ['lstm_model', 'autoencoder'])
def test_unfused_plan_issues_the_launch_list_of_the_tape(env, kind):
    """`fused=False` issues exactly the tape's launches: both go through lstm_tools.convlstm_forward, the BatchNorm helpers, the
    build_lstm_layers2 tail and Dense1x1.forward.  bf16, B = 3, 16 x 16: per ConvLSTM2D one input convolution, T gate launches and T - 1
    recurrent convolutions; one satcv_add_act for the autoencoder's residual; one head."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('plan_manifest', os.path.join(HERE, '..', 'tools', 'plan_manifest.py'))
    pm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pm)
    from satellite_computervision_amd._lib import lib
    m = _lstm(env, 'bfloat16') if kind == 'lstm_model' else _autoencoder(env, 'bfloat16')
    _, x, shape = _ingested(env, m, 21)
    if kind == 'autoencoder':
        x = [x, torch.from_numpy(np.random.default_rng(22).standard_normal((B, H, W, 2)).astype(np.float32)).cuda()]
    plan = m.inference_plan(shape, fused=False)
    want, tape = pm.record_pass(lib, lambda: m.predict_on_device(x, shape=shape))
    got, planned = pm.record_pass(lib, lambda: plan.run(x))
    assert not plan.replaying and plan._runs == 1                        # the recorded run was the eager one
    tape, planned = _launch_list(tape), _launch_list(planned)
    steps = m.n_time
    count = {n: sum(c[0] == n for c in tape) for n in ('satcv_conv2d_igemm', 'satcv_convlstm_gates_fwd', 'satcv_add_act', 'satcv_dense_small_fwd')}
    assert count == {'satcv_conv2d_igemm': 2 * steps, 'satcv_convlstm_gates_fwd': 2 * steps, 'satcv_add_act': int(kind == 'autoencoder'),
                     'satcv_dense_small_fwd': 1}
    assert [c[0] for c in planned] == [c[0] for c in tape]
    for i, (a, b) in enumerate(zip(planned, tape)):
        assert a == b, (i, a[0])
    assert torch.equal(got, want) and want.abs().max() > 0


def test_hybrid_and_hierarchical_models_are_refused(env):
    lt = env['lt']
    for cls in (lt.HybridModel, lt.HierarchicalModel):                  # (refused on the type, before anything of the model is read)
        with pytest.raises(NotImplementedError, match='LSTMModel and LSTMAutoencoder'):
            cls.__new__(cls).inference_plan((2, 3, 8, 8))
    with pytest.raises(ValueError, match='time steps'):
        _lstm(env, 'bfloat16').inference_plan((B, T + 1, H, W))


# ------------------------------------------------------------------------------------------------ 2. eager == replay
@pytest.mark.parametrize('fused', [False, True])
def test_replay_equals_the_eager_plan_on_two_inputs(env, fused, monkeypatch):
    m = _lstm(env, 'bfloat16')
    _, xa, shape = _ingested(env, m, 5)
    _, xb, _ = _ingested(env, m, 6)
    monkeypatch.setenv('SATCV_LSTM_GRAPH', '0')
    eager = m.inference_plan(shape, fused=fused)
    wa = eager.run(xa).clone()
    wb = eager.run(xb).clone()
    assert not eager.replaying and not torch.equal(wa, wb)
    monkeypatch.setenv('SATCV_LSTM_GRAPH', '1')
    plan = m.inference_plan(shape, fused=fused)
    assert torch.equal(plan.run(xa), wa) and not plan.replaying          # the first run is eager
    assert torch.equal(plan.run(xa), wa) and plan.replaying              # captured and replayed
    assert torch.equal(plan.run(xb), wb)                                 # a stale static input would give wa again
    assert torch.equal(plan.run(xa), wa)
    monkeypatch.setenv('SATCV_LSTM_GRAPH', '0')                          # the switch is read per call: eager again, same buffers
    assert torch.equal(plan.run(xb), wb) and not plan.replaying


def test_a_plan_follows_changed_weights(env):
    m = _lstm(env, 'bfloat16')
    _, xt, shape = _ingested(env, m, 7)
    plan = m.inference_plan(shape, fused=True)
    for _ in range(2):
        first = plan.run(xt).clone()
    _randomise(m, 99)
    fresh = m.inference_plan(shape, fused=True).run(xt)
    got = plan.run(xt)                                                   # replayed, from repacked weights in the same buffers
    assert plan.replaying and torch.equal(got, fresh) and not torch.equal(got, first)


# ------------------------------------------------------------------------------------------------ 3. fused numerics
def _oracle_model(env, dtype):
    """get_lstm_model with the weights of oracle/convlstm.py's LSTMLayersOracle and non-trivial moving statistics -> (model, x, float64 prediction)"""
    lt = env['lt']
    o = CL.LSTMLayersOracle(NB, NCLS, filters=64, rec_act=lt.RECURRENT_ACTIVATION, seed=5)
    m = lt.get_lstm_model(NB, NCLS, T)
    m.compute_dtype = dtype
    names = {'l1': 'conv_lstm', 'l2': 'dilated_conv_lstm', 'bn1': 'batch_norm', 'bn2': 'batch_norm2', 'dense': 'conv2d'}
    w = {}
    for lk, lv in o.p.items():
        for pk, pv in lv.items():
            lv[pk] = pv.astype(np.float32).astype(np.float64)
            w[f'{names[lk]}/{pk}'] = lv[pk]
    rng = np.random.default_rng(8)
    mv = {'bn1': (rng.standard_normal(64) * 0.05, 0.5 + rng.random(64)), 'bn2': (rng.standard_normal(64) * 0.05, 0.5 + rng.random(64))}
    w.update({'batch_norm/moving_mean': mv['bn1'][0], 'batch_norm/moving_var': mv['bn1'][1],
              'batch_norm2/moving_mean': mv['bn2'][0], 'batch_norm2/moving_var': mv['bn2'][1]})
    m.set_weights_dict(w)
    mv64 = {k: (v[0].astype(np.float32).astype(np.float64), v[1].astype(np.float32).astype(np.float64)) for k, v in mv.items()}
    x = rng.random((B, T, H, W, NB)).astype(np.float32)
    return m, x, o.forward_infer(x.astype(np.float64), mv64)


def test_fused_plan_float32_against_predict_on_device(env):
    m, x, ref = _oracle_model(env, 'float32')
    xt, shape = env['lt']._ingest_seq(torch.from_numpy(x).cuda(), 16, m.dtype_code)
    want = m.predict_on_device(xt, shape=shape).cpu().numpy().astype(np.float64)
    plan = m.inference_plan(shape, fused=True)
    assert plan.fused_layers == ('conv_lstm', 'dilated_conv_lstm')
    for i in range(2):
        got = plan.run(xt).cpu().numpy().astype(np.float64)
        print(f'[fig] fused plan vs predict_on_device, float32, run {i}: {rel(got, want):.3e} (bound {F32_BOUND:.0e}); vs oracle {rel(got, ref):.3e}')
        assert rel(got, want) < F32_BOUND
        assert rel(got, ref) < F32_BOUND


def test_fused_plan_and_tape_bf16_against_the_oracle(env):
    m, x, ref = _oracle_model(env, 'bfloat16')
    xt, shape = env['lt']._ingest_seq(torch.from_numpy(x).cuda(), 16, m.dtype_code)
    tape = m.predict_on_device(xt, shape=shape).cpu().numpy().astype(np.float64)
    plan = m.inference_plan(shape, fused=True)
    assert plan.fused_layers == ('conv_lstm', 'dilated_conv_lstm')
    got = plan.run(xt).cpu().numpy().astype(np.float64)
    print(f'[fig] bf16 vs oracle/convlstm.py: tape {rel(tape, ref):.3e}, fused plan {rel(got, ref):.3e} (bound {BF16_BOUND:.0e})')
    assert rel(tape, ref) < BF16_BOUND
    assert rel(got, ref) < BF16_BOUND


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
def test_fused_plan_of_the_autoencoder(env, dtype):
    """F = 16 layers (build_lstm_layers2) with the state_h residual.  float32: against predict_on_device within the float32 bound.  bf16:
    oracle/convlstm.py has no inference form of the autoencoder, so both bf16 paths are held to the model's own float32 tape (which the test
    above ties to the oracle) within the bf16 bound."""
    m = _autoencoder(env, 'float32')
    x, xt32, shape = _ingested(env, m, 12)
    sincos = torch.from_numpy(np.random.default_rng(13).standard_normal((B, H, W, 2)).astype(np.float32)).cuda()
    ref = m.predict_on_device([xt32, sincos], shape=shape).cpu().numpy().astype(np.float64)
    if dtype == 'float32':
        plan = m.inference_plan(shape, fused=True)
        assert plan.fused_layers == ('conv_lstm', 'dilated_conv_lstm')
        got = plan.run([xt32, sincos]).cpu().numpy().astype(np.float64)
        print(f'[fig] autoencoder fused plan vs tape, float32: {rel(got, ref):.3e} (bound {F32_BOUND:.0e})')
        assert rel(got, ref) < F32_BOUND
        return
    m.compute_dtype = 'bfloat16'
    xt, _ = env['lt']._ingest_seq(torch.from_numpy(x).cuda(), 16, m.dtype_code)
    tape = m.predict_on_device([xt, sincos], shape=shape).cpu().numpy().astype(np.float64)
    got = m.inference_plan(shape, fused=True).run([xt, sincos]).cpu().numpy().astype(np.float64)
    print(f'[fig] autoencoder bf16 vs its float32 tape: tape {rel(tape, ref):.3e}, fused plan {rel(got, ref):.3e} (bound {BF16_BOUND:.0e})')
    assert rel(tape, ref) < BF16_BOUND and rel(got, ref) < BF16_BOUND


# ------------------------------------------------------------------------------------------------ 4. fallback
def test_a_refused_filter_count_takes_the_pair_and_equals_the_tape(env):
    lt = env['lt']

    class Small(lt.LSTMModel):
        def __init__(self):
            rng = np.random.default_rng(3)
            self.P = lt._Params()
            self.n_channels, self.n_classes, self.n_time = NB, NCLS, T
            self.layers_ = lt.LSTMLayers(self.P, rng, NB, filters=8)
            self._no_graph = False
            self.dense = lt.Dense1x1(self.P, rng, 'conv2d', [8], NCLS, 'relu', 2.0)
            self._finish()
    m = _randomise(Small(), 3)
    m.compute_dtype = 'bfloat16'
    _, xt, shape = _ingested(env, m, 14)
    want = m.predict_on_device(xt, shape=shape)
    plan = m.inference_plan(shape, fused=True)
    assert plan.fused_layers == ()                                       # decided at build
    for _ in range(2):
        assert torch.equal(plan.run(xt), want)
    assert want.abs().max() > 0


# ------------------------------------------------------------------------------------------------ 5. scene
SH, SW, KERNEL, BUFF, BATCH, MAXVAL = 80, 112, 16, 16, 4, 10000
OFF, SIDE = BUFF // 2, KERNEL + BUFF


def _indices(pt, cover):
    return pt.generate_chip_indices(np.empty((SH, SW, 0)), BUFF, KERNEL) if cover == 'reference' else pt.full_cover_indices((SH, SW), KERNEL)


@pytest.fixture(scope='module')
def scene(env):
    stack = np.random.default_rng(31).integers(-200, 12000, (T, NB, SH, SW)).astype(np.int16)
    return dict(stack=stack, m=_lstm(env, 'bfloat16'))


def _plan_host_map(env, plan, m, stack, cover):
    """a host loop over the same chips and batches: windows of the reflect-padded stack, normalised as the gather does, ingested, run
    through `plan` (a short last batch as a prefix), the centres added into a zero map on the host"""
    lt, pt = env['lt'], env['pt']
    idx = _indices(pt, cover)
    p = SIDE
    padded = np.pad(stack[:T], ((0, 0), (0, 0), (p, p), (p, p)), mode='reflect')
    out = np.zeros((SH + KERNEL, SW + KERNEL, NCLS), np.float32)
    for s in range(0, len(idx), BATCH):
        part = idx[s:s + BATCH]
        cut = np.stack([padded[:, :, p + y - OFF:p + y - OFF + SIDE, p + x - OFF:p + x - OFF + SIDE] for y, x in part])
        x = (np.moveaxis(cut, 2, 4).astype(np.float64) / MAXVAL).astype(np.float32)
        xt, _ = lt._ingest_seq(torch.from_numpy(x).cuda(), 16, m.dtype_code)
        pred = plan.run(xt)[:len(part)].cpu().numpy()
        for k, (y, x_) in enumerate(part):
            out[y:y + KERNEL, x_:x_ + KERNEL] += pred[k, OFF:OFF + KERNEL, OFF:OFF + KERNEL]
    return out[:SH, :SW]


@pytest.mark.parametrize('cover', ['reference', 'full'])
def test_scene_with_an_unfused_plan_equals_the_default_path(env, scene, cover):
    pt, m = env['pt'], scene['m']
    n = len(_indices(pt, cover))
    assert n > BATCH and n % BATCH != 0                                  # several batches, a short last one
    kw = dict(kernel=KERNEL, buff=BUFF, batch_size=BATCH, channel=None, cover=cover, maxval=MAXVAL)
    want = pt.predict_series_scene(scene['stack'], m, **kw)
    plan = m.inference_plan((BATCH, T, SIDE, SIDE), fused=False)
    got = pt.predict_series_scene(scene['stack'], m, plan=plan, **kw)
    assert np.ptp(want) > 0 and np.array_equal(got, want)
    assert plan.replaying
    assert np.array_equal(pt.predict_series_scene(scene['stack'], m, plan=True, **kw), want)       # (plan=True: unfused by default)
    with pytest.raises(ValueError, match='SeriesInferPlan'):
        pt.predict_series_scene(scene['stack'], m, plan=m.inference_plan((BATCH + 1, T, SIDE, SIDE)), **kw)


@pytest.mark.parametrize('cover', ['reference', 'full'])
def test_scene_with_a_fused_plan_equals_a_host_loop_over_the_same_plan(env, scene, cover):
    pt, m = env['pt'], scene['m']
    plan = m.inference_plan((BATCH, T, SIDE, SIDE), fused=True)
    assert plan.fused_layers == ('conv_lstm', 'dilated_conv_lstm')
    want = _plan_host_map(env, plan, m, scene['stack'], cover)
    got = pt.predict_series_scene(scene['stack'], m, kernel=KERNEL, buff=BUFF, batch_size=BATCH, channel=None, cover=cover, maxval=MAXVAL, plan=plan)
    assert np.ptp(want) > 0 and np.array_equal(got, want)
