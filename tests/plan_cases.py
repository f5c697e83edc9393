"""Small models that between them reach every arm and every fused form of the plan lowering (engine._ForwardLowering, _BackwardLowering):
shared by tools/plan_manifest.py -- step lists, recorded library calls and result hashes of a plan, compared between two
checkouts -- and by tests/test_model_gpu.py::test_plan_lowering_reaches_its_forms.

A case is Case(name, make, dtype, training, env, labels):
  make(mt, lt)  -> (model, x, y): built from a fixed seed; x a batch (a list of batches for two-input models), y its target (None: inference)
  env            SATCV_* variables set while the model and its plan are built (model and plan rows of switches.py)
  labels         label fragments the backward step list of the case must contain
IMPORT_VARIANTS are import rows: they need a process of their own and apply to the five-level bf16 case.

FOLDED_CASES reach every arm of the folded inference lowering (fp8_infer._FoldedLowering) in the same way, for the same tool and for
tests/test_fp8_gpu.py::test_folded_lowering_reaches_its_forms.  A case is FoldedCase(name, make, store, plan_kw, arms):
  make(mt, lt)  -> (model, x): the model carries BatchNorm statistics, gamma, beta and biases drawn from a fixed seed (a freshly
                 initialised model would hide an error in the folding); x a batch, a pair of batches for the Siamese graph
  store          'bf16' | 'fp8' (fp8: the scales come from fp8_infer.calibrate on x)
  plan_kw        hybrid / first_bf16 / pair of fp8_infer.Fp8Plan
  arms           what the case is there to reach (documentation; folded_forms() says what a recorded run did reach)

SERIES_CASES are the inference passes of the ConvLSTM2D family (lstm_tools' tape, lstm_infer's plans), for the same tool (--series):
predict_on_device, an unfused plan eager and replayed, a fused plan -- see the list."""
from collections import Counter, namedtuple

import numpy as np

Case = namedtuple('Case', 'name make dtype training env labels', defaults=(True, {}, ()))


def _xy(rng, n, h, w, ch=4, ncls=2):
    x = rng.random((n, h, w, ch)).astype(np.float32)
    y = np.eye(ncls, dtype=np.float32)[(rng.random((n, h, w)) * ncls * 0.999).astype(np.int64)]
    return x, y


def _cce(mt, m, weights, lr=1e-3):
    m.compile(optimizer=mt.Adam(lr), loss=lambda t, p: mt.weighted_categorical_crossentropy(t, p, weights))
    return m


def _unet(filters=None, factors=None, n=2, hw=64, flags=None, w=None, **kw):
    def make(mt, lt):
        mt.reset_uids(); mt.set_seed(21)
        m = mt.get_unet_model(2, 4, **(dict(filters=filters, factors=factors) if filters else {}), **kw)
        for k in flags or ():
            setattr(m, k, False)
        return (_cce(mt, m, [1.0, 5.0]),) + _xy(np.random.default_rng(12), n, hw, w or hw)
    return make


def _frozen(mt, lt):
    m, x, y = _unet([32, 64], [2, 2], 4, 32)(mt, lt)
    for layer in m.layers[:-1]:
        layer.trainable = False
    return m, x, y


def _zero_gamma(mt, lt):
    m, x, y = _unet([32, 64, 128], [2, 2, 2], 3, 64)(mt, lt)
    w = m.get_weights_dict()
    for k in [k for k in w if k.endswith('/gamma')][::2]:            # every other BatchNorm: raw_bn layers below and above fused launches
        w[k] = np.where(np.arange(w[k].size) % 3 == 0, 0.0, w[k]).astype(np.float32)
    m.set_weights_dict(w)
    return m, x, y


def _siamese(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = mt.make_siamese_unet(4, [32, 64], [2, 2], class_thresh=0.4)
    m.compile(optimizer=mt.Adam(1e-3), loss=lambda t, p: mt.weighted_bce(t, p, 5.0))
    rng = np.random.default_rng(17)
    xa, xb = (rng.random((2, 48, 48, 4)).astype(np.float32) for _ in range(2))
    return m, [xa, xb], (rng.random((2, 48, 48, 1)) < 0.3).astype(np.float32)


def _acnn(second):
    def make(mt, lt):
        mt.reset_uids(); mt.set_seed(9)
        m = mt.get_acnn_model2(3, 4, nfilters=16, depth=3) if second else mt.get_acnn_model(3, 16, 4, 3)
        return (_cce(mt, m, [1.0, 2.0, 3.0]),) + _xy(np.random.default_rng(23), 2, 40, 36, ncls=3)
    return make


def _aspp(mt, lt):
    mt.reset_uids(); mt.set_seed(2)
    inp = mt.Input([None, None, 4])
    pooled, enc = mt.encoder_block(32, name='encoder_0')(inp)
    d = mt.decoder_block(mt.DilatedSpatialPyramidPooling(64)(pooled), enc, 32)
    probs = mt._Head(2, 'softmax', None, 'probs')(d)
    m = mt.Model(inp, [probs, mt._classes(probs, 'classes')])
    return (_cce(mt, m, [1.0, 3.0]),) + _xy(np.random.default_rng(5), 2, 32, 32)


def _hybrid(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = lt.get_hybrid_model((48, 48, 4), (3, 8, 8, 6), 3, filters=[32, 64], factors=[3, 2], compile_model=True, optim=mt.Adam(1e-3),
                            loss=lambda t, p: mt.weighted_categorical_crossentropy(t, p, [1.0, 1.0, 1.0]))
    rng = np.random.default_rng(2)
    xu, y = _xy(rng, 2, 48, 48, ncls=3)
    return m, [xu, rng.random((2, 3, 8, 8, 6)).astype(np.float32)], y


# the tape models (no engine plan: the manifest holds their calls, losses and weights), at the hybrid case's scale
def _lstm(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = lt.get_lstm_model(6, 3, 3, optim=mt.Adam(1e-3), loss=mt.mse_4d)
    rng = np.random.default_rng(2)
    return m, rng.random((2, 3, 8, 8, 6)).astype(np.float32), rng.random((2, 8, 8, 3)).astype(np.float32)


def _lstm_autoencoder(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = lt.get_lstm_autoencoder(6, 3, 6, compile=True, optim=mt.Adam(1e-3), loss=mt.mse_4d)
    rng = np.random.default_rng(2)
    x = rng.random((2, 3, 8, 8, 6)).astype(np.float32)
    return m, [x, rng.random((2, 8, 8, 2)).astype(np.float32)], [np.flip(x, axis=1).copy(), rng.random((2, 8, 8, 6)).astype(np.float32)]


def _hierarchical(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = lt.get_hierarchical_model(3, 4, 5, (24, 24, 4), (3, 8, 8, 6), 16, 3)
    m.compile(optimizer=mt.Adam(1e-3), loss=lambda t, p: mt.weighted_categorical_crossentropy(t, p, [1.0] * 5))
    rng = np.random.default_rng(2)
    ys = [np.eye(k, dtype=np.float32)[rng.integers(0, k, (2, 24, 24))] for k in (5, 4, 3)]
    return m, [rng.random((2, 24, 24, 4)).astype(np.float32), rng.random((2, 3, 8, 8, 6)).astype(np.float32)], ys


def _deeplab(mt, lt):
    mt.reset_uids(); mt.set_seed(7)
    return mt.get_deeplabv3_model(3, 4), np.random.default_rng(8).random((1, 64, 64, 4)).astype(np.float32), None


def _unet_infer(mt, lt):
    m, x, _ = _unet(n=1)(mt, lt)
    return m, x, None


FUSE_FLAGS = ('fuse_thin_bwd', 'fuse_pool_bwd', 'fuse_pool_bn_sums', 'fuse_dgrad_bn_bwd', 'fuse_head_bn_bwd')
FIVE = 'unet5_bf16'
CASES = [
    Case(FIVE, _unet(), 'bfloat16', labels=('+bnred', '+poolsums', '+skipsums', '(part)', 'pooled', 'pooled nodx', '+headgrad', 'convT f2')),
    Case('unet5_fp32', _unet(), 'float32', labels=('convT f2',)),
    # (the fused transposed-conv backward needs input rows of a multiple of its pixel tile -- 64 pixels for 32 filters, 32 for 64: `w_ % PX`
    #  in csrc/convt_bwd_fused.hip -- which a 64 x 64 input does not give it: one case of 128-pixel rows)
    Case('unet3_wide', _unet([32, 64, 128], [2, 2, 2], 1, 32, w=128), 'bfloat16', labels=('(skip half)', 'convt_bwd_fused')),
    Case('unet3_unfused', _unet([32, 64, 128], [2, 2, 2], 3, 64, FUSE_FLAGS), 'bfloat16'),
    Case('unet_dropout', _unet([32, 64], [2, 2], 2, 32, dropout=0.25), 'bfloat16'),
    Case('siamese', _siamese, 'bfloat16'),
    Case('acnn', _acnn(False), 'bfloat16'),
    Case('acnn2', _acnn(True), 'bfloat16'),
    Case('aspp', _aspp, 'bfloat16'),
    Case('frozen', _frozen, 'bfloat16'),
    Case('zero_gamma', _zero_gamma, 'bfloat16'),
    Case('unet16', _unet([16, 32], [2, 2], 2, 32), 'bfloat16'),
    Case('hybrid', _hybrid, 'float32'),
    Case('lstm', _lstm, 'float32'),
    Case('lstm_autoencoder', _lstm_autoencoder, 'float32'),
    Case('hierarchical', _hierarchical, 'float32'),
    Case('unet5_infer', _unet_infer, 'float32', training=False),
    Case('deeplab_infer', _deeplab, 'float32', training=False),
    # the plan / model rows of the switch table, on the five-level bf16 case
    Case(FIVE + '[wgrad_stream=0]', _unet(), 'bfloat16', env={'SATCV_WGRAD_STREAM': '0'}),
    Case(FIVE + '[wgrad_last_full=0]', _unet(), 'bfloat16', env={'SATCV_WGRAD_LAST_FULL': '0'}),
]
IMPORT_VARIANTS = {'ctbf=0': {'SATCV_CTBF': '0'}, 'bn_bias_noise': {'SATCV_BN_BIAS_NOISE': '1'}, 'fuse_dgrad_bn_bwd=2': {'SATCV_FUSE_DGRAD_BN_BWD': '2'}}
# every suffix the backward lowering can put on a label: the union over CASES and IMPORT_VARIANTS must hold them all
# the cases whose label fragments no other test of the suite asserts (tests/test_model_gpu.py holds bwd_fused / pooled / +poolsums /
# +skipsums; tests/test_bn_numerics_gpu.py the fused +bnred)
IN_SUITE = (FIVE, 'unet3_wide')
SUFFIXES = ('+bnred', '+poolsums', '+skipsums', '(skip half)', '(part)', 'pooled', 'pooled nodx', '+headgrad', 'convt_bwd_fused', 'convT f2')


# ------------------------------------------------------------------ folded inference (fp8_infer.Fp8Plan)
FoldedCase = namedtuple('FoldedCase', 'name make store plan_kw arms')


def _trained_look(m, seed):
    """non-trivial moving statistics, gamma, beta and biases (kernels as initialised) through set_weights_dict"""
    rng = np.random.default_rng(seed)
    w = m.get_weights_dict()
    for k in w:
        if k.endswith('moving_mean') or k.endswith('/bias') or k.endswith('/beta'):
            w[k] = (0.2 * rng.standard_normal(w[k].shape)).astype(np.float32)
        elif k.endswith('moving_var') or k.endswith('/gamma'):
            w[k] = (0.5 + rng.random(w[k].shape)).astype(np.float32)
    m.set_weights_dict(w)
    return m


def _f_unet(n, h, w, **kw):
    def make(mt, lt):
        mt.reset_uids(); mt.set_seed(6)
        m = mt.get_unet_model(2, 4, filters=[32, 64, 128], factors=[2, 2, 2], **kw)
        return _trained_look(m, 3), np.random.default_rng(31).random((n, h, w, 4)).astype(np.float32)
    return make


def _f_hybrid_branch(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = lt.get_hybrid_model((48, 48, 4), (3, 8, 8, 6), 3, filters=[32, 64], factors=[3, 2])
    return _trained_look(m.unet, 5), np.random.default_rng(32).random((2, 48, 48, 4)).astype(np.float32)


def _f_siamese(mt, lt):
    mt.reset_uids(); mt.set_seed(4)
    m = _trained_look(mt.make_siamese_unet(4, [32, 64], [2, 2], class_thresh=0.4), 17)
    rng = np.random.default_rng(33)
    return m, [rng.random((3, 64, 64, 4)).astype(np.float32) for _ in range(2)]


def _f_two_date_extras(mt, lt):
    """A two-date graph from the package's own blocks with what make_siamese_unet lacks: a shared level that is no skip and whose
    max-pool cannot fuse (factor 3: no kernel tile holds whole 3 x 3 windows), SpatialDropout2D on the two-date part, and an ASPP on
    8 x 8 maps (dilation 12 reads only padding off the centre tap).  The head works at a third of the input resolution."""
    from satellite_computervision_amd import engine as E
    mt.reset_uids(); mt.set_seed(11)
    ia, ib = mt.Input((None, None, 4)), mt.Input((None, None, 4))
    stem, enc, aspp = mt.encoder_block(32, pool_size=(3, 3), name='stem'), mt.encoder_block(64, name='encoder_0'), mt.DilatedSpatialPyramidPooling(128)
    pooled, skips = [], []
    for x in (ia, ib):
        p, _ = stem(x)
        p, e = enc(mt._dropout(p, 0.25, True))
        pooled.append(aspp(p)); skips.append(e)

    def cat(a, b):
        return E.Node('concat', [b, a]).out(a.channels + b.channels, a.down)
    dec = mt.decoder_block(cat(*pooled), cat(*skips), 64)
    probs = mt._Head(1, 'sigmoid', None, 'probs')(dec)
    m = _trained_look(mt.Model(inputs=[ia, ib], outputs=[probs, mt._classes(probs, 'classes', thresh=0.5)]), 19)
    rng = np.random.default_rng(34)
    return m, [rng.random((2, 48, 48, 4)).astype(np.float32) for _ in range(2)]


def _f_siamese32(mt, lt):
    m, _ = _f_siamese(mt, lt)
    rng = np.random.default_rng(35)
    return m, [rng.random((2, 32, 32, 4)).astype(np.float32) for _ in range(2)]


_ALL8 = dict(hybrid=False)
FOLDED_CASES = [
    FoldedCase('unet3 bf16', _f_unet(2, 64, 64), 'bf16', {}, 'input (bf16 bands), cba with fused pool, two-source cba, convT to its own tensor, head, classes'),
    FoldedCase('unet3 fp8 hybrid', _f_unet(2, 64, 64), 'fp8', {}, 'pooled map quantised at the boundary, convT input de-quantised, block-scaled deep layers'),
    FoldedCase('unet3 fp8', _f_unet(2, 64, 64), 'fp8', _ALL8, 'cba behind bf16 bands (conv + requant), thin fp8 layers, two-source fp8 read'),
    FoldedCase('unet3 fp8 scaled-ingest', _f_unet(2, 64, 64), 'fp8', dict(hybrid=False, first_bf16=False), 'input (scaled e4m3 ingest)'),
    FoldedCase('unet3 fp8 first-bf16', _f_unet(2, 64, 64), 'fp8', dict(hybrid=False, first_bf16=True), 'the same plan as "unet3 fp8", first_bf16 given'),
    FoldedCase('unet3 24x40 fp8', _f_unet(3, 24, 40), 'fp8', _ALL8, 'separate max-pool (fp8), materialised concatenation (skip half re-quantised)'),
    FoldedCase('hybrid-branch bf16', _f_hybrid_branch, 'bf16', {}, 'separate max-pool (factor 3, bf16), linear head without a classes node'),
    FoldedCase('hybrid-branch fp8', _f_hybrid_branch, 'fp8', {}, 'separate max-pool whose pooled map is quantised at the boundary'),
    FoldedCase('unet3 dropout bf16', _f_unet(2, 64, 64, dropout=0.25), 'bf16', {}, 'dropout (identity)'),
    FoldedCase('unet3 dropout fp8', _f_unet(2, 64, 64, dropout=0.25), 'fp8', {}, 'dropout behind a boundary tensor'),
    FoldedCase('siamese bf16 paired', _f_siamese, 'bf16', dict(pair=True), 'two-date input / cba / pool / concat, pair store, ASPP slot tensor, pair concatenation'),
    FoldedCase('siamese bf16 unpaired', _f_siamese, 'bf16', dict(pair=False), 'one launch per date into the concatenation'),
    FoldedCase('siamese fp8 paired', _f_siamese, 'fp8', dict(pair=True), 'pair store in e4m3, group scales, dilated plain-e4m3 packing'),
    FoldedCase('siamese fp8 unpaired', _f_siamese, 'fp8', dict(pair=False), 'one launch per date in e4m3'),
    FoldedCase('siamese 32x32 fp8 paired', _f_siamese32, 'fp8', dict(pair=True), 'centre-tap cut of the dilation-12 branch on 8 x 8 maps, in e4m3'),
    FoldedCase('two-date extras bf16', _f_two_date_extras, 'bf16', dict(pair=True), 'two-date dropout, two-date separate max-pool (2n images), centre-tap cut'),
]
FOLDED_IN_SUITE = ('siamese bf16 paired', 'siamese bf16 unpaired', 'unet3 fp8 hybrid', 'hybrid-branch bf16')


# ------------------------------------------------------------------ inference of the ConvLSTM2D family (lstm_tools, lstm_infer)
SeriesCase = namedtuple('SeriesCase', 'name make dtype')


def randomise(m, seed):
    """non-trivial BatchNorm statistics and biases of a tape model; the kernels keep their initialisers"""
    rng = np.random.default_rng(seed)
    w = {}
    for k, v in m.get_weights_dict().items():
        if k.endswith('/moving_var'):
            w[k] = (0.5 + rng.random(v.shape)).astype(np.float32)
        elif k.endswith('/gamma'):
            w[k] = (1 + 0.2 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith(('/beta', '/moving_mean')):
            w[k] = (0.2 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith('/bias'):
            w[k] = (v + 0.1 * rng.standard_normal(v.shape)).astype(np.float32)
    m.set_weights_dict(w)
    return m


def _ingested(lt, m, x):
    import torch
    return lt._ingest_seq(torch.from_numpy(x).cuda(), (m.n_channels + 15) // 16 * 16, m.dtype_code)


def _plan_passes(run):
    """the first run of a plan (eager) and its third (the second captures, the third replays), recorded; the second not"""
    return [('plan, run 1 (eager)', run), (None, run), ('plan, run 3 (replayed)', run)]


def _s_series(autoencoder):
    """get_lstm_model(6, 3, 3) / get_lstm_autoencoder(2, 2, 1) at B = 3, 16 x 16, the shapes of tests/test_series_plan_gpu.py: T = 3 is the
    smallest length at which the plan's two-slot c ring is reused (step 2 writes slot 0 again) and a step has both neighbours"""
    def make(mt, lt):
        import torch
        mt.set_seed(9 if autoencoder else 7)
        m = randomise(lt.get_lstm_autoencoder(2, 2, 1) if autoencoder else lt.get_lstm_model(6, 3, 3), 9 if autoencoder else 7)
        rng = np.random.default_rng(1)
        x, shape = _ingested(lt, m, rng.random((3, m.n_time, 16, 16, m.n_channels)).astype(np.float32))
        if autoencoder:
            x = [x, torch.from_numpy(rng.standard_normal((3, 16, 16, 2)).astype(np.float32)).cuda()]
        plan = m.inference_plan(shape, fused=False)
        return m, ([('predict_on_device', lambda: m.predict_on_device(x, shape=shape))] + _plan_passes(lambda: plan.run(x)) +
                   [('fused plan, run 1', lambda: m.inference_plan(shape, fused=True).run(x))])
    return make


def _s_hybrid(mt, lt):
    """the hybrid case above: predict_on_device, scene_plan(2, 48, 8) unfused, and that plan on ONE chip (the prefix staging)"""
    import torch
    m, (xu, xl), _ = _hybrid(mt, lt)
    randomise(m, 4)
    xu = torch.from_numpy(xu).cuda()
    (xt, shape), (xt1, _) = _ingested(lt, m, xl), _ingested(lt, m, xl[:1])
    plan = m.scene_plan(2, 48, 8)
    return m, ([('predict_on_device', lambda: m.predict_on_device([xu, xt], shape=shape, want_classes=True))] +
               _plan_passes(lambda: plan.run(xu, xt, want_classes=True)) + [('plan, 1 chip (prefix)', lambda: plan.run(xu[:1], xt1, want_classes=True))])


def _s_hierarchical(mt, lt):
    import torch
    m, (xa, xl), _ = _hierarchical(mt, lt)
    randomise(m, 4)
    xa = torch.from_numpy(xa).cuda()
    xt, shape = _ingested(lt, m, xl)
    return m, [(f'predict_on_device {o}', lambda o=o: m.predict_on_device([xa, xt], shape=shape, output=o)) for o in m.output_names]


# make(mt, lt) -> (model, [(label, pass)]) under the case's compute dtype: every pass returns a tensor or a tuple of tensors; the passes
# with a label are recorded (tools/plan_manifest.py --series: their library calls and output hashes), one with None only runs
SERIES_CASES = [
    SeriesCase('lstm_model fp32', _s_series(False), 'float32'),
    SeriesCase('lstm_model bf16', _s_series(False), 'bfloat16'),
    SeriesCase('lstm_autoencoder bf16', _s_series(True), 'bfloat16'),
    SeriesCase('hybrid', _s_hybrid, 'bfloat16'),
    SeriesCase('hierarchical', _s_hierarchical, 'float32'),
]


def folded_forms(calls):
    """Counter of the forms the recorded calls of one Fp8Plan.run_forward took (calls: tools/plan_manifest.py's Recorder)"""
    from satellite_computervision_amd._lib import BF16, FP8
    code = {BF16: 'bf16', FP8: 'fp8'}
    forms = Counter()
    for name, _, structs, scalars in calls:
        if name == 'satcv_conv2d_igemm':
            d = structs[0]
            forms['convT' if d['mode_out'] == 1 else 'conv'] += 1
            forms['conv, pair store over 2n images'] += bool(d['pair_n'] and d['n'] == 2 * d['pair_n'])
            forms['conv, fused pool'] += bool(d['pool_f'])
            forms['conv, two sources'] += bool(d['c1'])
            forms['conv, raw output'] += not d['out_relu']
        elif name == 'satcv_maxpool':
            forms['separate maxpool'] += 1
        elif name == 'satcv_affine_requant':
            ld_src, relu, ld_dst, npix, c, dt_in, dt_out = scalars
            forms[f'requant {code[dt_in]} -> {code[dt_out]}' + (', BN + ReLU' if relu else '') + (' into a concatenation' if ld_dst != c else '')] += 1
        else:
            forms[name[len('satcv_'):]] += 1
    return +forms
