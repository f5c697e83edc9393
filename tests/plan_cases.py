"""Small models that between them reach every arm and every fused form of the plan lowering (engine._ForwardLowering, _BackwardLowering,
_SlabSums): shared by tools/plan_manifest.py -- step lists, recorded library calls and result hashes of a plan, compared between two
checkouts -- and by tests/test_model_gpu.py::test_plan_lowering_reaches_its_forms.

A case is Case(name, make, dtype, training, env, early_opt, labels):
  make(mt, lt)  -> (model, x, y): built from a fixed seed; x a batch (a list of batches for two-input models), y its target (None: inference)
  env            SATCV_* variables set while the model and its plan are built (model and plan rows of switches.py)
  early_opt      engine.EARLY_OPT for the case (the tests' way of switching it: tests/test_model_gpu.py)
  labels         label fragments the backward step list of the case must contain
IMPORT_VARIANTS are import rows: they need a process of their own and apply to the five-level bf16 case."""
from collections import namedtuple

import numpy as np

Case = namedtuple('Case', 'name make dtype training env early_opt labels', defaults=(True, {}, False, ()))


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
    Case('unet5_infer', _unet_infer, 'float32', training=False),
    Case('deeplab_infer', _deeplab, 'float32', training=False),
    # the plan / model rows of the switch table and engine.EARLY_OPT, on the five-level bf16 case
    Case(FIVE + '[defer_reduce]', _unet(), 'bfloat16', env={'SATCV_DEFER_REDUCE': '1'}, labels=('wgrad_reduce_batched',)),
    Case(FIVE + '[reduce_stream]', _unet(), 'bfloat16', env={'SATCV_REDUCE_STREAM': '1'}),
    Case(FIVE + '[early_opt]', _unet(), 'bfloat16', early_opt=True, labels=('early optimizer step',)),
    Case(FIVE + '[wgrad_stream=0]', _unet(), 'bfloat16', env={'SATCV_WGRAD_STREAM': '0'}),
    Case(FIVE + '[wgrad_last_full=0]', _unet(), 'bfloat16', env={'SATCV_WGRAD_LAST_FULL': '0'}),
]
IMPORT_VARIANTS = {'wgrad_late': {'SATCV_WGRAD_LATE': '1'}, 'ctbf=0': {'SATCV_CTBF': '0'}, 'bn_bias_noise': {'SATCV_BN_BIAS_NOISE': '1'},
                   'fuse_dgrad_bn_bwd=2': {'SATCV_FUSE_DGRAD_BN_BWD': '2'}}
# every suffix the backward lowering can put on a label: the union over CASES and IMPORT_VARIANTS must hold them all
# the cases whose label fragments no other test of the suite asserts (tests/test_model_gpu.py holds bwd_fused / pooled / +poolsums /
# +skipsums, wgrad_reduce_batched and the early optimizer step; tests/test_bn_numerics_gpu.py the fused +bnred)
IN_SUITE = (FIVE, 'unet3_wide')
SUFFIXES = ('+bnred', '+poolsums', '+skipsums', '(skip half)', '(part)', 'pooled', 'pooled nodx', '+headgrad', 'convt_bwd_fused',
            'wgrad_reduce_batched', 'early optimizer step', 'convT f2')
