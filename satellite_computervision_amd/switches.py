"""The SATCV_* environment variables the Python package reads: ONE table, one row per variable (the library's own switches are the
table of csrc/options.hpp; SATCV_RCCL_LIB is a path read in csrc/comm.hip).  Standard library only: _lib.py imports this module.

`read(key)` parses os.environ NOW with the row's reader; nothing is cached.  `when` says where the package calls it: 'import' = once, into
a module constant (set the variable before the import; tests patch the constant), 'model' = in the model's constructor / builder,
'plan' = when a training plan is built, 'call' = at every call of the function that uses it.  DESIGN.md (appendix "Switches") holds the
same rows; tests/test_switches_cpu.py pins every default and every reading, and holds table, appendix and consumers together.
"""
import os
from collections import namedtuple


# ---- the readers: (variable, default text or None) -> value.  What an odd value means is the READER's business: on('2') is True, only('2') False.
def on(var, default):
    """on unless '0'"""
    return os.environ.get(var, default) != '0'


def only(var, default):
    """on only if '1'"""
    return os.environ.get(var, default) == '1'


def integer(var, default):
    """int(); a word raises ValueError"""
    return int(os.environ.get(var, default))


def int_list(var, default):
    """comma list of ints; empty items are skipped"""
    return tuple(int(v) for v in os.environ.get(var, default).split(',') if v)


def string(var, default):
    return os.environ.get(var, default)


def level012(var, default):
    """'0' -> 0, '2' -> 2, anything else 1 (what `!= '0'` and `== '2'` made of the variable)"""
    return {'0': 0, '2': 2}.get(os.environ.get(var, default), 1)


Row = namedtuple('Row', 'key env default reader when cls meaning')
PROD, OPT_IN, COMPAT, TEST, PROF = 'production', 'opt-in feature', 'compatibility aid', 'test aid', 'profiling aid'

_ROWS = tuple(Row(*r) for r in (
    ('bn_bias_noise', 'SATCV_BN_BIAS_NOISE', '0', only, 'import', COMPAT, "1: the summed (rounding-noise) bias gradient under BatchNorm, as TensorFlow forms it; otherwise the exact zero"),
    ('ctbf', 'SATCV_CTBF', '1', on, 'import', PROD, "the decoder's up-sampling path backward as one launch, csrc/convt_bwd_fused.hip (profiles/r05_ab_convt_bwd_fused.txt)"),
    ('ctbf_couts', 'SATCV_CTBF_COUTS', '32,64', int_list, 'import', PROD, "the Conv2DTranspose filter counts that launch serves"),
    ('fuse_residual', 'SATCV_FUSE_RESIDUAL', '1', only, 'import', PROD, "inference: residual joins written in place by the block's last convolution; off: separate satcv_add_act launches (profiles/r04_deeplab_ab_residual_in_place.txt)"),
    ('fuse_dgrad_bn_bwd', 'SATCV_FUSE_DGRAD_BN_BWD', '1', level012, 'import', PROD, "data-gradient epilogues form the BatchNorm-backward sums of the layer below: 0 none (read again per model), 2 every eligible one (at import; measured slower, profiles/r06_ab_env_switches.txt)"),
    ('wgrad_last_full', 'SATCV_WGRAD_LAST_FULL', '1', on, 'plan', PROD, "the last weight gradient of the step on the whole chip; 0 on the shared workgroup count too"),
    ('deeplab_splitk', 'SATCV_DEEPLAB_SPLITK', '1', only, 'model', PROD, "DeepLab inference plans of one or two tiles set library option splitk to 2 around their launches (profiles/r04_deeplab_ab_splitk_1x1.txt)"),
    ('prefetch', 'SATCV_PREFETCH', '1', on, 'call', PROD, "fit / evaluate: host batches uploaded one batch ahead on a copy stream; 0 on the compute stream"),
    ('fuse_head_bn_bwd', 'SATCV_FUSE_HEAD_BN_BWD', '1', on, 'model', PROD, "the head's backward also does the reduce pass of the last BatchNorm"),
    ('wgrad_stream', 'SATCV_WGRAD_STREAM', '1', on, 'model', PROD, "weight gradients on a second HIP stream; 0 in line (profiles/r03_ab_wgrad_stream.txt)"),
    ('fuse_pool_bn_sums', 'SATCV_FUSE_POOL_BN_SUMS', '1', on, 'model', PROD, "encoder BatchNorm-backward sums formed by the producers of its gradients (profiles/r03_ab_pool_bn_sums.txt)"),
    ('fuse_head_grad', 'SATCV_FUSE_HEAD_GRAD', '1', on, 'model', PROD, "the block under the head forms the head's data gradient in its loader (profiles/r03_ab_head_grad.txt)"),
    ('fuse_pool_bwd', 'SATCV_FUSE_POOL_BWD', '1', on, 'model', PROD, "encoder blocks: pooled BatchNorm apply + weight (+ data) gradient in one launch (profiles/r03_ab_pooled_fused_bwd.txt)"),
    ('fuse_thin_bwd', 'SATCV_FUSE_THIN_BWD', '1', on, 'model', PROD, "thin layers: BatchNorm-backward apply + data + weight gradient in one launch (profiles/r03_ab_fused_thin_bwd.txt)"),
    ('sync_bn', 'SATCV_SYNC_BN', '0', only, 'model', OPT_IN, "data parallel: BatchNorm statistics over all replicas (parallel.py)"),
    ('folded_infer', 'SATCV_FOLDED_INFER', '1', on, 'call', PROD, "bf16 inference on the folded plan; 0 the training-style plan"),
    ('infer_graph', 'SATCV_INFER_GRAPH', '1', integer, 'call', PROD, "hipGraph replay of launch-bound inference plans: 0 never, 2 every plan (profiles/r04_deeplab_ab_graph_splitk.txt)"),
    ('infer_graph_min', 'SATCV_INFER_GRAPH_MIN', '64', integer, 'call', PROD, "the launch count that replay starts at"),
    ('fp8_scaled', 'SATCV_FP8_SCALED', '1', on, 'import', PROD, "fp8 layers whose input channels are a multiple of 64 on the block-scaled K = 64 MFMA (profiles/r03_ab_fp8_plans.txt)"),
    ('fuse_pool', 'SATCV_FUSE_POOL', '1', on, 'import', PROD, "folded plans: max-pool fused into the conv epilogue (profiles/r03_ab_fp8_plans.txt)"),
    ('fp8_hybrid', 'SATCV_FP8_HYBRID', '1', on, 'import', PROD, "fp8 plans keep the full- and half-resolution levels in bf16 (profiles/r03_ab_fp8_plans.txt)"),
    ('fp8_thin', 'SATCV_FP8_THIN', '1', on, 'import', PROD, "fp8 levels: thin 3x3 convolutions on the persistent thin-layer kernel, two-source concatenations (profiles/r03_ab_fp8_plans.txt)"),
    ('siamese_pair', 'SATCV_SIAMESE_PAIR', '1', on, 'import', PROD, "Siamese graphs: the two dates of a shared layer as one launch of 2n images; 0 one launch per date (profiles/siamese_infer_probe.txt)"),
    ('force_collectives', 'SATCV_FORCE_COLLECTIVES', '0', only, 'import', TEST, "collectives at world size 1 too, so that the RCCL path runs on one GPU (tests/test_dp_gpu.py)"),
    ('cabi_comm', 'SATCV_CABI_COMM', '0', only, 'import', OPT_IN, "gradient exchange and SyncBN means on the C-ABI RCCL communicator (no world >= 2 run recorded)"),
    ('grad_payload', 'SATCV_GRAD_PAYLOAD', 'fp32', string, 'call', OPT_IN, "per GradSync: bf16 halves the gradient's wire size (needs SATCV_CABI_COMM=1)"),
    ('overlap_allreduce', 'SATCV_OVERLAP_ALLREDUCE', '1', on, 'call', PROD, "per make_grad_sync: all-reduce in buckets under the backward pass; 0 one all-reduce after it"),
    ('lstm_recurrent_activation', 'SATCV_LSTM_RECURRENT_ACTIVATION', 'hard_sigmoid', string, 'import', COMPAT, "default recurrent activation of the ConvLSTM2D builders (sigmoid: the newer Keras default)"),
    ('lstm_graph', 'SATCV_LSTM_GRAPH', '1', on, 'call', PROD, "ConvLSTM training steps replayed from a captured graph from the third step on; 0 always eager"),
    ('lib', 'SATCV_LIB', None, string, 'import', PROF, "path of an alternative build of the library (ablation variants); unset or empty: libsatcv.so beside the package"),
))
_BY_KEY = {r.key: r for r in _ROWS}


def rows():
    return _ROWS


def read(key):
    r = _BY_KEY[key]
    return r.reader(r.env, r.default)
