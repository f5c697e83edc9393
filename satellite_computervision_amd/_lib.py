"""ctypes binding of libsatcv.so (the C-ABI HIP library, include/satcv.h).

The product path has NO fallback: if the shared library is missing or a symbol
declared in include/satcv.h is absent, import fails loudly.
"""
import ctypes as C
import os

# The library takes device pointers and streams from torch, so both must sit on ONE HIP runtime:
# import torch first (it loads its bundled libamdhip64) so that libsatcv.so binds to that copy.
import torch  # noqa: F401

from . import switches

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = switches.read('lib') or os.path.join(_HERE, 'libsatcv.so')

F32, BF16, FP8, FP8X, F64 = 0, 1, 2, 3, 4
STAT_ROWS = 32
COMPOSITE_MAX_T = 256       # SATCV_COMPOSITE_MAX_T of include/satcv.h

c_i32, c_i64, c_f32, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class ConvDesc(C.Structure):
    _fields_ = [('x0', c_vp), ('x1', c_vp), ('c0', c_i32), ('c1', c_i32),
                ('in_scale', c_vp), ('in_shift', c_vp), ('in_relu', c_i32),
                ('w', c_vp), ('bias', c_vp), ('y', c_vp), ('ldy', c_i32),
                ('stats', c_vp), ('stats_ld', c_i32),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32),
                ('cout', c_i32), ('cout_pad', c_i32),
                ('kh', c_i32), ('kw', c_i32), ('dil', c_i32),
                ('mode_in', c_i32), ('mode_out', c_i32), ('f', c_i32),
                ('cstat', c_i32), ('out_relu', c_i32), ('dtype', c_i32), ('accumulate', c_i32),
                ('stride', c_i32), ('hin', c_i32), ('win', c_i32), ('out_scale', c_vp), ('pool_y', c_vp), ('pool_ld', c_i32), ('pool_f', c_i32),
                ('bst_y', c_vp), ('bst_y1', c_vp), ('bst_ld', c_i32), ('bst_ld1', c_i32), ('bst_split', c_i32),
                ('bst_scale', c_vp), ('bst_shift', c_vp), ('bst_mean', c_vp), ('bst_rstd', c_vp), ('bst_relu', c_i32), ('tile_policy', c_i32),
                ('pair_n', c_i32), ('pair_c0', c_i32), ('pair_c1', c_i32)]


class PackJob(C.Structure):
    _fields_ = [('src', c_vp), ('dst', c_vp), ('mode', c_i32), ('taps', c_i32), ('cin', c_i32), ('cout', c_i32), ('kpad', c_i32), ('npad', c_i32)]


class TileDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('n', c_i32), ('c', c_i32), ('hin', c_i32), ('win', c_i32), ('h', c_i32), ('w_', c_i32),
                ('rescale', C.c_double), ('nan_mask', c_i32), ('replace', c_i32), ('seed', C.c_uint64), ('ch_mean', c_vp),
                ('contra_mul', C.c_double), ('bright_mul', C.c_double), ('flip_v', c_i32), ('flip_h', c_i32), ('rot', c_i32),
                ('dst', c_vp), ('ldc', c_i32), ('coff', c_i32)]


class SceneGatherDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('h', c_i32), ('w_', c_i32), ('c', c_i32), ('rescale', C.c_double),
                ('origins', c_vp), ('total', c_i32), ('first', c_i32), ('n', c_i32), ('off', c_i32), ('side', c_i32),
                ('dst', c_vp), ('ldc', c_i32), ('coff', c_i32)]


class SceneScatterDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('n', c_i32), ('sh', c_i32), ('sw', c_i32), ('lds', c_i32), ('c0', c_i32), ('nc', c_i32),
                ('crop_y', c_i32), ('crop_x', c_i32), ('crop_h', c_i32), ('crop_w', c_i32),
                ('origins', c_vp), ('total', c_i32), ('first', c_i32), ('dst', c_vp), ('dst_kind', c_i32),
                ('h', c_i32), ('w_', c_i32), ('ldd', c_i32), ('doff', c_i32), ('accumulate', c_i32)]


class SeriesGatherDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('t', c_i32), ('c', c_i32), ('h', c_i32), ('w_', c_i32), ('steps', c_i32),
                ('maxval', C.c_double), ('origins', c_vp), ('total', c_i32), ('first', c_i32), ('n', c_i32), ('off', c_i32), ('side', c_i32),
                ('dst', c_vp), ('dtype', c_i32), ('cpad', c_i32)]


class CompositeDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('t', c_i32), ('c', c_i32), ('h', c_i32), ('w_', c_i32), ('offsets', c_vp),
                ('median', c_vp), ('ld_med', c_i32), ('coff_med', c_i32), ('norm', c_vp), ('ld_norm', c_i32), ('coff_norm', c_i32),
                ('use_fill', c_i32), ('fill', c_f32)]


Q_QA60, Q_CLOUD, Q_SHADOW, Q_WATER, Q_SCL = 1, 2, 4, 8, 16     # SATCV_Q_* of include/satcv.h
Q_ROLES = ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60', 'SCL')      # the order of satcv_quality_desc.band


class QualityDesc(C.Structure):
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('t', c_i32), ('cs', c_i32), ('h', c_i32), ('w_', c_i32), ('offsets', c_vp),
                ('band', c_i32 * len(Q_ROLES)), ('rules', c_i32), ('cloud_max', c_i32), ('shadow_min', c_f32),
                ('clear', c_vp), ('cloud_score', c_vp), ('water_score', c_vp)]


class CompositeMaskedDesc(C.Structure):
    _fields_ = [('base', CompositeDesc), ('clear', c_vp), ('cs', c_i32), ('band_idx', c_i32 * 16)]


class RasterDesc(C.Structure):
    """satcv_raster_desc: one descriptor for satcv_raster_convert / _overview / _tiles"""
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('h', c_i32), ('w_', c_i32), ('c', c_i32), ('ld', c_i32), ('coff', c_i32),
                ('dst', c_vp), ('dst_kind', c_i32), ('scale', c_f32), ('has_nodata', c_i32), ('nodata', C.c_double),
                ('resampling', c_i32), ('blocksize', c_i32), ('predictor', c_i32)]


class UntileDesc(C.Structure):
    """satcv_untile_desc: decoded blocks -> a window of a resident raster (satcv_raster_untile)"""
    _fields_ = [('src', c_vp), ('src_stride', c_i64), ('blocks', c_vp), ('nblocks', c_i32), ('bh', c_i32), ('bw', c_i32), ('across', c_i32),
                ('per_plane', c_i32), ('spp', c_i32), ('planar', c_i32), ('kind', c_i32), ('predictor', c_i32), ('row0', c_i32), ('col0', c_i32),
                ('h', c_i32), ('w_', c_i32), ('dst', c_vp), ('layout', c_i32), ('ld', c_i32), ('coff', c_i32), ('band_map', c_i32 * 16)]


class WarpDesc(C.Structure):
    """satcv_warp_desc: a resident raster resampled onto another grid of the same CRS (satcv_raster_warp)"""
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('src_layout', c_i32), ('sh', c_i32), ('sw', c_i32), ('src_ld', c_i32), ('src_coff', c_i32),
                ('src_row0', c_i32), ('src_col0', c_i32), ('dst', c_vp), ('dst_kind', c_i32), ('dst_layout', c_i32), ('dh', c_i32), ('dw', c_i32),
                ('dst_ld', c_i32), ('dst_coff', c_i32), ('dst_row0', c_i32), ('dst_col0', c_i32), ('c', c_i32), ('su', C.c_double), ('ou', C.c_double),
                ('sv', C.c_double), ('ov', C.c_double), ('resampling', c_i32), ('has_src_nodata', c_i32), ('src_nodata', C.c_double),
                ('has_dst_nodata', c_i32), ('dst_nodata', C.c_double), ('keep', c_i32)]


class Crs(C.Structure):
    """satcv_crs: kind 0 geographic, 1 transverse Mercator, 2 spherical Mercator; ellipsoid, central meridian, scale, false origin"""
    _fields_ = [('kind', c_i32), ('a', C.c_double), ('inv_f', C.c_double), ('lon0', C.c_double), ('k0', C.c_double), ('fe', C.c_double), ('fn', C.c_double)]


class ReprojectMap(C.Structure):
    """satcv_reproject_map: destination CRS and transform (a, c, e, f), source CRS and, with has_src_transform, its transform"""
    _fields_ = [('dst_crs', Crs), ('dst_a', C.c_double), ('dst_c', C.c_double), ('dst_e', C.c_double), ('dst_f', C.c_double), ('src_crs', Crs),
                ('has_src_transform', c_i32), ('src_a', C.c_double), ('src_c', C.c_double), ('src_e', C.c_double), ('src_f', C.c_double)]


class CalibApplyDesc(C.Structure):
    """satcv_calib_apply_desc: a (c, h, w_) raster through a per-band table into a planar or pixel-interleaved destination"""
    _fields_ = [('src', c_vp), ('src_kind', c_i32), ('c', c_i32), ('h', c_i32), ('w_', c_i32), ('has_nodata', c_i32), ('nodata', C.c_double),
                ('table', c_vp), ('dst', c_vp), ('dst_kind', c_i32), ('dst_layout', c_i32), ('dst_ld', c_i32), ('dst_coff', c_i32), ('keep', c_i32)]


class RasterizeDesc(C.Structure):
    """satcv_rasterize_desc: an edge table (host pointers) burned into a mask or a label raster (satcv_rasterize)"""
    _fields_ = [('edges', c_vp), ('n_items', c_i64), ('row_start', c_vp), ('h', c_i32), ('w_', c_i32), ('n_geoms', c_i32), ('mode', c_i32), ('invert', c_i32),
                ('values', c_vp), ('fill', C.c_double), ('dst', c_vp), ('dst_kind', c_i32), ('dst_layout', c_i32), ('dst_ld', c_i32), ('dst_coff', c_i32),
                ('keep', c_i32), ('on_device', c_i32), ('workspace', c_vp), ('workspace_bytes', c_i64)]


class MaskApplyDesc(C.Structure):
    """satcv_mask_apply_desc: one uint8 (h, w_) mask applied to the channels coff ... coff + c - 1 of a raster or a stack"""
    _fields_ = [('mask', c_vp), ('h', c_i32), ('w_', c_i32), ('invert', c_i32), ('src', c_vp), ('dst', c_vp), ('kind', c_i32), ('layout', c_i32),
                ('c', c_i32), ('ld', c_i32), ('coff', c_i32), ('has_nodata', c_i32), ('nodata', C.c_double)]


RECORD_MAX_PLANES = 32     # SATCV_RECORD_MAX_PLANES of include/satcv.h
RECORD_STAT_SPLITS = 16    # SATCV_RECORD_STAT_SPLITS
_i32p, _f32p = c_i32 * RECORD_MAX_PLANES, c_f32 * RECORD_MAX_PLANES


class RecordDesc(C.Structure):
    _fields_ = [('src', c_vp), ('n', c_i32), ('k', c_i32), ('h', c_i32), ('w_', c_i32), ('kind', _i32p), ('depth', _i32p),
                ('params', c_vp), ('ld_params', c_i32), ('color', c_i32), ('morph', c_i32), ('mode', c_i32), ('stat_src', c_i32),
                ('ngroups', c_i32), ('gstart', _i32p), ('glen', _i32p), ('mom_a', _f32p), ('mom_b', _f32p), ('eps', c_f32),
                ('stats', c_vp), ('stats_ws', c_vp), ('stats_ws_bytes', c_i64), ('mean_in', c_vp),
                ('x', c_vp), ('ld_x', c_i32), ('coff_x', c_i32), ('y', c_vp), ('ld_y', c_i32), ('coff_y', c_i32)]


class WgradDesc(C.Structure):
    _fields_ = [('x0', c_vp), ('x1', c_vp), ('c0', c_i32), ('c1', c_i32),
                ('in_scale', c_vp), ('in_shift', c_vp), ('in_relu', c_i32),
                ('dy', c_vp), ('lddy', c_i32), ('dw', c_vp),
                ('cin', c_i32), ('cout', c_i32),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32),
                ('kh', c_i32), ('kw', c_i32), ('dil', c_i32),
                ('mode_dy', c_i32), ('f', c_i32), ('transposed', c_i32),
                ('workspace', c_vp), ('workspace_bytes', c_i64), ('dtype', c_i32), ('accumulate', c_i32), ('whole_chip', c_i32), ('defer_reduce', c_i32)]


class WgradPlanInfo(C.Structure):
    """satcv_wgrad_plan_info: the kernel form satcv_conv2d_wgrad would run (host-only query, nothing is launched)."""
    _fields_ = [(k, c_i32) for k in ('kernel', 'tw', 'nci', 'nco', 'nw', 'nks', 'ntaps', 'pix', 'db', 'dma', 'm16',
                                     'nsplit', 'kpad', 'npad', 'n_ci_blk', 'n_co_blk', 'reduce', 'per_tap')] + \
               [('ws_bytes', c_i64), ('lds_bytes', c_i64)]


WGRAD_KERNELS = ('single', 'db', 'dma')              # SATCV_WGRAD_KERNEL_*
WGRAD_REDUCES = ('generic', 'reduce4', 'reduce16')   # SATCV_WGRAD_REDUCE_*


class ConvPlanInfo(C.Structure):
    """satcv_conv_plan_info: the kernel form satcv_conv2d_igemm would run (host-only query, nothing is launched)."""
    _fields_ = [(k, c_i32) for k in ('family', 'dtype', 'tw', 'wm', 'wn', 'mt', 'nt', 'ks', 'taps', 'tl', 'db', 'wps', 'wdma', 'sk', 'm16', 'dyn',
                                     'cin', 'cout', 'th', 'nw', 'nsplit', 'dil', 'bn', 'roles', 'bst',
                                     'imgs', 'rpi', 'tiles_x', 'tiles_y', 'n_tiles', 'nchunks', 'ksplit', 'centre_tap')] + \
               [('workgroups', c_i64), ('lds_bytes', c_i64)]


CONV_FAMILIES = ('generic', 'fast', 'm16', 'm16p', 'ws', 'tr', 'convt_thin', 'convt_thin_dgrad')      # SATCV_CONV_FAMILY_*
# the fields of ConvPlanInfo that name the instantiation of each family (its template arguments)
CONV_KEY_FIELDS = {'generic': ('tw', 'wm', 'wn', 'mt', 'nt', 'ks'),
                   'fast': ('tw', 'wm', 'wn', 'mt', 'nt', 'ks', 'taps', 'tl', 'db', 'wps', 'wdma', 'sk', 'm16', 'dyn'),
                   'm16': ('tw', 'roles', 'bst'), 'm16p': ('bn', 'bst'),
                   'ws': ('cin', 'nt', 'wps', 'wn', 'dil'), 'tr': ('cin', 'cout', 'th'),
                   'convt_thin': ('cin', 'cout', 'nw', 'wps', 'nsplit'), 'convt_thin_dgrad': ('cin', 'cout', 'nw', 'wps')}


class BwdfDesc(C.Structure):
    _fields_ = [('g', c_vp), ('yraw', c_vp), ('ldg', c_i32),
                ('bn_scale', c_vp), ('bn_shift', c_vp), ('bn_mean', c_vp), ('bn_rstd', c_vp), ('bn_coef', c_vp), ('linear', c_i32),
                ('x0', c_vp), ('x1', c_vp), ('c0', c_i32), ('c1', c_i32),
                ('in_scale', c_vp), ('in_shift', c_vp), ('in_relu', c_i32),
                ('w_dgrad', c_vp), ('dx', c_vp), ('lddx', c_i32),
                ('dw', c_vp), ('cin', c_i32), ('cout', c_i32),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32), ('kh', c_i32), ('kw', c_i32), ('dil', c_i32),
                ('workspace', c_vp), ('workspace_bytes', c_i64), ('dtype', c_i32), ('accumulate', c_i32),
                ('bst_sums', c_vp), ('bst_sums_ld', c_i32), ('bst_mean', c_vp), ('bst_rstd', c_vp), ('bst_act_form', c_i32),
                ('dpool', c_vp), ('lddp', c_i32), ('amax', c_vp),
                ('hg_dlogits', c_vp), ('hg_w', c_vp), ('hg_ncls', c_i32), ('defer_reduce', c_i32)]


class CtbfDesc(C.Structure):
    _fields_ = [('g', c_vp), ('ldg', c_i32), ('yup', c_vp), ('ldy', c_i32),
                ('bn_scale', c_vp), ('bn_shift', c_vp), ('bn_mean', c_vp), ('bn_rstd', c_vp), ('bn_c1', c_vp), ('bn_c2', c_vp), ('linear', c_i32),
                ('x', c_vp), ('ldx', c_i32), ('in_scale', c_vp), ('in_shift', c_vp), ('in_relu', c_i32),
                ('w_dgrad', c_vp), ('w_npad', c_i32), ('dx', c_vp), ('lddx', c_i32), ('dw', c_vp), ('cin', c_i32), ('cout', c_i32),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32), ('f', c_i32), ('workspace', c_vp), ('workspace_bytes', c_i64),
                ('dtype', c_i32), ('accumulate', c_i32), ('defer_reduce', c_i32),
                ('bst_sums', c_vp), ('bst_sums_ld', c_i32), ('bst_mean', c_vp), ('bst_rstd', c_vp)]


class BwdfPlanInfo(C.Structure):
    """satcv_bwdf_plan_info: the instantiation satcv_conv2d_bwd_fused would run and its tile ranges (host-only query, nothing is launched)."""
    _fields_ = [(k, c_i32) for k in ('cin', 'cout', 'nw', 'wps', 'pool', 'nodg', 'cins', 'hg', 'bst', 'pad_')] + \
               [(k, c_i64) for k in ('tiles', 'workgroups', 'tiles_min', 'tiles_max', 'lds_bytes', 'ws_bytes')]


class CtbfPlanInfo(C.Structure):
    """satcv_ctbf_plan_info: the same for satcv_convt_bwd_fused."""
    _fields_ = [(k, c_i32) for k in ('cout4', 'px', 'cblk', 'nblk')] + \
               [(k, c_i64) for k in ('slabs', 'tiles', 'tiles_min', 'tiles_max', 'lds_bytes', 'ws_bytes')]


class ReduceJob(C.Structure):
    _fields_ = [('ws', c_vp), ('dw', c_vp), ('nslab', c_i32), ('taps', c_i32), ('kpad', c_i32), ('npad', c_i32), ('cin', c_i32), ('nvalid', c_i32),
                ('transposed', c_i32), ('accumulate', c_i32), ('lanes', c_i32), ('pad_', c_i32)]


class BnBwdDesc(C.Structure):
    _fields_ = [('da', c_vp), ('ldda', c_i32), ('dpool', c_vp), ('lddp', c_i32), ('f', c_i32),
                ('yraw', c_vp), ('ldy', c_i32),
                ('scale', c_vp), ('shift', c_vp), ('mean', c_vp), ('rstd', c_vp),
                ('sums', c_vp), ('sums_ld', c_i32), ('coef', c_vp),
                ('dy', c_vp), ('lddy_out', c_i32), ('dbias', c_vp),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32), ('c', c_i32), ('dtype', c_i32), ('linear', c_i32),
                ('yraw1', c_vp), ('ldy1', c_i32), ('dy1', c_vp), ('lddy1', c_i32), ('c_split', c_i32),
                ('sk_sums', c_vp), ('sk_sums_ld', c_i32)]


class HeadDesc(C.Structure):
    _fields_ = [('x', c_vp), ('ldx', c_i32), ('cin', c_i32),
                ('in_scale', c_vp), ('in_shift', c_vp), ('w', c_vp), ('b', c_vp),
                ('ncls', c_i32), ('activation', c_i32), ('thresh', c_f32),
                ('probs', c_vp), ('classes', c_vp), ('dlogits', c_vp),
                ('dx', c_vp), ('lddx', c_i32), ('dw', c_vp), ('db', c_vp),
                ('bnr_mean', c_vp), ('bnr_rstd', c_vp), ('bnr_sums', c_vp), ('bnr_sums_ld', c_i32),
                ('npix', c_i64), ('dtype', c_i32), ('partials', c_vp)]


class LstmGatesDesc(C.Structure):
    _fields_ = [('xg', c_vp), ('ldx', c_i32), ('hg', c_vp), ('ldh_g', c_i32), ('c_prev', c_vp),
                ('c_out', c_vp), ('h_out', c_vp), ('ldh', c_i32), ('gates_out', c_vp),
                ('stats', c_vp), ('stats_ld', c_i32),
                ('dh_a', c_vp), ('lddh_a', c_i32), ('dh_b', c_vp), ('lddh_b', c_i32), ('dc_next', c_vp),
                ('dz_out', c_vp), ('lddz', c_i32), ('dc_prev_out', c_vp),
                ('npix', c_i64), ('filters', c_i32), ('rec_act', c_i32), ('act', c_i32), ('dtype', c_i32)]


class LstmStepDesc(C.Structure):
    _fields_ = [('h_prev', c_vp), ('ldh_prev', c_i32), ('w', c_vp), ('xg', c_vp), ('ldx', c_i32), ('c_prev', c_vp),
                ('c_out', c_vp), ('h_out', c_vp), ('ldh', c_i32),
                ('n', c_i32), ('h', c_i32), ('w_', c_i32), ('filters', c_i32), ('rec_act', c_i32), ('act', c_i32), ('dtype', c_i32)]


class DenseSrc(C.Structure):
    _fields_ = [('x', c_vp), ('ld', c_i32), ('cin', c_i32), ('dtype', c_i32),
                ('in_scale', c_vp), ('in_shift', c_vp), ('in_relu', c_i32),
                ('hs', c_i32), ('ws', c_i32),
                ('dx', c_vp), ('lddx', c_i32), ('dx_dtype', c_i32)]


class DenseDesc(C.Structure):
    _fields_ = [('src', DenseSrc * 2), ('nsrc', c_i32),
                ('w', c_vp), ('b', c_vp), ('cout', c_i32),
                ('activation', c_i32), ('max_value', c_f32),
                ('out', c_vp), ('classes', c_vp), ('z_out', c_vp),
                ('npix', c_i64), ('h', c_i32), ('w_', c_i32),
                ('dout', c_vp), ('dz_out', c_vp), ('dw', c_vp), ('db', c_vp)]


class DenseSceneDesc(C.Structure):
    """satcv_dense_scene_desc: a DenseDesc (out / classes / z_out / backward fields NULL) + the crop, the origin table and the scene map"""
    _fields_ = [('head', DenseDesc),
                ('crop_y', c_i32), ('crop_x', c_i32), ('crop_h', c_i32), ('crop_w', c_i32),
                ('origins', c_vp), ('total', c_i32), ('first', c_i32),
                ('map', c_vp), ('map_h', c_i32), ('map_w', c_i32), ('ldm', c_i32), ('c0', c_i32), ('nc', c_i32),
                ('class_map', c_vp)]


# name -> (restype, argtypes); every symbol declared in include/satcv.h
_SIGS = {
    'satcv_version': (C.c_char_p, []),
    'satcv_last_error': (C.c_char_p, []),
    'satcv_device_info': (C.c_int, [C.POINTER(c_i32)]),
    'satcv_ingest_nhwc': (C.c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_i32, c_vp]),
    'satcv_ingest_nhwc_scaled': (C.c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_f32, c_i32, c_vp]),
    'satcv_ingest_chw': (C.c_int, [c_vp, c_i32, c_f32, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_pack_weights': (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_pack_job_items': (c_i64, [C.POINTER(PackJob)]),
    'satcv_pack_weights_batched': (C.c_int, [c_vp, c_vp, c_i32, c_i64, c_i32, c_vp]),
    'satcv_conv2d_igemm': (C.c_int, [C.POINTER(ConvDesc), c_vp]),
    'satcv_conv2d_igemm_pipelined': (C.c_int, [C.POINTER(ConvDesc)]),
    'satcv_conv2d_igemm_plan_info': (C.c_int, [C.POINTER(ConvDesc), c_i32, C.POINTER(ConvPlanInfo)]),
    'satcv_conv2d_wgrad_workspace': (c_i64, [C.POINTER(WgradDesc)]),
    'satcv_conv2d_wgrad': (C.c_int, [C.POINTER(WgradDesc), c_vp]),
    'satcv_conv2d_wgrad_plan_info': (C.c_int, [C.POINTER(WgradDesc), C.POINTER(WgradPlanInfo)]),
    'satcv_conv2d_wgrad_reduce_job': (C.c_int, [C.POINTER(WgradDesc), C.POINTER(ReduceJob)]),
    'satcv_reduce_job_items': (c_i64, [C.POINTER(ReduceJob)]),
    'satcv_reduce_slabs_batched': (C.c_int, [c_vp, c_vp, c_i32, c_i64, c_vp]),
    'satcv_conv2d_bwd_fused_workspace': (c_i64, [C.POINTER(BwdfDesc)]),
    'satcv_conv2d_bwd_fused': (C.c_int, [C.POINTER(BwdfDesc), c_vp]),
    'satcv_conv2d_bwd_fused_reduce_job': (C.c_int, [C.POINTER(BwdfDesc), C.POINTER(ReduceJob)]),
    'satcv_conv2d_bwd_fused_plan_info': (C.c_int, [C.POINTER(BwdfDesc), c_i32, C.POINTER(BwdfPlanInfo)]),
    'satcv_convt_bwd_fused_plan_info': (C.c_int, [C.POINTER(CtbfDesc), c_i32, C.POINTER(CtbfPlanInfo)]),
    'satcv_convt_bwd_fused_workspace': (c_i64, [C.POINTER(CtbfDesc)]),
    'satcv_convt_bwd_fused': (C.c_int, [C.POINTER(CtbfDesc), c_vp]),
    'satcv_convt_bwd_fused_reduce_job': (C.c_int, [C.POINTER(CtbfDesc), C.POINTER(ReduceJob)]),
    'satcv_bn_finalize_train': (C.c_int, [c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_f32, c_f32, c_i32, c_i32,
                                          c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    'satcv_bn_affine_infer': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_f32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_bn_affine_infer_batched': (C.c_int, [c_vp, c_i32, c_f32, c_vp]),
    'satcv_bn_relu_pool': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_bn_relu_pool_amax': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_bn_bwd_reduce': (C.c_int, [C.POINTER(BnBwdDesc), c_vp]),
    'satcv_bn_bwd_finalize': (C.c_int, [c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_i32, c_vp]),
    'satcv_bn_bwd_apply': (C.c_int, [C.POINTER(BnBwdDesc), c_vp]),
    'satcv_bn_bwd_finalize2': (C.c_int, [c_vp, c_i32, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp]),
    'satcv_maxpool': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_affine_requant': (C.c_int, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_i64, c_i32, c_i32, c_i32, c_vp]),
    'satcv_add_act': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp, c_i64, c_i32, c_i32, c_vp]),
    'satcv_relu_bwd': (C.c_int, [c_vp, c_vp, c_i64, c_i32, c_vp]),
    'satcv_bias_grad_workspace': (c_i64, [c_i64, c_i32]),
    'satcv_bias_grad': (C.c_int, [c_vp, c_i32, c_i64, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_upsample_head': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp]),
    'satcv_dropout_mask': (C.c_int, [C.c_uint64, C.c_uint64, c_f32, c_i64, c_vp, c_vp]),
    'satcv_dropout_apply': (C.c_int, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_tile_channel_mean': (C.c_int, [C.POINTER(TileDesc), c_vp, c_vp]),
    'satcv_tile_ingest': (C.c_int, [C.POINTER(TileDesc), c_vp]),
    'satcv_scene_gather': (C.c_int, [C.POINTER(SceneGatherDesc), c_vp]),
    'satcv_scene_scatter': (C.c_int, [C.POINTER(SceneScatterDesc), c_vp]),
    'satcv_series_gather': (C.c_int, [C.POINTER(SeriesGatherDesc), c_vp]),
    'satcv_median_composite': (C.c_int, [C.POINTER(CompositeDesc), c_vp]),
    'satcv_quality_mask': (C.c_int, [C.POINTER(QualityDesc), c_vp]),
    'satcv_median_composite_masked': (C.c_int, [C.POINTER(CompositeMaskedDesc), c_vp]),
    'satcv_raster_convert': (C.c_int, [C.POINTER(RasterDesc), c_vp]),
    'satcv_raster_overview': (C.c_int, [C.POINTER(RasterDesc), c_vp]),
    'satcv_raster_tiles': (C.c_int, [C.POINTER(RasterDesc), c_vp]),
    'satcv_lzw_tiles': (C.c_int, [c_vp, c_i32, c_i64, c_vp, c_vp, c_vp]),
    'satcv_lzw_encode_host': (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.POINTER(c_i64)]),
    'satcv_bytes_compact': (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp]),
    'satcv_lzw_decode_tiles': (C.c_int, [c_vp, c_i64, c_vp, c_vp, c_i32, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp]),
    'satcv_lzw_decode_host': (C.c_int, [c_vp, c_i64, c_vp, c_i64, C.POINTER(c_i64), C.POINTER(c_i32)]),
    'satcv_raster_untile': (C.c_int, [C.POINTER(UntileDesc), c_vp]),
    'satcv_raster_warp': (C.c_int, [C.POINTER(WarpDesc), c_vp]),
    'satcv_crs_transform': (C.c_int, [C.POINTER(Crs), C.POINTER(Crs), c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_i32, c_vp]),
    'satcv_grid_coords': (C.c_int, [C.POINTER(ReprojectMap), c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_raster_reproject': (C.c_int, [C.POINTER(WarpDesc), C.POINTER(ReprojectMap), c_vp]),
    'satcv_calib_overlap': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, C.c_double, c_vp, c_vp, c_vp]),
    'satcv_calib_histogram': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i32, c_vp]),
    'satcv_calib_match_lut': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_calib_scale_lut': (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_calib_apply': (C.c_int, [C.POINTER(CalibApplyDesc), c_vp]),
    'satcv_rasterize_workspace': (C.c_int, [c_i64, c_i32, c_i64, c_i32, C.POINTER(c_i64)]),
    'satcv_rasterize': (C.c_int, [C.POINTER(RasterizeDesc), c_vp]),
    'satcv_raster_mask_apply': (C.c_int, [C.POINTER(MaskApplyDesc), c_vp]),
    'satcv_record_stats': (C.c_int, [C.POINTER(RecordDesc), c_vp]),
    'satcv_record_to_tuple': (C.c_int, [C.POINTER(RecordDesc), c_vp]),
    'satcv_label_onehot': (C.c_int, [c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_i32, c_i32, c_vp]),
    'satcv_crc32c': (C.c_uint32, [c_vp, C.c_uint64, C.c_uint32]),
    'satcv_head_fwd': (C.c_int, [C.POINTER(HeadDesc), c_vp]),
    'satcv_head_bwd': (C.c_int, [C.POINTER(HeadDesc), c_vp]),
    'satcv_head_bwd_workspace': (c_i64, [C.POINTER(HeadDesc)]),
    'satcv_head_bwd_finalize': (C.c_int, [C.POINTER(HeadDesc), c_vp]),
    'satcv_loss_fwd_bwd': (C.c_int, [c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i64, c_f32, c_vp, c_vp, c_vp]),
    'satcv_loss_global_fwd_bwd': (C.c_int, [c_i32, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i64, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp]),
    'satcv_confusion': (C.c_int, [c_vp, c_vp, c_i32, c_i64, c_vp, c_vp]),
    'satcv_adam_step': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp]),
    'satcv_adam_step_part': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_vp, c_vp, c_i32, c_vp]),
    'satcv_sgd_step': (C.c_int, [c_vp, c_vp, c_vp, c_i64, c_f32, c_i32, c_vp, c_vp, c_vp]),
    'satcv_rmsprop_step': (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp]),
    'satcv_grad_clip_workspace': (c_i64, [c_i64]),
    'satcv_grad_clip': (C.c_int, [c_vp, c_i64, c_i32, c_f32, c_vp, c_vp, c_vp]),
    'satcv_comm_unique_id': (C.c_int, [c_vp]),
    'satcv_comm_init': (C.c_int, [C.POINTER(c_vp), c_i32, c_i32, c_vp]),
    'satcv_comm_destroy': (C.c_int, [c_vp]),
    'satcv_comm_info': (C.c_int, [c_vp, C.POINTER(c_i32), C.POINTER(c_i32)]),
    'satcv_allreduce_grads': (C.c_int, [c_vp, c_vp, c_i64, c_i64, c_i64, c_i32, c_vp, c_vp]),
    'satcv_allreduce': (C.c_int, [c_vp, c_vp, c_i64, c_i32, c_i32, c_vp]),
    'satcv_ingest_seq': (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp]),
    'satcv_convlstm_gates_fwd': (C.c_int, [C.POINTER(LstmGatesDesc), c_vp]),
    'satcv_convlstm_gates_bwd': (C.c_int, [C.POINTER(LstmGatesDesc), c_vp]),
    'satcv_convlstm_step_fwd': (C.c_int, [C.POINTER(LstmStepDesc), c_vp]),
    'satcv_convlstm_step_supported': (C.c_int, [c_i32, c_i32]),
    'satcv_dense_small_fwd': (C.c_int, [C.POINTER(DenseDesc), c_vp]),
    'satcv_dense_small_bwd': (C.c_int, [C.POINTER(DenseDesc), c_vp]),
    'satcv_dense_scene_fwd': (C.c_int, [C.POINTER(DenseSceneDesc), c_vp]),
    'satcv_zero2': (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp]),
    'satcv_graph_begin': (C.c_int, [c_vp]),
    'satcv_graph_end': (C.c_int, [c_vp, C.POINTER(c_vp)]),
    'satcv_graph_launch': (C.c_int, [c_vp, c_vp]),
    'satcv_graph_destroy': (C.c_int, [c_vp]),
    'satcv_prof_enable': (C.c_int, [c_i32]),
    'satcv_prof_collect': (C.c_int, [c_i32, C.POINTER(C.c_double), C.POINTER(c_i64), C.POINTER(C.c_double)]),
    'satcv_set_option': (C.c_int, [C.c_char_p, c_i32]),
    'satcv_get_option': (C.c_int, [C.c_char_p, C.POINTER(c_i32)]),
    'satcv_option_key': (C.c_char_p, [c_i32]),
}

EXPORTED_SYMBOLS = tuple(_SIGS)


class SatcvError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} not found: the HIP extension is required (no CPU fallback). '
            'Build it with `python -m satellite_computervision_amd.build` or __graft_entry__.build().')
    hip = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    if os.path.exists(hip):
        C.CDLL(hip, mode=C.RTLD_GLOBAL)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)           # AttributeError if a declared symbol is missing
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc):
    if rc != 0:
        raise SatcvError(f'satcv error {rc}: {lib.satcv_last_error().decode()}')


def call(name, *args):
    check(getattr(lib, name)(*args))
