"""The reference's utils/calibration.py on device arrays instead of Earth Engine images: histogram matching of a scene to its western
neighbour inside their overlap, so that mosaics of neighbouring orbits or flight lines show no seam.

    get_overlap         :64-76    the region two rasters share: every band valid in both (the footprint geometry becomes validity)
    make_FC, hist_to_FC :78-134   per-band histograms of a region, one bin per stored value; (dn, probability) of the occupied bins
    equalize            :136-182  image 2 matched to image 1: DN -> cumulative probability -> DN
    clamp_and_scale     :12-45    clip at a percentile of the region and rescale to [0, 1]
    equalize_collection :184-233  the chain: every scene matched to its already equalized western neighbour

The reference fits two 100-tree random-forest regressors to a 4096-bucket histogram, an approximation of CDF matching.  Here the thing
it approximates is computed exactly and in integers (include/satcv.h, "Radiometric calibration"): `lut[v]` is the smallest `u` with
`cum1[u] * n2 >= max(cum2[v], 1) * n1`, always an occupied bin of image 1.  Kernels: csrc/calibrate.hip.  Rasters are (C, H, W), C <= 16,
uint8, uint16 or int16 -- a host array goes up once, a CUDA tensor is used where it lies (`dtype='uint16'` names the kind of an int16
tensor that stores uint16 bytes).
float32 and int32 rasters are refused: float32 needs a binning rule whose rounding can be pinned.  A sample equal to `nodata` is
invalid; without one every sample is valid.  Nothing here synchronises with the host except `hist_to_FC`.

`scene_median` (:47-62) is not mirrored: `pc_tools.median_composite` already is the per-scene median, and its float32 output is outside
the kinds supported here.  `clamp_and_scale` honours `p`; the reference's body ignores it and always asks for the 99th percentile, which
the default reproduces.
"""
import numpy as np

KINDS = {'uint8': 0, 'uint16': 1, 'int16': 3}            # the kinds of satcv_raster_desc that are binned
BINS = {'uint8': 256, 'uint16': 65536, 'int16': 65536}
BIAS = {'uint8': 0, 'uint16': 0, 'int16': 32768}         # bin = value + bias


def kind_name(dtype, dtype_name=None):
    """the kind of a raster from its NumPy / torch dtype (and `dtype=` of the caller); ValueError for what is not binned"""
    name = str(dtype).replace('torch.', '')
    if dtype_name is None:
        if name not in KINDS:
            raise ValueError(f'a raster of {name}: calibration bins uint8, uint16 and int16 rasters (float32 and int32 are refused)')
        return name
    if dtype_name not in KINDS:
        raise ValueError(f'dtype {dtype_name!r}: calibration bins uint8, uint16 and int16 rasters (float32 and int32 are refused)')
    if name not in KINDS or np.dtype(dtype_name).itemsize != np.dtype(name).itemsize:
        raise ValueError(f'dtype {dtype_name!r} does not describe a raster of {name}')
    return dtype_name


def check_percentile(p):
    if isinstance(p, bool) or not isinstance(p, (int, np.integer)) or not 1 <= p <= 100:
        raise ValueError(f'p = {p!r}: an integer percentile 1 ... 100')
    return int(p)


def check_shape(shape, ndim=3, what='a raster'):
    """(C, H, W) (or (S, C, H, W)) with 1 <= C <= 16 and H * W < 2^31"""
    shape = tuple(int(v) for v in shape)
    want = '(C, H, W)' if ndim == 3 else '(S, C, H, W)'
    if len(shape) != ndim or 0 in shape:
        raise ValueError(f'{what} is a non-empty {want} array, got shape {shape}')
    c, h, w = shape[-3:]
    if c > 16:
        raise ValueError(f'{c} bands: {what} has at most 16')
    if h * w >= 2 ** 31:
        raise ValueError(f'{what} of {h} x {w} pixels: at most 2^31 - 1')
    return shape


def check_order(order, n):
    """a permutation of range(n) as a list; None: the given order"""
    if order is None:
        return list(range(n))
    order = [int(v) for v in order]
    if sorted(order) != list(range(n)):
        raise ValueError(f'order must be a permutation of 0 ... {n - 1}, got {order}')
    return order


def _resident(x, dtype=None, ndim=3, what='a raster'):
    """-> (contiguous CUDA tensor, kind name); every refusal comes before the device is touched"""
    import torch
    from .prediction_tools import _to_device
    if isinstance(x, torch.Tensor) and x.is_cuda:
        name = kind_name(x.dtype, dtype)
        check_shape(x.shape, ndim, what)
        return x.contiguous(), name
    x = np.asarray(x.numpy() if isinstance(x, torch.Tensor) else x)
    name = kind_name(x.dtype, dtype)
    check_shape(x.shape, ndim, what)
    t = _to_device(x, what)
    return (t.view(torch.uint16) if x.dtype == np.uint16 and hasattr(torch, 'uint16') else t), name


def _nodata(nodata):
    return (0, 0.0) if nodata is None else (1, float(nodata))


def _mask(region, hw):
    import torch
    if region is None:
        return None
    if not isinstance(region, torch.Tensor):
        region = torch.from_numpy(np.ascontiguousarray(np.asarray(region) != 0).view(np.uint8)).to('cuda')
    if region.dtype == torch.bool:
        region = region.view(torch.uint8)
    if not (region.is_cuda and region.dtype == torch.uint8 and tuple(region.shape) == tuple(hw)):
        raise ValueError(f'region is a uint8 or bool (H, W) = {tuple(hw)} mask on the device, got {region.dtype} {tuple(region.shape)}')
    return region.contiguous()


# ---------------------------------------------------------------------------------------------------------- one launch each
def _overlap(a, b, name, nodata, mask):
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    c, h, w = (int(v) for v in a.shape)
    region = _device_empty((h, w), torch.uint8, 'the overlap region')
    has, nd = _nodata(nodata)
    check(lib.satcv_calib_overlap(a.data_ptr(), b.data_ptr() if b is not None else None, KINDS[name], c, h, w, has, nd,
                                  mask.data_ptr() if mask is not None else None, region.data_ptr(), ops.stream_ptr()))
    return region


def _histogram(img, name, region, split=0):
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    c, h, w = (int(v) for v in img.shape)
    hist = _device_empty((c, BINS[name]), torch.int32, 'the histograms')
    check(lib.satcv_calib_histogram(img.data_ptr(), KINDS[name], c, h, w, region.data_ptr(), hist.data_ptr(), int(split), ops.stream_ptr()))
    return hist


def _match_lut(hist1, hist2, name, like, counts=False):
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    c = int(hist1.shape[0])
    lut = _device_empty((c, BINS[name]), like.dtype, 'the matching table')
    n = _device_empty((c, 2), torch.int64, 'the overlap sizes') if counts else None
    check(lib.satcv_calib_match_lut(hist1.data_ptr(), hist2.data_ptr(), KINDS[name], c, lut.data_ptr(), n.data_ptr() if counts else None, ops.stream_ptr()))
    return (lut, n) if counts else lut


def _scale_lut(hist, name, p):
    import torch
    from . import ops
    from ._lib import check, lib
    from .prediction_tools import _device_empty
    c = int(hist.shape[0])
    table = _device_empty((c, BINS[name]), torch.float32, 'the scale table')
    upper = _device_empty((c,), torch.int32, 'the percentiles')
    check(lib.satcv_calib_scale_lut(hist.data_ptr(), KINDS[name], c, int(p), table.data_ptr(), upper.data_ptr(), ops.stream_ptr()))
    return table, upper


def _apply(src, name, table, dst, nodata, dst_float=False, layout=1, ld=None, coff=0, keep=False):
    """satcv_calib_apply: the (C, H, W) tensor `src` through `table` into the tensor `dst` (layout 1 (ld, H, W), 0 (H, W, ld))"""
    import ctypes as C
    from . import ops
    from ._lib import CalibApplyDesc, check, lib
    c, h, w = (int(v) for v in src.shape)
    has, nd = _nodata(nodata)
    d = CalibApplyDesc(src=src.data_ptr(), src_kind=KINDS[name], c=c, h=h, w_=w, has_nodata=has, nodata=nd, table=table.data_ptr(), dst=dst.data_ptr(),
                       dst_kind=2 if dst_float else KINDS[name], dst_layout=int(layout), dst_ld=c if ld is None else int(ld), dst_coff=int(coff), keep=int(bool(keep)))
    check(lib.satcv_calib_apply(C.byref(d), ops.stream_ptr()))
    return dst


def _equalize(img1, img2, name, nodata, mask, out):
    region = _overlap(img1, img2, name, nodata, mask)
    lut = _match_lut(_histogram(img1, name, region), _histogram(img2, name, region), name, img2)
    return _apply(img2, name, lut, out, nodata)


def _chain(stack, name, nodata, order):
    """`equalize_collection` on a resident (S, C, H, W) stack, in place"""
    for k in range(1, len(order)):
        _equalize(stack[order[k - 1]], stack[order[k]], name, nodata, None, stack[order[k]])
    return stack


# ---------------------------------------------------------------------------------------------------------- the reference's names
def get_overlap(a, b=None, nodata=None, region=None, dtype=None):
    """`get_overlap` (:64-76) on arrays: the uint8 (H, W) device mask of the pixels where every band of `a` and of `b` (None: of `a`
    alone) is valid; `region`, a uint8 / bool (H, W) mask, restricts it further -- it stands in for the reference's footprint geometry."""
    a, name = _resident(a, dtype)
    if b is not None:
        b, nb = _resident(b, dtype)
        if nb != name or tuple(b.shape) != tuple(a.shape):
            raise ValueError(f'the two rasters differ: {name} {tuple(a.shape)} against {nb} {tuple(b.shape)}')
    return _overlap(a, b, name, nodata, _mask(region, a.shape[1:]))


def make_FC(image, region=None, nodata=None, dtype=None):
    """`make_FC` (:106-134): the histograms of the bands of `image` over the region -> (C, bins) int32 device tensor (counts stay below
    2^31), bins = 256 (uint8) or 65536 (uint16; int16 with bin = value + 32768).  The region is `get_overlap(image, None, nodata, region)`."""
    image, name = _resident(image, dtype)
    return _histogram(image, name, _overlap(image, None, name, nodata, _mask(region, image.shape[1:])))


def hist_to_FC(hist, band, dtype=None):
    """`hist_to_FC` (:78-104): -> (dn, probability) host arrays over the occupied bins of band `band` of a `make_FC` histogram -- the
    reference's feature properties of the same names; probability = cum / n in float64.  dtype='int16' for the histogram of an int16
    raster (dn = bin - 32768)."""
    h = np.asarray(hist[int(band)].cpu().numpy() if hasattr(hist, 'cpu') else hist[int(band)]).astype(np.int64)
    if h.ndim != 1 or h.size not in (256, 65536):
        raise ValueError(f'a histogram row has 256 or 65536 bins, got shape {h.shape}')
    if dtype is not None and (dtype not in KINDS or BINS[dtype] != h.size):
        raise ValueError(f'dtype {dtype!r} does not describe a histogram of {h.size} bins')
    occupied = np.nonzero(h)[0]
    cum = np.cumsum(h)
    n = int(cum[-1])
    return occupied - (BIAS[dtype] if dtype else 0), (cum[occupied] / n if n else np.zeros(0))


def equalize(image1, image2, region=None, nodata=None, out=None, dtype=None):
    """`equalize` (:136-182): image 2 matched to image 1 over their overlap (`get_overlap(image1, image2, nodata, region)`) -> a CUDA
    tensor like image 2.  The table is applied to the whole of image 2; invalid samples stay nodata; an empty overlap leaves image 2 as
    it is (the `ee.Algorithms.If` of :225, decided on the device).  out: None a new tensor, or a tensor like image 2 -- image 2 itself
    for in place."""
    import torch
    image1, name = _resident(image1, dtype)
    image2, n2 = _resident(image2, dtype)
    if n2 != name or tuple(image1.shape) != tuple(image2.shape):
        raise ValueError(f'the two rasters differ: {name} {tuple(image1.shape)} against {n2} {tuple(image2.shape)}')
    if out is None:
        out = torch.empty_like(image2)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype == image2.dtype and out.shape == image2.shape):
        raise ValueError('out must be a contiguous CUDA tensor of the shape and dtype of image2')
    return _equalize(image1, image2, name, nodata, _mask(region, image1.shape[1:]), out)


def clamp_and_scale(img, p=99, region=None, nodata=None, dtype=None):
    """`clamp_and_scale` (:12-45): per band, `upper` = the p-th percentile (nearest rank) of the region's valid pixels; the result is
    min(v, upper) / upper as float32 (C, H, W), computed in double and rounded once.  Invalid samples are NaN; a band whose region is
    empty or whose upper is 0 is NaN throughout."""
    import torch
    p = check_percentile(p)
    img, name = _resident(img, dtype)
    region = _overlap(img, None, name, nodata, _mask(region, img.shape[1:]))
    table, _ = _scale_lut(_histogram(img, name, region), name, p)
    return _apply(img, name, table, torch.empty(tuple(img.shape), dtype=torch.float32, device='cuda'), nodata, dst_float=True)


def equalize_collection(stack, nodata=None, order=None, inplace=False, dtype=None):
    """`equalize_collection` (:184-233) on an (S, C, H, W) stack of scenes on one grid (what `raster_tools.read_aligned_stack`
    returns): scene order[0] is unchanged; for k >= 1 scene order[k] is matched to the already equalized scene order[k - 1] over their
    overlap.  order: None is the given order (the reference sorts by centroid longitude: pass the scenes west to east, or their order).
    inplace=True equalizes a resident stack where it lies; otherwise the result is a new tensor."""
    import torch
    order = check_order(order, len(stack))
    resident = isinstance(stack, torch.Tensor) and stack.is_cuda and stack.is_contiguous()
    st, name = _resident(stack, dtype, ndim=4, what='a stack')
    if inplace and not resident:
        raise ValueError('inplace=True needs a contiguous CUDA tensor')
    if resident and not inplace:
        st = st.clone()
    return _chain(st, name, nodata, order)
