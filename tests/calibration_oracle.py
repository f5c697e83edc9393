"""The rules of the calibration kernels (include/satcv.h, "Radiometric calibration") said again in NumPy with 64-bit integers: bincount,
cumsum, searchsorted on the cross-multiplied counts.  No torch and no import of the package: the tests compare the kernels to THIS, bit
for bit.  Rasters are (C, H, W) arrays of uint8, uint16 or int16; bin = value + bias."""
import numpy as np

BINS = {'uint8': 256, 'uint16': 65536, 'int16': 65536}
BIAS = {'uint8': 0, 'uint16': 0, 'int16': 32768}


def kind(a):
    name = np.asarray(a).dtype.name
    if name not in BINS:
        raise ValueError(f'{name} rasters are not binned')
    return name


def valid(a, nodata=None):
    """a sample equal to nodata is invalid; a nodata that is no value of the kind matches no sample"""
    a = np.asarray(a)
    if nodata is None or nodata != nodata or float(nodata) != int(nodata):
        return np.ones(a.shape, bool)
    info = np.iinfo(a.dtype)
    if not info.min <= int(nodata) <= info.max:
        return np.ones(a.shape, bool)
    return a != a.dtype.type(int(nodata))


def overlap(a, b=None, nodata=None, mask=None):
    """uint8 (H, W): every band of a and of b valid, and the mask non-zero"""
    ok = valid(a, nodata).all(axis=0)
    if b is not None:
        ok &= valid(b, nodata).all(axis=0)
    if mask is not None:
        ok &= np.asarray(mask) != 0
    return ok.astype(np.uint8)


def histogram(img, region):
    name = kind(img)
    sel = np.asarray(region).astype(bool)
    return np.stack([np.bincount(band[sel].astype(np.int64) + BIAS[name], minlength=BINS[name]) for band in img]).astype(np.uint32)


def match_lut(hist1, hist2, name):
    """-> (lut (C, bins) of the kind, counts int64 (C, 2)): the smallest u with cum1[u] * n2 >= max(cum2[v], 1) * n1 (the maximum
    keeps bins below image 2's smallest occupied one off an unoccupied bin 0); identity when n1 or n2 is 0"""
    bins, bias = BINS[name], BIAS[name]
    lut = np.empty((len(hist1), bins), np.dtype(name))
    counts = np.empty((len(hist1), 2), np.int64)
    for b, (h1, h2) in enumerate(zip(hist1, hist2)):
        cum1, cum2 = np.cumsum(h1.astype(np.int64)), np.cumsum(h2.astype(np.int64))
        n1, n2 = int(cum1[-1]), int(cum2[-1])
        counts[b] = n1, n2
        if n1 == 0 or n2 == 0:
            u = np.arange(bins)
        else:
            assert n1 < 2 ** 31 and n2 < 2 ** 31                      # the products stay below 2^62
            u = np.minimum(np.searchsorted(cum1 * n2, np.maximum(cum2, 1) * n1, side='left'), bins - 1)
        lut[b] = (u - bias).astype(name)
    return lut, counts


def scale_lut(hist, name, p):
    """-> (table float32 (C, bins), upper int32 (C)): upper = the value of the smallest bin v with cum[v] * 100 >= p * n, -1 for an empty band"""
    bins, bias = BINS[name], BIAS[name]
    table = np.full((len(hist), bins), np.nan, np.float32)
    upper = np.full(len(hist), -1, np.int32)
    values = np.arange(bins, dtype=np.int64) - bias
    for b, h in enumerate(hist):
        cum = np.cumsum(h.astype(np.int64))
        n = int(cum[-1])
        if n == 0:
            continue
        up = int(np.searchsorted(cum * 100, p * n, side='left')) - bias
        upper[b] = up
        if up != 0:
            table[b] = (np.minimum(values, up).astype(np.float64) / np.float64(up)).astype(np.float32)
    return table, upper


def apply(src, table, nodata, dst, keep=False):
    """src (C, H, W) through table (C, bins) into a copy of dst (C, H, W) of the table's dtype: invalid samples keep dst with `keep`,
    else they become nodata (integer tables; 0 without one) or NaN (float32 tables)"""
    name = kind(src)
    out = np.array(dst, copy=True)
    ok = valid(src, nodata)
    if table.dtype == np.float32:
        fill = np.float32(np.nan)
    else:
        fill = np.dtype(name).type(int(nodata)) if not ok.all() else np.dtype(name).type(0)
    for b in range(src.shape[0]):
        mapped = table[b][src[b].astype(np.int64) + BIAS[name]]
        out[b] = np.where(ok[b], mapped, out[b] if keep else fill)
    return out


def equalize(img1, img2, nodata=None, mask=None):
    name = kind(img1)
    region = overlap(img1, img2, nodata, mask)
    lut, _ = match_lut(histogram(img1, region), histogram(img2, region), name)
    return apply(img2, lut, nodata, np.zeros_like(img2))


def clamp_and_scale(img, p=99, nodata=None, mask=None):
    name = kind(img)
    region = overlap(img, None, nodata, mask)
    table, _ = scale_lut(histogram(img, region), name, p)
    return apply(img, table, nodata, np.zeros(img.shape, np.float32))


def equalize_collection(stack, nodata=None, order=None):
    out = np.array(stack, copy=True)
    order = list(range(len(out))) if order is None else list(order)
    for k in range(1, len(order)):
        out[order[k]] = equalize(out[order[k - 1]], out[order[k]], nodata)
    return out
