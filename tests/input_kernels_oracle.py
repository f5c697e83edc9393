"""NumPy restatements of the kernels that bring data and weights into the model -- the tile input pipeline (satcv_tile_channel_mean,
satcv_tile_ingest, satcv_label_onehot), satcv_ingest_chw and the weight packers (satcv_pack_weights[_batched], satcv_pack_job_items) --
written from the semantics documented in include/satcv.h (helper module, no tests in it).  tests/test_input_kernels_cpu.py pins them to
independent implementations (oracle/input_pipeline.py, the reference's recorded aug_array_morph outputs, oracle/keras_ops and torch
float64 autograd); tests/test_input_kernels_gpu.py holds the kernels to them.  The case tables both files share are at the end."""
import math

import numpy as np

import elementwise_oracle as O

KIND_DTYPES = [np.uint8, np.uint16, np.float32, np.int16, np.float64, np.int32, np.int64]         # src_kind 0 ... 6
KIND_NAMES = ['u8', 'u16', 'f32', 'i16', 'f64', 'i32', 'i64']
GRID_FOR_CAP = 65536 * 256                    # threads of the largest tile-pipeline launch (a constant of csrc/input_pipeline.hip)
MORPHS = [(v, h, r) for v in (0, 1) for h in (0, 1) for r in range(4)]


def kind_of(a):
    return KIND_DTYPES.index(np.asarray(a).dtype.type)


def rup(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------- counter RNG
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def splitmix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _bits(seed, idx):
    with np.errstate(over='ignore'):
        return splitmix64(np.uint64(seed) ^ (np.asarray(idx, np.uint64) * np.uint64(0xD1342543DE82EF95)))


def draw_uniform(seed, idx):
    """U[0, 1): the upper 53 bits of the element's 64 random bits times 2^-53 (exact in double)"""
    return (_bits(seed, idx) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def draw_normal(seed, idx):
    """Box-Muller on the two 32-bit halves: u1 = (hi + 1) / (2^32 + 1) in (0, 1), u2 = lo / 2^32"""
    r = _bits(seed, idx)
    u1 = ((r >> np.uint64(32)).astype(np.float64) + 1.0) / 4294967297.0
    u2 = (r & np.uint64(0xFFFFFFFF)).astype(np.float64) / 4294967296.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


# ------------------------------------------------------------- tile input pipeline
def morph(a, flip_v, flip_h, rot):
    """flip_v, flip_h, then np.rot90(k) of an (n, h, w, ...) stack"""
    a = a[:, ::-1] if flip_v else a
    a = a[:, :, ::-1] if flip_h else a
    return np.ascontiguousarray(np.rot90(a, rot % 4, axes=(1, 2)))


def _trim(a, h, w):
    """centre window of the last two axes, offsets rounded down"""
    ty, tx = (a.shape[-2] - h) // 2, (a.shape[-1] - w) // 2
    return a[..., ty:ty + h, tx:tx + w]


def tile_values(planes, h, w, rescale=0.0, nan_mask=0, replace=1, seed=0, fill=None):
    """(values (n, c, h, w), flagged (n, h, w) or None): the rescaled, masked / replaced and trimmed planes before the colour step and the
    morph.  float32 planes stay float32 (the replacement draws are doubles), every other kind is float64.  `fill`: a constant that stands
    in for the draws."""
    planes = np.asarray(planes)
    n, c, hin, win = planes.shape
    if planes.dtype == np.float32:
        v = planes / np.float32(rescale) if rescale else planes.copy()
    else:
        v = planes.astype(np.float64)
        if rescale:
            v = v / np.float64(rescale)
    v = v.astype(np.float64)                                   # exact for float32; the draws need the room
    flagged = None
    if nan_mask:
        idx = np.arange(v.size, dtype=np.uint64).reshape(v.shape)   # the element's index in the source planes
    with np.errstate(invalid='ignore'):
        if nan_mask == 1:
            flagged = np.logical_or.accumulate(np.isnan(v) | (v < -5000.0), axis=1)          # this channel or an earlier one
            if replace:
                v = np.where(flagged, draw_normal(seed, idx) if fill is None else fill, v)
            flagged = flagged[:, -1] if replace else np.zeros((n, hin, win), bool)
        elif nan_mask == 2:
            isn = np.isnan(v)
            flagged = (isn | (v < -1.0)).any(axis=1)
            v = np.where(isn, draw_uniform(seed, idx) if fill is None else fill, v)
    return _trim(v, h, w), (None if flagged is None else _trim(flagged, h, w))


def tile_replaced(planes, h, w, rescale=0.0, nan_mask=0, replace=1, flip_v=0, flip_h=0, rot=0):
    """(n, ho, wo, c) bool: the elements that hold a draw"""
    a, _ = tile_values(planes, h, w, rescale, nan_mask, replace, 0, fill=np.inf)
    b, _ = tile_values(planes, h, w, rescale, nan_mask, replace, 0, fill=-np.inf)
    return morph(np.moveaxis(np.isposinf(a) & np.isneginf(b), 1, 3), flip_v, flip_h, rot)


def tile_ingest(planes, h, w, rescale=0.0, nan_mask=0, replace=1, seed=0, ch_mean=None, contra=1.0, bright=1.0, flip_v=0, flip_h=0, rot=0,
                fill=None, as64=False):
    """-> (n, ho, wo, c[+1]) float32 (as64: the doubles before the output rounding; float32 planes have none after the colour step).
    ch_mean: (n, c) doubles or None; the mask channel is 1 where mode 1 replaced, or where mode 2 found every band valid."""
    f32 = np.asarray(planes).dtype == np.float32
    v, flagged = tile_values(planes, h, w, rescale, nan_mask, replace, seed, fill)
    if ch_mean is not None:
        mu = np.asarray(ch_mean, np.float64)[:, :, None, None]
        with np.errstate(invalid='ignore', over='ignore'):
            if f32:
                m = mu.astype(np.float32)
                t1 = (v.astype(np.float32) - m) * np.float32(contra)
                t2 = m * np.float32(bright)
                v = t1 + t2
            else:
                t1 = (v - mu) * np.float64(contra)
                t2 = mu * np.float64(bright)
                v = t1 + t2
    with np.errstate(over='ignore', invalid='ignore'):
        out = np.moveaxis(v, 1, 3).astype(np.float64 if as64 else np.float32)
    if nan_mask:
        m = flagged if nan_mask == 1 else ~flagged
        out = np.concatenate([out, m.astype(out.dtype)[..., None]], axis=-1)
    return morph(out, flip_v, flip_h, rot)


def tile_channel_mean(planes, h, w, rescale=0.0, nan_mask=0, seed=0):
    """(mean, cnt, sum|v|), each (n, c): the correctly rounded (math.fsum) mean of the non-NaN values of the trimmed window, the mode-2 draws
    included; NaN where no value is valid"""
    v, _ = tile_values(planes, h, w, rescale, 2 if nan_mask == 2 else 0, 0, seed)
    n, c = v.shape[:2]
    mean, cnt, sabs = np.zeros((n, c)), np.zeros((n, c), np.int64), np.zeros((n, c))
    for b in range(n):
        for ch in range(c):
            x = v[b, ch].reshape(-1)
            x = x[~np.isnan(x)]
            cnt[b, ch], sabs[b, ch] = x.size, math.fsum(np.abs(x))
            mean[b, ch] = math.fsum(x) / x.size if x.size else np.nan
    return mean, cnt, sabs


def mean_bound(cnt, sabs):
    """|device mean - fsum mean| <= (cnt + 1) 2^-53 sum|v| / cnt: cnt - 1 double additions in any order, the division, the reference's own
    rounding"""
    return (cnt + 1) * 2.0 ** -53 * sabs / np.maximum(cnt, 1)


def label_class(lc, lut=None, lu=None, lu_lut=None):
    """class index per label element (int64; negative = none)"""
    lc = np.asarray(lc)
    if lc.dtype.kind == 'f':
        x = lc.astype(np.float64)
        ok = np.isfinite(x) & (x >= -2.0 ** 63) & (x < 2.0 ** 63)
        v = np.where(ok, np.trunc(np.where(ok, x, 0.0)), -1.0).astype(np.int64)              # toward zero
    else:
        v = lc.astype(np.int64)
    cls = v.copy()
    if lut is not None:
        lut = np.asarray(lut, np.int64)
        inr = (v >= 0) & (v < 256)
        e = lut[np.where(inr, v, 0)]
        cls = np.where(inr & (e >= 0), e, cls)
    if lu is not None:
        lu_lut = np.asarray(lu_lut, np.int64)
        u = np.asarray(lu).astype(np.float64)
        with np.errstate(invalid='ignore'):
            inr = (u >= 0) & (u < 256) & (u == np.floor(u))
        e = lu_lut[np.where(inr, u, 0).astype(np.int64)]
        cls = np.where(inr & (e >= 0), e, cls)
    return cls


def label_onehot(lc, lut, lu, lu_lut, h, w, ncls, morph_):
    """(n, 1, hin, win) labels -> (n, ho, wo, ncls) float32; a class outside [0, ncls) gives a zero row"""
    cls = _trim(label_class(lc, lut, lu, lu_lut), h, w)[:, 0]
    return morph((cls[..., None] == np.arange(ncls)).astype(np.float32), *morph_)


# --------------------------------------------------------------------- ingest_chw
def ingest_chw(planes, scale, cpad, kind):
    """(n, c, h, w) u8 / u16 / f32 -> (n, h, w, cpad) float64 values of the storage type: one float32 multiply, one storage rounding"""
    p = np.asarray(planes)
    n, c, h, w = p.shape
    out = np.zeros((n, h, w, cpad), np.float32)
    out[..., :c] = np.moveaxis(p.astype(np.float32) * np.float32(scale), 1, 3)
    return O.to_storage(out, kind)


# ----------------------------------------------------------------- weight packing
PACK_MODES = ['conv fwd', 'conv dgrad', 'convT fwd', 'convT dgrad']


def pack_dims(mode, taps, cin, cout, cin_pad):
    """(image taps, kpad, npad)"""
    kpad = [cin_pad, rup(cout, 16), cin_pad, rup(taps * cout, 16)][mode]
    npad = rup([cout, cin, taps * cout, cin][mode], 32)
    return (taps if mode < 2 else 1), kpad, npad


def pack_matrix(kernel, mode, cin_pad):
    """the zero-padded GEMM operand M[tap, k, n] (float64) of a Keras kernel: (kh, kw, cin, cout) for modes 0 / 1, the Conv2DTranspose
    layout (kh, kw, cout, cin) for modes 2 / 3"""
    kernel = np.asarray(kernel, np.float64)
    kh, kw = kernel.shape[:2]
    taps = kh * kw
    if mode < 2:
        cin, cout = kernel.shape[2:]
    else:
        cout, cin = kernel.shape[2:]
    ptaps, kpad, npad = pack_dims(mode, taps, cin, cout, cin_pad)
    m = np.zeros((ptaps, kpad, npad))
    k3 = kernel.reshape(taps, *kernel.shape[2:])
    if mode == 0:                                   # k = ci, n = co
        m[:, :cin, :cout] = k3
    elif mode == 1:                                 # k = co, n = ci, taps flipped
        m[:, :cout, :cin] = k3[::-1].transpose(0, 2, 1)
    elif mode == 2:                                 # k = ci, n = (i kw + j) cout + o
        m[0, :cin, :taps * cout] = k3.reshape(taps * cout, cin).T
    else:                                           # k = (i kw + j) cout + o, n = ci
        m[0, :taps * cout, :cin] = k3.reshape(taps * cout, cin)
    return m


def pack_image(kernel, mode, cin_pad, el=8, kind='f32'):
    """flat image P[tap, k // el, n, k % el] as float64 values of the storage type ('f64': unrounded)"""
    m = pack_matrix(kernel, mode, cin_pad)
    t, kpad, npad = m.shape
    assert kpad % el == 0
    p = m.reshape(t, kpad // el, el, npad).transpose(0, 1, 3, 2).reshape(-1)
    return p if kind == 'f64' else O.to_storage(p.astype(np.float32), kind)


def pack_owned(kernel, mode, cin_pad, el=8):
    """boolean flat image: True where the element comes from the kernel, False where it is padding"""
    m = pack_matrix(np.ones_like(np.asarray(kernel, np.float64)), mode, cin_pad)
    t, kpad, npad = m.shape
    return m.reshape(t, kpad // el, el, npad).transpose(0, 1, 3, 2).reshape(-1) != 0


def storage_bits(values, kind):
    """the bit pattern (unsigned integers) of values that the storage type holds exactly"""
    if kind == 'fp8':
        return O.e4m3_round(values)
    u = np.asarray(values, np.float64).astype(np.float32).view(np.uint32)
    return u if kind == 'f32' else (u >> 16).astype(np.uint16)


# ------------------------------------------------- cases shared by the CPU and the GPU file (same seeds, same shapes)
TILE_SHAPES = [((5, 7), (8, 10), (8, 12)), ((16, 16), (20, 18), (19, 21)), ((12, 20), (16, 22), (15, 25))]     # (h, w), even trim, odd trim
RESCALE = {'u8': 255.0, 'u16': 10000.0, 'f32': 100.0, 'i16': 10000.0, 'f64': 100.0, 'i32': 10000.0, 'i64': 10000.0}
MEAN_WINDOWS = [(5, 7), (16, 16), (300, 300)]


def make_planes(kind, shape, seed, nan_frac=0.0, low_frac=0.0, rescale=0.0, mode=1):
    """random planes of one kind; `nan_frac` of the elements NaN (float kinds), `low_frac` below the mode's threshold after the rescale
    (signed and float kinds)"""
    rng = np.random.default_rng(seed)
    dt = KIND_DTYPES[KIND_NAMES.index(kind)]
    if kind == 'u8':
        p = rng.integers(0, 256, shape)
    elif kind == 'u16':
        p = rng.integers(0, 65536, shape)
    elif kind in ('f32', 'f64'):
        p = rng.standard_normal(shape) * 300.0 + 100.0
    else:
        p = rng.integers(-3000, 12000, shape)
    p = p.astype(dt)
    thr = (-5000.0 if mode == 1 else -1.0) * (rescale or 1.0)
    can_low = kind in ('f32', 'f64') or (kind not in ('u8', 'u16') and thr * 3 >= np.iinfo(dt).min)
    if low_frac and can_low:
        sel = rng.random(shape) < low_frac
        p[sel] = np.asarray(thr * 3).astype(dt)
    if nan_frac and kind in ('f32', 'f64'):
        p[rng.random(shape) < nan_frac] = np.nan
    return p


def threshold_planes(kind, rescale, mode):
    """(1, 3, 4, 6) planes holding the threshold of the mode (-5000 or -1, times the rescale), its two neighbours in the plane's type, and
    values well on either side, in every channel position: first, middle and last"""
    dt = KIND_DTYPES[KIND_NAMES.index(kind)]
    t = (-5000.0 if mode == 1 else -1.0) * (rescale or 1.0)
    if kind in ('f32', 'f64'):
        t = dt(t)
        vals = [t, np.nextafter(t, dt(-np.inf)), np.nextafter(t, dt(np.inf)), dt(2 * t), dt(0.5 * t)]
    else:
        vals = [t, t - 1, t + 1, 2 * t, t // 2]
    p = np.full((1, 3, 4, 6), 7, dtype=dt)
    for ch in range(3):
        for i, x in enumerate(vals):
            p[0, ch, ch, i] = x                                                          # row ch of channel ch: other channels stay clean
    return p, [dt(x) for x in vals[:3]]


def threshold_cases():
    """(kind, rescale, mode) whose threshold, scaled, fits the plane's type"""
    return [('f32', 0.0, 1), ('f32', 100.0, 1), ('f64', 0.0, 1), ('f64', 100.0, 1), ('i16', 0.0, 1), ('i32', 10000.0, 1), ('i64', 10000.0, 1),
            ('f32', 0.0, 2), ('f32', 10000.0, 2), ('f64', 10000.0, 2), ('i16', 10000.0, 2), ('i32', 100.0, 2), ('i64', 0.0, 2)]


def exact_mean_planes(kind, shape, seed):
    """integer planes whose window sums are exact in double whatever the order: |v| < 2^28, so that after a power-of-two rescale down to
    1/8 the values are multiples of 1/4 below 2^31 and fewer than 2^17 of them sum to less than 2^52 quarter units"""
    rng = np.random.default_rng(seed)
    dt = KIND_DTYPES[KIND_NAMES.index(kind)]
    hi = {'u8': 256, 'u16': 65536, 'i16': 32768, 'i32': 2 ** 28, 'i64': 2 ** 28}[kind]
    lo = 0 if kind in ('u8', 'u16') else -hi
    return rng.integers(lo, hi, shape).astype(dt)


LABEL_KINDS = ['u8', 'i16', 'f32', 'f64', 'i32', 'i64']


def label_planes(kind, shape, seed):
    rng = np.random.default_rng(seed)
    dt = KIND_DTYPES[KIND_NAMES.index(kind)]
    lc = rng.integers(0, 14, shape).astype(dt)
    flat = lc.reshape(-1)
    extra = {'u8': [255, 200], 'i16': [255, 256, 300, -1, -7, 32767], 'i32': [256, -1, 2 ** 31 - 1, -2 ** 31, 1000], 'i64': [256, -1, 2 ** 62, -2 ** 63, 2 ** 63 - 1],
             'f32': [2.7, -0.5, 255.9, 256.0, -1.0, np.nan, np.inf, -np.inf, 1e30, 3.999], 'f64': [2.7, -0.5, 255.9, 256.0, -1.5, np.nan, np.inf, -np.inf, 1e300, 1e19],
             'u16': [256, 65535, 255]}[kind]
    flat[rng.permutation(flat.size)[:len(extra)]] = np.array(extra).astype(dt) if kind not in ('f32', 'f64') else np.array(extra, dt)
    return lc


def landuse_planes(kind, shape, seed):
    rng = np.random.default_rng(seed)
    dt = KIND_DTYPES[KIND_NAMES.index(kind)]
    lu = rng.choice([0, 82, 84, 5], size=shape).astype(dt)
    if kind in ('f32', 'f64'):
        lu.reshape(-1)[:6] = [82.5, 256.0, 338.0, np.nan, -82.0, np.inf]
    elif kind != 'u8':
        lu.reshape(-1)[:3] = [256 + 82, 256, 84]
    return lu


EXACT_MEAN_KINDS = ['u8', 'u16', 'i16', 'i32', 'i64']
EXACT_MEAN_RESCALES = [0.0, 4.0, 0.125]           # none, or a power of two: the division is exact too

# plain kernels (kh, kw, cin, cout, cin_pad) and transposed ones (kh, kw, cout, cin, cin_pad)
PACK_PLAIN = [(3, 3, 4, 32, 16), (3, 3, 13, 24, 16), (1, 1, 32, 2, 32), (7, 7, 3, 40, 16), (3, 3, 64, 64, 96)]
PACK_TRANSPOSED = [(2, 2, 2, 32, 32), (2, 2, 64, 32, 32), (2, 2, 24, 13, 16)]
PACK_FP8X = [(3, 3, 64, 64, 64, 0), (3, 3, 13, 24, 16, 0), (1, 1, 32, 2, 32, 0), (2, 2, 64, 32, 32, 1), (2, 2, 24, 13, 16, 1)]      # (..., transposed)


def pack_kernel_values(shape, seed):
    """normal weights, a few beyond the e4m3 range (saturation) and a few in its subnormal range (2^-9 steps below 2^-6)"""
    rng = np.random.default_rng(seed)
    k = rng.standard_normal(shape).astype(np.float32)
    flat = k.reshape(-1)
    pick = rng.permutation(flat.size)[:min(24, flat.size // 2)]
    special = np.array([500.0, -1000.0, 448.0, 449.0, 464.0, 3e38, -465.0, 480.0, 2.0 ** -9, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, -3.5 * 2.0 ** -9,
                        2.0 ** -10, 1.0000001 * 2.0 ** -10, 0.9 * 2.0 ** -10, 7.4 * 2.0 ** -9, 2.0 ** -6, -0.0146, 0.0137, 1e-30, 0.0, 0.001, -0.002,
                        0.0107], np.float32)
    flat[pick] = special[:pick.size]
    return k


def batched_jobs(big=512):
    """(kh, kw, cin, cout, cin_pad, mode) in launch order: a small job first, the large ones in the middle, a small one last"""
    jobs = [(1, 1, 32, 2, 32, 0)]
    for kh, kw, cin, cout, cp in PACK_PLAIN:
        jobs += [(kh, kw, cin, cout, cp, 0), (kh, kw, cin, cout, cp, 1)]
    for kh, kw, cout, cin, cp in PACK_TRANSPOSED:
        jobs += [(kh, kw, cin, cout, cp, 2), (kh, kw, cin, cout, cp, 3)]
    jobs += [(3, 3, 16, 16, 16, 1), (3, 3, 48, 48, 48, 1), (3, 3, 32, 64, 32, 1), (3, 3, 64, 64, 64, 1), (3, 3, 64, 64, 64, 0)]
    jobs += [(3, 3, big, big, big, 0), (3, 3, big, big, big, 1)]
    jobs += [(3, 3, 13, 24, 16, 1), (3, 3, 4, 32, 16, 0)]
    return jobs


def job_real_items(job):
    """16-byte (8-element) items of the image, before the rounding up to 256"""
    kh, kw, cin, cout, cp, mode = job
    t, kpad, npad = pack_dims(mode, kh * kw, cin, cout, cp)
    return t * (kpad // 8) * npad


def job_kernel_shape(job):
    kh, kw, cin, cout, cp, mode = job
    return (kh, kw, cin, cout) if mode < 2 else (kh, kw, cout, cin)


CHW_CASES = [(4, 16), (13, 16), (8, 8), (3, 24)]          # (c, cpad); n = 3, h x w = 5 x 7
CHW_SOURCES = ['u8', 'u16', 'f32']


def chw_planes(src, shape, seed):
    rng = np.random.default_rng(seed)
    if src == 'u8':
        return rng.integers(0, 256, shape).astype(np.uint8), 1.0 / 255
    if src == 'u16':
        p = rng.integers(0, 65536, shape).astype(np.uint16)
        p.reshape(-1)[:4] = [32768, 65535, 32767, 40000]
        return p, 1.0 / 10000
    return (rng.standard_normal(shape) * 50).astype(np.float32), 0.37
