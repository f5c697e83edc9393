"""NumPy restatement of the Sentinel-2 quality masks (reference utils/ee_tools.py) for the quality tests, in two forms:

  exact    the definition of include/satcv.h in integers: every threshold as a cross-multiplied inequality, the cloud score as a floor
           division.  int64 holds every intermediate exactly for 16-bit DN (the largest, L^2 and 16 (5 sum x^2 - (sum x)^2) of the
           water rule, stay below 2^41), which `_roles` asserts; Python's `//` on these arrays is the floor.
  literal  the reference's expressions as written, in float64: `/ 10000` (sentinel2toa :90), `rescale` (:110), `normalizedDifference`,
           `min`, `clamp`, `.multiply(100).byte()` (saturating, truncating).

The two can differ only on samples that sit exactly on a threshold; the exact form says which ones those are.  Earth Engine cannot be
run here, so two of its conventions are taken from its documentation: a division by zero gives 0, and ee.Reducer.stdDev is the
population form (ddof 0).  A masked (nodata) input masks the result: score 255 / NaN, and the sample fails the rule.

Also the seeded land / cloud / water / nodata generator with the planted pixels of both test files, and the masked composite."""
import numpy as np

import composite_oracle

QA60, CLOUD, SHADOW, WATER, SCL = 1, 2, 4, 8, 16
PRESETS = {'toa': QA60 | CLOUD, 'sr': QA60 | SCL, 'mask': QA60 | CLOUD | SHADOW | WATER}
REFL = ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12')
NEED = {CLOUD: ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11'), SHADOW: ('B11',), WATER: ('B2', 'B3', 'B4', 'B8', 'B11', 'B12')}
BANDS9 = ['B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60']
BANDS14 = ['B11', 'QA60', 'B4', 'B8A', 'B2', 'SCL', 'B12', 'B3', 'B1', 'B10', 'B5', 'B8', 'B7', 'B6']      # shuffled order


def _roles(stack, bands, offsets):
    """-> ({role: harmonised DN, int64 (T, H, W)}, {role: valid}, {code name: (int64 code, ok)})"""
    s = np.asarray(stack)
    T = s.shape[0]
    off = np.zeros(T, np.int64) if offsets is None else np.rint(np.maximum(np.asarray(offsets, np.float64), 0)).astype(np.int64)
    x, valid, codes = {}, {}, {}
    for i, b in enumerate(bands):
        p = s[:, i]
        if b in REFL:
            v = p > 0                                          # NaN and negative values are nodata
            q = np.where(v, p, 0).astype(np.float64)
            assert np.all(q == np.floor(q)) and q.max(initial=0) < 65536, 'the exact form is for integer-valued DN below 2^16'
            o = off[:, None, None]
            x[b] = np.where(v, np.maximum(q.astype(np.int64), o) - o, 0)
            valid[b] = v
        elif b in ('QA60', 'SCL'):
            ok = ~np.isnan(p) if p.dtype.kind == 'f' else np.ones(p.shape, bool)
            codes[b] = (np.trunc(np.where(ok, p, 0)).astype(np.int64), ok)
    return x, valid, codes


def _all_valid(valid, rule):
    return np.logical_and.reduce([valid[b] for b in NEED[rule]])


def cloud_score_exact(stack, bands, offsets=None, with_flag=False):
    """floor(min(100, t1 ... t6)) limited to 0 ... 100, 255 where a band it reads is nodata; with_flag: also where the minimum is an
    integer, i.e. the sample sits on a threshold of the truncation"""
    x, valid, _ = _roles(stack, bands, offsets)
    B1, B2, B3, B4, B8, B10, B11 = (x[b] for b in NEED[CLOUD])
    d5, d6 = B8 + B11, B3 + B11
    terms = [(B2 - 1000, np.full_like(B2, 40), 0), (B1 - 1000, np.full_like(B2, 20), 0), (B1 + B10 - 1500, np.full_like(B2, 5), 0),
             (B2 + B3 + B4 - 2000, np.full_like(B2, 60), 0),
             (np.where(d5 > 0, 500 * (B8 - B11), 0), np.where(d5 > 0, d5, 1), 50),
             (np.where(d6 > 0, -500 * (B3 - B11), 0), np.where(d6 > 0, d6, 1), 400)]
    floors = [num // den + add for num, den, add in terms]
    F = np.minimum.reduce(floors + [np.full_like(B2, 100)])
    on = np.zeros(F.shape, bool)
    for (num, den, add), f in zip(terms, floors):
        on |= (num % den == 0) & (f == F)
    ok = _all_valid(valid, CLOUD)
    score = np.where(ok, np.clip(F, 0, 100), 255).astype(np.uint8)
    return (score, on & ok & (F > 0) & (F <= 100)) if with_flag else score


def water_decision_exact(stack, bands, offsets=None, with_flag=False):
    """all three terms of waterScore above 1/4 (False where a band it reads is nodata: the caller fails the rule there)"""
    x, valid, _ = _roles(stack, bands, offsets)
    B2, B3, B4, B8, B11, B12 = (x[b] for b in NEED[WATER])
    S = B8 + B11 + B12
    sx = B3 + B4 + B8 + B11 + B12
    sq = B3 * B3 + B4 * B4 + B8 * B8 + B11 * B11 + B12 * B12
    L, Q = 20 * B2 - sx, 5 * sq - sx * sx
    w1 = S < 3125
    w2 = (sx > 0) & (L > 0) & (L * L > 16 * Q)
    w3 = 40 * (B3 - B11) > 17 * (B3 + B11)
    ok = _all_valid(valid, WATER)
    water = ok & w1 & w2 & w3
    on = ok & ((S == 3125) | ((L > 0) & (L * L == 16 * Q)) | ((40 * (B3 - B11) == 17 * (B3 + B11)) & (B3 + B11 > 0)))
    return (water, on) if with_flag else water


def rule_passes(stack, bands, offsets=None, cloud_max=15, shadow_min=900):
    """{rule bit: (T, H, W) bool, the sample passes that rule} for the rules whose planes the stack has"""
    x, valid, codes = _roles(stack, bands, offsets)
    out = {}
    if 'QA60' in codes:
        qa, ok = codes['QA60']
        out[QA60] = ok & ((qa & 1024) == 0) & ((qa & 2048) == 0)
    if 'SCL' in codes:
        scl, ok = codes['SCL']
        out[SCL] = ok & ~np.isin(scl, [0, 2, 3, 8, 9, 10, 11])
    out[CLOUD] = cloud_score_exact(stack, bands, offsets).astype(np.int64) <= min(cloud_max, 254)      # 255: nodata, never clear
    out[SHADOW] = valid['B11'] & (x['B11'] > shadow_min)
    out[WATER] = _all_valid(valid, WATER) & ~water_decision_exact(stack, bands, offsets)
    return out


def combine(passes, rules):
    """the clear mask of the bit set `rules` from `rule_passes`"""
    return np.logical_and.reduce([passes[r] for r in (QA60, CLOUD, SHADOW, WATER, SCL) if rules & r])


def clear_exact(stack, bands, rules, offsets=None, cloud_max=15, shadow_min=900):
    """(T, H, W) bool: the sample passes every rule of the bit set `rules`"""
    return combine(rule_passes(stack, bands, offsets, cloud_max, shadow_min), rules)


# ---------------------------------------------------------------------------------------------------------------- the literal float64 forms
def _toa(stack, bands, offsets):
    """sentinel2toa :90 on the harmonised samples: {role: reflectance float64, NaN = masked}"""
    s = np.asarray(stack).astype(np.float64)
    T = s.shape[0]
    off = np.zeros(T) if offsets is None else np.rint(np.maximum(np.asarray(offsets, np.float64), 0))
    out = {}
    for i, b in enumerate(bands):
        if b in REFL:
            p = s[:, i]
            with np.errstate(invalid='ignore'):
                v = p > 0
            o = off[:, None, None]
            out[b] = np.where(v, np.maximum(np.where(v, p, 0), o) - o, np.nan) / 10000
    return out


def _rescale(img, thresholds):
    return (img - thresholds[0]) / (thresholds[1] - thresholds[0])


def _nd(a, b):
    """normalizedDifference; 0 where the sum is 0 (Earth Engine's division by zero)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(a + b == 0, 0.0, (a - b) / (a + b))


def cloud_score_float(stack, bands, offsets=None):
    """sentinelCloudScore :218-255 as written -> uint8, 255 where masked"""
    im = _toa(stack, bands, offsets)
    score = np.ones_like(im['B2'])
    score = np.minimum(score, _rescale(im['B2'], [0.1, 0.5]))
    score = np.minimum(score, _rescale(im['B1'], [0.1, 0.3]))
    score = np.minimum(score, _rescale(im['B1'] + im['B10'], [0.15, 0.2]))
    score = np.minimum(score, _rescale(im['B4'] + im['B3'] + im['B2'], [0.2, 0.8]))
    score = np.minimum(score, _rescale(_nd(im['B8'], im['B11']), [-0.1, 0.1]))
    score = np.minimum(score, _rescale(_nd(im['B3'], im['B11']), [0.8, 0.6]))
    masked = np.isnan(score)
    byte = np.trunc(np.clip(np.where(masked, 0, score * 100), 0, 255))
    return np.where(masked, 255, byte).astype(np.uint8)


def water_score_float(stack, bands, offsets=None):
    """waterScore :115-157 as written -> float64 in [0, 1], NaN where masked"""
    im = _toa(stack, bands, offsets)
    score = np.ones_like(im['B2'])
    total = im['B8'] + im['B11'] + im['B12']
    score = np.minimum(score, np.clip(_rescale(total, [0.35, 0.2]), 0, 1))
    dark = np.stack([im[b] for b in ('B3', 'B4', 'B8', 'B11', 'B12')])
    mean, std = dark.mean(axis=0), dark.std(axis=0)
    with np.errstate(invalid='ignore', divide='ignore'):
        z = np.where(mean == 0, 0.0, (im['B2'] - std) / mean)
    z = np.where(np.isnan(mean + im['B2']), np.nan, z)
    score = np.minimum(score, np.clip(_rescale(z, [0, 1]), 0, 1))
    score = np.minimum(score, _rescale(_nd(im['B3'], im['B11']), [0.3, 0.8]))
    return np.clip(score, 0, 1)


# ---------------------------------------------------------------------------------------------------------------- composite, bit-planes
def pack_bits(clear):
    """(T, H, W) bool -> (ceil(T / 32), H, W) uint32, bit j % 32 of word j / 32"""
    T = clear.shape[0]
    words = np.zeros(((T + 31) // 32,) + clear.shape[1:], np.uint32)
    for j in range(T):
        words[j // 32] |= clear[j].astype(np.uint32) << np.uint32(j % 32)
    return words


def zero_unclear(stack, clear, band_idx):
    """the planes `band_idx` of the stack with every sample that is not clear set to 0 (nodata)"""
    sel = np.ascontiguousarray(np.asarray(stack)[:, list(band_idx)])
    sel[~np.broadcast_to(clear[:, None], sel.shape)] = 0
    return sel


def masked_composite(stack, clear, offsets, band_idx):
    """composite_oracle.composite of the stack whose non-clear samples are nodata -> (median, norm) float64 (H, W, len(band_idx))"""
    return composite_oracle.composite(zero_unclear(stack, clear, band_idx), offsets)


# ---------------------------------------------------------------------------------------------------------------- generator
# harmonised DN (low, high) per role for the three valid populations
_POP = {'land':  dict(B1=(300, 1300), B2=(300, 1700), B3=(400, 1800), B4=(300, 2200), B8=(1800, 4500), B10=(5, 60), B11=(700, 3200), B12=(500, 2500)),
        'cloud': dict(B1=(1300, 6000), B2=(1500, 7000), B3=(1800, 7000), B4=(1800, 7000), B8=(2500, 7000), B10=(50, 900), B11=(1500, 6000), B12=(1000, 5000)),
        'water': dict(B1=(600, 1300), B2=(500, 1300), B3=(300, 1000), B4=(100, 700), B8=(30, 500), B10=(5, 40), B11=(20, 400), B12=(10, 300))}
_LAND = dict(B1=700, B2=800, B3=900, B4=1000, B8=3000, B10=20, B11=2000, B12=1500)
_CLOUD = dict(B1=3000, B2=3000, B3=3000, B4=3000, B8=4000, B10=500, B11=3500, B12=2000)
# (role values that put cloud term k exactly on 16, the change that takes it one DN below): every other term stays >= 16
PLANTED_TERMS = [(dict(B2=1640), dict(B2=1639)), (dict(B1=1320), dict(B1=1319)), (dict(B1=1400, B10=180), dict(B1=1400, B10=179)),
                 (dict(B2=1700, B3=630, B4=630), dict(B2=1700, B3=630, B4=629)), (dict(B8=466, B11=534), dict(B8=465, B11=534)),
                 (dict(B3=884, B11=116), dict(B3=885, B11=116))]
# flat pixel index of each planted case (maps of at least 24 pixels)
P_NONE, P_ALL, P_ONE, P_TWO, P_TERM0, P_QA10, P_QA11, P_SCL0, P_NODATA_BAND = 0, 1, 2, 3, 4, 16, 17, 18, 19
PLANTED_PIXELS = 24


def make_stack(seed, dtype, t, H, W, bands):
    """-> (stack (t, len(bands), H, W) of `dtype`, offsets (t,) float32: the later half of the acquisitions at 1000).

    Per sample one of four populations: clear land 58 %, cloud 20 %, water 12 %, nodata 10 % (all reflectance bands 0; f32 also NaN
    and negative values, i16 negative values); 3 % of the valid samples lose one band.  QA60 carries bit 10 / 11 on 8 % / 5 % of the
    samples (and unrelated low bits), SCL is drawn from 0 ... 11.  Maps of at least PLANTED_PIXELS pixels get the planted pixels."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    npix = H * W
    pop = rng.choice(4, size=(t, npix), p=[0.58, 0.20, 0.12, 0.10])
    val = {}
    for b in REFL:
        v = np.zeros((t, npix), np.int64)
        for k, name in enumerate(('land', 'cloud', 'water')):
            lo, hi = _POP[name][b]
            v = np.where(pop == k, rng.integers(lo, hi, (t, npix)), v)
        val[b] = v
    cl = pop == 1                                                  # clouds: B11 follows B8, so that the moisture term stays high for most
    val['B11'] = np.where(cl, (val['B8'] * rng.uniform(0.55, 1.15, (t, npix))).astype(np.int64), val['B11'])
    lost = (rng.random((t, npix)) < 0.03) & (pop < 3)
    which = rng.integers(0, len(REFL), (t, npix))
    for k, b in enumerate(REFL):
        val[b] = np.where(lost & (which == k), 0, val[b])
    qa = rng.integers(0, 8, (t, npix)) * (rng.random((t, npix)) < 0.2)
    r = rng.random((t, npix))
    qa = qa | np.where(r < 0.08, 1024, 0) | np.where((r > 0.05) & (r < 0.10), 2048, 0)
    scl = rng.choice(12, size=(t, npix), p=[0.03, 0.01, 0.04, 0.05, 0.35, 0.25, 0.08, 0.03, 0.05, 0.05, 0.03, 0.03])

    def plant(p, j, values, q=0, s=4):
        for b in REFL:
            val[b][j, p] = values.get(b, 0)
        qa[j, p], scl[j, p] = q, s
    if npix >= PLANTED_PIXELS:
        every = slice(None)
        plant(P_NONE, every, {}, 1024, 0)                          # no clear acquisition under any rule
        plant(P_ALL, every, _LAND)                                 # clear throughout under every rule
        plant(P_ONE, every, {}, 1024, 0)
        plant(P_ONE, t - 1, _LAND)                                 # exactly one clear sample (the last acquisition)
        plant(P_TWO, every, {}, 1024, 0)
        plant(P_TWO, 0, _LAND)
        plant(P_TWO, t - 1, dict(_LAND, B2=600))                   # exactly two (one for t = 1)
        for k, (on, below) in enumerate(PLANTED_TERMS):
            plant(P_TERM0 + 2 * k, every, dict(_CLOUD, **on))      # cloud term k exactly on its threshold: score 16, cloudy
            plant(P_TERM0 + 2 * k + 1, every, dict(_CLOUD, **below))       # one DN below: score 15, clear
        plant(P_QA10, every, _LAND, 1024)
        plant(P_QA11, every, _LAND, 2048)
        plant(P_SCL0, every, _LAND, 0, 0)
        plant(P_NODATA_BAND, every, dict(_LAND, B11=0))            # a rule band that is nodata where the others are valid
    offsets = np.where(np.arange(t) >= (t + 1) // 2, 1000.0, 0.0).astype(np.float32)
    stack = np.zeros((t, len(bands), npix), np.float64)
    for i, b in enumerate(bands):
        if b in REFL:
            stack[:, i] = np.where(val[b] > 0, val[b] + offsets[:, None].astype(np.int64), 0)
        elif b == 'QA60':
            stack[:, i] = qa
        elif b == 'SCL':
            stack[:, i] = scl
        else:                                                      # a band no rule reads
            stack[:, i] = rng.integers(0, 5000, (t, npix))
    if dtype.kind == 'f' or dtype == np.int16:                     # other spellings of nodata, away from the planted pixels
        refl = np.array([b in REFL for b in bands])
        alt = (rng.random(stack.shape) < 0.5) & (stack == 0) & refl[None, :, None]
        alt[:, :, :PLANTED_PIXELS] = False
        stack[alt] = -rng.integers(1, 3000, int(alt.sum()))
        if dtype.kind == 'f':
            nan = alt & (rng.random(stack.shape) < 0.5)
            stack[nan] = np.nan
            code = np.array([b in ('QA60', 'SCL') for b in bands])
            bad = (rng.random(stack.shape) < 0.02) & code[None, :, None]
            bad[:, :, :PLANTED_PIXELS] = False
            stack[bad] = np.nan                                    # a NaN code fails its rule
    with np.errstate(invalid='ignore'):
        out = stack.astype(dtype)
    return np.ascontiguousarray(out.reshape(t, len(bands), H, W)), offsets
