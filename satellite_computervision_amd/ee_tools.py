"""The per-sample quality masks of the reference's utils/ee_tools.py on arrays instead of Earth Engine images: what every composite
its models were trained on was masked with before the median.

    basicQA            :159-180   QA60 cloud and cirrus bits
    sentinelCloudScore :218-255   the custom cloud likelihood, 0 ... 100; maskTOA :288-306 keeps `cloudScore <= 15`
    waterScore         :115-157   the water likelihood, [0, 1]; mask :257-268 keeps `<= 0.25` and `B11 > 900` (shadow)
    maskSR             :270-286   QA60 and the scene classification (SCL)

All of it is ONE kernel (satcv_quality_mask, csrc/quality.hip) over a (T, C, H, W) stack that is uploaded once; the masks leave it as
uint32 bit-planes (`ClearMask`) that `pc_tools.median_composite(clear=...)` reads on the device.  The Cloud Displacement Index and the
JRC surface-water history that `mask` also consults are external products and stay with the caller, as the reference's own maskTOA
leaves them out.  The exact definition of every rule (integer arithmetic, nodata, zero denominators) is in include/satcv.h.

Each function takes `(stack, bands, offsets=None, times=None)`: `stack` as `pc_tools.median_composite` takes it, `bands` the names of
its planes (`B01` / `B1` and `B08` / `B8` are both accepted), `offsets` / `times` the harmonisation (applied to the reflectance bands
only).  Nothing here synchronises with the host.
"""
import numpy as np

from . import pc_tools

QA60, CLOUD, SHADOW, WATER, SCL = 1, 2, 4, 8, 16         # SATCV_Q_* of include/satcv.h
ROLES = ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11', 'B12', 'QA60', 'SCL')
RULE_NAMES = {'qa60': QA60, 'cloud': CLOUD, 'shadow': SHADOW, 'water': WATER, 'scl': SCL}
# maskTOA :300-306, maskSR :279-286, mask :262-268 (without CDI and JRC)
PRESETS = {'toa': QA60 | CLOUD, 'sr': QA60 | SCL, 'mask': QA60 | CLOUD | SHADOW | WATER}
# the reflectance roles each rule reads (a rule without its roles is refused before any launch)
RULE_ROLES = {QA60: ('QA60',), CLOUD: ('B1', 'B2', 'B3', 'B4', 'B8', 'B10', 'B11'), SHADOW: ('B11',),
              WATER: ('B2', 'B3', 'B4', 'B8', 'B11', 'B12'), SCL: ('SCL',)}
CLOUD_MAX, SHADOW_MIN = 15, 900.0                          # maskTOA :301, mask :267


def canonical_band(name):
    """'B01' -> 'B1', 'b08' -> 'B8'; 'B8A', 'QA60', 'SCL' and everything else: upper case, unchanged"""
    n = str(name).strip().upper()
    if len(n) == 3 and n[0] == 'B' and n[1] == '0' and n[2].isdigit():
        n = 'B' + n[2]
    return n


def band_table(bands):
    """the plane of each role of `ROLES` among the plane names `bands`, -1 for a role that is absent"""
    names = [canonical_band(b) for b in bands]
    if len(set(names)) != len(names):
        raise ValueError(f'band names repeat: {list(bands)}')
    return [names.index(r) if r in names else -1 for r in ROLES]


def rule_set(rules):
    """'toa' / 'sr' / 'mask', a SATCV_Q_* bit set, one rule name or an iterable of rule names -> the bit set"""
    if isinstance(rules, str):
        key = rules.lower()
        if key in PRESETS:
            return PRESETS[key]
        if key in RULE_NAMES:
            return RULE_NAMES[key]
        raise ValueError(f'unknown rule set {rules!r}: one of {sorted(PRESETS)} or of {sorted(RULE_NAMES)}')
    if isinstance(rules, (int, np.integer)):
        if rules <= 0 or rules & ~31:
            raise ValueError(f'rule bit set {rules}: a non-empty combination of QA60 1, CLOUD 2, SHADOW 4, WATER 8, SCL 16')
        return int(rules)
    out = 0
    for r in rules:
        if str(r).lower() not in RULE_NAMES:
            raise ValueError(f'unknown rule {r!r}: one of {sorted(RULE_NAMES)}')
        out |= RULE_NAMES[str(r).lower()]
    if not out:
        raise ValueError('an empty rule set')
    return out


def _require(table, bits, bands):
    for rule, roles in RULE_ROLES.items():
        if bits & rule:
            missing = [r for r in roles if table[ROLES.index(r)] < 0]
            if missing:
                name = [k for k, v in RULE_NAMES.items() if v == rule][0]
                raise ValueError(f'rule {name} reads {", ".join(missing)}, absent from bands {list(bands)}')


class ClearMask:
    """The clear bits of a (T, H, W) stack on the device: `words` is (ceil(T / 32), H, W) int32 holding the uint32 bit-planes of
    satcv_quality_mask -- bit j % 32 of word j / 32 is 1 when acquisition j passes every selected rule at that pixel."""

    def __init__(self, words, t):
        self.words, self.T = words, int(t)
        if words.dim() != 3 or words.shape[0] != (self.T + 31) // 32:
            raise ValueError(f'{self.T} acquisitions need ({(self.T + 31) // 32}, H, W) words, got {tuple(words.shape)}')

    @property
    def shape(self):
        return (self.T,) + tuple(self.words.shape[1:])

    def numpy(self):
        """(T, H, W) bool on the host"""
        w = self.words.cpu().numpy().view(np.uint32)
        j = np.arange(self.T)
        return ((w[j // 32] >> (j % 32).astype(np.uint32)[:, None, None]) & 1).astype(bool)

    def count(self):
        """(H, W) clear acquisitions per pixel, on the host"""
        return self.numpy().sum(axis=0, dtype=np.int32)


def _quality(src, kind, table, bits, off_dev, clear=False, cloud=False, water=False, cloud_max=CLOUD_MAX, shadow_min=SHADOW_MIN):
    """one launch of satcv_quality_mask on a resident stack -> (ClearMask | None, cloud score | None, water score | None)"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import Q_ROLES, QualityDesc, check, lib
    from .prediction_tools import _device_empty
    T, cs, H, W = (int(v) for v in src.shape)
    words = _device_empty(((T + 31) // 32, H, W), torch.int32, 'the clear bit-planes') if clear else None
    cl = _device_empty((T, H, W), torch.uint8, 'the cloud score') if cloud else None
    wa = _device_empty((T, H, W), torch.float32, 'the water score') if water else None
    d = QualityDesc(src=src.data_ptr(), src_kind=kind, t=T, cs=cs, h=H, w_=W, offsets=off_dev.data_ptr() if off_dev is not None else None,
                    band=(C.c_int32 * len(Q_ROLES))(*table), rules=int(bits), cloud_max=int(cloud_max), shadow_min=float(shadow_min),
                    clear=words.data_ptr() if clear else None, cloud_score=cl.data_ptr() if cloud else None,
                    water_score=wa.data_ptr() if water else None)
    check(lib.satcv_quality_mask(C.byref(d), ops.stream_ptr()))
    return (ClearMask(words, T) if clear else None), cl, wa


def _run(stack, bands, offsets, times, bits, **outputs):
    if getattr(stack, 'ndim', 0) != 4:
        raise ValueError(f'expected a (T, C, H, W) stack, got shape {tuple(getattr(stack, "shape", ()))}')
    if len(bands) != int(stack.shape[1]):
        raise ValueError(f'{int(stack.shape[1])} planes need {int(stack.shape[1])} band names, got {len(bands)}')
    table = band_table(bands)
    need = bits | (CLOUD if outputs.get('cloud') else 0) | (WATER if outputs.get('water') else 0)
    _require(table, need, bands)
    if int(stack.shape[1]) > 16:
        raise ValueError(f'{int(stack.shape[1])} planes per acquisition: the quality kernel takes at most 16')
    off_dev = pc_tools._offsets_to_device(int(stack.shape[0]), times, offsets)
    src, kind = pc_tools._stack_to_device(stack)
    return _quality(src, kind, table, bits, off_dev, **outputs)


def sentinelCloudScore(stack, bands, offsets=None, times=None):
    """`sentinelCloudScore` (:218-255): (T, H, W) uint8 CUDA tensor, 0 ... 100; 255 where a band the score reads is nodata."""
    return _run(stack, bands, offsets, times, 0, cloud=True)[1]


def waterScore(stack, bands, offsets=None, times=None):
    """`waterScore` (:115-157): (T, H, W) float32 CUDA tensor in [0, 1]; NaN where a band the score reads is nodata."""
    return _run(stack, bands, offsets, times, 0, water=True)[2]


def basicQA(stack, bands, offsets=None, times=None):
    """`basicQA` (:159-180): the `ClearMask` of QA60 bits 10 (cloud) and 11 (cirrus) both being 0."""
    return _run(stack, bands, offsets, times, QA60, clear=True)[0]


def maskTOA(stack, bands, offsets=None, times=None):
    """`maskTOA` (:288-306): basicQA and `cloudScore <= 15`."""
    return _run(stack, bands, offsets, times, PRESETS['toa'], clear=True)[0]


def maskSR(stack, bands, offsets=None, times=None):
    """`maskSR` (:270-286): basicQA and SCL none of 2, 3 (dark, shadow), 8, 9 (cloud), 10 (cirrus), 11 (snow); SCL 0 is nodata."""
    return _run(stack, bands, offsets, times, PRESETS['sr'], clear=True)[0]


def mask(stack, bands, offsets=None, times=None, rules='mask', cloud_max=CLOUD_MAX, shadow_min=SHADOW_MIN):
    """`mask` (:257-268) without its external products (CDI, JRC): basicQA, `cloudScore <= 15`, `B11 > 900`, not water
    (`waterScore <= 0.25`: not all three water terms above 1/4).  rules: another rule set, see `rule_set`."""
    return _run(stack, bands, offsets, times, rule_set(rules), clear=True, cloud_max=cloud_max, shadow_min=shadow_min)[0]


def rescale(img, exp, thresholds):
    """`rescale` (:110-113) on an array: `(exp(img) - thresholds[0]) / (thresholds[1] - thresholds[0])`; exp: 'img' (the array itself,
    the only expression the scores use on a single band) or a callable of the array."""
    x = img if exp == 'img' else exp(img)
    return (x - thresholds[0]) / (thresholds[1] - thresholds[0])


def sentinel2toa(stack, bands):
    """`sentinel2toa` (:90-108) on a (..., C, H, W) host array: the reflectance planes divided by 10000 as float64, QA60 (and SCL)
    unchanged.  A plain array helper: the kernels work on the DN and carry the factor in their constants."""
    x = np.asarray(stack).astype(np.float64)
    for i, b in enumerate(bands):
        if canonical_band(b) not in ('QA60', 'SCL'):
            x[..., i, :, :] /= 10000.0
    return x
