"""Seeded inputs and the float64 oracle of satcv_convlstm_step_fwd, shared by tests/test_lstm_step_cpu.py and tests/test_lstm_step_gpu.py
(helper module, no tests in it).

Oracle (the issue's): a float64 direct 3x3 'same' convolution (zero padding, per image) of the STORED h_prev and the STORED recurrent
kernel, plus the stored xg, through lstm_kernels_oracle.cell_fwd64.  Everything here is in NATURAL Keras channel order (i, f, c, o blocks
of F); the GPU file permutes xg and the kernel's output channels with lstm_infer.gate_order for the device.

Input scales: h_prev ~ N(0, 0.5^2), kernel ~ N(0, 1 / (9 F)), so conv ~ N(0, 0.5^2); xg ~ N(0, 0.8^2): z ~ N(0, 0.94^2), of order 1 and
about 99 % inside (-2.5, 2.5) -- few gates sit on a corner of the hard sigmoid (the CPU file holds the share below 1 %)."""
import functools

import numpy as np

import lstm_kernels_oracle as O

TILE_H, TILE_W = 8, 16               # pixel patch of one workgroup of csrc/convlstm_step.hip
SMALL, RAGGED = (5, 7), (19, 37)     # smaller than any tile; 3 x 3 tiles, ragged in both directions
N_IMG = 2                            # two images: a halo leaking across the image boundary would show


def _cases():
    """(kind, h, w, F, rec_act, act, t0, pad): pad = extra channels of every leading dimension"""
    out = []
    for kind in ('f32', 'bf16'):
        for F in (16, 64):
            for rec in (0, 1):
                for act in (0, 1):
                    out.append((kind, *SMALL, F, rec, act, False, 8))
            out.append((kind, *RAGGED, F, 0, 0, False, 8))
            out.append((kind, *RAGGED, F, 1, 1, False, 8))
            out.append((kind, *SMALL, F, 0, 1, True, 8))              # t = 0: NULL h_prev and c_prev
        out.append((kind, *RAGGED, 32, 0 if kind == 'bf16' else 1, 0 if kind == 'bf16' else 1, False, 0))
    return out


CASES = _cases()


def case_id(c):
    kind, h, w, F, rec, act, t0, pad = c
    return f'{kind}-{h}x{w}-F{F}-ra{rec}-act{act}' + ('-t0' if t0 else '') + f'-pad{pad}'


def case_seed(c):
    return 1000 + CASES.index(c)


def conv3x3_same64(x, k):
    """x (n, h, w, cin), k (3, 3, cin, cout), float64; zero padding per image"""
    n, h, w, cin = x.shape
    xp = np.zeros((n, h + 2, w + 2, cin))
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((n, h, w, k.shape[-1]))
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + h, kx:kx + w].reshape(-1, cin).dot(k[ky, kx]).reshape(n, h, w, -1)
    return out


@functools.lru_cache(maxsize=None)
def inputs(c):
    """storage-exact float64 arrays: h_prev (n, h, w, F), wr (3, 3, F, 4 F), xg (npix, 4 F), float32-exact c_prev (npix, F); None at t = 0"""
    kind, h, w, F, rec, act, t0, pad = c
    rng = np.random.default_rng(case_seed(c))
    st = lambda shape, s, k=kind: O.to_storage((rng.standard_normal(shape) * s).astype(np.float32), k)
    npix = N_IMG * h * w
    d = dict(h_prev=st((N_IMG, h, w, F), 0.5), wr=st((3, 3, F, 4 * F), 1.0 / np.sqrt(9 * F)), xg=st((npix, 4 * F), 0.8), c_prev=st((npix, F), 1.0, 'f32'))
    assert np.all(d['h_prev'] != 0)                      # nonzero everywhere: any pixel read across an image or tile boundary counts
    if t0:
        d['h_prev'] = d['c_prev'] = None
    for v in d.values():
        if v is not None:
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(c):
    """-> dict z (npix, 4 F), c64, h64 (npix, F) float64, corner (npix, F) bool: a hard-sigmoid gate of the element within one storage
    rounding of 0 / 1 (O.hard_sigmoid_ambiguous), all False for the sigmoid"""
    kind, h, w, F, rec, act, t0, pad = c
    d = inputs(c)
    z = d['xg'] if t0 else d['xg'] + conv3x3_same64(d['h_prev'], d['wr']).reshape(-1, 4 * F)
    _, _, _, _, c64, h64 = O.cell_fwd64(z, d['c_prev'], rec, act)
    zi, zf, _, zo = O.split4(z)
    corner = np.zeros(c64.shape, bool)
    if rec == 0:
        corner = O.hard_sigmoid_ambiguous(zi, kind) | O.hard_sigmoid_ambiguous(zf, kind) | O.hard_sigmoid_ambiguous(zo, kind)
    out = dict(z=z, c64=c64, h64=h64, corner=corner)
    for v in out.values():
        v.setflags(write=False)
    return out
