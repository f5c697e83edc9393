"""NumPy float64 restatements of the element-wise glue kernels of csrc/elementwise.hip, written from the semantics documented in
include/satcv.h (helper module, no tests in it).  tests/test_elementwise_cpu.py pins each of them to an independent implementation
(torch on the CPU); tests/test_elementwise_gpu.py holds the kernels to them.

All tensors are NHWC; `x64` arguments are float64 arrays whose values are exactly representable in the storage type under test."""
import numpy as np

EW_BLOCK = 256               # threads per workgroup of every grid-stride kernel
EW_PER_CU_DEFAULT = 6        # documented default of SATCV_EW_PER_CU: a launch is capped at 256 * 6 workgroups
E4M3_MAX = 448.0


def grid_cap_threads(per_cu=EW_PER_CU_DEFAULT):
    """threads of the largest launch: a kernel with more work items than this takes a second trip round its grid-stride loop"""
    return 256 * per_cu * EW_BLOCK


def close_tol(kind):
    """the project's op-level bounds (tests/test_ops_gpu.py close()): relative to the largest reference magnitude"""
    return 2e-5 if kind == 'f32' else 1.2e-2


def close_err(got, ref):
    scale = max(np.abs(ref).max(), 1e-6)
    return np.abs(np.asarray(got, np.float64) - ref).max() / scale, scale


# ------------------------------------------------------------------------- max pool
def pool_out(h, k, s, pad):
    return (h + 2 * pad - k) // s + 1


def maxpool(x, k, s, pad):
    """window k, stride s, symmetric padding with -inf; output size floor((h + 2 pad - k) / s) + 1"""
    n, h, w, c = x.shape
    ho, wo = pool_out(h, k, s, pad), pool_out(w, k, s, pad)
    assert ho > 0 and wo > 0
    xp = np.full((n, h + 2 * pad, w + 2 * pad, c), -np.inf)
    xp[:, pad:pad + h, pad:pad + w] = x
    out = np.full((n, ho, wo, c), -np.inf)
    for i in range(k):
        for j in range(k):
            out = np.maximum(out, xp[:, i:i + (ho - 1) * s + 1:s, j:j + (wo - 1) * s + 1:s])
    return out


# ----------------------------------------------------------- residual join, ReLU backward, bias gradient
def affine(x, scale=None, shift=None, relu=False):
    a = x if scale is None else x * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return np.maximum(a, 0.0) if relu else a


def add_act(y, y_scale, y_shift, res, res_scale, res_shift, relu):
    """relu?(affine?(y) + affine?(res))"""
    return affine(affine(y, y_scale, y_shift) + affine(res, res_scale, res_shift), relu=bool(relu))


def relu_bwd(act, g):
    """g where act > 0, else +0 (so -0.0, +0.0, negative activations all block the gradient)"""
    return np.where(act > 0, g, 0.0)


def bias_grad(dy):
    """sum over every pixel, per channel"""
    return dy.reshape(-1, dy.shape[-1]).sum(0)


def bias_grad_bound(dy):
    """order-independent bound of an fp32 sum of npix terms: (npix - 1) 2^-24 sum|dy| per channel"""
    a = np.abs(dy.reshape(-1, dy.shape[-1]))
    return (a.shape[0] - 1) * 2.0 ** -24 * a.sum(0)


# ---------------------------------------------------------------- up-sampling head
def _src(o, f, size):
    s = np.clip((np.arange(o) + 0.5) / f - 0.5, 0.0, size - 1.0)          # half-pixel centres, edge clamped
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), s - i0


def upsample_bilinear(x, f):
    n, h, w, c = x.shape
    y0, y1, fy = _src(h * f, f, h)
    x0, x1, fx = _src(w * f, f, w)
    fy, fx = fy[None, :, None, None], fx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - fx) + x[:, y0][:, :, x1] * fx
    bot = x[:, y1][:, :, x0] * (1 - fx) + x[:, y1][:, :, x1] * fx
    return top * (1 - fy) + bot * fy


def upsample_head(logits, f, activation, thresh=0.5):
    """-> probs (n, hf, wf, ncls), classes, margin.  activation 0: softmax, classes (n, hf, wf) = argmax, lowest index on ties, margin =
    best minus second-best probability (inf for one class); 1: sigmoid, classes (n, hf, wf, ncls) = probs > thresh, margin = |probs - thresh|."""
    z = upsample_bilinear(logits, f)
    if activation == 0:
        e = np.exp(z - z.max(-1, keepdims=True))
        p = e / e.sum(-1, keepdims=True)
        cls = p.argmax(-1).astype(np.int32)
        if p.shape[-1] == 1:
            margin = np.full(cls.shape, np.inf)
        else:
            srt = np.sort(p, -1)
            margin = srt[..., -1] - srt[..., -2]
        return p, cls, margin
    p = 1.0 / (1.0 + np.exp(-z))
    return p, (p > np.float64(np.float32(thresh))).astype(np.int32), np.abs(p - np.float64(np.float32(thresh)))


# ----------------------------------------------------------------------- dropout
def dropout_keep_value(rate):
    """the non-zero mask value float32(1 / (1 - rate)), rate as the float32 the C ABI receives"""
    return np.float32(1.0 / (1.0 - np.float64(np.float32(rate))))


def dropout_apply(x, mask, mode, hw, scale=None, shift=None, relu=False):
    """x (npix, c); mask (n, c) for mode 0 (whole feature maps: pixel p uses row p // hw) or (npix, c) for mode 1"""
    a = affine(x, scale, shift, relu) if scale is not None else x
    m = mask[np.arange(x.shape[0]) // hw] if mode == 0 else mask
    return a * m


def five_sigma(rate, n):
    return 5.0 * np.sqrt(rate * (1.0 - rate) / n)


# ----------------------------------------------------------------- e4m3 rounding
def _e4m3_table():
    """every finite non-negative OCP e4m3fn value, ascending, and its byte code"""
    vals = []
    for code in range(0x7f):                                   # 0x7f is NaN
        e, m = code >> 3, code & 7
        vals.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7))
    return np.array(vals), np.arange(0x7f, dtype=np.uint8)


_E4M3_VALS, _E4M3_CODES = _e4m3_table()


def e4m3_decode(codes):
    c = np.asarray(codes, np.uint8)
    v = _E4M3_VALS[np.minimum(c & 0x7f, 0x7e)]
    v = np.where((c & 0x7f) == 0x7f, np.nan, v)
    return np.where(c & 0x80, -v, v)


def e4m3_round(v):
    """saturating round-to-nearest-even of float64 values -> byte codes"""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), E4M3_MAX)
    hi = np.clip(np.searchsorted(_E4M3_VALS, a, side='left'), 1, len(_E4M3_VALS) - 1)
    lo = hi - 1
    mid = 0.5 * (_E4M3_VALS[lo] + _E4M3_VALS[hi])
    up = (a > mid) | ((a == mid) & (_E4M3_CODES[lo] & 1 == 1))            # ties to the even code
    code = np.where(up, _E4M3_CODES[hi], _E4M3_CODES[lo]).astype(np.uint8)
    return code | np.where(np.signbit(v), 0x80, 0).astype(np.uint8)


def f32_ulp(v):
    """float32 unit in the last place at magnitude |v| (normal range)"""
    return np.spacing(np.maximum(np.abs(v), 2.0 ** -126).astype(np.float32)).astype(np.float64)


def affine_requant_fp8(x, scale, shift, relu):
    """-> (value, lo, hi, ambiguous), all decoded e4m3 values: the rounding of relu?(scale x + shift) evaluated in float64, and the roundings
    of the same expression moved down / up by the rounding error of the kernel's float32 arithmetic; `ambiguous` marks the elements where
    they differ, i.e. where the float64 value sits within that error of a rounding boundary and either neighbour is right.  The float32
    result differs from the exact one by at most half an ulp of the product plus half an ulp of the sum (none of the product if the
    compiler contracts scale x + shift into one FMA): one float32 ulp at max(|scale x|, |shift|, |value|)."""
    prod = x * np.asarray(scale, np.float64)
    pre = affine(x, scale, shift)
    err = f32_ulp(np.maximum(np.maximum(np.abs(prod), np.abs(np.asarray(shift, np.float64))), np.abs(pre)))
    act = (lambda a: np.maximum(a, 0.0)) if relu else (lambda a: a)
    val, lo, hi = (e4m3_decode(e4m3_round(act(pre + d))) for d in (0.0, -err, err))
    return val, lo, hi, lo != hi


# ------------------------------------------------------------------------ ingest
def ingest_scaled_f32(src, cpad, mul):
    """(npix, c) float32 -> (npix, cpad) float32 BEFORE the storage rounding: one float32 multiply, pad channels zero"""
    out = np.zeros((src.shape[0], cpad), np.float32)
    out[:, :src.shape[1]] = src.astype(np.float32) * np.float32(mul)
    return out


# ------------------------------------------------------------------- head backward
def head_bwd(x, in_scale, in_shift, w, dlogits):
    """Conv2D(ncls, (1, 1)) on a = relu(in_scale x + in_shift) (a = x without in_scale): dx is the gradient w.r.t. the ACTIVATED input,
    dw (cin, ncls), db (ncls)"""
    a = affine(x, in_scale, in_shift, relu=True) if in_scale is not None else x
    return dlogits @ np.asarray(w, np.float64).T, a.T @ dlogits, dlogits.sum(0)


# --------------------------------------------------------------------- confusion
def confusion(classes, y_true, ncls):
    """conf[t, p] += 1 with t = argmax of the one-hot (or soft) label row, first maximum"""
    conf = np.zeros((ncls, ncls), np.int64)
    np.add.at(conf, (y_true.reshape(-1, ncls).argmax(-1), np.asarray(classes).reshape(-1)), 1)
    return conf


# ------------------------------------------------- cases shared by the CPU and the GPU file (same seeds, same shapes)
def _past_cap_rows(per_row):
    """smallest row count with at least two full trips of the grid-stride loop at the default launch cap"""
    return -(-2 * grid_cap_threads() // per_row)


def upsample_cases():
    """(n, h, w, ncls, factor, activation, thresh)"""
    cases = [(1, 4, 4, 2, 1, 0, 0.5), (2, 5, 7, 2, 2, 0, 0.5), (3, 5, 3, 3, 3, 0, 0.5), (1, 6, 4, 4, 4, 0, 0.5), (1, 3, 5, 2, 16, 0, 0.5),
             (2, 1, 9, 2, 4, 0, 0.5), (2, 9, 1, 3, 2, 0, 0.5), (1, 1, 1, 2, 3, 0, 0.5), (3, 7, 5, 1, 2, 1, 0.5), (1, 6, 6, 1, 4, 1, 0.3),
             (2, 3, 3, 4, 3, 1, 0.3)]
    cases += [(3, 3, 5, k, 2, 0, 0.5) for k in range(1, 9)]
    w, f = 60, 16
    cases.append((1, _past_cap_rows(w * f * f), w, 2, f, 0, 0.5))             # output pixels past the launch cap
    return cases


def upsample_logits(case):
    n, h, w, ncls = case[:4]
    rng = np.random.default_rng(abs(hash(tuple(case))) % 2 ** 31)
    return (rng.standard_normal((n, h, w, ncls)) * 2.0).astype(np.float32)


REQUANT_PAIRS = [('f32', 'f32'), ('bf16', 'bf16'), ('fp8', 'fp8'), ('f32', 'fp8'), ('bf16', 'fp8'), ('fp8', 'bf16')]
REQUANT_SHAPES = [(64, 8), (3 * 7 * 5, 24), (1031, 40)]                      # (npix, c); the GPU file adds one past the launch cap


def bf16_round(x):
    """float32 -> nearest-even bfloat16, returned as float32 (finite values)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def to_storage(x, kind):
    """float32 array -> float64 array of the values the storage type `kind` ('f32', 'bf16', 'fp8') holds for it"""
    if kind == 'bf16':
        return bf16_round(x).astype(np.float64)
    if kind == 'fp8':
        return e4m3_decode(e4m3_round(np.asarray(x, np.float64)))
    return np.asarray(x, np.float32).astype(np.float64)


def requant_inputs(npix, c, kind, seed):
    """x (float64, exactly representable in the input storage type `kind`), float32 scale, shift.  The results span the e4m3 range and
    exceed it: a few per cent of |scale x + shift| lie beyond 448."""
    rng = np.random.default_rng(seed)
    x = to_storage((rng.standard_normal((npix, c)) * 40.0).astype(np.float32), kind)
    scale = rng.uniform(0.5, 5.0, c).astype(np.float32) * rng.choice([-1.0, 1.0], c).astype(np.float32)
    shift = (rng.standard_normal(c) * 20.0).astype(np.float32)
    return x, scale, shift
