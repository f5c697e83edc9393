"""NumPy float64 restatements of the five entry points of csrc/convlstm.hip (satcv_ingest_seq, satcv_convlstm_gates_fwd / _bwd,
satcv_dense_small_fwd / _bwd), written from the semantics documented in include/satcv.h (helper module, no tests in it).
tests/test_lstm_kernels_cpu.py pins each of them to torch float64 autograd and to oracle/convlstm.py; tests/test_lstm_kernels_gpu.py
holds the kernels to them.

`x64` arguments are float64 arrays whose values are exactly representable in the storage type under test.  Gate order along the 4 F
channels is i, f, g (the Keras "c" gate), o."""
import numpy as np

from elementwise_oracle import bf16_round, close_err, close_tol, to_storage  # noqa: F401  (re-exported to the two test files)

LSTM_BLOCK = 256
LSTM_CAP_ITEMS = 256 * 8 * LSTM_BLOCK        # lstm_grid(): at most 2048 workgroups of 256 threads; more items take a second trip
DENSE_LANE_CAP_BLOCKS = 1024                 # satcv_dense_small_bwd's lane kernel: at most 1024 workgroups of pl * 16 pixels
STAT_ROWS = 32


# ---------------------------------------------------------------------------- ingest
def ingest_seq(src, cpad, kind):
    """(B, T, H, W, C) float32 -> (T, B, H, W, cpad) in the storage type, pad channels zero"""
    b, t, h, w, c = src.shape
    out = np.zeros((t, b, h, w, cpad), np.float32)
    out[..., :c] = np.asarray(src, np.float32).transpose(1, 0, 2, 3, 4)
    return to_storage(out, kind)


# ----------------------------------------------------------------------------- gates
def rec_act(z, kind):
    """kind 0 hard_sigmoid = clip(0.2 z + 0.5, 0, 1), 1 sigmoid"""
    return np.clip(0.2 * z + 0.5, 0.0, 1.0) if kind == 0 else 1.0 / (1.0 + np.exp(-z))


def cell_act(z, kind):
    """kind 0 linear, 1 tanh"""
    return np.tanh(z) if kind else z


def split4(a):
    f = a.shape[-1] // 4
    return a[..., :f], a[..., f:2 * f], a[..., 2 * f:3 * f], a[..., 3 * f:]


def cell_fwd64(z, c_prev, rec_kind, act_kind):
    """-> i, f, g, o, c, h in float64, nothing rounded"""
    zi, zf, zg, zo = split4(z)
    i, f, o = rec_act(zi, rec_kind), rec_act(zf, rec_kind), rec_act(zo, rec_kind)
    g = cell_act(zg, act_kind)
    c = i * g if c_prev is None else f * c_prev + i * g
    return i, f, g, o, c, o * cell_act(c, act_kind)


def gates_fwd(xg, hg, c_prev, rec_kind, act_kind, kind):
    """xg, hg (npix, 4 F) (hg None at t = 0), c_prev (npix, F) or None.  -> dict: c (float32 storage), h and gates rounded to the storage
    type, h64 / gates64 / c64 the same before any rounding, s1 / s2 the per-channel sum and sum of squares of the STORED h"""
    z = xg if hg is None else xg + hg
    i, f, g, o, c, h = cell_fwd64(z, c_prev, rec_kind, act_kind)
    gates64 = np.concatenate([i, f, g, o], -1)
    hs = to_storage(h.astype(np.float32), kind)
    return dict(c64=c, c=to_storage(c.astype(np.float32), 'f32'), h64=h, h=hs, gates64=gates64, gates=to_storage(gates64.astype(np.float32), kind),
                s1=hs.sum(0), s2=(hs * hs).sum(0))


def stat_bound(v):
    """order-independent bound of a float32 sum of the rows of v (count, F): (count - 1) 2^-24 sum|v| per channel"""
    a = np.abs(v)
    return (a.shape[0] - 1) * 2.0 ** -24 * a.sum(0)


def rec_act_grad_from_value(y, kind):
    """the header's rule: the hard sigmoid has slope 0.2 where its STORED value lies strictly inside (0, 1)"""
    return np.where((y > 0.0) & (y < 1.0), 0.2, 0.0) if kind == 0 else y * (1.0 - y)


def rec_act_grad_from_z(z, kind):
    """the rule of oracle/convlstm.py: from the pre-activation"""
    if kind == 0:
        return np.where((z > -2.5) & (z < 2.5), 0.2, 0.0)
    y = rec_act(z, 1)
    return y * (1.0 - y)


def _cell_bwd(dh, dc_next, i, f, g, o, c_prev, c, si, sf, so, act_kind):
    ac = cell_act(c, act_kind)
    dc = dh * o * ((1.0 - ac * ac) if act_kind else 1.0)
    if dc_next is not None:
        dc = dc + dc_next
    di = dc * g * si
    df = np.zeros_like(di) if c_prev is None else dc * c_prev * sf
    dg = dc * i * ((1.0 - g * g) if act_kind else 1.0)
    do = dh * ac * so
    return np.concatenate([di, df, dg, do], -1), dc * f


def gates_bwd(dh_a, dh_b, dc_next, gates, c_prev, c, rec_kind, act_kind):
    """from the given STORED inputs: dh = dh_a + dh_b (either may be None), gates (npix, 4 F) post-activation, c_prev / dc_next None at the
    ends of the sequence.  -> dz (npix, 4 F), dc_prev (npix, F), float64"""
    dh = sum(d for d in (dh_a, dh_b) if d is not None)
    i, f, g, o = split4(gates)
    s = [rec_act_grad_from_value(y, rec_kind) for y in (i, f, o)]
    return _cell_bwd(dh, dc_next, i, f, g, o, c_prev, c, s[0], s[1], s[2], act_kind)


def gates_bwd_from_z(dh, dc_next, z, c_prev, rec_kind, act_kind):
    """the float64 cell end to end: forward from the pre-activations z, slopes by the pre-activation rule"""
    i, f, g, o, c, _ = cell_fwd64(z, c_prev, rec_kind, act_kind)
    zi, zf, _, zo = split4(z)
    s = [rec_act_grad_from_z(v, rec_kind) for v in (zi, zf, zo)]
    return _cell_bwd(dh, dc_next, i, f, g, o, c_prev, c, s[0], s[1], s[2], act_kind)


def bf16_half_ulp(v):
    """largest error of ONE round-to-nearest bfloat16 conversion of v (8 significant bits): 2^(floor(log2 |v|) - 8), 0 at 0"""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.where(a > 0, 2.0 ** (e - 8), 0.0)


def storage_bound(ref64, kind):
    """per-element bound of a value computed in float32 and stored as `kind`: the float32 op-level bound (relative to the largest
    reference magnitude) plus, for bf16, one bf16 rounding of the float64 value"""
    base = close_tol('f32') * max(np.abs(ref64).max(), 1e-6)
    return base + (bf16_half_ulp(ref64) if kind == 'bf16' else 0.0)


# margin within which the float32 evaluation of u = 0.2 z + 0.5 can land on the other side of 0 or 1: |u| <= 0.5 + 0.2 |z| < 4 for the
# inputs used here (|z| < 16), three roundings (the sum z = xg + hg, the product, the sum) of at most 2^-24 * 4 each -> 3 * 2^-22 < 2^-20
F32_GATE_MARGIN = 2.0 ** -20


def hard_sigmoid_ambiguous(z, kind):
    """elements whose float64 hard-sigmoid value lies within one storage rounding of 0 or 1, where the value rule and the pre-activation
    rule may disagree: the stored value is exactly 0 / 1 while z is strictly inside (-2.5, 2.5), or the reverse.  bf16 rounds every value in
    [1 - 2^-9, 1) up to 1 (half a bf16 ulp below 1); near 0 bf16 is as fine as float32."""
    u = 0.2 * z + 0.5
    below_one = F32_GATE_MARGIN + (2.0 ** -9 if kind == 'bf16' else 0.0)
    return (np.abs(u) <= F32_GATE_MARGIN) | ((u >= 1.0 - below_one) & (u <= 1.0 + F32_GATE_MARGIN))


def composed_ambiguous(z, kind):
    """(npix, 4 F) mask of the dz elements of the composed test that hard_sigmoid_ambiguous sets aside (the g gate has no such rule)"""
    zi, zf, zg, zo = split4(z)
    return np.concatenate([hard_sigmoid_ambiguous(zi, kind), hard_sigmoid_ambiguous(zf, kind), np.zeros(zg.shape, bool), hard_sigmoid_ambiguous(zo, kind)], -1)


# --------------------------------------------------------------------------- nearest
def nn_index(n_in, n_out, form):
    """source index of every destination index of a nearest-neighbour resize with half-pixel centres, min(floor((i + 0.5) in / out), in - 1).
    'exact': integer arithmetic, ((2 i + 1) in) // (2 out).  'tf32': the float32 evaluation (i + 0.5f) * (in / (float) out), then floorf."""
    i = np.arange(n_out)
    if form == 'exact':
        return np.minimum(((2 * i + 1) * n_in) // (2 * n_out), n_in - 1).astype(np.int64)
    assert form == 'tf32'
    scale = np.float32(n_in) / np.float32(n_out)
    s = np.floor((i.astype(np.float32) + np.float32(0.5)) * scale)
    assert s.dtype == np.float32
    return np.minimum(s.astype(np.int64), n_in - 1)


def nn_forms_agree(n_in, n_out):
    return bool(np.array_equal(nn_index(n_in, n_out, 'exact'), nn_index(n_in, n_out, 'tf32')))


# ----------------------------------------------------------------------- dense heads
class Src:
    """one source of a dense head: x (nimg, hs, ws, cin) float64 (storage-exact), optional pending scale / shift (+ ReLU), `resized`
    when it sits on its own grid and is read through the nearest index maps"""

    def __init__(self, x, scale=None, shift=None, relu=False, resized=False):
        self.x, self.scale, self.shift, self.relu, self.resized = x, scale, shift, relu, resized

    def activated(self):
        a = self.x
        if self.scale is not None:
            a = a * np.asarray(self.scale, np.float64) + np.asarray(self.shift, np.float64)
            if self.relu:
                a = np.maximum(a, 0.0)
        return a


def _maps(s, h, w, form):
    return nn_index(s.x.shape[1], h, form), nn_index(s.x.shape[2], w, form)


def dense_concat(srcs, h, w, form='tf32'):
    """the activated sources on the output grid, concatenated: (nimg, h, w, sum cin)"""
    cols = []
    for s in srcs:
        a = s.activated()
        if s.resized:
            iy, ix = _maps(s, h, w, form)
            a = a[:, iy][:, :, ix]
        assert a.shape[1:3] == (h, w)
        cols.append(a)
    return np.concatenate(cols, -1)


def dense_fwd(srcs, w, b, activation, max_value, h, w_, form='tf32'):
    """w (sum cin, cout), b (cout).  activation 0 softmax, 1 sigmoid, 2 linear, 3 ReLU clipped at max_value (<= 0: not clipped).
    -> z, out (npix, cout), classes (npix; argmax of the first maximum), margin (best minus second-best probability, inf for one class)"""
    a = dense_concat(srcs, h, w_, form)
    z = a.reshape(-1, a.shape[-1]) @ np.asarray(w, np.float64) + np.asarray(b, np.float64)
    if activation == 0:
        e = np.exp(z - z.max(-1, keepdims=True))
        out = e / e.sum(-1, keepdims=True)
    elif activation == 1:
        out = 1.0 / (1.0 + np.exp(-z))
    elif activation == 2:
        out = z
    else:
        out = np.maximum(z, 0.0)
        if max_value > 0:
            out = np.minimum(out, max_value)
    srt = np.sort(out, -1)
    margin = srt[:, -1] - srt[:, -2] if out.shape[1] > 1 else np.full(out.shape[0], np.inf)
    return z, out, out.argmax(-1).astype(np.int32), margin


def relu_mask(out, max_value):
    return (out > 0.0) & ((out < max_value) if max_value > 0 else True)


def dense_bwd(srcs, w, dout, out, activation, max_value, h, w_, form='tf32', dz=None):
    """activation 2: dz = dout; 3: dz = dout where 0 < out (< max_value); a given `dz` replaces both.  -> dict dz, dw, db, dw_abs / db_abs (the sums of the absolute
    terms, for the derived bound), dx: per source the gradient of its ACTIVATED values on its own grid (scatter-add over the index maps;
    a source pixel with an empty pre-image gets 0)"""
    assert activation in (2, 3)
    w = np.asarray(w, np.float64)
    if dz is None:
        dz = dout * relu_mask(out, max_value) if activation == 3 else dout.copy()
    a = dense_concat(srcs, h, w_, form)
    a2 = a.reshape(-1, a.shape[-1])
    res = dict(dz=dz, dw=a2.T @ dz, db=dz.sum(0), dw_abs=np.abs(a2).T @ np.abs(dz), db_abs=np.abs(dz).sum(0), dx=[])
    da = (dz @ w.T).reshape(a.shape)
    row = 0
    for s in srcs:
        cin = s.x.shape[-1]
        d = da[..., row:row + cin]
        if s.resized:
            iy, ix = _maps(s, h, w_, form)
            dx = np.zeros(s.x.shape)
            np.add.at(dx, (slice(None), iy[:, None], ix[None, :]), d)
            d = dx
        res['dx'].append(d)
        row += cin
    return res


def sum_bound(nterms, abs_sum, prefill=0.0):
    """(n - 1) 2^-24 sum|terms| of a float32 sum in any order; a pre-filled accumulator counts as one more term"""
    extra = 1 if np.any(prefill) else 0
    return (nterms - 1 + extra) * 2.0 ** -24 * (abs_sum + np.abs(prefill))


# --------------------------------------------------------- cases shared by the CPU and the GPU file (same seeds, same shapes)
# (hs, ws, h, w): integer upsample, non-integer upsample, downsample, non-integer downsample, and two pairs on which the float32 and the
# exact index map differ
RESIZE_PAIRS = [(4, 4, 8, 8), (5, 5, 16, 16), (8, 8, 4, 4), (7, 7, 5, 5), (14, 4, 23, 8), (26, 8, 11, 4)]
SPLIT_PAIRS = [(14, 23), (26, 11)]


def size_pairs():
    """every (in, out) pair of RESIZE_PAIRS, rows and columns"""
    return sorted({(hs, h) for hs, _, h, _ in RESIZE_PAIRS} | {(ws, w) for _, ws, _, w in RESIZE_PAIRS})


# composed cell test: (kind, npix, F, rec_act, act, seed).  bf16 keeps the linear cell of every reference call site: with tanh the factor
# 1 - g^2 of a ROUNDED g amplifies one bf16 rounding without bound as g -> 1
COMPOSED = [('f32', 3 * 5 * 7, 16, 0, 1, 11), ('bf16', 2 * 9 * 11, 64, 0, 0, 12)]
GATE_Z_SCALE = 2.0       # z = xg + hg ~ N(0, 2^2 + 1): about a fifth of the gates sit in either clipped arm of the hard sigmoid


def cell_inputs(kind, npix, f, seed, t0=False, scale=GATE_Z_SCALE):
    """storage-exact xg, hg (npix, 4 F), float32-exact c_prev, dc_next (npix, F), storage-exact dh_a, dh_b (npix, F); t0: hg = c_prev = None"""
    rng = np.random.default_rng(seed)
    st = lambda shape, s, k=kind: to_storage((rng.standard_normal(shape) * s).astype(np.float32), k)
    xg, hg = st((npix, 4 * f), scale), st((npix, 4 * f), 1.0)
    c_prev, dc_next = st((npix, f), 1.0, 'f32'), st((npix, f), 1.0, 'f32')
    dh_a, dh_b = st((npix, f), 1.0), st((npix, f), 0.5)
    return dict(xg=xg, hg=None if t0 else hg, c_prev=None if t0 else c_prev, dc_next=dc_next, dh_a=dh_a, dh_b=dh_b)


# dense forward cases of the GPU file: (name, cout, activation, max_value, sources) with a source = (cin, ld, kind, affine, relu, resized)
def dense_cases():
    cases = []
    acts = [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (3, 2.0)]
    for n, (act, mx) in enumerate(acts):
        cout = (1, 3, 16)[n % 3]
        cases.append((f'one-{act}-{mx}', cout, act, mx, [(13, 16, 'f32' if n % 2 else 'bf16', n % 2 == 0, n % 4 == 0, False)]))
        cases.append((f'two-{act}-{mx}', (3, 16, 1)[n % 3], act, mx, [(8, 8, 'bf16', True, True, True), (5, 8, 'f32', n % 2 == 1, False, False)]))
    return cases


def dense_gpu_cases():
    """every (case, pair, nimg, seed) of the GPU file's forward test; the CPU file holds their set-aside shares under the cap"""
    for n, case in enumerate(dense_cases()):
        for m, pair in enumerate(RESIZE_PAIRS):
            if len(case[4]) == 2 or m == 0:                   # one-source cases have nothing to resize
                yield case, pair, 2, 100 + 10 * n + m


def dense_inputs(case, pair, nimg, seed):
    """-> srcs (list of Src), per-source (kind, ld), w, b.  `pair` (hs, ws, h, w) places the resized sources"""
    _, cout, act, mx, specs = case
    hs, ws, h, w_ = pair
    rng = np.random.default_rng(seed)
    srcs, meta = [], []
    for cin, ld, kind, affine, relu, resized in specs:
        shape = (nimg, hs, ws, cin) if resized else (nimg, h, w_, cin)
        x = to_storage(rng.standard_normal(shape).astype(np.float32), kind)
        sc = rng.uniform(0.5, 1.5, cin).astype(np.float32) if affine else None
        sh = (rng.standard_normal(cin) * 0.5).astype(np.float32) if affine else None
        srcs.append(Src(x, sc, sh, relu, resized))
        meta.append((kind, ld))
    rows = sum(s[0] for s in specs)
    wt = (rng.standard_normal((rows, cout)) / np.sqrt(rows)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.5 + (1.0 if act == 3 else 0.0)).astype(np.float32)
    return srcs, meta, wt, b


def relu_ambiguous(z, max_value, tol):
    """ReLU outputs within the float32 bound `tol` of 0 or of max_value: the mask of the backward may go either way"""
    amb = np.abs(z) <= tol
    return amb | (np.abs(z - max_value) <= tol) if max_value > 0 else amb
