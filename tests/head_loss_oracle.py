"""NumPy float64 restatements of the classifier head forward (satcv_head_fwd) and of the loss entry points (satcv_loss_fwd_bwd,
satcv_loss_global_fwd_bwd) of csrc/elementwise.hip, with the error bounds, input builders and case tables their tests share (helper
module, no tests in it).  tests/test_head_loss_cpu.py pins the gradients to torch autograd and checks every builder's condition;
tests/test_head_loss_gpu.py holds the kernels to them.

The five losses are those of oracle/losses.py; this module adds the Jacobian of the head's activation (softmax, sigmoid, linear),
`grad_scale`, and the per-image / global layout of the ratio losses.  `U` = 2^-24 is the unit roundoff of float32."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from elementwise_oracle import EW_BLOCK, affine, close_err, close_tol, grid_cap_threads, to_storage  # noqa: E402,F401
from oracle import keras_ops as K  # noqa: E402
from oracle import losses as OL  # noqa: E402

U = 2.0 ** -24
HEAD_NCMAX = 8
SOFTMAX, SIGMOID, LINEAR = 0, 1, 2
CCE, BCE, DICE, IOU, MSE = 0, 1, 2, 3, 4                     # `kind` of the two loss entry points

# launch geometry (threads of a full launch = the stride of the kernel's pixel loop once the cap is reached)
HEAD_FAST_STRIDE = 1024 * EW_BLOCK                            # head_fwd_fast_kernel: ew_grid(npix, 1024)
LOSS_GENERAL_STRIDE = 1024 * EW_BLOCK                         # loss_kernel: ew_grid(npix, 1024)
GLOBAL_STRIDE = 256 * EW_BLOCK                                # both ratio-loss kernels: at most 256 workgroups per image


def capped_stride():
    """head_fwd_kernel and loss_cce_softmax_kernel: the default cap of the element-wise launches"""
    return grid_cap_threads()


# ------------------------------------------------------------------------------------------------ head forward
# written by hand from head_fast_launch (csrc/elementwise.hip): the register-resident (ncls, cin) forms
HEAD_FAST_FORMS = [(1, 16), (2, 16), (1, 32), (2, 32), (3, 32), (4, 32), (1, 64), (2, 64)]
HEAD_GENERIC_FORMS = [(8, 32), (5, 64), (2, 8), (3, 24), (1, 128)]              # served by the LDS kernel head_fwd_kernel
HEAD_FORMS = HEAD_FAST_FORMS + HEAD_GENERIC_FORMS
HEAD_KINDS = ['f32', 'bf16', 'fp8']                                             # the storage types DISPATCH_T8 admits
HEAD_UNIQUE_ROWS = 4099       # past the launch cap the input repeats these rows (a prime: no stride of a launch is a multiple of it)


def head_shapes():
    """pixel counts: small, ragged (n = 3, h = 7, w = 9), past the launch cap of either head kernel"""
    return [8 * 8, 3 * 7 * 9, 2 * grid_cap_threads() + 3]


def head_inputs(ncls, cin, kind, seed=0):
    """x (HEAD_UNIQUE_ROWS, cin) float64 as stored in `kind`, float32 w (cin, ncls), b, in_scale, in_shift.  The rows whose class the margin
    masks below set aside (for either input form, the argmax, or the thresholds 0.5 and 0.3) come last, so that the share set aside stays
    under 1 % for the small shapes too, which are the first rows; nothing is removed."""
    rng = np.random.default_rng(1000 * ncls + cin + seed)
    x = to_storage(rng.standard_normal((HEAD_UNIQUE_ROWS, cin)).astype(np.float32), kind)
    w = (rng.standard_normal((cin, ncls)) * 0.3).astype(np.float32)
    b = rng.standard_normal(ncls).astype(np.float32)
    sc = (rng.uniform(0.5, 1.5, cin) * rng.choice([-1.0, 1.0], cin)).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    unsure = np.zeros(HEAD_UNIQUE_ROWS, bool)
    for s_, h_ in ((None, None), (sc, sh)):
        p, _ = head_fwd(x, w, b, s_, h_, SOFTMAX)
        unsure |= ~argmax_margin_mask(p, head_fwd_bound(x, w, b, s_, h_, SOFTMAX))
        for thresh in (0.5, 0.3):
            p, _ = head_fwd(x, w, b, s_, h_, SIGMOID, thresh)
            unsure |= ~thresh_margin_mask(p, head_fwd_bound(x, w, b, s_, h_, SIGMOID, thresh), thresh).all(-1)
    return x[np.argsort(unsure, kind='stable')], w, b, sc, sh


def _f64(v):
    return None if v is None else np.asarray(v, np.float64)


def head_logits(x, w, b, in_scale=None, in_shift=None):
    a = affine(x, in_scale, in_shift, relu=True) if in_scale is not None else x
    return a @ _f64(w) + _f64(b), a


def head_fwd(x, w, b, in_scale, in_shift, activation, thresh=0.5):
    """Conv2D(ncls, (1, 1)) on a = relu(in_scale x + in_shift) (a = x without in_scale), then the activation.  x: (npix, cin) float64
    holding the values AS STORED (bf16 / fp8 rounded first), so the reference carries no storage error.
    -> (probs, classes): softmax with classes (npix,) = argmax, lowest index on ties; sigmoid with classes (npix, ncls) = probs > thresh
    (thresh as the float32 the C ABI receives); linear: the logits and None."""
    z, _ = head_logits(x, w, b, in_scale, in_shift)
    if activation == SOFTMAX:
        p = K.softmax(z)
        return p, K.argmax_classes(p)
    if activation == SIGMOID:
        p = K.sigmoid(z)
        return p, (p > np.float64(np.float32(thresh))).astype(np.int32)
    return z, None


def head_fwd_bound(x, w, b, in_scale, in_shift, activation, thresh=0.5):
    """per-element bound of |kernel - head_fwd|, derived from the reference (nothing fitted).
    Logits: z_k = b_k + sum_c a_c w_ck in float32, cin products and cin additions in any order (FMA or not):
        dz_k = (cin + 3) U (sum_c |a_c| |w_ck| + |b_k|)
      plus, with the fused input BatchNorm + ReLU, sum_c |w_ck| da_c with da_c = U (|scale_c x_c| + |scale_c x_c + shift_c|): the
      activation a_c is itself one rounded product and one rounded sum (ReLU does not enlarge the error).
    Softmax / sigmoid: a logit error of e changes p_k by at most a relative 2 max_k dz_k (first order, numerator and denominator), and
      the float32 evaluation adds 8 U relative (expf to one ulp = 2 U twice, the reciprocal, the product, the sum of two terms); the sum
      of ncls > 3 exponentials adds one U for each further term: max(8, ncls + 5) U.  2^-149 absolute for a result that underflows.
    Linear: dz_k."""
    z, a = head_logits(x, w, b, in_scale, in_shift)
    w64, cin, ncls = np.abs(_f64(w)), np.shape(w)[0], np.shape(w)[1]
    dz = (cin + 3) * U * (np.abs(a) @ w64 + np.abs(_f64(b)))
    if in_scale is not None:
        prod = x * _f64(in_scale)
        dz = dz + (U * (np.abs(prod) + np.abs(prod + _f64(in_shift)))) @ w64
    if activation == LINEAR:
        return dz
    p = K.softmax(z) if activation == SOFTMAX else K.sigmoid(z)
    return p * (2.0 * dz.max(-1, keepdims=True) + max(8, ncls + 5) * U) + 2.0 ** -149


def argmax_margin_mask(p_ref, bound):
    """True where the argmax cannot depend on the rounding: best minus second-best probability above the sum of the two largest bounds of
    the pixel (every pixel for one class)"""
    if p_ref.shape[-1] == 1:
        return np.ones(p_ref.shape[:-1], bool)
    srt = np.sort(p_ref, -1)
    bs = np.sort(np.broadcast_to(bound, p_ref.shape), -1)
    return (srt[..., -1] - srt[..., -2]) > (bs[..., -1] + bs[..., -2])


def thresh_margin_mask(p_ref, bound, thresh=0.5):
    """True where `p > thresh` cannot depend on the rounding"""
    return np.abs(p_ref - np.float64(np.float32(thresh))) > bound


# ------------------------------------------------------------------------------------------------ Jacobians
def activation_bwd(p, g, activation, grad_scale=1.0):
    """dL/dlogits from g = dL/dprobs, through the head's activation, times grad_scale (as the float32 the C ABI receives)"""
    gs = np.float64(np.float32(grad_scale))
    if activation == SOFTMAX:
        return gs * K.softmax_bwd(p, g)
    if activation == SIGMOID:
        return gs * g * p * (1.0 - p)
    return gs * g


# ------------------------------------------------------------------------------------------------ point-wise losses
CCE_LO, CCE_HI = OL.K_EPSILON, 1.0 - OL.K_EPSILON
BCE_LO, BCE_HI = 0.00001, 0.99999


def _f32_const_shift(c64, f32_value):
    """log of the float32 constant the kernel clips at, minus log c64"""
    return np.log(np.float64(f32_value)) - np.log(c64)


# the kernels clip at float32 constants: 1e-7f, 1.f - 1e-7f (= 1 - 2^-23), 0.00001f, 0.99999f and 1.f - those; a clipped term's logarithm
# differs from the one oracle/losses.py takes by these amounts (-1.9e-8 ... 1.4e-3), which are no rounding error: pointwise_loss reports
# their sum as `clip_shift`, and loss + clip_shift is the float64 value of what the kernel is asked to compute
_ONE = np.float32(1.0)
CCE_SHIFT_LO = _f32_const_shift(CCE_LO, np.float32(1e-7))
CCE_SHIFT_HI = _f32_const_shift(CCE_HI, _ONE - np.float32(1e-7))
BCE_SHIFT = {('lo', 'p'): _f32_const_shift(BCE_LO, np.float32(BCE_LO)), ('lo', 'q'): _f32_const_shift(1.0 - BCE_LO, _ONE - np.float32(BCE_LO)),
             ('hi', 'p'): _f32_const_shift(BCE_HI, np.float32(BCE_HI)), ('hi', 'q'): _f32_const_shift(1.0 - BCE_HI, _ONE - np.float32(BCE_HI))}


def cce_inside(p):
    o = p / p.sum(-1, keepdims=True)
    return (o >= CCE_LO) & (o <= CCE_HI), o


def bce_inside(p):
    return (p >= BCE_LO) & (p <= BCE_HI)


def pointwise_loss(kind, p, t, wts, activation, grad_scale=1.0):
    """p, t: (npix, ncls) float64 (p holding float32 values).  -> dict:
    loss, dlogits; inside (the elements whose gradient w.r.t. the probability is not clipped away); abs_sum = sum of |term| over the terms
    the loss adds up, nterms = how many of them are non-zero; clip_shift = what clipping at the kernel's float32 constants instead adds to the loss."""
    wts = _f64(wts)
    if kind == CCE:
        loss, g, _ = OL.weighted_categorical_crossentropy(t, p, wts)
        inside, o = cce_inside(p)
        coef = wts.reshape(1, -1) * t / p.shape[0]
        terms = np.abs(coef * np.log(np.clip(o, CCE_LO, CCE_HI)))
        shift = -(coef * ((o < CCE_LO) * CCE_SHIFT_LO + (o > CCE_HI) * CCE_SHIFT_HI)).sum()
    else:
        loss, g = OL.weighted_bce(t, p, wts[0])
        inside = bce_inside(p)
        yp = np.clip(p, BCE_LO, BCE_HI)
        tp, tq = np.abs(t * wts[0] * np.log(yp)) / p.size, np.abs((1 - t) * np.log(1 - yp)) / p.size
        terms = np.stack([tp, tq])
        lo, hi = p < BCE_LO, p > BCE_HI
        cp, cq = t * wts[0] / p.size, (1 - t) / p.size
        shift = -(cp * (lo * BCE_SHIFT['lo', 'p'] + hi * BCE_SHIFT['hi', 'p']) + cq * (lo * BCE_SHIFT['lo', 'q'] + hi * BCE_SHIFT['hi', 'q'])).sum()
    return dict(loss=float(loss), dlogits=activation_bwd(p, g, activation, grad_scale), inside=inside, abs_sum=float(terms.sum()),
                nterms=int(np.count_nonzero(terms)), clip_shift=float(shift))


def sum_bound(nterms, abs_sum):
    """the derived bound of the element-wise suite for a float32 sum of `nterms` terms in any order, (nterms - 1) U sum|term|, plus
    4 U sum|term| for the rounding of each term (logf, the division, the products)"""
    return (max(nterms, 1) - 1 + 4) * U * abs_sum


def probe_bound(abs_sum):
    """a handful of terms: 16 U relative"""
    return 16 * U * abs_sum


# ------------------------------------------------------------------------------------------------ ratio losses
def global_loss(kind, p, t, activation, grad_scale=1.0, class_weights=None, eps=1e-6):
    """p, t: (nimg, ppi, ncls) float64.  gen_dice (per image, mean over images; class_weights None: per-image count weights 1 / count^2,
    eps for an absent class), iou_loss and mse_4d (over the whole batch; NaN targets are left out).
    -> dict loss, dlogits, loss_bound.  loss_bound applies sum_bound to each of the sums the loss is formed from and carries it, to first
    order, through the few float32 operations that follow (4 U per quotient and difference, one U per further addend)."""
    nimg, ppi, ncls = p.shape
    p4, t4 = p.reshape(nimg, ppi, 1, ncls), t.reshape(nimg, ppi, 1, ncls)
    if kind == DICE:
        gw = None if class_weights is None else [float(v) for v in np.asarray(class_weights, np.float32)]
        loss, g = OL.gen_dice(t4, p4, eps=float(np.float32(eps)), global_weights=gw)
        if gw is None:
            with np.errstate(divide='ignore'):
                wk = 1.0 / t.sum(1) ** 2
            wk = np.where(np.isfinite(wk), wk, float(np.float32(eps)))
        else:
            wk = np.broadcast_to(np.asarray(gw), (nimg, ncls))
        a, b = (t * p).sum(1), (t + p).sum(1)                                    # (nimg, ncls); every term is >= 0
        da, db = sum_bound(ppi, a), sum_bound(ppi, b)
        num, den = (wk * a).sum(-1), (wk * b).sum(-1)
        dnum, dden = (wk * da).sum(-1) + (ncls + 3) * U * num, (wk * db).sum(-1) + (ncls + 3) * U * den
        r = num / den
        per = 2.0 * (dnum / den + num * dden / den ** 2) + 4 * U * (1.0 + 2.0 * r)
        bound = per.mean() + (nimg + 1) * U * np.abs(1.0 - 2.0 * r).mean()
    elif kind == IOU:
        loss, g = OL.iou_loss(t4, p4)
        i, un, n = (t * p).sum(), (t + (1 - t) * p).sum(), p.size
        bound = sum_bound(n, i) / un + i * sum_bound(n, un) / un ** 2 + 4 * U * (1.0 + i / un)
    else:
        with np.errstate(invalid='ignore'):
            loss, g = OL.mse_4d(t4, p4)
        sq = np.nansum(np.square(p - t))
        bound = (sum_bound(p.size, sq) + 3 * U * sq) / np.isfinite(t).sum() + 2 * U * loss
    return dict(loss=float(loss), dlogits=activation_bwd(p, g.reshape(p.shape), activation, grad_scale), loss_bound=float(bound))


# ------------------------------------------------------------------------------------------------ input builders
def _softmax32(z):
    z = z.astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def _sigmoid32(z):
    with np.errstate(over='ignore'):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-z.astype(np.float32)))).astype(np.float32)


def cce_ambiguous(p):
    """normalised probabilities in [0.5e-7, 2e-7] or [1 - 2.4e-7, 1 - 0.3e-7]: float32 (o = p / s rounded, clip constants 1e-7f and
    1 - 2^-23) and float64 may disagree about `inside` there"""
    p = np.asarray(p, np.float64)
    o = p / p.sum(-1, keepdims=True)
    return ((o >= 0.5e-7) & (o <= 2e-7)) | ((o >= 1 - 2.4e-7) & (o <= 1 - 0.3e-7))


def bce_ambiguous(p):
    """p within a factor 1 +- 1e-4 of 1e-5, or 1 - p within that factor of 1e-5 (the upper limit 0.99999 is taken on the side of 1 - p:
    read on p itself the band would hold 1.0 and all of the clipped branch).  The kernel compares the float32 p with float32 constants,
    so the two precisions can disagree only at p == 0.00001f itself."""
    p = np.asarray(p, np.float64)
    return (np.abs(p / BCE_LO - 1.0) <= 1e-4) | (np.abs((1.0 - p) / (1.0 - BCE_HI) - 1.0) <= 1e-4)


def _probs(ncls, npix, seed, kind, saturate, rows_sum_to_one=None):
    """kind decides the bands to keep clear of; rows_sum_to_one (default: kind == CCE) whether a softmax or a per-element sigmoid makes them"""
    soft = kind == CCE if rows_sum_to_one is None else rows_sum_to_one
    assert soft or kind == BCE
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((npix, ncls)) * (2.0 if soft else 3.0)
    if saturate:
        pix, col = np.arange(npix), rng.integers(0, ncls, npix)
        mode = pix % 5                  # 0: as drawn; 1 / 2: one logit +100 / -100 against the others (exactly 1 / 0); 3 / 4: clipped, not 0 / 1
        if not soft:
            for m, v in ((1, 100.0), (2, -100.0), (3, 14.0), (4, -14.0)):
                z[pix[mode == m], col[mode == m]] = v
        else:
            top = z.max(-1)
            for m, shift, v in ((1, -100.0, 100.0), (2, 100.0, -100.0), (3, 0.0, None), (4, 0.0, None)):
                sel = mode == m
                z[sel] += shift
                z[pix[sel], col[sel]] = v if v is not None else top[sel] + (20.0 if m == 3 else -22.0)
    p = _softmax32(z) if soft else _sigmoid32(z)
    if soft:
        amb = cce_ambiguous if kind == CCE else bce_ambiguous
        bad = amb(p).any(-1)
        p[bad] = _softmax32(np.zeros((1, ncls)))[0]
        assert not amb(p).any() and (p.sum(-1) > 0.5).all()
    else:
        bad = bce_ambiguous(p)
        p[bad] = np.float32(0.5)
        assert not bce_ambiguous(p).any()
    return p, float(np.mean(bad))


def probs_random(ncls, npix, seed, kind, rows_sum_to_one=None):
    """float32 (npix, ncls): a float32 softmax (kind CCE, or rows_sum_to_one) or sigmoid (BCE) of normal logits; values in the ambiguous
    bands of `kind` removed"""
    return _probs(ncls, npix, seed, kind, False, rows_sum_to_one)[0]


def probs_saturated(ncls, npix, seed, kind=CCE):
    """float32 (npix, ncls) that reach every clipping branch of the loss `kind`: exactly 0 and exactly 1 as a real float32 softmax / sigmoid
    produces them from logits of magnitude 100, non-zero values below the lower clip and (BCE) values other than 1 above the upper one,
    and unclipped values, cycling over the pixels so that the first five hold every mode.  Asserts the branches are reached and that no
    value lies in the ambiguous bands (such values are replaced, not left for the test to skip)."""
    p, _ = _probs(ncls, npix, seed, kind, True)
    p64 = p.astype(np.float64)
    if kind == CCE:
        inside, o = cce_inside(p64)
        assert (o > CCE_HI).any() and (p == 1).any() and (ncls == 1 or ((o == 0).any() and ((o > 0) & (o < CCE_LO)).any() and inside.any()))
    else:
        assert (p == 0).any() and (p == 1).any() and ((p > 0) & (p < BCE_LO)).any() and ((p < 1) & (p > BCE_HI)).any() and bce_inside(p64).any()
    return p


def targets_random(ncls, npix, seed):
    """one-hot labels (Bernoulli(0.3) for one class), float32"""
    rng = np.random.default_rng(seed + 7)
    if ncls == 1:
        return (rng.random((npix, 1)) < 0.3).astype(np.float32)
    return np.eye(ncls, dtype=np.float32)[rng.integers(0, ncls, npix)]


def probe_picks(npix, strides):
    """the first pixel, the last pixel of the first trip of a loop of each stride and the first of its second trip, the last three"""
    picks = {0, npix - 3, npix - 2, npix - 1}
    for s in strides:
        picks |= {s - 1, s}
    return sorted(q for q in picks if 0 <= q < npix)


def probe_targets(npix, picks, ncls=1, classes=None):
    """y_true (npix, ncls) float32, zero except a one at the picked pixels (class classes[i] of pick i, default pick % ncls): the loss
    consists of those few terms, so a skipped tail or trip changes it by a large factor, not by rounding"""
    t = np.zeros((npix, ncls), np.float32)
    picks = np.asarray(picks)
    t[picks, (picks % ncls) if classes is None else np.asarray(classes)] = 1.0
    return t


def least_likely(p, picks):
    """class of the smallest probability at each pick: |log o| >= log ncls there, so the term is not a difference of nearly equal numbers"""
    return np.asarray(p)[np.asarray(picks)].argmin(-1)


# ------------------------------------------------------------------------------------------------ case tables
ACTIVATIONS = [SOFTMAX, SIGMOID, LINEAR]
POINTWISE_NCLS = [1, 2, 3, 4, 5, 8]
GRAD_SCALES = [1.0, 128.0]
GLOBAL_NCLS = [1, 2, 3, 8]
CCE_WEIGHTS = lambda ncls: (1.0 + 3.0 * np.arange(ncls)).astype(np.float32)  # noqa: E731
BCE_WEIGHTS = np.array([5.0], np.float32)
DICE_WEIGHTS = lambda ncls: np.array(([0.3, 0.5] + [0.1] * 6)[:ncls], np.float32)  # noqa: E731


def pointwise_shapes():
    """pixel counts: small, ragged, past the launch cap of either loss kernel"""
    return [8 * 8, 3 * 7 * 9, 2 * grid_cap_threads() + 3]


def pointwise_strides():
    return [LOSS_GENERAL_STRIDE, capped_stride()]


def global_shapes():
    """(nimg, pix_per_img): small, ragged, past the per-image cap of 65 536 threads"""
    return [(1, 8 * 8), (3, 7 * 9), (2, 2 * GLOBAL_STRIDE + 3)]


def pointwise_seed(kind, ncls, npix):
    return 100 * ncls + 10 * kind + npix % 97


def global_cases():
    """(kind, activation, weights mode) pairings that mean something: the overlap losses on probabilities (softmax needs two classes, checked by
    the caller), mse_4d also on a linear head"""
    return [(DICE, SOFTMAX, 'global'), (DICE, SIGMOID, 'global'), (DICE, SOFTMAX, 'counts'), (DICE, SIGMOID, 'counts'),
            (IOU, SOFTMAX, None), (IOU, SIGMOID, None), (MSE, LINEAR, None), (MSE, SIGMOID, None), (MSE, SOFTMAX, None)]


def global_runs():
    """(kind, activation, weights mode, ncls): every pairing above at every class count, less the one-class softmax of the overlap losses (the
    constant 1: no gradient, nothing to test)"""
    return [c + (n,) for c in global_cases() for n in GLOBAL_NCLS if not (c[1] == SOFTMAX and n == 1 and c[0] != MSE)]


def global_inputs(kind, activation, ncls, nimg, ppi, probe=False):
    """p, t (nimg, ppi, ncls) float32.  Overlap losses: one-hot targets with the last class absent from image 1 (every class from an image of
    zeros for ncls = 1), or probe targets per image; mse_4d: real-valued targets with three NaNs, one of them in the last pixel."""
    rng = np.random.default_rng(1000 * kind + 100 * activation + 10 * ncls + nimg + ppi % 89)
    z = rng.standard_normal((nimg, ppi, ncls)) * 2.0
    p = z.astype(np.float32) if activation == LINEAR else (_softmax32(z) if activation == SOFTMAX else _sigmoid32(z))
    if kind == MSE:
        t = rng.random((nimg, ppi, ncls)).astype(np.float32)
        t[0, 0, 0] = t[nimg - 1, ppi // 2, ncls - 1] = t[nimg - 1, ppi - 1, 0] = np.nan
        return p, t
    if probe:
        picks = probe_picks(ppi, [GLOBAL_STRIDE])
        return p, np.stack([probe_targets(ppi, picks, ncls, [(q + i) % ncls for q in picks]) for i in range(nimg)])
    lab = rng.integers(0, ncls, (nimg, ppi))
    t = np.eye(ncls, dtype=np.float32)[lab] if ncls > 1 else (rng.random((nimg, ppi, 1)) < 0.3).astype(np.float32)
    if nimg > 1:
        if ncls > 1:
            t[1][lab[1] == ncls - 1] = np.eye(ncls, dtype=np.float32)[0]
        else:
            t[1] = 0.0
    return p, t
