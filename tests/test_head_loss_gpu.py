"""Op-level parity of the classifier head forward (satcv_head_fwd) and of the loss kernels (satcv_loss_fwd_bwd,
satcv_loss_global_fwd_bwd) through the C ABI against the float64 restatements of tests/head_loss_oracle.py: all eight register-resident
head forms and five served by the LDS kernel, every storage type, the three activations, with and without the fused input BatchNorm,
channel slices of wider tensors guarded by NaN, `classes` given and NULL; the losses at 1 ... 8 classes on random and on saturated
probabilities (every clipping branch), on probe targets that make a skipped trip or tail of a grid-stride loop change the loss by a large
factor, the vectorised cross-entropy kernel against the general one, and the argument checks.  Every shape comes small, ragged
(n = 3, h = 7, w = 9) and past the launch cap of its kernel.

Bounds (none tuned on the device; tests/test_head_loss_cpu.py shows the input conditions for the reference alone): the per-element
head_fwd_bound; exact equality of classes outside the margin masks and in the tie / threshold / saturation cases; dlogits within the
op-level close() bound (2e-5 of the largest reference magnitude) and exactly zero where clipping removes the gradient; losses within the
derived summation bound, or 16 * 2^-24 relative where only a handful of terms remain (cross-entropy on probe targets; weighted BCE keeps
a (1 - t) log(1 - p) term at every pixel, so its probe runs are held to the summation bound and catch a dropped pixel through dlogits,
which is prefilled with a sentinel).  Probe runs start from loss_out = 0; a preset loss_out is tested on the other inputs.  Every
toleranced check prints its worst error and bound as a `[fig]` line (pytest -rP)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import head_loss_oracle as H  # noqa: E402
import test_elementwise_gpu as G  # noqa: E402  (the helpers of the element-wise suite: device arrays, sentinels, `refused`, `[fig]` lines)

pytestmark = pytest.mark.gpu

E, SENT, CODE, TD, RAW = G.E, G.SENT, G.CODE, G.TD, G.RAW
dev, f32dev, host, raw, ptr, fig, refused, sync = G.dev, G.f32dev, G.host, G.raw, G.ptr, G.fig, G.refused, G.sync
U = H.U


def within(got, ref, bound, what):
    """every element within its own bound; prints the worst error as a fraction of its bound"""
    worst = float((np.abs(np.asarray(got, np.float64) - ref) / bound).max())
    fig(what + ' (fraction of the derived bound)', worst, 1.0)
    assert worst <= 1.0, f'{what}: {worst:.3f} of the bound'


def close_f32(got, ref, what):
    G.close(got, ref, 'f32', what)


# ------------------------------------------------------------------------------------------------ head forward
def head_desc(xd, ld, off, cin, ncls, wd, bd, scd, shd, activation, thresh, probs, classes, npix, kind):
    d = E.HeadDesc()
    d.x, d.ldx, d.cin = ptr(xd, off) if xd is not None else None, ld, cin
    d.in_scale, d.in_shift = (scd.data_ptr(), shd.data_ptr()) if scd is not None else (None, None)
    d.w, d.b, d.ncls = wd.data_ptr() if wd is not None else None, bd.data_ptr() if bd is not None else None, ncls
    d.activation, d.thresh = activation, thresh
    d.probs, d.classes = probs.data_ptr() if probs is not None else None, classes.data_ptr() if classes is not None else None
    d.npix, d.dtype = npix, CODE[kind]
    return d


def run_head(xd, ld, off, cin, ncls, wd, bd, scd, shd, activation, thresh, npix, kind, with_classes=True):
    """-> (probs float64, classes int32 or None); both outputs are prefilled with sentinels"""
    probs = torch.full((npix, ncls), SENT, dtype=torch.float32, device='cuda')
    classes = torch.full((npix,) if activation == H.SOFTMAX else (npix, ncls), -5, dtype=torch.int32, device='cuda')
    d = head_desc(xd, ld, off, cin, ncls, wd, bd, scd, shd, activation, thresh, probs, classes if with_classes else None, npix, kind)
    E.check(E.lib.satcv_head_fwd(C.byref(d), E.st))
    sync()
    if not with_classes or activation == H.LINEAR:
        assert (classes == -5).all().item(), 'classes written although not asked for'
        return host(probs), None
    return host(probs), classes.cpu().numpy()


def gather_rows(base, idx):
    """rows idx of a device tensor of any storage type (through its raw integer view)"""
    return base.view(RAW[{4: 'f32', 2: 'bf16', 1: 'fp8'}[base.element_size()]])[idx].view(base.dtype).contiguous()


@pytest.mark.parametrize('kind', H.HEAD_KINDS)
@pytest.mark.parametrize('form', H.HEAD_FORMS)
def test_head_fwd(form, kind):
    ncls, cin = form
    x, w, b, sc, sh = H.head_inputs(ncls, cin, kind)
    wd, bd, scd, shd = f32dev(w), f32dev(b), f32dev(sc), f32dev(sh)
    bases = {False: (dev(x, kind), cin, 0), True: (G.wide(x, kind, cin + 16, 8, np.nan), cin + 16, 8)}
    salt = H.HEAD_FORMS.index(form) + H.HEAD_KINDS.index(kind)

    @functools.lru_cache(maxsize=None)
    def reference(bn, activation, thresh):
        args = (x, w, b, sc if bn else None, sh if bn else None, activation, thresh)
        return H.head_fwd(*args) + (H.head_fwd_bound(*args),)

    for npix in H.head_shapes():
        big = npix > H.HEAD_UNIQUE_ROWS
        rows = np.arange(npix) % H.HEAD_UNIQUE_ROWS
        idx = torch.tensor(rows, device='cuda')
        xs = {wide_: (gather_rows(t, idx), ld, off) for wide_, (t, ld, off) in bases.items()} if not big else {}
        combos = [(a, bn, wide_, cl) for a in H.ACTIVATIONS for bn in (False, True) for wide_ in (False, True) for cl in (True, False)]
        if big:         # past the launch cap: each activation once, the other choices cycling over forms and storage types
            combos = [(a, bool((salt + a) & 1), bool((salt + a) & 2), not (salt + a) & 4) for a in H.ACTIVATIONS]
        for activation, bn, wide_, with_classes in combos:
            if big and wide_ not in xs:
                xs = {wide_: (gather_rows(bases[wide_][0], idx),) + bases[wide_][1:]}
            xd, ld, off = xs[wide_]
            thresh = 0.3 if wide_ else 0.5
            p_ref, c_ref, bound = reference(bn, activation, thresh)
            tag = f'head_fwd {kind} ncls={ncls} cin={cin} npix={npix} act={activation} bn={int(bn)} ldx={ld} classes={int(with_classes)}'
            probs, classes = run_head(xd, ld, off, cin, ncls, wd, bd, scd if bn else None, shd if bn else None, activation, thresh, npix, kind, with_classes)
            assert np.isfinite(probs).all(), tag + ': NaN / Inf (a read outside the channel slice, or an unwritten pixel)'
            within(probs, p_ref[rows], bound[rows], tag)
            if classes is None:
                continue
            sure = (H.argmax_margin_mask(p_ref, bound) if activation == H.SOFTMAX else H.thresh_margin_mask(p_ref, bound, thresh))[rows]
            assert 1.0 - sure.mean() <= 0.01
            assert np.array_equal(classes[sure], c_ref[rows][sure]), tag + ': classes'
            assert ((classes >= 0) & (classes < (ncls if activation == H.SOFTMAX else 2))).all(), tag + ': a class outside its range'


@pytest.mark.parametrize('form', [f for f in H.HEAD_FORMS if f[0] >= 2])
def test_head_fwd_equal_logits_give_the_lower_class(form):
    ncls, cin = form
    npix = 3 * 7 * 9
    x, w, b, sc, sh = H.head_inputs(ncls, cin, 'f32')
    lo, hi = ncls - 2, ncls - 1
    w[:, hi], b[hi] = w[:, lo], b[lo]                     # two identical columns: bit-equal logits and probabilities
    w[:, :lo], b[:lo] = 0.0, -60.0                        # every other class far below
    xd = dev(x[:npix], 'f32')
    for bn in (False, True):
        probs, classes = run_head(xd, cin, 0, cin, ncls, f32dev(w), f32dev(b), f32dev(sc) if bn else None, f32dev(sh) if bn else None, H.SOFTMAX, 0.5, npix, 'f32')
        assert np.array_equal(probs[:, lo], probs[:, hi]) and (probs[:, lo] > 0.49).all()
        assert (classes == lo).all(), f'tf.argmax picks the lowest index on a tie: {np.unique(classes)}'


@pytest.mark.parametrize('form', [(1, 16), (2, 32), (1, 128), (3, 24)])
def test_head_fwd_threshold_equality(form):
    """zero weights and bias: the sigmoid is 0.5 exactly; `p > thresh` is false at 0.5 and true just below"""
    ncls, cin = form
    npix = 3 * 7 * 9
    x = H.head_inputs(ncls, cin, 'f32')[0][:npix]
    wd, bd, xd = f32dev(np.zeros((cin, ncls))), f32dev(np.zeros(ncls)), dev(x, 'f32')
    for thresh, want in ((0.5, 0), (float(np.nextafter(np.float32(0.5), np.float32(0))), 1)):
        probs, classes = run_head(xd, cin, 0, cin, ncls, wd, bd, None, None, H.SIGMOID, thresh, npix, 'f32')
        assert (probs == 0.5).all() and (classes == want).all(), (thresh, np.unique(classes))


@pytest.mark.parametrize('form', [(2, 16), (4, 32), (1, 64), (8, 32), (1, 128), (3, 24)])
def test_head_fwd_saturated_logits(form):
    """logits of +-100: probabilities exactly 0 / 1, no NaN or Inf, in either kernel"""
    ncls, cin = form
    npix = 3 * 7 * 9
    x = H.head_inputs(ncls, cin, 'f32')[0][:npix]
    for first in (100.0, -100.0):
        b = np.full(ncls, -first, np.float32)
        b[0] = first
        for activation in (H.SOFTMAX, H.SIGMOID):
            probs, classes = run_head(dev(x, 'f32'), cin, 0, cin, ncls, f32dev(np.zeros((cin, ncls))), f32dev(b), None, None, activation, 0.5, npix, 'f32')
            assert np.isfinite(probs).all()
            if activation == H.SIGMOID:
                want = (b > 0).astype(np.float64)
                assert np.array_equal(probs, np.broadcast_to(want, probs.shape)) and np.array_equal(classes, np.broadcast_to(want.astype(np.int32), classes.shape))
            else:
                top = (b == b.max())
                share = np.float64(np.float32(1.0) / np.float32(top.sum()))                     # the kernel's ex * (1.f / s) with ex = 1
                assert np.array_equal(probs, np.broadcast_to(top * share, probs.shape)) and (classes == int(top.argmax())).all()


def test_head_fwd_refuses_bad_arguments():
    cin, ncls, npix = 16, 2, 8
    x, w, b = dev(np.ones((npix, 24)), 'f32'), f32dev(np.ones((24, 9))), f32dev(np.ones(9))
    probs = torch.full((npix, 9), SENT, dtype=torch.float32, device='cuda')
    classes = torch.full((npix, 9), -5, dtype=torch.int32, device='cuda')
    before, cbefore = raw(probs), raw(classes)

    def call(**kw):
        a = dict(xd=x, ld=24, off=0, cin=cin, ncls=ncls, wd=w, bd=b, scd=None, shd=None, activation=0, thresh=0.5, probs=probs, classes=classes, npix=npix, kind='f32')
        a.update(kw)
        d = head_desc(**a)
        refused(E.lib.satcv_head_fwd(C.byref(d), E.st), probs, before)
        assert np.array_equal(raw(classes), cbefore)

    for name in ('xd', 'wd', 'bd', 'probs'):
        call(**{name: None})
    for bad in (dict(cin=12), dict(cin=0), dict(cin=-8), dict(ncls=0), dict(ncls=9), dict(npix=0)):
        call(**bad)
    d = head_desc(x, 24, 0, cin, ncls, w, b, None, None, 0, 0.5, probs, classes, npix, 'f32')
    d.dtype = 7
    refused(E.lib.satcv_head_fwd(C.byref(d), E.st), probs, before)
    assert E.lib.satcv_head_fwd(None, E.st) != 0


# ------------------------------------------------------------------------------------------------ point-wise losses
LOSS0 = 3.25                                     # a non-zero loss_out: the kernels add to it


def shifted(a32, shift):
    """device copy of a float32 array that starts `shift` floats into its allocation (shift = 1: 4-byte aligned only)"""
    buf = torch.full((a32.size + 8,), SENT, dtype=torch.float32, device='cuda')
    view = buf[shift:shift + a32.size].view(a32.shape)
    view.copy_(torch.tensor(a32))
    return buf, view


def run_pointwise(kind, pd, td, wd, ncls, activation, npix, gs, loss0, shift=0):
    lossd = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    buf, dl = shifted(np.full((npix, ncls), SENT, np.float32), shift)
    E.check(E.lib.satcv_loss_fwd_bwd(kind, pd.data_ptr(), td.data_ptr(), wd.data_ptr(), ncls, activation, npix, gs, lossd.data_ptr(), dl.data_ptr(), E.st))
    sync()
    assert (buf[:shift] == SENT).all().item() and (buf[shift + npix * ncls:] == SENT).all().item(), 'the loss wrote outside dlogits'
    return float(lossd.item()), host(dl)


def preset_slack(npix, loss0):
    """loss_out takes one atomic add per workgroup, each rounding at the magnitude of the running total: what the summation bound does not
    cover of that is the preset value's share, U |loss0| per workgroup of the launch (nothing for loss_out = 0)"""
    return min(-(-npix // H.EW_BLOCK), H.capped_stride() // H.EW_BLOCK) * U * abs(loss0)


def check_pointwise(kind, ncls, activation, npix, p, t, gs, loss0, shift, tag, probe=False, ref=None):
    """one launch against the oracle -> (dlogits, ref); `ref` carries the gs = 1 reference of the same inputs over"""
    wts = H.CCE_WEIGHTS(ncls) if kind == H.CCE else H.BCE_WEIGHTS
    if ref is None:
        ref = H.pointwise_loss(kind, p.astype(np.float64), t.astype(np.float64), wts, activation, 1.0)
    (_, pd), (_, td) = shifted(p, shift), shifted(t, shift)
    loss, dl = run_pointwise(kind, pd, td, f32dev(wts), ncls, activation, npix, gs, loss0, shift)
    dl_ref = ref['dlogits'] * gs                                             # a power of two: exact in either precision
    assert np.isfinite(dl).all(), tag + ': NaN / Inf / an unwritten pixel in dlogits'
    close_f32(dl, dl_ref, tag + ' dlogits')
    clipped = ~ref['inside'] & (dl_ref == 0)
    assert not dl[clipped].any(), tag + f': {np.count_nonzero(dl[clipped])} clipped elements carry a gradient'
    few = probe and kind == H.CCE                                            # BCE keeps a (1 - t) log(1 - p) term at every pixel
    want = ref['loss'] + ref['clip_shift']                                   # the float64 loss, clipped at the kernel's float32 constants
    assert not (probe and loss0), 'probe runs start from loss_out = 0: the handful of terms is all that loss_out holds'
    bound = H.probe_bound(ref['abs_sum']) if few else H.sum_bound(ref['nterms'], ref['abs_sum']) + preset_slack(npix, loss0)
    err = abs(loss - loss0 - want)
    fig(tag + (' probe loss' if probe else ' loss') + f' = {want:.6g}', err, bound)
    assert err <= bound, f'{tag}: loss {loss - loss0!r} vs {want!r}'
    return dl, ref


@functools.lru_cache(maxsize=4)
def pointwise_inputs(kind, ncls, npix):
    seed = H.pointwise_seed(kind, ncls, npix)
    pr = H.probs_random(ncls, npix, seed, kind)
    picks = H.probe_picks(npix, H.pointwise_strides())
    ps = H.probs_saturated(ncls, npix, seed, kind)
    return pr, ps, H.targets_random(ncls, npix, seed), H.probe_targets(npix, picks, ncls, H.least_likely(pr, picks)), H.probe_targets(npix, picks, ncls, H.least_likely(ps, picks))


@pytest.mark.parametrize('activation', H.ACTIVATIONS)
@pytest.mark.parametrize('kind', [H.CCE, H.BCE])
@pytest.mark.parametrize('ncls', H.POINTWISE_NCLS)
def test_pointwise_losses(ncls, kind, activation):
    for npix in H.pointwise_shapes():
        pr, ps, t, tprobe, tprobe_s = pointwise_inputs(kind, ncls, npix)
        tag = f'loss kind={kind} ncls={ncls} act={activation} npix={npix}'
        for name, p in (('random', pr), ('saturated', ps)):
            ref = None
            for gs, loss0 in ((1.0, 0.0), (128.0, LOSS0)):
                _, ref = check_pointwise(kind, ncls, activation, npix, p, t, gs, loss0, 0, f'{tag} {name} gs={gs:g}', ref=ref)
        check_pointwise(kind, ncls, activation, npix, pr, tprobe, 1.0, 0.0, 0, tag, probe=True)
        check_pointwise(kind, ncls, activation, npix, ps, tprobe_s, 128.0, 0.0, 0, tag + ' saturated', probe=True)
        if kind == H.BCE and activation == H.SOFTMAX:        # what a softmax head hands this loss: rows that sum to one
            pn = H.probs_random(ncls, npix, H.pointwise_seed(kind, ncls, npix), kind, rows_sum_to_one=True)
            check_pointwise(kind, ncls, activation, npix, pn, t, 128.0, LOSS0, 0, tag + ' rows sum to one')


def loss_fast_option():
    """-> (value of the startup option loss_fast, whether satcv_set_option can change it in this process)"""
    val = C.c_int32(-1)
    E.check(E.lib.satcv_get_option(b'loss_fast', C.byref(val)))
    return val.value, E.lib.satcv_set_option(b'loss_fast', val.value) == 0


@pytest.mark.parametrize('ncls', [2, 4])
def test_vectorised_cross_entropy_against_the_general_kernel(ncls):
    """tensors that start one float into their allocation fail the 4 * ncls byte alignment test, so the same call runs loss_kernel: the
    fallback, and the general kernel at 2 and 4 classes.  loss_fast must be on for the aligned call to reach loss_cce_softmax_kernel; where
    the options table lets it be set at run time, the general kernel is reached that way as well."""
    value, settable = loss_fast_option()
    assert value != 0, 'SATCV_LOSS_FAST=0 in the environment: this process cannot reach the vectorised kernel'
    routes = [('misaligned', 1, None)] + ([('loss_fast=0', 0, 0)] if settable else [])
    for npix in H.pointwise_shapes():
        pr, ps, t, tprobe, _ = pointwise_inputs(H.CCE, ncls, npix)
        for name, p, tt, probe in (('random', pr, t, False), ('saturated', ps, t, False), ('random', pr, tprobe, True)):
            tag = f'cce softmax ncls={ncls} npix={npix} {name}'
            gs, loss0 = (1.0, 0.0) if probe else (128.0, LOSS0)
            fast, ref = check_pointwise(H.CCE, ncls, H.SOFTMAX, npix, p, tt, gs, loss0, 0, tag + ' vectorised', probe)
            for route, shift, option in routes:
                try:
                    if option is not None:
                        E.check(E.lib.satcv_set_option(b'loss_fast', option))
                    gen, _ = check_pointwise(H.CCE, ncls, H.SOFTMAX, npix, p, tt, gs, loss0, shift, f'{tag} general ({route})', probe, ref)
                finally:
                    if option is not None:
                        E.check(E.lib.satcv_set_option(b'loss_fast', value))
                diff, _ = H.close_err(fast, gen)
                fig(f'{tag} vectorised vs general ({route}) dlogits, not asserted', diff, H.close_tol('f32'))


def test_pointwise_loss_refuses_bad_arguments():
    npix = 8
    p, t, w = f32dev(np.full((npix, 9), 0.5)), f32dev(np.ones((npix, 9))), f32dev(np.ones(9))
    dl = torch.full((npix, 9), SENT, dtype=torch.float32, device='cuda')
    loss = torch.full((1,), SENT, dtype=torch.float32, device='cuda')
    before = raw(dl)

    def call(kind=0, pp=p, tt=t, ww=w, ncls=2, n=npix, lo=loss, d=dl):
        a = [x.data_ptr() if x is not None else None for x in (pp, tt, ww, lo, d)]
        refused(E.lib.satcv_loss_fwd_bwd(kind, a[0], a[1], a[2], ncls, 0, n, 1.0, a[3], a[4], E.st), dl, before)
        assert loss.item() == SENT

    for kind in (-1, 2, 3, 4):
        call(kind=kind)
    for kw in (dict(ncls=0), dict(ncls=9), dict(n=0), dict(pp=None), dict(tt=None), dict(ww=None), dict(lo=None), dict(d=None)):
        call(**kw)


# ------------------------------------------------------------------------------------------------ ratio losses
def run_global(kind, pd, td, cwd, ncls, activation, nimg, ppi, gs, loss0, ws):
    lossd = torch.full((1,), loss0, dtype=torch.float32, device='cuda')
    dl = torch.full((nimg, ppi, ncls), SENT, dtype=torch.float32, device='cuda')
    E.check(E.lib.satcv_loss_global_fwd_bwd(kind, pd.data_ptr(), td.data_ptr(), cwd.data_ptr() if cwd is not None else None, ncls, activation, nimg, ppi,
                                            1e-6, gs, ws.data_ptr(), lossd.data_ptr(), dl.data_ptr(), E.st))
    sync()
    assert (ws[nimg * 3 * ncls:] == SENT).all().item(), 'the loss wrote past nimg * 3 * ncls floats of its workspace'
    return float(lossd.item()), host(dl)


@pytest.mark.parametrize('run', H.global_runs())
def test_global_losses(run):
    kind, activation, mode, ncls = run
    gw = H.DICE_WEIGHTS(ncls) if mode == 'global' else None
    cwd = f32dev(gw) if gw is not None else None
    for nimg, ppi in H.global_shapes():
        for probe in ((False, True) if kind != H.MSE else (False,)):
            p, t = H.global_inputs(kind, activation, ncls, nimg, ppi, probe)
            ref = H.global_loss(kind, p.astype(np.float64), t.astype(np.float64), activation, 1.0, gw, 1e-6)
            pd, td = f32dev(p), f32dev(t)
            ws = torch.full((nimg * 3 * ncls + 64,), SENT, dtype=torch.float32, device='cuda')          # never initialised: the call clears it
            tag = f'global loss kind={kind} mode={mode} ncls={ncls} act={activation} nimg={nimg} ppi={ppi}' + (' probe' if probe else '')
            for gs, loss0 in ((1.0, 0.0), (128.0, LOSS0)):                                              # the second run finds the first one's sums
                loss, dl = run_global(kind, pd, td, cwd, ncls, activation, nimg, ppi, gs, loss0, ws)
                assert np.isfinite(dl).all(), tag + ': NaN / Inf / an unwritten pixel in dlogits'
                close_f32(dl, ref['dlogits'] * gs, f'{tag} gs={gs:g} dlogits')
                bound = ref['loss_bound'] + (nimg + 1) * U * (abs(loss0) + abs(ref['loss']))             # one atomic add per image into loss_out
                err = abs(loss - loss0 - ref['loss'])
                fig(f'{tag} gs={gs:g} loss = {ref["loss"]:.6g}', err, bound)
                assert err <= bound, f'{tag}: loss {loss - loss0!r} vs {ref["loss"]!r}'
            if kind == H.MSE and activation != H.SOFTMAX:
                assert not dl[np.isnan(t)].any(), 'a NaN target carries a gradient'


def test_global_loss_refuses_bad_arguments():
    nimg, ppi = 2, 8
    p, t = f32dev(np.full((nimg, ppi, 9), 0.5)), f32dev(np.ones((nimg, ppi, 9)))
    dl = torch.full((nimg, ppi, 9), SENT, dtype=torch.float32, device='cuda')
    loss = torch.full((1,), SENT, dtype=torch.float32, device='cuda')
    ws = torch.full((256,), SENT, dtype=torch.float32, device='cuda')
    before = raw(dl)

    def call(kind=2, pp=p, tt=t, ncls=2, n=nimg, q=ppi, w=ws, lo=loss, d=dl):
        a = [x.data_ptr() if x is not None else None for x in (pp, tt, w, lo, d)]
        refused(E.lib.satcv_loss_global_fwd_bwd(kind, a[0], a[1], None, ncls, 0, n, q, 1e-6, 1.0, a[2], a[3], a[4], E.st), dl, before)
        assert loss.item() == SENT and (ws == SENT).all().item()

    for kind in (0, 1, 5, -1):
        call(kind=kind)
    for kw in (dict(n=0), dict(n=65536), dict(n=-1), dict(q=0), dict(ncls=0), dict(ncls=9), dict(pp=None), dict(tt=None), dict(w=None), dict(lo=None), dict(d=None)):
        call(**kw)
