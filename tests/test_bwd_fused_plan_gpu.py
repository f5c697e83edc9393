"""The two fused backward kernels (satcv_conv2d_bwd_fused, satcv_convt_bwd_fused), one test per entry of tests/bwd_fused_cases.py: every template
instantiation at a multi-tile shape (every workgroup iterates its persistent tile loop, some once more than others, ranges across row ends
and image ends), at one tile and at fewer tiles than CUs, and every feature the engine uses on small maps.

Per case
  * the plan query (satcv_conv2d_bwd_fused_plan_info / satcv_convt_bwd_fused_plan_info, with the real pointers and ncu = 0: the device's CU
    count) names the intended instantiation before the launch, and for a multi-tile case at least 2 (3) tiles per workgroup (slab) with some
    getting one more -- on a device with another CU count the case fails loudly instead of testing one tile per workgroup;
  * Gaussian data, pre-rounded to bf16, against the float64 oracle (oracle.keras_ops on the CPU; for the multi-tile thin-layer cases a float64
    per-tap matrix product on the device) fed with the bf16-rounded dy, under close() of tests/test_ops_gpu.py with the k of the existing test of
    the kernel: 1.5 for the thin-layer kernel, 1 (dx) and 0.5 (dK) for the transposed-conv one; the fused sums against the sums of the STORED
    gradient under the tolerance of those tests;
  * integer-lattice data, BIT-EXACT.  g, yraw, x, the weights, dpool and the accumulate base are small integers; bn_scale and in_scale are from
    {1, 2, -1, 0.5} (never 0), the shifts are the integers -scale * v0 with v0 a value the data takes (a pre-activation is exactly 0 at one
    element in 2 a + 1, a the data's amplitude: 11 to 33 %, and `>` against `>=` in the dy mask and in the sums' [a > 0] decides the result
    there; the loader's ReLU gives 0 at 0 under either comparison, so it is not discriminated), mean is an integer, rstd from {0.5, 1, 2}, c1 a multiple of 0.5, c2 from {0, 0.5, 1, -1}, hg_dlogits multiples of 0.25, hg_w integers.  Every fp32 intermediate of
    sc * gm + B * y + C is then exact in any order, dy is a multiple of its channel's grid |sc| * grid(g, c1, rstd c2) >= 1 / 8, the activated
    input a multiple of min(1, |in_scale|).  lattice() picks the largest amplitudes for which, from the shape alone, every fp32 accumulator
    stays below 2^24 units of its own grid: 9 cout max|dy| max|w| in units of 1 / 8 (data gradient; 4 cout for the transposed conv), and
    pixels x max|a| x max|dy| in units of the (ci, co) pair's grid (weight gradient, the accumulate base included) -- fp32 addition of
    multiples of a power of two is exact while the result is below 2^24 of them, in any order and any split over tiles, workgroups, K
    slices and slabs.  The multi-tile thin-layer cases get the smallest amplitudes that way (all 1).  dy is the float64 formula of satcv.h
    rounded ONCE to bf16 (round to nearest even: what torch's .to(bfloat16) does), dx the exact data gradient of that dy rounded once, dw and
    the two fused sums exact: all compared with np.array_equal.  The fused sums are accumulated per thread in fp32 over the thread's pixels
    of the workgroup's tiles, then in double: exact while (a thread's pixels per tile x tiles per workgroup) x max|dx| x max|a| < 2^24 units,
    asserted with the reference's dx.  The zero tolerance is derived, not measured;
  * the pooled form's arg-max bytes are random bytes 0 .. 3 fed directly (every routing, ties or not); the two `amax-from-the-pooling-kernel`
    cases take them from satcv_bn_relu_pool_amax on the lattice activations -- about half of them 0, so a window in four or more ties -- and check them
    against NumPy's first maximum in row-major window order;
  * dx, dw and the workspace are NaN-filled before each launch (a slab that is summed but was not written, an output element that was
    skipped, shows as NaN); g, yraw, x, dpool, the logit gradients and the operand image sit in buffers whose other channels / rows are NaN,
    with a NaN image row before and after them; stored channels of dx
    beyond the input channels, rows of the fused sums beyond them and the floats behind the workspace carry a sentinel and must come back
    untouched, and dx has a sentinel image row before and after it; pre-filled sum rows must come back as the pre-fill PLUS the sums;
  * two runs are torch.equal; for a defer_reduce case the second run leaves its slabs to satcv_*_bwd_fused_reduce_job +
    satcv_reduce_slabs_batched, must not touch dw itself, and the batched sum must equal the in-launch sum bit for bit (exact data: any order
    gives the same bits; the Gaussian run of such a case goes through the deferred path under close()).

Every case prints one record line (key, tiles per workgroup, Gaussian error, lattice outcome).  profiles/bwd_fused_parity.txt is those lines:
`python tests/test_bwd_fused_plan_gpu.py` runs every case with the same checks and rewrites the file.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import bwd_fused_cases as W  # noqa: E402
from oracle import keras_ops as K  # noqa: E402
from test_ops_gpu import close  # noqa: E402  (the one tolerance rule of the op tests)

pytestmark = pytest.mark.gpu
SENTINEL = 777.0
TD = torch.bfloat16
SCALES, RSTDS, C2S = (1.0, 2.0, -1.0, 0.5), (0.5, 1.0, 2.0), (0.0, 0.5, 1.0, -1.0)


@pytest.fixture(scope='module')
def ops():
    from satellite_computervision_amd import ops as _ops
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return _ops


def rne(a):
    """float64 array (or tensor) rounded once to bf16, round to nearest even"""
    if isinstance(a, torch.Tensor):
        return a.to(torch.float32).to(TD).to(torch.float64)
    return torch.tensor(a, dtype=torch.float64).to(torch.float32).to(TD).to(torch.float64).numpy()


def dims(c):
    """(stored input channels, output-resolution factor, taps x cout of the data gradient's K, pixels of a tile one thread adds to its fused
    sums: 256 pixels x CIN / 8 channel groups dealt to NW x 64 threads; PX pixels x CBLK / 8 groups to the 256 threads of the staging waves)"""
    if c['kind'] == 'bwdf':
        cin, _, nw = W.BWDF_FORMS[c['form']][:3]
        return c['c0'] + c['c1'], 1, 9 * c['cout'], 256 * (cin // 8) // (nw * 64)
    _, px, cblk = W.CTBF_FORMS[c['form']]
    return c['cin'], 2, 4 * c['cout'], px * (cblk // 8) // 256


def lattice(c):
    """amplitudes of the lattice data: ag (g, dpool, 4 x the logit gradients), ay (yraw and bn_shift), ax (x and in_shift), aw (weights), the
    largest of three sets for which the two matrix products are exact by the shape alone (module docstring); dy8: bound of |dy| in units of
    1 / 8; ua: bound of the activated input in units of its channel's grid"""
    cs, f, kk, _ = dims(c)
    npix = c['n'] * c['h'] * c['w']
    for ag, ay, ax, aw in ((4, 4, 2, 2), (2, 2, 2, 1), (1, 1, 1, 1)):
        gmax, ggrid = ag * (2 if c['kind'] == 'bwdf' and c['pool'] else 1), 0.25 if c['kind'] == 'bwdf' and c['hg'] else 1.0
        udy, dy8 = 0, 0
        for r in RSTDS:
            for k2 in C2S:
                inner = gmax + 0.5 + (ay + 1) * r * abs(k2)                       # |gm| + |c1| + |y - mean| rstd |c2|
                grid = min([ggrid, 0.5] + ([r * abs(k2)] if k2 else []))
                udy = max(udy, math.ceil(inner / grid * (1 + 2.0 ** -8)))         # (the rounding to bf16 moves |dy| by at most 2^-8 of it)
                dy8 = max(dy8, math.ceil(2 * inner * 8 * (1 + 2.0 ** -8)))
        ua = 2 * ax + 2 if c['affine'] else ax                                    # (|sc| ax + |shift|) / min(1, |sc|) with |shift| <= 2: 2 ax + 2, ax + 2, ax + 1
        acc_dx = kk * dy8 * aw
        acc_dw = npix * ua * udy + (64 if c['accumulate'] else 0)                 # (base: integers up to 4, in units of at least 1 / 16)
        if acc_dx < 2 ** 24 and acc_dw < 2 ** 24:
            break
    assert acc_dx < 2 ** 24 and acc_dw < 2 ** 24, (c['name'], acc_dx, acc_dw)
    return dict(ag=ag, ay=ay, ax=ax, aw=aw, dy8=dy8, ua=ua, acc_dx=acc_dx, acc_dw=acc_dw)


def make_data(c, rng, lat):
    """float64 arrays exactly representable in their storage type"""
    cs, f, _, _ = dims(c)
    n, h, w, cin, co = c['n'], c['h'], c['w'], c['cin'], c['cout']
    gs, xs = (n, h * f, w * f, co), (n, h, w, cs)
    ks = (3, 3, cin, co) if c['kind'] == 'bwdf' else (2, 2, co, cin)
    pool, hg = c['kind'] == 'bwdf' and c['pool'], c['kind'] == 'bwdf' and c['hg']
    d = {}
    if lat:
        L = lattice(c)
        ri = lambda a, s: rng.integers(-a, a + 1, s).astype(np.float64)
        d['g'], d['y'], d['x'], d['kern'] = ri(L['ag'], gs), ri(L['ay'], gs), ri(L['ax'], xs), ri(L['aw'], ks)
        # shift = -scale * v0, an integer, with v0 a value of the data: the pre-activation is exactly 0 wherever the data equals v0
        shift = lambda sc: -sc * np.where(sc == 0.5, 2.0, 1.0) * ri(1, sc.shape)
        d['sc'], d['mu'], d['rs'] = rng.choice(SCALES, co), ri(1, co), rng.choice(RSTDS, co)
        d['sh'] = shift(d['sc'])
        d['c1'], d['c2'] = 0.5 * ri(1, co), rng.choice(C2S, co)
        d['isc'], d['bmu'], d['brs'] = rng.choice(SCALES, cs), ri(1, cs), rng.choice(RSTDS, cs)
        d['ish'] = shift(d['isc'])
        if c['bst'] == 'act':
            d['x'] = np.maximum(d['x'], 0)                                        # an activation: non-negative, about half of it exactly 0
        if pool:
            d['dp'] = ri(L['ag'], (n, h // 2, w // 2, co))
        if hg:
            d['dl'], d['hw'] = 0.25 * ri(L['ag'], (n * h * w, 2)), ri(2, (co, 2))
        d['base'] = ri(4, ks)
        d['pre'] = ri(1000, (32, 2, cs))
    else:
        r = lambda s, k=1.0: rne(rng.standard_normal(s) * k)
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        if c['kind'] == 'bwdf':
            d['g'], d['y'], d['x'], d['kern'] = r(gs), rne(r(gs) * 1.5 + 0.25), r(xs), r(ks, 0.2)
            d['sc'], d['sh'] = f32((0.5 + rng.random(co)) * rng.choice([-1, 1], co)), f32(rng.standard_normal(co) * 0.5)
            d['c1'], d['c2'] = f32(rng.standard_normal(co) * 0.1), f32(rng.standard_normal(co) * 0.1)
        else:
            d['g'], d['y'], d['x'], d['kern'] = r(gs), rne(r(gs) * 1.3 + 0.2), rne(r(xs) * 1.2 + 0.1), r(ks, 0.15)
            d['sc'], d['sh'] = f32(rng.standard_normal(co)), f32(rng.standard_normal(co) * 0.5)
            d['c1'], d['c2'] = f32(rng.standard_normal(co) * 0.05), f32(rng.standard_normal(co) * 0.05)
        d['mu'], d['rs'] = f32(rng.standard_normal(co) * 0.3), f32(0.5 + rng.random(co))
        d['isc'], d['ish'] = f32(0.5 + rng.random(cs)), f32(rng.standard_normal(cs) * 0.3)
        d['bmu'], d['brs'] = f32(rng.standard_normal(cs) * 0.3), f32(0.5 + rng.random(cs))
        if c['affine'] and c['bst']:
            # keep the input's pre-activations away from 0 (the rule of test_convt_bwd_fused): the device forms them in fp32, the oracle in
            # float64, and a ReLU mask that flips on a pre-activation of 1e-7 moves a fused sum by a whole gradient value
            for _ in range(3):
                pre = d['x'] * d['isc'] + d['ish']
                d['x'] = rne(np.where(np.abs(pre) < 0.03, d['x'] + 0.25 / d['isc'], d['x']))
        if c['bst'] == 'act':
            d['x'] = np.abs(d['x'])
            d['x'][d['x'] < 0.3] = 0
        if pool:
            d['dp'] = r((n, h // 2, w // 2, co))
        if hg:
            d['dl'], d['hw'] = f32(rng.standard_normal((n * h * w, 2)) * 0.1), f32(rng.standard_normal((co, 2)))
        d['base'] = f32(rng.standard_normal(ks))
        d['pre'] = f32(rng.standard_normal((32, 2, cs)) * 100)
    if pool:
        d['amax'] = rng.integers(0, 4, (n, h // 2, w // 2, co)).astype(np.uint8)      # (amax = 'kernel': replaced by run())
    return d


def reference(c, d):
    """float64: g as the kernel forms it, dy (rounded to bf16), the activated input a (rounded), dx (rounded, None without a data gradient),
    dw unrounded.  Multi-tile thin-layer cases: on the device (torch), everything else with NumPy / oracle.keras_ops"""
    cs, f, _, _ = dims(c)
    cin, co = c['cin'], c['cout']
    pool, hg = c['kind'] == 'bwdf' and c['pool'], c['kind'] == 'bwdf' and c['hg']
    g = d['g']
    if hg:      # what satcv_head_bwd would have stored (test_fused_backward_forms_the_head_gradient_in_its_loader)
        g = torch.tensor(d['dl'] @ d['hw'].T, dtype=torch.float64).to(torch.float32).to(TD).to(torch.float64).numpy().reshape(d['y'].shape)
    if pool:    # MaxPooling2D's gradient goes to the window position the arg-max byte names (row-major: 2 * row + column)
        n, h, w = c['n'], c['h'], c['w']
        pos = (2 * (np.arange(h) % 2)[:, None] + (np.arange(w) % 2)[None, :])[None, :, :, None]
        up = lambda a: np.repeat(np.repeat(a, 2, 1), 2, 2)
        g = g + np.where(up(d['amax']) == pos, up(d['dp']), 0.0)
    mask = np.ones(g.shape, bool) if c['linear'] else (d['y'] * d['sc'] + d['sh'] > 0)
    dy = rne(d['sc'] * (np.where(mask, g, 0.0) - d['c1'] - (d['y'] - d['mu']) * d['rs'] * d['c2']))
    a = d['x']
    if c['affine']:
        a = a * d['isc'] + d['ish']
        a = rne(np.maximum(a, 0) if c['in_relu'] else a)
    out = dict(g=g, dy=dy, a=a)
    if c['kind'] == 'ctbf':
        dx, dk, _ = K.conv2d_transpose_ks_bwd(a, d['kern'], dy)
    elif not c['multi']:
        kern = np.zeros((3, 3, cs, co))
        kern[:, :, :cin] = d['kern']
        dx, dk, _ = K.conv2d_same_bwd(a, kern, dy, 1)
        dk = dk[:, :, :cin]
    else:
        # float64 per-tap matrix products on the device (exact for lattice data like any float64 evaluation: every partial sum is an integer
        # multiple of the grid far below 2^53).  y[p] = sum_ij x[p + (i - 1, j - 1)] W[i, j]  =>  dx[q] = sum_ij dy[q - (i - 1, j - 1)] W[i, j]^T,
        # dW[i, j] = sum_p x[p + (i - 1, j - 1)]^T dy[p]
        dev = torch.device('cuda')
        ta, tdy, tk = torch.tensor(a, device=dev), torch.tensor(dy, device=dev), torch.tensor(d['kern'], device=dev)
        n, h, w = c['n'], c['h'], c['w']
        pad = lambda t: torch.nn.functional.pad(t, (0, 0, 1, 1, 1, 1))
        ap, dyp = pad(ta), pad(tdy)
        tdx = torch.zeros((n, h, w, cs), dtype=torch.float64, device=dev)
        tdk = torch.zeros((3, 3, cin, co), dtype=torch.float64, device=dev)
        for i in range(3):
            for j in range(3):
                tdx[..., :cin] += dyp[:, 2 - i:2 - i + h, 2 - j:2 - j + w, :] @ tk[i, j].T
                tdk[i, j] = ap[:, i:i + h, j:j + w, :cin].reshape(-1, cin).T @ tdy.reshape(-1, co)
        dx, dk = tdx.cpu().numpy(), tdk.cpu().numpy()
    out['dw'] = dk
    out['dx'] = None if pool == 'nodx' else rne(dx)
    return out


def sums_of(c, d, a, dx):
    """the two fused sums of the layer below (satcv.h: bst_*) from a stored gradient dx: sum gm and sum gm xhat with gm = dx [a > 0] and
    xhat = (x - mean) rstd, or in the activated form sum dx [x > 0] and sum dx x"""
    gm = np.where(a > 0, dx, 0.0)
    if c['bst'] == 'act':
        return gm.sum((0, 1, 2)), (dx * a).sum((0, 1, 2))
    return gm.sum((0, 1, 2)), (gm * ((d['x'] - d['bmu']) * d['brs'])).sum((0, 1, 2))


def run(ops, c, d, defer):
    """one launch of the case (and, with defer, the batched slab sum behind it); returns dict(dx, dw, sums, plan) -- dx (n, h, w, lddx), sums
    (ROWS, 2, bst_ld) -- after the sentinel checks"""
    from satellite_computervision_amd import _lib
    lib, check = _lib.lib, _lib.check
    dev = torch.device('cuda')
    cs, f, _, _ = dims(c)
    n, h, w, cin, co = c['n'], c['h'], c['w'], c['cin'], c['cout']
    pool, hg = c['kind'] == 'bwdf' and c['pool'], c['kind'] == 'bwdf' and c['hg']
    nan = float('nan')
    f32 = lambda a: torch.tensor(a, dtype=torch.float32, device=dev).contiguous()
    keep, p = [], {}

    def wide(a, ld, off, td=TD, fill=nan):
        """a (.., rows, row length, ch) inside a NaN buffer of channel stride ld at channel offset off, one NaN image row before and after it (a
        tile origin that runs past a row end or an image end reads NaN, not another allocation); returns the address of its first element"""
        row = a.shape[-2]
        buf = torch.full((a[..., 0].size + 2 * row, ld), fill, dtype=td, device=dev)
        body = buf[row:-row].view(a.shape[:-1] + (ld,))
        body[..., off:off + a.shape[-1]] = torch.tensor(a, dtype=torch.float32 if td != torch.uint8 else td).to(td).to(dev)
        keep.append(buf)
        return body.data_ptr() + buf.element_size() * off

    def vec(name, a):
        keep.append(f32(a))
        p[name] = keep[-1].data_ptr()

    if not hg:
        p['g'] = wide(d['g'], c['ldg'], c['goff'])
    for name, key in (('bn_scale', 'sc'), ('bn_shift', 'sh'), ('bn_mean', 'mu'), ('bn_rstd', 'rs')):
        vec(name, d[key])
    if c['affine']:
        vec('in_scale', d['isc']); vec('in_shift', d['ish'])
    if c['bst'] == 'bn':
        vec('bst_mean', d['bmu']); vec('bst_rstd', d['brs'])
    code = ops.DTYPE_CODE[TD]
    if c['kind'] == 'bwdf':
        p['yraw'] = wide(d['y'], c['ldg'], c['yoff'])
        vec('bn_coef', np.stack([d['c1'], d['c2']]))
        p['x0'] = wide(d['x'][..., :c['c0']], c['c0'], 0)
        if c['c1']:
            p['x1'] = wide(d['x'][..., c['c0']:], c['c1'], 0)
        if pool != 'nodx':
            keep.append(ops.pack_weights(f32(d['kern']), cs, code)[1])
            p['w_dgrad'] = keep[-1].data_ptr()
        if hg:
            p['hg_dlogits'] = wide(d['dl'].reshape(n * h, w, 2), 2, 0, torch.float32)
            vec('hg_w', d['hw'])
        if pool:
            p['dpool'] = wide(d['dp'], c['lddp'], 0)
            p['amax'] = wide(d['amax'], co, 0, torch.uint8, 255)           # (255: no position of a window)
        dw = torch.full((3, 3, cin, co), nan, dtype=torch.float32, device=dev)
    else:
        p['yup'] = wide(d['y'], c['ldy'], c['yoff'])
        vec('bn_c1', d['c1']); vec('bn_c2', d['c2'])
        p['x'] = wide(d['x'], c['ldx'], 0)
        # the data-gradient operand image [4 cout / 8][cin][8] of satcv_pack_weights, its rows re-pitched to npad with NaN rows behind the real ones
        img = ops.pack_weights(f32(d['kern']), cin, code, transposed=True)[1].reshape(4 * co // 8, cin, 8)
        wimg = torch.full((4 * co // 8, c['npad'], 8), nan, dtype=TD, device=dev)
        wimg[:, :cin] = img
        keep.append(wimg)
        p['w_dgrad'] = wimg.data_ptr()
        dw = torch.full((2, 2, co, cin), nan, dtype=torch.float32, device=dev)
    if c['accumulate']:
        dw.copy_(f32(d['base']))
    dw0 = dw.clone()
    p['dw'] = dw.data_ptr()
    dxbuf = None
    if pool != 'nodx':      # one sentinel image row before and after, sentinel channels behind the stored ones
        dxbuf = torch.full((n * h + 2, w, c['lddx']), SENTINEL, dtype=TD, device=dev)
        dxbuf[1:-1, :, :cs] = nan
        p['dx'] = dxbuf[1:-1].data_ptr()
    sums = None
    if c['bst']:
        sums = torch.full((32, 2, c['bst_ld']), SENTINEL, dtype=torch.float64, device=dev)
        sums[..., :cs] = torch.tensor(d['pre'], device=dev) if c['prefill'] else 0.0
        p['bst_sums'] = sums.data_ptr()
    # the workspace size from a host-only plan of the device's CU count; NaN-filled, a sentinel behind it
    p['workspace'] = W.FAKE
    desc = W.make_desc(c, p)
    desc.defer_reduce = int(defer)
    nb = W.plan_info(c['kind'], desc, 0)['ws_bytes']
    wq = (lib.satcv_conv2d_bwd_fused_workspace if c['kind'] == 'bwdf' else lib.satcv_convt_bwd_fused_workspace)(C.byref(desc))
    assert wq == nb, (c['name'], wq, nb)
    ws = torch.full((nb // 4 + 64,), nan, dtype=torch.float32, device=dev)
    ws[nb // 4:] = SENTINEL
    desc.workspace, desc.workspace_bytes = ws.data_ptr(), nb
    plan = W.check_plan(c, desc, ncu=0)                  # with the real pointers and the device's CU count: the form about to run
    check((lib.satcv_conv2d_bwd_fused if c['kind'] == 'bwdf' else lib.satcv_convt_bwd_fused)(C.byref(desc), ops.stream_ptr()))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:       # a device fault: nothing more may run on this device in this session
        pytest.exit(f"{c['name']}: the device reported {e}", returncode=3)
    if defer:
        assert torch.equal(torch.nan_to_num(dw, nan=-1.0), torch.nan_to_num(dw0, nan=-1.0)), f"{c['name']}: a defer_reduce launch wrote dw"
        job = _lib.ReduceJob()
        check((lib.satcv_conv2d_bwd_fused_reduce_job if c['kind'] == 'bwdf' else lib.satcv_convt_bwd_fused_reduce_job)(C.byref(desc), C.byref(job)))
        assert job.nslab == plan['workgroups'] and job.accumulate == c['accumulate'], (c['name'], job.nslab, plan)
        items = int(lib.satcv_reduce_job_items(C.byref(job)))
        jd = torch.frombuffer(bytearray(bytes(job)), dtype=torch.uint8).to(dev)
        pd = torch.zeros(1, dtype=torch.int64, device=dev)
        check(lib.satcv_reduce_slabs_batched(jd.data_ptr(), pd.data_ptr(), 1, items, ops.stream_ptr()))
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:
            pytest.exit(f"{c['name']}: the device reported {e} (batched slab sum)", returncode=3)
    assert bool((ws[nb // 4:] == SENTINEL).all()), f"{c['name']}: the floats behind the workspace were overwritten"
    out = dict(dw=dw, sums=sums, plan=plan, dx=None)
    if dxbuf is not None:
        assert bool((dxbuf[0] == SENTINEL).all()) and bool((dxbuf[-1] == SENTINEL).all()), f"{c['name']}: a sentinel row around dx was overwritten"
        assert bool((dxbuf[1:-1, :, cs:] == SENTINEL).all()), f"{c['name']}: stored channels of dx beyond the input channels were overwritten"
        out['dx'] = dxbuf[1:-1].reshape(n, h, w, c['lddx'])
    if sums is not None:
        assert bool((sums[..., cs:] == SENTINEL).all()), f"{c['name']}: sum rows beyond the input channels were overwritten"
    return out


def stored(c, r):
    """float64 (dx (n, h, w, cs) or None, dw, summed rows (2, cs) or None) of a run; nothing may be left unwritten"""
    cs = dims(c)[0]
    dw = r['dw'].double().cpu().numpy()
    assert not np.isnan(dw).any(), f"{c['name']}: {int(np.isnan(dw).sum())} elements of dw are NaN (never written, or summed from a slab that was not)"
    dx = None
    if r['dx'] is not None:
        dx = r['dx'][..., :cs].double().cpu().numpy()
        assert not np.isnan(dx).any(), f"{c['name']}: {int(np.isnan(dx).sum())} elements of dx were never written"
    s = r['sums'][..., :cs].sum(0).cpu().numpy() if r['sums'] is not None else None
    return dx, dw, s


def amax_from_the_pooling_kernel(ops, c, d, lat):
    """arg-max bytes of satcv_bn_relu_pool_amax on the case's own yraw / bn_scale / bn_shift, checked against NumPy's first maximum in row-major
    window order of the activation the kernel stored; on lattice data that activation must itself equal the float64 formula rounded to bf16 (on
    Gaussian data the kernel's fp32 multiply-add may round an element the other way than a float64 evaluation, ties do not occur there)"""
    dev = torch.device('cuda')
    n, h, w, co = c['n'], c['h'], c['w'], c['cout']
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)
    act_d, pooled_d, amax_d = ops.bn_relu_pool_amax(f32(d['y']).to(TD).to(dev).contiguous(), f32(d['sc']).to(dev), f32(d['sh']).to(dev), 2)
    act = act_d.double().cpu().numpy()
    if lat:
        assert np.array_equal(act, rne(np.maximum(d['y'] * d['sc'] + d['sh'], 0))), f"{c['name']}: the stored activation differs from the exact one"
    win = act.reshape(n, h // 2, 2, w // 2, 2, co).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, co, 4)
    got = amax_d.cpu().numpy()
    assert np.array_equal(got, win.argmax(-1)), f"{c['name']}: arg-max bytes differ from the first maximum at {int((got != win.argmax(-1)).sum())} windows"
    assert np.array_equal(pooled_d.double().cpu().numpy(), win.max(-1)), f"{c['name']}: the pooled output is not the maximum of the stored activation"
    ties = float(((win == win.max(-1, keepdims=True)).sum(-1) > 1).mean())
    return got.astype(np.uint8), ties


def check_case(ops, c):
    """every check of one case; returns the record line of profiles/bwd_fused_parity.txt"""
    cs, f, _, thread_px = dims(c)
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(c['name'])) % 2**31
    npix = c['n'] * c['h'] * c['w']
    kdx, kdw = (1.5, 1.5) if c['kind'] == 'bwdf' else (1.0, 0.5)
    use_kernel_amax = c['kind'] == 'bwdf' and c['pool'] and c['amax'] == 'kernel'
    # ---- Gaussian parity (a defer_reduce case: through the deferred sum)
    d = make_data(c, np.random.default_rng(seed), False)
    if use_kernel_amax:
        d['amax'], _ = amax_from_the_pooling_kernel(ops, c, d, False)
    ref = reference(c, d)
    r = run(ops, c, d, c['defer'])
    dx, dw, s = stored(c, r)
    plan = r['plan']
    errs = []
    if dx is not None:
        errs.append(close(dx, ref['dx'], TD, f"dx {c['name']}", k=kdx)[0])
    errs.append(close(dw, ref['dw'] + (d['base'] if c['accumulate'] else 0.0), TD, f"dw {c['name']}", k=kdw)[0])
    if c['bst']:        # sums of the STORED gradient, the tolerances of test_fused_thin_layer_backward / test_convt_bwd_fused
        s1, s2 = sums_of(c, d, ref['a'], dx)
        pre = d['pre'].sum(0) if c['prefill'] else np.zeros((2, cs))
        xh = ref['a'] if c['bst'] == 'act' else (d['x'] - d['bmu']) * d['brs']
        tol = (2e-4 if c['kind'] == 'bwdf' else 3e-3) * np.sqrt(npix) * max(1.0, float(np.abs(dx).max()))
        rt1, rt2 = (1e-4, 1e-4 if c['bst'] == 'act' else 2e-3) if c['kind'] == 'bwdf' else (2e-3, 2e-2)
        at2 = tol * float(np.abs(xh).max()) * (1 if c['kind'] == 'bwdf' and c['bst'] == 'act' else 8)
        np.testing.assert_allclose(s[0] - pre[0], s1, rtol=rt1, atol=tol, err_msg=f"sum g {c['name']}")
        np.testing.assert_allclose(s[1] - pre[1], s2, rtol=rt2, atol=at2, err_msg=f"sum g xhat {c['name']}")
    # ---- integer lattice, bit-exact
    L = lattice(c)
    d = make_data(c, np.random.default_rng(seed + 1), True)
    notes = []
    if use_kernel_amax:
        d['amax'], ties = amax_from_the_pooling_kernel(ops, c, d, True)
        assert ties > 0.2, (c['name'], ties)
        notes.append(f'{100 * ties:.0f}% of the windows tie')
    ref = reference(c, d)
    assert np.abs(ref['dy']).max() * 8 <= L['dy8'] and np.array_equal(ref['dy'] * 8, np.rint(ref['dy'] * 8)), c['name']       # on the lattice, inside the bound
    zeros = float((d['y'] * d['sc'] + d['sh'] == 0).mean())
    assert zeros > 0.08, (c['name'], zeros)
    r = run(ops, c, d, False)
    dx, dw, s = stored(c, r)
    want_dw = ref['dw'] + (d['base'] if c['accumulate'] else 0.0)
    bad = []
    if dx is not None:
        bad.append(('dx', int((dx != ref['dx']).sum()), dx.size, float(np.abs(dx - ref['dx']).max())))
    bad.append(('dw', int((dw != want_dw).sum()), dw.size, float(np.abs(dw - want_dw).max())))
    if c['bst'] and not bad[0][1]:
        # (fp32 per-thread partial sums over the thread's pixels of the workgroup's tiles: exact below 2^24 units of 1 / 8 x the input's grid)
        assert thread_px * plan['tiles_max'] * float(np.abs(ref['dx']).max()) * 8 * L['ua'] < 2 ** 24, c['name']
        s1, s2 = sums_of(c, d, ref['a'], ref['dx'])
        pre = d['pre'].sum(0) if c['prefill'] else np.zeros((2, cs))
        bad.append(('sum g', int((s[0] != s1 + pre[0]).sum()), cs, float(np.abs(s[0] - s1 - pre[0]).max())))
        bad.append(('sum g xhat', int((s[1] != s2 + pre[1]).sum()), cs, float(np.abs(s[1] - s2 - pre[1]).max())))
        notes.append('sums exact' if not (bad[-1][1] or bad[-2][1]) else 'sums NOT exact')
    exact = not any(b[1] for b in bad)
    line = (f"BWDF-PARITY {c['name']:42s} {'/'.join(str(v) for v in c['key']):30s} tiles {plan['tiles']:4d} on {plan['workgroups']:3d}: {plan['tiles_min']}..{plan['tiles_max']}  "
            f"gauss {max(errs):.2e}  lattice a={L['ag']}{L['ay']}{L['ax']}{L['aw']} zero pre-activations {100 * zeros:.0f}% "
            f"{'exact' if exact else 'NOT EXACT'}{' ' + ', '.join(notes) if notes else ''}")
    print(line)
    assert exact, f"{c['name']}: " + '; '.join(f'{k}: {nb} of {tot} differ from the exact reference, max |diff| {md}' for k, nb, tot, md in bad if nb)
    # ---- a second run: bit-identical; a defer_reduce case through the batched sum
    r2 = run(ops, c, d, c['defer'])
    for k in ('dx', 'dw', 'sums'):
        if r[k] is not None:
            assert torch.equal(r[k][..., :cs] if k != 'dw' else r[k], r2[k][..., :cs] if k != 'dw' else r2[k]), \
                f"{c['name']}: {k} of two runs differ{' (in-launch against batched slab sum)' if c['defer'] and k == 'dw' else ''}"
    return line


@pytest.mark.parametrize('case', W.CASES, ids=[c['name'] for c in W.CASES])
def test_bwd_fused_case(ops, case):
    check_case(ops, case)


def hip_runtime():
    """the HIP runtime this process already uses (the copy beside torch, as _lib.py loads it; else by soname)"""
    path = os.path.join(os.path.dirname(torch.__file__), 'lib', 'libamdhip64.so')
    return C.CDLL(path if os.path.exists(path) else 'libamdhip64.so')


def test_plan_query_leaves_no_hip_error(ops):
    """a plan query with a CU count makes no HIP call, one with ncu = 0 asks the device's properties once: neither leaves an error in the runtime"""
    hip = hip_runtime()
    torch.cuda.synchronize()
    assert hip.hipGetLastError() == 0
    for c in W.CASES[:12]:
        W.check_plan(c, ncu=W.NCU)
        g = W.plan_info(c['kind'], W.make_desc(c), 0)
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert g['workgroups'] == min(g['tiles'], cus if c['kind'] == 'bwdf' else max(cus // g['nblk'], 1)), (c['name'], g, cus)
    assert hip.hipPeekAtLastError() == 0


if __name__ == '__main__':      # the record: every case, the same checks, the lines written to profiles/bwd_fused_parity.txt
    from satellite_computervision_amd import ops as _ops
    assert torch.cuda.is_available(), 'the record needs a ROCm device'
    _lines = [check_case(_ops, _c) for _c in W.CASES]
    with open(os.path.join(ROOT, 'profiles', 'bwd_fused_parity.txt'), 'w') as _f:
        _f.write('\n'.join(_lines) + '\n')
    print(f'{len(_lines)} cases written to profiles/bwd_fused_parity.txt')
