"""Device TFRecord pipeline on the GPU: satcv_record_stats / satcv_record_to_tuple (csrc/record_pipeline.hip) and the device= argument
of the tfrecord_io dataset functions, against the reference's own outputs (tests/golden/array_tools_reference.npz) and the NumPy
restatement of to_tuple (tests/record_pipeline_oracle.py).

Exact wherever no mean is involved (the kernel evaluates NumPy's fp32 expressions operation for operation, without FMA contraction).
Where a mean or a variance enters, the bound is measured in the test: the error of the NumPy fp32 computation against float64 on the same
data, times 4 for the different summation order."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, 'golden')
if HERE not in sys.path:
    sys.path.insert(0, HERE)

H = 16
BANDS = ['B2', 'B3', 'B4']


def _mods():
    import record_pipeline_oracle as O
    from satellite_computervision_amd import tfrecord_io as tio
    return tio, O


def _np(t):
    return t.detach().cpu().numpy()


def _params(rng, n, nband):
    p = np.empty((n, 2 * nband + 3), np.float32)
    p[:, :2 * nband] = rng.uniform(0.95, 1.05, (n, 2 * nband))
    p[:, 2 * nband:2 * nband + 2] = rng.random((n, 2)) < 0.5
    p[:, 2 * nband + 2] = rng.integers(0, 4, n)
    return p


def test_reference_fixtures_exact():
    """rescale_array by moments and over axes (0, 1), and all 16 flip / rot90 combinations of aug_array_morph -- different ones on the
    samples of ONE launch -- reproduce the reference's own outputs bit for bit."""
    tio, O = _mods()
    z = np.load(os.path.join(GOLD, 'array_tools_reference.npz'))
    img = z['rescale_in']                                                   # (16, 16, 4)
    planes = np.ascontiguousarray(np.transpose(img, (2, 0, 1)))[None]
    x, y, _ = tio.device_to_tuple(planes, ['band'] * 4, None, color=False, morph=False, moments=[(0, 3000)] * 4)
    assert y is None and np.array_equal(_np(x)[0], z['rescale_moments'])
    x, _, _ = tio.device_to_tuple(planes, ['band'] * 4, None, color=False, morph=False, axes=[0, 1])
    assert np.array_equal(_np(x)[0], z['rescale_axes01'])
    m = z['morph_in']                                                       # (2, 8, 8, 3)
    combos = [(v, h, r) for v in (0, 1) for h in (0, 1) for r in range(4)]
    for s in range(2):
        planes = np.ascontiguousarray(np.broadcast_to(np.transpose(m[s], (2, 0, 1)), (16, 3, 8, 8)))
        prm = np.ones((16, 9), np.float32)
        for i, (v, h, r) in enumerate(combos):                              # aug_array_morph(v, h): v flips axis 1 (up-down), h axis 2
            prm[i, 6:] = (h, v, r)
        x, _, _ = tio.device_to_tuple(planes, ['band'] * 3, prm, color=False, morph=True, mode=None)
        for i, (v, h, r) in enumerate(combos):
            assert np.array_equal(_np(x)[i], z[f'morph_{v}{h}{r}'][s]), (s, v, h, r)


@pytest.mark.parametrize('response', ['raw', 'onehot'])
def test_mean_free_paths_exact(response):
    """axes=[2] per-pixel rescale within `splits`, colour with the host's m_c injected, one-hot features, a raw response with values
    above 1 / a one-hot response, flips and rotations: bit-identical to the fp32 restatement of to_tuple; the channels beside the
    written slice of a wider tensor stay untouched.  Also at 40 x 40 (partial tiles) and with 9 planes (the 16 x 16 tile variant)."""
    tio, O = _mods()
    rng = np.random.default_rng(5)
    for hw, nband, splits in ((16, 4, [3, 1]), (40, 5, [2, 3]), (24, 7, None)):
        n = 5
        bands = (rng.random((n, nband, hw, hw)) * 3000).astype(np.float32)
        cat = rng.integers(0, 4, (n, 1, hw, hw)).astype(np.float32)
        resp = rng.integers(0, 4, (n, 1, hw, hw)).astype(np.float32)
        planes = np.concatenate([bands, cat] + ([cat] if nband == 7 else []) + [resp], axis=1)
        kinds = [(O.BAND, 0)] * nband + [(O.ONEHOT, 3)] * (2 if nband == 7 else 1) + [(O.RESPONSE, 0) if response == 'raw' else (O.RESPONSE_ONEHOT, 3)]
        prm = _params(rng, n, nband)
        mean = O.channel_means(planes, kinds)
        xw, yw = O.to_tuple(planes, kinds, prm, splits=splits, mean=mean)
        nx, ny = xw.shape[3], yw.shape[3]
        xt = torch.full((n, hw, hw, nx + 5), -7.0, device='cuda')
        yt = torch.full((n, hw, hw, ny + 3), -7.0, device='cuda')
        names = {O.BAND: 'band', O.ONEHOT: 'onehot', O.RESPONSE: 'response', O.RESPONSE_ONEHOT: 'response_onehot'}
        x, y, _ = tio.device_to_tuple(planes, [(names[c], d) for c, d in kinds], prm, splits=splits, mean=mean, x=xt, coff_x=2, y=yt, coff_y=1)
        assert x is xt and y is yt
        x, y = _np(x), _np(y)
        assert np.array_equal(x[..., 2:2 + nx], xw) and np.array_equal(y[..., 1:1 + ny], yw)
        assert np.all(x[..., :2] == -7.0) and np.all(x[..., 2 + nx:] == -7.0) and np.all(y[..., :1] == -7.0) and np.all(y[..., 1 + ny:] == -7.0)
        if response == 'raw':
            assert resp.max() > 1 and set(np.unique(y[..., 1])) <= {0.0, 1.0}
        # axes [0, 1, 2] (min / max of a whole group, through the monotone colour map) is mean-free as well
        xw, _ = O.to_tuple(planes, kinds, prm, splits=splits, mean=mean, axes=(0, 1, 2))
        x, _, _ = tio.device_to_tuple(planes, [(names[c], d) for c, d in kinds], prm, splits=splits, mean=mean, axes=[0, 1, 2])
        assert np.array_equal(_np(x), xw)
        xw, _ = O.to_tuple(planes, kinds, prm, mean=mean, axes=(0, 1))
        x, _, _ = tio.device_to_tuple(planes, [(names[c], d) for c, d in kinds], prm, mean=mean, axes=[0, 1])
        assert np.array_equal(_np(x), xw)


def test_statistics():
    """satcv_record_stats against float64 NumPy on 256 x 256 and 12 x 12 planes: min / max exact; mean and variance within 4 x the error
    of NumPy's own fp32 mean / var against float64 on the same plane, plane by plane."""
    tio, O = _mods()
    rng = np.random.default_rng(9)
    for hw in (256, 12):
        planes = (rng.random((3, 4, hw, hw)) * 3000).astype(np.float32)
        planes[1, 2] += 40000.0                                             # a large mean over a small spread
        planes[2, 1] = rng.normal(0, 1, (hw, hw)).astype(np.float32)
        _, _, _, stats = tio.device_to_tuple(planes, ['band'] * 3 + ['response'], None, color=False, morph=False, mode=None, return_stats=True)
        st = _np(stats)[:, :3]
        p64 = planes[:, :3].astype(np.float64)
        assert np.array_equal(st[..., 1], planes[:, :3].min((2, 3)).astype(np.float64)) and np.array_equal(st[..., 2], planes[:, :3].max((2, 3)).astype(np.float64))
        mean64, var64 = p64.mean((2, 3)), p64.var((2, 3))
        bound_mean = 4 * np.abs(planes[:, :3].mean((2, 3)).astype(np.float64) - mean64)          # (sample, plane)
        bound_var = 4 * np.abs(planes[:, :3].var((2, 3)).astype(np.float64) - var64)
        err_mean, err_var = np.abs(st[..., 0] - mean64), np.abs(st[..., 3] - var64)
        with np.printoptions(precision=2):
            print(f'stats {hw}: mean err {err_mean.ravel()} bound {bound_mean.ravel()}\n          var err {err_var.ravel()} bound {bound_var.ravel()}')
        assert np.all(err_mean <= bound_mean) and np.all(err_var <= bound_var)


def _write(tio, path, seed, n, hw=H):
    rng = np.random.default_rng(seed)
    recs = []
    with tio.TFRecordWriter(path, compression='GZIP') as w:
        for _ in range(n):
            lab = (rng.random((hw, hw)) < 0.4).astype(np.float32)
            d = {b: (rng.random((hw, hw)) * 3000).astype(np.float32) for b in BANDS}
            d['lc'] = lab.copy()
            d['landcover'] = lab * 3.0
            recs.append(d)
            w.write(tio.encode_example({k: v.reshape(-1) for k, v in d.items()}))
    return recs


def _ft(tio, hw=H):
    return {k: tio.FixedLenFeature([hw, hw]) for k in BANDS + ['lc', 'landcover']}


def test_end_to_end_with_colour(tmp_path):
    """get_training_dataset / get_eval_dataset / make_pred_dataset with device=None and device='cuda' after the same set_seed, over two
    passes of repeat() with a ragged last batch: same number of batches, same shapes, labels and one-hot channels bit-identical (same
    draws, same shuffle order, same morph).  The bands are compared with the float64 oracle given the draws the chain recorded, within
    4 x the error of the HOST fp32 path against that oracle on the same record.  Measured for these inputs: host fp32 against float64
    8.2e-06 (training, per-pixel rescale), 1.2e-07 (evaluation, moments) -- the bound is computed in the test, not these constants."""
    tio, O = _mods()
    path = str(tmp_path / 'train.tfrecord.gz')
    _write(tio, path, 3, 10)
    feats = BANDS + ['lc']
    kinds = [(O.BAND, 0)] * 3 + [(O.ONEHOT, 2), (O.RESPONSE_ONEHOT, 4)]
    kw = dict(buff=4, batch=4, one_hot={'lc': 2})
    tio.set_seed(1)
    host = [b for b, _ in zip(tio.get_training_dataset([path], _ft(tio), feats, {'landcover': 4}, **kw), range(6))]
    tio.set_seed(1)
    ds = tio.get_training_dataset([path], _ft(tio), feats, {'landcover': 4}, device='cuda', **kw)
    dev = [b for b, _ in zip(ds, range(6))]
    tio.set_seed(1)
    raw = [b for b, _ in zip(ds._source(), range(6))]                       # the (planes, params) batches behind them
    assert len(dev) == len(host) == 6 and [b[0].shape[0] for b in host] == [4, 4, 2, 4, 4, 2]
    for (xh, yh), (xd, yd), (planes, prm) in zip(host, dev, raw):
        assert xd.is_cuda and yd.is_cuda and xd.dtype == torch.float32 and tuple(xd.shape) == xh.shape and tuple(yd.shape) == yh.shape
        xd, yd = _np(xd), _np(yd)
        assert np.array_equal(yd, yh) and np.array_equal(xd[..., 3:], xh[..., 3:])
        x64, _ = O.to_tuple(planes, kinds, prm, dtype=np.float64)
        bound = 4 * np.abs(xh[..., :3] - x64[..., :3]).max(axis=(1, 2, 3))                       # per record
        err = np.abs(xd[..., :3] - x64[..., :3]).max(axis=(1, 2, 3))
        with np.printoptions(precision=2):
            print(f'training bands: device err {err}, host err x 4 {bound}')
        assert np.all(bound > 0) and np.all(err <= bound)

    kinds = [(O.BAND, 0)] * 3 + [(O.ONEHOT, 2), (O.RESPONSE, 0)]
    ekw = dict(one_hot={'lc': 2}, moments=[(0, 3000)] * 3)
    tio.set_seed(2)
    host = list(tio.get_eval_dataset([path], _ft(tio), feats, 'landcover', **ekw))
    tio.set_seed(2)
    ds = tio.get_eval_dataset([path], _ft(tio), feats, 'landcover', device='cuda', read_ahead=2, **ekw)
    dev = list(ds)
    tio.set_seed(2)
    raw = list(ds._source())
    assert len(dev) == len(host) == 10
    hx = np.concatenate([b[0] for b in host])
    dx, dy = np.concatenate([_np(b[0]) for b in dev]), np.concatenate([_np(b[1]) for b in dev])
    assert dx.shape == hx.shape == (10, H, H, 5)
    assert np.array_equal(dy, np.concatenate([b[1] for b in host])) and np.array_equal(dx[..., 3:], hx[..., 3:])
    x64, _ = O.to_tuple(np.concatenate([r[0] for r in raw]), kinds, np.concatenate([r[1] for r in raw]), moments=[(0, 3000)] * 3, dtype=np.float64)
    bound = 4 * np.abs(hx[..., :3] - x64[..., :3]).max(axis=(1, 2, 3))                           # per record
    err = np.abs(dx[..., :3] - x64[..., :3]).max(axis=(1, 2, 3))
    with np.printoptions(precision=2):
        print(f'evaluation bands: device err {err}, host err x 4 {bound}')
    assert np.all(bound > 0) and np.all(err <= bound)

    # prediction: non-square patches, a custom band function (appended after the rescale) and a one-hot feature: no mean -> exact
    ppath = str(tmp_path / 'pred.tfrecord.gz')
    rng = np.random.default_rng(4)
    with tio.TFRecordWriter(ppath, compression='GZIP') as w:
        for _ in range(3):
            d = {b: (rng.random((12, 20)) * 3000).astype(np.float32) for b in ['B4', 'B8']}
            d['lc'] = rng.integers(0, 3, (12, 20)).astype(np.float32)
            w.write(tio.encode_example({k: v.reshape(-1) for k, v in d.items()}))
    pkw = dict(kernel_shape=[8, 16], kernel_buffer=[4, 4], one_hot={'lc': 3}, ndvi=tio.calc_ndvi)
    for extra in (dict(), dict(axes=[0, 1]), dict(moments=[(0, 3000)] * 2)):
        host = list(tio.make_pred_dataset([ppath], ['B4', 'B8', 'lc'], **pkw, **extra))
        dev = list(tio.make_pred_dataset([ppath], ['B4', 'B8', 'lc'], device='cuda', **pkw, **extra))
        assert len(dev) == len(host) == 3
        for a, b in zip(host, dev):
            assert b.is_cuda and tuple(b.shape) == a.shape == (1, 12, 20, 6) and np.array_equal(_np(b), a)


def test_normalize_mode():
    """normalize_array over axes (0, 1) of the reference fixture, and normalize_tensor with `splits` and pass-through channels (per
    pixel, per channel and over whole groups, with and without colour): device against the float64 oracle within 4 x the error of the NumPy fp32 computation (the
    fixture / the host normalize_tensor) against the same oracle."""
    tio, O = _mods()
    z = np.load(os.path.join(GOLD, 'array_tools_reference.npz'))
    img = z['rescale_in']
    planes = np.ascontiguousarray(np.transpose(img, (2, 0, 1)))[None]
    kinds = [(O.BAND, 0)] * 4
    x64, _ = O.to_tuple(planes, kinds, None, color=False, morph=False, mode='normalize', axes=(0, 1), dtype=np.float64)
    x, _, _ = tio.device_to_tuple(planes, ['band'] * 4, None, color=False, morph=False, mode='normalize', axes=[0, 1])
    bound = 4 * np.abs(z['normalize_axes01'].astype(np.float64) - x64[0]).max(axis=(0, 1))      # per channel
    err = np.abs(_np(x)[0] - x64[0]).max(axis=(0, 1))
    print(f'normalize_axes01: device err {err}, fixture err x 4 {bound}')
    assert np.all(bound > 0) and np.all(err <= bound)
    rng = np.random.default_rng(2)
    n, nband, hw = 3, 5, 24
    planes = (rng.random((n, nband, hw, hw)) * 3000).astype(np.float32)
    kinds = [(O.BAND, 0)] * nband
    prm = _params(rng, n, nband)
    for axes, color in (([2], True), ([0, 1], True), ([0, 1], False), ([0, 1, 2], False), ([0, 1, 2], True)):
        x64, _ = O.to_tuple(planes, kinds, prm, color=color, mode='normalize', axes=tuple(axes), splits=[2, 2], dtype=np.float64)
        x32, _ = O.to_tuple(planes, kinds, prm, color=color, mode='normalize', axes=tuple(axes), splits=[2, 2], dtype=np.float32)
        x, _, _ = tio.device_to_tuple(planes, ['band'] * nband, prm, color=color, mode='normalize', axes=axes, splits=[2, 2])
        bound = 4 * np.abs(x32 - x64).max(axis=(1, 2))                                          # per record and channel
        err = np.abs(_np(x) - x64).max(axis=(1, 2))
        with np.printoptions(precision=2):
            print(f'normalize axes {axes} colour {color}: device err {err.ravel()}\n    host err x 4 {bound.ravel()}')
        assert np.all(bound[:, :4] > 0) and np.all(err <= bound)            # (the pass-through channel is exact without colour: 0 <= 0)
        # the fifth channel is outside the groups: coloured (or raw) values, not standardised
        assert np.abs(_np(x)[..., 4]).max() > 100


def test_determinism():
    """The same batch twice gives identical bytes, and a sample's result does not depend on which samples share its batch."""
    tio, O = _mods()
    rng = np.random.default_rng(8)
    n, hw = 5, 256
    planes = np.concatenate([(rng.random((n, 4, hw, hw)) * 3000).astype(np.float32), rng.integers(0, 3, (n, 2, hw, hw)).astype(np.float32)], axis=1)
    kinds = ['band'] * 4 + [('onehot', 3), 'response']
    prm = _params(rng, n, 4)
    for axes in ([2], [0, 1]):
        a = tio.device_to_tuple(planes, kinds, prm, axes=axes)
        b = tio.device_to_tuple(planes, kinds, prm, axes=axes)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for i in (0, 3):
            one = tio.device_to_tuple(planes[i:i + 1], kinds, prm[i:i + 1], axes=axes)
            assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[1][0], a[1][i])


def test_model_fit_consumes_the_device_dataset(tmp_path):
    """Model.fit straight from the device dataset: finite loss, and the tensors the dataset yielded are the very objects the training step
    received (device tensors, no host copy of the batch in between)."""
    tio, O = _mods()
    from satellite_computervision_amd import model_tools as mt
    path = str(tmp_path / 'train.tfrecord.gz')
    _write(tio, path, 3, 10)
    feats = BANDS + ['lc']
    tio.set_seed(1)
    ds = tio.get_training_dataset([path], _ft(tio), feats, {'landcover': 2}, buff=4, batch=4, one_hot={'lc': 2}, device='cuda')
    yielded = []

    class Tap:
        def __iter__(self):
            for b in ds:
                yielded.append(b)
                yield b
    mt.reset_uids()
    m = mt.get_unet_model(2, 5, filters=[16, 32], factors=[2, 2])
    m.compile(optimizer=mt.Adam(1e-3), loss=lambda a, b: mt.weighted_categorical_crossentropy(a, b, [1.0, 2.0]))
    received = []
    step = m.train_step_device

    def spy(xb, yb, *a, **k):
        received.append((xb, yb))
        return step(xb, yb, *a, **k)
    m.train_step_device = spy
    hist = m.fit(Tap(), epochs=1, steps_per_epoch=4, verbose=0)
    assert len(received) == 4 and np.all(np.isfinite(hist.history['loss']))
    for (xb, yb), (xy, yy) in zip(received, yielded):
        assert xb is xy and yb is yy and isinstance(xb, torch.Tensor) and xb.is_cuda and yb.is_cuda
        assert xb.dtype == torch.float32 and xb.is_contiguous() and tuple(xb.shape[1:]) == (H, H, 5) and tuple(yb.shape[1:]) == (H, H, 2)


def test_refusals(tmp_path):
    """Argument checks only: each call returns the library's error (or the Python refusal) and leaves the destination untouched -- no
    launch was started."""
    tio, O = _mods()
    from satellite_computervision_amd._lib import SatcvError
    rng = np.random.default_rng(0)
    sq = (rng.random((2, 3, 8, 8))).astype(np.float32)
    prm = _params(rng, 2, 2)
    kinds = ['band', 'band', 'response']

    def untouched(fn, match, shape=(2, 8, 8, 2)):
        x = torch.full(shape, -3.0, device='cuda')
        y = torch.full(shape[:3] + (1,), -3.0, device='cuda')
        with pytest.raises(SatcvError, match=match):
            fn(x, y)
        torch.cuda.synchronize()
        assert torch.all(x == -3.0) and torch.all(y == -3.0)

    rect = rng.random((2, 3, 8, 12)).astype(np.float32)
    untouched(lambda x, y: tio.device_to_tuple(rect, kinds, prm, x=x, y=y), 'square tiles', (2, 8, 12, 2))
    untouched(lambda x, y: tio.device_to_tuple(sq, ['band', 9, 'response'], prm, x=x, y=y), 'unknown plane kind')
    untouched(lambda x, y: tio.device_to_tuple(sq, kinds, prm, x=x, coff_x=1, y=y), 'ld_x')
    untouched(lambda x, y: tio.device_to_tuple(sq, kinds, None, x=x, y=y, color=False), 'parameter table')
    untouched(lambda x, y: tio.device_to_tuple(sq, kinds, prm[:, :5].copy(), x=x, y=y), 'parameter table')
    # training datasets refuse non-square tiles in Python, before anything is uploaded
    path = str(tmp_path / 'r.tfrecord.gz')
    with tio.TFRecordWriter(path, compression='GZIP') as w:
        w.write(tio.encode_example({'B2': np.zeros(8 * 12, np.float32), 'landcover': np.zeros(8 * 12, np.float32)}))
    ft = {k: tio.FixedLenFeature([8, 12]) for k in ('B2', 'landcover')}
    with pytest.raises(ValueError, match='square'):
        list(tio.get_eval_dataset([path], ft, ['B2'], 'landcover', device='cuda'))
