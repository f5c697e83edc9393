"""The float64 restatements of tests/elementwise_oracle.py against independent implementations that every machine has (torch on the
CPU, in float64), on the shapes the GPU file uses; and the "share left out" of the two checks that set ambiguous elements aside
(classes of the up-sampling head near a tie, e4m3 roundings near a boundary) stays under its 1 % cap for the seeds the GPU file uses,
so that the cap is met by construction."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_oracle as O  # noqa: E402

POOL_WINDOWS = [(2, 2, 0), (3, 2, 1), (3, 1, 1), (3, 2, 0), (1, 2, 0)]
POOL_MAPS = [(2, 8, 8, 8), (3, 7, 9, 8), (1, 5, 4, 16), (3, 2, 2, 8), (1, 3, 3, 24), (2, 16, 17, 40)]


def nchw(x):
    return torch.tensor(x).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('win', POOL_WINDOWS)
@pytest.mark.parametrize('shape', POOL_MAPS)
def test_maxpool_restatement_is_torch_max_pool2d(win, shape):
    k, s, pad = win
    n, h, w, c = shape
    if O.pool_out(h, k, s, pad) < 1 or O.pool_out(w, k, s, pad) < 1:
        with pytest.raises(AssertionError):
            O.maxpool(np.zeros(shape), k, s, pad)
        return
    rng = np.random.default_rng(k * 100 + s * 10 + pad)
    for x in (rng.standard_normal(shape), -1.0 - rng.random(shape)):           # all-negative: zero padding would win every border window
        ref = nhwc(F.max_pool2d(nchw(x), k, s, padding=pad))
        got = O.maxpool(x, k, s, pad)
        assert got.shape == ref.shape == (n, O.pool_out(h, k, s, pad), O.pool_out(w, k, s, pad), c)
        assert np.array_equal(got, ref)
    if pad:
        assert O.maxpool(-1.0 - rng.random(shape), k, s, pad).max() < 0


def test_maxpool_map_smaller_than_window_needs_padding():
    x = -np.arange(1.0, 1 + 2 * 2 * 8).reshape(1, 2, 2, 8)
    assert O.pool_out(2, 3, 2, 0) == 0 and O.pool_out(2, 3, 2, 1) == 1
    assert np.array_equal(O.maxpool(x, 3, 2, 1), x.max((1, 2), keepdims=True))


@pytest.mark.parametrize('case', O.upsample_cases())
def test_upsample_head_restatement_and_share_left_out(case):
    n, h, w, ncls, f, act, thresh = case
    lg = O.upsample_logits(case).astype(np.float64)
    ref = nhwc(F.interpolate(nchw(lg), scale_factor=f, mode='bilinear', align_corners=False))
    z = O.upsample_bilinear(lg, f)
    assert z.shape == (n, h * f, w * f, ncls)
    assert np.abs(z - ref).max() <= 1e-13 * max(np.abs(ref).max(), 1.0)
    p, cls, margin = O.upsample_head(lg, f, act, thresh)
    pt = torch.softmax(torch.tensor(ref), -1) if act == 0 else torch.sigmoid(torch.tensor(ref))
    assert np.abs(p - pt.numpy()).max() <= 1e-13
    if act == 0:
        sure = margin > 1e-9
        assert np.array_equal(cls[sure], pt.argmax(-1).numpy()[sure])
        assert cls.shape == (n, h * f, w * f)
    else:
        assert cls.shape == p.shape and np.array_equal(cls == 1, p > np.float32(thresh))
    bound = O.close_tol('f32') * max(np.abs(p).max(), 1e-6)
    left_out = float((margin <= bound).mean())
    assert left_out < 0.01, f'{case}: {left_out:.4%} of the pixels within {bound:.1e} of a tie'


def test_upsample_half_pixel_centres_by_hand():
    """factor 2 on a row [0, 4]: sources at -0.25, 0.25, 0.75, 1.25 -> 0, 1, 3, 4 (edge clamped); dropping the half-pixel shift would
    give 0, 2, 4, 4"""
    x = np.array([0.0, 4.0]).reshape(1, 1, 2, 1)
    assert np.array_equal(O.upsample_bilinear(x, 2), np.array([0.0, 1.0, 3.0, 4.0] * 2).reshape(1, 2, 4, 1))
    assert np.array_equal(O.upsample_bilinear(x, 1), x)


def test_upsample_ties_go_to_the_lower_index():
    lg = np.zeros((1, 2, 2, 3)); lg[..., 0] = -1.0
    _, cls, margin = O.upsample_head(lg, 2, 0)
    assert (cls == 1).all() and (margin == 0).all()


@pytest.mark.parametrize('cin,ncls', [(16, 1), (32, 3), (64, 2), (24, 2), (32, 5)])
@pytest.mark.parametrize('affine', [False, True])
def test_head_bwd_restatement_is_autograd(cin, ncls, affine):
    rng = np.random.default_rng(cin + ncls)
    npix = 77
    x, w, dl = rng.standard_normal((npix, cin)), rng.standard_normal((cin, ncls)), rng.standard_normal((npix, ncls))
    sc, sh = (rng.uniform(0.5, 1.5, cin), rng.standard_normal(cin)) if affine else (None, None)
    xt = torch.tensor(x)
    a = (torch.relu(xt * torch.tensor(sc) + torch.tensor(sh)) if affine else xt).detach().requires_grad_(True)
    wt, bt = torch.tensor(w, requires_grad=True), torch.zeros(ncls, dtype=torch.float64, requires_grad=True)
    ((a @ wt + bt) * torch.tensor(dl)).sum().backward()
    dx, dw, db = O.head_bwd(x, sc, sh, w, dl)
    for got, ref in ((dx, a.grad), (dw, wt.grad), (db, bt.grad)):
        assert np.abs(got - ref.numpy()).max() <= 1e-12 * max(np.abs(ref.numpy()).max(), 1.0)


@pytest.mark.parametrize('ya,ra,relu', [(a, b, r) for a in (0, 1) for b in (0, 1) for r in (0, 1)])
def test_add_act_and_relu_bwd_and_bias_grad_restatements(ya, ra, relu):
    rng = np.random.default_rng(ya * 4 + ra * 2 + relu)
    c = 24
    y, res = rng.standard_normal((3, 5, 7, c)), rng.standard_normal((3, 5, 7, c))
    s0, h0, s1, h1 = (rng.standard_normal(c) for _ in range(4))
    yt = torch.tensor(y, requires_grad=True)
    u = (yt * torch.tensor(s0) + torch.tensor(h0) if ya else yt) + (torch.tensor(res) * torch.tensor(s1) + torch.tensor(h1) if ra else torch.tensor(res))
    out = torch.relu(u) if relu else u
    got = O.add_act(y, s0 if ya else None, h0 if ya else None, res, s1 if ra else None, h1 if ra else None, relu)
    assert np.abs(got - out.detach().numpy()).max() <= 1e-14 * 10
    # the gradient through the ReLU of a materialised activation, and its per-channel sum
    if relu and not ya:
        g = rng.standard_normal(y.shape)
        out.backward(torch.tensor(g))
        assert np.array_equal(O.relu_bwd(out.detach().numpy(), g), yt.grad.numpy())
        assert np.abs(O.bias_grad(g) - torch.tensor(g).sum((0, 1, 2)).numpy()).max() <= 1e-12
        assert (O.bias_grad_bound(g) > 0).all()


def test_relu_bwd_zeros_and_denormals():
    act = np.array([0.0, -0.0, 1e-40, -1e-40, 2.0, -2.0])
    assert np.array_equal(O.relu_bwd(act, np.full(6, 7.0)), [0, 0, 7, 0, 7, 0])


def test_e4m3_rounding_is_torch_float8_e4m3fn():
    codes = np.arange(256, dtype=np.uint8)
    dec = torch.tensor(codes).view(torch.float8_e4m3fn).double().numpy()
    mine = O.e4m3_decode(codes)
    assert np.array_equal(np.isnan(dec), np.isnan(mine)) and np.array_equal(dec[~np.isnan(dec)], mine[~np.isnan(dec)])
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(200000) * s for s in (0.01, 1.0, 50.0, 300.0)]).astype(np.float32)
    fin = dec[~np.isnan(dec)]
    mids = ((np.sort(fin)[1:] + np.sort(fin)[:-1]) / 2).astype(np.float32)                  # every tie, exactly representable
    v = np.concatenate([v, mids, fin.astype(np.float32), np.float32([448.0, 464.0, 465.0, 1e6, -1e6, 2.0 ** -10, 2.0 ** -11, 0.0])])
    ref = torch.tensor(np.clip(v, -448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = O.e4m3_round(v.astype(np.float64))
    nz = v != 0                                                                              # the sign of a zero is not compared
    assert np.array_equal(got[nz], ref[nz])
    assert not np.isnan(O.e4m3_decode(got)).any() and np.abs(O.e4m3_decode(got)).max() == 448.0


def test_storage_roundings_are_torch():
    x = (np.random.default_rng(1).standard_normal(100000) * 40).astype(np.float32)
    assert np.array_equal(O.bf16_round(x), torch.tensor(x).bfloat16().float().numpy())
    assert np.array_equal(O.to_storage(x, 'fp8'), torch.tensor(x).clamp(-448, 448).to(torch.float8_e4m3fn).double().numpy())


@pytest.mark.parametrize('pair', [p for p in O.REQUANT_PAIRS if p[1] == 'fp8'])
@pytest.mark.parametrize('shape', O.REQUANT_SHAPES + [(4099, 2048)])
@pytest.mark.parametrize('relu', [0, 1])
def test_requant_share_near_a_rounding_boundary(pair, shape, relu):
    npix, c = shape
    x, sc, sh = O.requant_inputs(npix, c, pair[0], seed=npix + c + relu)
    val, lo, hi, amb = O.affine_requant_fp8(x, sc, sh, relu)
    assert ((lo <= val) & (val <= hi)).all()
    assert amb.mean() < 0.01, f'{amb.mean():.4%} ambiguous'
    assert (np.abs(O.affine(x, sc, sh)) > O.E4M3_MAX).mean() > 0.001                           # saturation is exercised
    assert not np.isnan(val).any() and np.abs(val).max() == O.E4M3_MAX
    # away from the boundaries the value is torch's rounding of the float32 arithmetic
    pre = torch.tensor(x).float() * torch.tensor(sc) + torch.tensor(sh)
    pre = torch.relu(pre) if relu else pre
    ref = pre.clamp(-448, 448).to(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(val[~amb], ref[~amb])


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('fused', [False, True])
def test_dropout_apply_restatement(mode, fused):
    rng = np.random.default_rng(mode * 2 + fused)
    n, hw, c = 3, 7 * 9, 24
    x = rng.standard_normal((n * hw, c))
    mask = (rng.random((n if mode == 0 else n * hw, c)) > 0.3) * 2.0
    sc, sh = (rng.standard_normal(c), rng.standard_normal(c)) if fused else (None, None)
    a = torch.tensor(x).reshape(n, hw, c)
    if fused:
        a = torch.relu(a * torch.tensor(sc) + torch.tensor(sh))
    m = torch.tensor(mask).reshape(n, 1 if mode == 0 else hw, c)
    assert np.abs(O.dropout_apply(x, mask, mode, hw, sc, sh, True) - (a * m).reshape(-1, c).numpy()).max() <= 1e-14


@pytest.mark.parametrize('rate', [0.0, 0.1, 0.25, 0.5, 0.9])
def test_dropout_keep_value_has_one_reading(rate):
    """float32(1 / (1 - rate)) is the same number whether the division is carried out in float32 or in float64, for the tested rates"""
    r = np.float32(rate)
    assert O.dropout_keep_value(rate) == np.float32(1.0) / (np.float32(1.0) - r)
    assert O.dropout_keep_value(0.0) == 1.0
    assert O.five_sigma(0.5, 2 ** 22) == pytest.approx(5 * 0.5 / 2048)


def test_ingest_and_confusion_restatements():
    rng = np.random.default_rng(3)
    src = rng.random((11, 13)).astype(np.float32)
    out = O.ingest_scaled_f32(src, 16, 37.5)
    assert np.array_equal(out[:, :13], (torch.tensor(src) * 37.5).numpy()) and not out[:, 13:].any()
    for ncls in range(1, 9):
        cls, lab = rng.integers(0, ncls, 500), rng.integers(0, ncls, 500)
        ref = torch.bincount(torch.tensor(lab * ncls + cls), minlength=ncls * ncls).reshape(ncls, ncls).numpy()
        got = O.confusion(cls, np.eye(ncls, dtype=np.float32)[lab], ncls)
        assert got.dtype == np.int64 and np.array_equal(got, ref) and got.sum() == 500


def test_past_cap_sizes_follow_the_documented_default():
    assert O.grid_cap_threads() == 1536 * 256
    n, h, w, ncls, f = O.upsample_cases()[-1][:5]
    assert n * h * f * w * f >= 2 * O.grid_cap_threads()
