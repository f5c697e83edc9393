"""Pins tests/input_kernels_oracle.py, which tests/test_input_kernels_gpu.py holds the input and packing kernels to, on a machine without
a GPU:
  tile_ingest / label_onehot   bit for bit against oracle/input_pipeline.py (the line-by-line restatement of the reference's generators)
                               on every case that one can express -- a constant fill for the draws, non-square tiles, odd trims, all seven
                               kinds -- and against the recorded outputs of the reference's own aug_array_morph / aug_array_color
  pack_image                   to the semantics, not to the kernel: used as the B operand of a GEMM over (tap, k) in float64 the four
                               images reproduce conv2d 'same', its input gradient (torch float64 autograd), conv2d-transpose (k == s) and
                               that operator's input gradient, for ragged cin / cout, at 1e-12
  the inputs of the GPU file   really contain what their names say (thresholds and neighbours, exact sums, few ambiguous draws)
One case the restatement cannot express bit for bit: SiameseDataGenerator turns float32 planes into float64 before its colour step,
where the kernel (and the oracle, as include/satcv.h documents) keeps float32 planes in float32 -- the values are compared without the
colour step there, the mask with it."""
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
import input_kernels_oracle as I  # noqa: E402
from oracle import input_pipeline as ip  # noqa: E402
from oracle import keras_ops as K  # noqa: E402

GOLD = os.path.join(HERE, 'golden')
FILL = 777.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def tile_cases():
    """(kind, (h, w), (hin, win)) over every kind, tile and trim parity"""
    return [(k, hw, src) for k in I.KIND_NAMES for hw, even, odd in I.TILE_SHAPES for src in (even, odd)]


# ------------------------------------------------------------------------------ tile_ingest
@pytest.mark.parametrize('kind,hw,src', tile_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_tile_ingest_is_the_reference_generator(kind, hw, src):
    """UNETDataGenerator's source path: rescale, trim, colour about np.nanmean, morph; mask mode 1 with and without replacement"""
    (h, w), (hin, win) = hw, src
    for c in (1, 3, 4):
        for rescale in (I.RESCALE[kind], 0.0):
            planes = I.make_planes(kind, (3, c, hin, win), seed=c + hin, nan_frac=0.02, low_frac=0.03, rescale=rescale, mode=1)
            with np.errstate(invalid='ignore'):
                d = ip.get_unet_data(list(planes), (h, w), rescale if rescale else False)
                assert d.dtype == (np.float32 if kind == 'f32' else np.float64 if rescale else planes.dtype)     # integers become double in the colour step
                mu = np.nanmean(d, axis=(1, 2))
                for morph, color in (((0, 0, 0), None), ((1, 0, 3), (0.97, 1.04)), ((0, 1, 1), (1.05, 0.95)), ((1, 1, 2), None)):
                    ref = ip.aug_array_color(d, *color) if color else d
                    ref = ip.aug_array_morph(ref, *morph).astype(np.float32)
                    got = I.tile_ingest(planes, h, w, rescale, ch_mean=mu if color else None, contra=color[0] if color else 1.0,
                                        bright=color[1] if color else 1.0, flip_v=morph[0], flip_h=morph[1], rot=morph[2])
                    assert same_bits(got, ref), (c, rescale, morph, color)
                for replace in (1, 0):
                    ref = ip.get_unet_data([p.copy() for p in planes], (h, w), rescale if rescale else False, add_nan_mask=True, to_fit=bool(replace),
                                           fill=lambda k: np.full(k, FILL))
                    for morph in ((0, 0, 0), (0, 1, 3)):
                        got = I.tile_ingest(planes, h, w, rescale, nan_mask=1, replace=replace, fill=FILL, flip_v=morph[0], flip_h=morph[1], rot=morph[2])
                        assert same_bits(got, ip.aug_array_morph(ref, *morph).astype(np.float32)), (c, rescale, replace, morph)


@pytest.mark.parametrize('kind,hw,src', tile_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_tile_ingest_mode_2_is_the_siamese_generator(kind, hw, src):
    (h, w), (hin, win) = hw, src
    c, n = 3, 3
    planes = I.make_planes(kind, (n, c, hin, win), seed=hin * 7 + h, nan_frac=0.03, low_frac=0.04, rescale=10000.0, mode=2)
    labels = [np.ones((hin, win), np.uint8)] * n
    fill = lambda k: np.full(k, FILL)  # noqa: E731
    with np.errstate(invalid='ignore'):
        vals = ip.siamese_getitem(list(planes), list(planes), labels, (h, w), c, True, to_fit=False, fill=fill)[0]
        got = I.tile_ingest(planes, h, w, 10000.0, nan_mask=2, fill=FILL)
        assert same_bits(got[..., :c], vals)
        for morph in I.MORPHS[::3]:
            color = (1.03, 0.96)
            (xb, _), y = ip.siamese_getitem(list(planes), list(planes), labels, (h, w), c, True, True, color, color, morph, fill=fill)
            v, _ = I.tile_values(planes, h, w, 10000.0, 2, fill=FILL)
            mu = np.nanmean(np.moveaxis(v, 1, 3), axis=(1, 2))
            got = I.tile_ingest(planes, h, w, 10000.0, nan_mask=2, fill=FILL, ch_mean=mu, contra=color[0], bright=color[1], flip_v=morph[0],
                                flip_h=morph[1], rot=morph[2])
            assert same_bits(got[..., c:], y), morph                                   # labels of ones times the validity mask
            if kind != 'f32':
                assert same_bits(got[..., :c], xb), morph


def test_tile_ingest_and_labels_reproduce_the_recorded_reference_morphs_and_colour():
    z = np.load(os.path.join(GOLD, 'array_tools_reference.npz'))
    chw = np.ascontiguousarray(np.moveaxis(z['morph_in'], 3, 1))
    for v, h, r in I.MORPHS:
        assert same_bits(I.tile_ingest(chw, 8, 8, flip_v=v, flip_h=h, rot=r), z[f'morph_{v}{h}{r}']), (v, h, r)
    x = z['color_in']
    chw = np.ascontiguousarray(np.moveaxis(x, 3, 1))
    for i in (0, 1):
        got = I.tile_ingest(chw, x.shape[1], x.shape[2], ch_mean=np.nanmean(x, axis=(1, 2)), contra=z[f'color_mul_{i}'][0], bright=z[f'color_mul_{i}'][1])
        assert same_bits(got, z[f'color_out_{i}']), i


def test_morph_of_a_non_square_tile_is_the_reference_morph_of_the_unmorphed_output():
    planes = I.make_planes('i16', (3, 4, 8, 12), 3)
    base = I.tile_ingest(planes, 5, 7)
    for v, h, r in I.MORPHS:
        got = I.tile_ingest(planes, 5, 7, flip_v=v, flip_h=h, rot=r)
        assert got.shape == ((3, 7, 5, 4) if r % 2 else (3, 5, 7, 4))
        assert same_bits(got, np.ascontiguousarray(ip.aug_array_morph(base, v, h, r)))


# ----------------------------------------------------------------------------- label_onehot
LC_T, LU_T = [(12, 3), (11, 3), (10, 3), (9, 8), (255, 0), (3, 12)], [(82, 9), (84, 1), (0, 2)]


@pytest.mark.parametrize('kind', I.LABEL_KINDS)
def test_label_onehot_is_process_y(kind):
    for (h, w), even, odd in I.TILE_SHAPES:
        for hin, win in (even, odd):
            lc = I.label_planes(kind, (3, 1, hin, win), hin)
            for lu_kind in (None, 'f32', 'i16'):
                lu = I.landuse_planes(lu_kind, lc.shape, win) if lu_kind else None
                for ncls in (1, 2, 8):
                    for lc_t in (LC_T, None):
                        with np.errstate(invalid='ignore'):
                            ref = ip.process_y(list(lc), (h, w), ncls, lc_t, list(lu) if lu is not None else None, LU_T).reshape(3, h, w, ncls)
                        lut = ip.merge_lut(lc_t) if lc_t else None
                        for morph in I.MORPHS[1::5]:
                            got = I.label_onehot(lc, lut, lu, ip.merge_lut(LU_T) if lu is not None else None, h, w, ncls, morph)
                            assert same_bits(got, np.ascontiguousarray(ip.aug_array_morph(ref, *morph))), (hin, win, lu_kind, ncls, morph)


def test_label_rules_the_issue_names():
    lc = np.array([2.7, -0.5, np.nan, np.inf, -np.inf, 300.0, 1.0, 7.0], np.float32).reshape(1, 1, 2, 4)
    lu = np.array([82.5, 82.0, 82.0, 0.0, 0.0, 0.0, 338.0, 82.0], np.float32).reshape(1, 1, 2, 4)
    lut = np.full(256, -1)
    lut[2], lut[7] = 5, -1
    lu_lut = np.full(256, -1)
    lu_lut[82] = 3
    got = I.label_onehot(lc, lut, None, None, 2, 4, 8, (0, 0, 0)).reshape(8, 8)
    assert got.argmax(1).tolist() == [5, 0, 0, 0, 0, 0, 1, 7] and got.sum(1).tolist() == [1, 1, 0, 0, 0, 0, 1, 1]
    got = I.label_onehot(lc, lut, lu, lu_lut, 2, 4, 8, (0, 0, 0)).reshape(8, 8)
    assert got.argmax(1).tolist() == [5, 3, 3, 0, 0, 0, 1, 3] and got.sum(1).tolist() == [1, 1, 1, 0, 0, 0, 1, 1]


# ------------------------------------------------------------------------------- pack_image
def unpack(img, taps, kpad, npad, el):
    """M[tap, k, n] of the image P[tap, k // el, n, k % el], element by element (the layout as the header states it)"""
    m = np.zeros((taps, kpad, npad))
    p = np.asarray(img).reshape(taps, kpad // el, npad, el)
    for k in range(kpad):
        m[:, k, :] = p[:, k // el, :, k % el]
    return m


def gemm_conv(x, m, kh, kw):
    """'same' cross-correlation as one GEMM per tap: out[p, n] = sum_tap sum_k x[p + tap offset, k] M[tap, k, n]; x zero-padded to kpad"""
    n, h, w, c = x.shape
    taps, kpad, npad = m.shape
    xp = np.zeros((n, h + kh - 1, w + kw - 1, kpad))
    xp[:, kh // 2:kh // 2 + h, kw // 2:kw // 2 + w, :c] = x
    out = np.zeros((n, h, w, npad))
    for i in range(kh):
        for j in range(kw):
            out += xp[:, i:i + h, j:j + w] @ m[i * kw + j]
    return out


@pytest.mark.parametrize('shape', I.PACK_PLAIN + [(3, 3, 5, 7, 16), (5, 5, 9, 33, 16)], ids=str)
@pytest.mark.parametrize('el', [8, 16])
def test_conv_images_reproduce_conv2d_and_its_input_gradient(shape, el):
    kh, kw, cin, cout, cin_pad = shape
    rng = np.random.default_rng(cin * 100 + cout)
    k = rng.standard_normal((kh, kw, cin, cout))
    x, dy = rng.standard_normal((2, 6, 5, cin)), rng.standard_normal((2, 6, 5, cout))
    t, kpad, npad = I.pack_dims(0, kh * kw, cin, cout, cin_pad)
    assert (kpad, npad) == (cin_pad, I.rup(cout, 32))
    if kpad % el == 0:
        img = I.pack_image(k, 0, cin_pad, el, 'f64')
        y = gemm_conv(x, unpack(img, t, kpad, npad, el), kh, kw)
        ref = K.conv2d_same(x, k)
        assert np.abs(y[..., :cout] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) and not y[..., cout:].any()
    if el == 8:
        t, kpad, npad = I.pack_dims(1, kh * kw, cin, cout, cin_pad)
        assert (kpad, npad) == (I.rup(cout, 16), I.rup(cin, 32))
        dx = gemm_conv(dy, unpack(I.pack_image(k, 1, cin_pad, 8, 'f64'), t, kpad, npad, 8), kh, kw)
        xt = torch.tensor(x.transpose(0, 3, 1, 2), dtype=torch.float64, requires_grad=True)
        wt = torch.tensor(k.transpose(3, 2, 0, 1).copy(), dtype=torch.float64)
        torch.nn.functional.conv2d(xt, wt, padding=(kh // 2, kw // 2)).backward(torch.tensor(dy.transpose(0, 3, 1, 2).copy()))
        ref = xt.grad.numpy().transpose(0, 2, 3, 1)
        assert np.abs(dx[..., :cin] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) and not dx[..., cin:].any()


@pytest.mark.parametrize('shape', I.PACK_TRANSPOSED + [(3, 3, 5, 7, 16)], ids=str)
@pytest.mark.parametrize('el', [8, 16])
def test_transposed_images_reproduce_conv2d_transpose_and_its_input_gradient(shape, el):
    s, _, cout, cin, cin_pad = shape
    rng = np.random.default_rng(cin * 100 + cout)
    k = rng.standard_normal((s, s, cout, cin))
    n, h, w = 2, 4, 3
    x, dy = rng.standard_normal((n, h, w, cin)), rng.standard_normal((n, h * s, w * s, cout))
    t, kpad, npad = I.pack_dims(2, s * s, cin, cout, cin_pad)
    assert (t, kpad, npad) == (1, cin_pad, I.rup(s * s * cout, 32))
    m = unpack(I.pack_image(k, 2, cin_pad, el, 'f64'), 1, kpad, npad, el)[0]
    xp = np.zeros((n * h * w, kpad))
    xp[:, :cin] = x.reshape(-1, cin)
    cols = xp @ m                                                                      # N index = (i s + j) cout + o: depth to space
    y = cols[:, :s * s * cout].reshape(n, h, w, s, s, cout).transpose(0, 1, 3, 2, 4, 5).reshape(n, h * s, w * s, cout)
    ref = K.conv2d_transpose_ks(x, k)
    assert np.abs(y - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) and not cols[:, s * s * cout:].any()
    if el == 8:
        t, kpad, npad = I.pack_dims(3, s * s, cin, cout, cin_pad)
        assert (t, kpad, npad) == (1, I.rup(s * s * cout, 16), I.rup(cin, 32))
        m = unpack(I.pack_image(k, 3, cin_pad, 8, 'f64'), 1, kpad, npad, 8)[0]
        d = np.zeros((n * h * w, kpad))                                                # K index = (i s + j) cout + o: space to depth
        d[:, :s * s * cout] = dy.reshape(n, h, s, w, s, cout).transpose(0, 1, 3, 2, 4, 5).reshape(-1, s * s * cout)
        dx = d @ m
        ref = K.conv2d_transpose_ks_bwd(x, k, dy)[0].reshape(-1, cin)
        assert np.abs(dx[:, :cin] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) and not dx[:, cin:].any()


def test_pack_image_padding_is_plus_zero_and_storage_rounding_comes_last():
    k = I.pack_kernel_values((3, 3, 13, 24), 1)
    for kind in ('f32', 'bf16', 'fp8'):
        for mode in (0, 1):
            img, own = I.pack_image(k, mode, 16, 8, kind), I.pack_owned(k, mode, 16)
            assert own.sum() == k.size and img.size == int(np.prod(I.pack_dims(mode, 9, 13, 24, 16)))
            assert not I.storage_bits(img, kind)[~own].any()
            assert np.array_equal(np.sort(img[own]), np.sort(I.O.to_storage(k.reshape(-1), kind)))
    codes = I.storage_bits(I.pack_image(k, 0, 16, 8, 'fp8'), 'fp8')
    assert (codes & 0x7f).max() == 0x7e and 0 < (codes & 0x7f)[(codes & 0x78) == 0].max() < 8     # saturated to 448; subnormal codes present


def test_batched_table_has_the_item_counts_the_issue_asks_for():
    for big in (512, 256):
        real = [I.job_real_items(j) for j in I.batched_jobs(big)]
        assert any(r % 256 == 0 for r in real) and any(r % 256 == 64 for r in real)
        assert real[0] < 256 and real[-1] < 4096 and max(real) == real[-4] == 9 * (big // 8) * big
    two = I.job_real_items((3, 3, 512, 512, 512, 0)) + I.job_real_items((3, 3, 512, 512, 512, 1))
    assert two == 589824 > O_CAP                                                        # a workgroup's later trips fall into other jobs
    assert 2 * I.job_real_items((3, 3, 256, 256, 256, 0)) > I.O.grid_cap_threads(1)     # and so they do in the small-grid child
    modes1 = [(j, I.pack_dims(1, 9, j[2], j[3], j[4])[1]) for j in I.batched_jobs() if j[5] == 1]
    assert {kp % 32 == 0 for _, kp in modes1} == {True, False}                         # the remapped path and the plain one


O_CAP = I.O.grid_cap_threads()


# --------------------------------------------------------------------- conditions of the inputs
@pytest.mark.parametrize('case', I.threshold_cases(), ids=str)
def test_threshold_planes_hold_the_threshold_and_its_neighbours(case):
    kind, rescale, mode = case
    p, (t, below, above) = I.threshold_planes(kind, rescale, mode)
    thr = -5000.0 if mode == 1 else -1.0
    assert float(t) == thr * (rescale or 1.0) and below < t < above
    if kind in ('f32', 'f64'):
        assert np.nextafter(t, type(t)(-np.inf)) == below and np.nextafter(t, type(t)(np.inf)) == above
    else:
        assert (int(below), int(above)) == (int(t) - 1, int(t) + 1)
    for ch in range(3):
        assert {t, below, above} <= set(p[0, ch, ch].tolist())
    v, flagged = I.tile_values(p, 4, 6, rescale, mode, replace=0)
    at = v[0, 0, 0, 0]
    assert at == thr                                                                    # exactly the threshold after the rescale: not flagged
    out = I.tile_ingest(p, 4, 6, rescale, nan_mask=mode, replace=1, fill=FILL)
    mask = out[0, ..., 3]
    if mode == 1:
        assert mask[0, 0] == 0 and mask[0, 3] == 1 and mask[0, 4] == 0                  # the threshold itself, twice it, half of it
        if not rescale:
            assert mask[0, 1] == 1 and mask[0, 2] == 0                                  # predecessor flagged, successor not
        assert out[0, 0, 3, 0] == FILL and out[0, 0, 3, 2] == FILL and out[0, 1, 3, 0] != FILL      # replaced from the flagging channel on
    else:
        assert mask[0, 0] == 1 and mask[0, 3] == 0 and mask[0, 4] == 1
        if not rescale:
            assert mask[0, 1] == 0 and mask[0, 2] == 1


@pytest.mark.parametrize('kind', I.EXACT_MEAN_KINDS)
def test_exact_mean_cases_have_an_exact_double_sum(kind):
    for h, w in I.MEAN_WINDOWS:
        p = I.exact_mean_planes(kind, (2, 2, h + 3, w + 2), h)
        for rescale in I.EXACT_MEAN_RESCALES:
            v, _ = I.tile_values(p, h, w, rescale)
            assert np.array_equal(v * rescale if rescale else v, I._trim(p, h, w).astype(np.float64))       # the division was exact
            q = v * 4.0                                                                                       # quarter units
            assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2.0 ** 34 and h * w < 2 ** 17           # any partial sum < 2^51 units
            mean, cnt, sabs = I.tile_channel_mean(p, h, w, rescale)
            assert np.array_equal(mean, v.reshape(2, 2, -1).sum(-1) / (h * w)) and (cnt == h * w).all()


def test_tile_channel_mean_skips_nans_and_includes_the_mode_2_draws():
    p = I.make_planes('f64', (2, 3, 9, 9), 5, nan_frac=0.2)
    p[1, 2] = np.nan
    mean, cnt, sabs = I.tile_channel_mean(p, 5, 7, 100.0)
    w = I._trim(p, 5, 7) / 100.0
    ref = np.nanmean(w[:, :2], axis=(2, 3))
    assert np.isnan(mean[1, 2]) and cnt[1, 2] == 0 and np.allclose(mean[:, :2], ref, rtol=1e-14)
    m2, c2, _ = I.tile_channel_mean(p, 5, 7, 100.0, nan_mask=2, seed=9)
    assert (c2 == 35).all() and 0 <= m2[1, 2] < 1
    full = I.tile_ingest(p, 5, 7, 100.0, nan_mask=2, seed=9)                          # exactly the draws the ingest writes
    assert np.allclose(m2, full[..., :3].astype(np.float64).mean(axis=(1, 2)), rtol=1e-6)
    assert (np.abs(mean[:, :2] - ref) <= 2 * I.mean_bound(cnt, sabs)[:, :2]).all()      # NumPy's pairwise sum obeys the same bound, as does fsum


def test_draws_few_sit_on_a_float32_rounding_boundary():
    """the ambiguity rule of the GPU file (a replaced value may differ from the oracle's float32 where the double draw lies within the double
    functions' last places of a float32 rounding boundary) is needed by far fewer than its cap of 1e-3 of the draws"""
    idx = np.arange(1 << 18, dtype=np.uint64)
    for seed in (0, 11, 2 ** 63 + 5):
        z = I.draw_normal(seed, idx)
        u = I.draw_uniform(seed, idx)
        assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 5 / np.sqrt(12 * idx.size) and len(np.unique(u)) == idx.size
        assert np.isfinite(z).all() and abs(z.mean()) < 5 / np.sqrt(idx.size) and abs(z.std() - 1) < 0.01 and np.abs(z).max() < 6.7
        f = z.astype(np.float32).astype(np.float64)
        half = 0.5 * np.spacing(np.abs(z).astype(np.float32)).astype(np.float64)
        near = np.abs(np.abs(z - f) - half) <= 2.0 ** -46 * np.abs(z)                   # 64 double units from the midpoint of two floats
        assert near.mean() < 1e-4
    assert np.array_equal(I.draw_uniform(3, idx[:5]), I.draw_uniform(3, idx[:5])) and not np.array_equal(I.draw_uniform(3, idx[:5]), I.draw_uniform(4, idx[:5]))
    # one value by hand: splitmix64(0 ^ 0) of the published generator
    assert int(I.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_ingest_chw_sources_cover_the_upper_half_of_uint16():
    p, scale = I.chw_planes('u16', (3, 4, 5, 7), 0)
    assert (p >= 32768).any() and (p < 32768).any() and p.max() == 65535
    ref = I.ingest_chw(p, scale, 16, 'f32')
    assert ref.shape == (3, 5, 7, 16) and not ref[..., 4:].any() and ref.min() >= 0                # unsigned: nothing negative
    assert np.array_equal(ref[0, 0, 0, :4], (p[0, :, 0, 0].astype(np.float32) * np.float32(scale)).astype(np.float64))
    b = I.ingest_chw(p, scale, 16, 'bf16')
    assert np.array_equal(b, I.O.bf16_round(ref.astype(np.float32)).astype(np.float64))


# ------------------------------------------------------------------------- processing.merge_lut
def test_merge_lut_refuses_rules_the_table_cannot_apply():
    from satellite_computervision_amd import processing as P
    for trans in ([(256, 1)], [(-1, 0)], [(82.5, 9)], [(3, 1), (1000, 2)], [(float('nan'), 1)], [(float('inf'), 1)]):
        with pytest.raises(ValueError, match='merge_lut'):
            P.merge_lut(trans, 'cpu')
    lc_t, lu_t = [(12, 3), (11, 3), (10, 3), (9, 8), (255, 0)], [(82, 9), (84, 10)]         # the generators' defaults
    for trans in (lc_t, lu_t, None, [], [(3, 1), (3, 2)]):
        lut = P.merge_lut(trans, 'cpu').numpy()
        assert lut.dtype == np.int32 and np.array_equal(lut, ip.merge_lut(trans or []))
    assert P.merge_lut([(82.0, 9)], 'cpu')[82] == 9 and P.merge_lut([(3, 1), (3, 2)], 'cpu')[3] == 2                                    # the last rule wins
