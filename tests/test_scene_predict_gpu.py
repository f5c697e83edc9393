"""Device-resident scene prediction on the GPU: the gather and scatter kernels (satcv_scene_gather / satcv_scene_scatter) against NumPy,
bit for bit; predict_chips_device against predict_chips on the same model, indices and batch size; predict_scene's two covers;
callback_predictions; no host synchronisation inside the batch loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

FILTERS, FACTORS = [32, 64], [2, 2]
KIND = {np.uint8: 0, np.uint16: 1, np.float32: 2, np.int16: 3}


@pytest.fixture(scope='module')
def env():
    from satellite_computervision_amd import ops, model_tools as mt, prediction_tools as pt, _lib
    assert torch.cuda.is_available()
    return dict(ops=ops, mt=mt, pt=pt, L=_lib)


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _scene(rng, dtype, H, W, c):
    if dtype == np.float32:
        return rng.standard_normal((H, W, c)).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, (H, W, c), endpoint=True).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------- 1. gather
@pytest.mark.parametrize('dtype,c,ldc,coff,rescale', [
    (np.uint8, 3, 3, 0, 255.0), (np.uint8, 4, 4, 0, 0.0), (np.uint16, 4, 4, 0, 10000.0), (np.uint16, 4, 6, 1, 10000.0), (np.uint16, 13, 16, 2, 10000.0),
    (np.int16, 4, 4, 0, 100.0), (np.int16, 13, 13, 0, 0.0), (np.int16, 3, 5, 2, 2000.0), (np.float32, 4, 4, 0, 0.0), (np.float32, 4, 4, 0, 3.0),
    (np.float32, 3, 8, 5, 0.0), (np.float32, 13, 14, 1, 7.0)])
def test_gather_equals_windows_of_the_reflect_padded_scene(env, dtype, c, ldc, coff, rescale):
    L, ops = env['L'], env['ops']
    rng = np.random.default_rng(c * 100 + ldc)
    H, W, kernel, buff = 77, 91, 32, 16
    off, side = buff // 2, kernel + buff
    scene = _scene(rng, dtype, H, W, c)
    # inside, flush with each edge, overhanging the top / left / bottom / right edge, and the four corners
    origins = [(8, 8), (20, 33), (H - kernel - off, W - kernel - off), (0, 30), (30, 0), (H - kernel + 5, 30), (30, W - kernel + 3),
               (0, 0), (0, W - kernel + 7), (H - 9, 0), (H - 9, W - 11), (3, 5)]
    pad = side
    padded = np.pad(scene, ((pad, pad), (pad, pad), (0, 0)), mode='reflect')
    vals = (padded.astype(np.float64) / rescale).astype(np.float32) if rescale else padded.astype(np.float32)
    want_all = np.stack([vals[pad + y - off:pad + y - off + side, pad + x - off:pad + x - off + side] for y, x in origins])
    src, org = _dev(scene), _dev(np.asarray(origins, np.int32))
    first, n = 1, len(origins) - 2                           # a launch takes chips [first, first + n) of the table
    dst = torch.full((n, side, side, ldc), -777.0, dtype=torch.float32, device='cuda')
    d = L.SceneGatherDesc(src=src.data_ptr(), src_kind=KIND[dtype], h=H, w_=W, c=c, rescale=rescale, origins=org.data_ptr(), total=len(origins),
                          first=first, n=n, off=off, side=side, dst=dst.data_ptr(), ldc=ldc, coff=coff)
    L.check(L.lib.satcv_scene_gather(C.byref(d), ops.stream_ptr()))
    got = dst.cpu().numpy()
    assert np.array_equal(got[..., coff:coff + c].view(np.uint32), want_all[first:first + n].view(np.uint32))          # bit for bit
    rest = np.delete(got, np.s_[coff:coff + c], axis=-1)
    assert np.all(rest == -777.0)                            # channels outside [coff, coff + c) keep the sentinel


def test_gather_never_reads_outside_the_scene_for_any_origin(env):
    """origins far outside the scene are clamped to edge samples: every gathered value is a value of the scene"""
    L, ops = env['L'], env['ops']
    H, W, side = 40, 50, 24
    scene = (np.arange(H * W * 4, dtype=np.float32) + 1).reshape(H, W, 4)
    origins = np.asarray([(-10 ** 9, 5), (5, 2 ** 31 - 1), (-2 ** 31, -2 ** 31), (10 ** 6, -77), (3 * H, 3 * W)], np.int32)
    src, org = _dev(scene), _dev(origins)
    dst = torch.zeros((len(origins), side, side, 4), dtype=torch.float32, device='cuda')
    d = L.SceneGatherDesc(src=src.data_ptr(), src_kind=2, h=H, w_=W, c=4, rescale=0.0, origins=org.data_ptr(), total=len(origins), first=0,
                          n=len(origins), off=4, side=side, dst=dst.data_ptr(), ldc=4, coff=0)
    L.check(L.lib.satcv_scene_gather(C.byref(d), ops.stream_ptr()))
    got = dst.cpu().numpy()
    assert got.min() >= 1 and got.max() <= H * W * 4
    assert np.array_equal(got[2], np.broadcast_to(scene[H - 1, W - 1], (side, side, 4)))     # -i beyond the scene clamps to the last sample
    assert np.array_equal(got[4], np.broadcast_to(scene[0, 0], (side, side, 4)))             # 2 (n - 1) - i below zero clamps to the first


# ---------------------------------------------------------------------------------------------------------------- 2. scatter
def _scatter(env, src, dst, origins, crop, c0, nc, doff, accumulate, first=0, n=None):
    L, ops = env['L'], env['ops']
    n = src.shape[0] if n is None else n
    d = L.SceneScatterDesc(src=src.data_ptr(), src_kind=2 if src.dtype == torch.float32 else 5, n=n, sh=src.shape[1], sw=src.shape[2], lds=src.shape[3],
                           c0=c0, nc=nc, crop_y=crop[0], crop_x=crop[1], crop_h=crop[2], crop_w=crop[3], origins=origins.data_ptr(),
                           total=origins.shape[0], first=first, dst=dst.data_ptr(), dst_kind=2 if dst.dtype == torch.float32 else 0,
                           h=dst.shape[0], w_=dst.shape[1], ldd=dst.shape[2], doff=doff, accumulate=accumulate)
    L.check(L.lib.satcv_scene_scatter(C.byref(d), ops.stream_ptr()))


def _scatter_numpy(src, dst, origins, crop, c0, nc, doff, accumulate):
    H, W = dst.shape[:2]
    for k, (y, x) in enumerate(origins):
        h, w = max(min(crop[2], H - y), 0), max(min(crop[3], W - x), 0)
        part = src[k, crop[0]:crop[0] + h, crop[1]:crop[1] + w, c0:c0 + nc].astype(dst.dtype)
        if accumulate:
            dst[y:y + h, x:x + w, doff:doff + nc] += part
        else:
            dst[y:y + h, x:x + w, doff:doff + nc] = part


@pytest.mark.parametrize('lds,c0,nc,ldd,doff,accumulate,crop', [
    (2, 0, 1, 1, 0, 1, (8, 8, 32, 32)), (2, 1, 1, 1, 0, 0, (8, 8, 32, 32)), (2, 0, 2, 2, 0, 1, (8, 8, 32, 32)), (1, 0, 1, 3, 2, 1, (8, 8, 32, 32)),
    (4, 1, 2, 5, 2, 1, (8, 8, 32, 32)), (4, 3, 1, 1, 0, 0, (8, 4, 36, 28)), (7, 2, 3, 4, 1, 1, (8, 8, 32, 32)), (3, 0, 3, 3, 0, 0, (4, 8, 28, 36))])
def test_scatter_f32_equals_numpy_slicing(env, lds, c0, nc, ldd, doff, accumulate, crop):
    rng = np.random.default_rng(lds * 10 + nc)
    H, W, G = 70, 85, 9                                      # G: guard rows above and below the map in the same allocation
    # disjoint centres: inside, clipped at the bottom, at the right, at the corner
    origins = [(0, 0), (3, 40), (H - 20, 2), (0, W - 8), (H - 5, W - 6)]
    src = rng.standard_normal((len(origins), 48, 48, lds)).astype(np.float32)
    full = rng.standard_normal((H + 2 * G, W, ldd)).astype(np.float32)
    want = full.copy()
    _scatter_numpy(src, want[G:G + H], origins, crop, c0, nc, doff, accumulate)
    buf = _dev(full)
    _scatter(env, _dev(src), buf[G:G + H], _dev(np.asarray(origins, np.int32)), crop, c0, nc, doff, accumulate)
    got = buf.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))            # the map, the untouched pixels / channels and the guard band
    assert np.array_equal(got[:G], full[:G]) and np.array_equal(got[G + H:], full[G + H:])


def test_scatter_classes_i32_to_u8_and_to_f32(env):
    rng = np.random.default_rng(3)
    H, W, G = 61, 67, 5
    origins = [(1, 2), (33, 3), (H - 7, 40), (2, W - 9)]
    src = rng.integers(0, 200, (len(origins) + 2, 48, 48, 1)).astype(np.int32)
    org = _dev(np.asarray([(0, 0)] + origins + [(0, 0)], np.int32))
    for dtype in (np.uint8, np.float32):
        full = np.full((H + 2 * G, W, 1), 255, dtype)
        want = full.copy()
        _scatter_numpy(src[1:-1], want[G:G + H], origins, (8, 8, 32, 32), 0, 1, 0, 0)
        buf = _dev(full)
        _scatter(env, _dev(src[1:-1]), buf[G:G + H], org, (8, 8, 32, 32), 0, 1, 0, 0, first=1, n=len(origins))      # a window of the table
        assert np.array_equal(buf.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- models
def _unet(mt, dtype, seed=5):
    """a [32, 64] two-class U-Net with non-trivial weights and BatchNorm statistics"""
    mt.reset_uids(); mt.set_seed(seed)
    m = mt.get_unet_model(2, 4, FILTERS, FACTORS)
    m.compute_dtype = dtype
    _randomise(m, seed)
    return m


def _randomise(m, seed):
    rng = np.random.default_rng(seed + 13)
    w = {}
    for ps in m.param_specs:
        if ps.kind == 'kernel':
            w[ps.name] = (rng.standard_normal(ps.shape) * np.sqrt(2.0 / np.prod(ps.shape[:3]))).astype(np.float32)
        elif ps.kind == 'moving_var':
            w[ps.name] = (0.5 + rng.random(ps.shape)).astype(np.float32)
        elif ps.kind == 'gamma':
            w[ps.name] = (1 + 0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
        else:
            w[ps.name] = (0.2 * rng.standard_normal(ps.shape)).astype(np.float32)
    m.set_weights_dict(w)


def _model(mt, which, rng):
    if which == 'fp32':
        return _unet(mt, 'float32')
    if which == 'bf16':                                      # the folded bf16 plan is the default of a bf16 U-Net
        return _unet(mt, 'bfloat16')
    if which == 'fp8':
        return _unet(mt, 'bfloat16').enable_fp8_inference(rng.random((4, 48, 48, 4)).astype(np.float32))
    mt.reset_uids(); mt.set_seed(4)
    m = mt.make_siamese_unet(4, FILTERS, FACTORS, class_thresh=0.4)
    m.compute_dtype = 'bfloat16'
    _randomise(m, 4)
    return m.enable_folded_inference()


# ---------------------------------------------------------------------------------------------------------------- 3. == predict_chips
@pytest.mark.parametrize('which', ['fp32', 'bf16', 'fp8', 'siamese'])
def test_predict_chips_device_equals_predict_chips(env, which):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(11)
    m = _model(mt, which, rng)
    H, W, kernel, buff = 200, 232, 32, 16
    a = rng.random((H, W, 4)).astype(np.float32)
    arr = (a, rng.random((H, W, 4)).astype(np.float32)) if which == 'siamese' else a
    idx = pt.generate_chip_indices(a, buff, kernel)
    assert len(idx) % 4 != 0 and len(idx) > 8                # the last batch is short
    start = rng.standard_normal((H, W))                      # non-zero incoming float64 template
    for channel in ((0,) if which == 'siamese' else (0, 1)):      # (the change model has one sigmoid channel)
        want = pt.predict_chips(arr, idx, start.copy(), m, kernel=kernel, buff=buff, batch_size=4, channel=channel)
        got = pt.predict_chips_device(arr, idx, start.copy(), m, kernel=kernel, buff=buff, batch_size=4, channel=channel)
        assert got.dtype == np.float64 and not np.array_equal(want, start)
        assert np.array_equal(got, want), (which, channel, np.abs(got - want).max())


# ---------------------------------------------------------------------------------------------------------------- 4. integer scene
def test_uint16_scene_with_rescale(env):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(12)
    m = _unet(mt, 'bfloat16')
    scene = rng.integers(0, 12000, (150, 170, 4)).astype(np.uint16)
    idx = pt.generate_chip_indices(scene, 16, 32)
    want = pt.predict_chips((scene.astype(np.float64) / 10000).astype(np.float32), idx, np.zeros(scene.shape[:2]), m, kernel=32, buff=16, batch_size=5)
    got = pt.predict_chips_device(scene, idx, np.zeros(scene.shape[:2]), m, kernel=32, buff=16, batch_size=5, rescale=10000)
    assert want.max() > 0 and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 5. covers
def test_predict_scene_full_and_reference_cover(env):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(13)
    m = _unet(mt, 'bfloat16')
    H, W, kernel, buff = 131, 97, 32, 16
    off, side = buff // 2, kernel + buff
    scene = rng.random((H, W, 4)).astype(np.float32)
    probs, cls = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=4, channel=None, cover='full', classes=True)
    assert probs.shape == (H, W, 2) and probs.dtype == np.float32 and cls.shape == (H, W) and cls.dtype == np.uint8
    # predict_chips-style stitching on the reflect-padded scene, cropped back; same batches (same plans) as the device path
    padded = np.pad(scene, ((off, kernel + off), (off, kernel + off), (0, 0)), mode='reflect')
    grid = [(y, x) for y in range(0, H, kernel) for x in range(0, W, kernel)]
    wp = np.zeros((H + kernel, W + kernel, 2), np.float32)
    wc = np.full((H + kernel, W + kernel), 255, np.uint8)
    for s in range(0, len(grid), 4):
        part = grid[s:s + 4]
        p, c = m.predict(np.stack([padded[y:y + side, x:x + side] for y, x in part]), batch_size=len(part))
        for k, (y, x) in enumerate(part):
            wp[y:y + kernel, x:x + kernel] = p[k, off:off + kernel, off:off + kernel]
            wc[y:y + kernel, x:x + kernel] = c[k, off:off + kernel, off:off + kernel]
    assert np.array_equal(probs, wp[:H, :W]) and np.array_equal(cls, wc[:H, :W])
    assert not np.any(cls == 255) and set(np.unique(cls)) <= {0, 1}
    one = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=4, channel=1, cover='full')
    assert one.shape == (H, W) and np.array_equal(one, probs[..., 1])
    # cover='reference' is predict_chips, border left unpredicted
    idx = pt.generate_chip_indices(scene, buff, kernel)
    ref, rcls = pt.predict_scene(scene, m, kernel=kernel, buff=buff, batch_size=4, channel=0, cover='reference', classes=True)
    want = pt.predict_chips(scene, idx, np.zeros((H, W), np.float32), m, kernel=kernel, buff=buff, batch_size=4)
    assert np.array_equal(ref, want) and ref.dtype == np.float32
    seen = np.zeros((H, W), bool)
    for y, x in idx:
        seen[y:y + kernel, x:x + kernel] = True
    assert not seen[:off].any() and np.all(ref[~seen] == 0) and np.all(rcls[~seen] == 255) and np.all(rcls[seen] < 2)
    with pytest.raises(ValueError, match='leaves the'):
        pt.predict_chips_device(scene, [(0, 0)], np.zeros((H, W)), m, kernel=kernel, buff=buff)


# ---------------------------------------------------------------------------------------------------------------- 6. overlaps
def test_overlapping_centres_are_summed_deterministically(env):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(14)
    m = _unet(mt, 'bfloat16')
    scene = rng.random((120, 120, 4)).astype(np.float32)
    idx = [(8, 8), (24, 20), (60, 60), (8, 8 + 32)]          # the second centre overlaps the first and the fourth
    want = pt.predict_chips(scene, idx, np.zeros((120, 120)), m, kernel=32, buff=16, batch_size=4)
    got = pt.predict_chips_device(scene, idx, np.zeros((120, 120)), m, kernel=32, buff=16, batch_size=4)
    again = pt.predict_chips_device(scene, idx, np.zeros((120, 120)), m, kernel=32, buff=16, batch_size=4)
    assert np.array_equal(got, again)
    # host: float64 sum of two float32 terms (exact to 2^-53); device: the same sum rounded once to float32 -> one float32 ulp
    np.testing.assert_allclose(got, want, rtol=2.0 ** -23, atol=0)
    single = np.ones((120, 120), bool)
    single[24:56, 20:52] = False
    assert np.array_equal(got[single], want[single]) and want[30, 30] > 0          # one contribution: equal bits


# ---------------------------------------------------------------------------------------------------------------- 7. callback_predictions
def test_callback_predictions_mosaic(env):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(15)
    m = _unet(mt, 'bfloat16')
    patches = rng.random((7, 48, 48, 4)).astype(np.float32)  # 2 rows of 3; the seventh patch is a trailing partial row
    kshape, kbuf = [32, 32], [16, 8]                          # non-square buffer: 36 x 28 crops
    got = pt.callback_predictions(patches, m, {'totalPatches': 7, 'patchesPerRow': 3}, kshape, kbuf)
    p = m.predict(patches, batch_size=16)[0]
    xb, yb = kbuf[0] // 2, kbuf[1] // 2
    crops = [q[yb:kshape[1] + xb, xb:kshape[0] + yb, 1] for q in p]
    want = np.concatenate([np.concatenate(crops[r * 3:r * 3 + 3], axis=1) for r in range(2)], axis=0)
    assert got.shape == (72, 84) and got.dtype == np.float32 and np.array_equal(got, want)
    it = pt.callback_predictions(iter([patches[:4], patches[4:]]), m, {'totalPatches': 7, 'patchesPerRow': 3}, kshape, kbuf)
    p2 = np.concatenate([m.predict(patches[:4], batch_size=4)[0], m.predict(patches[4:], batch_size=3)[0]])      # the plans of batches of 4 and 3
    crops = [q[yb:kshape[1] + xb, xb:kshape[0] + yb, 1] for q in p2]
    assert np.array_equal(it, np.concatenate([np.concatenate(crops[r * 3:r * 3 + 3], axis=1) for r in range(2)], axis=0))


# ---------------------------------------------------------------------------------------------------------------- 8. no sync in the loop
def test_no_host_synchronisation_inside_the_batch_loop(env, monkeypatch):
    mt, pt = env['mt'], env['pt']
    rng = np.random.default_rng(16)
    m = _unet(mt, 'bfloat16')
    scene = rng.random((152, 152, 4)).astype(np.float32)
    idx = pt.generate_chip_indices(scene, 16, 32)
    assert len(idx) == 9                                      # three batches of 4, 4, 1
    warm = pt.predict_chips_device(scene, idx, np.zeros(scene.shape[:2]), m, kernel=32, buff=16, batch_size=4)      # plan construction may synchronise
    count = {'n': 0}
    real_sync, real_stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

    def counted_sync(*a, **k):
        count['n'] += 1
        return real_sync(*a, **k)

    def counted_stream_sync(self):
        count['n'] += 1
        return real_stream_sync(self)
    monkeypatch.setattr(torch.cuda, 'synchronize', counted_sync)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', counted_stream_sync)
    got = pt.predict_chips_device(scene, idx, np.zeros(scene.shape[:2]), m, kernel=32, buff=16, batch_size=4)
    assert count['n'] <= 1, count
    assert np.array_equal(got, warm)
    pt.predict_chips(scene, idx, np.zeros(scene.shape[:2]), m, kernel=32, buff=16, batch_size=4)
    assert count['n'] >= 3                                    # (the counter does see the host path's per-batch synchronisation)
