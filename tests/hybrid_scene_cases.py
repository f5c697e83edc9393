"""Seeded scenes, models and the HOST LOOP that defines prediction_tools.predict_hybrid_scene (helper module, no tests in it; shared by
tests/test_hybrid_scene_cpu.py and tests/test_hybrid_scene_gpu.py).

The host loop, for a fine (H, W, C) scene and a coarse (T, c, h, w) stack with H = r h, W = r w:
  * fine chips: windows of the scene (np.pad mode='reflect' for cover='full') as (float64(v) / rescale).astype(float32);
  * coarse chips: windows of the stack (reflect-padded on its own grid) as float32(float64(v) / maxval), NaN -> 0, moved to
    (n, T, side_lo, side_lo, c);
  * `m.predict([hi, lo])` per batch of the same batch_size, in the same order;
  * pred[:, off:off + kernel, off:off + kernel, channel] placed at the origins with NumPy, clipped to the scene.

Shapes are the smallest that take every path.  Hybrid: r = 6, kernel 24, buff 24 (off 12, side 48 = 6 * 8, a multiple of the pooling
product 3 * 2; side_lo 8, off_lo 2); the reference cover of the 96 x 120 scene has 2 x 3 chips -- batches of 4 + 2, a short last batch --
the full cover of the 108 x 132 scene 5 x 6 chips with both far edges reflected and the last row and column clipped.  Hierarchical:
r = 2, kernel 8, buff 8 (off 4, side 16, side_lo 8, off_lo 2), a 32 x 40 scene: 2 x 3 chips."""
import numpy as np

MAXVAL, RESCALE = 10000, 10000

HYBRID = dict(r=6, kernel=24, buff=24, off=12, side=48, side_lo=8, off_lo=2, batch=4, T=3, TS=4, C=4, c=6, ncls=3,
              reference=dict(hi=(96, 120), lo=(16, 20), chips=(2, 3)), full=dict(hi=(108, 132), lo=(18, 22), chips=(5, 6)))
HIER = dict(r=2, kernel=8, buff=8, off=4, side=16, side_lo=8, off_lo=2, batch=4, T=3, TS=3, C=4, c=6,
            reference=dict(hi=(32, 40), lo=(16, 20), chips=(2, 3)))


def hybrid_model(lt, mt, dtype, seed=21):
    mt.set_seed(seed)
    m = lt.get_hybrid_model((48, 48, 4), (3, 8, 8, 6), 3, filters=[32, 64], factors=[3, 2])
    m.compute_dtype = dtype
    return randomise(m, seed)


def hierarchical_model(lt, mt, dtype, seed=22):
    mt.set_seed(seed)
    m = lt.get_hierarchical_model(3, 4, 2, (16, 16, 4), (3, 8, 8, 6), 16, 3)
    m.compute_dtype = dtype
    return randomise(m, seed)


def randomise(m, seed, scale=1.0):
    """non-trivial BatchNorm statistics and biases of the tape's parameters and wide softmax heads; the other kernels keep their initialisers"""
    rng = np.random.default_rng(seed)
    w = {}
    for k, v in m.get_weights_dict().items():
        if k.endswith('/moving_var'):
            w[k] = (0.5 + rng.random(v.shape)).astype(np.float32)
        elif k.endswith('/gamma'):
            w[k] = (1 + 0.2 * scale * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith(('/beta', '/moving_mean')):
            w[k] = (0.2 * scale * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith('/bias'):
            w[k] = (v + 0.1 * scale * rng.standard_normal(v.shape)).astype(np.float32)
        elif k in ('probabilities/kernel', 'lstm_probs/kernel', 'acnn_probs/kernel', 'sub_probs/kernel'):
            w[k] = (3.0 * rng.standard_normal(v.shape)).astype(np.float32)      # heads that separate the classes: a class map with every class
    m.set_weights_dict(w)
    return m


def hybrid_scene(cover, seed=40):
    """uint16 scene (rescale 10000) and int16 stack with negatives, one more acquisition than the model reads"""
    g = HYBRID[cover]
    rng = np.random.default_rng(seed)
    scene = rng.integers(0, 12000, g['hi'] + (HYBRID['C'],)).astype(np.uint16)
    stack = rng.integers(-300, 12000, (HYBRID['TS'], HYBRID['c']) + g['lo']).astype(np.int16)
    assert (stack[:HYBRID['T']] < 0).any()
    return scene, stack


def hier_scene(seed=41):
    """float32 scene and float32 stack with a few NaNs"""
    g = HIER['reference']
    rng = np.random.default_rng(seed)
    scene = rng.random(g['hi'] + (HIER['C'],)).astype(np.float32)
    stack = (rng.standard_normal((HIER['TS'], HIER['c']) + g['lo']) * 3000 + 3000).astype(np.float32)
    stack[rng.random(stack.shape) < 0.02] = np.nan
    assert np.isnan(stack).any()
    return scene, stack


def origins(hi_shape, kernel, buff, cover):
    """brute-force restatement of the two covers: [(y, x)] centre origins on the fine grid"""
    H, W = hi_shape
    off = buff // 2
    if cover == 'reference':                 # the reference's exclusive stop H - (buff + kernel): a chip ending on the image edge is skipped
        ys = [y for y in range(H) if (y - off) % kernel == 0 and y >= off and y < H - (buff + kernel)]
        xs = [x for x in range(W) if (x - off) % kernel == 0 and x >= off and x < W - (buff + kernel)]
    else:
        ys = [y for y in range(H) if y % kernel == 0]
        xs = [x for x in range(W) if x % kernel == 0]
    return [(y, x) for y in ys for x in xs]


def cut_chips(scene, stack, part, geo, T, rescale, maxval):
    """the two host batches of the chips `part` [(y, x)]: (n, side, side, C) float32 and (n, T, side_lo, side_lo, c) float32"""
    r, off, side, off_lo, side_lo = geo['r'], geo['off'], geo['side'], geo['off_lo'], geo['side_lo']
    # np.pad(mode='reflect') on each grid.  The last row / column of a full cover starts less than `kernel` before the far edge, so its
    # window overhangs by up to kernel - 1 + off: the pad is a whole window (side, side_lo), of which a chip reads what it needs; within
    # the first off (off_lo) samples it is the pad by off (off_lo)
    ps = np.pad(scene, ((side, side), (side, side), (0, 0)), mode='reflect')
    pl = np.pad(stack[:T], ((0, 0), (0, 0), (side_lo, side_lo), (side_lo, side_lo)), mode='reflect')
    hi = np.stack([ps[side + y - off:2 * side + y - off, side + x - off:2 * side + x - off] for y, x in part])
    hi = (hi.astype(np.float64) / rescale).astype(np.float32) if rescale else hi.astype(np.float32)
    lo = np.stack([pl[:, :, side_lo + y // r - off_lo:2 * side_lo + y // r - off_lo, side_lo + x // r - off_lo:2 * side_lo + x // r - off_lo]
                   for y, x in part])                                                                           # (n, T, c, side_lo, side_lo)
    lo = (np.moveaxis(lo, 2, 4).astype(np.float64) / maxval).astype(np.float32)
    return hi, np.where(np.isnan(lo), np.float32(0), lo)


def host_loop(scene, stack, predict, geo, kernel, buff, cover, batch_size, T, rescale=None, maxval=MAXVAL):
    """the definition of the feature -> (H, W, n_classes) float32 map of `predict(hi, lo) -> (n, side, side, n_classes)`, 0 where nothing
    is predicted, and the (H, W) bool mask of the predicted pixels"""
    H, W = scene.shape[:2]
    off = geo['off']
    idx = origins((H, W), kernel, buff, cover)
    out, mask = None, np.zeros((H, W), bool)
    for s in range(0, len(idx), batch_size):
        part = idx[s:s + batch_size]
        hi, lo = cut_chips(scene, stack, part, geo, T, rescale, maxval)
        pred = np.asarray(predict(hi, lo))
        if out is None:
            out = np.zeros((H, W, pred.shape[-1]), np.float32)
        for k, (y, x) in enumerate(part):
            hh, ww = min(kernel, H - y), min(kernel, W - x)
            out[y:y + hh, x:x + ww] = pred[k, off:off + hh, off:off + ww]
            mask[y:y + hh, x:x + ww] = True
    return out, mask
