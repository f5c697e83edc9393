"""NumPy restatement of to_tuple (utils/processing.py:335-392) for a BATCH of record planes, as the oracle of
csrc/record_pipeline.hip (helper module, no tests in it).  With dtype=np.float32 it is the host arithmetic of tfrecord_io.to_tuple
operation for operation -- no float64 anywhere, and the mean m_c of the colour step can be injected -- so everything the kernel
computes without a mean of its own must match it bit for bit; with dtype=np.float64 it is the reference value that tolerances are
measured against."""
import numpy as np

BAND, ONEHOT, RESPONSE, RESPONSE_ONEHOT, PASS = 0, 1, 2, 3, 4


def _groups(mode, nband, splits):
    if not splits:
        return [(0, nband)]
    starts = [0] + [int(v) for v in np.cumsum(splits)[:-1]]
    ends = starts[1:] + [nband if mode == 'rescale' else int(sum(splits))]
    return list(zip(starts, ends))


def channel_means(planes, kinds, dtype=np.float32):
    """(n, nband) means over (h, w) as the host computes them: ndarray.mean of the HWC stack in `dtype`."""
    idx = [j for j, (c, _) in enumerate(kinds) if c == BAND]
    return np.stack([np.transpose(p[idx], (1, 2, 0)).astype(dtype).mean(axis=(0, 1)) for p in planes]).astype(dtype)


def to_tuple(planes, kinds, params=None, *, color=True, morph=True, mode='rescale', axes=(2,), splits=None, moments=None, eps=1e-8,
             mean=None, dtype=np.float32):
    """planes (n, k, h, w); kinds [(code, depth)]; params (n, 2 nband + 3) -> (features (n, h, w, cx), labels (n, h, w, cy) or None)"""
    dt = dtype
    planes = np.asarray(planes, np.float32)
    idx = {c: [j for j, (cc, _) in enumerate(kinds) if cc == c] for c in (BAND, ONEHOT, RESPONSE, RESPONSE_ONEHOT, PASS)}
    nband = len(idx[BAND])
    xs, ys = [], []
    for i, p in enumerate(planes):
        bands = np.transpose(p[idx[BAND]], (1, 2, 0)).astype(dt)
        if color:
            m = (bands.mean(axis=(0, 1), keepdims=True) if mean is None else np.asarray(mean[i], dt).reshape(1, 1, nband)).astype(dt)
            contra = params[i, :nband].astype(dt).reshape(1, 1, nband)
            bright = params[i, nband:2 * nband].astype(dt).reshape(1, 1, nband)
            bands = (bands - m) * contra + m * bright
        if mode is not None:
            out = bands.copy()
            for c0, c1 in _groups(mode, nband, splits):
                part = bands[:, :, c0:c1]
                if mode == 'rescale':
                    if moments:
                        mn = np.array([t[0] for t in moments], np.float32)[c0:c1].astype(dt)
                        mx = np.array([t[1] for t in moments], np.float32)[c0:c1].astype(dt)
                    else:
                        mn, mx = part.min(axis=tuple(axes), keepdims=True), part.max(axis=tuple(axes), keepdims=True)
                    out[:, :, c0:c1] = (part - mn) / ((mx - mn) + dt(eps))
                else:
                    if moments:
                        mu = np.array([t[0] for t in moments], np.float32)[c0:c1].astype(dt)
                        var = np.array([t[1] for t in moments], np.float32)[c0:c1].astype(dt)
                    else:
                        mu, var = part.mean(axis=tuple(axes), keepdims=True), part.var(axis=tuple(axes), keepdims=True)
                    out[:, :, c0:c1] = (part - mu) / np.sqrt(var + dt(eps))
            bands = out
        feats = [bands] + [p[j][..., None].astype(dt) for j in idx[PASS]]
        feats += [(p[j].astype(np.uint8)[..., None] == np.arange(kinds[j][1])).astype(dt) for j in idx[ONEHOT]]
        labs = []
        for j, (c, d) in enumerate(kinds):
            if c == RESPONSE:
                labs.append(p[j][..., None].astype(dt))
            elif c == RESPONSE_ONEHOT:
                labs.append((p[j].astype(np.uint8)[..., None] == np.arange(d)).astype(dt))
        stacked = np.concatenate(feats + labs, axis=2)
        if morph:
            flr, fud, rot = params[i, 2 * nband] != 0, params[i, 2 * nband + 1] != 0, int(params[i, 2 * nband + 2])
            stacked = stacked[:, ::-1] if flr else stacked
            stacked = stacked[::-1] if fud else stacked
            stacked = np.rot90(stacked, rot, axes=(0, 1))
        ny = sum(a.shape[2] for a in labs)
        if ny:
            f, l = stacked[:, :, :-ny], stacked[:, :, -ny:]
            ys.append(np.where(l > 1.0, dt(1.0), l))
        else:
            f = stacked
        xs.append(f)
    return np.stack(xs).astype(dt), (np.stack(ys).astype(dt) if ys else None)
