"""Overlap-tile (sliding window) inference: drop-in for the chip helpers of the reference's
utils/prediction_tools.py:87-156, with the per-chip batch-1 `m.predict` loop replaced by
batched device inference.

Index arithmetic is restated exactly (including the exclusive range stop that skips a chip
ending on the image edge and the never-predicted buff//2 border), so
outputs are identical to the reference's for the same model outputs.
"""
import numpy as np


def generate_chip_indices(arr, buff=128, kernel=256):
    """utils/prediction_tools.py:87-109.  Returns [(y, x)] upper-left corners of the kernel-sized
    centres; arr is (H, W, C)."""
    H, W, C = arr.shape
    side = buff + kernel
    x_buff = y_buff = buff // 2
    y_indices = list(range(y_buff, H - side, kernel))
    x_indices = list(range(x_buff, W - side, kernel))
    return [(y_index, x_index) for y_index in y_indices for x_index in x_indices]


def extract_chips(arr, buff=128, kernel=256):
    """utils/prediction_tools.py:111-131 (as coded: the (y, x) tuples are unpacked as `x, y`, :127)."""
    x_buff = y_buff = buff // 2
    chips = []
    for x, y in generate_chip_indices(arr, buff, kernel):
        chips.append(arr[y - y_buff:y + kernel + y_buff, x - x_buff:x + kernel + x_buff, :])
    return chips


def _scenes(arr):
    """(scenes, two_date): a single (H, W, C) scene, or the pair (arr_a, arr_b) of co-registered scenes of a two-input change model"""
    if isinstance(arr, (tuple, list)):
        if len(arr) != 2:
            raise ValueError(f'expected one (H, W, C) scene or a pair (arr_a, arr_b), got {len(arr)} arrays')
        a, b = arr
        if a.ndim != 3 or a.shape != b.shape:
            raise ValueError(f'the two scenes must be co-registered (H, W, C) arrays of equal shape, got {a.shape} and {b.shape}')
        return (a, b), True
    return (arr,), False


def predict_chips(arr, chip_indices, template, m, kernel=256, buff=128, batch_size=16, channel=0):
    """utils/prediction_tools.py:133-156: predict every (kernel+buff)^2 chip and accumulate the centre
    kernel^2 of one output channel into `template` (+=).

    Differences from the reference, by design: chips are predicted `batch_size` at a time on the
    device instead of one `m.predict` per chip; a model with list outputs ([probs, classes],
    get_unet_model) contributes its first output (the reference indexes the list as if it were an
    array, Appendix B Q11); `channel` selects the class probability written (reference: 0).

    Two-date change detection (make_siamese_unet, utils/model_tools.py:576-663): `arr = (arr_a, arr_b)`, two co-registered
    (H, W, C) scenes of equal shape (a: T2, b: T1, the model's input order); the chip indices are those of arr_a and every batch
    is predicted as `m.predict([chips_a, chips_b])`."""
    scenes, _ = _scenes(arr)
    y_buff = x_buff = buff // 2
    idx = list(chip_indices)
    for s in range(0, len(idx), batch_size):
        part = idx[s:s + batch_size]
        chips = [np.stack([sc[y - y_buff:y + kernel + y_buff, x - x_buff:x + kernel + x_buff, :] for y, x in part]) for sc in scenes]
        preds = m.predict(chips if len(chips) > 1 else chips[0], batch_size=len(part), verbose=0)
        if isinstance(preds, (list, tuple)):
            preds = preds[0]
        for k, (y, x) in enumerate(part):
            template[y:y + kernel, x:x + kernel] += preds[k, y_buff:(kernel + y_buff), x_buff:(kernel + x_buff), channel]
    return template


def predict_chips_sharded(arr, chip_indices, template, m, kernel=256, buff=128, batch_size=16, channel=0):
    """Multi-GPU form of `predict_chips` (one process per GPU): the chip list of `generate_chip_indices` is split
    round-robin over the ranks, every rank predicts its share into a zero template -- no collective on the data path, the chips
    are independent units (utils/prediction_tools.py:147-154 loops over them one by one) -- and the per-rank templates are
    summed once (disjoint centres, so the sum equals the single-process result).  Every rank returns the full template.
    Without an initialised process group it is `predict_chips`.  `arr` may be a pair of scenes, as for `predict_chips`."""
    import torch
    _scenes(arr)
    from . import parallel
    rank, world = (parallel.dist.get_rank(), parallel.dist.get_world_size()) if parallel.dist.is_initialized() else (0, 1)
    if world == 1:
        return predict_chips(arr, chip_indices, template, m, kernel, buff, batch_size, channel)
    mine = parallel.shard_list(list(chip_indices), rank, world)
    part = predict_chips(arr, mine, np.zeros_like(template), m, kernel, buff, batch_size, channel)
    dev = 'cuda' if parallel.dist.get_backend() == 'nccl' else 'cpu'
    t = torch.from_numpy(np.ascontiguousarray(part)).to(dev)
    parallel.reduce_templates(t)
    template += t.cpu().numpy().astype(template.dtype)
    return template


# ---------------------------------------------------------------------------------------------------------------------------------
# Device-resident scene prediction: the scene goes to the device once, windows are cut there (satcv_scene_gather), the model reads them
# in place (Model.predict_on_device) and the centres are stitched into a device-resident map (satcv_scene_scatter).  Layout, the
# reflect rule and the disjointness contract: DESIGN.md, "Device-resident scene prediction".
_SCENE_KIND = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3}     # kinds of satcv_tile_desc


def _disjoint_runs(origins, height, width):
    """Greedy split, in list order, of placed height x width rectangles with upper-left corners `origins` [(y, x)] into consecutive runs
    [(start, stop)] whose rectangles are pairwise disjoint: a rectangle that overlaps one of the current run opens the next run.  One
    run is one scatter launch (its contract: no two chips of a launch write the same pixel); runs are launched in order."""
    runs, start = [], 0
    for i, (y, x) in enumerate(origins):
        if any(abs(y - origins[j][0]) < height and abs(x - origins[j][1]) < width for j in range(start, i)):
            runs.append((start, i))
            start = i
    if len(origins) > start:
        runs.append((start, len(origins)))
    return runs


def full_cover_indices(shape, kernel=256):
    """Centre origins of the full-cover grid of an (H, W[, C]) scene: range(0, H, kernel) x range(0, W, kernel).  The centres tile the
    scene, the last row / column clipped by the scatter, so every pixel is predicted exactly once."""
    H, W = int(shape[0]), int(shape[1])
    return [(y, x) for y in range(0, H, kernel) for x in range(0, W, kernel)]


def _check_geometry(kernel, buff, batch_size):
    if int(kernel) < 1 or int(buff) < 0 or int(batch_size) < 1:
        raise ValueError(f'kernel and batch_size must be positive and buff non-negative, got kernel={kernel}, buff={buff}, batch_size={batch_size}')


def _check_windows(idx, H, W, kernel, off):
    for y, x in idx:
        if y - off < 0 or x - off < 0 or y + kernel + off > H or x + kernel + off > W:
            raise ValueError(f'chip index ({y}, {x}): its window rows {y - off}:{y + kernel + off}, columns {x - off}:{x + kernel + off} '
                             f'leaves the {H} x {W} scene')


def _patch_grid(patches, cols, patch_hw, kernel_shape, kernel_buffer):
    """Placement rule of callback_predictions (utils/prediction_tools.py:245-291), as coded there.  Returns
    (crop, origins, mosaic_hw): crop = (row0, col0, height, width) of the window kept of every patch, origins = [(y, x)] of the kept
    patches in the mosaic.

    The half buffers are x_buffer = kernel_buffer[0] // 2 and y_buffer = kernel_buffer[1] // 2.  The window keeps patch rows from
    y_buffer up to (not including) kernel_shape[1] + x_buffer and columns from x_buffer up to kernel_shape[0] + y_buffer (:258-267: the
    start of each axis uses its own buffer, the stop the other axis' one), limited to the patch like any NumPy slice.  Patch i goes to
    mosaic row i // cols, column i % cols; only complete mosaic rows are kept (:282-288), so a trailing partial row is dropped."""
    patches, cols = int(patches), int(cols)
    if cols < 1 or patches // cols < 1:
        raise ValueError(f'totalPatches={patches} does not fill one mosaic row of patchesPerRow={cols}')
    x_buffer, y_buffer = int(kernel_buffer[0] / 2), int(kernel_buffer[1] / 2)
    row0, row1 = y_buffer, min(int(kernel_shape[1]) + x_buffer, int(patch_hw[0]))
    col0, col1 = x_buffer, min(int(kernel_shape[0]) + y_buffer, int(patch_hw[1]))
    if row1 <= row0 or col1 <= col0:
        raise ValueError(f'empty crop rows {row0}:{row1}, columns {col0}:{col1} of a {patch_hw[0]} x {patch_hw[1]} patch')
    ch, cw = row1 - row0, col1 - col0
    rows = patches // cols
    origins = [((i // cols) * ch, (i % cols) * cw) for i in range(rows * cols)]
    return (row0, col0, ch, cw), origins, (rows * ch, cols * cw)


def _to_device(a, what):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)                 # (bytes only: the kernel is told the real kind)
    try:
        return torch.from_numpy(a).to('cuda')
    except torch.cuda.OutOfMemoryError as e:
        raise MemoryError(f'{what} of {a.nbytes / 2 ** 20:.0f} MiB does not fit in device memory (scenes are not tiled into strips)') from e


def _device_empty(shape, dtype, what, fill=None):
    import torch
    try:
        return torch.empty(shape, dtype=dtype, device='cuda') if fill is None else torch.full(shape, fill, dtype=dtype, device='cuda')
    except torch.cuda.OutOfMemoryError as e:
        raise MemoryError(f'{what} of shape {tuple(shape)} does not fit in device memory (scenes are not tiled into strips)') from e


def _scatter(src, src_first, n, crop, origins_dev, total, first, dst, doff, c0, nc, accumulate):
    """centres of chips [src_first, src_first + n) of the (N, sh, sw[, lds]) tensor `src` -> map `dst` (H, W, ldd) at origins[first:first + n]"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import SceneScatterDesc, check, lib
    sh, sw = src.shape[1], src.shape[2]
    lds = src.shape[3] if src.dim() == 4 else 1
    d = SceneScatterDesc(src=src.data_ptr() + src_first * sh * sw * lds * src.element_size(), src_kind=2 if src.dtype == torch.float32 else 5,
                         n=n, sh=sh, sw=sw, lds=lds, c0=c0, nc=nc, crop_y=crop[0], crop_x=crop[1], crop_h=crop[2], crop_w=crop[3],
                         origins=origins_dev.data_ptr(), total=total, first=first, dst=dst.data_ptr(), dst_kind=2 if dst.dtype == torch.float32 else 0,
                         h=dst.shape[0], w_=dst.shape[1], ldd=dst.shape[2], doff=doff, accumulate=int(accumulate))
    check(lib.satcv_scene_scatter(C.byref(d), ops.stream_ptr()))


def _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, channel, want_classes, rescale):
    """Shared loop of predict_chips_device / predict_scene: -> (device map (H, W, nc) float32, device class map (H, W, 1) uint8 or
    None).  channel: int, or None for every class.  A scene is a host array, or a contiguous float32 CUDA tensor (H, W, C) that is
    read where it lies."""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import SceneGatherDesc, check, lib
    H, W = scenes[0].shape[:2]
    off = buff // 2
    side = kernel + 2 * off                  # the window of predict_chips; kernel + buff for an even buff
    dev, kinds = [], []
    for sc in scenes:
        if isinstance(sc, torch.Tensor):     # a scene that is already resident (pc_tools.median_composite): used in place
            if not (sc.is_cuda and sc.dtype == torch.float32 and sc.dim() == 3 and sc.is_contiguous()):
                raise ValueError(f'a tensor scene must be a contiguous float32 CUDA tensor (H, W, C), got {sc.dtype} {tuple(sc.shape)} on {sc.device}')
            dev.append(sc)
            kinds.append(_SCENE_KIND[np.dtype(np.float32)])
            continue
        sc = np.asarray(sc)
        if sc.dtype not in _SCENE_KIND:
            if rescale:
                raise ValueError(f'rescale needs a uint8 / uint16 / int16 / float32 scene, got {sc.dtype}')
            sc = sc.astype(np.float32)        # what Model.predict does with a host batch
        dev.append(_to_device(sc, 'the scene'))
        kinds.append(_SCENE_KIND[sc.dtype])
    total = len(idx)
    origins = _to_device(np.asarray(idx, np.int32).reshape(total, 2), 'the origin table')
    runs = [[(s + a, s + b) for a, b in _disjoint_runs(idx[s:s + batch_size], kernel, kernel)] for s in range(0, total, batch_size)]
    nb = min(batch_size, total)
    bufs = [_device_empty((nb, side, side, sc.shape[2]), torch.float32, 'the chip batch') for sc in dev]
    st = ops.stream_ptr()
    out = cls = None
    # No host synchronisation inside this loop.  Every launch -- gather, the plan's kernels, scatter -- goes to the current stream, so
    # stream order alone keeps the gather of batch i + 1 from overwriting `bufs` (and the plan from overwriting its output tensors) while
    # batch i still reads them.
    for b, s in enumerate(range(0, total, batch_size)):
        n = min(batch_size, total - s)
        xs = []
        for sc, kind, buf in zip(dev, kinds, bufs):
            d = SceneGatherDesc(src=sc.data_ptr(), src_kind=kind, h=H, w_=W, c=sc.shape[2], rescale=float(rescale or 0.0),
                                origins=origins.data_ptr(), total=total, first=s, n=n, off=off, side=side,
                                dst=buf.data_ptr(), ldc=sc.shape[2], coff=0)
            check(lib.satcv_scene_gather(C.byref(d), st))
            xs.append(buf[:n])
        res = m.predict_on_device(xs if len(xs) > 1 else xs[0])
        res = list(res) if isinstance(res, (list, tuple)) else [res]
        probs = res[0]
        if probs.dtype != torch.float32 or not probs.is_contiguous():
            probs = probs.to(torch.float32).contiguous()
        if out is None:
            ncls = probs.shape[-1]
            if channel is not None and not -ncls <= channel < ncls:
                raise IndexError(f'channel {channel} of a {ncls}-class output')
            c0, nc = (0, ncls) if channel is None else (channel % ncls, 1)
            out = _device_empty((H, W, nc), torch.float32, 'the prediction map', 0.0)
            if want_classes:
                if len(res) < 2 or res[1].dim() != 3:
                    raise ValueError('classes=True needs a model with an (n, h, w) class output next to its probabilities')
                cls = _device_empty((H, W, 1), torch.uint8, 'the class map', 255)
        for a, e in runs[b]:
            _scatter(probs, a - s, e - a, (off, off, kernel, kernel), origins, total, a, out, 0, c0, nc, True)
            if cls is not None:
                _scatter(res[1], a - s, e - a, (off, off, kernel, kernel), origins, total, a, cls, 0, 0, 1, False)
    return out, cls


def predict_chips_device(arr, chip_indices, template, m, kernel=256, buff=128, batch_size=16, channel=0, rescale=None):
    """`predict_chips` with the scene and the prediction map resident on the device: same signature, same result.

    The scene(s) go to the device once in their own dtype (uint8 / uint16 / int16 / float32; `rescale` divides an integer scene in
    float64 and rounds to float32, (scene.astype(float64) / rescale).astype(float32)), the index list once.  Per batch the windows are
    gathered on the device, predicted by `m.predict_on_device` and the centres of `probs[..., channel]` accumulated into a zero float32
    device map; nothing synchronises with the host until the one copy back, after which `template += map`.  Every pixel of the map
    receives the value `predict_chips` would add, so for chips with disjoint centres the two functions return equal templates.

    Differences from `predict_chips`:
    * an index whose window leaves the scene raises ValueError (there a negative start wraps silently and an overrun fails on shapes);
    * centres that overlap (legal in both) are summed in float32 on the device, in list order, before they meet the template, where
      `predict_chips` adds each in the template's dtype.
    `arr` may be the two-date pair (arr_a, arr_b), as for `predict_chips`.  A scene that is already resident -- a contiguous float32 CUDA
    tensor (H, W, C), e.g. from `pc_tools.median_composite` -- is read in place.  An empty index list returns `template` untouched."""
    scenes, _ = _scenes(arr)
    _check_geometry(kernel, buff, batch_size)
    idx = [(int(y), int(x)) for y, x in chip_indices]
    if not idx:
        return template
    if scenes[0].ndim != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {scenes[0].shape}')
    _check_windows(idx, scenes[0].shape[0], scenes[0].shape[1], kernel, buff // 2)
    out, _ = _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, int(channel), False, rescale)
    template += out[..., 0].cpu().numpy()
    return template


def predict_scene(arr, m, kernel=256, buff=128, batch_size=16, channel=0, cover='reference', classes=False, rescale=None):
    """Prediction map of a whole (H, W, C) scene (or two-date pair of scenes), stitched on the device; returns new arrays.

    cover='reference': the chips of `generate_chip_indices` -- the buff // 2 border and a last chip ending on the image edge stay
    unpredicted (0 in the map, 255 in the class map), as in the reference.
    cover='full': centres on the grid range(0, H, kernel) x range(0, W, kernel); windows that overhang the scene are filled by
    reflection (np.pad mode='reflect') inside the gather and the centres are clipped to the scene, so every pixel is predicted exactly
    once.  Needs H, W >= kernel + buff (one reflection then suffices), else ValueError.
    channel: int -> (H, W) float32; None -> (H, W, n_classes).  classes=True returns (map, class map (H, W) uint8) from the model's
    second output (ValueError for a single-output model).  The returned arrays are the only device-to-host traffic.  A scene may be a
    contiguous float32 CUDA tensor (H, W, C), read in place."""
    scenes, _ = _scenes(arr)
    _check_geometry(kernel, buff, batch_size)
    if scenes[0].ndim != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {scenes[0].shape}')
    H, W = scenes[0].shape[:2]
    if cover == 'reference':
        idx = generate_chip_indices(scenes[0], buff, kernel)
    elif cover == 'full':
        if H < kernel + buff or W < kernel + buff:
            raise ValueError(f"cover='full' needs a scene of at least kernel + buff = {kernel + buff} pixels a side, got {H} x {W}")
        idx = full_cover_indices((H, W), kernel)
    else:
        raise ValueError(f"cover must be 'reference' or 'full', got {cover!r}")
    if classes and len(getattr(m, 'outputs', ())) < 2:
        raise ValueError('classes=True needs a model with a class output next to its probabilities')
    if not idx:                              # (a scene too small for one reference chip: nothing is predicted)
        ncls = m.outputs[0].channels
        probs = np.zeros((H, W) if channel is not None else (H, W, ncls), np.float32)
        return (probs, np.full((H, W), 255, np.uint8)) if classes else probs
    out, cls = _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, None if channel is None else int(channel), classes, rescale)
    probs = (out if channel is None else out[..., 0]).cpu().numpy()
    return (probs, cls[..., 0].cpu().numpy()) if classes else probs


# ---------------------------------------------------------------------------------------------------------------------------------
# Scene prediction for the ConvLSTM2D time-series models (lstm_tools.LSTMModel / LSTMAutoencoder): the (T, C, H, W) stack goes to the
# device once, satcv_series_gather cuts, normalises and ingests a chip batch in one launch, the model reads the result in place
# (predict_on_device(..., shape=...)) and satcv_scene_scatter stitches the centres.  DESIGN.md, "Scene prediction for the time-series
# models".
_SERIES_KIND = {np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3}     # kinds of satcv_tile_desc the gather reads


def predict_series_scene(stack, m, kernel=256, buff=128, batch_size=16, channel=0, cover='reference', classes=False, maxval=10000,
                         harmonics=None, plan=None):
    """Prediction map of a (T, C, H, W) time stack -- the layout of the LSTMDataGenerator files and of `pc_tools.median_composite`'s
    input -- by a ConvLSTM2D time-series model (get_lstm_model, get_lstm_autoencoder), stitched on the device; returns new arrays.

    stack: a host array (uint16 / int16 / float32; anything else is cast to float32) or a contiguous int16 / float32 CUDA tensor, read in
    place.  The first m.n_time acquisitions are used (of a host stack only those are uploaded); every sample becomes float32(float64(v) / maxval) with NaN -> 0
    (normalize_timeseries, what LSTMDataGenerator feeds the model).  ValueError unless the stack is 4-D with T >= m.n_time and
    C == m.n_channels.
    kernel, buff, batch_size, channel, cover, classes: as for `predict_scene` -- cover='reference' predicts the chips of
    `generate_chip_indices` on the (H, W) plane (the border stays 0, 255 in the class map), cover='full' the full-cover grid with
    reflected windows (needs H, W >= kernel + buff); channel int -> (H, W) float32, None -> (H, W, n_classes); classes=True returns
    (map, class map (H, W) uint8) and needs a model with a softmax head (ValueError for another head or an autoencoder).
    harmonics=(sin, cos): the scene-wide harmonic pair of an LSTMAutoencoder (processing.sin_cos of the series' start), whose `single`
    output -- the next image -- is the map; required for the autoencoder, refused for any other model.
    plan: None runs every batch through m.predict_on_device (the eager tape).  True builds one lstm_infer.SeriesInferPlan for batch_size
    chips (m.inference_plan), a SeriesInferPlan built for (batch_size, m.n_time, kernel + buff, kernel + buff) is used as given: the
    batches run through its preallocated, graph-replayed forward; a short last batch fills a prefix of the plan's input, the stale rest
    is computed and ignored.
    The returned arrays are the only device-to-host traffic; hybrid and hierarchical models (two inputs at two resolutions) go through
    `predict_hybrid_scene`."""
    from .lstm_tools import LSTMAutoencoder
    _check_geometry(kernel, buff, batch_size)
    if getattr(stack, 'ndim', None) != 4:
        raise ValueError(f'expected a (T, C, H, W) time stack, got shape {tuple(getattr(stack, "shape", ()))}')
    T, C_, H, W = (int(v) for v in stack.shape)
    if T < m.n_time:
        raise ValueError(f'the model reads {m.n_time} acquisitions, the stack holds {T}')
    if C_ != m.n_channels:
        raise ValueError(f'the model reads {m.n_channels} bands, the stack holds {C_}')
    if not float(maxval) or float(maxval) != float(maxval):
        raise ValueError(f'maxval must be a non-zero number, got {maxval}')
    if cover == 'reference':
        idx = generate_chip_indices(np.empty((H, W, 0)), buff, kernel)
    elif cover == 'full':
        if H < kernel + buff or W < kernel + buff:
            raise ValueError(f"cover='full' needs a scene of at least kernel + buff = {kernel + buff} pixels a side, got {H} x {W}")
        idx = full_cover_indices((H, W), kernel)
    else:
        raise ValueError(f"cover must be 'reference' or 'full', got {cover!r}")
    is_ae = isinstance(m, LSTMAutoencoder)
    if is_ae and harmonics is None:
        raise ValueError('an LSTMAutoencoder needs harmonics=(sin, cos), its second input')
    if harmonics is not None:
        if not is_ae:
            raise ValueError('harmonics is the second input of an LSTMAutoencoder; this model has none')
        if len(harmonics) != 2:
            raise ValueError(f'harmonics must be the pair (sin, cos), got {len(harmonics)} values')
        harmonics = (float(harmonics[0]), float(harmonics[1]))
    if classes and (is_ae or not getattr(m, 'class_output', True)):
        raise ValueError("classes=True needs a model with a class output: an LSTMModel with activation='softmax'")
    ncls = m.n_classes if idx else None
    if idx and channel is not None and not -ncls <= int(channel) < ncls:
        raise IndexError(f'channel {channel} of a {ncls}-class output')
    if not idx:                              # (a scene too small for one reference chip: nothing is predicted)
        probs = np.zeros((H, W) if channel is not None else (H, W, m.n_classes), np.float32)
        return (probs, np.full((H, W), 255, np.uint8)) if classes else probs
    if plan is not None and plan is not False:
        side = kernel + 2 * (buff // 2)
        want = (min(batch_size, len(idx)), m.n_time, side, side)
        if plan is True:
            plan = m.inference_plan(want)
        elif getattr(plan, 'model', None) is not m or tuple(plan.shape) != want:
            raise ValueError(f'plan must be a SeriesInferPlan of this model for shape {want}, got {getattr(plan, "shape", plan)!r}')
    else:
        plan = None
    out, cls = _stitch_series(stack, idx, m, kernel, buff, batch_size, None if channel is None else int(channel), classes, float(maxval), harmonics,
                              plan)
    probs = (out if channel is None else out[..., 0]).cpu().numpy()
    return (probs, cls[..., 0].cpu().numpy()) if classes else probs


def _stitch_series(stack, idx, m, kernel, buff, batch_size, channel, want_classes, maxval, harmonics, plan=None):
    """the batch loop of predict_series_scene: -> (device map (H, W, nc) float32, device class map (H, W, 1) uint8 or None)"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import SeriesGatherDesc, check, lib
    T, C_, H, W = stack.shape
    steps = m.n_time
    off = buff // 2
    side = kernel + 2 * off
    if isinstance(stack, torch.Tensor):      # a stack that is already resident: read where it lies
        if not (stack.is_cuda and stack.dtype in (torch.int16, torch.float32) and stack.is_contiguous()):
            raise ValueError(f'a tensor stack must be a contiguous int16 / float32 CUDA tensor (T, C, H, W), got {stack.dtype} on {stack.device}')
        dev, kind = stack, _SERIES_KIND[np.dtype(np.int16 if stack.dtype == torch.int16 else np.float32)]
    else:
        st_ = np.asarray(stack)[:steps]      # (only the acquisitions the model reads are cast and uploaded: a contiguous prefix)
        T = steps
        if st_.dtype not in _SERIES_KIND:
            st_ = st_.astype(np.float32)
        kind = _SERIES_KIND[st_.dtype]
        dev = _to_device(st_, 'the time stack')
    total = len(idx)
    origins = _to_device(np.asarray(idx, np.int32).reshape(total, 2), 'the origin table')
    runs = [[(s + a, s + b) for a, b in _disjoint_runs(idx[s:s + batch_size], kernel, kernel)] for s in range(0, total, batch_size)]
    nb = min(batch_size, total)
    cpad, dtype = ops.rup(C_, 16), m.dtype_code
    # with a plan, full batches are gathered straight into its static input; a short last batch goes through a buffer of its own and
    # is spread over a prefix of every time step by plan.run
    buf = plan.x_in.view(-1) if plan is not None else _device_empty((steps * nb * side * side * cpad,), ops.TORCH_DTYPE[dtype], 'the chip batch')
    short = _device_empty((steps * (total % nb) * side * side * cpad,), ops.TORCH_DTYPE[dtype], 'the chip batch') if plan is not None and total % nb else None
    sincos = None
    if harmonics is not None:
        sincos = _device_empty((nb, side, side, 2), torch.float32, 'the harmonics')
        sincos[..., 0] = harmonics[0]
        sincos[..., 1] = harmonics[1]
    ncls = m.n_classes
    c0, nc = (0, ncls) if channel is None else (channel % ncls, 1)
    out = _device_empty((H, W, nc), torch.float32, 'the prediction map', 0.0)
    cls = _device_empty((H, W, 1), torch.uint8, 'the class map', 255) if want_classes else None
    st = ops.stream_ptr()
    # No host synchronisation inside this loop.  Every launch -- gather, the model's kernels, scatter -- goes to the current stream, so
    # stream order alone keeps the gather of batch i + 1 from overwriting `buf` (and the model from overwriting its output tensors) while
    # batch i still reads them.
    for b, s in enumerate(range(0, total, batch_size)):
        n = min(batch_size, total - s)
        xt = (buf if n == nb or short is None else short)[:steps * n * side * side * cpad].view(steps * n, side, side, cpad)      # (steps, n, ...) is contiguous for every n
        d = SeriesGatherDesc(src=dev.data_ptr(), src_kind=kind, t=T, c=C_, h=H, w_=W, steps=steps, maxval=maxval, origins=origins.data_ptr(),
                             total=total, first=s, n=n, off=off, side=side, dst=xt.data_ptr(), dtype=dtype, cpad=cpad)
        check(lib.satcv_series_gather(C.byref(d), st))
        try:
            if plan is not None:
                res = plan.run(xt if sincos is None else [xt, sincos[:n]], want_classes=want_classes)
                res = res if want_classes else (res,)
            elif sincos is not None:
                res = (m.predict_on_device([xt, sincos[:n]], shape=(n, steps, side, side)),)
            elif want_classes:
                res = m.predict_on_device(xt, shape=(n, steps, side, side), want_classes=True)
            else:
                res = (m.predict_on_device(xt, shape=(n, steps, side, side)),)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f'a batch of {n} chips of {steps} x {side} x {side} does not fit in device memory; lower batch_size') from e
        for a, e in runs[b]:
            _scatter(res[0], a - s, e - a, (off, off, kernel, kernel), origins, total, a, out, 0, c0, nc, True)
            if cls is not None:
                _scatter(res[1], a - s, e - a, (off, off, kernel, kernel), origins, total, a, cls, 0, 0, 1, False)
    return out, cls


# ---------------------------------------------------------------------------------------------------------------------------------
# Scene prediction for the two-resolution models (lstm_tools.HybridModel / HierarchicalModel): a fine (H, W, C) scene and a coarse
# (T, c, h, w) time stack with H = r h, W = r w.  Per batch one satcv_scene_gather on the fine grid, one satcv_series_gather on the coarse
# grid, the model up to its last dense layer, and satcv_dense_scene_fwd, which computes that layer on the chip centres only and stores
# them into the map.  DESIGN.md, "Scene prediction for the hybrid and hierarchical models".
def hybrid_chip_tables(hi_shape, lo_shape, kernel, buff, cover, multiple=1):
    """Chip geometry on two grids.  hi_shape = (H, W[, ...]) of the fine plane, lo_shape = (h, w) of the coarse one, with one integer ratio
    r >= 1: H == r h and W == r w.  -> (hi, lo, geo): int32 (total, 2) tables of the (y, x) centre origins on the fine grid
    (`generate_chip_indices` for cover='reference', `full_cover_indices` for cover='full') and of the same chips on the coarse grid
    (hi // r), and geo = dict(r, off, side, off_lo, side_lo): a fine window starts at origin - off and is side = kernel + 2 (buff // 2)
    wide, a coarse window starts at origin_lo - off_lo and is side_lo = side // r wide.

    ValueError unless kernel % r == 0, (buff // 2) % r == 0 and side % multiple == 0 (multiple: the product of the pooling factors of the
    U-Net branch of a hybrid model, 1 for the hierarchical model); cover='full' needs H, W >= side.  With these conditions every fine
    window starts on a multiple of r, so the nearest resize inside the model maps fine chip pixel u to coarse chip pixel u // r: the
    coarse chip is exactly the coarse footprint of the fine chip."""
    H, W = int(hi_shape[0]), int(hi_shape[1])
    h, w = int(lo_shape[0]), int(lo_shape[1])
    kernel, buff, multiple = int(kernel), int(buff), int(multiple)
    if kernel < 1 or buff < 0 or multiple < 1:
        raise ValueError(f'kernel and multiple must be positive and buff non-negative, got kernel={kernel}, buff={buff}, multiple={multiple}')
    if min(H, W, h, w) < 1 or H % h or W % w:
        raise ValueError(f'ratio: the fine plane {H} x {W} is not an integer multiple of the coarse plane {h} x {w}')
    r = H // h
    if W // w != r:
        raise ValueError(f'ratio: rows {H} / {h} = {r} and columns {W} / {w} = {W // w} differ')
    off = buff // 2
    side = kernel + 2 * off
    if kernel % r:
        raise ValueError(f'kernel = {kernel} is not a multiple of the resolution ratio r = {r}')
    if off % r:
        raise ValueError(f'buff // 2 = {off} is not a multiple of the resolution ratio r = {r}')
    if side % multiple:
        raise ValueError(f'side = kernel + 2 (buff // 2) = {side} is not a multiple of {multiple}')
    if cover == 'reference':
        idx = generate_chip_indices(np.empty((H, W, 0)), buff, kernel)
    elif cover == 'full':
        if H < side or W < side:
            raise ValueError(f"cover='full' needs a scene of at least side = {side} pixels a side, got {H} x {W}")
        idx = full_cover_indices((H, W), kernel)
    else:
        raise ValueError(f"cover must be 'reference' or 'full', got {cover!r}")
    hi = np.asarray(idx, np.int32).reshape(len(idx), 2)
    assert not (hi % r).any()
    return hi, hi // r, dict(r=r, off=off, side=side, off_lo=off // r, side_lo=side // r)


def _hybrid_head(m, output):
    """(the last dense layer that writes the map, multiple of the chip side) of a two-resolution model"""
    from .lstm_tools import HierarchicalModel, HybridModel
    if isinstance(m, HybridModel):
        if output not in (None,) + tuple(m.output_names):
            raise ValueError(f'output must be one of {m.output_names}, got {output!r}')
        return m.fusion, int(np.prod(m.factors))
    if isinstance(m, HierarchicalModel):
        output = 'lstm_probs' if output is None else output
        if output not in m.output_names:
            raise ValueError(f'output must be one of {m.output_names}, got {output!r}')
        return {'sub_probs': m.sub, 'acnn_probs': m.acnn, 'lstm_probs': m.fuse}[output], 1
    raise ValueError(f'predict_hybrid_scene covers HybridModel and HierarchicalModel, got {type(m).__name__}')


def predict_hybrid_scene(scene, stack, m, kernel=256, buff=128, batch_size=16, channel=0, cover='reference', classes=False, rescale=None,
                         maxval=10000, output=None, plan=None):
    """Prediction map of a fine (H, W, C) scene together with a coarse (T, c, h, w) time stack by a two-resolution model
    (get_hybrid_model, get_hierarchical_model), stitched on the device; returns new arrays.

    scene: as for `predict_scene` -- a host array (uint8 / uint16 / int16 / float32, `rescale` divides in float64 and rounds to float32;
    anything else is cast to float32) or a contiguous float32 CUDA tensor read in place.  stack: as for `predict_series_scene` -- the first
    m.n_time acquisitions, float32(float64(v) / maxval) with NaN -> 0, a host array or a contiguous int16 / float32 CUDA tensor.
    Geometry: `hybrid_chip_tables` (H == r h, W == r w, kernel and buff // 2 multiples of r, the chip side a multiple of the U-Net
    branch's pooling product); ValueError otherwise.  kernel, buff, batch_size, channel, cover, classes: as for `predict_scene`; the border
    the reference cover leaves out stays 0 (255 in the class map).
    output: the head that is mapped -- None: 'probabilities' (hybrid) / 'lstm_probs' (hierarchical); the hierarchical model also takes
    'sub_probs' and 'acnn_probs'.  classes=True needs a softmax head.
    plan: None runs every batch through m.predict_on_device; True builds a lstm_infer.HybridInferPlan(m, batch_size, side, side_lo), a
    HybridInferPlan of this model and these sizes is used as given (HybridModel only: NotImplementedError for a hierarchical model, whose
    ACNN trunk lives on the tape).
    Per batch the model stops before its last dense layer; satcv_dense_scene_fwd computes that layer on the chip centres and stores
    them into the map.  The returned arrays are the only device-to-host traffic."""
    import torch
    from .lstm_tools import HierarchicalModel
    head, multiple = _hybrid_head(m, output)
    _check_geometry(kernel, buff, batch_size)
    if getattr(scene, 'ndim', None) != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {tuple(getattr(scene, "shape", ()))}')
    if getattr(stack, 'ndim', None) != 4:
        raise ValueError(f'expected a (T, c, h, w) time stack, got shape {tuple(getattr(stack, "shape", ()))}')
    H, W, C_ = (int(v) for v in scene.shape)
    T, c_, h, w = (int(v) for v in stack.shape)
    if C_ != m.hi_channels:
        raise ValueError(f'the model reads {m.hi_channels} fine bands, the scene holds {C_}')
    if T < m.n_time:
        raise ValueError(f'the model reads {m.n_time} acquisitions, the stack holds {T}')
    if c_ != m.n_channels:
        raise ValueError(f'the model reads {m.n_channels} coarse bands, the stack holds {c_}')
    if not float(maxval) or float(maxval) != float(maxval):
        raise ValueError(f'maxval must be a non-zero number, got {maxval}')
    hi, lo, geo = hybrid_chip_tables((H, W), (h, w), kernel, buff, cover, multiple)
    ncls = head.cout
    if classes and head.activation != head.ACT['softmax']:
        raise ValueError(f'classes=True needs a head with a class output (softmax); {head.name!r} has none')
    if channel is not None and not -ncls <= int(channel) < ncls:
        raise IndexError(f'channel {channel} of a {ncls}-class output')
    if plan is not None and plan is not False and isinstance(m, HierarchicalModel):
        raise NotImplementedError('plan: HybridInferPlan covers HybridModel; the ACNN trunk of a HierarchicalModel lives on the tape')
    if not len(hi):                          # (a scene too small for one reference chip: nothing is predicted)
        probs = np.zeros((H, W) if channel is not None else (H, W, ncls), np.float32)
        return (probs, np.full((H, W), 255, np.uint8)) if classes else probs
    if plan is not None and plan is not False:
        want = (min(int(batch_size), len(hi)), geo['side'], geo['side_lo'])
        if plan is True:
            try:
                plan = m.scene_plan(*want)
            except torch.cuda.OutOfMemoryError as e:
                raise MemoryError(f'a HybridInferPlan for (batch, side, side_lo) = {want} does not fit in device memory; lower batch_size') from e
        elif getattr(plan, 'model', None) is not m or tuple(getattr(plan, 'shape', ())) != want:
            raise ValueError(f'plan must be a HybridInferPlan of this model for (batch, side, side_lo) = {want}, got {getattr(plan, "shape", plan)!r}')
    else:
        plan = None
    out, cls = _stitch_hybrid(scene, stack, hi, lo, geo, m, head, output, int(kernel), int(batch_size), None if channel is None else int(channel),
                              bool(classes), rescale, float(maxval), plan)
    probs = (out if channel is None else out[..., 0]).cpu().numpy()
    return (probs, cls.cpu().numpy()) if classes else probs


def _stitch_hybrid(scene, stack, hi, lo, geo, m, head, output, kernel, batch_size, channel, want_classes, rescale, maxval, plan):
    """the batch loop of predict_hybrid_scene: -> (device map (H, W, nc) float32, device class map (H, W) uint8 or None)"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import DenseSceneDesc, SceneGatherDesc, SeriesGatherDesc, check, lib
    from .lstm_tools import HybridModel
    H, W, C_ = scene.shape
    T, c_, h, w = stack.shape
    steps, off, side, off_lo, side_lo = m.n_time, geo['off'], geo['side'], geo['off_lo'], geo['side_lo']
    if isinstance(scene, torch.Tensor):      # a scene that is already resident: read where it lies
        if not (scene.is_cuda and scene.dtype == torch.float32 and scene.is_contiguous()):
            raise ValueError(f'a tensor scene must be a contiguous float32 CUDA tensor (H, W, C), got {scene.dtype} {tuple(scene.shape)} on {scene.device}')
        sdev, skind = scene, _SCENE_KIND[np.dtype(np.float32)]
    else:
        sc = np.asarray(scene)
        if sc.dtype not in _SCENE_KIND:
            if rescale:
                raise ValueError(f'rescale needs a uint8 / uint16 / int16 / float32 scene, got {sc.dtype}')
            sc = sc.astype(np.float32)
        sdev, skind = _to_device(sc, 'the scene'), _SCENE_KIND[sc.dtype]
    if isinstance(stack, torch.Tensor):
        if not (stack.is_cuda and stack.dtype in (torch.int16, torch.float32) and stack.is_contiguous()):
            raise ValueError(f'a tensor stack must be a contiguous int16 / float32 CUDA tensor (T, c, h, w), got {stack.dtype} on {stack.device}')
        tdev, tkind = stack, _SERIES_KIND[np.dtype(np.int16 if stack.dtype == torch.int16 else np.float32)]
    else:
        st_ = np.asarray(stack)[:steps]      # (only the acquisitions the model reads are cast and uploaded: a contiguous prefix)
        T = steps
        if st_.dtype not in _SERIES_KIND:
            st_ = st_.astype(np.float32)
        tdev, tkind = _to_device(st_, 'the time stack'), _SERIES_KIND[st_.dtype]
    total = len(hi)
    org_hi, org_lo = _to_device(hi, 'the origin table'), _to_device(np.ascontiguousarray(lo, np.int32), 'the origin table')
    nb = min(batch_size, total)
    cpad, dtype = ops.rup(c_, 16), m.dtype_code
    td = ops.TORCH_DTYPE[dtype]
    buf_hi = _device_empty((nb, side, side, C_), torch.float32, 'the fine chip batch')
    # with a plan, full batches are gathered straight into its static input; a short last batch goes through a buffer of its own and is
    # spread over a prefix of every time step by plan.run
    buf_lo = plan.x_in.view(-1) if plan is not None else _device_empty((steps * nb * side_lo * side_lo * cpad,), td, 'the coarse chip batch')
    short = _device_empty((steps * (total % nb) * side_lo * side_lo * cpad,), td, 'the coarse chip batch') if plan is not None and total % nb else None
    ncls = head.cout
    c0, nc = (0, ncls) if channel is None else (channel % ncls, 1)
    out = _device_empty((H, W, nc), torch.float32, 'the prediction map', 0.0)
    cls = _device_empty((H, W), torch.uint8, 'the class map', 255) if want_classes else None
    st = ops.stream_ptr()
    kw = {} if isinstance(m, HybridModel) else {'output': output or 'lstm_probs'}
    first = [0]

    def scene_head(d):
        """the model's last dense layer (its sources in `d`) on the chip centres, stored into the map"""
        sd = DenseSceneDesc(head=d, crop_y=off, crop_x=off, crop_h=kernel, crop_w=kernel, origins=org_hi.data_ptr(), total=total, first=first[0],
                            map=out.data_ptr(), map_h=H, map_w=W, ldm=nc, c0=c0, nc=nc, class_map=cls.data_ptr() if cls is not None else None)
        check(lib.satcv_dense_scene_fwd(C.byref(sd), st))
    # No host synchronisation inside this loop.  Every launch -- the gathers, the model's kernels, the head -- goes to the current stream, so
    # stream order alone keeps the gathers of batch i + 1 from overwriting the chip buffers while batch i still reads them.  The windows
    # of both covers are pairwise disjoint, so one head launch per batch meets the kernel's contract.
    for s in range(0, total, batch_size):
        n = min(batch_size, total - s)
        first[0] = s
        d = SceneGatherDesc(src=sdev.data_ptr(), src_kind=skind, h=H, w_=W, c=C_, rescale=float(rescale or 0.0), origins=org_hi.data_ptr(), total=total,
                            first=s, n=n, off=off, side=side, dst=buf_hi.data_ptr(), ldc=C_, coff=0)
        check(lib.satcv_scene_gather(C.byref(d), st))
        xt = (buf_lo if n == nb or short is None else short)[:steps * n * side_lo * side_lo * cpad].view(steps * n, side_lo, side_lo, cpad)
        d = SeriesGatherDesc(src=tdev.data_ptr(), src_kind=tkind, t=T, c=c_, h=h, w_=w, steps=steps, maxval=maxval, origins=org_lo.data_ptr(),
                             total=total, first=s, n=n, off=off_lo, side=side_lo, dst=xt.data_ptr(), dtype=dtype, cpad=cpad)
        check(lib.satcv_series_gather(C.byref(d), st))
        try:
            if plan is not None:
                plan.run(buf_hi[:n], xt, scene_head=scene_head)
            else:
                m.predict_on_device([buf_hi[:n], xt], shape=(n, steps, side_lo, side_lo), scene_head=scene_head, **kw)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f'a batch of {n} chips of {side} x {side} and {steps} x {side_lo} x {side_lo} does not fit in device memory; lower batch_size') from e
    return out, cls


def callback_predictions(imageDataset, model, mixer, kernel_shape=[256, 256], kernel_buffer=[128, 128]):
    """utils/prediction_tools.py:245-291 without its prints: predict mixer['totalPatches'] patches, keep the probability of class 1 and
    assemble the cropped patches into a mosaic of mixer['patchesPerRow'] patches per row; returns the (rows, columns) float32 mosaic.

    The crop and the placement are those of `_patch_grid` (as coded in the reference: each axis starts at its own half buffer and stops
    at its kernel size plus the OTHER axis' half buffer; patch i lands at mosaic row i // patchesPerRow, column i % patchesPerRow; a
    trailing partial row is dropped).  imageDataset: an (N, h, w, c) array or an iterable of batches.  The patches are cropped and
    placed on the device by the scatter kernel; the mosaic is the only copy back."""
    import torch
    from .model_tools import _as_batches
    patches, cols = int(mixer['totalPatches']), int(mixer['patchesPerRow'])
    multi = len(getattr(model, 'inputs', ())) > 1
    batches, _ = _as_batches(imageDataset, None, 16)
    grid = origins = mosaic = None
    filled = 0
    for xb in batches:
        if isinstance(xb, (tuple, list)) and not multi:
            xb = xb[0]
        res = model.predict_on_device(xb)
        probs = (list(res) if isinstance(res, (list, tuple)) else [res])[0]
        if probs.dtype != torch.float32 or not probs.is_contiguous():
            probs = probs.to(torch.float32).contiguous()
        if grid is None:
            if probs.shape[-1] < 2:
                raise ValueError('callback_predictions writes the probability of class 1: the model has a single output channel')
            grid, place, hw = _patch_grid(patches, cols, probs.shape[1:3], kernel_shape, kernel_buffer)
            origins = _to_device(np.asarray(place, np.int32).reshape(-1, 2), 'the origin table')
            mosaic = _device_empty(hw + (1,), torch.float32, 'the mosaic', 0.0)
        n = min(probs.shape[0], len(place) - filled)
        _scatter(probs, 0, n, grid, origins, len(place), filled, mosaic, 0, 1, 1, False)
        filled += n
        if filled >= len(place):
            break
    if grid is None or filled < len(place):
        raise ValueError(f'the dataset ended after {filled} patches, mixer announces {patches}')
    return mosaic[..., 0].cpu().numpy()
