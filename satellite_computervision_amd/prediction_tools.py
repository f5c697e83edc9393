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
# reflect rule and the disjointness contract: DESIGN.md, "Device-resident scene prediction".  The pieces from here to `_stitch_batches`
# are shared by the three predictors of this file (predict_scene, predict_series_scene, predict_hybrid_scene).
_SCENE_KIND = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3}     # kinds of satcv_tile_desc
_SERIES_KIND = {np.dtype(np.uint16): 1, np.dtype(np.float32): 2, np.dtype(np.int16): 3}     # kinds of satcv_tile_desc the series gather reads


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


def _cover_indices(H, W, kernel, buff, cover, need, need_name):
    """The chip list [(y, x)] of a cover of an H x W plane: `generate_chip_indices` for 'reference', `full_cover_indices` for 'full', which
    needs H, W >= need (the caller's window size, named `need_name` in the error: one reflection then fills an overhanging window)."""
    if cover == 'reference':
        return generate_chip_indices(np.empty((H, W, 0)), buff, kernel)
    if cover == 'full':
        if H < need or W < need:
            raise ValueError(f"cover='full' needs a scene of at least {need_name} = {need} pixels a side, got {H} x {W}")
        return full_cover_indices((H, W), kernel)
    raise ValueError(f"cover must be 'reference' or 'full', got {cover!r}")


def _check_geometry(kernel, buff, batch_size):
    if int(kernel) < 1 or int(buff) < 0 or int(batch_size) < 1:
        raise ValueError(f'kernel and batch_size must be positive and buff non-negative, got kernel={kernel}, buff={buff}, batch_size={batch_size}')


def _check_windows(idx, H, W, kernel, off):
    for y, x in idx:
        if y - off < 0 or x - off < 0 or y + kernel + off > H or x + kernel + off > W:
            raise ValueError(f'chip index ({y}, {x}): its window rows {y - off}:{y + kernel + off}, columns {x - off}:{x + kernel + off} '
                             f'leaves the {H} x {W} scene')


def _check_stack(stack, m, layout='(T, C, H, W)', bands='bands'):
    """-> (C, H, W) of a time stack a ConvLSTM model can read: 4-D, at least m.n_time acquisitions of m.n_channels bands"""
    if getattr(stack, 'ndim', None) != 4:
        raise ValueError(f'expected a {layout} time stack, got shape {tuple(getattr(stack, "shape", ()))}')
    T, C_, H, W = (int(v) for v in stack.shape)
    if T < m.n_time:
        raise ValueError(f'the model reads {m.n_time} acquisitions, the stack holds {T}')
    if C_ != m.n_channels:
        raise ValueError(f'the model reads {m.n_channels} {bands}, the stack holds {C_}')
    return C_, H, W


def _check_maxval(maxval):
    if not float(maxval) or float(maxval) != float(maxval):
        raise ValueError(f'maxval must be a non-zero number, got {maxval}')
    return float(maxval)


def _channel_range(channel, ncls):
    """(c0, nc): the channels of an ncls-class output that the map holds -- all of them for channel None, else the one (negative from the end)"""
    if channel is None:
        return 0, ncls
    if not -ncls <= int(channel) < ncls:
        raise IndexError(f'channel {channel} of a {ncls}-class output')
    return int(channel) % ncls, 1


def _resolve_plan(plan, m, want, build, kind, sizes):
    """The `plan` argument of a predictor: None / False -> None (the eager tape), True -> build(), a plan object -> itself if it was built
    for this model and for `want` (its `shape`), else ValueError."""
    if plan is None or plan is False:
        return None
    if plan is True:
        return build()
    if getattr(plan, 'model', None) is not m or tuple(getattr(plan, 'shape', ())) != want:
        raise ValueError(f'plan must be a {kind} of this model for {sizes} {want}, got {getattr(plan, "shape", plan)!r}')
    return plan


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


def _origin_table(idx):
    """the (y, x) origins of a chip list as an int32 (total, 2) device tensor: uploaded once, every launch reads its rows [first, first + n)"""
    return _to_device(np.asarray(idx, np.int32).reshape(len(idx), 2), 'the origin table')


def _resident_scene(sc, rescale):
    """(device tensor (H, W, C), its kind of satcv_tile_desc) of one scene: a host array goes up once in its own dtype, a contiguous
    float32 CUDA tensor (pc_tools.median_composite) is used where it lies"""
    import torch
    if isinstance(sc, torch.Tensor):
        if not (sc.is_cuda and sc.dtype == torch.float32 and sc.dim() == 3 and sc.is_contiguous()):
            raise ValueError(f'a tensor scene must be a contiguous float32 CUDA tensor (H, W, C), got {sc.dtype} {tuple(sc.shape)} on {sc.device}')
        return sc, _SCENE_KIND[np.dtype(np.float32)]
    sc = np.asarray(sc)
    if sc.dtype not in _SCENE_KIND:
        if rescale:
            raise ValueError(f'rescale needs a uint8 / uint16 / int16 / float32 scene, got {sc.dtype}')
        sc = sc.astype(np.float32)            # what Model.predict does with a host batch
    return _to_device(sc, 'the scene'), _SCENE_KIND[sc.dtype]


def _resident_stack(stack, steps, layout):
    """(device tensor (T, C, H, W), its kind of satcv_tile_desc) of a time stack: of a host array the first `steps` acquisitions go up (the
    tensor's T is then `steps`), a contiguous int16 / float32 CUDA tensor is read where it lies"""
    import torch
    if isinstance(stack, torch.Tensor):
        if not (stack.is_cuda and stack.dtype in (torch.int16, torch.float32) and stack.is_contiguous()):
            raise ValueError(f'a tensor stack must be a contiguous int16 / float32 CUDA tensor {layout}, got {stack.dtype} on {stack.device}')
        return stack, _SERIES_KIND[np.dtype(np.int16 if stack.dtype == torch.int16 else np.float32)]
    st_ = np.asarray(stack)[:steps]          # (only the acquisitions the model reads are cast and uploaded: a contiguous prefix)
    if st_.dtype not in _SERIES_KIND:
        st_ = st_.astype(np.float32)
    return _to_device(st_, 'the time stack'), _SERIES_KIND[st_.dtype]


def _scene_gatherer(src, kind, rescale, origins, off, dst):
    """-> gather(first, n): one satcv_scene_gather of the windows of chips [first, first + n) of the resident scene `src` into the
    (nb, side, side, C) float32 buffer `dst`; returns dst[:n].  The descriptor is filled once, a launch sets `first` and `n`."""
    import ctypes as C
    from . import ops
    from ._lib import SceneGatherDesc, check, lib
    H, W, C_ = src.shape
    d = SceneGatherDesc(src=src.data_ptr(), src_kind=kind, h=H, w_=W, c=C_, rescale=float(rescale or 0.0), origins=origins.data_ptr(),
                        total=origins.shape[0], first=0, n=0, off=off, side=dst.shape[1], dst=dst.data_ptr(), ldc=C_, coff=0)
    ref, st = C.byref(d), ops.stream_ptr()

    def gather(first, n):
        d.first, d.n = first, n
        check(lib.satcv_scene_gather(ref, st))
        return dst[:n]
    return gather


def _series_buffers(plan, per_chip, nb, total, dtype, what):
    """(buf, short): the flat buffers the series gather fills, per_chip = steps * side * side * cpad elements a chip.  Without a plan one
    buffer of nb chips.  With a plan, full batches are gathered straight into its static input; a short last batch goes through a buffer
    of its own and is spread over a prefix of every time step by plan.run."""
    from . import ops
    td = ops.TORCH_DTYPE[dtype]
    if plan is None:
        return _device_empty((nb * per_chip,), td, what), None
    return plan.x_in.view(-1), (_device_empty(((total % nb) * per_chip,), td, what) if total % nb else None)


def _series_gatherer(src, kind, maxval, origins, off, side, steps, dtype, cpad, nb, buf, short):
    """-> gather(first, n): one satcv_series_gather of chips [first, first + n) of the resident stack `src` -- cut, normalised, ingested --
    into the buffers of `_series_buffers`; returns the time-major (steps * n, side, side, cpad) tensor a ConvLSTM model reads.  The
    descriptor is filled once, a launch sets `first`, `n` and the destination."""
    import ctypes as C
    from . import ops
    from ._lib import SeriesGatherDesc, check, lib
    T, C_, H, W = src.shape
    d = SeriesGatherDesc(src=src.data_ptr(), src_kind=kind, t=T, c=C_, h=H, w_=W, steps=steps, maxval=maxval, origins=origins.data_ptr(),
                         total=origins.shape[0], first=0, n=0, off=off, side=side, dst=None, dtype=dtype, cpad=cpad)
    ref, st = C.byref(d), ops.stream_ptr()

    def gather(first, n):
        xt = (buf if n == nb or short is None else short)[:steps * n * side * side * cpad].view(steps * n, side, side, cpad)      # (steps, n, ...) is contiguous for every n
        d.first, d.n, d.dst = first, n, xt.data_ptr()
        check(lib.satcv_series_gather(ref, st))
        return xt
    return gather


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


class _Maps:
    """The device-resident result of a scene predictor: `out` (H, W, nc) float32, channels [c0, c0 + nc) of the model's output, 0 where
    nothing is predicted; `cls` (H, W, 1) uint8, 255 there, or None.  `alloc` runs before the batch loop where the class count is known
    from the model, inside the first batch where only its output tells it (predict_chips_device takes any object with predict_on_device)."""
    out = cls = None

    def alloc(self, H, W, channel, ncls, want_classes):
        import torch
        self.c0, self.nc = _channel_range(channel, ncls)
        self.out = _device_empty((H, W, self.nc), torch.float32, 'the prediction map', 0.0)
        self.cls = _device_empty((H, W, 1), torch.uint8, 'the class map', 255) if want_classes else None

    def host(self, channel, device=False):
        """the one copy back: the (H, W) map of an int channel or (H, W, n_classes), with a class map the pair (map, (H, W) uint8).
        device=True: no copy, the same shapes as views of the CUDA tensors held here (what raster_tools.write_cog reads in place)"""
        probs = self.out if channel is None else self.out[..., 0]
        cls = None if self.cls is None else self.cls[..., 0]
        if not device:
            probs, cls = probs.cpu().numpy(), (None if cls is None else cls.cpu().numpy())
        return probs if cls is None else (probs, cls)


def _empty_result(H, W, channel, ncls, classes, device=False):
    """what a predictor returns for a scene too small for one reference chip: nothing is predicted"""
    if device:
        import torch
        probs = _device_empty((H, W) if channel is not None else (H, W, ncls), torch.float32, 'the prediction map', 0.0)
        return (probs, _device_empty((H, W), torch.uint8, 'the class map', 255)) if classes else probs
    probs = np.zeros((H, W) if channel is not None else (H, W, ncls), np.float32)
    return (probs, np.full((H, W), 255, np.uint8)) if classes else probs


def _stitch_batches(idx, origins, batch_size, kernel, off, maps, gather, forward):
    """The batch loop of the three scene predictors.  gather(first, n) launches the gathers of chips [first, first + n) and returns the
    model's inputs; forward(inputs, first, n) runs the model on them and returns (probs, classes or None) -- (n, side, side, k) and
    (n, side, side) tensors whose centres are scattered into `maps` here, one launch per run of pairwise disjoint chips -- or None where
    the model's head has stored the centres itself."""
    total = len(idx)
    crop = (off, off, kernel, kernel)
    # No host synchronisation inside this loop.  Every launch -- gather, the model's or the plan's kernels, scatter -- goes to the current
    # stream, so stream order alone keeps the gather of batch i + 1 from overwriting the chip buffers (and the model or the plan from
    # overwriting its output tensors) while batch i still reads them.
    for s in range(0, total, batch_size):
        n = min(batch_size, total - s)
        res = forward(gather(s, n), s, n)
        if res is None:
            continue
        for a, e in _disjoint_runs(idx[s:s + n], kernel, kernel):
            _scatter(res[0], a, e - a, crop, origins, total, s + a, maps.out, 0, maps.c0, maps.nc, True)
            if maps.cls is not None:
                _scatter(res[1], a, e - a, crop, origins, total, s + a, maps.cls, 0, 0, 1, False)
    return maps


def _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, channel, want_classes, rescale):
    """predict_chips_device / predict_scene on the device: -> _Maps.  channel: int, or None for every class.  A scene is a host array,
    or a contiguous float32 CUDA tensor (H, W, C) that is read where it lies."""
    import torch
    H, W = scenes[0].shape[:2]
    off = buff // 2
    side = kernel + 2 * off                  # the window of predict_chips; kernel + buff for an even buff
    dev = [_resident_scene(sc, rescale) for sc in scenes]
    origins = _origin_table(idx)
    nb = min(batch_size, len(idx))
    bufs = [_device_empty((nb, side, side, sc.shape[2]), torch.float32, 'the chip batch') for sc, _ in dev]
    gathers = [_scene_gatherer(sc, kind, rescale, origins, off, buf) for (sc, kind), buf in zip(dev, bufs)]
    maps = _Maps()

    def gather(first, n):
        return [g(first, n) for g in gathers]

    def forward(xs, first, n):
        res = m.predict_on_device(xs if len(xs) > 1 else xs[0])
        res = list(res) if isinstance(res, (list, tuple)) else [res]
        probs = res[0]
        if probs.dtype != torch.float32 or not probs.is_contiguous():
            probs = probs.to(torch.float32).contiguous()
        if maps.out is None:                 # (the class count is the model's to tell: known with its first output)
            _channel_range(channel, probs.shape[-1])
            if want_classes and (len(res) < 2 or res[1].dim() != 3):
                raise ValueError('classes=True needs a model with an (n, h, w) class output next to its probabilities')
            maps.alloc(H, W, channel, probs.shape[-1], want_classes)
        return probs, (res[1] if want_classes else None)
    return _stitch_batches(idx, origins, batch_size, kernel, off, maps, gather, forward)


def predict_chips_device(arr, chip_indices, template, m, kernel=256, buff=128, batch_size=16, channel=0, rescale=None, device=False):
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
    tensor (H, W, C), e.g. from `pc_tools.median_composite` -- is read in place.  An empty index list returns `template` untouched.
    device=True: nothing is copied back and `template` is neither read nor changed (it may be None): the return value is the (H, W)
    float32 CUDA map itself, the values `template` would receive, zero where no chip lands."""
    scenes, _ = _scenes(arr)
    _check_geometry(kernel, buff, batch_size)
    idx = [(int(y), int(x)) for y, x in chip_indices]
    if not idx:
        return _empty_result(scenes[0].shape[0], scenes[0].shape[1], 0, 1, False, True) if device else template
    if scenes[0].ndim != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {scenes[0].shape}')
    _check_windows(idx, scenes[0].shape[0], scenes[0].shape[1], kernel, buff // 2)
    maps = _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, int(channel), False, rescale)
    if device:
        return maps.host(int(channel), True)
    template += maps.host(int(channel))
    return template


def predict_scene(arr, m, kernel=256, buff=128, batch_size=16, channel=0, cover='reference', classes=False, rescale=None, device=False):
    """Prediction map of a whole (H, W, C) scene (or two-date pair of scenes), stitched on the device; returns new arrays.

    cover='reference': the chips of `generate_chip_indices` -- the buff // 2 border and a last chip ending on the image edge stay
    unpredicted (0 in the map, 255 in the class map), as in the reference.
    cover='full': centres on the grid range(0, H, kernel) x range(0, W, kernel); windows that overhang the scene are filled by
    reflection (np.pad mode='reflect') inside the gather and the centres are clipped to the scene, so every pixel is predicted exactly
    once.  Needs H, W >= kernel + buff (one reflection then suffices), else ValueError.
    channel: int -> (H, W) float32; None -> (H, W, n_classes).  classes=True returns (map, class map (H, W) uint8) from the model's
    second output (ValueError for a single-output model).  The returned arrays are the only device-to-host traffic.  A scene may be a
    contiguous float32 CUDA tensor (H, W, C), read in place.
    device=True: nothing is copied back; the same shapes come as CUDA tensors (float32 map, uint8 class map with 255 where nothing is
    predicted -- the nodata of `raster_tools.write_cog`, which reads them where they lie)."""
    scenes, _ = _scenes(arr)
    _check_geometry(kernel, buff, batch_size)
    if scenes[0].ndim != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {scenes[0].shape}')
    H, W = scenes[0].shape[:2]
    idx = _cover_indices(H, W, kernel, buff, cover, kernel + buff, 'kernel + buff')
    if classes and len(getattr(m, 'outputs', ())) < 2:
        raise ValueError('classes=True needs a model with a class output next to its probabilities')
    if not idx:
        return _empty_result(H, W, channel, m.outputs[0].channels, classes, device)
    channel = None if channel is None else int(channel)
    return _stitch_on_device(scenes, idx, m, kernel, buff, batch_size, channel, classes, rescale).host(channel, device)


def predict_raster(in_file, m, out_file, window=None, cog_options=None, **predict_scene_kwargs):
    """File to file: `raster_tools.read_cog` -> `predict_scene(..., device=True)` -> `raster_tools.write_cog`, the pixels never on the host
    uncompressed; returns what `predict_scene` returns (CUDA tensors).

    in_file: a GeoTIFF / COG `read_cog` reads; window: (row0, col0, h, w) of it, None: all.  The scene is predicted in float32: an integer
    file is cast on the device (satcv_raster_convert, exact for 8- and 16-bit samples).  out_file: the prediction map (the first result of
    `predict_scene`) as a Cloud-Optimized GeoTIFF that carries the source's transform -- of the window -- and CRS; cog_options: a dict of
    further `write_cog` arguments (dtype, scale, nodata, compress, ...).  predict_scene_kwargs: kernel, buff, batch_size, channel, cover,
    classes, rescale.  ValueError when the file carries no transform or no EPSG code."""
    from . import raster_tools as rt
    if 'device' in predict_scene_kwargs:
        raise ValueError('predict_raster keeps the scene and the map on the device: device is not an argument')
    r = rt.read_cog(in_file, window=window, layout='hwc', device=True)
    if r.transform is None or r.crs is None:
        raise ValueError(f'{in_file} carries no transform or no EPSG code: the output cannot be georeferenced')
    scene = r.array if r.dtype == 'float32' else rt.to_float32(r.array, r.dtype, what='the float32 scene', as_raster=True)
    res = predict_scene(scene, m, device=True, **predict_scene_kwargs)
    rt.write_cog(res[0] if isinstance(res, tuple) else res, out_file, r.transform, r.crs, **dict(cog_options or {}))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# Scene prediction for the ConvLSTM2D time-series models (lstm_tools.LSTMModel / LSTMAutoencoder): the (T, C, H, W) stack goes to the
# device once, satcv_series_gather cuts, normalises and ingests a chip batch in one launch, the model reads the result in place
# (predict_on_device(..., shape=...)) and satcv_scene_scatter stitches the centres.  DESIGN.md, "Scene prediction for the time-series
# models".
def predict_series_scene(stack, m, kernel=256, buff=128, batch_size=16, channel=0, cover='reference', classes=False, maxval=10000,
                         harmonics=None, plan=None, device=False):
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
    `predict_hybrid_scene`.  device=True: as for `predict_scene`, the results stay on the device."""
    from .lstm_tools import LSTMAutoencoder
    _check_geometry(kernel, buff, batch_size)
    _, H, W = _check_stack(stack, m)
    maxval = _check_maxval(maxval)
    idx = _cover_indices(H, W, kernel, buff, cover, kernel + buff, 'kernel + buff')
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
    if not idx:
        return _empty_result(H, W, channel, m.n_classes, classes, device)
    channel = None if channel is None else int(channel)
    _channel_range(channel, m.n_classes)
    side = kernel + 2 * (buff // 2)
    want = (min(batch_size, len(idx)), m.n_time, side, side)
    plan = _resolve_plan(plan, m, want, lambda: m.inference_plan(want), 'SeriesInferPlan', 'shape')
    return _stitch_series(stack, idx, m, kernel, buff, batch_size, channel, classes, maxval, harmonics, plan).host(channel, device)


def _stitch_series(stack, idx, m, kernel, buff, batch_size, channel, want_classes, maxval, harmonics, plan=None):
    """predict_series_scene on the device: -> _Maps"""
    import torch
    from . import ops
    _, C_, H, W = stack.shape
    steps, off = m.n_time, buff // 2
    side = kernel + 2 * off
    dev, kind = _resident_stack(stack, steps, '(T, C, H, W)')
    origins = _origin_table(idx)
    total = len(idx)
    nb = min(batch_size, total)
    cpad, dtype = ops.rup(C_, 16), m.dtype_code
    buf, short = _series_buffers(plan, steps * side * side * cpad, nb, total, dtype, 'the chip batch')
    sincos = None
    if harmonics is not None:
        sincos = _device_empty((nb, side, side, 2), torch.float32, 'the harmonics')
        sincos[..., 0] = harmonics[0]
        sincos[..., 1] = harmonics[1]
    maps = _Maps()
    maps.alloc(H, W, channel, m.n_classes, want_classes)

    gather = _series_gatherer(dev, kind, maxval, origins, off, side, steps, dtype, cpad, nb, buf, short)

    def forward(xt, first, n):
        try:
            if plan is not None:
                res = plan.run(xt if sincos is None else [xt, sincos[:n]], want_classes=want_classes)
                return res if want_classes else (res, None)
            if sincos is not None:
                return m.predict_on_device([xt, sincos[:n]], shape=(n, steps, side, side)), None
            if want_classes:
                return m.predict_on_device(xt, shape=(n, steps, side, side), want_classes=True)
            return m.predict_on_device(xt, shape=(n, steps, side, side)), None
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f'a batch of {n} chips of {steps} x {side} x {side} does not fit in device memory; lower batch_size') from e
    return _stitch_batches(idx, origins, batch_size, kernel, off, maps, gather, forward)


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
    idx = _cover_indices(H, W, kernel, buff, cover, side, 'side')
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
                         maxval=10000, output=None, plan=None, device=False):
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
    them into the map.  The returned arrays are the only device-to-host traffic.  device=True: as for `predict_scene`, the results stay
    on the device."""
    import torch
    from .lstm_tools import HierarchicalModel
    head, multiple = _hybrid_head(m, output)
    _check_geometry(kernel, buff, batch_size)
    if getattr(scene, 'ndim', None) != 3:
        raise ValueError(f'expected an (H, W, C) scene, got shape {tuple(getattr(scene, "shape", ()))}')
    H, W, C_ = (int(v) for v in scene.shape)
    if C_ != m.hi_channels:
        raise ValueError(f'the model reads {m.hi_channels} fine bands, the scene holds {C_}')
    _, h, w = _check_stack(stack, m, '(T, c, h, w)', 'coarse bands')
    maxval = _check_maxval(maxval)
    hi, lo, geo = hybrid_chip_tables((H, W), (h, w), kernel, buff, cover, multiple)
    ncls = head.cout
    if classes and head.activation != head.ACT['softmax']:
        raise ValueError(f'classes=True needs a head with a class output (softmax); {head.name!r} has none')
    channel = None if channel is None else int(channel)
    _channel_range(channel, ncls)
    if plan is not None and plan is not False and isinstance(m, HierarchicalModel):
        raise NotImplementedError('plan: HybridInferPlan covers HybridModel; the ACNN trunk of a HierarchicalModel lives on the tape')
    if not len(hi):
        return _empty_result(H, W, channel, ncls, classes, device)
    want = (min(int(batch_size), len(hi)), geo['side'], geo['side_lo'])

    def build():
        try:
            return m.scene_plan(*want)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f'a HybridInferPlan for (batch, side, side_lo) = {want} does not fit in device memory; lower batch_size') from e
    plan = _resolve_plan(plan, m, want, build, 'HybridInferPlan', '(batch, side, side_lo) =')
    return _stitch_hybrid(scene, stack, hi, lo, geo, m, head, output, int(kernel), int(batch_size), channel, bool(classes), rescale, maxval,
                          plan).host(channel, device)


def _model_ratio(m):
    """the resolution ratio r a two-resolution model was built for: the side of its fine input over the side of its coarse input"""
    hi_dim = getattr(m, 'unet_dim', None) or getattr(m, 'acnn_dim', None)
    if hi_dim is None or not hasattr(m, 'lstm_dim'):
        raise ValueError(f'predict_hybrid_raster covers HybridModel and HierarchicalModel, got {type(m).__name__}')
    side, side_lo = int(hi_dim[0]), int(m.lstm_dim[1])
    if side_lo < 1 or side % side_lo:
        raise ValueError(f'the fine input side {side} of the model is not a multiple of its coarse input side {side_lo}')
    return side // side_lo


def predict_hybrid_raster(scene_file, stack_items, m, out_file, window=None, resampling='nearest', cog_options=None, reproject=False, **kwargs):
    """File to file for the two-resolution models: a fine scene file and the files of a coarse time series that need not share its
    grid -> `predict_hybrid_scene(..., device=True)` -> a Cloud-Optimized GeoTIFF; returns what `predict_hybrid_scene` returns (CUDA
    tensors).

    scene_file: a GeoTIFF / COG; window: (row0, col0, h, w) of it, None: all.  The fine grid is that of the file (of the window).  The
    coarse grid has the same bounds with pixels r times larger, r being the ratio the model was built for (fine input side / coarse
    input side); stack_items (per acquisition a path or a list of paths, as for `raster_tools.read_aligned_stack`) are resampled onto it
    with `resampling`.  A fine extent that is not a multiple of r is a ValueError: cut the window, or trim the scene as
    `pc_tools.trim_array` does.  out_file carries the scene file's transform -- of the window -- and CRS; cog_options: further `write_cog`
    arguments.  kwargs: the other arguments of `predict_hybrid_scene` (kernel, buff, batch_size, channel, cover, classes, rescale,
    maxval, output, plan).  reproject=True: the series may be in another EPSG code than the scene (a 10 m Sentinel series in 326xx beside
    a NAIP scene in 269xx): it is reprojected onto the coarse grid (`raster_tools.read_warped(reproject=True)`)."""
    import torch
    from . import raster_tools as rt
    if 'device' in kwargs:
        raise ValueError('predict_hybrid_raster keeps the scene, the stack and the map on the device: device is not an argument')
    r = _model_ratio(m)
    info = rt.read_info(scene_file)[0]
    if info.transform is None or info.crs is None:
        raise ValueError(f'{scene_file} carries no transform or no EPSG code: the output cannot be georeferenced')
    (row0, col0, h, w), transform = rt.level_window(info, window)
    if h % r or w % r:
        raise ValueError(f'the fine extent {h} x {w} is not a multiple of the resolution ratio r = {r}: choose a window that is, or trim the scene '
                         f'(pc_tools.trim_array(arr, {r}))')
    fine = rt.Grid(transform, (h, w), info.crs)
    a, _, c, _, e, f = fine.transform
    coarse = rt.Grid((a * r, 0.0, c, 0.0, e * r, f), (h // r, w // r), info.crs)
    scene = rt.read_cog(scene_file, window=(row0, col0, h, w), layout='hwc', device=True)
    stack = rt.read_aligned_stack(stack_items, coarse, resampling=resampling, reproject=reproject)[0]
    fine_scene = scene.array if scene.dtype == 'float32' else rt.to_float32(scene.array, scene.dtype)
    if stack.dtype not in (torch.int16, torch.float32):       # (the series gather reads int16 and float32)
        stack = rt.to_float32(stack, rt.read_info(_first_path(stack_items))[0].dtype)
    res = predict_hybrid_scene(fine_scene, stack, m, device=True, **kwargs)
    rt.write_cog(res[0] if isinstance(res, tuple) else res, out_file, fine.transform, fine.crs, **dict(cog_options or {}))
    return res


def get_img_bounds(img, jsonFile, dst_crs=None):
    """utils/prediction_tools.py:560-600: the corner coordinates of an image, for a map viewer.  img: a two-dimensional array, placed by
    the mixer's transform, or the path of a GeoTIFF, whose own bounds are taken (`raster_tools.read_info`).  jsonFile: the mixer JSON
    of the export ('projection': 'affine': 'doubleMatrix' and 'crs').  dst_crs: the bounds are taken to it with
    `raster_tools.transform_bounds(..., densify_pts=21)` as the reference does with rasterio's (no datum shift between WGS84 and NAD83).
    -> [[lat_min, lon_min], [lat_max, lon_max]], i.e. [[bottom, left], [top, right]]."""
    import json
    import os
    from . import raster_tools as rt
    with open(jsonFile) as f:
        mixer = json.load(f)
    src_crs = mixer['projection']['crs']
    if isinstance(img, (str, os.PathLike)):
        info = rt.read_info(img)[0]
        if info.transform is None:
            raise ValueError(f'{img} carries no transform')
        left, bottom, right, top = rt.Grid(info.transform, info.shape).bounds
    else:
        shape = tuple(getattr(img, 'shape', ()))
        if len(shape) != 2:
            raise ValueError(f'expected an (H, W) array or the path of a GeoTIFF, got shape {shape}')
        left, bottom, right, top = rt.Grid(tuple(mixer['projection']['affine']['doubleMatrix'][:6]), shape).bounds
    if dst_crs:
        left, bottom, right, top = rt.transform_bounds(src_crs, dst_crs, left=left, bottom=bottom, right=right, top=top, densify_pts=21)
    return [[bottom, left], [top, right]]


def _first_path(items):
    import os
    first = list(items)[0]
    return first if isinstance(first, (str, os.PathLike)) else list(first)[0]


def _stitch_hybrid(scene, stack, hi, lo, geo, m, head, output, kernel, batch_size, channel, want_classes, rescale, maxval, plan):
    """predict_hybrid_scene on the device: -> _Maps"""
    import ctypes as C
    import torch
    from . import ops
    from ._lib import DenseSceneDesc, check, lib
    from .lstm_tools import HybridModel
    H, W, C_ = scene.shape
    steps, off, side, off_lo, side_lo = m.n_time, geo['off'], geo['side'], geo['off_lo'], geo['side_lo']
    sdev, skind = _resident_scene(scene, rescale)
    tdev, tkind = _resident_stack(stack, steps, '(T, c, h, w)')
    total = len(hi)
    org_hi, org_lo = _origin_table(hi), _origin_table(lo)
    nb = min(batch_size, total)
    cpad, dtype = ops.rup(stack.shape[1], 16), m.dtype_code
    buf_hi = _device_empty((nb, side, side, C_), torch.float32, 'the fine chip batch')
    buf_lo, short = _series_buffers(plan, steps * side_lo * side_lo * cpad, nb, total, dtype, 'the coarse chip batch')
    maps = _Maps()
    maps.alloc(H, W, channel, head.cout, want_classes)
    kw = {} if isinstance(m, HybridModel) else {'output': output or 'lstm_probs'}
    st = ops.stream_ptr()

    gather_hi = _scene_gatherer(sdev, skind, rescale, org_hi, off, buf_hi)
    gather_lo = _series_gatherer(tdev, tkind, maxval, org_lo, off_lo, side_lo, steps, dtype, cpad, nb, buf_lo, short)

    def gather(first, n):
        return [gather_hi(first, n), gather_lo(first, n)]

    def forward(xs, first, n):
        """the model up to its last dense layer; that layer runs in `scene_head`, so nothing is left to scatter.  The windows of both
        covers are pairwise disjoint, so one head launch per batch meets the kernel's contract."""
        def scene_head(d):
            """the model's last dense layer (its sources in `d`) on the chip centres, stored into the map"""
            sd = DenseSceneDesc(head=d, crop_y=off, crop_x=off, crop_h=kernel, crop_w=kernel, origins=org_hi.data_ptr(), total=total, first=first,
                                map=maps.out.data_ptr(), map_h=H, map_w=W, ldm=maps.nc, c0=maps.c0, nc=maps.nc,
                                class_map=maps.cls.data_ptr() if maps.cls is not None else None)
            check(lib.satcv_dense_scene_fwd(C.byref(sd), st))
        try:
            if plan is not None:
                plan.run(*xs, scene_head=scene_head)
            else:
                m.predict_on_device(xs, shape=(n, steps, side_lo, side_lo), scene_head=scene_head, **kw)
        except torch.cuda.OutOfMemoryError as e:
            raise MemoryError(f'a batch of {n} chips of {side} x {side} and {steps} x {side_lo} x {side_lo} does not fit in device memory; lower batch_size') from e
    return _stitch_batches(hi, org_hi, batch_size, kernel, off, maps, gather, forward)


def _device_mosaic(imageDataset, model, patches, cols, channel, grid_of):
    """The batch loop of `callback_predictions`: predict `patches` patches and place the kept window of channel `channel` of each into a
    device-resident (rows, columns, 1) float32 mosaic, which is returned.  grid_of(patch_hw) -> (crop, origins, mosaic_hw) as
    `_patch_grid` returns them.  The patches are cropped and placed on the device by the scatter kernel."""
    import torch
    from .model_tools import _as_batches
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
            if probs.shape[-1] <= channel:
                raise ValueError(f'the mosaic holds output channel {channel}: the model has {probs.shape[-1]} output channel(s)')
            grid, place, hw = grid_of(probs.shape[1:3])
            origins = _origin_table(place)
            mosaic = _device_empty(tuple(hw) + (1,), torch.float32, 'the mosaic', 0.0)
        n = min(probs.shape[0], len(place) - filled)
        _scatter(probs, 0, n, grid, origins, len(place), filled, mosaic, 0, channel, 1, False)
        filled += n
        if filled >= len(place):
            break
    if grid is None or filled < len(place):
        raise ValueError(f'the dataset ended after {filled} patches, mixer announces {patches}')
    return mosaic


def callback_predictions(imageDataset, model, mixer, kernel_shape=[256, 256], kernel_buffer=[128, 128]):
    """utils/prediction_tools.py:245-291 without its prints: predict mixer['totalPatches'] patches, keep the probability of class 1 and
    assemble the cropped patches into a mosaic of mixer['patchesPerRow'] patches per row; returns the (rows, columns) float32 mosaic.

    The crop and the placement are those of `_patch_grid` (as coded in the reference: each axis starts at its own half buffer and stops
    at its kernel size plus the OTHER axis' half buffer; patch i lands at mosaic row i // patchesPerRow, column i % patchesPerRow; a
    trailing partial row is dropped).  imageDataset: an (N, h, w, c) array or an iterable of batches.  The patches are cropped and
    placed on the device by the scatter kernel; the mosaic is the only copy back."""
    patches, cols = int(mixer['totalPatches']), int(mixer['patchesPerRow'])
    mosaic = _device_mosaic(imageDataset, model, patches, cols, 1, lambda hw: _patch_grid(patches, cols, hw, kernel_shape, kernel_buffer))
    return mosaic[..., 0].cpu().numpy()


def _mixer_georeference(jsonFile):
    """(mixer dict, transform (a, b, c, d, e, f), crs) of an Earth-Engine mixer file: projection.affine.doubleMatrix and projection.crs"""
    import json
    with open(jsonFile) as file:
        mixer = json.load(file)
    transform = tuple(float(v) for v in mixer['projection']['affine']['doubleMatrix'][0:6])
    return mixer, transform, mixer['projection']['crs']


def _plain_blocksize(H, W):
    return min(512, -(-max(int(H), int(W)) // 16) * 16)


def write_geotiff_prediction(image, jsonFile, aoi):
    """utils/prediction_tools.py:447-472: write `image` -- (H, W) or (H, W, C), a host array or a CUDA tensor -- as f'{aoi}.tif' with the
    georeference of the Earth-Engine mixer file `jsonFile`: uncompressed, no overviews, no nodata tag, in the image's own dtype (float64
    becomes float32), as rasterio's defaults give it there.  The file is tiled where the reference's is written in strips; readers do
    not care.  Returns the path."""
    from . import raster_tools as rt
    _, transform, crs = _mixer_georeference(jsonFile)
    H, W = image.shape[:2]
    return rt.write_cog(image, f'{aoi}.tif', transform, crs, nodata=None, compress=None, overviews=0, blocksize=_plain_blocksize(H, W))


def write_geotiff_predictions(imageDataset, model, jsonFile, outImgBase, outImgPath, kernel_buffer=[128, 128]):
    """utils/prediction_tools.py:475-536 without its prints: predict the mixer's totalPatches patches, keep output channel 0 of each
    without its buffer (rows y_buffer : y_buffer + patchDimensions[0], columns x_buffer : x_buffer + patchDimensions[1], :520), place patch
    i at row i // patchesPerRow, column i % patchesPerRow of a float32 mosaic, and write it as join(outImgPath, f'{outImgBase}.tif') with
    the mixer's georeference -- uncompressed and without overviews, as `write_geotiff_prediction`.  The mosaic is assembled on the
    device by the scatter kernel of `callback_predictions` and written from there; returns the path.
    (Where the reference calls `model.predict` once per patch, the patches run in batches.)"""
    from os.path import join
    from . import raster_tools as rt
    mixer, transform, crs = _mixer_georeference(jsonFile)
    cols, patches = int(mixer['patchesPerRow']), int(mixer['totalPatches'])
    rows = int(patches / cols)
    kh, kw = (int(v) for v in mixer['patchDimensions'][:2])
    x_buffer, y_buffer = int(kernel_buffer[0] / 2), int(kernel_buffer[1] / 2)
    if cols < 1 or rows < 1:
        raise ValueError(f'totalPatches={patches} does not fill one mosaic row of patchesPerRow={cols}')

    def grid_of(patch_hw):
        if y_buffer + kh > patch_hw[0] or x_buffer + kw > patch_hw[1]:
            raise ValueError(f'a {patch_hw[0]} x {patch_hw[1]} patch does not hold patchDimensions {kh} x {kw} behind buffers {y_buffer}, {x_buffer}')
        return (y_buffer, x_buffer, kh, kw), [((i // cols) * kh, (i % cols) * kw) for i in range(rows * cols)], (rows * kh, cols * kw)
    mosaic = _device_mosaic(imageDataset, model, rows * cols, cols, 0, grid_of)
    out_image_file = join(outImgPath, f'{outImgBase}.tif')
    return rt.write_cog(mosaic, out_image_file, transform, crs, nodata=None, compress=None, overviews=0, blocksize=_plain_blocksize(rows * kh, cols * kw))
