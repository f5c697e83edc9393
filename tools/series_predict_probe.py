"""GPU probe: scene prediction of get_lstm_model(6, 3, 6) over a synthetic int16 time stack (T = 6, C = 6, 1024 x 1024; kernel 32, buff 32:
900 reference chips of 64^2, batch 64) -- prediction_tools.predict_series_scene (stack and map resident on the device) against the host
loop it replaces (windows cut and moved in NumPy, normalize_timeseries, LSTMModel.predict per batch, centres stitched in NumPy), and
the device time of satcv_series_gather for one full batch (HIP events around back-to-back launches).  Interleaved: every round times
each variant once, after one warm-up round; median and min-max over the rounds.  No thresholds: the output is the record."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from satellite_computervision_amd import lstm_tools as lt, model_tools as mt, ops, prediction_tools as pt, processing
from satellite_computervision_amd._lib import SeriesGatherDesc, check, lib

ROUNDS = int(os.environ.get('SERIES_PROBE_ROUNDS', '7'))
T, NB, S, KERNEL, BUFF, BATCH, MAXVAL = 6, 6, 1024, 32, 32, 64, 10000
OFF, SIDE = BUFF // 2, KERNEL + BUFF
GATHER_LAUNCHES = 50
rng = np.random.default_rng(0)
stack = (rng.beta(2, 5, (T, NB, S, S)) * 10000).astype(np.int16)
idx = pt.generate_chip_indices(np.empty((S, S, 0)), BUFF, KERNEL)
mt.set_seed(0)
m = lt.get_lstm_model(NB, 3, T)
m.compute_dtype = 'bfloat16'


def host_loop():
    out = np.zeros((S, S), np.float32)
    for s in range(0, len(idx), BATCH):
        part = idx[s:s + BATCH]
        cut = np.stack([stack[:, :, y - OFF:y + KERNEL + OFF, x - OFF:x + KERNEL + OFF] for y, x in part])        # (n, T, C, side, side)
        x = processing.normalize_timeseries(np.moveaxis(cut, 2, 4), maxval=MAXVAL).astype(np.float32)
        p = m.predict(x, batch_size=len(part))
        for k, (y, x_) in enumerate(part):
            out[y:y + KERNEL, x_:x_ + KERNEL] += p[k, OFF:OFF + KERNEL, OFF:OFF + KERNEL, 0]
    return out


def device_path():
    return pt.predict_series_scene(stack, m, KERNEL, BUFF, BATCH, channel=0, cover='reference', maxval=MAXVAL)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def gather_ms():
    """device time of one satcv_series_gather launch of a full batch, bf16 destination"""
    dev = torch.from_numpy(stack).cuda()
    org = torch.from_numpy(np.asarray(idx, np.int32)).cuda()
    cpad = ops.rup(NB, 16)
    dst = torch.empty(T * BATCH * SIDE * SIDE * cpad, dtype=torch.bfloat16, device='cuda')
    d = SeriesGatherDesc(src=dev.data_ptr(), src_kind=3, t=T, c=NB, h=S, w_=S, steps=T, maxval=float(MAXVAL), origins=org.data_ptr(), total=len(idx),
                         first=0, n=BATCH, off=OFF, side=SIDE, dst=dst.data_ptr(), dtype=m.dtype_code, cpad=cpad)
    st = ops.stream_ptr()
    out = []
    for r in range(ROUNDS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(GATHER_LAUNCHES):
            d.first = (i * BATCH) % (len(idx) - BATCH)
            check(lib.satcv_series_gather(C.byref(d), st))
        b.record()
        torch.cuda.synchronize()
        if r:
            out.append(a.elapsed_time(b) / GATHER_LAUNCHES)
    return out


def line(name, t, unit_ms=1e3):
    med = float(np.median(t))
    return (f'  {name:28s} median {med * unit_ms:9.3f} ms   min-max {min(t) * unit_ms:9.3f} - {max(t) * unit_ms:9.3f} ms   '
            f'spread {(max(t) - min(t)) / med * 100:5.1f} %')


batches = (len(idx) + BATCH - 1) // BATCH
print(f'stack int16 ({T}, {NB}, {S}, {S}), get_lstm_model({NB}, 3, {T}) bf16, kernel {KERNEL}, buff {BUFF}: {len(idx)} reference chips of {SIDE}^2 in '
      f'{batches} batches of {BATCH}; one warm-up round, then {ROUNDS} interleaved rounds', flush=True)
variants = {'predict_series_scene': device_path, 'host loop (LSTMModel.predict)': host_loop}
times, results = {v: [] for v in variants}, {}
for r in range(ROUNDS + 1):
    for v, fn in variants.items():
        t, results[v] = timed(fn)
        if r:
            times[v].append(t)
equal = np.array_equal(results['predict_series_scene'], results['host loop (LSTMModel.predict)'])
print('wall time of one whole scene (host clock around the call, device synchronised before and after):', flush=True)
for v in variants:
    print(line(v, times[v]), flush=True)
md, mh = (float(np.median(times[v])) for v in variants)
print(f'  maps equal: {equal}; the host loop takes {mh / md:.2f}x the time of predict_series_scene (medians), {len(idx) / md:.0f} against {len(idx) / mh:.0f} chips/s', flush=True)
g = gather_ms()
nbytes = T * BATCH * SIDE * SIDE * (NB * 2 + ops.rup(NB, 16) * 2)
print(f'satcv_series_gather, one full batch ({GATHER_LAUNCHES} back-to-back launches between two HIP events, per launch):', flush=True)
print(line('series_gather_kernel<i16,bf16>', [v * 1e-3 for v in g]), flush=True)
print(f'  bytes of a full batch: {T} * {BATCH} * {SIDE}^2 * ({NB} * 2 read + {ops.rup(NB, 16)} * 2 written) = {nbytes / 1e6:.1f} MB -> '
      f'{nbytes / (float(np.median(g)) * 1e-3) / 1e12:.2f} TB/s at the median; {batches} launches per scene = '
      f'{float(np.median(g)) * batches:.3f} ms of {md * 1e3:.1f} ms', flush=True)
