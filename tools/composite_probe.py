"""GPU probe: satcv_median_composite on uint16 stacks of one Sentinel-2 tile (10 980 x 10 980, 4 bands) at t = 6, 12, 24 acquisitions and
on a 2 048 x 2 048 stack; --quick runs the small one only.

Per configuration: kernel time (3 warm-up launches, then the median of `--reps` launches timed one by one with device events), its
rate over the ALGORITHMIC bytes (t c h w sizeof(S) read, 4 c h w written per output, both outputs on), the streaming rate of the same
box in the same run (a device-to-device copy that moves the same number of bytes, read + written, timed the same way) and the
ratio of the two.  The only baseline a new capability has is the host: np.nanmedian + the normalisation of the 2 048 x 2 048 stack
(NumPy's nan-reductions are single-threaded; the probe does not pin anything).

    python tools/composite_probe.py [--quick] [--reps 9] > profiles/composite_probe.txt"""
import argparse
import ctypes as C
import os
import socket
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from satellite_computervision_amd import ops
from satellite_computervision_amd._lib import CompositeDesc, check, lib


def event_times(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(out)), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--no-host', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures on the GPU only'
    p = torch.cuda.get_device_properties(0)
    print(f'box {socket.gethostname()}: {p.name}, {p.multi_processor_count} CUs, {p.total_memory / 2 ** 30:.0f} GiB; torch {torch.__version__}; reps {a.reps} (median [min, max])')
    configs = [(2048, 12)] if a.quick else [(2048, 6), (2048, 12), (2048, 24), (10980, 6), (10980, 12), (10980, 24)]
    c = 4
    small = None
    for side, t in configs:
        g = torch.Generator(device='cuda').manual_seed(side + t)
        stack = torch.randint(1, 12000, (t, c, side, side), generator=g, device='cuda', dtype=torch.int16)
        stack[torch.rand(stack.shape, generator=g, device='cuda') < 0.3] = 0                      # ~30 % nodata
        offsets = torch.tensor([0.0] * (t // 2) + [1000.0] * (t - t // 2), device='cuda')
        med = torch.empty((side, side, c), dtype=torch.float32, device='cuda')
        nrm = torch.empty((side, side, c), dtype=torch.float32, device='cuda')
        d = CompositeDesc(src=stack.data_ptr(), src_kind=1, t=t, c=c, h=side, w_=side, offsets=offsets.data_ptr(), median=med.data_ptr(), ld_med=c,
                          coff_med=0, norm=nrm.data_ptr(), ld_norm=c, coff_norm=0, use_fill=0, fill=0.0)
        st = ops.stream_ptr()
        tk = event_times(lambda: check(lib.satcv_median_composite(C.byref(d), st)), a.reps)
        nbytes = stack.numel() * 2 + 2 * med.numel() * 4
        half = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
        dst = torch.empty_like(half)
        tc = event_times(lambda: dst.copy_(half), a.reps)
        del half, dst
        rk, rc = nbytes / tk[0] / 1e12, nbytes / tc[0] / 1e12
        print(f'u16 {side:5d}^2 x {c} bands, t = {t:2d}: {nbytes / 1e9:7.2f} GB | kernel {tk[0] * 1e3:8.3f} ms [{tk[1] * 1e3:.3f}, {tk[2] * 1e3:.3f}] = {rk:5.2f} TB/s | '
              f'copy of equal volume {tc[0] * 1e3:8.3f} ms [{tc[1] * 1e3:.3f}, {tc[2] * 1e3:.3f}] = {rc:5.2f} TB/s | kernel / streaming = {rk / rc:.2f}', flush=True)
        if side == 2048 and t == 12:
            small = (stack.cpu().numpy().view(np.uint16), offsets.cpu().numpy(), tk[0])
        del stack, med, nrm
    if small is not None and not a.no_host:
        s, off, tk = small
        warnings.simplefilter('ignore', RuntimeWarning)          # (all-NaN pixels are part of the data)
        t0 = time.perf_counter()
        x = s.astype(np.float64)
        x = np.where(x > 0, x, np.nan)
        o = off.reshape(-1, 1, 1, 1)
        x = np.where(o > 0, np.clip(x, o, None) - o, x)
        m = np.nanmedian(x, axis=0)
        n = (m - np.nanmean(m, axis=0)) / (np.nanstd(m, axis=0) + 1e-6)
        th = time.perf_counter() - t0
        print(f'host baseline, 2048^2 x 4 bands, t = 12 (NumPy float64: where / clip / nanmedian / nanmean / nanstd): {th:.2f} s = {th / tk:.0f} x the kernel', flush=True)


if __name__ == '__main__':
    main()
