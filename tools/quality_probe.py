"""GPU probe: satcv_quality_mask and satcv_median_composite_masked on uint16 stacks of one Sentinel-2 tile (10 980 x 10 980) with 14 planes
per acquisition, t = 8 and 24; --quick runs 2 048 x 2 048 only.

Per depth, timed A / B / A / B on one box (3 warm-up launches, then the median of `--reps` launches timed one by one with device events):
  mask     the 'toa' rules (QA60 | CLOUD: 8 of the 14 planes are read), clear bit-planes out
  A        the existing satcv_median_composite of a separate 4-plane stack (B2, B3, B4, B8)
  B        satcv_median_composite_masked of the same 4-plane stack under the 'toa' mask
  B idx    the same composite read out of the 14-plane stack through band_idx (no copy of the planes)
  B ones   B under a mask of all ones: against A it shows what the mask costs beyond its own traffic
Each line gives the ALGORITHMIC bytes (planes read + outputs written; the masked composite reads 4 bytes per pixel and 32 acquisitions
more), the rate over them, and the rate of a device-to-device copy of the same volume in the same run.

    python tools/quality_probe.py [--quick] [--reps 9] > profiles/quality_probe.txt"""
import argparse
import ctypes as C
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from satellite_computervision_amd import ee_tools, ops
from satellite_computervision_amd._lib import CompositeDesc, CompositeMaskedDesc, QualityDesc, check, lib

BANDS = ['B1', 'B2', 'B3', 'B4', 'B5', 'B6', 'B7', 'B8', 'B8A', 'B10', 'B11', 'B12', 'QA60', 'SCL']
SEL = [1, 2, 3, 7]


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


def copy_rate(nbytes, reps):
    half = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(half)
    tc = event_times(lambda: dst.copy_(half), reps)
    return nbytes / tc[0] / 1e12


def line(name, nbytes, tk, rc):
    rk = nbytes / tk[0] / 1e12
    print(f'  {name:<8s} {nbytes / 1e9:7.2f} GB | {tk[0] * 1e3:8.3f} ms [{tk[1] * 1e3:.3f}, {tk[2] * 1e3:.3f}] = {rk:5.2f} TB/s | copy of equal volume {rc:5.2f} TB/s | '
          f'kernel / streaming = {rk / rc:.2f}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures on the GPU only'
    p = torch.cuda.get_device_properties(0)
    print(f'box {socket.gethostname()}: {p.name}, {p.multi_processor_count} CUs, {p.total_memory / 2 ** 30:.0f} GiB; torch {torch.__version__}; reps {a.reps} (median [min, max])')
    side = 2048 if a.quick else 10980
    cs, c = len(BANDS), len(SEL)
    st = ops.stream_ptr()
    for t in (8, 24):
        g = torch.Generator(device='cuda').manual_seed(side + t)
        stack = torch.empty((t, cs, side, side), device='cuda', dtype=torch.int16)
        for j in range(t):                                      # per acquisition: the random draws stay small next to the stack
            stack[j] = torch.randint(1, 6000, (cs, side, side), generator=g, device='cuda', dtype=torch.int16)
            stack[j][torch.rand((cs, side, side), generator=g, device='cuda') < 0.2] = 0           # ~20 % nodata
            stack[j, BANDS.index('QA60')] = torch.where(torch.rand((side, side), generator=g, device='cuda') < 0.1, 1024, 0).to(torch.int16)
        sub = stack[:, SEL].contiguous()
        offsets = torch.tensor([0.0] * (t // 2) + [1000.0] * (t - t // 2), device='cuda')
        npix, nw = side * side, (t + 31) // 32
        words = torch.empty((nw, side, side), dtype=torch.int32, device='cuda')
        ones = torch.full((nw, side, side), -1, dtype=torch.int32, device='cuda')
        med = torch.empty((side, side, c), dtype=torch.float32, device='cuda')
        nrm = torch.empty((side, side, c), dtype=torch.float32, device='cuda')
        q = QualityDesc(src=stack.data_ptr(), src_kind=1, t=t, cs=cs, h=side, w_=side, offsets=offsets.data_ptr(),
                        band=(C.c_int32 * 10)(*ee_tools.band_table(BANDS)), rules=ee_tools.PRESETS['toa'], cloud_max=15, shadow_min=900.0,
                        clear=words.data_ptr(), cloud_score=None, water_score=None)

        def comp(src):
            return CompositeDesc(src=src.data_ptr(), src_kind=1, t=t, c=c, h=side, w_=side, offsets=offsets.data_ptr(), median=med.data_ptr(), ld_med=c,
                                 coff_med=0, norm=nrm.data_ptr(), ld_norm=c, coff_norm=0, use_fill=0, fill=0.0)
        da = comp(sub)
        db = CompositeMaskedDesc(base=comp(sub), clear=words.data_ptr(), cs=c, band_idx=(C.c_int32 * 16)(0, 1, 2, 3))
        di = CompositeMaskedDesc(base=comp(stack), clear=words.data_ptr(), cs=cs, band_idx=(C.c_int32 * 16)(*SEL))
        do = CompositeMaskedDesc(base=comp(sub), clear=ones.data_ptr(), cs=c, band_idx=(C.c_int32 * 16)(0, 1, 2, 3))
        run_mask = lambda: check(lib.satcv_quality_mask(C.byref(q), st))
        run_a = lambda: check(lib.satcv_median_composite(C.byref(da), st))
        run_m = lambda d: (lambda: check(lib.satcv_median_composite_masked(C.byref(d), st)))
        b_mask = 8 * t * npix * 2 + nw * npix * 4
        b_a = t * c * npix * 2 + 2 * c * npix * 4
        b_b = b_a + nw * npix * 4
        run_mask()
        share = float((torch.bitwise_and(words[0], 1) != 0).float().mean())
        print(f'u16 {side}^2 x {cs} planes, t = {t}: composite of {c} bands; clear share of acquisition 0 under toa {share:.2f}')
        rc_mask, rc_a = copy_rate(b_mask, a.reps), copy_rate(b_a, a.reps)
        line('mask', b_mask, event_times(run_mask, a.reps), rc_mask)
        for rep in range(2):                                    # A / B / A / B
            line('A', b_a, event_times(run_a, a.reps), rc_a)
            line('B', b_b, event_times(run_m(db), a.reps), rc_a)
        line('B idx', b_b, event_times(run_m(di), a.reps), rc_a)
        line('A', b_a, event_times(run_a, a.reps), rc_a)
        line('B ones', b_b, event_times(run_m(do), a.reps), rc_a)
        line('A', b_a, event_times(run_a, a.reps), rc_a)
        del stack, sub, words, ones, med, nrm


if __name__ == '__main__':
    main()
