"""GPU probe: the five calibration kernels (csrc/calibrate.hip) on two uint16 rasters of one Sentinel-2 tile (10 980 x 10 980) with 4
bands and a full-overlap region; --quick runs 2 048 x 2 048 only.

Timed with device events (3 warm-up launches, then the median [min, max] of `--reps` launches timed one by one):
  overlap    both rasters in, the region out
  histogram  the plain form (split = -1: global atomicAdd only, no LDS) against the LDS-private form at several split points, on
             (a) reflectance-like data (most samples below 8192, a bright tail above), (b) uniform over all 65536 bins, (c) a constant plane
  match_lut, scale_lut   one workgroup per band: microseconds, no streaming
  apply      planar in the source kind, planar to float32, pixel-interleaved in the source kind
Each streaming line gives the ALGORITHMIC bytes (planes read + outputs written), the rate over them, and the rate of a device-to-device
copy of the same volume in the same run.  The histogram has no streaming roof to be held to: its lines are read against one another.

    python tools/calibration_probe.py [--quick] [--reps 9] > profiles/calibration_probe.txt"""
import argparse
import ctypes as C
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from satellite_computervision_amd import calibration as cal, ops
from satellite_computervision_amd._lib import CalibApplyDesc, check, lib

SPLITS = (-1, 1024, 4096, 8192, 16384, 32768)


def event_times(fn, reps, warm=3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    if a.elapsed_time(b) > 300.0:                                # a launch beyond 0.3 s (global atomics on one address): 3 launches, no more warm-up
        reps, warm = min(reps, 3), 0
    for _ in range(max(0, warm - 1)):
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
    print(f'  {name:<22s} {nbytes / 1e9:6.2f} GB | {tk[0] * 1e3:8.3f} ms [{tk[1] * 1e3:.3f}, {tk[2] * 1e3:.3f}] = {rk:5.2f} TB/s | copy of equal volume {rc:5.2f} TB/s | '
          f'kernel / streaming = {rk / rc:.2f}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures on the GPU only'
    p = torch.cuda.get_device_properties(0)
    print(f'box {socket.gethostname()}: {p.name}, {p.multi_processor_count} CUs, {p.total_memory / 2 ** 30:.0f} GiB; torch {torch.__version__}; reps {a.reps} (median [min, max])')
    side, c = (2048 if a.quick else 10980), 4
    npix, st = side * side, ops.stream_ptr()
    g = torch.Generator(device='cuda').manual_seed(side)

    def reflectance():
        x = torch.randn((c, side, side), generator=g, device='cuda') * 900 + 2000
        bright = torch.rand((c, side, side), generator=g, device='cuda')
        x = torch.where(bright < 0.02, 6000 + bright * 3e5, x).clamp_(1, 65535)
        return x.to(torch.int32).to(torch.int16)                # (values below 32768: the int16 holds the uint16 bytes)
    img1, img2 = reflectance(), reflectance()
    uniform = torch.randint(-32768, 32768, (c, side, side), generator=g, device='cuda', dtype=torch.int16)
    constant = torch.full((c, side, side), 1500, device='cuda', dtype=torch.int16)
    region = torch.empty((side, side), dtype=torch.uint8, device='cuda')
    hist1 = torch.empty((c, 65536), dtype=torch.int32, device='cuda')
    hist2 = torch.empty_like(hist1)
    lut = torch.empty((c, 65536), dtype=torch.int16, device='cuda')
    table = torch.empty((c, 65536), dtype=torch.float32, device='cuda')
    upper = torch.empty((c,), dtype=torch.int32, device='cuda')
    print(f'u16 {side}^2 x {c} bands, two rasters, nodata 0, full-overlap region; share of raster 1 below bin 8192: {float((img1 < 8192).float().mean()):.3f}')

    run_overlap = lambda: check(lib.satcv_calib_overlap(img1.data_ptr(), img2.data_ptr(), 1, c, side, side, 1, 0.0, None, region.data_ptr(), st))
    b_overlap = npix * (2 * c * 2 + 1)
    line('overlap', b_overlap, event_times(run_overlap, a.reps), copy_rate(b_overlap, a.reps))
    assert bool(region.all())

    b_hist = npix * c * 3
    rc_hist = copy_rate(b_hist, a.reps)
    for what, img in (('(a) reflectance', img1), ('(b) uniform', uniform), ('(c) constant', constant)):
        for rep in range(2):                                     # the whole table twice: the spread between the two passes is the noise
            for split in SPLITS:
                run = lambda: check(lib.satcv_calib_histogram(img.data_ptr(), 1, c, side, side, region.data_ptr(), hist1.data_ptr(), split, st))
                name = f'{what} ' + ('plain' if split < 0 else f'split {split}')
                line(name, b_hist, event_times(run, a.reps), rc_hist)
    check(lib.satcv_calib_histogram(img1.data_ptr(), 1, c, side, side, region.data_ptr(), hist1.data_ptr(), 0, st))
    check(lib.satcv_calib_histogram(img2.data_ptr(), 1, c, side, side, region.data_ptr(), hist2.data_ptr(), 0, st))
    assert int(hist1.sum()) == c * npix

    tm = event_times(lambda: check(lib.satcv_calib_match_lut(hist1.data_ptr(), hist2.data_ptr(), 1, c, lut.data_ptr(), None, st)), a.reps)
    ts = event_times(lambda: check(lib.satcv_calib_scale_lut(hist2.data_ptr(), 1, c, 99, table.data_ptr(), upper.data_ptr(), st)), a.reps)
    print(f'  match_lut  {tm[0] * 1e6:8.1f} us [{tm[1] * 1e6:.1f}, {tm[2] * 1e6:.1f}]   scale_lut  {ts[0] * 1e6:8.1f} us [{ts[1] * 1e6:.1f}, {ts[2] * 1e6:.1f}]   (c = {c} workgroups)')

    def apply(tab, dst, f32, layout):
        d = CalibApplyDesc(src=img2.data_ptr(), src_kind=1, c=c, h=side, w_=side, has_nodata=1, nodata=0.0, table=tab.data_ptr(), dst=dst.data_ptr(),
                           dst_kind=2 if f32 else 1, dst_layout=layout, dst_ld=c, dst_coff=0, keep=0)
        return lambda: check(lib.satcv_calib_apply(C.byref(d), st))
    out16 = torch.empty((c, side, side), dtype=torch.int16, device='cuda')
    out32 = torch.empty((c, side, side), dtype=torch.float32, device='cuda')
    for name, run, nbytes in (('apply planar u16', apply(lut, out16, False, 1), npix * c * 4), ('apply planar f32', apply(table, out32, True, 1), npix * c * 6),
                              ('apply interleaved u16', apply(lut, out16, False, 0), npix * c * 4)):
        line(name, nbytes, event_times(run, a.reps), copy_rate(nbytes, a.reps))

    torch.cuda.synchronize()
    t = event_times(lambda: cal.equalize(img1.view(torch.uint16), img2.view(torch.uint16), nodata=0, out=out16.view(torch.uint16)), max(3, a.reps // 3), warm=1)
    print(f'  calibration.equalize (overlap, two histograms, table, apply): {t[0] * 1e3:.3f} ms [{t[1] * 1e3:.3f}, {t[2] * 1e3:.3f}]')


if __name__ == '__main__':
    main()
