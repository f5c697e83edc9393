"""GPU probe: raster_tools.reproject (satcv_raster_reproject) on a resident Sentinel-2-sized scene, 10980 x 10980 x 4 uint16 in
EPSG:32617 at the eastern edge of its zone, onto the 10 m grid of EPSG:32618 that holds it (--quick: 2048 x 2048).

Per row:
  * reproject nearest / bilinear / cubic: milliseconds and effective GB/s -- the source bytes under the destination counted ONCE plus
    the destination bytes, over the time (the rate a user sees, not the traffic);
  * the same-CRS `warp` of the same scene onto its own grid shifted by a fraction of a pixel, same three rules: the sampling without
    the projection chain;
  * a plain device copy (Tensor.copy_) that moves as many bytes: the yardstick;
  * `pixel_coords` (satcv_grid_coords) of the destination grid alone: the float64 chain per pixel and 16 bytes written -- the cost of
    the chain.
One warm-up of every variant, then REPS rounds that alternate the variants; a sample is the host clock around INNER back-to-back calls
that end in a device synchronise, divided by INNER.  Median and range over the rounds.  Nothing here is asserted.

    python tools/reproject_probe.py [--quick] [--out profiles/reproject_probe.txt]      (appends to --out)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from satellite_computervision_amd import ops, raster_tools as rt
from satellite_computervision_amd._lib import check, lib

T17 = (10.0, 0.0, 600000.0, 0.0, -10.0, 4500000.0)
REPS, INNER = 5, 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / INNER


def copier(nbytes):
    """a device copy that reads nbytes / 2 and writes nbytes / 2"""
    a = torch.empty(nbytes // 2, dtype=torch.uint8, device='cuda')
    b = torch.empty_like(a)
    return lambda: b.copy_(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    n, c = (2048 if a.quick else 10980), 4
    g = torch.Generator(device='cuda').manual_seed(1)
    scene = torch.randint(1, 12000, (n, n, c), generator=g, device='cuda', dtype=torch.int16).view(torch.uint16)
    src = rt.Grid(T17, (n, n), 32617)
    grid = rt.reproject_grid(src, 32618, resolution=10.0)
    shifted = rt.Grid((10.0, 0.0, T17[2] + 3.5, 0.0, -10.0, T17[5] - 6.5), (n, n), 32617)
    out(f'reproject_probe: {torch.cuda.get_device_name(0)}, scene {n} x {n} x {c} uint16 ({scene.numel() * 2 / 1e6:.0f} MB) of EPSG:32617 onto '
        f'{grid.shape[0]} x {grid.shape[1]} pixels of EPSG:32618 at 10 m, {REPS} rounds of {INNER} calls')
    variants, nbytes, rows = {}, {}, []
    for method in ('nearest', 'bilinear', 'cubic'):
        dst = torch.empty(grid.shape + (c,), dtype=torch.uint16, device='cuda')
        name = f'32617 -> 32618  {method}'
        nbytes[name] = scene.numel() * 2 + dst.numel() * 2
        variants[name] = (lambda method=method, dst=dst: rt.reproject(scene, T17, 32617, grid, method, src_nodata=0, out=dst))
        variants[name + ' | copy'] = copier(nbytes[name])
        rows.append(name)
    for method in ('nearest', 'bilinear', 'cubic'):
        dst = torch.empty(shifted.shape + (c,), dtype=torch.uint16, device='cuda')
        name = f'same CRS, shift 0.35 px  {method}'
        win = rt.warp_window(T17, (n, n), shifted, 'nearest')
        nbytes[name] = win[2] * win[3] * c * 2 + dst.numel() * 2
        variants[name] = (lambda method=method, dst=dst: rt.warp(scene, T17, shifted, method, src_nodata=0, out=dst))
        variants[name + ' | copy'] = copier(nbytes[name])
        rows.append(name)
    # the chain alone, into a preallocated field
    m = rt._reproject_map(grid, 32617, T17)
    field = torch.empty((2,) + grid.shape, dtype=torch.float64, device='cuda')
    name = 'grid_coords (the chain alone)'
    nbytes[name] = field.numel() * 8
    variants[name] = lambda: check(lib.satcv_grid_coords(C.byref(m), grid.shape[0], grid.shape[1], 0, 0, field[0].data_ptr(), field[1].data_ptr(), ops.stream_ptr()))
    variants[name + ' | copy'] = copier(nbytes[name])
    rows.append(name)
    times = {k: [] for k in variants}
    for f in variants.values():
        timed(f)                                               # warm-up: code objects, allocator
    for _ in range(REPS):
        for k, f in variants.items():
            times[k].append(timed(f))
    med = {}
    for name in rows:
        t, tc = times[name], times[name + ' | copy']
        med[name], mc = statistics.median(t), statistics.median(tc)
        out(f'  {name:<34} {nbytes[name] / 1e6:8.0f} MB   {med[name]:8.3f} ms ({min(t):.3f} ... {max(t):.3f}) = {nbytes[name] / med[name] * 1e-6:7.0f} GB/s   '
            f'copy {mc:8.3f} ms ({min(tc):.3f} ... {max(tc):.3f}) = {nbytes[name] / mc * 1e-6:7.0f} GB/s   time / copy {med[name] / mc:6.2f}')
    px, spx = grid.shape[0] * grid.shape[1], n * n
    chain = med['grid_coords (the chain alone)']
    out(f'  per destination pixel: chain {chain / px * 1e6:.3f} ns' + ''.join(
        f'; {k}: reproject {med[f"32617 -> 32618  {k}"] / px * 1e6:.3f} ns against warp {med[f"same CRS, shift 0.35 px  {k}"] / spx * 1e6:.3f} ns '
        f'(x {(med[f"32617 -> 32618  {k}"] / px) / (med[f"same CRS, shift 0.35 px  {k}"] / spx):.1f})' for k in ('nearest', 'bilinear', 'cubic')))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
