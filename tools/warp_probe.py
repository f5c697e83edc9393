"""GPU probe: raster_tools.warp (satcv_raster_warp) on a resident Sentinel-2-sized scene, 10980 x 10980 x 4 uint16 (--quick: 2048 x 2048).

Destinations: the same grid shifted by a fraction of a pixel (nearest, bilinear, cubic; bilinear also into float32), a grid 2x finer
(bilinear), a grid 10x coarser (average).  Per row:
  * the warp's milliseconds and its effective GB/s -- the source bytes under the destination counted ONCE plus the destination bytes,
    over the time (a tap that is read again by a neighbour is not counted again: this is the rate a user sees, not the traffic);
  * the same figure for a plain device copy (Tensor.copy_) that moves as many bytes: the yardstick;
  * for the float32 bilinear row, torch.nn.functional.grid_sample on the same device, fed a float32 NCHW copy of the scene and a
    ready-made sampling grid (both prepared outside the timed call): what a user could do today.
One warm-up of every variant, then REPS rounds that alternate the variants; a sample is the host clock around INNER back-to-back calls
that end in a device synchronise, divided by INNER.  Median and range over the rounds.  Nothing here is asserted.

    python tools/warp_probe.py [--quick] [--out profiles/warp_probe.txt]      (appends to --out)"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from satellite_computervision_amd import raster_tools as rt

T10 = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
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
    shifted = rt.Grid((10.0, 0.0, T10[2] + 3.5, 0.0, -10.0, T10[5] - 6.5), (n, n))
    finer = rt.Grid((5.0, 0.0, T10[2], 0.0, -5.0, T10[5]), (2 * n, 2 * n))
    coarser = rt.Grid((100.0, 0.0, T10[2], 0.0, -100.0, T10[5]), (n // 10, n // 10))
    rows = [('shift 0.35 px  nearest', shifted, 'nearest', None), ('shift 0.35 px  bilinear', shifted, 'bilinear', None),
            ('shift 0.35 px  cubic', shifted, 'cubic', None), ('shift 0.35 px  bilinear -> f32', shifted, 'bilinear', 'float32'),
            ('2x finer       bilinear', finer, 'bilinear', None), ('10x coarser    average', coarser, 'average', None)]
    out(f'warp_probe: {torch.cuda.get_device_name(0)}, scene {n} x {n} x {c} uint16 ({scene.numel() * 2 / 1e6:.0f} MB), {REPS} rounds of {INNER} calls')
    variants, nbytes = {}, {}
    for name, grid, method, dtype in rows:
        dst = torch.empty(grid.shape + (c,), dtype=torch.float32 if dtype else torch.uint16, device='cuda')
        win = rt.warp_window(T10, (n, n), grid, 'nearest')
        nbytes[name] = win[2] * win[3] * c * 2 + dst.numel() * dst.element_size()
        variants[name] = (lambda grid=grid, method=method, dtype=dtype, dst=dst: rt.warp(scene, T10, grid, method, src_nodata=0, dtype=dtype, out=dst))
        variants[name + ' | copy'] = copier(nbytes[name])
    # grid_sample: normalised coordinates of the shifted grid's pixel centres in the scene (align_corners=False)
    f32 = scene.to(torch.int32).to(torch.float32).permute(2, 0, 1).unsqueeze(0).contiguous()
    xs = ((torch.arange(n, device='cuda', dtype=torch.float32) + 0.5 + 0.35) / n) * 2 - 1
    ys = ((torch.arange(n, device='cuda', dtype=torch.float32) + 0.5 + 0.65) / n) * 2 - 1
    sample_grid = torch.stack(torch.meshgrid(ys, xs, indexing='ij')[::-1], dim=-1).unsqueeze(0).contiguous()
    variants['grid_sample bilinear f32 (NCHW f32 in, f32 out)'] = lambda: torch.nn.functional.grid_sample(f32, sample_grid, mode='bilinear', padding_mode='zeros',
                                                                                                          align_corners=False)
    times = {k: [] for k in variants}
    for f in variants.values():
        timed(f)                                               # warm-up: code objects, allocator
    for _ in range(REPS):
        for k, f in variants.items():
            times[k].append(timed(f))
    for name, grid, method, dtype in rows:
        t, tc = times[name], times[name + ' | copy']
        m, mc = statistics.median(t), statistics.median(tc)
        out(f'  {name:<32} {nbytes[name] / 1e6:8.0f} MB   warp {m:8.3f} ms ({min(t):.3f} ... {max(t):.3f}) = {nbytes[name] / m * 1e-6:7.0f} GB/s   '
            f'copy {mc:8.3f} ms ({min(tc):.3f} ... {max(tc):.3f}) = {nbytes[name] / mc * 1e-6:7.0f} GB/s   warp / copy time {m / mc:5.2f}')
    k = 'grid_sample bilinear f32 (NCHW f32 in, f32 out)'
    t = times[k]
    out(f'  {k}: {statistics.median(t):.3f} ms ({min(t):.3f} ... {max(t):.3f}); it reads {f32.numel() * 4 / 1e6:.0f} MB of float32 and a '
        f'{sample_grid.numel() * 4 / 1e6:.0f} MB grid')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
