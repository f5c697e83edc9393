"""GPU probe: raster_tools.write_cog on the maps of one Sentinel-2 tile (10 980 x 10 980, blocksize 512, overviews 'auto'): a uint8
class map (blocky classes, 255 along the unpredicted border) and a float32 probability map (a smooth field plus noise in the low
mantissa bits, what a softmax leaves).  --quick runs 2 048 x 2 048 maps only.

Per map and compression: the device time of every stage of the writer -- convert, pyramid, tiles, LZW, compaction -- from device
events recorded through the writer's stage hook (one warm-up write, then one measured write), the host waits (the per-tile byte counts,
the copy of the payload), the bytes that cross to the host, the file's size and the wall time of the whole call.  Beside it the only
yardstick a new capability has: the same uncompressed tiles through host zlib level 6 on 16 threads (compress='deflate', the path a
user without the device coder would take), timed the same way.  Nothing here is asserted.

    python tools/cog_probe.py [--quick] [--out profiles/cog_probe.txt]"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from satellite_computervision_amd import raster_tools as rt

TRANSFORM = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)
DEVICE_STAGES = ('convert', 'pyramid', 'tiles', 'lzw', 'compact')


def class_map(n):
    g = torch.Generator(device='cuda').manual_seed(1)
    low = torch.randint(0, 6, (-(-n // 24), -(-n // 24)), generator=g, device='cuda', dtype=torch.uint8)
    m = low.repeat_interleave(24, 0).repeat_interleave(24, 1)[:n, :n].contiguous()
    m[:64] = 255
    m[-64:] = 255
    m[:, :64] = 255
    m[:, -64:] = 255
    return m


def probability_map(n):
    g = torch.Generator(device='cuda').manual_seed(2)
    low = torch.rand((1, 1, -(-n // 64) + 1, -(-n // 64) + 1), generator=g, device='cuda')
    smooth = torch.nn.functional.interpolate(low, size=(n, n), mode='bilinear', align_corners=True)[0, 0]
    return (smooth + 1e-4 * torch.rand((n, n), generator=g, device='cuda')).clamp_(0, 1).contiguous()


def measured_write(arr, path, **kw):
    """one write_cog under the stage hook -> (device seconds per stage, host seconds per stage, wall seconds)"""
    marks = []

    def hook(stage):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((stage, e, time.perf_counter()))
    torch.cuda.synchronize()
    rt._stage_hook = hook
    t0 = time.perf_counter()
    first = torch.cuda.Event(enable_timing=True)
    first.record()
    try:
        rt.write_cog(arr, path, TRANSFORM, 'EPSG:32618', **kw)
    finally:
        rt._stage_hook = None
    wall = time.perf_counter() - t0
    torch.cuda.synchronize()
    dev, host = {}, {}
    prev_e, prev_t = first, t0
    for stage, e, t in marks:
        dev[stage] = prev_e.elapsed_time(e) * 1e-3
        host[stage] = t - prev_t
        prev_e, prev_t = e, t
    return dev, host, wall


def report(name, arr, out, **kw):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'probe.tif')
        for compress in ('lzw', 'deflate'):
            measured_write(arr, path, compress=compress, **kw)                # warm-up: allocator, page cache, kernel load
            dev, host, wall = measured_write(arr, path, compress=compress, **kw)
            size = os.path.getsize(path)
            raw = arr.numel() * arr.element_size()
            out(f'{name}  compress={compress}  {tuple(arr.shape)} {str(arr.dtype).replace("torch.", "")}  options {kw or "{}"}')
            out('  device time per stage [ms]: ' + '  '.join(f'{s} {dev[s] * 1e3:.2f}' for s in DEVICE_STAGES if s in dev))
            out('  host time per stage   [ms]: ' + '  '.join(f'{s} {v * 1e3:.1f}' for s, v in host.items()))
            if compress == 'lzw':
                out(f'  device-to-host bytes: {size} payload + 4 per tile; file {size} bytes = {size / raw:.3f} of the raw map')
            else:
                out(f'  device-to-host bytes: the uncompressed tiles; file {size} bytes = {size / raw:.3f} of the raw map; '
                    f'zlib level 6 on {min(16, os.cpu_count() or 1)} threads {host["deflate"] * 1e3:.1f} ms')
            out(f'  total wall time of write_cog: {wall * 1e3:.1f} ms')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)
    n = 2048 if a.quick else 10980
    out(f'cog_probe: {torch.cuda.get_device_name(0)}, maps of {n} x {n}, blocksize 512, overviews auto')
    report('class map', class_map(n), out, resampling='mode')
    report('class map + predictor', class_map(n), out, resampling='mode', predictor=True)
    report('probability map', probability_map(n), out, resampling='average', nodata=None)
    report('probability map x 100 as uint8', probability_map(n), out, dtype='uint8', scale=100.0, resampling='average')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
