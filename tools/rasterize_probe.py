"""GPU probe: polygon rasterization and raster masking (csrc/rasterize.hip) at the size of one Sentinel-2 tile, 10 980 x 10 980.

    mask5     raster_tools.geometry_mask for a 5-vertex area of interest
    mask20k   the same for a polygon of about 20 000 vertices (a circle with radial noise)
    apply     raster_tools.mask_apply on a (6, 4, 10980, 10980) uint16 stack with the 5-vertex mask, in place and into a new tensor,
              beside the same masking with torch (masked_fill_ in place, torch.where into a new tensor): what a caller has today

Each step is a process of its own under `timeout`; a step that fails ends the probe, nothing runs after it.  The mask steps are timed
with a host clock around whole calls that end in a device synchronise (GeoJSON parsing and edge table on the host, the copies of the
table, both kernels); the edge table's time, the call from parsed rings and the time between device events around it are given beside it.  The apply step is timed with device events, 3 warm-up launches, then the
median [min, max] of `--reps` launches timed one by one.  Its rate is over the bytes the operation must move: into a new tensor the
stack read and written once and the mask read once; in place the samples outside the mask written once and the mask read once.  The
share of the HBM rate is that rate over 8.0 TB/s (spec) and over 6.29 TB/s (the measured copy rate of MI355X_MICROARCH.md).  Results
are compared with torch's at the size timed.

    python tools/rasterize_probe.py [--quick] [--reps 9] [--out profiles/rasterize_probe.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (('mask5', 240), ('mask20k', 240), ('apply', 420))
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def aoi5(n):
    return {'type': 'Polygon', 'coordinates': [[(0.08 * n, 0.12 * n), (0.71 * n, 0.03 * n), (0.97 * n, 0.55 * n), (0.52 * n, 0.96 * n), (0.05 * n, 0.66 * n)]]}


def aoi20k(n, vertices=20000):
    import numpy as np
    rng = np.random.default_rng(3)
    ang = np.linspace(0, 2 * np.pi, vertices, endpoint=False)
    rad = 0.42 * n * (1 + 0.003 * rng.standard_normal(vertices))
    return {'type': 'Polygon', 'coordinates': [np.stack([n / 2 + rad * np.cos(ang), n / 2 + rad * np.sin(ang)], axis=1).tolist()]}


def host_times(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def event_times(fn, reps, warm=3):
    import torch
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
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def step_mask(n, reps, geom, name):
    import numpy as np
    from satellite_computervision_amd import polygons as pg, raster_tools as rt
    grid = rt.Grid((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (n, n))
    rings = rt.geometry_rings(geom)
    t0 = time.perf_counter()
    table, row_start = pg.edge_table(rings, grid.shape)
    t_table = time.perf_counter() - t0
    tk = host_times(lambda: rt.geometry_mask(geom, grid), reps)
    tr = host_times(lambda: rt._mask_of(rings, grid), reps)
    te = event_times(lambda: rt._mask_of(rings, grid), reps)
    m = rt.geometry_mask(geom, grid)
    inside = int(m.sum().item())
    counts = np.diff(row_start)
    print(f'  {name:<8s} {n} x {n}, {sum(len(r) for g in rings for r in g)} vertices, {len(table)} work items, {int(row_start[-1])} crossings (at most {int(counts.max())} in a row): '
          f'{tk[0] * 1e3:8.3f} ms [{tk[1] * 1e3:.3f}, {tk[2] * 1e3:.3f}] per call, host edge table {t_table * 1e3:.3f} ms of it; {inside} pixels inside '
          f'({inside / n / n:.3f})')
    print(f'           from parsed rings (no GeoJSON parsing): {tr[0] * 1e3:8.3f} ms [{tr[1] * 1e3:.3f}, {tr[2] * 1e3:.3f}] per call; between device events around that call (the copies of the '
          f'table, the crossings and fill kernels): {te[0] * 1e3:8.3f} ms [{te[1] * 1e3:.3f}, {te[2] * 1e3:.3f}]; the mask is {n * n / 1e6:.1f} MB written: {n * n / te[0] / 1e9:.1f} GB/s of it')


def step_apply(n, reps):
    import torch
    from satellite_computervision_amd import raster_tools as rt
    grid = rt.Grid((1.0, 0.0, 0.0, 0.0, 1.0, 0.0), (n, n))
    mask = rt.geometry_mask(aoi5(n), grid)
    mb = mask.bool()
    T, Cn = 6, 4
    stack = torch.randint(1, 10000, (T, Cn, n, n), dtype=torch.int16, device='cuda')
    fresh = stack.clone()
    frac_out = 1.0 - float(mask.sum().item()) / n / n
    total = stack.numel() * 2
    # results first, at the size timed
    zero = torch.zeros((), dtype=torch.int16, device='cuda')
    want = torch.where(mb, stack, zero)
    got = rt.mask_apply(stack, mask, layout='chw', src_dtype='uint16')
    assert torch.equal(got, want), 'mask_apply differs from torch.where'
    work = stack.clone()
    rt.mask_apply(work, mask, layout='chw', inplace=True, src_dtype='uint16')
    assert torch.equal(work, want), 'mask_apply in place differs from torch.where'
    del got, work
    print(f'  apply    ({T}, {Cn}, {n}, {n}) uint16 = {total / 1e9:.2f} GB, {frac_out:.3f} of the pixels outside the mask; results equal torch.where: yes')

    def line(name, nbytes, tk):
        r = nbytes / tk[0]
        print(f'    {name:<44s} {nbytes / 1e9:6.2f} GB to move | {tk[0] * 1e3:8.3f} ms [{tk[1] * 1e3:.3f}, {tk[2] * 1e3:.3f}] = {r / 1e9:7.1f} GB/s = {r / HBM_SPEC:.2f} of 8.0 TB/s, '
              f'{r / HBM_COPY:.2f} of the 6.29 TB/s copy rate')
    new_bytes = 2 * total + n * n
    out = torch.empty_like(stack)
    line('mask_apply into a new tensor', new_bytes, event_times(lambda: rt.ops.raster_mask_apply(mask, stack, out, 1, 1, n, n, T * Cn, 0, T * Cn), reps))
    line('torch.where into a new tensor', new_bytes, event_times(lambda: torch.where(mb, stack, zero, out=out), reps))
    del out
    inplace_bytes = int(frac_out * total) + n * n

    # in place the data changes on the first launch only; every launch writes the same samples again (the kernel does not look at them)
    line('mask_apply in place', inplace_bytes, event_times(lambda: rt.ops.raster_mask_apply(mask, stack, stack, 1, 1, n, n, T * Cn, 0, T * Cn), reps))
    stack.copy_(fresh)
    nmb = ~mb
    line('torch masked_fill_ in place', inplace_bytes, event_times(lambda: stack.masked_fill_(nmb, 0), reps))
    line('copy of the stack (device to device)', 2 * total, event_times(lambda: fresh.copy_(stack), reps))


def run_step(name, quick, reps):
    import torch
    assert torch.cuda.is_available(), 'the probe needs the GPU'
    n = 2048 if quick else 10980
    if name == 'mask5':
        step_mask(n, reps, aoi5(n), name)
    elif name == 'mask20k':
        step_mask(n, reps, aoi20k(n), name)
    else:
        step_apply(n, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--quick', action='store_true')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rasterize_probe.txt'))
    ap.add_argument('--step')
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a.quick, a.reps)
    lines = [f'rasterize_probe: {"2048 x 2048 (--quick)" if a.quick else "10980 x 10980"}, reps {a.reps}; times are medians [min, max]']
    print(lines[0], flush=True)
    ok = True
    for name, limit in STEPS:
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--step', name, '--reps', str(a.reps)] + (['--quick'] if a.quick else [])
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines += r.stdout.rstrip().splitlines()
        print(r.stdout.rstrip(), flush=True)
        if r.returncode != 0:
            lines.append(f'  {name}: FAILED with exit status {r.returncode}; nothing was run after it')
            lines += ['    ' + l for l in r.stderr.rstrip().splitlines()[-12:]]
            print('\n'.join(lines[-13:]), flush=True)
            ok = False
            break
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
