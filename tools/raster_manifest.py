"""What the raster tools launch and what they compute, as one JSON file -- to compare two checkouts of the package (a change of
raster_tools.py that must not change a launch or a byte) on the same library:

    SATCV_LIB=<libsatcv.so> PYTHONPATH=<checkout A> python tools/raster_manifest.py --out a.json
    SATCV_LIB=<libsatcv.so> PYTHONPATH=<checkout B> python tools/raster_manifest.py --out b.json
    python tools/raster_manifest.py --compare a.json b.json [--baseline a2.json]

Only public names of raster_tools, prediction_tools and pc_tools are used (and `_stage_hook`), so the same file runs in either checkout;
the package is the first one on the path.  Per case (CASES below; inputs are made before the recording starts, from fixed seeds, with
`write_cog` and the hand-made strip and planar-2 files of tests/test_raster_read_cpu.py):
  steps   the stage names `_stage_hook` received, in order
  calls   every lib.satcv_* call under plan_manifest.Recorder: (name, stream, the non-pointer fields of its structures, its non-pointer
          scalars).  The host LZW decoder runs in a thread pool: a run of consecutive satcv_lzw_decode_host calls is sorted.
  hashes  sha256 of every returned tensor or array, of every written file's bytes, and of the repr of every other result
--compare is plan_manifest's: steps, calls and hashes are held to equality."""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(HERE, '..'))            # (behind PYTHONPATH: without one, the package of this checkout)
sys.path.append(os.path.join(HERE, '..', 'tests'))
sys.path.insert(0, HERE)
from plan_manifest import Recorder, _fields, _sha, compare  # noqa: E402,F401

T10 = (10.0, 0.0, 399960.0, 0.0, -10.0, 4500000.0)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, '..', 'tests', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _digest(v):
    import torch
    if isinstance(v, torch.Tensor):
        return _sha(v)
    if isinstance(v, np.ndarray):
        return hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest()
    if isinstance(v, (str, os.PathLike)) and os.path.isfile(v):
        return hashlib.sha256(open(v, 'rb').read()).hexdigest()
    if hasattr(v, 'array') and hasattr(v, 'transform'):                      # a Raster
        return [_digest(v.array), repr((v.transform, v.crs, v.nodata, v.dtype))]
    if isinstance(v, (tuple, list)) and not hasattr(v, 'transform'):
        return [_digest(e) for e in v]
    return hashlib.sha256(repr(v).encode()).hexdigest()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def make_inputs(d, rt):
    """every input of the cases: arrays from fixed seeds, files written into the directory `d`"""
    rng = np.random.default_rng(11)
    hand = _load('test_raster_read_cpu')
    x = dict(dir=d)
    x['u8'] = rng.integers(0, 6, (90, 70), dtype=np.uint8)
    x['f32'] = _dev(rng.random((64, 80, 3), dtype=np.float32))
    x['wide'] = _dev(rng.integers(0, 60000, (48, 64, 5)).astype(np.uint16))
    x['f64'] = rng.standard_normal((40, 56)) * 100
    x['u16'] = rng.integers(1, 60000, (90, 96, 3)).astype(np.uint16)
    x['u16'][20:30, 40:60] = 7
    x['file'] = rt.write_cog(x['u16'], os.path.join(d, 'u16.tif'), T10, 32633, nodata=7, predictor=True, blocksize=16)
    img = rng.integers(0, 60000, (33, 96, 3)).astype(np.uint16)
    for kind in ('lzw strips', 'planar'):
        x[kind] = os.path.join(d, kind.replace(' ', '_') + '.tif')
        open(x[kind], 'wb').write(hand._hand_made(kind, img))
    x['series'] = [rt.write_cog(rng.integers(-500, 9000, (64, 64, 2)).astype(np.int16), os.path.join(d, f's{t}.tif'), T10, 32633, nodata=-32768, blocksize=16)
                   for t in range(3)]
    # files that do not share a grid: a and b on one 10 m grid of zone 17, c at 20 m, d in zone 18
    px, py = rt.transform_points([-78.0], [40.0], 4326, 32617)
    x0, y0 = round(float(px[0]) / 20) * 20.0, round(float(py[0]) / 20) * 20.0
    qx, qy = rt.transform_points([x0 + 150.0], [y0 - 90.0], 32617, 32618)
    placed = {'a': ((10.0, 0.0, x0, 0.0, -10.0, y0), 32617), 'b': ((10.0, 0.0, x0 + 200.0, 0.0, -10.0, y0 - 100.0), 32617),
              'c': ((20.0, 0.0, x0 - 100.0, 0.0, -20.0, y0 + 60.0), 32617), 'd': ((10.0, 0.0, round(float(qx[0])), 0.0, -10.0, round(float(qy[0]))), 32618)}
    for k, (t, code) in placed.items():
        a = rng.integers(8, 60000, (48, 40, 2)).astype(np.uint16)
        a[5:9, 30:36] = 7
        x[k] = rt.write_cog(a, os.path.join(d, f'{k}.tif'), t, code, nodata=7, blocksize=16)
    x['ta'], x['origin'] = placed['a'][0], (x0, y0)
    x['grid'] = rt.Grid((10.0, 0.0, x0 + 53.5, 0.0, -10.0, y0 - 36.5), (33, 29), 32617)
    x['grid3'] = rt.Grid((3.0, 0.0, x0 + 20.5, 0.0, -3.0, y0 - 10.0), (41, 67), 32617)
    x['away'] = rt.Grid((10.0, 0.0, x0 + 9000.0, 0.0, -10.0, y0), (8, 9), 32617)
    x['grid18'] = rt.Grid((10.0, 0.0, round(float(qx[0])) - 100.0, 0.0, -10.0, round(float(qy[0])) + 60.0), (50, 44), 32618)
    x['src'] = _dev(rng.integers(8, 60000, (37, 53, 3)).astype(np.uint16))
    x['srcf'] = _dev((rng.standard_normal((37, 53, 2)) * 3000).astype(np.float32))
    x['lonlat'] = rt.Grid((1e-4, 0.0, -78.002, 0.0, -1e-4, 40.003), (37, 53), 4326)
    return x


def _cases(x, rt, pt):
    import torch
    d, f, g, g3, ta, src = x['dir'], x['file'], x['grid'], x['grid3'], x['ta'], x['src']
    out = lambda name: os.path.join(d, name)
    C = {}
    # ---- write_cog
    C['write uint8 lzw predictor mode'] = lambda: rt.write_cog(x['u8'], out('w1.tif'), T10, 32633, predictor=True, blocksize=16, resampling='mode')
    C['write float32 scale uint8 average'] = lambda: rt.write_cog(x['f32'], out('w2.tif'), T10, 32633, dtype='uint8', scale=100.0, blocksize=16, resampling='average')
    C['write channel slice'] = lambda: rt.write_cog(x['wide'].view(torch.int16)[..., 1:3], out('w3.tif'), T10, 32633, dtype='uint16', nodata=None, blocksize=16)
    C['write float64 host'] = lambda: rt.write_cog(x['f64'], out('w4.tif'), T10, 'EPSG:4326', nodata=None, blocksize=16)
    C['write deflate'] = lambda: rt.write_cog(x['u8'], out('w5.tif'), T10, 32633, compress='deflate', blocksize=16)
    C['write uncompressed'] = lambda: rt.write_cog(x['u16'], out('w6.tif'), T10, 32633, compress=None, blocksize=32, overviews=1)
    C['numpy_to_raster'] = lambda: rt.numpy_to_raster(x['u8'], {'transform': list(T10), 'crs': 'EPSG:32633', 'cols': 70, 'rows': 90}, out('w7.tif'), 'uint8')
    C['device_pyramid'] = lambda: rt.device_pyramid(x['f32'], dtype='uint8', scale=100.0, blocksize=16, resampling='average')
    # ---- read_cog
    C['read whole'] = lambda: rt.read_cog(f)
    C['read window'] = lambda: rt.read_cog(f, window=(13, 7, 40, 61))
    C['read bands'] = lambda: rt.read_cog(f, bands=[2, 0])
    C['read chw'] = lambda: rt.read_cog(f, window=(1, 2, 33, 50), layout='chw')
    C['read level 1'] = lambda: rt.read_cog(f, level=1)
    C['read decode host'] = lambda: rt.read_cog(f, decode='host')
    C['read decode device'] = lambda: rt.read_cog(f, decode='device')
    C['read strips'] = lambda: rt.read_cog(x['lzw strips'], window=(5, 3, 20, 70))
    C['read planar 2'] = lambda: rt.read_cog(x['planar'], bands=[1, 2])
    C['read device=False'] = lambda: rt.read_cog(f, window=(13, 7, 40, 61), bands=[1], device=False)
    C['read out='] = lambda: rt.read_cog(f, layout='chw', out=torch.zeros((3, 90, 96), dtype=torch.int16, device='cuda'))
    C['read_stack'] = lambda: rt.read_stack(x['series'], window=(3, 5, 50, 40))
    # ---- warp
    for method in ('nearest', 'bilinear', 'cubic'):
        C[f'warp {method}'] = lambda method=method: rt.warp(src, ta, g3, method, src_nodata=7, src_dtype='uint16')
    C['warp average'] = lambda: rt.warp(src, (1.0, 0.0, ta[2], 0.0, -1.0, ta[5]), rt.Grid((4.0, 0.0, ta[2] - 3.5, 0.0, -4.0, ta[5] + 2.5), (11, 15), 32617), 'average', src_nodata=7, src_dtype='uint16')
    C['warp float32'] = lambda: rt.warp(src, ta, g3, 'bilinear', src_nodata=7, nodata=-1.0, dtype='float32', src_dtype='uint16')
    C['warp chw source'] = lambda: rt.warp(src.permute(2, 0, 1).contiguous(), ta, g3, 'cubic', src_nodata=7, src_layout='chw', src_dtype='uint16')
    C['warp chw slot'] = lambda: rt.warp(src, ta, g3, 'nearest', src_nodata=7, layout='chw', out=torch.full((6,) + g3.shape, 5, dtype=torch.int16, device='cuda'), channel_offset=2, src_dtype='uint16')
    C['warp keep'] = lambda: rt.warp(src, ta, g3, 'bilinear', src_nodata=7, out=torch.full(g3.shape + (3,), 5, dtype=torch.int16, device='cuda'), keep=True, src_dtype='uint16')
    C['warp window origin'] = lambda: rt.warp(src[4:30, 6:50].contiguous(), ta, g3, 'cubic', src_nodata=7, src_origin=(4, 6), src_dtype='uint16')
    C['warp two-dimensional'] = lambda: rt.warp(x['srcf'][..., 0].contiguous(), ta, g3, 'bilinear')
    # ---- readers onto a grid
    C['read_warped hit'] = lambda: rt.read_warped(x['a'], g, resampling='bilinear')
    C['read_warped miss'] = lambda: rt.read_warped(x['a'], x['away'], layout='chw')
    C['read_warped miss out'] = lambda: rt.read_warped(x['a'], x['away'], out=torch.full((8, 9, 4), 5, dtype=torch.int16, device='cuda'), channel_offset=1)
    C['read_warped miss out keep'] = lambda: rt.read_warped(x['a'], x['away'], out=torch.full((8, 9, 4), 5, dtype=torch.int16, device='cuda'), channel_offset=1, keep=True)
    C['read_warped auto'] = lambda: rt.read_warped(f, rt.Grid((40.0, 0.0, T10[2] + 15.0, 0.0, -40.0, T10[5] - 25.0), (20, 21), 32633), resampling='bilinear', level='auto')
    C['read_mosaic last'] = lambda: rt.read_mosaic([x['a'], x['b'], x['c']], resampling='bilinear')
    C['read_mosaic first'] = lambda: rt.read_mosaic([x['a'], x['b'], x['c']], first=True, layout='chw', dtype='float32')
    C['read_aligned_stack'] = lambda: rt.read_aligned_stack([x['a'], [x['b'], x['c']]])
    # ---- between coordinate systems
    for method in ('nearest', 'bilinear', 'cubic'):
        C[f'reproject 17 -> 18 {method}'] = lambda method=method: rt.reproject(src, ta, 32617, x['grid18'], method, src_nodata=7, src_dtype='uint16')
    C['reproject 4326 -> utm'] = lambda: rt.reproject(x['srcf'], x['lonlat'].transform, 4326, g, 'bilinear')
    C['reproject same code'] = lambda: rt.reproject(src, ta, 32617, g3, 'cubic', src_nodata=7, src_dtype='uint16')
    C['pixel_coords'] = lambda: [rt.pixel_coords(g, crs=4326), rt.pixel_coords(x['grid18'], crs=32617, transform=ta)]
    C['reproject_grid'] = lambda: [rt.reproject_grid(x['a'], 32618), rt.reproject_grid(g, 4326, resolution=1e-4)]
    C['union_grid reproject'] = lambda: [rt.union_grid([x['a'], x['d']], reproject=True), rt.union_grid([x['d'], x['b']], resolution=20, reproject=True, crs=32617)]
    C['windows and levels'] = lambda: [rt.warp_window(ta, (48, 40), g, m) for m in ('nearest', 'cubic', 'average')] + [
        rt.reproject_window(ta, (48, 40), 32617, x['grid18'], 'bilinear'), rt.auto_level([ta, (20.0, 0.0, ta[2], 0.0, -20.0, ta[5])], x['grid18'], 32617)]
    C['read_warped reproject'] = lambda: rt.read_warped(x['a'], x['grid18'], resampling='cubic', reproject=True)
    C['read_mosaic reproject'] = lambda: rt.read_mosaic([x['a'], x['b'], x['d']], reproject=True)
    C['read_aligned_stack reproject'] = lambda: rt.read_aligned_stack([[x['a'], x['d']], x['b']], resampling='bilinear', reproject=True)
    return C


def _driver_cases(x, rt, pt, C):
    """one file-to-file prediction per driver, with the smallest models of tests/test_scene_predict_gpu.py and tests/hybrid_scene_cases.py"""
    from satellite_computervision_amd import lstm_tools as lt, model_tools as mt
    d = x['dir']
    rng = np.random.default_rng(3)
    scene = rng.integers(-200, 3000, (96, 96, 4)).astype(np.int16)
    sfile = rt.write_cog(scene, os.path.join(d, 'scene_i16.tif'), T10, 32633, nodata=None, blocksize=16)
    unet = _load('test_scene_predict_gpu')._unet(mt, 'bfloat16')
    C['predict_raster int16'] = lambda: [pt.predict_raster(sfile, unet, os.path.join(d, 'p1.tif'), kernel=32, buff=16, batch_size=4, channel=1, cog_options=dict(blocksize=16)),
                                         os.path.join(d, 'p1.tif')]
    HC = _load('hybrid_scene_cases')
    HY = HC.HYBRID
    hm = HC.hybrid_model(lt, mt, 'bfloat16')
    hscene, hstack = HC.hybrid_scene('reference')
    h, w = HY['reference']['lo']
    t1 = (1.0, 0.0, 500000.0, 0.0, -1.0, 4100000.0)
    hfile = rt.write_cog(hscene, os.path.join(d, 'hscene.tif'), t1, 32633, nodata=None, blocksize=16)
    items = []
    for t in range(HY['T']):
        big = np.full((h + 5, w + 6, HY['c']), -32768, np.int16)
        big[2 + t:2 + t + h, 3 - t:3 - t + w] = hstack[t].transpose(1, 2, 0)
        items.append(rt.write_cog(big, os.path.join(d, f'h{t}.tif'), (6.0, 0.0, t1[2] - 6.0 * (3 - t), 0.0, -6.0, t1[5] + 6.0 * (2 + t)), 32633, nodata=-32768, blocksize=16))
    kw = dict(kernel=HY['kernel'], buff=HY['buff'], batch_size=HY['batch'], rescale=HC.RESCALE, maxval=HC.MAXVAL)
    C['predict_hybrid_raster'] = lambda: [pt.predict_hybrid_raster(hfile, items, hm, os.path.join(d, 'p2.tif'), channel=None, **kw), os.path.join(d, 'p2.tif')]


def _sorted_pool_calls(calls):
    """runs of consecutive satcv_lzw_decode_host calls (a thread pool issues them in any order) in a canonical order"""
    out, run = [], []
    for c in calls + [None]:
        if c is not None and c[0] == 'satcv_lzw_decode_host':
            run.append(c)
            continue
        out += sorted(run, key=lambda v: json.dumps(v, sort_keys=True, default=str))
        run = []
        if c is not None:
            out.append(c)
    return out


def collect(path, only):
    import torch
    import satellite_computervision_amd
    from satellite_computervision_amd import prediction_tools as pt, raster_tools as rt
    from satellite_computervision_amd._lib import lib
    print('package:', os.path.dirname(satellite_computervision_amd.__file__), flush=True)
    res = {}
    with tempfile.TemporaryDirectory() as d:
        x = make_inputs(d, rt)
        cases = _cases(x, rt, pt)
        _driver_cases(x, rt, pt, cases)
        for name, run in cases.items():
            if only and name not in only:
                continue
            stages, rec = [], Recorder(lib)
            rt._stage_hook = stages.append
            try:
                result = run()
                torch.cuda.synchronize()
            finally:
                rt._stage_hook = None
                rec.restore()
            res[name] = dict(steps=stages, calls=json.loads(json.dumps(_sorted_pool_calls(rec.calls), default=lambda o: o.item() if hasattr(o, 'item') else str(o))),
                             hashes={'result': _digest(result)}, losses=[])
            print(f'{name}: {len(stages)} stages, {len(rec.calls)} calls', flush=True)
    json.dump(res, open(path, 'w'), indent=0, sort_keys=True)
    print(f'{len(res)} cases written to {path}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--baseline', nargs='+', help='further runs of checkout A')
    ap.add_argument('--cases', type=lambda v: v.split(','), help='only these cases (comma-separated names)')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.baseline))
    collect(a.out, a.cases)
