"""GPU probe: scene prediction of get_hybrid_model((600, 600, 4), (6, 60, 60, 6), 3) in bf16 over a synthetic 2400 x 2400 uint16 scene and
a (6, 6, 240, 240) int16 time stack (r = 10; kernel 360, buff 240: 25 reference chips of 600^2 / 60^2, batch 8) --
prediction_tools.predict_hybrid_scene (eager, plan=True, a plan with fused=True) against the host loop it replaces (both inputs cut in
NumPy, HybridModel.predict per batch, the full chip probabilities copied back, centres stitched in NumPy) -- and the device time of
satcv_dense_scene_fwd against satcv_dense_small_fwd + satcv_scene_scatter for one full batch of the fusion head (HIP events around
back-to-back launches).  Interleaved: every round times each variant once, after one warm-up round; median and min-max over the rounds.
No thresholds: the output is the record."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from satellite_computervision_amd import lstm_tools as lt, model_tools as mt, ops, prediction_tools as pt
from satellite_computervision_amd._lib import DenseSceneDesc, SceneScatterDesc, check, lib

ROUNDS = int(os.environ.get('HYBRID_PROBE_ROUNDS', '7'))
T, NB, C_, R, KERNEL, BUFF, BATCH, MAXVAL, RESCALE = 6, 6, 4, 10, 360, 240, 8, 10000, 10000
S = int(os.environ.get('HYBRID_PROBE_SCENE', '2400'))
SL = S // R
HEAD_LAUNCHES = 50
rng = np.random.default_rng(0)
scene = (rng.beta(2, 5, (S, S, C_)) * 10000).astype(np.uint16)
stack = (rng.beta(2, 5, (T, NB, SL, SL)) * 10000).astype(np.int16)
mt.set_seed(0)
m = lt.get_hybrid_model((600, 600, C_), (T, 60, 60, NB), 3)
m.compute_dtype = 'bfloat16'
hi, lo, geo = pt.hybrid_chip_tables((S, S), (SL, SL), KERNEL, BUFF, 'reference', int(np.prod(m.factors)))
OFF, SIDE, OFF_LO, SIDE_LO = geo['off'], geo['side'], geo['off_lo'], geo['side_lo']
idx = [tuple(v) for v in hi.tolist()]


def host_loop():
    out = np.zeros((S, S), np.float32)
    for s in range(0, len(idx), BATCH):
        part = idx[s:s + BATCH]
        xu = np.stack([scene[y - OFF:y - OFF + SIDE, x - OFF:x - OFF + SIDE] for y, x in part])
        xu = (xu.astype(np.float64) / RESCALE).astype(np.float32)
        cut = np.stack([stack[:, :, y // R - OFF_LO:y // R - OFF_LO + SIDE_LO, x // R - OFF_LO:x // R - OFF_LO + SIDE_LO] for y, x in part])
        xl = (np.moveaxis(cut, 2, 4).astype(np.float64) / MAXVAL).astype(np.float32)
        p = m.predict([xu, np.where(np.isnan(xl), np.float32(0), xl)], batch_size=len(part))
        for k, (y, x_) in enumerate(part):
            out[y:y + KERNEL, x_:x_ + KERNEL] = p[k, OFF:OFF + KERNEL, OFF:OFF + KERNEL, 0]
    return out


def device_path(plan=None):
    return pt.predict_hybrid_scene(scene, stack, m, KERNEL, BUFF, BATCH, channel=0, cover='reference', rescale=RESCALE, maxval=MAXVAL, plan=plan)


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def head_ms():
    """device time per launch of the fusion head of one full batch: (fused kernel, dense_small_fwd + scene_scatter)"""
    k = m.n_classes
    zl = torch.rand(BATCH, SIDE_LO, SIDE_LO, k, device='cuda')
    zu = torch.randn(BATCH, SIDE, SIDE, k, device='cuda')
    org = torch.from_numpy(hi).cuda()
    fmap = torch.zeros(S, S, 1, device='cuda')
    probs = torch.empty(BATCH, SIDE, SIDE, k, device='cuda')
    d = m.fusion._desc(m._fusion_sources(zl, zu), (SIDE, SIDE))
    d.npix = BATCH * SIDE * SIDE
    sd = DenseSceneDesc(head=d, crop_y=OFF, crop_x=OFF, crop_h=KERNEL, crop_w=KERNEL, origins=org.data_ptr(), total=len(idx), first=0,
                        map=fmap.data_ptr(), map_h=S, map_w=S, ldm=1, c0=0, nc=1, class_map=None)
    d.out = probs.data_ptr()
    sc = SceneScatterDesc(src=probs.data_ptr(), src_kind=2, n=BATCH, sh=SIDE, sw=SIDE, lds=k, c0=0, nc=1, crop_y=OFF, crop_x=OFF, crop_h=KERNEL, crop_w=KERNEL,
                          origins=org.data_ptr(), total=len(idx), first=0, dst=fmap.data_ptr(), dst_kind=2, h=S, w_=S, ldd=1, doff=0, accumulate=0)
    st = ops.stream_ptr()

    def fused():
        check(lib.satcv_dense_scene_fwd(C.byref(sd), st))

    def pair():
        check(lib.satcv_dense_small_fwd(C.byref(d), st))
        check(lib.satcv_scene_scatter(C.byref(sc), st))
    out = {'satcv_dense_scene_fwd': [], 'dense_small_fwd + scene_scatter': []}
    for r in range(ROUNDS + 1):
        for name, fn in (('satcv_dense_scene_fwd', fused), ('dense_small_fwd + scene_scatter', pair)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(HEAD_LAUNCHES):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                out[name].append(a.elapsed_time(b) / HEAD_LAUNCHES * 1e-3)
    return out


def line(name, t, unit_ms=1e3):
    med = float(np.median(t))
    return (f'  {name:34s} median {med * unit_ms:9.3f} ms   min-max {min(t) * unit_ms:9.3f} - {max(t) * unit_ms:9.3f} ms   '
            f'spread {(max(t) - min(t)) / med * 100:5.1f} %')


nb = min(BATCH, len(idx))
batches = (len(idx) + BATCH - 1) // BATCH
print(f'scene uint16 ({S}, {S}, {C_}), stack int16 ({T}, {NB}, {SL}, {SL}), get_hybrid_model((600, 600, {C_}), ({T}, 60, 60, {NB}), 3) bf16, r {R}, '
      f'kernel {KERNEL}, buff {BUFF}: {len(idx)} reference chips of {SIDE}^2 / {SIDE_LO}^2 in {batches} batches of {BATCH}; one warm-up round, then '
      f'{ROUNDS} interleaved rounds', flush=True)
plan_u = m.scene_plan(nb, SIDE, SIDE_LO, fused=False)
plan_f = m.scene_plan(nb, SIDE, SIDE_LO, fused=True)
variants = {'predict_hybrid_scene, eager': device_path, 'predict_hybrid_scene, plan': lambda: device_path(plan_u),
            'predict_hybrid_scene, fused plan': lambda: device_path(plan_f), 'host loop (HybridModel.predict)': host_loop}
times, results = {v: [] for v in variants}, {}
for r in range(ROUNDS + 1):
    for v, fn in variants.items():
        t, results[v] = timed(fn)
        if r:
            times[v].append(t)
print(f'fused layers of the fused plan: {plan_f.fused_layers}; plans replaying: {plan_u.replaying}, {plan_f.replaying}', flush=True)
print('wall time of one whole scene (host clock around the call, device synchronised before and after):', flush=True)
for v in variants:
    print(line(v, times[v]), flush=True)
host = results['host loop (HybridModel.predict)']
mh = float(np.median(times['host loop (HybridModel.predict)']))
for v in list(variants)[:3]:
    md = float(np.median(times[v]))
    print(f'  {v}: map equal to the host loop: {np.array_equal(results[v], host)}; the host loop takes {mh / md:.2f}x its time (medians), '
          f'{len(idx) / md:.1f} against {len(idx) / mh:.1f} chips/s', flush=True)
h = head_ms()
print(f'fusion head of one full batch ({BATCH} chips of {SIDE}^2, crop {KERNEL}^2, 3 + 3 float32 input channels, one of 3 output channels written; '
      f'{HEAD_LAUNCHES} back-to-back launches between two HIP events, per launch):', flush=True)
for name, t in h.items():
    print(line(name, t), flush=True)
a, b = (float(np.median(t)) for t in h.values())
print(f'  the pair takes {b / a:.2f}x the time of satcv_dense_scene_fwd (medians); the crop keeps {KERNEL * KERNEL / (SIDE * SIDE) * 100:.0f} % of the pixels',
      flush=True)
