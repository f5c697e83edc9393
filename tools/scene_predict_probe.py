"""GPU probe: whole-scene prediction of a five-level get_unet_model over one 4-band 2816^2 scene (256^2 centres, 128-pixel buffer: 100
reference chips of 384^2, 121 full-cover chips, batch 16) -- predict_chips (host windows, both outputs copied back per batch) against
predict_chips_device and predict_scene(cover='full') (scene and map resident on the device).  Scene dtypes float32 and uint16 with
rescale=10000; plans folded bf16 and fp8.  Interleaved A/B: every round times each variant once; median, min-max spread over the rounds,
and the share of predict_chips' wall time spent outside predict_on_device (the same batches, resident, run back to back)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from satellite_computervision_amd import model_tools as mt, prediction_tools as pt

ROUNDS = int(os.environ.get('SCENE_PROBE_ROUNDS', '5'))
S, KERNEL, BUFF, BATCH = 2816, 256, 128, 16
SIDE = KERNEL + BUFF
rng = np.random.default_rng(0)
scene_u16 = (rng.beta(2, 5, (S, S, 4)) * 10000).astype(np.uint16)
scene_f32 = (scene_u16.astype(np.float64) / 10000).astype(np.float32)
idx = pt.generate_chip_indices(scene_f32, BUFF, KERNEL)
full = pt.full_cover_indices(scene_f32.shape, KERNEL)


def model(plan):
    mt.reset_uids(); mt.set_seed(0); mt.set_compute_dtype('bfloat16')
    m = mt.get_unet_model(2, 4)                          # bf16: the folded plan is the default
    if plan == 'fp8':
        m.enable_fp8_inference(np.stack([scene_f32[y:y + SIDE, x:x + SIDE] for y, x in idx[:4]]))
    return m


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_only(m, x):
    """the model's share: the batches of the reference chip list, already resident, back to back"""
    for s in range(0, len(idx), BATCH):
        m.predict_on_device(x[:min(BATCH, len(idx) - s)])


print(f'scene {S}x{S}x4, kernel {KERNEL}, buff {BUFF}: {len(idx)} reference chips / {len(full)} full-cover chips of {SIDE}^2, batch {BATCH}; '
      f'median of {ROUNDS} interleaved rounds, spread = (max - min) / median', flush=True)
for plan in ('bf16', 'fp8'):
    m = model(plan)
    x = torch.from_numpy(np.stack([scene_f32[y:y + SIDE, x_:x_ + SIDE] for y, x_ in idx[:BATCH]])).cuda()
    for dt, scene_host, scene_dev, rescale in (('float32', scene_f32, scene_f32, None), ('uint16/10000', scene_f32, scene_u16, 10000)):
        # (predict_chips has no rescale: its uint16 row is fed the scene already divided on the host, outside the timed region)
        variants = {
            'predict_chips': (len(idx), lambda: pt.predict_chips(scene_host, idx, np.zeros((S, S), np.float32), m, KERNEL, BUFF, BATCH)),
            'predict_chips_device': (len(idx), lambda: pt.predict_chips_device(scene_dev, idx, np.zeros((S, S), np.float32), m, KERNEL, BUFF, BATCH, rescale=rescale)),
            'predict_scene full': (len(full), lambda: pt.predict_scene(scene_dev, m, KERNEL, BUFF, BATCH, cover='full', rescale=rescale)),
            'predict_on_device only': (len(idx), lambda: device_only(m, x)),
        }
        times = {v: [] for v in variants}
        for r in range(ROUNDS + 1):
            for v, (_, fn) in variants.items():
                t = timed(fn)
                if r:                                    # (round 0: plan builds and warm-up)
                    times[v].append(t)
        med = {v: float(np.median(t)) for v, t in times.items()}
        print(f'{plan} plan, {dt} scene:', flush=True)
        for v, (chips, _) in variants.items():
            t = times[v]
            print(f'  {v:24s} {med[v] * 1e3:8.2f} ms  {chips / med[v]:8.1f} chips/s  min-max {chips / max(t):8.1f} - {chips / min(t):8.1f} chips/s  '
                  f'spread {(max(t) - min(t)) / med[v] * 100:5.1f} %', flush=True)
        host = times['predict_chips']
        gain = med['predict_chips'] - med['predict_chips_device']
        print(f'  predict_chips outside predict_on_device: {(1 - med["predict_on_device only"] / med["predict_chips"]) * 100:5.1f} % of its wall time', flush=True)
        print(f'  predict_chips_device vs predict_chips: {med["predict_chips"] / med["predict_chips_device"]:.2f}x, gain {gain * 1e3:.2f} ms against a '
              f'predict_chips min-max spread of {(max(host) - min(host)) * 1e3:.2f} ms -> {"FASTER" if gain > max(host) - min(host) else "NOT faster"} '
              f'by more than the spread', flush=True)
    del m, x
