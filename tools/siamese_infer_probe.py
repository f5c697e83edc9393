"""GPU probe: Siamese U-Net inference (make_siamese_unet, 256^2 x 4 bands, filters [32, 64, 128]) -- the regular plan, the folded bf16
plan with one launch per date (pair=False) and with the pair store (pair=True), the hybrid fp8 plan -- at batch 16 and 64, and two-date
predict_chips over a 1024^2 scene pair.  Interleaved A/B: every round times each variant once (median over the rounds)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from satellite_computervision_amd import model_tools as mt, fp8_infer as fi, prediction_tools as pt

ROUNDS, REPS = 7, 10
mt.reset_uids(); mt.set_seed(0); mt.set_compute_dtype('bfloat16')
m = mt.make_siamese_unet(4, [32, 64, 128], [2, 2, 2])
rng = np.random.default_rng(0)


def use(variant, plans, q=None):
    """point the model's inference-plan state at one variant (its plans are built once and kept)"""
    if variant == 'regular':
        m.disable_fp8_inference()
    else:
        m._fp8_q, m._fp8_store, m._fp8_plans = (q if variant == 'fp8' else {}), (fi.FP8 if variant == 'fp8' else fi.BF16), plans


def build(variant, n, s, q):
    if variant == 'regular':
        return None
    plan = fi.Fp8Plan(m, n, s, s, q, store=fi.FP8 if variant == 'fp8' else fi.BF16, pair=variant != 'folded-unpaired')
    plan.weights_version = m.runtime.version
    return {(n, s, s): plan}


def run(x, reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        m.predict_on_device(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


VARIANTS = ['regular', 'folded-unpaired', 'folded-paired', 'fp8']
for n in (16, 64):
    s = 256
    xa = torch.from_numpy(rng.beta(2, 5, (n, s, s, 4)).astype(np.float32)).cuda()
    xb = torch.from_numpy(rng.beta(2, 5, (n, s, s, 4)).astype(np.float32)).cuda()
    x = [xa, xb]
    q = fi.calibrate(m, [xa[:8], xb[:8]])
    plans = {v: build(v, n, s, q) for v in VARIANTS}
    for v in VARIANTS:                                   # warm-up (and graph capture where the plan is replayed)
        use(v, plans[v], q); run(x, 3)
    times = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            use(v, plans[v], q)
            times[v].append(run(x, REPS))
    med = {v: float(np.median(t)) for v, t in times.items()}
    spread = {v: (max(t) - min(t)) / med[v] for v, t in times.items()}
    print(f'batch {n} pairs of {s}x{s}x4 (median of {ROUNDS} interleaved rounds x {REPS} runs):', flush=True)
    for v in VARIANTS:
        print(f'  {v:16s} {med[v] * 1e3:8.3f} ms  {n / med[v]:8.1f} pairs/s  spread {spread[v] * 100:4.1f} %  vs regular {med["regular"] / med[v]:.3f}x', flush=True)
    print(f'  pairing: folded-paired vs folded-unpaired {med["folded-unpaired"] / med["folded-paired"]:.3f}x', flush=True)
    del plans
    m.disable_fp8_inference()

# two-date predict_chips over a 1024^2 scene pair (256^2 centres, 128-pixel buffer: 384^2 chips, batch 16); the folded plan is built once
A = rng.beta(2, 5, (1024, 1024, 4)).astype(np.float32)
B = rng.beta(2, 5, (1024, 1024, 4)).astype(np.float32)
idx = pt.generate_chip_indices(A, 128, 256)
m.enable_folded_inference()
folded_plans = m._fp8_plans
chip_t = {'regular': [], 'folded-paired': []}
for r in range(ROUNDS + 1):
    for v in chip_t:
        use(v, folded_plans)
        tmpl = np.zeros(A.shape[:2], np.float32)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pt.predict_chips((A, B), idx, tmpl, m, kernel=256, buff=128, batch_size=16)
        torch.cuda.synchronize()
        if r:                                            # (round 0: plan builds and warm-up)
            chip_t[v].append(time.perf_counter() - t0)
print(f'predict_chips, scene pair {A.shape[0]}x{A.shape[1]}x4, {len(idx)} chips of 384^2, batch 16 (median of {ROUNDS} interleaved runs, host chip '
      f'extraction and copies included):')
for v, t in chip_t.items():
    print(f'  {v:16s} {np.median(t) * 1e3:8.2f} ms  {len(idx) / np.median(t):7.1f} chips/s  spread {(max(t) - min(t)) / np.median(t) * 100:4.1f} %')
