"""GPU probe of lstm_infer.SeriesInferPlan (the record is profiles/series_plan_probe.txt; no thresholds).

Whole scene: the workload of tools/series_predict_probe.py -- int16 (6, 6, 1024, 1024), get_lstm_model(6, 3, 6) bf16, kernel 32, buff 32,
900 reference chips of 64^2 in 15 batches of 64, stack resident on the device -- through predict_series_scene with
  default path (the eager tape)  |  plan unfused, eager (SATCV_LSTM_GRAPH=0)  |  plan unfused, replayed  |  plan fused, replayed.
One warm-up round, then the median and min - max of 7 interleaved rounds (host clock, device synchronised before and after).

Isolated step: HIP events around 50 back-to-back launches, bf16, B = 64 images of 64^2, F = 64 and F = 16: the recurrent ops.conv2d +
satcv_convlstm_gates_fwd pair against ONE satcv_convlstm_step_fwd, with the derived bytes per pixel (pair: xg 8F read, hg 8F written +
8F read, c 4F + 4F, h 2F written + 2F read by the conv; fused: the same minus the hg round trip) and 2 * 9 * F * 4F flop per pixel."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from satellite_computervision_amd import lstm_infer as li, lstm_tools as lt, model_tools as mt, ops, prediction_tools as pt
from satellite_computervision_amd._lib import BF16, LstmGatesDesc, LstmStepDesc, check, lib

ROUNDS = int(os.environ.get('SERIES_PROBE_ROUNDS', '7'))
T, NB, S, KERNEL, BUFF, BATCH, MAXVAL = 6, 6, 1024, 32, 32, 64, 10000
SIDE = KERNEL + BUFF
LAUNCHES = 50


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def line(name, t):
    med = float(np.median(t))
    return f'  {name:34s} median {med * 1e3:9.3f} ms   min-max {min(t) * 1e3:9.3f} - {max(t) * 1e3:9.3f} ms   spread {(max(t) - min(t)) / med * 100:5.1f} %'


def scene():
    rng = np.random.default_rng(0)
    stack = torch.from_numpy((rng.beta(2, 5, (T, NB, S, S)) * 10000).astype(np.int16)).cuda()
    idx = pt.generate_chip_indices(np.empty((S, S, 0)), BUFF, KERNEL)
    mt.set_seed(0)
    m = lt.get_lstm_model(NB, 3, T)
    m.compute_dtype = 'bfloat16'
    shape = (BATCH, T, SIDE, SIDE)
    os.environ['SATCV_LSTM_GRAPH'] = '1'
    plans = {'plan unfused, eager': m.inference_plan(shape, fused=False), 'plan unfused, replayed': m.inference_plan(shape, fused=False),
             'plan fused, replayed': m.inference_plan(shape, fused=True)}

    def run(name):
        os.environ['SATCV_LSTM_GRAPH'] = '0' if name == 'plan unfused, eager' else '1'       # (the switch is read per call)
        try:
            return pt.predict_series_scene(stack, m, KERNEL, BUFF, BATCH, channel=0, cover='reference', maxval=MAXVAL, plan=plans.get(name))
        finally:
            os.environ['SATCV_LSTM_GRAPH'] = '1'
    names = ['default path (eager tape)'] + list(plans)
    times, res = {n: [] for n in names}, {}
    print(f'stack int16 ({T}, {NB}, {S}, {S}) resident, get_lstm_model({NB}, 3, {T}) bf16, kernel {KERNEL}, buff {BUFF}: {len(idx)} reference chips of {SIDE}^2 in '
          f'{(len(idx) + BATCH - 1) // BATCH} batches of {BATCH}; one warm-up round, then {ROUNDS} interleaved rounds', flush=True)
    for r in range(ROUNDS + 1):
        for n in names:
            t, res[n] = timed(lambda: run(n))
            if r:
                times[n].append(t)
    print('wall time of one whole scene (host clock around predict_series_scene, device synchronised before and after):', flush=True)
    for n in names:
        print(line(n, times[n]), flush=True)
    base = times[names[0]]
    bmed, bspread = float(np.median(base)), max(base) - min(base)
    for n in names[1:]:
        med = float(np.median(times[n]))
        print(f'  [fig] {n}: {bmed / med:.2f}x the default path (medians); gain {1e3 * (bmed - med):.3f} ms against the baseline\'s min-max spread '
              f'{1e3 * bspread:.3f} ms -> {"beyond" if bmed - med > bspread else "within"} the spread', flush=True)
    print(f'  maps: unfused eager == default {np.array_equal(res[names[1]], res[names[0]])}, unfused replayed == default '
          f'{np.array_equal(res[names[2]], res[names[0]])}, fused vs default max |diff| {np.abs(res[names[3]] - res[names[0]]).max():.3e} '
          f'(map max {np.abs(res[names[0]]).max():.3f}); replaying: {[plans[n].replaying for n in names[2:]]}; fused layers {plans[names[3]].fused_layers}', flush=True)


def step(F, B=64, H=64, W=64):
    td, dev = torch.bfloat16, 'cuda'
    g = torch.Generator(device='cpu').manual_seed(F)
    npix = B * H * W
    hp = (torch.randn(B, H, W, F, generator=g) * 0.5).to(td).to(dev)
    xg = (torch.randn(B, H, W, 4 * F, generator=g) * 0.8).to(td).to(dev)
    cp = torch.randn(npix, F, generator=g).to(dev)
    k = (torch.randn(3, 3, F, 4 * F, generator=g) / np.sqrt(9 * F)).to(dev)
    perm = torch.from_numpy(li.gate_order(F)).to(dev)
    w_nat, _ = ops.pack_weights(k, F, BF16, want_dgrad=False)
    w_perm, _ = ops.pack_weights(k.index_select(3, perm), F, BF16, want_dgrad=False)
    xg_perm = xg.index_select(3, perm).contiguous()
    hg = torch.empty(B, H, W, 4 * F, dtype=td, device=dev)
    c_out = [torch.empty(npix, F, device=dev) for _ in range(2)]
    h_out = [torch.zeros(B, H, W, F, dtype=td, device=dev) for _ in range(2)]
    st = ops.stream_ptr()

    def pair(i):
        ops.conv2d(hp, w_nat, 4 * F, out=hg)
        d = LstmGatesDesc()
        d.xg, d.ldx, d.hg, d.ldh_g, d.c_prev = xg.data_ptr(), 4 * F, hg.data_ptr(), 4 * F, cp.data_ptr()
        d.c_out, d.h_out, d.ldh = c_out[0].data_ptr(), h_out[0].data_ptr(), F
        d.npix, d.filters, d.rec_act, d.act, d.dtype = npix, F, 0, 0, BF16
        check(lib.satcv_convlstm_gates_fwd(C.byref(d), st))

    def fused(i):
        d = LstmStepDesc()
        d.h_prev, d.ldh_prev, d.w, d.xg, d.ldx, d.c_prev = hp.data_ptr(), F, w_perm.data_ptr(), xg_perm.data_ptr(), 4 * F, cp.data_ptr()
        d.c_out, d.h_out, d.ldh = c_out[1].data_ptr(), h_out[1].data_ptr(), F
        d.n, d.h, d.w_, d.filters, d.rec_act, d.act, d.dtype = B, H, W, F, 0, 0, BF16
        check(lib.satcv_convlstm_step_fwd(C.byref(d), st))
    variants = {'conv2d + gates pair': pair, 'fused step (one launch)': fused}
    times = {v: [] for v in variants}
    for r in range(ROUNDS + 1):
        for v, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(LAUNCHES):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            if r:
                times[v].append(a.elapsed_time(b) * 1e-3 / LAUNCHES)
    bytes_pp = {'conv2d + gates pair': 36 * F, 'fused step (one launch)': 20 * F}
    flop = 2.0 * 9 * F * 4 * F * npix
    print(f'isolated step, bf16, F = {F}, {B} images of {H} x {W} ({LAUNCHES} back-to-back launches between two HIP events, per step; {ROUNDS} interleaved rounds):', flush=True)
    for v in variants:
        med = float(np.median(times[v]))
        print(line(v, times[v]) + f'   {bytes_pp[v]} B/pixel derived -> {bytes_pp[v] * npix / med / 1e12:.2f} TB/s, {flop / med / 1e12:.1f} TFLOP/s', flush=True)
    pm, fm = (float(np.median(times[v])) for v in variants)
    spread = max(times['conv2d + gates pair']) - min(times['conv2d + gates pair'])
    print(f'  [fig] F = {F}: fused / pair = {fm / pm:.3f} (medians); gain {1e3 * (pm - fm):.4f} ms against the pair\'s min-max spread {1e3 * spread:.4f} ms -> '
          f'{"beyond" if pm - fm > spread else "not beyond"} the spread; max |h fused - h pair| {(h_out[1].float() - h_out[0].float()).abs().max().item():.3e}', flush=True)


if __name__ == '__main__':
    what = sys.argv[1:] or ['scene', 'step']
    if 'step' in what:
        step(64)
        step(16)
    if 'scene' in what:
        scene()
