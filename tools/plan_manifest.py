"""What a plan launches and what it computes, as one JSON file -- to compare two checkouts of the package (a change of engine.py's lowering
that must not change a launch) on the same library:

    SATCV_LIB=<libsatcv.so> PYTHONPATH=<checkout A> python tools/plan_manifest.py --out a.json
    SATCV_LIB=<libsatcv.so> PYTHONPATH=<checkout B> python tools/plan_manifest.py --out b.json
    python tools/plan_manifest.py --compare a.json b.json [--baseline a2.json]
With --folded the same for plan_cases.FOLDED_CASES, the folded inference plans of fp8_infer.Fp8Plan (a change of its lowering); with
--series for plan_cases.SERIES_CASES, the inference passes of the ConvLSTM2D family (predict_on_device, lstm_infer's plans eager, replayed
and fused: a change of lstm_tools.convlstm_forward or of a plan's launch list).

For every case of tests/plan_cases.py (always the list beside THIS file; the package is the first one on the path):
  steps   (phase, label or null, work or null) of every step of plan.fwd and plan.bwd
  calls   one step under a recording wrapper around every lib.satcv_* entry point: (name, stream: main | side, the non-pointer
          fields of every ctypes structure argument, the non-pointer scalar arguments)
  hashes  training: three steps from a fixed seed, sha256 of pflat / gflat / sflat, of the first step's gflat and of the packed images,
          and the three losses; inference: sha256 of every output; a tape model (no `runtime`): no steps, sha256 of every variable
The import rows of the switch table (plan_cases.IMPORT_VARIANTS) run in a process each.  --compare holds steps, calls and hashes to
equality and the losses to rtol 1e-6 (a float atomic sum); with --baseline (further runs of checkout A) a case whose A runs differ among
themselves is held to equal steps and calls and to the largest loss difference between two A runs, and says so."""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(HERE, '..'))            # (behind PYTHONPATH: without one, the package of this checkout)


def _cases():
    spec = importlib.util.spec_from_file_location('plan_cases', os.path.join(HERE, '..', 'tests', 'plan_cases.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sha(t):
    import torch
    return hashlib.sha256(t.detach().contiguous().cpu().flatten().view(torch.uint8).numpy().tobytes()).hexdigest()


def _fields(s):
    """the non-pointer fields of a ctypes structure"""
    out = {}
    for name, typ in s._fields_:
        if typ in (C.c_void_p, C.c_char_p) or hasattr(typ, 'contents') or issubclass(typ, C._Pointer):
            continue
        v = getattr(s, name)
        out[name] = _fields(v) if isinstance(v, C.Structure) else ([_fields(e) if isinstance(e, C.Structure) else e for e in v] if isinstance(v, C.Array) else v)
    return out


class Recorder:
    """wraps every satcv_* entry point the library object has bound; `streams`: {handle: name} of the plan's side stream"""

    def __init__(self, lib):
        self.lib, self.calls, self.streams, self.orig = lib, [], {}, {}
        for name in [k for k in vars(lib) if k.startswith('satcv_')]:
            self.orig[name] = fn = getattr(lib, name)
            setattr(lib, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*args):
            last = args[-1] if args else None
            handle = last.value if isinstance(last, C.c_void_p) else last
            structs = [_fields(a._obj) for a in args if hasattr(a, '_obj') and isinstance(a._obj, C.Structure)]
            scalars = [a for a, t in zip(args, fn.argtypes or ()) if t not in (C.c_void_p, C.c_char_p) and not issubclass(t, C._Pointer)]
            self.calls.append([name, self.streams.get(handle, 'main') if handle else 'main', structs, scalars])
            return fn(*args)
        return call

    def restore(self):
        for name, fn in self.orig.items():
            setattr(self.lib, name, fn)


def run_case(case):
    import torch
    from satellite_computervision_amd import lstm_tools as lt, model_tools as mt, ops
    from satellite_computervision_amd._lib import lib
    saved = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    mt.set_compute_dtype(case.dtype)
    try:
        m, x, y = case.make(mt, lt)
        rt = getattr(m.unet if hasattr(m, 'unet') else m, 'runtime', None)
        rec = Recorder(lib)
        try:
            if rt is None:                     # a tape model (lstm_tools): no plan, no steps -- the calls of the second step, the weights
                losses = [m.train_on_batch(x, y)]
                rec.calls.clear()
                losses.append(m.train_on_batch(x, y))
                calls = list(rec.calls)
                rec.restore()
                losses.append(m.train_on_batch(x, y))
                torch.cuda.synchronize()
                hashes = {k: hashlib.sha256(v.tobytes()).hexdigest() for k, v in m.get_weights_dict().items()}
                return dict(steps=[], calls=calls, hashes=hashes, losses=[float(v) for v in losses])
            if case.training:
                losses = [m.train_on_batch(x, y)]
                torch.cuda.synchronize()
                plan = next(p for p in rt.plans.values() if p.training)
                rec.streams = {plan.side.cuda_stream: 'side'} if plan.side is not None else {}
                rec.calls.clear()
                g_first = _sha(rt.gflat)
                losses.append(m.train_on_batch(x, y))            # (the recorded step: plan and streams exist)
                calls = list(rec.calls)
                rec.restore()
                losses.append(m.train_on_batch(x, y))
                torch.cuda.synchronize()
                hashes = dict(pflat=_sha(rt.pflat), gflat=_sha(rt.gflat), sflat=_sha(rt.sflat), gflat_first=g_first,
                              packed=_sha(torch.cat([pk['fwd'].float().flatten() for pk in rt.packed.values()])))
            else:
                n, h, w = x.shape[:3]
                plan = rt.plan(n, h, w, False)
                plan.x_f32.copy_(torch.from_numpy(x))
                plan.run_forward(ops.stream_ptr())
                torch.cuda.synchronize()
                calls, losses = list(rec.calls), []
                hashes = {f'output{i}': _sha(plan.outputs[t.id]) for i, t in enumerate(m.outputs)}
        finally:
            rec.restore()
        steps = [[ph, getattr(s, 'label', None), getattr(s, 'work', None)] for ph, lst in (('fwd', plan.fwd), ('bwd', getattr(plan, 'bwd', []))) for s in lst]
        return dict(steps=steps, calls=calls, hashes=hashes, losses=[float(v) for v in losses])
    finally:
        mt.set_compute_dtype('bfloat16')
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_folded(case, made=None):
    """one Fp8Plan of a FoldedCase (made: what case.make returned, if the caller holds it): the calls of one run_forward (calibration and
    plan construction are not recorded) and its outputs"""
    import torch
    from satellite_computervision_amd import fp8_infer as fi, lstm_tools as lt, model_tools as mt, ops
    from satellite_computervision_amd._lib import lib
    m, x = made or case.make(mt, lt)
    n, h, w = (x[0] if isinstance(x, list) else x).shape[:3]
    q = fi.calibrate(m, x) if case.store == 'fp8' else None
    plan = fi.Fp8Plan(m, n, h, w, q, store=fi.FP8 if case.store == 'fp8' else fi.BF16, **case.plan_kw)
    m._stage_x(plan, x)
    rec = Recorder(lib)
    try:
        plan.run_forward(ops.stream_ptr())
        torch.cuda.synchronize()
    finally:
        rec.restore()
    return dict(steps=[], calls=rec.calls, hashes={f'output{i}': _sha(plan.outputs[t.id]) for i, t in enumerate(m.outputs)}, losses=[])


def record_pass(lib, fn):
    """-> (what fn() returned, the library calls it made)"""
    import torch
    rec = Recorder(lib)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        rec.restore()
    return res, rec.calls


def run_series(case):
    """the inference passes of a SeriesCase: the calls of every labelled pass behind a ['# label'] row, and the hashes of what it returned"""
    from satellite_computervision_amd import lstm_tools as lt, model_tools as mt
    from satellite_computervision_amd._lib import lib
    mt.set_compute_dtype(case.dtype)
    try:
        _, passes = case.make(mt, lt)
        calls, hashes = [], {}
        for label, fn in passes:
            if label is None:
                fn()
                continue
            res, made = record_pass(lib, fn)
            calls += [['# ' + label, 'main', [], []]] + made
            hashes.update({f'{label} / output{i}': _sha(t) for i, t in enumerate(res if isinstance(res, (list, tuple)) else [res])})
        return dict(steps=[], calls=calls, hashes=hashes, losses=[])
    finally:
        mt.set_compute_dtype('bfloat16')


def child_folded(out, only, series=False):
    import satellite_computervision_amd
    print('package:', os.path.dirname(satellite_computervision_amd.__file__), flush=True)
    pc = _cases()
    res = {}
    for c in [c for c in (pc.SERIES_CASES if series else pc.FOLDED_CASES) if not only or c.name in only]:
        res[c.name] = run_series(c) if series else run_folded(c)
        reach = [r[0] for r in res[c.name]['calls'] if r[0][0] == '#'] if series else dict(pc.folded_forms(res[c.name]['calls']))
        print(f"{c.name}: {len(res[c.name]['calls'])} calls, reaches {reach}", flush=True)
    json.dump(res, open(out, 'w'), indent=0, sort_keys=True)


def child(variant, out, only):
    pc = _cases()
    if variant:
        os.environ.update(pc.IMPORT_VARIANTS[variant])                 # (before the package is imported)
        cases = [c._replace(name=f'{pc.FIVE}[{variant}]') for c in pc.CASES if c.name == pc.FIVE]
    else:
        cases = pc.CASES
    import satellite_computervision_amd
    print('package:', os.path.dirname(satellite_computervision_amd.__file__), flush=True)
    res = {}
    for c in [c for c in cases if not only or c.name in only]:
        res[c.name] = run_case(c)
        labels = ' | '.join(s[1] or '' for s in res[c.name]['steps'])
        print(f"{c.name}: {len(res[c.name]['steps'])} steps, {len(res[c.name]['calls'])} calls, reaches {[s for s in pc.SUFFIXES if s in labels]}", flush=True)
    json.dump(res, open(out, 'w'))


def collect(out, only):
    pc = _cases()
    res = {}
    for variant in [''] + list(pc.IMPORT_VARIANTS):
        if only and not (set(only) & ({f'{pc.FIVE}[{variant}]'} if variant else {c.name for c in pc.CASES})):
            continue
        part = f'{out}.{len(res)}.part'
        subprocess.run([sys.executable, os.path.abspath(__file__), '--child', variant, '--out', part] + (['--cases', ','.join(only)] if only else []),
                       check=True, timeout=600)
        res.update(json.load(open(part)))
        os.remove(part)
    json.dump(res, open(out, 'w'), indent=0, sort_keys=True)
    labels = ' | '.join(s[1] or '' for r in res.values() for s in r['steps'])
    missing = [s for s in pc.SUFFIXES if s not in labels]
    print(f'{len(res)} cases written to {out}; label suffixes never reached: {missing or "none"}')
    return 3 if missing and not only else 0


def _diff(a, b):
    """what differs between two records of one case: [] or a list of part names (the losses to rtol 1e-6)"""
    bad = [k for k in ('steps', 'calls', 'hashes') if a[k] != b[k]]
    if len(a['losses']) != len(b['losses']) or not np.allclose(a['losses'], b['losses'], rtol=1e-6, atol=0):
        bad.append('losses')
    return bad


def _loss_gap(a, b):
    return float(np.abs(np.array(a['losses']) / np.array(b['losses']) - 1).max()) if a['losses'] else 0.0


def compare(fa, fb, fbase):
    a, b = json.load(open(fa)), json.load(open(fb))
    runs_a = [a] + [json.load(open(f)) for f in fbase or ()]
    rc = 0 if set(a) <= set(b) else 1
    print(f"{'case':34s} {'steps':>5s} {'calls':>5s}  manifest  hashes  note")
    for name in sorted(set(a) & set(b)):
        d, note = _diff(a[name], b[name]), ''
        others = [r[name] for r in runs_a[1:] if name in r]
        if any(_diff(a[name], o) for o in others):
            # two runs of A differ: B is held to equal steps and calls and to the largest loss difference seen between two runs of A
            allr = [a[name]] + others
            lim = max(_loss_gap(p, q) for i, p in enumerate(allr) for q in allr[i + 1:])
            gap = min(_loss_gap(b[name], p) for p in allr)
            note = f'{len(allr)} runs of A differ among themselves (losses by up to {lim:.1e}); B is within {gap:.1e} of one of them'
            d = [k for k in d if k in ('steps', 'calls')] + ([f'losses: {gap:.1e} > {lim:.1e}'] if gap > max(lim, 1e-6) else [])
        rc |= 1 if d else 0
        man = 'equal' if not {'steps', 'calls'} & set(d) else 'DIFFER'
        print(f"{name:34s} {len(b[name]['steps']):5d} {len(b[name]['calls']):5d}  {man:8s}  {'equal' if a[name]['hashes'] == b[name]['hashes'] else 'differ':6s}  {note}{' FAIL ' + str(d) if d else ''}")
    print('RESULT:', 'same launches, same numbers' if rc == 0 else 'DIFFERENT')
    return rc


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'))
    ap.add_argument('--baseline', nargs='+', help='further runs of checkout A')
    ap.add_argument('--cases', type=lambda v: v.split(','), help='only these cases (comma-separated names)')
    ap.add_argument('--folded', action='store_true', help='the folded inference cases (plan_cases.FOLDED_CASES), in this process')
    ap.add_argument('--series', action='store_true', help='the ConvLSTM2D inference cases (plan_cases.SERIES_CASES), in this process')
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(a.compare[0], a.compare[1], a.baseline))
    if a.folded or a.series:
        sys.exit(child_folded(a.out, a.cases, series=a.series))
    if a.child is not None:
        child(a.child, a.out, a.cases)
    else:
        sys.exit(collect(a.out, a.cases))
