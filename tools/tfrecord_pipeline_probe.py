"""Where the time of the TFRecord training input goes, for one batch of 64 records of 256 x 256 with 4 bands, one categorical
feature and a label (the solar notebook's shape):

  (a) host to_tuple + Dataset.batch of already parsed records (NumPy, one thread) -- the path every commit before the device
      pipeline had, and still the device=None path;
  (b) the device path, median of repeated batches after warm-up: the host fill of the pinned buffer (host clock), then -- between
      device events placed after that fill -- the upload of the stacked planes and the parameter table, and the two launches of
      csrc/record_pipeline.hip alone, with their achieved bytes/s;
  (c) gzip + framing + parse alone through the reader get_dataset uses, at read_ahead 0 and 4.

    python tools/tfrecord_pipeline_probe.py [--out profiles/tfrecord_device_pipeline.txt]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from satellite_computervision_amd import tfrecord_io as tio      # noqa: E402

N, HW, BANDS = 64, 256, ['B2', 'B3', 'B4', 'B8']
FEATS = BANDS + ['lc']


def records(rng, n):
    out = []
    for _ in range(n):
        d = {b: (rng.random((HW, HW)) * 3000).astype(np.float32) for b in BANDS}
        d['lc'] = rng.integers(0, 2, (HW, HW)).astype(np.float32)
        d['landcover'] = rng.integers(0, 2, (HW, HW)).astype(np.float32)
        out.append(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures the device path: it needs the GPU'
    rng = np.random.default_rng(0)
    recs = records(rng, N)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    commit = 'unknown'
    p = os.path.join(ROOT, 'satellite_computervision_amd', '_build_commit.txt')
    if os.path.exists(p):
        commit = open(p).read().strip()
    say(f'tfrecord pipeline probe: batch {N} x {HW} x {HW}, {len(BANDS)} bands + 1 one-hot(2) feature + label one-hot(2); axes=[2]')
    pr = torch.cuda.get_device_properties(0)
    say(f'device {torch.cuda.get_device_name(0)} ({getattr(pr, "gcnArchName", "?")}, {pr.multi_processor_count} CUs, {pr.total_memory / 2**30:.0f} GiB); built at commit {commit}')

    # (a) host: to_tuple per record + batch (np.stack), parsed records given
    tio.set_seed(0)
    ts = []
    for i in range(6):
        t0 = time.perf_counter()
        ds = tio.Dataset(lambda: (tio.to_tuple(d, FEATS, {'landcover': 2}, [2], None, {'lc': 2}, None) for d in recs)).batch(N)
        xb, yb = next(iter(ds))
        if i:
            ts.append(time.perf_counter() - t0)
    say(f'(a) host to_tuple + batch, one thread: median {statistics.median(ts) * 1e3:.1f} ms per batch of {N} (min {min(ts) * 1e3:.1f}, 5 runs after 1 warm-up)')

    # (b) device: upload + two launches, events around them
    names, kinds = tio._record_planes(FEATS, {'landcover': 2}, {'lc': 2})
    planes = np.stack([np.stack([d[k] for k in names]) for d in recs])
    nband = len(BANDS)
    params = np.ones((N, 2 * nband + 3), np.float32)
    params[:, :2 * nband] = rng.uniform(0.95, 1.05, (N, 2 * nband))
    params[:, 2 * nband:2 * nband + 2] = rng.random((N, 2)) < 0.5
    params[:, 2 * nband + 2] = rng.integers(0, 4, N)
    stage = tio._PinnedStage()
    dev = torch.device('cuda', 0)
    fill, up, kern = [], [], []
    for i in range(a.reps + 5):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t0 = time.perf_counter()
        fp, fq = stage.fill(planes), stage.fill(params)
        t1 = time.perf_counter()
        e0.record()
        dp, dq = stage.send(fp, dev), stage.send(fq, dev)
        e1.record()
        x, y, _ = tio.device_to_tuple(dp, kinds, dq)
        e2.record()
        e2.synchronize()
        if i >= 5:
            fill.append((t1 - t0) * 1e3)
            up.append(e0.elapsed_time(e1))
            kern.append(e1.elapsed_time(e2))
    nx, ny = x.shape[3], y.shape[3]
    moved = planes.nbytes * (1 + nband / planes.shape[1]) + (nx + ny) * N * HW * HW * 4       # planes read once + bands again for the statistics, outputs written
    say(f'(b) device path, {a.reps} batches after 5 warm-up:')
    say(f'    satcv_record_stats + satcv_record_to_tuple (events around the launches): median {statistics.median(kern):.3f} ms (min {min(kern):.3f}) = '
        f'{moved / statistics.median(kern) / 1e6:.0f} GB/s of {moved / 1e6:.0f} MB moved (tools/bw_probe.py gives the copy bandwidth of the same box class)')
    say(f'    upload of {planes.nbytes / 1e6:.0f} MB from pinned memory (events after the host fill): median {statistics.median(up):.3f} ms (min {min(up):.3f}) = '
        f'{planes.nbytes / statistics.median(up) / 1e6:.1f} GB/s')
    say(f'    host fill of the pinned buffer (NumPy copy, host clock): median {statistics.median(fill):.1f} ms (min {min(fill):.1f})')
    t0 = time.perf_counter()
    for _ in range(3):
        np.stack([np.stack([d[k] for k in names]) for d in recs])
    say(f'    host stacking of the {N} parsed records into (n, k, h, w) (Dataset.batch): {(time.perf_counter() - t0) / 3 * 1e3:.1f} ms')
    err = float(np.abs(x.cpu().numpy()[..., nband:] - 0.5).max())
    assert err == 0.5, 'one-hot channels must be 0 / 1'

    # (c) gzip + framing + parse, read_ahead 0 and 4, over 4 files of 16 records
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for f in range(4):
            path = os.path.join(td, f'p{f}.tfrecord.gz')
            with tio.TFRecordWriter(path, compression='GZIP') as w:
                for d in recs[f * 16:(f + 1) * 16]:
                    w.write(tio.encode_example({k: v.reshape(-1) for k, v in d.items()}))
            paths.append(path)
        ft = {k: tio.FixedLenFeature([HW, HW]) for k in FEATS + ['landcover']}
        for ra in (0, 4):
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                cnt = sum(1 for _ in tio._parsed_records(paths, ft, ra))
                ts.append(time.perf_counter() - t0)
                assert cnt == N
            say(f'(c) gzip + CRC + parse of {N} records in 4 files, read_ahead={ra}: median {statistics.median(ts) * 1e3:.1f} ms (min {min(ts) * 1e3:.1f}, 3 runs)')
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, 'w').write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
