#!/usr/bin/env python3
"""Device-event times of jrr_bootstrap_sums:

    python tools/exp/bootstrap_time.py [--reps 20] [--out profiles/bootstrap_time.json]

Two shapes: 10^5 units x 10^4 replicates in one segment (a split resampled by frames), and 240 units x 10^4 replicates in 16 segments of
15 (a split resampled by sequences, per action).  Each launch ALTERNATES with the best torch expression of the same resample on the same
device -- torch.randint + index_select + sum, the replicates chunked so that the gathered rows fit in 1 GiB --, median of `--reps`
launches.  The draws differ (torch's generator is not Philox at this counter assignment), the work is the same: rep_count x sum of
the segment counts random 40-byte gathers.  The first launch of each shape is compared word for word with the numpy restatement of
tests/bootstrap_cases.py on its first two replicates.  Needs a GPU: it fails without one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
PKG = 'joint-regressor-refinement_amd'
CHUNK_BYTES = 1 << 30


def torch_resample(units, segments, R):
    """(n_seg,R,5) int64: randint + index_select + sum per segment, the replicates in chunks of at most CHUNK_BYTES of gathered rows"""
    out = torch.empty((len(segments), R, 5), dtype=torch.int64, device=units.device)
    for s, (begin, count) in enumerate(segments):
        if count == 0:
            out[s] = 0
            continue
        step = max(1, min(R, CHUNK_BYTES // (count * 40)))
        for r0 in range(0, R, step):
            n = min(step, R - r0)
            idx = torch.randint(begin, begin + count, (n * count,), device=units.device)
            out[s, r0:r0 + n] = units.index_select(0, idx).view(n, count, 5).sum(1)
    return out


def timed_pair(fn, other, reps):
    """median ms of fn and of other, alternating"""
    fn()
    other()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for a, b, c in ev:
        a.record()
        fn()
        b.record()
        other()
        c.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b, _ in ev])), float(np.median([b.elapsed_time(c) for _, b, c in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20, help='launches per median')
    ap.add_argument('--replicates', type=int, default=10000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bootstrap_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bootstrap_time.py measures on a GPU; none is visible')
    import bootstrap_cases as bc
    eng = importlib.import_module(PKG + '.engine')
    dev = torch.device('cuda:0')
    R = a.replicates
    shapes = {'frames_1e5_units_1_segment': (100000, [[0, 100000]]),
              'sequences_240_units_16_segments': (240, [[15 * s, 15] for s in range(16)])}
    rows = {}
    for name, (n_units, segments) in shapes.items():
        rs = np.random.RandomState(n_units)
        units_np = np.concatenate([rs.randint(1 << 20, 1 << 34, size=(n_units, 4), dtype=np.int64), rs.randint(1, 50, size=(n_units, 1), dtype=np.int64)], 1)
        units = torch.from_numpy(units_np).to(dev)
        max_word = int(units_np.max())
        out = torch.empty((len(segments), R, 5), dtype=torch.int64, device=dev)
        first = eng.bootstrap_sums(units, segments, 7, 0, R, max_word=max_word, out=out)[:, :2].cpu().numpy()
        assert np.array_equal(first, bc.bootstrap_sums(units_np, segments, 7, 0, 2)), name
        draws = R * sum(c for _, c in segments)
        ms, ms_torch = timed_pair(lambda: eng.bootstrap_sums(units, segments, 7, 0, R, max_word=max_word, out=out),
                                  lambda: torch_resample(units, segments, R), a.reps)
        rows[name] = {'units': n_units, 'segments': len(segments), 'replicates': R, 'draws': draws, 'ms': ms, 'ms_torch': ms_torch,
                      'draws_per_s': draws / ms * 1e3, 'draws_per_s_torch': draws / ms_torch * 1e3, 'gathered_GB_per_s': draws * 40 / ms / 1e6,
                      'table_bytes': n_units * 40}
        print(f'{name:<34s} {ms:10.3f} ms   torch {ms_torch:10.3f} ms   {draws / ms / 1e6:8.2f} G draws/s   ({draws * 40 / ms / 1e6:8.1f} GB/s gathered)')
    doc = {'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'rows': rows,
           'note': 'median of device-event times, each launch alternating with torch.randint + index_select + sum of the same resample'}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
