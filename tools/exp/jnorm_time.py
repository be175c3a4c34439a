#!/usr/bin/env python3
"""Device-event time of one reweighted moments pass (jrr_jfit_norm_moments, INV mode) beside one plain moments pass (jrr_jfit_moments)
on the same table -- DESIGN.md, "The MPJPE solve":

    python tools/exp/jnorm_time.py [--rows 65536] [--reps 15] [--rings-ns 380] [--out profiles/jnorm_time.json]

The table: `rows` synthetic samples with the shipped regressor's support (62 entries on 58 vertices), random vertices of body size and
ground truth, as tools/exp/jmom_time.py -- neither time depends on the values.  HIP events around ONE call of each over all rows,
alternating in the same process; two warm-up rounds of each, then `reps` timed rounds; the median and the spread (min, max), in
microseconds.  The weights are uploaded once, outside the timed region; the call's own read-back of the 17 counts (one stream
synchronisation) is inside it.  `--rings-ns N` (0: off) does the same on a second table whose support is N random vertices dealt to the 17
rows in turn (what `--fit_rings 1` makes of the shipped support is about 380 vertices, 25 entries a row).  Needs a GPU: it fails
without one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
NJ, NV = 17, 6890


def _table(eng, J, rows, dev, g):
    fit = eng.RegressorFit(J, None, rows)
    fit.cache[:, :3 * fit.ns] = (torch.randn(rows, 3 * fit.ns, generator=g) * 0.3).to(dev)
    gt = torch.randn(rows, NJ, 3, generator=g) * 300
    fit.cache[:, 3 * fit.ns:3 * fit.ns + 3 * NJ] = (gt - gt[:, :1]).reshape(rows, -1).to(dev)
    return fit


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def _measure(eng, fit, rows, reps, dev):
    x = torch.zeros(NJ, 128, dtype=torch.float64, device=dev)
    for i, c in enumerate(fit.counts):
        if c:
            x[i, :c] = 1.0 / c
    times = {'norm': [], 'moments': []}
    for rep in range(reps + 2):                                      # alternating, so that neither owns the caches
        for name, fn in (('norm', lambda: fit.norm_moments(x, eng.NORM_INV, 1e-5, 0, rows)), ('moments', lambda: fit.moments(0, rows))):
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    K = [c + fit.counts[0] if c else 0 for c in fit.counts[1:]]
    items = sum(((k + 16) // 16) * ((k + 16) // 16 + 1) // 2 for k in K if k)
    W = fit.ns + NJ
    tiles = ((W + 15) // 16) * ((W + 15) // 16 + 1) // 2
    nbytes = rows * fit.row_floats * 4
    res = {'rows': rows, 'ns': fit.ns, 'entries': fit.entries, 'row_bytes': fit.row_floats * 4, 'reps': reps, 'K': K, 'items': items,
           'moments_tiles': tiles, 'bytes_per_pass': nbytes, 'mfma_per_pass': items * 3 * ((rows + 3) // 4),
           'useful_fp64_flop_per_pass': int(2 * 3 * rows * sum(k * (k + 1) // 2 + k for k in K))}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    res['norm_gbytes_per_s'] = nbytes / res['norm_us'] / 1e3
    print(f'{rows} rows, NS {fit.ns}, K up to {max(K)} ({items} items): norm pass {res["norm_us"]:.1f} us ({min(times["norm"]):.1f} .. '
          f'{max(times["norm"]):.1f}), moments pass ({tiles} tiles) {res["moments_us"]:.1f} us ({min(times["moments"]):.1f} .. '
          f'{max(times["moments"]):.1f}); {nbytes} bytes of rows, {res["norm_gbytes_per_s"]:.0f} GB/s')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--rings-ns', type=int, default=380)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jnorm_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('jnorm_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    J = torch.from_numpy(sm.default_h36m_regressor()).float().to(dev)
    res = {'shipped': _measure(eng, _table(eng, J, a.rows, dev, g), a.rows, a.reps, dev)}
    if a.rings_ns > 0:
        rng = np.random.RandomState(0)
        Jw = torch.zeros(NJ, NV)
        for k, c in enumerate(np.sort(rng.choice(NV, a.rings_ns, replace=False)).tolist()):
            Jw[k % NJ, c] = 1.0
        res['wide'] = _measure(eng, _table(eng, Jw.to(dev), a.rows, dev, g), a.rows, a.reps, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
