#!/usr/bin/env python3
"""Time k_pose_smooth and k_pose_jitter (csrc/smooth.hip) at M = 100 000 positions, radius 6: what `--smooth_refined` launches once per
run on a table of that size.

    python tools/refined_smooth_time.py [--positions 100000] [--radius 6] [--out profiles/refined_smooth_time.json]

Device events around back-to-back launches after a warm-up.  The positions are runs of 500 consecutive frames over a shuffled table
(a row per position), as a dataset's cameras are.  The kernels alternate, round by round, with a `torch` device copy that moves the
same number of bytes (per position 640 B read -- 6-D values, betas, cam, marker, its `order` and `run` entries, each counted once,
without the halo rows a tile re-reads -- and 632 B written); medians over the rounds are reported.  No threshold: the number is
recorded for what it is."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--positions', type=int, default=100000)
    ap.add_argument('--radius', type=int, default=6)
    ap.add_argument('--sigma', type=float, default=2.0)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'refined_smooth_time.json'))
    a = ap.parse_args()
    eng = importlib.import_module('joint-regressor-refinement_amd.engine')
    refined = importlib.import_module('joint-regressor-refinement_amd.refined')
    dev, M = 'cuda:0', a.positions
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(M, 240, device=dev, generator=g)
    table[:, 229] = 1.0
    order = torch.randperm(M, device=dev, generator=g).to(torch.int32).contiguous()
    run = (torch.arange(M, device=dev) // 500).to(torch.int32).contiguous()
    w = torch.from_numpy(refined.smooth_weights(a.sigma, a.radius)).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = eng.pose_smooth(table, order, run, w, status)
    jit = eng.pose_jitter(table, order, run, status)
    nbytes = M * (640 + 632)
    nbytes_j = M * (588 + 4)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(a.reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / a.reps

    s, j, c = [], [], []
    for rnd in range(a.rounds + 1):                  # round 0 warms up
        ts = timed(lambda: eng.pose_smooth(table, order, run, w, status, out=out))
        tc = timed(lambda: dst.copy_(src))
        tj = timed(lambda: eng.pose_jitter(table, order, run, status, out=jit))
        if rnd:
            s.append(ts); c.append(tc); j.append(tj)
    assert int(status.item()) == 0 and bool(torch.isfinite(out[3]).all().item())
    sm, jm, cm = statistics.median(s), statistics.median(j), statistics.median(c)
    res = {'device': torch.cuda.get_device_name(0), 'positions': M, 'radius': a.radius, 'run_length': 500,
           'k_pose_smooth': {'ms': sm, 'ms_min': min(s), 'ms_max': max(s), 'bytes': nbytes, 'tb_per_s': nbytes / (sm * 1e-3) / 1e12,
                             'copy_ms': cm, 'copy_tb_per_s': nbytes / (cm * 1e-3) / 1e12, 'rounds': a.rounds, 'launches_per_round': a.reps},
           'k_pose_jitter': {'ms': jm, 'ms_min': min(j), 'ms_max': max(j), 'bytes': nbytes_j, 'tb_per_s': nbytes_j / (jm * 1e-3) / 1e12},
           'mean_delta_deg': float(np.nanmean(out[3].cpu().numpy()))}
    r = res['k_pose_smooth']
    print(f"k_pose_smooth M={M} radius {a.radius}: {r['ms']:.4f} ms ({r['ms_min']:.4f}-{r['ms_max']:.4f}), {nbytes / 1e6:.2f} MB -> "
          f"{r['tb_per_s']:.3f} TB/s; a copy of as many bytes {r['copy_ms']:.4f} ms, {r['copy_tb_per_s']:.3f} TB/s; k_pose_jitter {jm:.4f} ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
