#!/usr/bin/env python3
"""Time k_pose_export (csrc/export.hip) at B = 4096 poses: the one launch `--save_refined` adds per outer batch.

    python tools/refined_export_time.py [--batch 4096] [--out profiles/refined_export_time.json]

Device events around back-to-back launches after a warm-up.  Every launch of a round writes rows of its own (shuffled indices into a
table of reps x B rows, zeroed between the rounds outside the timed region), as the driver's launches do: a launch onto rows that are
already marked would raise status bit 1 from every pose.  The kernel alternates, round by round, with a `torch` device copy that
moves the same number of bytes (664 B read with seven extras + 960 B written per pose); medians over the rounds are reported.  No
threshold: the number is recorded for what it is."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'refined_export_time.json'))
    a = ap.parse_args()
    lib_mod = importlib.import_module('joint-regressor-refinement_amd._lib')
    lib, ptr, dev, B, n_extra = lib_mod.load(), lib_mod.ptr, 'cuda:0', a.batch, 7
    stream = lib_mod.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    x6d = torch.randn(B, 24, 6, device=dev, generator=g)
    betas, cam, extra = (torch.randn(B, k, device=dev, generator=g) for k in (10, 3, n_extra))
    n_rows = a.reps * B
    table = torch.zeros(n_rows, 240, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    index = [(torch.randperm(B, device=dev, generator=g) + r * B).contiguous() for r in range(a.reps)]
    nbytes = B * (576 + 40 + 12 + 8 + 4 * n_extra + 960)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)

    def export(r):
        lib_mod.check(lib.jrr_pose_export(ptr(x6d), ptr(betas), ptr(cam), ptr(extra), n_extra, ptr(index[r]), ptr(table), n_rows, ptr(status), B,
                                          stream), 'pose_export')

    def timed(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for r in range(a.reps):
            fn(r)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / a.reps

    k, c = [], []
    for rnd in range(a.rounds + 1):                  # round 0 warms up
        table.zero_()
        tk, tc = timed(export), timed(lambda r: dst.copy_(src))
        if rnd:
            k.append(tk); c.append(tc)
    assert int(status.item()) == 0 and int((table[:, 229] == 1).sum().item()) == n_rows
    km, cm = statistics.median(k), statistics.median(c)
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'n_extra': n_extra,
           'k_pose_export': {'ms': km, 'ms_min': min(k), 'ms_max': max(k), 'bytes': nbytes, 'tb_per_s': nbytes / (km * 1e-3) / 1e12,
                             'copy_ms': cm, 'copy_tb_per_s': nbytes / (cm * 1e-3) / 1e12, 'rounds': a.rounds, 'launches_per_round': a.reps}}
    r = res['k_pose_export']
    print(f"k_pose_export B={B}: {r['ms']:.4f} ms ({r['ms_min']:.4f}-{r['ms_max']:.4f}), {nbytes / 1e6:.2f} MB -> {r['tb_per_s']:.3f} TB/s; "
          f"a copy of as many bytes {r['copy_ms']:.4f} ms, {r['copy_tb_per_s']:.3f} TB/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
