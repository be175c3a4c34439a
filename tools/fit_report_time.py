#!/usr/bin/env python3
"""Time the two kernels of the fit report (csrc/report.hip) at B = 256 poses of 224 x 224.

    python tools/fit_report_time.py [--batch 256] [--out profiles/fit_report_time.json]

Device events around back-to-back launches after a warm-up.  Each kernel alternates, round by round, with a `torch` device copy
that moves the same number of bytes (read + written), so both see the same clocks and the same neighbours; the medians over the
rounds are reported.  k_sil_compare reads alpha + mask (8 B per pixel); k_fit_overlay reads alpha, mask and the three image planes
(20 B per pixel) and writes 3 B per pixel, with three joint sets drawn.  No threshold: the numbers are recorded for what they are."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def beside_copy(fn, nbytes, dev, rounds, reps):
    """median ms of fn and of a device copy moving nbytes (half read, half written), alternating"""
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)      # noqa: E731
    for _ in range(5):
        fn(); copy()
    torch.cuda.synchronize()
    k, c = [], []
    for _ in range(rounds):
        k.append(timed(fn, reps))
        c.append(timed(copy, reps))
    km, cm = statistics.median(k), statistics.median(c)
    return {'ms': km, 'ms_min': min(k), 'ms_max': max(k), 'bytes': nbytes, 'tb_per_s': nbytes / (km * 1e-3) / 1e12,
            'copy_ms': cm, 'copy_tb_per_s': nbytes / (cm * 1e-3) / 1e12, 'rounds': rounds, 'launches_per_round': reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'fit_report_time.json'))
    a = ap.parse_args()
    report = importlib.import_module('joint-regressor-refinement_amd.report')
    data = importlib.import_module('joint-regressor-refinement_amd.data')
    dev, B, S = 'cuda:0', a.batch, a.size
    g = torch.Generator(device=dev).manual_seed(0)
    alpha = torch.rand(B, S, S, device=dev, generator=g)
    mask = (torch.rand(B, S, S, device=dev, generator=g) > 0.5).float()
    image = torch.randn(B, 3, S, S, device=dev, generator=g)
    sets = [torch.rand(B, 17, 2, device=dev, generator=g) * S for _ in range(3)]
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    px = B * S * S
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'size': S}
    # the C ABI directly on buffers allocated once: the wrappers of report.py allocate and upload small tensors per call
    lib_mod = importlib.import_module('joint-regressor-refinement_amd._lib')
    lib, ptr, stream = lib_mod.load(), lib_mod.ptr, lib_mod.stream_ptr(dev)
    counts = torch.empty(B, 4, dtype=torch.int32, device=dev)
    mean, std = (torch.tensor(v, dtype=torch.float32, device=dev) for v in data.SPIN_NORMALIZE)
    j2d = torch.stack(sets).contiguous()

    def compare():
        lib_mod.check(lib.jrr_silhouette_compare(ptr(alpha), ptr(mask), B, S, S, 0.5, 0.8, ptr(counts), stream), 'silhouette_compare')

    def overlay():
        lib_mod.check(lib.jrr_fit_overlay(ptr(alpha), ptr(mask), ptr(image), ptr(mean), ptr(std), ptr(j2d), 3, B, S, 0.5, 0.8, 2.0, ptr(out),
                                          stream), 'fit_overlay')
    res['k_sil_compare'] = beside_copy(compare, 8 * px, dev, a.rounds, a.reps)
    res['k_fit_overlay'] = beside_copy(overlay, 23 * px, dev, a.rounds, a.reps)
    assert torch.equal(counts, report.silhouette_compare(alpha, mask))
    for k in ('k_sil_compare', 'k_fit_overlay'):
        r = res[k]
        print(f"{k:<14s} B={B} {S}x{S}: {r['ms']:.4f} ms ({r['ms_min']:.4f}-{r['ms_max']:.4f}), {r['bytes'] / 1e6:.1f} MB -> {r['tb_per_s']:.3f} TB/s; "
              f"a copy of as many bytes {r['copy_ms']:.4f} ms, {r['copy_tb_per_s']:.3f} TB/s")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
