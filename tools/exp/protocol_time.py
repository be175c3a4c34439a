#!/usr/bin/env python3
"""Device-event time of jrr_evaluate_protocol (one launch: masked per-joint errors + the table) beside the pair it stands next to,
jrr_evaluate_joints + jrr_eval_accumulate (two launches) -- DESIGN.md section 3t:

    python tools/exp/protocol_time.py [--batches 256 4096] [--rounds 9] [--launches 50] [--out profiles/protocol_time.json]

Body-sized random skeletons, the target a rotated, scaled, noisy copy in millimetres; 15 groups; no time depends on the values.  All
three candidates -- the protocol launch at `all17` and at `lsp14`, both with the table and both outputs, and the pair -- write into
buffers allocated once and are called through the C ABI directly, so the host does the same work for each.  HIP events around
`launches` back-to-back calls, the three alternating in the same process; two warm-up rounds, then `rounds` timed ones; per call the
median over the rounds and the spread (min, max), in microseconds.  No threshold is set: the default protocol keeps the pair.  Needs
a GPU: it fails without one."""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
NJ, N_GROUPS, ROW, TRAILER = 17, 15, 338, 2
MASKS = {'all17': 0x1FFFF, 'lsp14': 0x1FD7E}
P = ctypes.c_void_p


def _span(fn, launches):
    """microseconds per call between two events around `launches` calls of fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / launches


def _measure(lib, batch, rounds, launches, dev, g):
    pred = (torch.randn(batch, NJ, 3, generator=g) * torch.tensor([0.15, 0.5, 0.05])).to(dev)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g))
    gt = ((pred.cpu() @ q) * 1.1 + 0.02 * torch.randn(batch, NJ, 3, generator=g) + 0.2).mul(1000).to(dev)
    group = torch.randint(0, N_GROUPS, (batch,), generator=g, dtype=torch.int32).to(dev)
    e, pa = torch.empty(batch, NJ, device=dev), torch.empty(batch, NJ, device=dev)
    acc = torch.zeros(N_GROUPS * ROW + TRAILER, dtype=torch.int64, device=dev)
    stream = P(torch.cuda.current_stream(dev).cuda_stream)
    a = [P(t.data_ptr()) for t in (pred, gt, group, e, pa, acc)]

    def check(rc):
        if rc != 0:
            raise RuntimeError(lib.jrr_last_error().decode())

    def pair():
        check(lib.jrr_evaluate_joints(a[0], a[1], a[3], a[4], batch, stream))
        check(lib.jrr_eval_accumulate(a[3], a[4], a[2], batch, N_GROUPS, a[5], stream))

    def fused(mask):
        return lambda: check(lib.jrr_evaluate_protocol(a[0], a[1], 0, mask, 0, a[2], batch, N_GROUPS, a[3], a[4], a[5], stream))

    fns = (('pair', pair), ('protocol_all17', fused(MASKS['all17'])), ('protocol_lsp14', fused(MASKS['lsp14'])))
    times = {k: [] for k, _ in fns}
    for r in range(rounds + 2):                                      # alternating, so that none owns the caches
        for name, fn in fns:
            t = _span(fn, launches)
            if r >= 2:
                times[name].append(t)
    # the table of the fused launch at all17 is what jrr_eval_accumulate makes of the arrays that launch wrote (integers): fresh tables
    t_pair, t_fused = torch.zeros_like(acc), torch.zeros_like(acc)
    check(lib.jrr_evaluate_protocol(a[0], a[1], 0, MASKS['all17'], 0, a[2], batch, N_GROUPS, a[3], a[4], P(t_fused.data_ptr()), stream))
    check(lib.jrr_eval_accumulate(a[3], a[4], a[2], batch, N_GROUPS, P(t_pair.data_ptr()), stream))
    torch.cuda.synchronize()
    res = {'batch': batch, 'rounds': rounds, 'launches_per_round': launches, 'groups': N_GROUPS,
           'tables_differ_in_words': int((t_pair != t_fused).sum())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    print(f'batch {batch}: pair {res["pair_us"]:.2f} us ({min(times["pair"]):.2f} .. {max(times["pair"]):.2f}); protocol all17 '
          f'{res["protocol_all17_us"]:.2f} us ({min(times["protocol_all17"]):.2f} .. {max(times["protocol_all17"]):.2f}); lsp14 '
          f'{res["protocol_lsp14_us"]:.2f} us ({min(times["protocol_lsp14"]):.2f} .. {max(times["protocol_lsp14"]):.2f}); words of the all17 table '
          f'that differ from jrr_eval_accumulate of its own outputs: {res["tables_differ_in_words"]}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'protocol_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('protocol_time.py measures on a GPU; none is visible')
    lib = importlib.import_module(PKG + '._lib').load()
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    res = {str(b): _measure(lib, b, a.rounds, a.launches, dev, g) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
