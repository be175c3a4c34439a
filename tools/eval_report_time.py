#!/usr/bin/env python3
"""Device-event times of jrr_evaluate and of the evaluation report's three launches at B = 4096:

    python tools/eval_report_time.py [--batch 4096] [--reps 50] [--out profiles/eval_report_time.json]

jrr_evaluate, jrr_evaluate_joints, jrr_regress_joints (the shipped 62-entry regressor and a dense one, n_reg = 1 and 2) and jrr_eval_accumulate,
each ALTERNATING with a torch device copy of as many bytes as the launch reads and writes (the copy reads and writes that many
bytes each, so its time is an upper bound of the memory floor).  Bytes and FLOP are computed here from the shapes.  Needs a GPU: it
fails without one."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = 'joint-regressor-refinement_amd'
NJ, NV = 17, 6890


def timed_pair(fn, nbytes, reps, dev):
    """median ms of fn and of a device copy of nbytes, alternating"""
    src = torch.empty(max(nbytes, 4) // 4, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    for _ in range(5):
        fn()
        dst.copy_(src)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for a, b, c in ev:
        a.record()
        fn()
        b.record()
        dst.copy_(src)
        c.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b, _ in ev])), float(np.median([b.elapsed_time(c) for _, b, c in ev]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_report_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_report_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev, B = torch.device('cuda:0'), a.batch
    g = torch.Generator().manual_seed(0)
    pred = (torch.randn(B, NJ, 3, generator=g) * 0.3).to(dev)
    tgt = ((torch.randn(B, NJ, 3, generator=g) * 0.3) * 1000).to(dev)
    verts = (torch.randn(B, NV, 3, generator=g) * 0.4).to(dev)
    group = (torch.arange(B, dtype=torch.int32) % 15).to(dev)
    J_sparse = torch.from_numpy(sm.default_h36m_regressor()).float().to(dev)
    J_dense = (torch.rand(NJ, NV, generator=g) + 0.01).to(dev)
    err_j, err_pa_j = eng.evaluate_joints(pred, tgt)
    acc = torch.zeros(15 * 338 + 2, dtype=torch.int64, device=dev)
    rows = {}

    def add(name, fn, nbytes, flop):
        ms, ms_copy = timed_pair(fn, nbytes, a.reps, dev)
        rows[name] = {'ms': ms, 'ms_copy_same_bytes': ms_copy, 'bytes': nbytes, 'flop': flop,
                      'GB_per_s': nbytes / ms / 1e6, 'GFLOP_per_s': flop / ms / 1e6}
        print(f'{name:<28s} {ms:9.4f} ms   copy of {nbytes} B {ms_copy:9.4f} ms')

    add('evaluate', lambda: eng.evaluate(pred, tgt), B * (2 * NJ * 3 * 4 + 2 * 4), 0)
    add('evaluate_joints', lambda: eng.evaluate_joints(pred, tgt), B * (2 * NJ * 3 * 4 + 2 * NJ * 4), 0)
    add('eval_accumulate', lambda: eng.eval_accumulate(err_j, err_pa_j, group, 15, acc), B * (2 * NJ * 4 + 4), 0)
    for tag, J in (('sparse', J_sparse), ('dense', J_dense)):
        nnz = int((J > 0).sum())
        for n_reg in (1, 2):
            table = eng.JointRegressorTable(torch.stack([J] * n_reg))
            read = B * (NV * 3 * 4 if tag == 'dense' else nnz * n_reg * 12)        # dense: the whole mesh once; sparse: the gathered vertices
            add(f'regress_{tag}_n_reg{n_reg}', lambda t=table: t.regress(verts), read + B * n_reg * NJ * 3 * 4, 2 * 3 * nnz * n_reg * B)
    doc = {'batch': B, 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'rows': rows,
           'note': 'median of device-event times, each launch alternating with a device copy of as many bytes'}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print('wrote', a.out)


if __name__ == '__main__':
    main()
