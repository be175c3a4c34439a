#!/usr/bin/env python3
"""Device-event time of one depth query (jrr_point_mesh_depth) beside a chunked torch float32 expression of the same formulas --
DESIGN.md section 3p:

    python tools/exp/depth_time.py [--batches 256 4096] [--reps 15] [--torch_reps 3] [--out profiles/depth_time.json]

The synthetic body (6890 vertices, 13 776 faces), every pose a rigidly moved copy with 0.5 mm of vertex noise; 51 points per pose: the
shipped regressor's joints and two copies displaced by 5 mm and 20 mm of noise (inside, near the skin, some outside -- the mix the report
sees).  HIP events around ONE call, two warm-up rounds, then `reps` timed rounds; the median and the spread (min, max) in microseconds, and
face-point pairs per second.  The torch expression evaluates the seven regions by `where` and the solid angle by `atan2` on (chunk, 51,
13 776) tensors, `--torch_chunk` poses at a time (about 110 MB of intermediates per pose); it is what a user without the kernel would
write, timed over the whole batch with its own, smaller number of rounds.  Needs a GPU: it fails without one."""
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
NP = 51


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def _dot(a, b):
    return (a * b).sum(-1)


def _torch_chunk(verts, faces, points):
    """verts (n,V,3), faces (F,3) int64, points (n,P,3) -> dist, wind (n,P) in float32 (the winding sum in float64)"""
    a, b, c = (verts[:, faces[:, k]][:, None] for k in range(3))           # (n,1,F,3)
    p = points[:, :, None]
    ab, ac = b - a, c - a
    A, B, C = a - p, b - p, c - p
    d1, d2, d3, d4, d5, d6 = -_dot(ab, A), -_dot(ac, A), -_dot(ab, B), -_dot(ac, B), -_dot(ab, C), -_dot(ac, C)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    in_a, in_b = (d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3)
    in_ab, in_c = (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6)
    in_ac, in_bc = (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)
    r = 1.0 / torch.where(in_ab, d1 - d3, torch.where(in_ac, d2 - d6, torch.where(in_bc, d43 + d56, va + vb + vc)))
    zero = torch.zeros_like(r)
    v = torch.where(in_ab, d1, torch.where(in_ac, zero, torch.where(in_bc, d56, vb))) * r
    u = torch.where(in_ab, zero, torch.where(in_ac, d2, torch.where(in_bc, d43, vc))) * r
    e = A + v[..., None] * ab + u[..., None] * ac
    at_b, at_c = ~in_a & in_b, ~in_a & ~in_b & ~in_ab & in_c
    dl = torch.where(in_a[..., None], A, torch.where(at_b[..., None], B, torch.where(at_c[..., None], C, e)))
    d2f = _dot(dl, dl)
    d2f = torch.where(torch.isnan(d2f), torch.full_like(d2f, float('inf')), d2f)
    la, lb, lc = _dot(A, A).sqrt(), _dot(B, B).sqrt(), _dot(C, C).sqrt()
    num = _dot(A, torch.cross(B, C, dim=-1))
    dn = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    omega = 2.0 * torch.atan2(num, dn)
    return d2f.min(dim=2).values.sqrt(), (omega.double().sum(dim=2) / (4.0 * np.pi)).float()


def _torch_depth(verts, faces, points, chunk):
    out = [_torch_chunk(verts[i:i + chunk], faces, points[i:i + chunk]) for i in range(0, verts.shape[0], chunk)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def _measure(eng, batch, reps, torch_reps, chunk, dev, vt, faces, Jn):
    g = torch.Generator().manual_seed(batch)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.linalg.det(q).sign()[:, None, None]
    verts = (torch.einsum('vc,bdc->bvd', vt, q) + torch.rand(batch, 1, 3, generator=g, dtype=torch.float64) * 0.6 - 0.3
             + torch.randn(batch, vt.shape[0], 3, generator=g, dtype=torch.float64) * 0.0005).float()
    j = torch.einsum('jv,bvc->bjc', Jn, verts.double())
    points = torch.cat([j, j + torch.randn(batch, 17, 3, generator=g, dtype=torch.float64) * 0.005,
                        j + torch.randn(batch, 17, 3, generator=g, dtype=torch.float64) * 0.020], dim=1).float()
    verts, points = verts.to(dev), points.to(dev).contiguous()
    faces32, faces64 = faces.to(dev), faces.long().to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    got = {}

    def kernel():
        got['k'] = eng.point_mesh_depth(verts, faces32, points, status)

    def expression():
        got['t'] = _torch_depth(verts, faces64, points, chunk)
    times = {'kernel': [], 'torch': []}
    for rep in range(reps + 2):
        t = _once(kernel)
        if rep >= 2:
            times['kernel'].append(t)
    for rep in range(torch_reps + 1):
        t = _once(expression)
        if rep >= 1:
            times['torch'].append(t)
    dist, wind, _ = got['k']
    tdist, twind = got['t']
    pairs = batch * NP * int(faces.shape[0])
    res = {'batch': batch, 'points': NP, 'faces': int(faces.shape[0]), 'vertices': int(vt.shape[0]), 'reps': reps, 'torch_reps': torch_reps,
           'torch_chunk': chunk, 'pairs': pairs, 'status': int(status.item()), 'outside_share': float((wind.abs() <= 0.5).float().mean()),
           'largest_distance_from_torch_m': float((dist - tdist).abs().max()), 'largest_winding_distance_from_torch': float((wind - twind).abs().max())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    res['kernel_pairs_per_s'] = pairs / res['kernel_us'] * 1e6
    res['torch_pairs_per_s'] = pairs / res['torch_us'] * 1e6
    print(f'batch {batch}: kernel {res["kernel_us"]:.1f} us ({min(times["kernel"]):.1f} .. {max(times["kernel"]):.1f}), {res["kernel_pairs_per_s"]:.3e} '
          f'pairs/s; torch float32 in chunks of {chunk} {res["torch_us"]:.1f} us ({min(times["torch"]):.1f} .. {max(times["torch"]):.1f}); distance '
          f'from torch {res["largest_distance_from_torch_m"]:.2e} m, winding {res["largest_winding_distance_from_torch"]:.2e}; '
          f'{100 * res["outside_share"]:.1f} % of the points outside')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--torch_reps', type=int, default=3)
    ap.add_argument('--torch_chunk', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'depth_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('depth_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    rr = importlib.import_module(PKG + '.regressor_report')
    dev = torch.device('cuda:0')
    model = sm.synthetic_smpl()
    vt = torch.from_numpy(np.asarray(model['v_template'], dtype=np.float64))
    faces = torch.from_numpy(np.asarray(model['faces']).astype(np.int32))
    Jn = torch.from_numpy(rr.normalised(sm.default_h36m_regressor()))
    res = {str(b): _measure(eng, b, a.reps, a.torch_reps, a.torch_chunk, dev, vt, faces, Jn) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
