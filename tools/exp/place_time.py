#!/usr/bin/env python3
"""Device-event time of `--place_refined`'s two per-pose launches beside torch expressions of the same arithmetic -- DESIGN.md section 3u:

    python tools/exp/place_time.py [--batches 256 4096] [--iters 10] [--points 6890] [--reps 15] [--out profiles/place_time.json]

jrr_place_translation (the linear start + `iters` Levenberg-Marquardt steps, fp64) at every batch, against what a user without the
kernel would write on the GPU: float64 tensors, the normal equations by broadcasting and sums over the joints, `torch.linalg.solve` on
the batched 3x3 systems, the accept / reject rule by `torch.where`, in a Python loop of `iters` steps.  jrr_project_points at `points`
points per pose, against the one-line fp32 torch expression.  Random bodies 2.5 .. 7 m in front of cameras with 5 px of noise; neither
time depends on the values.  HIP events around ONE call of each, alternating in the same process; two warm-up rounds of each, then
`reps` timed rounds; the median and the spread (min, max), in microseconds.  No threshold is set: the pass has no predecessor.
Needs a GPU: it fails without one."""
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
NJ = 17


def _once(fn):
    """microseconds between two events around fn()"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0


def _torch_cost(S, uv, f, c, t):
    P = S + t[:, None]
    r = f[:, None] * P[..., :2] / P[..., 2:] + c[:, None] - uv
    return (r * r).sum((1, 2)), (P[..., 2] > 0).all(1)


def _torch_place(joints, j2d, K, iters):
    """(B,3) float64: the linear start and `iters` damped Gauss-Newton steps with the kernel's accept / reject rule"""
    S, uv = joints.double(), j2d.double()
    f, c = torch.stack([K[:, 0, 0], K[:, 1, 1]], 1).double(), torch.stack([K[:, 0, 2], K[:, 1, 2]], 1).double()
    B = S.shape[0]
    ab = uv - c[:, None]
    rows = torch.zeros(B, NJ, 2, 3, dtype=torch.float64, device=S.device)
    rows[..., 0, 0], rows[..., 1, 1], rows[..., 2] = f[:, None, 0], f[:, None, 1], -ab
    rhs = ab * S[..., 2:] - f[:, None] * S[..., :2]
    A = torch.einsum('bjri,bjrk->bik', rows, rows)
    t = torch.linalg.solve(A, torch.einsum('bjri,bjr->bi', rows, rhs))
    cost, _ = _torch_cost(S, uv, f, c, t)
    lam = torch.full((B,), 1e-3, dtype=torch.float64, device=S.device)
    eye = torch.eye(3, dtype=torch.float64, device=S.device)
    for _ in range(iters):
        P = S + t[:, None]
        q = 1.0 / P[..., 2]
        r = f[:, None] * P[..., :2] * q[..., None] + c[:, None] - uv
        J = torch.zeros(B, NJ, 2, 3, dtype=torch.float64, device=S.device)
        J[..., 0, 0], J[..., 1, 1] = f[:, None, 0] * q, f[:, None, 1] * q
        J[..., 2] = -f[:, None] * P[..., :2] * (q * q)[..., None]
        H = torch.einsum('bjri,bjrk->bik', J, J)
        g = torch.einsum('bjri,bjr->bi', J, r)
        d = torch.linalg.solve(H + lam[:, None, None] * H * eye, -g)
        cn, front = _torch_cost(S, uv, f, c, t + d)
        accept = (cn < cost) & front
        t, cost = torch.where(accept[:, None], t + d, t), torch.where(accept, cn, cost)
        lam = torch.where(accept, (lam / 10).clamp_min(1e-7), (lam * 10).clamp_max(1e7))
    return t


def _torch_project(points, trans, K):
    t = trans.float()
    P = points + t[:, None]
    f, c = torch.stack([K[:, 0, 0], K[:, 1, 1]], 1), torch.stack([K[:, 0, 2], K[:, 1, 2]], 1)
    uv = f[:, None] * P[..., :2] / P[..., 2:] + c[:, None]
    return torch.where(P[..., 2:] > 0, uv, torch.full_like(uv, float('nan')))


def _measure(eng, batch, iters, points, reps, dev, g):
    joints = (torch.randn(batch, NJ, 3, generator=g) * torch.tensor([0.25, 0.45, 0.15])).to(dev)
    planted = torch.stack([torch.rand(batch, generator=g) * 3 - 1.5, torch.rand(batch, generator=g) * 3 - 1.5, torch.rand(batch, generator=g) * 4.5 + 2.5], 1)
    K = torch.zeros(batch, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = 1100 + 50 * torch.rand(batch, generator=g), 1150 + 50 * torch.rand(batch, generator=g)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 480 + 60 * torch.rand(batch, generator=g), 480 + 60 * torch.rand(batch, generator=g), 1
    K, planted = K.to(dev), planted.double().to(dev)
    j2d = (_torch_project(joints, planted, K) + 5 * torch.randn(batch, NJ, 2, generator=g).to(dev)).contiguous()
    verts = (torch.randn(batch, points, 3, generator=g) * torch.tensor([0.25, 0.45, 0.15])).to(dev)
    out = eng.place_translation(joints, j2d, K, None, iters)
    uv = torch.empty(batch, points, 2, device=dev)
    fns = (('place_translation', lambda: eng.place_translation(joints, j2d, K, None, iters, out=out)),
           ('torch_place', lambda: _torch_place(joints, j2d, K, iters)),
           ('project_points', lambda: eng.project_points(verts, planted, K, out=(uv, None))),
           ('torch_project', lambda: _torch_project(verts, planted, K)))
    times = {k: [] for k, _ in fns}
    for rep in range(reps + 2):                                      # alternating, so that none owns the caches
        for name, fn in fns:
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    ref = _torch_place(joints, j2d, K, iters)
    res = {'batch': batch, 'iters': iters, 'points': points, 'reps': reps, 'project_bytes': batch * points * 20,
           'largest_distance_from_torch_m': float((out[0] - ref).abs().max()),
           'largest_projection_distance_from_torch_px': float(torch.nan_to_num(uv - _torch_project(verts, planted, K)).abs().max())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
    res['project_gb_per_s'] = res['project_bytes'] / res['project_points_us'] / 1e3
    print(f'batch {batch}: place_translation ({iters} steps) {res["place_translation_us"]:.1f} us ({min(times["place_translation"]):.1f} .. '
          f'{max(times["place_translation"]):.1f}), torch {res["torch_place_us"]:.1f} us ({min(times["torch_place"]):.1f} .. {max(times["torch_place"]):.1f}), '
          f'distance {res["largest_distance_from_torch_m"]:.2e} m; project_points ({points} points) {res["project_points_us"]:.1f} us '
          f'({min(times["project_points"]):.1f} .. {max(times["project_points"]):.1f}) = {res["project_gb_per_s"]:.0f} GB/s, torch '
          f'{res["torch_project_us"]:.1f} us ({min(times["torch_project"]):.1f} .. {max(times["torch_project"]):.1f})')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--points', type=int, default=6890)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'place_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('place_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    res = {str(b): _measure(eng, b, a.iters, a.points, a.reps, dev, g) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
