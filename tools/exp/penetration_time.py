#!/usr/bin/env python3
"""Device-event time of one winding-number query of a whole mesh (jrr_mesh_winding: every vertex of the body, pushed 2 mm under the
skin, against every face) beside two yardsticks on the same GPU and the same meshes -- DESIGN.md section 3r:

    python tools/exp/penetration_time.py [--batches 16 256] [--reps 10] [--torch_poses 4] [--out profiles/penetration_time.json]

The synthetic body (6890 vertices, 13 776 faces: 94.9 M point-face pairs per pose), every pose a rigidly moved copy with 0.5 mm of
vertex noise.  HIP events around ONE call, two warm-up rounds, then `reps` timed rounds; the median and the spread (min, max), as
milliseconds per pose and as point-face pairs per second.  Yardsticks: (1) the chunked torch float32 expression of the same sum
(`--torch_chunk` points of one pose against all faces at a time, about 1.5 GB of intermediates; the Omega summed in float64), on
`--torch_poses` poses; (2) jrr_point_mesh_depth on the same meshes with its 64 points per pose -- that call finds the closest point as
well and splits the FACES over its 16 waves, where the winding kernel gives every wave all faces and a point to every lane.  Needs a
GPU: it fails without one."""
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
PUSH = 0.002


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


def _torch_winding(verts, faces, points, chunk):
    """verts (n,V,3), faces (F,3) int64, points (n,P,3) -> wind (n,P) float32; one pose and `chunk` points at a time"""
    out = torch.empty(points.shape[:2], dtype=torch.float32, device=verts.device)
    for b in range(verts.shape[0]):
        a, bb, c = (verts[b, faces[:, k]][None] for k in range(3))             # (1,F,3)
        for s in range(0, points.shape[1], chunk):
            p = points[b, s:s + chunk, None]
            A, B, C = a - p, bb - p, c - p
            la, lb, lc = _dot(A, A).sqrt(), _dot(B, B).sqrt(), _dot(C, C).sqrt()
            num = _dot(A, torch.cross(B, C, dim=-1))
            dn = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
            out[b, s:s + chunk] = ((2.0 * torch.atan2(num, dn)).double().sum(dim=1) / (4.0 * np.pi)).float()
    return out


def _measure(eng, rep_mod, batch, a, dev, vt, faces_np, sign):
    g = torch.Generator().manual_seed(batch)
    q, _ = torch.linalg.qr(torch.randn(batch, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.linalg.det(q).sign()[:, None, None]
    verts = (torch.einsum('vc,bdc->bvd', vt, q) + torch.rand(batch, 1, 3, generator=g, dtype=torch.float64) * 0.6 - 0.3
             + torch.randn(batch, vt.shape[0], 3, generator=g, dtype=torch.float64) * 0.0005).float().to(dev)
    faces32 = torch.from_numpy(faces_np).to(dev)
    faces64 = faces32.long()
    points = (verts + (-sign * PUSH) * rep_mod.vertex_normals(verts, faces_np)).contiguous()
    first64 = points[:, :64].contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    n_t = min(batch, a.torch_poses)
    got = {}

    def kernel():
        got['k'] = eng.mesh_winding(verts, faces32, points, status)

    def depth():
        got['d'] = eng.point_mesh_depth(verts, faces32, first64, status, want_face=False)

    def expression():
        got['t'] = _torch_winding(verts[:n_t], faces64, points[:n_t], a.torch_chunk)
    times = {'kernel': [], 'depth': [], 'torch': []}
    for fn, name, reps, warm in ((kernel, 'kernel', a.reps, 2), (depth, 'depth', a.reps, 2), (expression, 'torch', a.torch_reps, 1)):
        for rep in range(reps + warm):
            t = _once(fn)
            if rep >= warm:
                times[name].append(t)
    wind = got['k']
    V, F = int(vt.shape[0]), int(faces_np.shape[0])
    pairs = {'kernel': batch * V * F, 'depth': batch * 64 * F, 'torch': n_t * V * F}
    k = wind.abs().round()
    res = {'batch': batch, 'points': V, 'faces': F, 'reps': a.reps, 'torch_reps': a.torch_reps, 'torch_poses': n_t, 'torch_chunk': a.torch_chunk,
           'status': int(status.item()), 'mean_penetrating_vertices': float((k >= 2).sum(1).float().mean()), 'mean_thin_vertices': float((k == 0).sum(1).float().mean()),
           'largest_distance_from_an_integer': float((wind.abs() - k).abs().max()),
           'largest_distance_from_torch': float((wind[:n_t] - got['t']).abs().max()),
           'largest_distance_from_point_mesh_depth': float((wind[:, :64] - got['d'][1]).abs().max())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
        res[name + '_pairs_per_s'] = pairs[name] / res[name + '_us'] * 1e6
    res['kernel_ms_per_pose'] = res['kernel_us'] / 1000.0 / batch
    res['torch_ms_per_pose'] = res['torch_us'] / 1000.0 / n_t
    print(f'batch {batch}: kernel {res["kernel_us"] / 1000:.2f} ms ({min(times["kernel"]) / 1000:.2f} .. {max(times["kernel"]) / 1000:.2f}), '
          f'{res["kernel_ms_per_pose"]:.3f} ms per pose, {res["kernel_pairs_per_s"]:.3e} pairs/s;  point_mesh_depth with 64 points '
          f'{res["depth_us"] / 1000:.2f} ms, {res["depth_pairs_per_s"]:.3e} pairs/s;  torch float32 on {n_t} poses {res["torch_ms_per_pose"]:.1f} ms per pose, '
          f'{res["torch_pairs_per_s"]:.3e} pairs/s;  from torch {res["largest_distance_from_torch"]:.2e}, from the depth call '
          f'{res["largest_distance_from_point_mesh_depth"]:.2e}, from an integer {res["largest_distance_from_an_integer"]:.2e}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--torch_reps', type=int, default=2)
    ap.add_argument('--torch_poses', type=int, default=4)
    ap.add_argument('--torch_chunk', type=int, default=1024)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'penetration_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('penetration_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    rep_mod = importlib.import_module(PKG + '.report')
    pen = importlib.import_module(PKG + '.penetration_report')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev = torch.device('cuda:0')
    model = sm.synthetic_smpl()
    vt = torch.from_numpy(np.asarray(model['v_template'], dtype=np.float64))
    faces_np = np.ascontiguousarray(np.asarray(model['faces']).astype(np.int32))
    sign = pen.orientation(vt.numpy()[None], faces_np)
    res = {str(b): _measure(eng, rep_mod, b, a, dev, vt, faces_np, sign) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
