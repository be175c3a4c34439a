#!/usr/bin/env python3
"""Device-event time of one visibility query of a whole mesh (jrr_point_visibility: every vertex of the placed body against every
face) beside two yardsticks on the same GPU and the same meshes -- DESIGN.md section 3v:

    python tools/exp/visibility_time.py [--batches 16 256] [--reps 10] [--torch_poses 4] [--out profiles/visibility_time.json]

The synthetic body (6890 vertices, 13 776 faces: 94.9 M ray-face pairs per pose), every pose turned about the vertical by a random
angle, placed 4 m in front of the camera and given 0.5 mm of vertex noise.  HIP events around ONE call, two warm-up rounds, then `reps`
timed rounds in which the candidates ALTERNATE (visibility, winding, visibility, ...), the median and the spread (min, max), as
milliseconds per pose and as pairs per second.  Yardsticks: (1) jrr_mesh_winding on the same meshes and the same 6890 points -- the
same pair count, about a hundred vector instructions a pair; (2) the chunked torch float32 expression of the same decision
(`--torch_chunk` queries of one pose against all faces at a time), on `--torch_poses` poses.  Needs a GPU: it fails without one."""
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
MARGIN, DEPTH = 0.005, 4.0


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


def _torch_visibility(verts, faces, margin, chunk):
    """verts (n,V,3) float32, faces (F,3) int64 -> count (n,V) int32 of the faces that cross in front of each vertex, the faces that
    name it skipped; one pose and `chunk` queries at a time, the header's Moeller-Trumbore form"""
    out = torch.empty(verts.shape[:2], dtype=torch.int32, device=verts.device)
    for b in range(verts.shape[0]):
        a, bb, c = (verts[b, faces[:, k]][None] for k in range(3))             # (1,F,3)
        e1, e2 = bb - a, c - a
        q = -torch.cross(a, e1, dim=-1)
        e2q = _dot(e2, q)
        for s in range(0, verts.shape[1], chunk):
            p = verts[b, s:s + chunk, None]                                      # (P,1,3)
            idx = torch.arange(s, s + p.shape[0], device=verts.device)[:, None]
            h = torch.cross(p.expand(-1, faces.shape[0], -1), e2.expand(p.shape[0], -1, -1), dim=-1)
            det = _dot(e1, h)
            u, v, t = -_dot(a, h) / det, _dot(p, q) / det, e2q / det
            d = p[..., 2]
            hit = (torch.minimum(torch.minimum(1 - u - v, u), v) >= 0) & (t > 0) & (t * d < d - margin)
            hit &= (faces[None, :, 0] != idx) & (faces[None, :, 1] != idx) & (faces[None, :, 2] != idx)
            out[b, s:s + chunk] = hit.sum(1).int()
    return out


def _measure(eng, batch, a, dev, vt, faces_np):
    g = torch.Generator().manual_seed(batch)
    yaw = torch.rand(batch, generator=g, dtype=torch.float64) * 2 * np.pi
    R = torch.zeros(batch, 3, 3, dtype=torch.float64)
    R[:, 0, 0], R[:, 0, 2], R[:, 1, 1], R[:, 2, 0], R[:, 2, 2] = yaw.cos(), yaw.sin(), 1.0, -yaw.sin(), yaw.cos()
    place = torch.cat([torch.rand(batch, 1, 2, generator=g, dtype=torch.float64) * 0.6 - 0.3, torch.full((batch, 1, 1), DEPTH, dtype=torch.float64)], 2)
    verts = (torch.einsum('vc,bdc->bvd', vt, R) + place + torch.randn(batch, vt.shape[0], 3, generator=g, dtype=torch.float64) * 0.0005).float().to(dev)
    faces32 = torch.from_numpy(faces_np).to(dev)
    faces64 = faces32.long()
    K = torch.tensor([[1145.0, 0, 512.0], [0, 1145.0, 512.0], [0, 0, 1]], device=dev).repeat(batch, 1, 1)
    rect = torch.tensor([[0.0, 0.0, 1000.0, 1000.0]], device=dev).repeat(batch, 1)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    out = (torch.empty(batch, vt.shape[0], dtype=torch.int32, device=dev), torch.empty(batch, vt.shape[0], dtype=torch.uint8, device=dev))
    n_t = min(batch, a.torch_poses)
    got = {}

    def kernel():
        eng.point_visibility(verts, faces32, None, K, rect, MARGIN, 1, status, out=out)

    def winding():
        got['w'] = eng.mesh_winding(verts, faces32, verts, status)

    def expression():
        got['t'] = _torch_visibility(verts[:n_t], faces64, MARGIN, a.torch_chunk)
    times = {'kernel': [], 'winding': [], 'torch': []}
    for rep in range(a.reps + 2):                                               # the candidates alternate inside every round
        for fn, name in ((kernel, 'kernel'), (winding, 'winding')):
            t = _once(fn)
            if rep >= 2:
                times[name].append(t)
    for rep in range(a.torch_reps + 1):
        t = _once(expression)
        if rep >= 1:
            times['torch'].append(t)
    count, code = out
    V, F = int(vt.shape[0]), int(faces_np.shape[0])
    pairs = {'kernel': batch * V * F, 'winding': batch * V * F, 'torch': n_t * V * F}
    differs = count[:n_t] != got['t']
    res = {'batch': batch, 'points': V, 'faces': F, 'reps': a.reps, 'torch_reps': a.torch_reps, 'torch_poses': n_t, 'torch_chunk': a.torch_chunk,
           'status': int(status.item()), 'share_of_vertices_seen': float((code == 0).float().mean()), 'share_of_vertices_outside': float(((code & 2) != 0).float().mean()),
           'share_of_counts_that_differ_from_torch': float(differs.float().mean()),
           'share_of_bits_that_differ_from_torch': float(((count[:n_t] >= 1) != (got['t'] >= 1)).float().mean())}
    for name, v in times.items():
        res[name + '_us'] = float(np.median(v))
        res[name + '_us_min_max'] = [min(v), max(v)]
        res[name + '_pairs_per_s'] = pairs[name] / res[name + '_us'] * 1e6
    res['kernel_ms_per_pose'] = res['kernel_us'] / 1000.0 / batch
    res['winding_ms_per_pose'] = res['winding_us'] / 1000.0 / batch
    res['torch_ms_per_pose'] = res['torch_us'] / 1000.0 / n_t
    print(f'batch {batch}: visibility {res["kernel_us"] / 1000:.2f} ms ({min(times["kernel"]) / 1000:.2f} .. {max(times["kernel"]) / 1000:.2f}), '
          f'{res["kernel_ms_per_pose"]:.3f} ms per pose, {res["kernel_pairs_per_s"]:.3e} pairs/s;  mesh_winding {res["winding_us"] / 1000:.2f} ms '
          f'({min(times["winding"]) / 1000:.2f} .. {max(times["winding"]) / 1000:.2f}), {res["winding_pairs_per_s"]:.3e} pairs/s;  torch float32 on {n_t} poses '
          f'{res["torch_ms_per_pose"]:.1f} ms per pose, {res["torch_pairs_per_s"]:.3e} pairs/s;  seen {100 * res["share_of_vertices_seen"]:.1f} %, counts that differ '
          f'from torch {100 * res["share_of_counts_that_differ_from_torch"]:.3f} %')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[16, 256])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--torch_reps', type=int, default=2)
    ap.add_argument('--torch_poses', type=int, default=4)
    ap.add_argument('--torch_chunk', type=int, default=512)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'visibility_time.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('visibility_time.py measures on a GPU; none is visible')
    eng = importlib.import_module(PKG + '.engine')
    sm = importlib.import_module(PKG + '.smpl_model')
    dev = torch.device('cuda:0')
    model = sm.synthetic_smpl()
    vt = torch.from_numpy(np.asarray(model['v_template'], dtype=np.float64))
    faces_np = np.ascontiguousarray(np.asarray(model['faces']).astype(np.int32))
    res = {str(b): _measure(eng, b, a, dev, vt, faces_np) for b in a.batches}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
