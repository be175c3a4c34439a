"""The comparator of tests/test_gpu_silhouette_edges.py, pinned on the CPU: the fp32 oracle (oracle/silhouette_port.py) against the
float64 rasteriser with margins (tests/silhouette_cases.py) on every scene, so that the GPU test can neither pass nor fail because
of the comparator.  Per scene and pose: ZERO winning-face disagreements outside the ambiguous pixels, the ambiguous share within
its cap (a condition, not a measurement: 2 % of the covered pixels where every Z > 0, 10 % for the scene that straddles Z = 0),
the oracle's alpha within the derived bound of the float64 alpha, and the hand-made scenes' stated outcomes for both rasterisers.
Run with -s to see the counts (they are printed per scene either way on failure)."""
import numpy as np
import pytest
import torch

import silhouette_cases as sc
from oracle import silhouette_port as sp

BODY_PARAMS = [(name, S) for S in (224, 256) for name in sc.BODY_CAMS]


def _compare(name, scene, cap):
    """-> list of per-pose dicts (p2f32, p2f64, amb, alpha32, ref); asserts the comparator's conditions"""
    verts, cam, faces, S = scene
    ndc = sc.project32(verts, cam, S)
    with np.errstate(all='ignore'):
        alpha32, p2f32 = sp.soft_silhouette(torch.from_numpy(verts), faces, torch.from_numpy(cam), S, return_pix_to_face=True)
    alpha32 = alpha32[:, 0].numpy()
    out = []
    for b in range(len(verts)):
        p64, amb, cand = sc.raster64(ndc[b], faces, S, return_candidates=True)
        covered = int((p64 >= 0).sum())
        diff = p2f32[b] != p64
        unexplained = int((diff & ~amb).sum())
        ref = sc.alpha64(ndc[b], faces, p64, S)
        same = (p2f32[b] == p64) & (p64 >= 0)
        err = np.abs(alpha32[b].astype(np.float64) - ref['alpha'])
        need = sc.needed_delta_constant(alpha32[b], ref, same)
        print(f'{name} S={S} pose {b}: covered {covered}, ambiguous {int(amb.sum())} ({int((amb & (p64 >= 0)).sum())} of them covered), '
              f'fp32 != float64 on {int(diff.sum())}, unexplained {unexplained}, alpha needs k_delta {need:.2f} of 8')
        assert unexplained == 0, (name, S, b, np.argwhere(diff & ~amb)[:8])
        assert int(amb.sum()) <= cap * max(covered, 1), (name, S, b, int(amb.sum()), covered)
        assert sc.is_candidate(cand, p2f32[b]).all()
        assert np.array_equal(p2f32[b] >= 0, alpha32[b] > 0)
        assert (err[same] <= ref['bound'][same]).all(), (name, S, b, float((err - ref['bound'])[same].max()), need)
        out.append(dict(p2f32=p2f32[b], p2f64=p64, amb=amb, alpha32=alpha32[b], ref=ref))
    return out


@pytest.mark.parametrize('name,S', BODY_PARAMS)
def test_oracle_fp32_vs_float64_body_scenes(name, S):
    scene = sc.body_scene(name, S)
    ndc = sc.project32(scene[0], scene[1], S)
    assert bool((ndc[..., 2] > 0).all()) == sc.ALL_Z_POSITIVE[name]
    res = _compare(name, scene, 0.02 if sc.ALL_Z_POSITIVE[name] else 0.10)
    cov = [int((r['p2f64'] >= 0).sum()) for r in res]
    # the scenes are what they claim to be
    if name == 'off':
        assert cov == [0, 0]
    elif name in ('left', 'right', 'top', 'bottom'):
        full = [int((r['p2f64'] >= 0).sum()) for r in _control(S)]
        assert all(0.2 * f < c < 0.9 * f for c, f in zip(cov, full)), (cov, full)     # a good part of the body is cut off
        p = np.stack([r['p2f64'] >= 0 for r in res])
        border = {'left': p[:, :, 0], 'right': p[:, :, -1], 'top': p[:, 0, :], 'bottom': p[:, -1, :]}[name]
        assert border.reshape(len(res), -1).any(1).all()              # the body does cross that border
    elif name == 'corner':
        p = np.stack([r['p2f64'] >= 0 for r in res])
        assert p[:, 0, :].any(1).all() and p[:, :, 0].any(1).all()    # two clamps at once
    elif name == 'third':
        rows = [np.nonzero((r['p2f64'] >= 0).any(1))[0] for r in res]
        assert all(r[0] == 0 and r[-1] >= S - 4 for r in rows)        # overflows the frame top and bottom: many strips, seams in the body
        assert min(sc.strips(ndc[b], S) for b in range(2)) >= 4
    elif name == 'close_1p2':
        assert max(cov) == S * S                                      # the frame fully covered: the whole image in 6 / 8 strips
        assert [sc.strips(ndc[b], S) for b in range(2)] == [-(-S * S // 8960)] * 2
    elif name == 'close_0p37':
        fz = ndc[0, :, 2][sc.body_faces()]
        assert ((fz.min(1) < 0) & (fz.max(1) > 0)).sum() > 100 and np.abs(ndc[..., :2]).max() > 1e3
    elif name == 'centre':
        assert max(sc.strips(ndc[b], S) for b in range(2)) == 2      # the regime of the older tests


_CONTROL = {}


def _control(S):
    if S not in _CONTROL:
        ndc = sc.project32(*sc.body_scene('centre', S)[:2], S)
        _CONTROL[S] = [dict(p2f64=sc.raster64(ndc[b], sc.body_faces(), S)[0]) for b in range(2)]
    return _CONTROL[S]


def test_oracle_fp32_vs_float64_hand_made_scenes():
    res = {name: _compare(name, fn(), 0.02)[0] for name, fn in sc.HAND_SCENES.items()}
    for key in ('p2f32', 'p2f64'):
        others = {n: r[key] for n, r in res.items()}
        for name, r in res.items():
            sc.check_expectation(name, r[key], r['alpha32'] if key == 'p2f32' else r['ref']['alpha'], others)
    # the non-finite faces change nothing, the parked vertices change nothing
    for name in ('big_triangle_far_parked', 'big_triangle_nonfinite'):
        assert np.array_equal(res[name]['p2f32'], res['big_triangle']['p2f32'])
        assert np.array_equal(res[name]['alpha32'], res['big_triangle']['alpha32'])
    # the winner of the interpenetrating pair changes along a line: both faces win large parts
    p = res['interpenetrating']['p2f64']
    assert (p == 0).sum() > 20000 and (p == 1).sum() > 20000 and (p >= 0).all()


def test_margins_flag_what_they_should():
    """the comparator's own edge cases: exact ties of identical faces are NOT ambiguous (lowest index), a pixel centre exactly on
    an edge IS, and so is a depth tie of two different faces"""
    v, cam, f, S = sc.scene_identical_faces()
    p, amb = sc.raster64(sc.project32(v, cam, S)[0], f, S)
    assert not amb[p == sc.TIE_PAIRS[0][0]][10:-10].all() and amb.sum() < 0.02 * (p >= 0).sum()
    v, cam, f, S = sc.scene_edge_through_centres()
    p, amb = sc.raster64(sc.project32(v, cam, S)[0], f, S)
    assert amb[60:121, sc.EDGE_COL].all() and amb[sc.VERTEX_PIXEL] and not amb[62:119, sc.EDGE_COL - 1].any()
    v, cam, f, S = sc.scene_interpenetrating()
    ndc = sc.project32(v, cam, S)[0].copy()
    ndc[:, 2] = ndc[0, 2]                       # both planes at one depth: every pixel is a depth tie of two different faces
    p, amb = sc.raster64(ndc, f, S)
    assert amb.all()


def test_comparator_notices_small_errors():
    """what a subtly wrong rasteriser would hand in, made from the fp32 oracle's own output: one box row lost at a strip seam (~40
    pixels of ~4400: about the 0.5 % the older tests allow), one column lost at a clamped border, one pixel with its neighbour's
    face, the higher index of two identical faces.  Every one of them must show as an unexplained disagreement."""
    S = 224
    verts, cam, faces, _ = sc.body_scene('centre', S)
    ndc = sc.project32(verts, cam, S)[1]
    p64, amb = sc.raster64(ndc, faces, S)
    good = sp.rasterize_nearest(ndc, faces, S, S)
    assert not ((good != p64) & ~amb).any()
    bx0, bx1, by0, by1 = sc.pixel_box(ndc, S)
    seam = by0 + 8960 // (bx1 - bx0 + 1)                         # first row of the kernel's second strip
    assert sc.strips(ndc, S) == 2 and (p64[seam - 1] >= 0).sum() > 20
    bad = good.copy()
    bad[seam - 1] = -1
    lost = int(((bad != p64) & ~amb).sum())
    assert lost > 20, lost
    # one pixel, its right-hand neighbour's face
    yx = np.argwhere((p64[:, :-1] >= 0) & (p64[:, 1:] >= 0) & (p64[:, :-1] != p64[:, 1:]) & ~amb[:, :-1])[50]
    bad = good.copy()
    bad[yx[0], yx[1]] = p64[yx[0], yx[1] + 1]
    assert ((bad != p64) & ~amb).sum() == 1
    # the last column of a pose cut by the right-hand border
    verts, cam, faces, _ = sc.body_scene('right', S)
    ndc = sc.project32(verts, cam, S)[0]
    p64, amb = sc.raster64(ndc, faces, S)
    bad = sp.rasterize_nearest(ndc, faces, S, S)
    bad[:, -1] = -1
    assert ((bad != p64) & ~amb).sum() > 10
    # identical faces: the higher index
    v, cam, f, S = sc.scene_identical_faces()
    ndc = sc.project32(v, cam, S)[0]
    p64, amb = sc.raster64(ndc, f, S)
    bad = np.where(p64 == sc.TIE_PAIRS[0][0], sc.TIE_PAIRS[0][1], p64)
    assert ((bad != p64) & ~amb).sum() > 1000
