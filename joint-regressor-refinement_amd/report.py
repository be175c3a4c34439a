"""The fit report: how well the refined meshes cover their masks, and pictures of it.

The reference renders the mesh before and after its 100 iterations and hands the render to `viz()`
(/root/reference/scripts/optimize.py:204-218, :268-274, viz at :28-74): `render > 0.5`, `mask_rcnn > 0.8`, the map
`mask + render == 1` with the 2-D joints scattered over it, one PNG per pose.  Here the comparison (jrr_silhouette_compare) and the
compositing (jrr_fit_overlay) run on the device over the whole batch; only the PNG encoder is host code, standard library only.

`--fit_report_mesh` adds what the reference had pytorch3d for: the fitted body itself, shaded, from the front and from the side
(jrr_vertex_normals, jrr_mesh_shade over the rasteriser's pix_to_face; include/jrr.h states the arithmetic).
"""
from __future__ import annotations

import ctypes
import hashlib
import math
import struct
import zlib
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, dist as jdist, engine as _engine

THR_RENDER, THR_MASK = 0.5, 0.8        # scripts/optimize.py:35,41


def _planes(t: torch.Tensor, name: str) -> torch.Tensor:
    """(B,S,S) or (B,1,S,S) float32 device tensor -> contiguous (B,h,w)"""
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f'{name}: expected a float32 device tensor (B,h,w) or (B,1,h,w), got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t.contiguous()


def _pair(alpha: torch.Tensor, mask: torch.Tensor):
    alpha, mask = _planes(alpha, 'alpha'), _planes(mask, 'mask')
    if alpha.shape != mask.shape or alpha.device != mask.device:
        raise ValueError(f'alpha {tuple(alpha.shape)} on {alpha.device} and mask {tuple(mask.shape)} on {mask.device} differ')
    return alpha, mask


def silhouette_compare(alpha: torch.Tensor, mask: torch.Tensor, thr_render: float = THR_RENDER, thr_mask: float = THR_MASK) -> torch.Tensor:
    """per pose the pixel counts {r & m, r | m, r, m} of r = alpha > thr_render, m = mask > thr_mask (strict, fp32): int32 (B,4)"""
    alpha, mask = _pair(alpha, mask)
    B, h, w = alpha.shape
    counts = torch.empty(B, 4, dtype=torch.int32, device=alpha.device)
    _lib.check(_lib.load().jrr_silhouette_compare(_lib.ptr(alpha), _lib.ptr(mask), B, h, w, float(thr_render), float(thr_mask),
                                                  _lib.ptr(counts), _lib.stream_ptr(alpha.device)), 'silhouette_compare')
    return counts


def iou_from_counts(counts: torch.Tensor) -> torch.Tensor:
    """intersection / union in float64; 1.0 where the union is empty (both silhouettes are empty and agree)"""
    inter, union = counts[:, 0].double(), counts[:, 1].double()
    return torch.where(union > 0, inter / union.clamp(min=1), torch.ones_like(union))


def silhouette_iou(alpha: torch.Tensor, mask: torch.Tensor, thr_render: float = THR_RENDER, thr_mask: float = THR_MASK) -> torch.Tensor:
    """intersection over union of the two thresholded silhouettes per pose: float64 (B)"""
    return iou_from_counts(silhouette_compare(alpha, mask, thr_render, thr_mask))


def fit_overlay(alpha: torch.Tensor, mask: torch.Tensor, image: Optional[torch.Tensor] = None, normalize=None,
                joints2d: Sequence[torch.Tensor] = (), radius: float = 2.0, thr_render: float = THR_RENDER,
                thr_mask: float = THR_MASK, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The picture of every pose: uint8 (B,S,S,3).  image (B,3,S,S) is the background (black without one); normalize = (mean, std)
    says it is the normalised SPIN crop and is undone; render only red, mask only blue, both green, each averaged with the
    background; joints2d: up to three (B,17,2) sets in the crop's pixel frame, drawn as discs of `radius` pixels in green (set 0: the
    target), yellow, magenta, a later set over an earlier one.  `out`: a caller-owned contiguous uint8 (B,S,S,3) tensor to write into."""
    alpha, mask = _pair(alpha, mask)
    B, S, S2 = alpha.shape
    dev = alpha.device
    if S != S2:
        raise ValueError(f'fit_overlay: square images, got {S} x {S2}')
    if image is not None:
        if tuple(image.shape) != (B, 3, S, S) or image.dtype != torch.float32 or image.device != dev:
            raise ValueError(f'image: expected float32 {(B, 3, S, S)} on {dev}, got {tuple(image.shape)} {image.dtype} on {image.device}')
        image = image.contiguous()
    mean = std = None
    if normalize is not None:
        if image is None:
            raise ValueError('fit_overlay: normalize without an image')
        mean = torch.tensor(normalize[0], dtype=torch.float32, device=dev)
        std = torch.tensor(normalize[1], dtype=torch.float32, device=dev)
        if mean.shape != (3,) or std.shape != (3,):
            raise ValueError('fit_overlay: normalize = (mean, std) of 3 values each')
    sets = list(joints2d)
    if len(sets) > 3:
        raise ValueError('fit_overlay: at most three joint sets')
    j2d = None
    if sets:
        for s in sets:
            if tuple(s.shape) != (B, 17, 2):
                raise ValueError(f'joints2d: expected (B,17,2) = {(B, 17, 2)}, got {tuple(s.shape)}')
        j2d = torch.stack([s.to(dev, torch.float32) for s in sets]).contiguous()
    if out is None:
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (B, S, S, 3) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out: expected a contiguous uint8 {(B, S, S, 3)} on {dev}')
    _lib.check(_lib.load().jrr_fit_overlay(_lib.ptr(alpha), _lib.ptr(mask), _lib.ptr(image), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(j2d),
                                           len(sets), B, S, float(thr_render), float(thr_mask), float(radius), _lib.ptr(out),
                                           _lib.stream_ptr(dev)), 'fit_overlay')
    return out


MESH_COLOUR = (0.65, 0.74, 0.86)       # the light blue SMPL fits are usually shown in
SIDE_GREY = 0.25                        # background of the side view
_ADJACENCY, _DEVICE_MESH = {}, {}


def _faces_np(faces) -> np.ndarray:
    if torch.is_tensor(faces):
        faces = faces.detach().cpu().numpy()
    faces = np.ascontiguousarray(np.asarray(faces))
    if faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or not np.issubdtype(faces.dtype, np.integer):
        raise ValueError(f'faces: expected an integer array (F,3), got {faces.dtype} {faces.shape}')
    return faces


def vertex_face_adjacency(faces, n_verts: int):
    """The faces at every vertex in CSR form: (adj_offset int32 [n_verts + 1], adj_face int32 [3 F]); the faces of vertex v are
    adj_face[adj_offset[v]:adj_offset[v + 1]] in ascending face index; a vertex no face names has an empty list.  Cached per faces
    array (by content)."""
    faces = _faces_np(faces)
    n_verts = int(n_verts)
    key = (hashlib.sha1(faces.astype(np.int64).tobytes()).hexdigest(), faces.shape[0], n_verts)
    if key not in _ADJACENCY:
        if n_verts < 1 or faces.min() < 0 or faces.max() >= n_verts:
            raise ValueError(f'faces: vertex indices outside [0, {n_verts})')
        flat = faces.reshape(-1).astype(np.int64)
        order = np.argsort(flat, kind='stable')                 # stable: within a vertex the corners stay in face order
        offset = np.zeros(n_verts + 1, dtype=np.int64)
        np.cumsum(np.bincount(flat, minlength=n_verts), out=offset[1:])
        _ADJACENCY[key] = (offset.astype(np.int32), (order // 3).astype(np.int32))
    return _ADJACENCY[key]


def _device_mesh(faces, n_verts: int, device):
    """(faces, adj_offset, adj_face) as int32 tensors on `device`, uploaded once per faces array and device"""
    faces = _faces_np(faces)
    offset, adj = vertex_face_adjacency(faces, n_verts)
    key = (hashlib.sha1(faces.astype(np.int64).tobytes()).hexdigest(), faces.shape[0], int(n_verts), str(torch.device(device)))
    if key not in _DEVICE_MESH:
        _DEVICE_MESH[key] = tuple(torch.from_numpy(np.ascontiguousarray(a.astype(np.int32))).to(device) for a in (faces, offset, adj))
    return _DEVICE_MESH[key]


def _verts(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 3 or t.shape[2] != 3 or t.shape[1] < 1 or t.dtype != torch.float32 or not t.is_cuda:
        raise ValueError(f'{name}: expected a float32 device tensor (B,V,3), got {tuple(t.shape)} {t.dtype} on {t.device}')
    return t.contiguous()


def vertex_normals(verts: torch.Tensor, faces) -> torch.Tensor:
    """pytorch3d's verts_normals_packed per pose: verts (B,V,3), faces (F,3) -> unit normals (B,V,3), the area-weighted sum of the
    face normals at each vertex (summed in ascending face index: reproducible); exactly zero at a vertex without faces"""
    verts = _verts(verts, 'verts')
    B, V, _ = verts.shape
    f_dev, off_dev, adj_dev = _device_mesh(faces, V, verts.device)
    normals = torch.empty_like(verts)
    _lib.check(_lib.load().jrr_vertex_normals(_lib.ptr(verts), _lib.ptr(f_dev), _lib.ptr(off_dev), _lib.ptr(adj_dev), B, V, f_dev.shape[0],
                                              _lib.ptr(normals), _lib.stream_ptr(verts.device)), 'vertex_normals')
    return normals


def mesh_shade(verts: torch.Tensor, cam: torch.Tensor, pix_to_face: torch.Tensor, faces, normals: Optional[torch.Tensor] = None,
               image: Optional[torch.Tensor] = None, normalize=None, colour=MESH_COLOUR, opacity: float = 1.0, ambient: float = 0.3,
               light=(0.0, 0.0, -1.0), out: Optional[torch.Tensor] = None, want_depth: bool = False, want_normals: bool = False,
               background: float = 0.0, status: Optional[torch.Tensor] = None):
    """The shaded mesh behind a pix_to_face map (engine.silhouette_pix_to_face of a render of `verts`, `cam`): uint8 (B,S,S,3).
    verts (B,V,3) in SMPL space, cam (B,3), pix_to_face (B,S,S) int32, faces (F,3); normals (B,V,3) default to vertex_normals(verts,
    faces).  image (B,3,S,S) / normalize = (mean, std) are the background as in fit_overlay, `background` the grey without an image.
    colour: base colour in [0, 1]; light: direction in view space (normalised here; default the headlight), two-sided.
    `out`: a caller-owned contiguous uint8 (B,S,S,3).  `status`: a caller-zeroed int32 tensor of one element; bit 0 = a face or vertex
    index outside the mesh, bit 1 = a degenerate face (both draw background).  With want_depth / want_normals the return value is
    (rgb, depth (B,S,S) or None, normal (B,S,S,3) or None): interpolated view depth (-1 on background) and unit view-space normal."""
    verts = _verts(verts, 'verts')
    B, V, _ = verts.shape
    dev = verts.device
    if not torch.is_tensor(pix_to_face) or pix_to_face.dim() != 3 or pix_to_face.shape[0] != B or pix_to_face.shape[1] != pix_to_face.shape[2] \
            or pix_to_face.dtype != torch.int32 or pix_to_face.device != dev:
        raise ValueError(f'pix_to_face: expected int32 (B,S,S) with B = {B} on {dev}')
    S = int(pix_to_face.shape[1])
    if S % 4 or not 4 <= S <= 256:
        raise ValueError(f'mesh_shade: image size {S}: a multiple of 4, at most 256')
    pix_to_face = pix_to_face.contiguous()
    if tuple(cam.shape) != (B, 3) or cam.dtype != torch.float32 or cam.device != dev:
        raise ValueError(f'cam: expected float32 {(B, 3)} on {dev}, got {tuple(cam.shape)} {cam.dtype} on {cam.device}')
    cam = cam.contiguous()
    if normals is None:
        normals = vertex_normals(verts, faces)
    elif tuple(normals.shape) != (B, V, 3) or normals.dtype != torch.float32 or normals.device != dev:
        raise ValueError(f'normals: expected float32 {(B, V, 3)} on {dev}')
    normals = normals.contiguous()
    f_dev = _device_mesh(faces, V, dev)[0]
    if image is not None:
        if tuple(image.shape) != (B, 3, S, S) or image.dtype != torch.float32 or image.device != dev:
            raise ValueError(f'image: expected float32 {(B, 3, S, S)} on {dev}, got {tuple(image.shape)} {image.dtype} on {image.device}')
        image = image.contiguous()
    mean = std = None
    if normalize is not None:
        if image is None:
            raise ValueError('mesh_shade: normalize without an image')
        mean = torch.tensor(normalize[0], dtype=torch.float32, device=dev)
        std = torch.tensor(normalize[1], dtype=torch.float32, device=dev)
        if mean.shape != (3,) or std.shape != (3,):
            raise ValueError('mesh_shade: normalize = (mean, std) of 3 values each')
    colour = [float(c) for c in colour]
    light = [float(x) for x in light]
    norm = math.sqrt(sum(x * x for x in light)) if len(light) == 3 else 0.0
    if len(colour) != 3 or not all(0.0 <= c <= 1.0 for c in colour):
        raise ValueError('mesh_shade: colour = 3 values in [0, 1]')
    if not (norm > 0.0 and math.isfinite(norm)):
        raise ValueError('mesh_shade: light = a non-zero direction of 3 values')
    if not (0.0 <= opacity <= 1.0 and 0.0 <= ambient <= 1.0):
        raise ValueError('mesh_shade: opacity and ambient in [0, 1]')
    if out is None:
        out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (B, S, S, 3) or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
        raise ValueError(f'out: expected a contiguous uint8 {(B, S, S, 3)} on {dev}')
    if status is not None and (status.dtype != torch.int32 or status.numel() != 1 or status.device != dev):
        raise ValueError(f'status: expected one int32 on {dev}')
    depth = torch.empty(B, S, S, device=dev) if want_depth else None
    nmap = torch.empty(B, S, S, 3, device=dev) if want_normals else None
    c3, l3 = (ctypes.c_float * 3)(*colour), (ctypes.c_float * 3)(*[x / norm for x in light])
    _lib.check(_lib.load().jrr_mesh_shade(_lib.ptr(verts), _lib.ptr(normals), _lib.ptr(f_dev), _lib.ptr(cam), _lib.ptr(pix_to_face),
                                          _lib.ptr(image), _lib.ptr(mean), _lib.ptr(std), B, V, f_dev.shape[0], S, c3, float(opacity),
                                          float(ambient), l3, float(background), _lib.ptr(out), _lib.ptr(depth), _lib.ptr(nmap),
                                          _lib.ptr(status), _lib.stream_ptr(dev)), 'mesh_shade')
    return (out, depth, nmap) if (want_depth or want_normals) else out


def side_view(verts: torch.Tensor, cam: torch.Tensor, degrees: float = 90.0, centre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The vertices that the SAME `cam` renders as the body seen from the side: verts (B,V,3) in SMPL space -> (B,V,3).  In view space
    (x, y, z) -> (-2x + cx, -2y + cy, 2z + cz) each pose is turned by `degrees` about the vertical axis through its centroid, so its
    distance from the camera stays what it was.  The view-space offsets from the centroid are d = (v - mean v) * (-2, -2, 2), exact in
    floating point; the result is v + ((R - I) d) * (-1/2, -1/2, 1/2), the map back to SMPL space, exact as well -- the camera's
    translation cancels.  A turn by 0 adds zeros: the identity bit for bit.  A torch op on the tensors' device; not differentiated
    through by anything here.  `centre` (B,1,3), default the centroid of `verts`: other points of the same bodies (their joints) are
    turned WITH the vertices by passing the vertices' centroid."""
    if verts.dim() != 3 or verts.shape[2] != 3 or not verts.is_floating_point():
        raise ValueError(f'verts: expected a floating-point (B,V,3), got {tuple(verts.shape)} {verts.dtype}')
    if tuple(cam.shape) != (verts.shape[0], 3) or cam.device != verts.device:
        raise ValueError(f'cam: expected {(verts.shape[0], 3)} on {verts.device}, got {tuple(cam.shape)} on {cam.device}')
    quarter = float(degrees) / 90.0
    if quarter == round(quarter):                                 # whole quarter turns: exact cosine and sine
        c, s = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(round(quarter)) % 4]
    else:
        c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    flip = verts.new_tensor([-2.0, -2.0, 2.0])
    if centre is None:
        centre = verts.mean(dim=1, keepdim=True)
    elif tuple(centre.shape) != (verts.shape[0], 1, 3) or centre.device != verts.device:
        raise ValueError(f'centre: expected {(verts.shape[0], 1, 3)} on {verts.device}, got {tuple(centre.shape)} on {centre.device}')
    d = (verts - centre) * flip
    turned = torch.stack([(c - 1.0) * d[..., 0] + s * d[..., 2], torch.zeros_like(d[..., 1]), (c - 1.0) * d[..., 2] - s * d[..., 0]], dim=-1)
    return verts + turned * verts.new_tensor([-0.5, -0.5, 0.5])


def frame_camera(verts: torch.Tensor, size: int, margin: float = 0.1) -> torch.Tensor:
    """A camera translation (B,3) that frames each pose of verts (B,V,3) in a size x size picture of the rasteriser, for meshes that
    come without a camera (`--eval_vertices`).  The rasteriser projects (include/jrr.h, jrr_mesh_shade step 1) X = -2x + cx,
    Y = -2y + cy, Z = 2z + cz, (u, v) = (F X / Z, F Y / Z) with F = 5000 / size, and the picture is |u|, |v| <= 1.  Rule, per pose, from
    the bounding box of its vertices [lo, hi]:
        cx = lo_x + hi_x, cy = lo_y + hi_y       the box's centre projects to the picture's centre
        E  = max(hi_x - lo_x, hi_y - lo_y)       the larger half extent in view units (the projection doubles x and y)
        cz = F E / (1 - margin) - 2 lo_z         the nearest vertex sits at depth Z0 = F E / (1 - margin)
    Every vertex then has Z >= Z0 > 0 and |X|, |Y| <= E, so |u|, |v| <= 1 - margin: all of them land inside the picture, and the larger
    extent fills (1 - margin) Z0 / (Z0 + 2 (hi_z - lo_z)) of it -- Z0 is tens of metres at F = 5000 / size, so nearly 1 - margin.  A pose of
    zero extent gets E = 1e-6.  Computed in float64, returned in the vertices' dtype on their device."""
    if verts.dim() != 3 or verts.shape[2] != 3 or not verts.is_floating_point():
        raise ValueError(f'verts: expected a floating-point (B,V,3), got {tuple(verts.shape)} {verts.dtype}')
    if not 0.0 <= float(margin) < 1.0 or int(size) < 1:
        raise ValueError(f'frame_camera: size {size} >= 1 and margin {margin} in [0, 1)')
    v = verts.detach().double()
    lo, hi = v.min(dim=1).values, v.max(dim=1).values
    F = 5000.0 / float(int(size))
    E = torch.maximum(hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1]).clamp(min=1e-6)
    cam = torch.stack([lo[:, 0] + hi[:, 0], lo[:, 1] + hi[:, 1], F * E / (1.0 - float(margin)) - 2.0 * lo[:, 2]], dim=1)
    return cam.to(verts.dtype)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def write_png(path: str, rgb) -> None:
    """an (H,W,3) uint8 array or tensor as an 8-bit RGB PNG, non-interlaced, filter 0 on every scanline (zlib and struct only)"""
    if torch.is_tensor(rgb):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.ascontiguousarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != np.uint8 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f'write_png: expected uint8 (H,W,3), got {rgb.dtype} {rgb.shape}')
    h, w = rgb.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)           # filter byte 0 + the scanline
    rows[:, 1:] = rgb.reshape(h, 3 * w)
    png = (b'\x89PNG\r\n\x1a\n' + _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
           + _chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + _chunk(b'IEND', b''))
    with open(path, 'wb') as f:
        f.write(png)


class FitReport:
    """`--fit_report DIR` of one run (scripts/optimize.py:204-218 before the loop, :268-274 after it, viz() at :28-74): per outer batch and
    shard the mesh is rendered with the poses as they stand, compared with the batch's mask, the regressed joints are projected.
    `before` and `after` each run a forward of their own on the batch's engine, so each sits where no later call reads the engine's
    most recent forward.  They take the driver's batch object: its engine, mask, poses, shard bounds and global batch.
    `mesh` (`--fit_report_mesh`): each render also reads the rasteriser's pix_to_face and rasterises the body once more turned by 90
    degrees (side_view), on the same engine and at the same place; the first poses of both views are written as one shaded picture."""

    def __init__(self, directory: str, n_images: int, mesh: bool = False):
        self.directory, self.n_images, self.mesh = directory, int(n_images), bool(mesh)
        self.last = None           # the run's `fit_report` return value: per-pose IoU of the last batch's shard

    def before(self, b):
        self.gt_j2d = b.gt_j2d     # the loop's own 2-D target (--reprojection), else the dataset's, else none
        if self.gt_j2d is None and 'gt_j2d' in b.full:
            self.gt_j2d = b.full['gt_j2d'][b.lo:b.hi].to(b.sil_mask.device).float().contiguous()
        self.n = max(0, min(self.n_images, b.eng.batch))
        self.sums = torch.zeros(4, dtype=torch.float64, device=b.sil_mask.device)     # IoU before / after, pixel error before / after
        self.iou, self.kept, self.kept_mesh = {}, {}, {}
        self._render('before', b)

    def after(self, b):
        self._render('after', b)
        jdist.all_reduce_sum_(self.sums)                                              # the one extra (32-byte) collective of --fit_report
        self._write(b)

    def record(self, b) -> dict:
        """the record's four fields (means over the GLOBAL batch); reads the sums back"""
        fs = self.sums.cpu().numpy() / b.B_global
        px = (fs[2], fs[3]) if self.gt_j2d is not None else (None, None)
        self.last = {'iou_before': self.iou['before'].cpu().numpy(), 'iou_after': self.iou['after'].cpu().numpy(), 'shard': (b.lo, b.hi)}
        return {'silhouette_iou_before': fs[0], 'silhouette_iou_after': fs[1], 'j2d_error_px_before': px[0], 'j2d_error_px_after': px[1]}

    def _render(self, when: str, b):
        k = ('before', 'after').index(when)
        joints, verts = b.eng.find_joints_forward(b.betas, x6d=b.x6d, return_verts=True)
        alpha = b.eng.silhouette_forward(verts, b.cam)
        if self.mesh:              # nothing below reads the engine's rasterisation: the second one may overwrite it
            n = self.n
            front = b.eng.silhouette_pix_to_face()
            turned = side_view(verts, b.cam)
            b.eng.silhouette_forward(turned, b.cam)
            side = b.eng.silhouette_pix_to_face()
            self.kept_mesh[when] = (b.cam[:n].clone(), verts[:n].clone(), front[:n].clone(), turned[:n].clone(), side[:n].clone())
        j2d = _engine.project_joints(joints, b.cam)
        self.iou[when] = iou_from_counts(silhouette_compare(alpha, b.sil_mask))
        self.sums[k] = self.iou[when].sum()
        if self.gt_j2d is not None:
            self.sums[2 + k] = (j2d - self.gt_j2d).norm(dim=-1).mean(-1).sum().double()
        self.kept[when] = (alpha[:self.n].clone(), j2d[:self.n].clone())

    def _write(self, b):
        """overlays of the shard's first poses: target joints green, initial yellow, refined magenta (the last on `after` only); under
        `--image_masks` over the 224 crop the SPIN network saw, de-normalised"""
        import os
        from .data import SPIN_NORMALIZE
        if self.n == 0:
            return
        os.makedirs(self.directory, exist_ok=True)
        n = self.n
        image = b.images['spin_image'][:n] if b.images is not None else None
        target = self.gt_j2d[:n] if self.gt_j2d is not None else torch.full_like(self.kept['before'][1], float('nan'))
        sets = {'before': [target, self.kept['before'][1]], 'after': [target, self.kept['before'][1], self.kept['after'][1]]}
        for when in ('before', 'after'):
            rgb = fit_overlay(self.kept[when][0], b.sil_mask[:n], image=image, normalize=SPIN_NORMALIZE if image is not None else None,
                              joints2d=sets[when]).cpu().numpy()
            for i in range(n):
                write_png(os.path.join(self.directory, f'b{b.it:04d}_p{b.lo + i:05d}_{when}.png'), rgb[i])
            if self.mesh:          # (S, 2S, 3): the front view over the crop (or black), the side view over grey
                cam, verts, front, turned, side = self.kept_mesh[when]
                faces = b.eng.model.faces
                left = mesh_shade(verts, cam, front, faces, image=image, normalize=SPIN_NORMALIZE if image is not None else None)
                right = mesh_shade(turned, cam, side, faces, background=SIDE_GREY)
                both = torch.cat([left, right], dim=2).cpu().numpy()
                for i in range(n):
                    write_png(os.path.join(self.directory, f'b{b.it:04d}_p{b.lo + i:05d}_{when}_mesh.png'), both[i])
