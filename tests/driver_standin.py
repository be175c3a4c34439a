"""A recording stand-in that lets the real `optimize_pose_refiner()` run on the CPU: the engine, the body's upload, the engine module's
free functions and the kernels behind report.py / refined.py / data.py are replaced by fakes on CPU tensors.  A fake computes nothing:
it appends one line to LOG -- ordinal, name, the shapes and dtypes of its tensor arguments, its scalar arguments, a CRC over the name
and all of them -- and fills the tensors the real call writes with values drawn from that CRC, so whatever a call is handed
depends on every call that wrote it before.  The collectives (dist.all_reduce_sum_) and the bucket's read-back are logged too, and
`torch.arange(..., dtype=int64, device=...)`, which is how the driver makes the refined-pose table's row indices.

    result, log = run(['--batch_size', '6', ...])                      # in this process
    python tests/driver_standin.py TREE OUT.json [driver flags ...]   # in a process of its own, on the package of another tree
"""
import importlib
import json
import os
import sys
import tempfile
import zlib

import torch

PKG = 'joint-regressor-refinement_amd'
BASE_FLAGS = ['--synthetic', '--smpl_dir', '/nonexistent', '--j_regressor_init', '/nonexistent', '--device', 'cpu']
LOG = []
BODIES = {}
CREATED = {}               # data_ptr of an int64 arange -> the ordinal it was made at


def fill(t, seed):
    g = torch.Generator().manual_seed(seed & 0x7fffffff)
    if t.dtype.is_floating_point:
        t.copy_(torch.rand(t.shape, generator=g).to(t.dtype))
    else:
        t.copy_(torch.randint(0, 2, t.shape, generator=g).to(t.dtype))


def new(seed, *shape, dtype=torch.float32):
    t = torch.empty(*shape, dtype=dtype)
    fill(t, seed)
    return t


def record(name, tensors=(), outs=(), **scalars):
    """log one call; fill `outs`; -> the CRC (the seed of whatever else the fake returns)"""
    crc, desc = zlib.crc32(name.encode()), []
    for t in tensors:
        if t is None:
            desc.append('None')
            continue
        crc = zlib.crc32(t.detach().contiguous().numpy().tobytes(), crc)
        desc.append(f'{tuple(t.shape)}:{str(t.dtype)[6:]}')
    sc = ' '.join(f'{k}={v!r}' for k, v in scalars.items())
    crc = zlib.crc32(sc.encode(), crc)
    LOG.append(f'{len(LOG):04d} {name} [{" ".join(desc)}] {sc} crc={crc:08x}')
    for k, o in enumerate(outs):
        if o is not None:
            fill(o, crc + k)
    return crc


class FakeDeviceModel:
    def __init__(self, model, device='cpu', hint_vertices=None):
        self.device, self.faces = torch.device(device), model.get('faces')
        record('DeviceModel', hint=None if hint_vertices is None else len(hint_vertices))


class FakeEngine:
    J_SUPPORT_CAP = 128

    def __init__(self, model, batch, batch_norm=None, flags=0, device=None):
        self.model, self.device, self.batch, self.flags = model, model.device, int(batch), int(flags)
        self.sil = 32 * ((self.flags >> 16) & 15) or 224
        self._hist = None
        record('RefineEngine', batch=batch, batch_norm=batch_norm, flags=flags)

    # configuration
    def set_batch_norm(self, n):
        record('set_batch_norm', n=int(n))

    def set_j_regressor(self, J, mask=None):
        record('set_j_regressor', [J, mask])

    def set_pose_disc(self, flat):
        record('set_pose_disc', [flat])

    def set_shape_disc(self, flat):
        record('set_shape_disc', [flat])

    def set_reprojection(self, gt_j2d=None, cam=None, cam_m=None, cam_v=None):
        record('set_reprojection', [gt_j2d, cam, cam_m, cam_v])
        self._reproj = () if gt_j2d is None else (cam, cam_m, cam_v)

    def set_silhouette(self, mask=None, cam=None, cam_m=None, cam_v=None):
        record('set_silhouette', [mask, cam, cam_m, cam_v])
        self._sil = () if mask is None else (cam, cam_m, cam_v)

    def set_loss_history(self, records=0, every=10):
        record('set_loss_history', records=records, every=every)
        self._hist = torch.zeros(records, 5) if records > 0 else None

    def loss_history(self):
        record('loss_history')
        return self._hist

    def j_support_info(self):
        record('j_support_info')
        return [3] * 17, True

    def support_tiles(self):
        record('support_tiles')
        on = bool(self.flags & 128) and not self.flags & 16
        return on, 15 if on else 216

    def support_vertices(self):
        record('support_vertices')
        on = bool(self.flags & 128) and not self.flags & 16
        return on, 51 if on else 0

    # forwards: each overwrites the engine's most recent forward
    def find_joints_forward(self, betas, x6d=None, R=None, return_verts=False):
        crc = record('find_joints_forward', [betas, x6d, R], return_verts=return_verts)
        joints = new(crc, self.batch, 17, 3)
        return (joints, new(crc + 1, self.batch, 6890, 3)) if return_verts else joints

    def silhouette_forward(self, verts, cam):
        return new(record('silhouette_forward', [verts, cam]), self.batch, self.sil, self.sil)

    def camera_prefit(self, x6d, betas, gt_j2d, cam, n_steps=1000, lr=1e-2):
        return new(record('camera_prefit', [x6d, betas, gt_j2d, cam], [cam], n_steps=n_steps, lr=lr), self.batch)

    def _loop_state(self):
        terms = tuple(getattr(self, '_reproj', ())) + tuple(getattr(self, '_sil', ()))
        return list(terms) + [self._hist]

    def refine_run(self, x6d, betas, gt, m, v, step, lr, n_iters, sqerr=None, after_j_step=False):
        record('refine_run', [x6d, betas, gt, m, v, step, sqerr], [x6d, betas, m, v, sqerr] + self._loop_state(), lr=lr, n_iters=n_iters,
               after_j_step=after_j_step)
        step += n_iters

    def refine_run_j_steps(self, x6d, betas, gt, m, v, step, lr, n_iters, j_every, J, J_m, J_v, J_step, j_lr, mask=None, sqerr=None,
                           j_sqerr=None, after_j_step=False, reuse_forward=True):
        record('refine_run_j_steps', [x6d, betas, gt, m, v, step, J, J_m, J_v, J_step, mask, sqerr, j_sqerr],
               [x6d, betas, m, v, sqerr, J, J_m, J_v, j_sqerr] + self._loop_state(), lr=lr, n_iters=n_iters, j_every=j_every, j_lr=j_lr,
               after_j_step=after_j_step, reuse_forward=reuse_forward)
        step += n_iters
        J_step += n_iters // j_every

    def refine_aux_losses(self, pose_disc=True, shape_disc=False):
        crc = record('refine_aux_losses', pose_disc=pose_disc, shape_disc=shape_disc)
        return (new(crc, self.batch) if pose_disc else None), (new(crc + 1, self.batch) if shape_disc else None)

    def pose_disc_backward_params(self, x6d, target, dparams):
        return new(record('pose_disc_backward_params', [x6d, dparams], [dparams], target=target), self.batch)

    def shape_disc_backward_params(self, betas, target, dparams):
        return new(record('shape_disc_backward_params', [betas, dparams], [dparams], target=target), self.batch)

    def j_regressor_grad(self, x6d, betas, gt, sqerr=None, out=None, joints=None):
        out = out if out is not None else torch.empty(17, 6890)
        record('j_regressor_grad', [x6d, betas, gt], [out, sqerr, joints])
        return out

    def j_regressor_grad_support(self, x6d, betas, gt, out, sqerr=None, joints=None):
        record('j_regressor_grad_support', [x6d, betas, gt], [out, sqerr, joints])
        return out

    def j_step_apply(self, J, dJ, J_m, J_v, J_step, lr, mask=None):
        record('j_step_apply', [J, dJ, J_m, J_v, J_step, mask], [J, J_m, J_v], lr=lr)
        J_step += 1

    def j_step_apply_support(self, J, dJs, J_m, J_v, J_step, lr, mask=None):
        record('j_step_apply_support', [J, dJs, J_m, J_v, J_step, mask], [J, J_m, J_v], lr=lr)
        J_step += 1

    def find_joints_after_j_step(self, betas, x6d):
        return new(record('find_joints_after_j_step', [betas, x6d]), self.batch, 17, 3)


# ---- the engine module's free functions and the kernels behind report / refined / data ----
def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    record('adam_step', [p, g, m, v, step], [p, m, v], lr=lr)


def evaluate(pred, target):
    crc = record('evaluate', [pred, target])
    return new(crc, pred.shape[0]), new(crc + 1, pred.shape[0])


def project_joints(joints, cam):
    return new(record('project_joints', [joints, cam]), joints.shape[0], 17, 2)


def rodrigues_forward(aa):
    return new(record('rodrigues_forward', [aa]), aa.shape[0], 3, 3)


def pose_export(x6d, betas, cam, index, table, status, extra=None):
    crc = record('pose_export', [x6d, betas, cam, index, extra], index_created_at=CREATED.get(index.data_ptr()))
    rows = new(crc, index.shape[0], table.shape[1])
    rows[:, 229] = 1.0                                     # refined.MARKER: the row is stored
    table[index] = rows


def silhouette_compare(alpha, mask, thr_render=0.5, thr_mask=0.8):
    counts = new(record('silhouette_compare', [alpha, mask]), alpha.shape[0], 4, dtype=torch.int32)
    counts[:, 1] += 1                                      # the union is no smaller than the intersection
    return counts


def fit_overlay(alpha, mask, image=None, normalize=None, joints2d=(), **_):
    crc = record('fit_overlay', [alpha, mask, image] + list(joints2d), normalize=normalize)
    return new(crc, alpha.shape[0], alpha.shape[-1], alpha.shape[-1], 3, dtype=torch.uint8)


def image_crop(pixels, desc, bboxes, sizes=(224, 256), normalize=None, status=None):
    crc = record('image_crop', [pixels, desc, bboxes], sizes=tuple(sizes), normalize=normalize)
    return [new(crc + k, bboxes.shape[0], 3, n, n) for k, n in enumerate(sizes)]


def mask_prepare(masks):
    crc = record('mask_prepare', [masks])
    return new(crc, masks.shape[0], 1, *masks.shape[1:]), new(crc + 1, masks.shape[0], dtype=torch.bool)


class _ReadBackLogged(torch.Tensor):
    def cpu(self, *a, **k):
        record('read_back', [self.as_subclass(torch.Tensor)])
        return self.as_subclass(torch.Tensor).cpu(*a, **k)


def install(tree=None):
    """patch the package (of the repository at `tree`, default: this one) and torch; -> (optimize module, a function that undoes it)"""
    tree = tree or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if tree not in sys.path:
        sys.path.insert(0, tree)
    mod = lambda name: importlib.import_module(f'{PKG}.{name}')
    eng, opt, jdist, smpl, report, data = (mod(n) for n in ('engine', 'optimize', 'dist', 'smpl', 'report', 'data'))
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def smpl_to(self, device, hint_vertices=None):
        self.device, self.device_model = torch.device(device), FakeDeviceModel(self.model_np, device, hint_vertices)
        return self

    real_reduce, real_arange, real_body = jdist.all_reduce_sum_, torch.arange, mod('smpl_model').synthetic_smpl

    def synthetic_smpl(*a):           # a second of host arithmetic per run otherwise
        if a not in BODIES:
            BODIES[a] = real_body(*a)
        return BODIES[a]

    def all_reduce_sum_(t):
        record('all_reduce_sum_', [t], nbytes=t.numel() * t.element_size())
        return real_reduce(t)

    def arange(*a, **k):
        t = real_arange(*a, **k)
        if k.get('dtype') == torch.int64 and 'device' in k:
            CREATED[t.data_ptr()] = len(LOG)
            record('arange', [t])
        return t

    class Bucket(opt.SharedBucket):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.tail = self.tail.as_subclass(_ReadBackLogged)

    for obj, fakes in ((eng, (adam_step, evaluate, project_joints, rodrigues_forward, pose_export)), (report, (silhouette_compare, fit_overlay)),
                       (data, (image_crop, mask_prepare)), (jdist, (all_reduce_sum_,)), (torch, (arange,))):
        for f in fakes:
            patch(obj, f.__name__, f)
    patch(mod('smpl_model'), 'synthetic_smpl', synthetic_smpl)
    patch(eng, 'RefineEngine', FakeEngine)
    patch(eng, 'DeviceModel', FakeDeviceModel)
    patch(smpl.SMPL, 'to', smpl_to)
    patch(opt, 'SharedBucket', Bucket)
    patch(torch.cuda, 'set_device', lambda device: None)
    return opt, lambda: [setattr(o, n, v) for o, n, v in reversed(saved)]


def run(flags, tree=None, one_rank_group=False):
    """the driver under the stand-in with `flags`; one_rank_group: the collectives run over a one-rank gloo group (JRR_DIST_SINGLE_RANK=1).
    -> (the driver's return value, the call log)"""
    import torch.distributed as dist
    opt, undo = install(tree)
    argsmod = importlib.import_module(PKG + '.args')
    saved_ns, saved_env = argsmod._LazyArgs._ns, os.environ.get('JRR_DIST_SINGLE_RANK')
    del LOG[:]
    CREATED.clear()
    try:
        argsmod._LazyArgs._ns = argsmod.get_args(list(flags) + BASE_FLAGS)
        if one_rank_group:
            os.environ['JRR_DIST_SINGLE_RANK'] = '1'
            with tempfile.TemporaryDirectory() as tmp:
                dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
                try:
                    return opt.optimize_pose_refiner(log=lambda r: None), list(LOG)
                finally:
                    dist.destroy_process_group()
        return opt.optimize_pose_refiner(log=lambda r: None), list(LOG)
    finally:
        argsmod._LazyArgs._ns = saved_ns
        os.environ.pop('JRR_DIST_SINGLE_RANK', None)
        if saved_env is not None:
            os.environ['JRR_DIST_SINGLE_RANK'] = saved_env
        undo()


def comparable(result):
    """the driver's return value as JSON: the records without their two timings, tensors and arrays as shape + CRC"""
    def enc(x):
        if isinstance(x, dict):
            return {k: enc(v) for k, v in x.items() if k not in ('seconds', 'seconds_batch')}
        if isinstance(x, (list, tuple)):
            return [enc(v) for v in x]
        if torch.is_tensor(x) or hasattr(x, 'tobytes'):
            a = x.detach().contiguous().numpy() if torch.is_tensor(x) else x
            return f'{a.dtype}{list(a.shape)} crc={zlib.crc32(a.tobytes()):08x}'
        return x
    return enc(result)


if __name__ == '__main__':
    tree, out_path, flags = sys.argv[1], sys.argv[2], sys.argv[3:]
    group = os.environ.get('JRR_DIST_SINGLE_RANK') == '1'
    result, log = run(flags, tree=tree, one_rank_group=group)
    with open(out_path, 'w') as f:
        json.dump({'log': log, 'result': comparable(result)}, f, indent=1)
