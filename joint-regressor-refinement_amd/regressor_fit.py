"""The regressor fit (`--fit_regressor OUT --fit_from PATH`): Adam steps of the J_regressor on a table of fixed meshes.

The driver gives the regressor one Adam step per outer batch, behind 100 inner pose iterations (/root/reference/scripts/optimize.py:300-312).
Once the poses are fixed -- a `--save_refined` table, its smoothed or view-fused form, or the meshes of another model in the
`--eval_vertices` format -- that step needs very little of a mesh: ReLU' zeroes the gradient outside the positive entries of
J*mask, and an entry whose gradient is always zero keeps m = v = 0 under torch.optim.Adam and never moves.  So the meshes are made
ONCE (the existing SMPL operator, in chunks of --batch_size) and only the support vertices and the ground truth of each sample are
kept, in a device cache (engine.RegressorFit, include/jrr.h jrr_jfit_*: under 1 KB per sample for the shipped regressor).  An epoch is
one jrr_jfit_run over all minibatches of the training rows, one launch per step, nothing read back; per epoch there is one
read-back: the steps' losses and MPJPE / PA-MPJPE of the training and the held-out rows (jrr_jfit_joints + jrr_evaluate).

The regressor, the mask, the learning rate, the batch and the seed are the driver's: --j_regressor_init, utils.find_j_reg_mask,
--j_reg_lr, --batch_size, --seed.  The cache holds the training rows first, the held-out rows behind them; `--fit_shuffle` permutes
the training rows between epochs with an index copy (a seeded torch.randperm): the kernel always reads contiguous row ranges.

`--fit_solve` replaces the epochs by the exact solve of the same loss from the second moments of the cache rows (regressor_solve.py;
OUT/solve.json instead of fit.json); sources, hold-out split, cache fill, scores and checkpoint are the ones below.
"""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import args as jargs
from . import dist as jdist

LAYOUT_VERSION = 1
CHECKPOINT_NAME = 'retrained_J_Regressor.pt'
ROW_CAP = 128                 # include/jrr.h: JRR_JFIT_ROW_CAP
NJ, NV = 17, 6890
# what fit.json holds (tests/test_regressor_fit.py checks the schema)
DOC_KEYS = ('layout_version', 'source', 'flags', 'rows', 'support', 'steps_per_epoch', 'epochs', 'initial', 'final', 'checkpoint',
            'j_regressor_init')
EPOCH_KEYS = ('epoch', 'loss', 'train', 'holdout')
SCORE_KEYS = ('mpjpe_mm', 'pampjpe_mm')
_EXCLUSIVE = ('eval_vertices', 'smooth_refined', 'fuse_refined', 'save_refined', 'init_refined', 'eval_report', 'regressor_report')


def is_vertices_dir(path: str) -> bool:
    return os.path.isdir(path) and os.path.isfile(os.path.join(path, 'vertices.npy'))


def check_flags(ns) -> None:
    """what the flags of the fit must satisfy, before anything is launched"""
    loss_kind, delta_mm = getattr(ns, 'fit_solve_loss', 'mse'), float(getattr(ns, 'fit_solve_delta_mm', 0.01))
    if loss_kind not in ('mse', 'mpjpe'):
        raise ValueError(f'--fit_solve_loss {loss_kind}: mse or mpjpe')
    if not (np.isfinite(delta_mm) and delta_mm > 0.0):
        raise ValueError(f'--fit_solve_delta_mm {delta_mm}: a finite positive number of millimetres')
    if (loss_kind != 'mse' or delta_mm != 0.01) and not getattr(ns, 'fit_solve', False):
        raise ValueError('--fit_solve_loss / --fit_solve_delta_mm need --fit_solve')
    grow, grow_add = getattr(ns, 'fit_grow', None), int(getattr(ns, 'fit_grow_add', 8))
    if grow is not None and int(grow) < 0:
        raise ValueError(f'--fit_grow {grow}: 0 or more rounds')
    if not 1 <= grow_add <= ROW_CAP:
        raise ValueError(f'--fit_grow_add {grow_add}: 1 .. {ROW_CAP}')
    if (grow is not None or grow_add != 8) and not getattr(ns, 'fit_solve', False):
        raise ValueError('--fit_grow / --fit_grow_add need --fit_solve')
    if grow_add != 8 and grow is None:
        raise ValueError('--fit_grow_add belongs to --fit_grow R')
    if ns.fit_regressor is None:
        if ns.fit_from is not None:
            raise ValueError('--fit_from belongs to --fit_regressor OUT')
        if getattr(ns, 'fit_solve', False) or int(getattr(ns, 'fit_rings', 0) or 0):
            raise ValueError('--fit_solve / --fit_rings belong to --fit_regressor OUT')
        return
    if not ns.fit_from:
        raise ValueError('--fit_regressor needs --fit_from PATH: a --save_refined table or a directory in the --eval_vertices format')
    for name in _EXCLUSIVE:
        if getattr(ns, name, None):
            raise ValueError(f'--fit_regressor runs alone and exits: it does not go with --{name}')
    if int(ns.fit_epochs) < 1:
        raise ValueError(f'--fit_epochs {ns.fit_epochs}: 1 or more')
    if not 0.0 <= float(ns.fit_holdout) < 1.0:
        raise ValueError(f'--fit_holdout {ns.fit_holdout}: a fraction in [0, 1)')
    if int(ns.batch_size) < 1:
        raise ValueError(f'--batch_size {ns.batch_size}: 1 or more')
    if not float(ns.j_reg_lr) > 0.0:
        raise ValueError(f'--j_reg_lr {ns.j_reg_lr}: a positive number')
    if not is_vertices_dir(ns.fit_from) and not ns.data_root:
        raise ValueError('--fit_from a --save_refined table needs --data_root (the ground truth of the split the table was written from)')
    rings = int(getattr(ns, 'fit_rings', 0) or 0)
    if rings < 0:
        raise ValueError(f'--fit_rings {rings}: 0 or more')
    if rings > 0 and not getattr(ns, 'fit_solve', False):
        raise ValueError('--fit_rings needs --fit_solve: Adam cannot move an entry that starts at zero (relu\'(0) = 0)')
    if getattr(ns, 'fit_solve', False):
        if not float(ns.fit_solve_tol) > 0.0:
            raise ValueError(f'--fit_solve_tol {ns.fit_solve_tol}: a positive number')
        if int(ns.fit_solve_iters) < 1:
            raise ValueError(f'--fit_solve_iters {ns.fit_solve_iters}: 1 or more')
        if rings > 0 and is_vertices_dir(ns.fit_from) and not ns.synthetic and ns.smpl_dir == 'SPIN/data/smpl':
            raise ValueError('--fit_rings on meshes in the --eval_vertices format needs the faces of their body model: --smpl_dir or --synthetic')


def schedule(n_rows: int, batch: int) -> List[Tuple[int, int]]:
    """the minibatches of one epoch: (first row, count) of step k = rows [k * batch, min((k + 1) * batch, n_rows)), the last one short"""
    n_rows, batch = int(n_rows), int(batch)
    if batch < 1 or n_rows < 0:
        raise ValueError(f'schedule: {n_rows} rows in minibatches of {batch}')
    return [(a, min(batch, n_rows - a)) for a in range(0, n_rows, batch)]


def holdout_split(n: int, fraction: float, paths: Optional[Sequence[str]] = None) -> np.ndarray:
    """bool (n,): the rows held out of training.  With frame paths whole sequences (refined.sequence_key) are held out: in sorted key
    order every round(1 / F)-th one, so that no sequence lies on both sides (a path without a key is a sequence of its own, sorted
    behind the keyed ones in row order).  Without paths: the last round(F n) rows.  F = 0 keeps everything for training."""
    n, F = int(n), float(fraction)
    if not 0.0 <= F < 1.0:
        raise ValueError(f'holdout: fraction {F}: in [0, 1)')
    held = np.zeros(n, dtype=bool)
    if F == 0.0 or n == 0:
        return held
    if paths is None:
        k = int(round(F * n))
        if k:
            held[n - k:] = True
        return held
    from .refined import sequence_key
    if len(paths) != n:
        raise ValueError(f'holdout: {len(paths)} paths for {n} rows')
    keys = [sequence_key(p)[0] for p in paths]
    names = sorted({k for k in keys if k is not None})
    order = {k: i for i, k in enumerate(names)}
    seq = np.array([order[k] if k is not None else len(names) + i for i, k in enumerate(keys)], dtype=np.int64)
    every = max(1, int(round(1.0 / F)))
    ranks = {s: r for r, s in enumerate(sorted(set(seq.tolist())))}
    rank = np.array([ranks[s] for s in seq.tolist()], dtype=np.int64)
    return (rank + 1) % every == 0


def support_lists(J_init: np.ndarray, mask: Optional[np.ndarray] = None):
    """what jrr_jfit_prepare builds, on the host: (cols (NS,), counts (17,), pos: per row the positions of its positive entries in cols,
    vtx: per row their vertices) -- the union of the columns where J_init * mask > 0 in ascending order and the rows' lists in ascending
    vertex order.  Raises ValueError for a row above 128 entries and for no positive entry at all."""
    J = np.asarray(J_init, dtype=np.float32)
    x = J if mask is None else J * np.asarray(mask, dtype=np.float32)
    on = x > 0
    counts = on.sum(1)
    if (counts > ROW_CAP).any():
        raise ValueError(f'row {int(np.argmax(counts > ROW_CAP))} of J_init * mask has {int(counts.max())} positive entries: at most {ROW_CAP}')
    if not on.any():
        raise ValueError('J_init * mask has no positive entry')
    cols = np.flatnonzero(on.any(0))
    where = np.full(J.shape[1], -1, dtype=np.int64)
    where[cols] = np.arange(cols.size)
    vtx = [np.flatnonzero(on[i]) for i in range(J.shape[0])]
    return cols.astype(np.int32), counts.astype(np.int32), [where[v].astype(np.int32) for v in vtx], vtx


def support_counts(J: np.ndarray, mask: Optional[np.ndarray] = None) -> List[int]:
    x = np.asarray(J, dtype=np.float32) if mask is None else np.asarray(J, dtype=np.float32) * np.asarray(mask, dtype=np.float32)
    return [int(c) for c in (x > 0).sum(1)]


def build_doc(source: str, flags: dict, n_train: int, n_holdout: int, support_before, support_after, steps_per_epoch: int,
              initial: dict, epochs: List[dict], checkpoint: str, j_regressor_init) -> dict:
    """fit.json.  initial / epochs[k]: {'train': {mpjpe_mm, pampjpe_mm}, 'holdout': the same or None}; an epoch adds its number and its
    mean loss (the steps' losses weighted by their counts)"""
    return {'layout_version': LAYOUT_VERSION, 'source': source, 'flags': flags, 'rows': {'train': int(n_train), 'holdout': int(n_holdout)},
            'support': {'before': [int(c) for c in support_before], 'after': [int(c) for c in support_after]},
            'steps_per_epoch': int(steps_per_epoch), 'initial': initial, 'epochs': epochs, 'final': epochs[-1] if epochs else initial,
            'checkpoint': checkpoint, 'j_regressor_init': j_regressor_init}


def flags_doc(ns) -> dict:
    from . import bones_report, ci_report, eval_protocol, penetration_report, regressor_report
    return {k: v for k, v in eval_protocol.flags_doc(penetration_report.flags_doc(bones_report.flags_doc(regressor_report.flags_doc(ci_report.flags_doc(jargs.recorded(ns)))))).items() if isinstance(v, (bool, int, float, str, type(None)))}


# ---- the sources ---------------------------------------------------------------------------------------------------------------
class _VerticesSource:
    """a directory in the --eval_vertices format: uploaded in chunks, no body model"""

    def __init__(self, ns):
        from . import eval_report
        self.verts, self.gt, _, _ = eval_report.open_vertices_dir(ns.fit_from, 'none')
        pp = os.path.join(ns.fit_from, 'paths.txt')
        self.paths = None
        if os.path.isfile(pp):
            with open(pp) as f:
                self.paths = [line.rstrip('\n') for line in f]
            if len(self.paths) != self.verts.shape[0]:
                raise ValueError(f'{pp}: {len(self.paths)} lines for {self.verts.shape[0]} meshes')
        self.rows = np.arange(self.verts.shape[0])
        self.kind = 'vertices'

    def chunk(self, rows: np.ndarray, device):
        from . import utils
        v = torch.from_numpy(np.ascontiguousarray(self.verts[rows])).to(device)
        g = torch.from_numpy(np.ascontiguousarray(self.gt[rows]).astype(np.float32)).to(device)
        return v, utils.move_pelvis(g).contiguous()


class _RefinedSource:
    """a --save_refined table (or a named .npz of it): the rows with has_refined, the ground truth of the split of --data_root, the
    meshes from the existing SMPL operator"""

    def __init__(self, ns, device):
        from . import data as jdata, refined
        from .smpl import SMPL
        table = refined.load_path(ns.fit_from)
        location = jdata.split_location('validation', ns.data_root)
        ds = jdata.data_set('validation', root=ns.data_root)
        n_table = table['has_refined'].shape[0]
        if len(ds) != n_table:
            raise ValueError(f'--fit_from: the table holds {n_table} samples, the split {len(ds)}')
        self.table, self.gt = table, ds.gt_j3d
        self.rows = np.flatnonzero(np.asarray(table['has_refined']).astype(bool))
        all_paths = jdata.split_image_paths(location)
        self.paths = None if all_paths is None else [all_paths[i] for i in self.rows]
        self.smpl = SMPL(ns.smpl_dir, batch_size=1, allow_synthetic=ns.synthetic or ns.smpl_dir == 'SPIN/data/smpl').to(device)
        self.kind = 'refined'

    def chunk(self, rows: np.ndarray, device):
        from . import engine as _engine, utils
        B = int(rows.size)
        x6d = torch.from_numpy(np.ascontiguousarray(self.table['pose6d'][rows])).to(device).float().contiguous()
        betas = torch.from_numpy(np.ascontiguousarray(self.table['shape'][rows])).to(device).float().contiguous()
        _, verts = self.smpl.engine(B, _engine.FLAG_KEEP_VERTS).find_joints_forward(betas, x6d=x6d, return_verts=True)
        gt = utils.move_pelvis(self.gt[torch.from_numpy(rows)].to(device).float()).contiguous()
        return verts, gt


def fill_cache(fit, source, order: np.ndarray, batch: int, device) -> None:
    """cache row k <- sample order[k] of the source, in chunks of `batch`: each chunk's meshes are gathered and dropped"""
    with torch.no_grad():
        for a in range(0, order.size, batch):
            verts, gt = source.chunk(order[a:a + batch], device)
            fit.gather(verts, gt, a)


def _scores(fit, n_train: int, n_hold: int) -> torch.Tensor:
    """(4,) device: MPJPE, PA-MPJPE in mm of the training rows and of the held-out rows (NaN without any)"""
    from . import engine as _engine
    out = torch.full((4,), float('nan'), device=fit.device)
    for k, (a, n) in enumerate(((0, n_train), (n_train, n_hold))):
        if n:
            err, err_pa = _engine.evaluate(fit.joints(a, n), fit.ground_truth_mm(a, n))
            out[2 * k], out[2 * k + 1] = err.mean() * 1000, err_pa.mean() * 1000
    return out


def _score_doc(v) -> dict:
    f = lambda x: None if np.isnan(x) else float(x)
    return {'train': {'mpjpe_mm': f(v[0]), 'pampjpe_mm': f(v[1])},
            'holdout': None if np.isnan(v[2]) and np.isnan(v[3]) else {'mpjpe_mm': f(v[2]), 'pampjpe_mm': f(v[3])}}


def fit(J_init: torch.Tensor, mask: Optional[torch.Tensor], source, ns, device):
    """the epochs.  Returns (J (17,6890) on the device, initial score doc, epoch docs, RegressorFit, n_train, n_holdout)."""
    from . import engine as _engine
    rows = np.asarray(source.rows)
    held = holdout_split(rows.size, ns.fit_holdout, source.paths)
    order = np.concatenate([rows[~held], rows[held]])
    n_train, n_hold = int((~held).sum()), int(held.sum())
    if n_train == 0:
        raise ValueError(f'--fit_regressor: no training row ({rows.size} rows, {n_hold} held out)')
    bs = int(ns.batch_size)
    jf = _engine.RegressorFit(J_init, mask, order.size)
    fill_cache(jf, source, order, bs, device)
    steps = schedule(n_train, bs)
    counts = torch.tensor([c for _, c in steps], dtype=torch.float32, device=device)
    loss = torch.empty(len(steps), device=device)
    gen = torch.Generator().manual_seed(int(ns.seed))
    initial = _score_doc(_scores(jf, n_train, n_hold).cpu().numpy())
    epochs = []
    for ep in range(int(ns.fit_epochs)):
        if ns.fit_shuffle and ep > 0:
            perm = torch.randperm(n_train, generator=gen).to(device)
            jf.cache[:n_train] = jf.cache[:n_train].index_select(0, perm)
        jf.run(bs, 0, len(steps), float(ns.j_reg_lr), loss=loss, n_rows=n_train)
        host = torch.cat([((loss * counts).sum() / n_train).reshape(1), _scores(jf, n_train, n_hold)]).cpu().numpy()   # the epoch's one read-back
        epochs.append(dict(_score_doc(host[1:]), epoch=ep + 1, loss=float(host[0])))
    jf.info()                                                  # raises if the device refused a call
    J, _, _ = jf.dense()
    return J, initial, epochs, jf, n_train, n_hold


def fit_command(log=print) -> Optional[dict]:
    """`python main.py --fit_regressor OUT --fit_from PATH [--data_root ROOT] [--fit_epochs 10] [--fit_shuffle] [--fit_holdout 0.1]`.
    One process: under torchrun rank 0 works and the other ranks return.  Prints one summary line."""
    from . import checkpoint, smpl_model, utils
    from .args import args
    ns = args._get()
    check_flags(ns)
    if ns.fit_solve:                                               # the exact solve in place of the epochs: OUT/solve.json
        from . import regressor_solve
        return regressor_solve.solve_command(log)
    if jdist.env_rank_world()[0] != 0:
        return None
    device = torch.device(ns.device)
    torch.cuda.set_device(device)
    J_np = smpl_model.default_h36m_regressor(ns.j_regressor_init,
                                             allow_default=ns.synthetic or ns.j_regressor_init == 'SPIN/data/J_regressor_h36m.npy')
    J_init = torch.from_numpy(J_np).float().to(device)
    mask = utils.find_j_reg_mask(J_init)
    _, counts, _, _ = support_lists(J_np, mask.cpu().numpy())      # a row above 128 entries is refused here, before any table is read
    if (counts == 0).any():
        log(f'--fit_regressor: rows {np.flatnonzero(counts == 0).tolist()} of --j_regressor_init have no positive entry: they have no '
            f'parameters, stay as they are and are left out of the loss; their joints evaluate as NaN')
    source = _VerticesSource(ns) if is_vertices_dir(ns.fit_from) else _RefinedSource(ns, device)
    J, initial, epochs, jf, n_train, n_hold = fit(J_init, mask, source, ns, device)
    path = ns.save_j_regressor or os.path.join(ns.fit_regressor, CHECKPOINT_NAME)
    os.makedirs(ns.fit_regressor, exist_ok=True)
    checkpoint.save_j_regressor(J, path)
    mask_np = mask.cpu().numpy()
    doc = build_doc(source.kind, flags_doc(ns), n_train, n_hold, support_counts(J_np, mask_np), support_counts(J.cpu().numpy(), mask_np),
                    len(schedule(n_train, int(ns.batch_size))), initial, epochs, path, ns.j_regressor_init)
    with open(os.path.join(ns.fit_regressor, 'fit.json'), 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True, default=str)
    fmt = lambda d, k: '-' if d is None or d[k] is None else format(d[k], '.4f')
    last = epochs[-1]
    log(f'fitted the regressor on {n_train} rows ({n_hold} held out, {jf.entries} entries on {jf.ns} vertices) for {len(epochs)} epochs of '
        f'{doc["steps_per_epoch"]} steps: loss {epochs[0]["loss"]:.6e} -> {last["loss"]:.6e}, MPJPE {fmt(initial["train"], "mpjpe_mm")} -> '
        f'{fmt(last["train"], "mpjpe_mm")} (held out {fmt(initial["holdout"], "mpjpe_mm")} -> {fmt(last["holdout"], "mpjpe_mm")}), PAMPJPE '
        f'{fmt(initial["train"], "pampjpe_mm")} -> {fmt(last["train"], "pampjpe_mm")} (held out {fmt(initial["holdout"], "pampjpe_mm")} -> '
        f'{fmt(last["holdout"], "pampjpe_mm")}); {path}')
    return doc
