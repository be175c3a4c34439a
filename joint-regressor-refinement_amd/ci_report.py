"""Paired bootstrap intervals of the evaluation report (`--eval_ci`): how sure the arrow of `before → after` is.

The report's evidence is a difference of two means over frames that are far from independent: they come in video sequences.  The
paired bootstrap resamples the evaluation UNITS with replacement R times -- a unit is a whole sequence (`--eval_ci_unit sequence`,
the default: the frames that share refined.sequence_key) or a frame (`frame`: the dataset index) --, recomputes BOTH regressors' means
on the same resample, and reports percentile intervals of before, after and after - before, the standard deviation over the
replicates as the standard error, and the share of replicates in which the retrained regressor was not better.

`PairedBootstrap` owns one int64 device buffer: the unit table (n_units,5) and the wins table (n_groups * 8 + 3 words) of
include/jrr.h (JRR_BOOT_*).  `add()` is jrr_evaluate_joints twice (under a non-default `--eval_protocol`: jrr_evaluate_protocol twice,
whose excluded columns hold zeros) and jrr_paired_units once, and reads nothing back.  `finish()`: ONE
int64 sum all-reduce of the buffer under data parallelism (exact: the shards are disjoint), the read-back, the checks, the units with
a counted pose ordered by (group, unit id), the segments (0: all units; 1 + g: the units of group g -- a group's interval resamples
that group's own units), the overflow rule in Python integers, the replicates sharded over the ranks with dist.shard_bounds, ONE
jrr_bootstrap_sums launch per rank and one more integer all-reduce.  Every word up to here is an integer and a function of the poses,
the seed and R alone: not of the batch size, the order, the sharding or the launch.  `derive()` is float64 numpy on those integers.

What the interval says: how much the numbers would move if the evaluated split were redrawn from units like its own.  It conditions on
that split (no word on other subjects or actions than those evaluated), and `sequence` treats the four cameras of a take as independent
sequences, which they are not: the truth lies between `sequence` and a resampling of whole takes, so read the interval as a lower bound
on the uncertainty.  `derive`, `markdown` and `write` work without a GPU.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import dist as jdist
from . import eval_protocol
from . import group_table
from .group_table import ALL, T_BAD_GROUP, T_IGNORED, fmt as _fmt

LAYOUT_VERSION = 1            # include/jrr.h: JRR_BOOT_LAYOUT_VERSION and the offsets below
UNIT_ROW, WINS_ROW, WINS_TRAILER = 5, 8, 3
BEFORE, BEFORE_PA, AFTER, AFTER_PA, UNIT_COUNT = 0, 1, 2, 3, 4
W_COUNT, W_BAD, W_BETTER, W_WORSE, W_TIE, W_BETTER_PA, W_WORSE_PA, W_TIE_PA = range(8)
T_BAD_UNIT = 2                # the third trailer word, behind the two of group_table
NJ = 17
FIXED = float(1 << 24)        # the sums are in units of 2^-24 m
SUM_LIMIT = 1 << 62           # include/jrr.h: (largest segment) x (largest unit word) stays below
UNIT_KINDS = ('sequence', 'frame')
METRICS = (('mpjpe', BEFORE, AFTER), ('pampjpe', BEFORE_PA, AFTER_PA))
_OWN_FLAGS = ('eval_ci', 'eval_ci_unit', 'eval_ci_reps', 'eval_ci_level')


def check_flags(ns) -> None:
    """`--eval_ci` needs `--eval_report DIR`; the replicates and the level are checked here too, before anything runs"""
    if not getattr(ns, 'eval_ci', False):
        return
    if not ns.eval_report:
        raise ValueError('--eval_ci needs --eval_report DIR (where ci.json / ci.md go)')
    if ns.eval_ci_unit not in UNIT_KINDS:
        raise ValueError(f'--eval_ci_unit {ns.eval_ci_unit!r}: one of {UNIT_KINDS}')
    if not 1 <= int(ns.eval_ci_reps) < 1 << 31:
        raise ValueError(f'--eval_ci_reps {ns.eval_ci_reps}: 1 .. 2^31 - 1')
    if not 0.0 < float(ns.eval_ci_level) < 1.0:
        raise ValueError(f'--eval_ci_level {ns.eval_ci_level}: strictly between 0 and 1')


def flags_doc(flags) -> dict:
    """the flags as the existing output files record them: the `eval_ci*` flags change none of those files, so they are not among them"""
    flags = flags if isinstance(flags, dict) else vars(flags)
    return {k: v for k, v in flags.items() if k not in _OWN_FLAGS}


def missing_paths_error(where: str) -> ValueError:
    return ValueError(f'--eval_ci --eval_ci_unit sequence: {where} is missing: the frame paths say which samples share a video sequence '
                      f'(or resample frames: --eval_ci_unit frame)')


def read_paths(directory: str, n: int) -> List[str]:
    """the frame paths of an --eval_vertices directory: `paths.txt`, one line per mesh"""
    p = os.path.join(directory, 'paths.txt')
    if not os.path.isfile(p):
        raise missing_paths_error(p)
    with open(p) as f:
        paths = [line.rstrip('\n') for line in f]
    if len(paths) != n:
        raise ValueError(f'{p}: {len(paths)} lines for {n} meshes')
    return paths


def unit_ids(kind: str, n_rows: int, paths: Optional[Sequence[str]] = None) -> Tuple[np.ndarray, int]:
    """((n_rows,) int32 unit of every dataset index, n_units).  frame: the index itself.  sequence: the index of the row's key among the
    sorted distinct keys of refined.sequence_key(path); a row without a key is a unit of its own, behind the keyed ones in dataset
    order.  Every rank computes the same from the same list."""
    if kind not in UNIT_KINDS:
        raise ValueError(f'unit kind {kind!r}: one of {UNIT_KINDS}')
    n_rows = int(n_rows)
    if kind == 'frame':
        return np.arange(n_rows, dtype=np.int32), n_rows
    from . import refined
    if paths is None or len(paths) != n_rows:
        raise ValueError(f'sequence units: {0 if paths is None else len(paths)} frame paths for {n_rows} rows')
    keys = [refined.sequence_key(p)[0] for p in paths]
    names = sorted({k for k in keys if k is not None})
    lut = {k: i for i, k in enumerate(names)}
    out, nxt = np.empty(n_rows, dtype=np.int32), len(names)
    for i, k in enumerate(keys):
        if k is None:
            out[i], nxt = nxt, nxt + 1
        else:
            out[i] = lut[k]
    return out, nxt


# ---- the tables ----------------------------------------------------------------------------------------------------------------
class PairedBootstrap:
    def __init__(self, group_names: Sequence[str], unit_of_row: np.ndarray, n_units: int, device, group_of_row: Optional[np.ndarray] = None,
                 protocol: Optional[eval_protocol.Protocol] = None):
        """unit_of_row (n_rows,) int32: the unit of every dataset index (unit_ids); group_of_row (n_rows,) int32 or None (the single
        group): the group of every dataset index, as the evaluation report assigns it; protocol None or `h36m17`: the reference's
        evaluate (all 17 joints, centred on joint 0)"""
        self.names = [str(g) for g in group_names]
        self.protocol = eval_protocol.H36M17 if protocol is None else protocol
        G = len(self.names)
        group_table.check_groups(G)
        self.unit_of_row = np.asarray(unit_of_row).astype(np.int32).reshape(-1)
        self.group_of_row = np.zeros_like(self.unit_of_row) if group_of_row is None else np.asarray(group_of_row).astype(np.int32).reshape(-1)
        if self.group_of_row.shape != self.unit_of_row.shape:
            raise ValueError(f'PairedBootstrap: {self.group_of_row.shape[0]} group ids for {self.unit_of_row.shape[0]} rows')
        self.n_units = int(n_units)
        if self.n_units < 1:
            raise ValueError('PairedBootstrap: no unit to resample')
        self.device = torch.device(device)
        self.flat = torch.zeros(self.n_units * UNIT_ROW + G * WINS_ROW + WINS_TRAILER, dtype=torch.int64, device=self.device)      # one buffer: one all-reduce
        self.units = self.flat[:self.n_units * UNIT_ROW].view(self.n_units, UNIT_ROW)
        self.wins = self.flat[self.n_units * UNIT_ROW:]

    def add(self, joints_before: torch.Tensor, joints_after: torch.Tensor, gt_mm, group_ids: Optional[torch.Tensor], index,
            target_unit: int = eval_protocol.TARGET_MM) -> None:
        """joints (B,17,3) m of both regressors on the same poses; gt (B,17,3) mm (target_unit TARGET_M: metres), one tensor for both
        regressors or a pair (before, after) -- ground-truth joints regressed from meshes differ between the two --; group_ids (B,) int32
        on the device (None: group 0; < 0 = do not score), index (B,): the poses' dataset indices, a host array or CPU tensor.  Three
        launches (the default protocol with a millimetre target: jrr_evaluate_joints twice; any other: jrr_evaluate_protocol twice,
        without a table; then jrr_paired_units, which sums the 17 columns -- the excluded ones hold zeros), nothing read back."""
        from . import engine as _engine
        idx = np.asarray(index.cpu() if torch.is_tensor(index) else index).astype(np.int64).reshape(-1)
        B = int(joints_before.shape[0])
        if idx.shape[0] != B:
            raise ValueError(f'PairedBootstrap.add: {idx.shape[0]} dataset indices for {B} poses')
        if B and (idx.min() < 0 or idx.max() >= self.unit_of_row.shape[0]):
            raise ValueError(f'PairedBootstrap.add: a dataset index outside [0, {self.unit_of_row.shape[0]})')
        dev = joints_before.device
        if group_ids is None:
            group_ids = torch.zeros(B, dtype=torch.int32, device=dev)
        if group_ids.device != dev or group_ids.dtype != torch.int32:
            raise ValueError(f'PairedBootstrap.add: group_ids must be an int32 tensor on {dev}, got {group_ids.dtype} on {group_ids.device}')
        unit = torch.from_numpy(self.unit_of_row[idx]).to(dev, non_blocking=True)
        gt_b, gt_a = (t.detach().float() for t in (gt_mm if isinstance(gt_mm, (tuple, list)) else (gt_mm, gt_mm)))
        if self.protocol.is_default and target_unit == eval_protocol.TARGET_MM:
            eb, eb_pa = _engine.evaluate_joints(joints_before.detach().float(), gt_b)
            ea, ea_pa = _engine.evaluate_joints(joints_after.detach().float(), gt_a)
        else:
            eb, eb_pa = _engine.evaluate_protocol(joints_before.detach().float(), gt_b, self.protocol.joint_mask, self.protocol.root, target_unit)
            ea, ea_pa = _engine.evaluate_protocol(joints_after.detach().float(), gt_a, self.protocol.joint_mask, self.protocol.root, target_unit)
        _engine.paired_units(eb, eb_pa, ea, ea_pa, group_ids, unit, len(self.names), self.units, self.wins)

    def finish(self, reps: int, seed: int, level: float, unit_kind: str, reduce: bool = True) -> dict:
        """the document's numbers (see the module docstring); reduce=False: this process evaluated everything alone"""
        import torch.distributed as dist
        from . import engine as _engine
        grouped = reduce and dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if grouped else (0, 1)
        host = group_table.all_reduce(self.flat, reduce, in_place=True).cpu().numpy()                 # the first integer collective and its read-back
        G = len(self.names)
        units = host[:self.n_units * UNIT_ROW].reshape(self.n_units, UNIT_ROW)
        wins = host[self.n_units * UNIT_ROW:]
        kept, group_of_unit, segments = plan(units, wins, G, self.unit_of_row, self.group_of_row)
        reps = int(reps)
        sums = np.zeros((len(segments), reps, UNIT_ROW), dtype=np.int64)
        if kept.shape[0]:
            check_overflow(units[kept], segments)
            table = torch.from_numpy(np.ascontiguousarray(units[kept])).to(self.device)
            lo, hi = jdist.shard_bounds(reps, rank, world)
            full = torch.zeros((len(segments), reps, UNIT_ROW), dtype=torch.int64, device=self.device)
            if hi > lo:
                full[:, lo:hi] = _engine.bootstrap_sums(table, segments, seed, lo, hi - lo, max_word=int(np.abs(units[kept]).max()))
            sums = group_table.all_reduce(full, reduce).cpu().numpy()                  # the second integer collective
        return derive(units[kept], group_of_unit, segments, sums, wins, self.names, level, seed=int(seed), unit_kind=unit_kind,
                      n_joints=self.protocol.n_joints)


def plan(units: np.ndarray, wins: np.ndarray, n_groups: int, unit_of_row: np.ndarray, group_of_row: np.ndarray):
    """(kept (K,) unit ids ordered by (group, unit id), their groups (K,), segments (1 + n_groups, 2) = (begin, count) rows of the
    ordered table) from the reduced tables.  Raises on poses that carried a bad group or unit, and on a unit with poses of two groups."""
    trailer = wins[n_groups * WINS_ROW:]
    if int(trailer[T_BAD_GROUP]) or int(trailer[T_BAD_UNIT]):
        raise RuntimeError(f'paired bootstrap: {int(trailer[T_BAD_GROUP])} poses carried a group id outside [0, {n_groups}), '
                           f'{int(trailer[T_BAD_UNIT])} a unit outside [0, {units.shape[0]}); they were not scored')
    n_units = units.shape[0]
    rows = (group_of_row >= 0) & (unit_of_row >= 0) & (unit_of_row < n_units)
    lo = np.full(n_units, np.iinfo(np.int32).max, dtype=np.int64)
    hi = np.full(n_units, -1, dtype=np.int64)
    np.minimum.at(lo, unit_of_row[rows], group_of_row[rows])
    np.maximum.at(hi, unit_of_row[rows], group_of_row[rows])
    used = np.nonzero(units[:, UNIT_COUNT] > 0)[0]
    mixed = used[lo[used] != hi[used]]
    if mixed.size:
        raise RuntimeError(f'paired bootstrap: unit {int(mixed[0])} holds poses of groups {int(lo[mixed[0]])} and {int(hi[mixed[0]])}: a '
                           f'resampling unit belongs to one group (group by something coarser than the unit, or resample frames)')
    g = lo[used]
    if used.size and (g.min() < 0 or g.max() >= n_groups):
        raise RuntimeError('paired bootstrap: a counted unit without a group')
    order = np.lexsort((used, g))
    kept, g = used[order], g[order]
    per = np.bincount(g, minlength=n_groups).astype(np.int64) if kept.size else np.zeros(n_groups, dtype=np.int64)
    begin = np.concatenate([[0], np.cumsum(per)[:-1]])
    segments = np.concatenate([[[0, kept.shape[0]]], np.stack([begin, per], axis=1)]).astype(np.int64)
    return kept, g, segments


def check_overflow(units: np.ndarray, segments: np.ndarray) -> None:
    """the overflow rule of include/jrr.h in Python integers: (largest segment) x (largest unit word) < 2^62, or OverflowError"""
    worst = int(np.asarray(segments)[:, 1].max()) * int(np.abs(units).max()) if units.size else 0
    if worst >= SUM_LIMIT:
        raise OverflowError(f'paired bootstrap: {int(np.asarray(segments)[:, 1].max())} draws of unit words up to {int(np.abs(units).max())} '
                            f'could reach {worst} >= 2^62')


# ---- the derivation ------------------------------------------------------------------------------------------------------------
def _mean_mm(total, count, n_joints: int = NJ):
    return total / FIXED / (n_joints * count) * 1000.0


def _interval(point: float, reps: np.ndarray, level: float) -> dict:
    lo, hi = np.percentile(reps, [100.0 * (1.0 - level) / 2.0, 100.0 * (1.0 + level) / 2.0])
    return {'mean_mm': float(point), 'lo_mm': float(lo), 'hi_mm': float(hi), 'se_mm': float(np.std(reps))}


def _stats(point: np.ndarray, reps: np.ndarray, n_units: int, wrow: np.ndarray, level: float, n_joints: int = NJ) -> dict:
    """point (5,) int64: the unresampled sums of the segment; reps (R,5) int64: its replicates; wrow (8,) int64; n_joints: the joints
    the sums run over (the protocol's)"""
    n = int(point[UNIT_COUNT])
    out = {'n_units': int(n_units), 'n_poses': n, 'n_bad': int(wrow[W_BAD]), 'raw_sums': [int(x) for x in point],
           'wins': {'mpjpe': {'better': int(wrow[W_BETTER]), 'worse': int(wrow[W_WORSE]), 'tie': int(wrow[W_TIE])},
                    'pampjpe': {'better': int(wrow[W_BETTER_PA]), 'worse': int(wrow[W_WORSE_PA]), 'tie': int(wrow[W_TIE_PA])}}}
    if n == 0:
        out.update({key: None for key, _, _ in METRICS})
        return out
    counts = reps[:, UNIT_COUNT].astype(np.float64)
    for key, cb, ca in METRICS:
        pb, pa = _mean_mm(np.float64(point[cb]), np.float64(n), n_joints), _mean_mm(np.float64(point[ca]), np.float64(n), n_joints)
        rb, ra = _mean_mm(reps[:, cb].astype(np.float64), counts, n_joints), _mean_mm(reps[:, ca].astype(np.float64), counts, n_joints)
        diff = _interval(pa - pb, ra - rb, level)
        diff['p_not_better'] = float(np.mean(ra - rb >= 0.0))
        out[key] = {'before': _interval(pb, rb, level), 'after': _interval(pa, ra, level), 'difference': diff}
    return out


def derive(units: np.ndarray, group_of_unit: np.ndarray, segments: np.ndarray, sums: np.ndarray, wins: np.ndarray, names: Sequence[str],
           level: float, seed: int = 0, unit_kind: str = 'frame', n_joints: int = NJ) -> dict:
    """the numbers from the integers: units (K,5) ordered as the segments say, sums (1 + G, R, 5) the replicates, wins (G * 8 + 3).
    Per segment and column mean_mm = sum / 2^24 / (n_joints count) * 1000 in float64 (n_joints: 17, or the protocol's number) -- the point estimate from the unresampled sums, a
    replicate's from its own sums and its own count --; numpy.percentile at (1 -+ level) / 2 of before, after and after - before; their
    standard deviation over the replicates as the standard error; p_not_better = the share of replicates with after - before >= 0."""
    units, sums, wins, segments = np.asarray(units), np.asarray(sums), np.asarray(wins), np.asarray(segments)
    G = len(names)
    if sums.dtype != np.int64 or sums.ndim != 3 or sums.shape[0] != G + 1 or sums.shape[2] != UNIT_ROW or segments.shape != (G + 1, 2):
        raise ValueError(f'bootstrap sums: ({G + 1},R,5) int64 expected for {G} groups, got {sums.dtype} {sums.shape}')
    if wins.shape != (G * WINS_ROW + WINS_TRAILER,):
        raise ValueError(f'wins table: {G * WINS_ROW + WINS_TRAILER} words expected for {G} groups, got {wins.shape}')
    wrows = wins[:G * WINS_ROW].reshape(G, WINS_ROW)
    point = lambda s: units[int(segments[s, 0]):int(segments[s, 0]) + int(segments[s, 1])].sum(0) if segments[s, 1] else np.zeros(UNIT_ROW, dtype=np.int64)
    return {'groups': {name: _stats(point(1 + i), sums[1 + i], int(segments[1 + i, 1]), wrows[i], level, n_joints) for i, name in enumerate(names)},
            ALL: _stats(point(0), sums[0], int(segments[0, 1]), wrows.sum(0), level, n_joints), 'ignored': int(wins[G * WINS_ROW + T_IGNORED]),
            'reps': int(sums.shape[1]), 'seed': int(seed), 'level': float(level), 'unit': unit_kind}


# ---- the files -----------------------------------------------------------------------------------------------------------------
def _cell(r: Optional[dict], spec='.2f') -> str:
    return '-' if r is None else f'{_fmt(r["mean_mm"], spec)} [{_fmt(r["lo_mm"], spec)}, {_fmt(r["hi_mm"], spec)}]'


def markdown(doc: dict) -> str:
    d = doc['data']
    pct = f'{100 * d["level"]:g} %'
    title = f', protocol {doc["protocol"]["name"]}' if doc.get('protocol') else ''
    lines = [f'# Paired bootstrap of before → after ({doc["source"]}, groups by {doc["group_kind"]}{title})', ''] + \
            ([eval_protocol.headline(doc['protocol']), ''] if doc.get('protocol') else []) + [
             f'{d["reps"]} resamples of the {d["unit"]}s with replacement, both regressors on the same resample; seed {d["seed"]}.  '
             f'Errors in mm with the {pct} percentile interval; p = the share of resamples in which the retrained regressor was not better '
             f'(difference >= 0); better / worse / tie count the poses themselves.  A group resamples its own {d["unit"]}s.  The intervals '
             f'condition on the evaluated split' + ('; the cameras of one take count as independent sequences.' if d['unit'] == 'sequence' else '.')]
    for name in list(doc['groups']) + [ALL]:
        r = d[ALL] if name == ALL else d['groups'][name]
        lines += ['', f'## {name}', '', f'{r["n_units"]} {d["unit"]}s, {r["n_poses"]} poses, {r["n_bad"]} bad.', '',
                  '| error | before → after | difference | p | better / worse / tie |', '|---|---|---|---|---|']
        for key, title in (('mpjpe', 'MPJPE'), ('pampjpe', 'PA-MPJPE')):
            m, w = r[key], r['wins'][key]
            arrow = '- → -' if m is None else f'{_cell(m["before"])} → {_cell(m["after"])}'
            diff = '-' if m is None else _cell(m['difference'], '+.3f')
            p = '-' if m is None else _fmt(m['difference']['p_not_better'], '.4f')
            lines.append(f'| {title} | {arrow} | {diff} | {p} | {w["better"]} / {w["worse"]} / {w["tie"]} |')
    if d.get('ignored'):
        lines += ['', f'{d["ignored"]} samples were not scored (marked invalid by the dataset).']
    return '\n'.join(lines) + '\n'


def write(directory: str, result: dict, group_names: Sequence[str], group_kind: str, source: str, protocol: Optional[dict] = None) -> Optional[dict]:
    """DIR/ci.json and DIR/ci.md from what finish() returned; rank 0 alone writes (the others return None).  protocol:
    eval_protocol.document(...), None under the default"""
    doc = {'layout_version': LAYOUT_VERSION, 'source': source, 'group_kind': group_kind, 'groups': list(group_names), 'data': result, 'unit': 'mm'}
    if protocol:
        doc['protocol'] = protocol
    return group_table.write(directory, 'ci', doc, markdown)


def load(directory: str) -> dict:
    return group_table.load(directory, 'ci', LAYOUT_VERSION)


def summary_line(doc: dict) -> str:
    d = doc['data']
    r = d[ALL]
    parts = []
    for key, title in (('mpjpe', 'MPJPE'), ('pampjpe', 'PA-MPJPE')):
        m = r[key]
        parts.append(f'{title} -' if m is None else f'{title} {_cell(m["difference"], "+.4f")} (p {_fmt(m["difference"]["p_not_better"], ".4f")})')
    return (f'paired bootstrap, after - before in mm with the {100 * d["level"]:g} % interval, {d["reps"]} resamples of {r["n_units"]} '
            f'{d["unit"]}s: ' + '  '.join(parts))
