"""The grouped int64 accumulator of the report tables, host side (csrc/acctab.h is the device side; DESIGN.md 3s states the contract).

A table is `n_groups` rows of `row` int64 words and a two-word trailer: poses ignored on purpose (group < 0), poses whose group id lay
outside the table.  The kernels add into it with integer atomics; a report's `finish()` sums it over the ranks ONCE (`all_reduce`),
reads it back once, refuses a table whose second trailer word is not zero (`split`) and derives its numbers per group and for `all`
(`derive`).  The files are `STEM.json` + `STEM.md`, written by rank 0 (`write`) and read back against the layout version (`load`).
"""
from __future__ import annotations

import json
import os
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import dist as jdist

TRAILER, T_IGNORED, T_BAD_GROUP = 2, 0, 1       # include/jrr.h: JRR_EVAL_ACC_TRAILER, _TRAILER_IGNORED, _TRAILER_BAD_GROUP
MAX_GROUPS = 1024                                # JRR_EVAL_ACC_MAX_GROUPS
ALL = 'all'


def rank() -> int:
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank()
    return jdist.env_rank_world()[0]


def check_groups(n: int, what: str = 'groups') -> None:
    if not 1 <= n <= MAX_GROUPS:
        raise ValueError(f'{n} {what}: 1 .. {MAX_GROUPS}')


def all_reduce(t, reduce: bool = True, op=None, in_place: bool = False):
    """the reduction of an integer (or float) tensor over the ranks -- the sum, unless `op` names another -- and nothing without an
    initialised process group or with reduce=False.  A device tensor goes through the host under gloo.  Returns the reduced tensor:
    `t` itself, but for the host copy of that detour; in_place=True copies it back into `t`."""
    import torch.distributed as dist
    if not (reduce and dist.is_available() and dist.is_initialized()):
        return t
    out = t.cpu() if t.is_cuda and dist.get_backend() == 'gloo' else t
    dist.all_reduce(out, op=dist.ReduceOp.SUM if op is None else op)
    if in_place and out is not t:
        t.copy_(out)
        return t
    return out


def split(table: np.ndarray, n_groups: int, row: int, name: str, noun: str = 'poses', verb: str = 'scored', what: str = 'groups',
          ident: str = 'group id') -> Tuple[np.ndarray, int]:
    """(rows (n_groups, row), ignored) of a flat table.  Refuses another dtype or size, and a table whose kernel met a group id outside
    [0, n_groups).  name / noun / verb / what / ident word the two refusals: `bone subject table`, `positions`, `counted`, `subjects`, `subject id`."""
    table = np.asarray(table)
    G = n_groups
    if table.dtype != np.int64 or table.shape != (G * row + TRAILER,):
        raise ValueError(f'{name}: {G * row + TRAILER} int64 expected for {G} {what}, got {table.dtype} {table.shape}')
    bad_group = int(table[G * row + T_BAD_GROUP])
    if bad_group:
        raise RuntimeError(f'{name}: {bad_group} {noun} carried a {ident} outside [0, {G}); they were not {verb}')
    return table[:G * row].reshape(G, row), int(table[G * row + T_IGNORED])


def assemble(rows: np.ndarray, ignored: int, names: Sequence[str], stats: Callable[[np.ndarray], dict]) -> dict:
    return {'groups': {name: stats(rows[i]) for i, name in enumerate(names)}, ALL: stats(rows.sum(0)), 'ignored': ignored}


def derive(table: np.ndarray, names: Sequence[str], row: int, stats: Callable[[np.ndarray], dict], name: str, noun: str = 'poses',
           verb: str = 'scored') -> dict:
    """per group and for `all` what `stats` makes of a row, and the number of ignored poses"""
    rows, ignored = split(table, len(names), row, name, noun, verb)
    return assemble(rows, ignored, names, stats)


def fmt(x, spec='.2f') -> str:
    return '-' if x is None else format(x, spec)


def arrow(b, a, spec='.2f') -> str:
    return f'{fmt(b, spec)} → {fmt(a, spec)}'


def write(directory: str, stem: str, doc, markdown: Callable[[dict], str]) -> Optional[dict]:
    """DIR/STEM.json and DIR/STEM.md; rank 0 alone writes (the others return None).  doc: the document, or a function without arguments
    that builds it -- called on rank 0 only, after the directory exists."""
    if rank() != 0:
        return None
    os.makedirs(directory, exist_ok=True)
    if callable(doc):
        doc = doc()
    with open(os.path.join(directory, stem + '.json'), 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True, default=str)
    with open(os.path.join(directory, stem + '.md'), 'w', encoding='utf-8') as f:
        f.write(markdown(doc))
    return doc


def load(directory: str, stem: str, version: int, what: str = 'table') -> dict:
    with open(os.path.join(directory, stem + '.json')) as f:
        doc = json.load(f)
    if doc.get('layout_version') != version:
        raise ValueError(f'{directory}: {what} layout version {doc.get("layout_version")!r}, this build reads version {version}')
    return doc
