"""Host restatement and cases of the acceleration error along each video sequence (jrr_accel_error; accel_report).

Written from include/jrr.h: the definition (pelvis-relative joints, the second difference along a triple, three lengths per joint, every
operation rounded once in the order written -- numpy's float32 arithmetic does exactly that), the table layout JRR_ACCEL_ACC_* and what
a position adds to it.  Evaluable in float32 (the kernel's format) and in float64 (the yardstick).  There is no reference
implementation, so a comparison is held to `bound(f32, f64) = 3 x max|f32 - f64| + 1e-7` of the restatement's two evaluations on the
test's OWN inputs, never to anything the kernel returned.
"""
import numpy as np

F, F64 = np.float32, np.float64
NJ = 17
ROW, TRAILER = 205, 2
COUNT, BAD, NO_TRIPLE, SUM_ERR, SUM_PRED, SUM_GT, HIST, BINS = 0, 1, 2, 3, 20, 37, 54, 151
TILE = 32

# the GPU case: a 96-row table, 70 listed rows in a non-monotone order, runs whose lengths cover every path of the triple rule; the
# run of 33 -- one more than the tile -- holds positions 3 .. 35, so its triples straddle the border between workgroups 0 and 1
N_ROWS = 96
RUN_LENGTHS = (3, 33, 1, 9, 2, 4, 18)
M = sum(RUN_LENGTHS)
N_GROUPS = 3
P_IGNORED, P_BAD_GROUP = 10, 50                    # the position with group -1, the one with group >= N_GROUPS


def bound(f32, f64):
    """3 x the float32 evaluation's largest distance from the float64 one + 1e-7; NaN must sit at the same places in both"""
    a, b = np.asarray(f32, dtype=F64), np.asarray(f64, dtype=F64)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    d = np.abs(a - b)
    return 3.0 * float(np.nanmax(d) if np.isfinite(d).any() else 0.0) + 1e-7


def dist(got, want):
    """largest distance of `got` from `want`; inf unless NaN sits at exactly the same places"""
    a, b = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float('inf')
    d = np.abs(a - b)
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


# ---- the restatement -------------------------------------------------------------------------------------------------------
def triples(order, run, n_rows):
    """(has_triple (M,) bool, absent (M,) bool): a position is absent when its order entry lies outside [0, n_rows); it has a triple
    when p - 1 and p + 1 are listed, carry its run and none of the three is absent"""
    order, run = np.asarray(order).astype(np.int64), np.asarray(run).astype(np.int64)
    m = order.shape[0]
    absent = (order < 0) | (order >= n_rows)
    has = np.zeros(m, dtype=bool)
    for p in range(1, m - 1):
        has[p] = (run[p - 1] == run[p] == run[p + 1]) and not (absent[p - 1] or absent[p] or absent[p + 1])
    return has, absent


def _len(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def accel(pred, gt_mm, order, run, dtype=F64):
    """(e, s, g), (M,17) each in `dtype`, NaN at the positions without a triple: the definition, each operation once, in order"""
    pred, gt_mm = np.asarray(pred, dtype=F).astype(dtype), np.asarray(gt_mm, dtype=F).astype(dtype)
    n_rows = pred.shape[0]
    has, absent = triples(order, run, n_rows)
    rows = np.where(absent, 0, np.asarray(order).astype(np.int64))
    with np.errstate(invalid='ignore', over='ignore'):
        x = pred[rows] - pred[rows][:, :1]
        q = gt_mm[rows] / dtype(1000)
        y = q - q[:, :1]
        m = rows.shape[0]
        out = [np.full((m, NJ), np.nan, dtype=dtype) for _ in range(3)]
        p = np.nonzero(has)[0]
        if p.size:
            a_pred = (x[p - 1] - dtype(2) * x[p]) + x[p + 1]
            a_gt = (y[p - 1] - dtype(2) * y[p]) + y[p + 1]
            out[0][p], out[1][p], out[2][p] = _len(a_pred - a_gt), _len(a_pred), _len(a_gt)
    return tuple(out)


def accumulate(e, s, g, has_triple, group, n_groups, table=None, positions=None):
    """ADD to `table` (int64, n_groups * 205 + 2; None = zeros) what jrr_accel_error adds for `positions` (None: all), in exact
    integers, from the float32 values e, s, g (M,17) a call wrote"""
    e, s, g = (np.asarray(a) for a in (e, s, g))
    assert e.dtype == F and s.dtype == F and g.dtype == F
    m = e.shape[0]
    table = np.zeros(n_groups * ROW + TRAILER, dtype=np.int64) if table is None else table
    group = np.zeros(m, dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    cap, scale = F(1.0e3), F(16777216.0)
    for p in (range(m) if positions is None else positions):
        gid = int(group[p])
        if gid < 0:
            table[n_groups * ROW] += 1
            continue
        if gid >= n_groups:
            table[n_groups * ROW + 1] += 1
            continue
        row = table[gid * ROW:(gid + 1) * ROW]
        if not has_triple[p]:
            row[NO_TRIPLE] += 1
            continue
        with np.errstate(invalid='ignore'):
            good = bool((e[p] < cap).all() and (s[p] < cap).all() and (g[p] < cap).all())
        if not good:
            row[BAD] += 1
            continue
        row[COUNT] += 1
        for v, at in ((e[p], SUM_ERR), (s[p], SUM_PRED), (g[p], SUM_GT)):
            row[at:at + NJ] += np.rint((v * scale).astype(F64)).astype(np.int64)      # llrintf: to nearest, ties to even
        bins = np.minimum(np.floor(e[p] * F(1000.0)).astype(np.int64), BINS - 1)
        np.add.at(row, HIST + bins, 1)
    return table


def host_accel_error(pred, gt_mm, order, run, status, group=None, n_groups=1, acc=None, begin=0, count=None, out=None, rows=True):
    """engine.accel_error on CPU tensors by the float32 restatement (the GPU tests hold the kernel to it)"""
    import torch
    m = int(order.shape[0])
    count = m - int(begin) if count is None else int(count)
    o, r = order.numpy(), run.numpy()
    e, s, g = accel(pred.numpy(), gt_mm.numpy(), o, r, F)
    has, absent = triples(o, r, pred.shape[0])
    if absent.any():
        status |= 1
    span = range(int(begin), int(begin) + count)
    if acc is not None:
        accumulate(e, s, g, has, None if group is None else group.numpy(), int(n_groups), acc.numpy(), span)
    if not rows:
        return None
    if out is None:
        out = tuple(torch.full((m, NJ), float('nan')) for _ in range(3))
    for t, v in zip(out, (e, s, g)):
        t[int(begin):int(begin) + count] = torch.from_numpy(v[int(begin):int(begin) + count])
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------
def lists(run_lengths=RUN_LENGTHS, n_rows=N_ROWS, seed=2):
    """(order (M,) int32, run (M,) int32): distinct table rows in a shuffled, non-monotone order; run ids ascend from 0"""
    rng = np.random.RandomState(seed)
    m = int(sum(run_lengths))
    assert m <= n_rows
    order = rng.permutation(n_rows)[:m].astype(np.int32)
    run = np.repeat(np.arange(len(run_lengths)), run_lengths).astype(np.int32)
    assert (np.diff(order) < 0).any() and (np.diff(order) > 0).any() and len(set(order.tolist())) == m
    return order, run


def motion_case(seed=7, noise_m=0.004):
    """(pred (96,17,3) float32 m, gt_mm (96,17,3) float32 mm, order, run, group (M,) int32): per run a smooth ground-truth motion (a
    skeleton of ~0.5 m that drifts and sways, pelvis included) and a prediction = ground truth + a constant offset per run + noise of a
    few mm per frame; rows outside the order hold other finite values.  Groups: run % 3, one position -1, one N_GROUPS."""
    rng = np.random.RandomState(seed)
    order, run = lists()
    pred = rng.normal(0, 1, size=(N_ROWS, NJ, 3)).astype(F)
    gt = (rng.normal(0, 1000, size=(N_ROWS, NJ, 3))).astype(F)
    at = 0
    for length in RUN_LENGTHS:
        t = np.arange(length, dtype=F64)[:, None, None]
        skel = rng.normal(0, 0.25, size=(1, NJ, 3))
        path = rng.normal(0, 0.02, size=(1, 1, 3)) * t + 0.05 * np.sin(0.3 * t + rng.uniform(0, 6, size=(1, NJ, 3)))
        g_m = skel + path + rng.normal(0, 1.0, size=(1, 1, 3))
        rows = order[at:at + length]
        gt[rows] = (g_m * 1000.0).astype(F)
        pred[rows] = (g_m + rng.normal(0, 0.05, size=(1, NJ, 3)) + rng.normal(0, noise_m, size=(length, NJ, 3))).astype(F)
        at += length
    group = (run % N_GROUPS).astype(np.int32)
    group[P_IGNORED], group[P_BAD_GROUP] = -1, N_GROUPS
    has, absent = triples(order, run, N_ROWS)
    assert not absent.any() and int(has.sum()) == sum(max(0, n - 2) for n in RUN_LENGTHS)
    assert has[31] and has[32] and run[31] == run[32] == 1                                  # a triple on either side of the tile border
    assert has[P_IGNORED] and has[P_BAD_GROUP]                                              # both would have counted
    assert len({int(x) for x in group[:TILE] if 0 <= x < N_GROUPS}) > 1                      # a tile with more than one group ...
    assert len({int(x) for x in group[2 * TILE:M]}) == 1                                    # ... and one with a single group
    return pred, gt, order, run, group


def dyadic_track(n=12, seed=1, velocity=True):
    """(pred (n,17,3) m, gt_mm (n,17,3) mm) float32 in which every position is k / 1024 m with a small integer k and the ground truth
    is 1000 x such a value, so that G / 1000, every difference and every second difference are exact in float32: joints = a skeleton
    + a constant velocity x t (velocity=False: no motion)"""
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=F64)[:, None, None]
    out = []
    for _ in range(2):
        skel = rng.randint(-512, 512, size=(1, NJ, 3))
        vel = rng.randint(-16, 16, size=(1, NJ, 3)) if velocity else 0
        out.append((skel + vel * t) / 1024.0)
    pred, gt = out[0].astype(F), (out[1] * 1000.0).astype(F)
    assert np.array_equal(pred.astype(F64), out[0]) and np.array_equal(gt.astype(F64), out[1] * 1000.0)
    assert np.array_equal((gt / F(1000)).astype(F64), out[1])                               # the division is exact
    return pred, gt


def one_run(n):
    return np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32)


def frame_path(action, camera, frame, subject='S9'):
    return f'/data/h36m/{subject}/{action}/imageSequence/{camera}/img_{frame:06d}.jpg'


def track_case():
    """(pred, gt_mm, order, run, paths, present) of a 96-sample split: motion_case with frame paths that make refined.sequence_runs
    return exactly its (order, run) -- the run as camera directory under an action whose name sorts with the run, the place as frame
    number (stride 5) -- and stray paths for the rows outside the order, which are not present"""
    pred, gt, order, run, _ = motion_case()
    actions = ['Eating', 'Eating', 'Sitting 1', 'Sitting 1', 'Sitting 2', 'Walking', 'Walking']
    paths = ['/data/stray/%d.jpg' % i for i in range(N_ROWS)]
    for p, (row, r) in enumerate(zip(order, run)):
        paths[int(row)] = frame_path(actions[int(r)], str(int(r)), 5 * p)
    present = np.zeros(N_ROWS, dtype=bool)
    present[order] = True
    return pred, gt, order, run, paths, present


def fill(track, pred, gt, present, lo=0, hi=N_ROWS, batch=40):
    """add the present rows of [lo, hi) to an accel_report.JointTrack of two sets, `after` = half of `before`, in batches"""
    import torch
    rows = np.nonzero(present)[0]
    rows = rows[(rows >= lo) & (rows < hi)]
    for a in range(0, rows.size, batch):
        idx = rows[a:a + batch]
        track.add(torch.from_numpy(idx), (torch.from_numpy(pred[idx]), torch.from_numpy(pred[idx]) * 0.5), torch.from_numpy(gt[idx]))
