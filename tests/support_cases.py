"""Support structures for the per-vertex iteration (csrc/supk.h, k_sup_gather in csrc/sup.hip) beyond the shipped H36M regressor's:
seeded builders of support vertex sets, regressors over them and bodies with other influence counts, and the table of cases that
tests/test_support_cases.py pins on the CPU and tests/test_gpu_support_shapes.py runs on the GPU.  numpy only.

The shipped regressor on the synthetic surface body has 58 support vertices in rows 13 .. 6828, 2 to 5 entries per row, no vertex read
by more than 2 H36M joints, 4 skinning influences on every vertex and at most 22 support vertices per SMPL joint.  The cases here are
what that structure never reaches: other counts of support vertices (2 .. 64, and 65: the tile lists), vertices read by all 17 rows,
full rows, the first vertex and the partial last tile (rows 6880 .. 6889), 1 / 2 / 3 / 6 influences, one SMPL joint that skins all 64
support vertices, and a support that shrinks under J steps.
"""
import numpy as np

V, NH, NJ = 6890, 17, 24
SUP_NSV = 64                                  # most support vertices of the per-vertex iteration (csrc/kernels.h)
EDGES = (0, 6889, 31, 32, 6879, 6880)         # first vertex, last vertex, both sides of the first and of the last full tile's end


def vertices_spread(n: int, seed: int) -> np.ndarray:
    """n sorted vertex indices: the first min(n, 6) of EDGES, the rest random"""
    rng = np.random.RandomState(seed)
    base = np.array(EDGES[:min(n, len(EDGES))], dtype=np.int64)
    rest = rng.choice(np.setdiff1d(np.arange(V), base), n - len(base), replace=False)
    return np.sort(np.concatenate([base, rest]).astype(np.int64))


def vertices_of_joint(model, n: int, j: int, seed: int) -> np.ndarray:
    """n sorted vertices with a non-zero skinning weight on SMPL joint j"""
    rng = np.random.RandomState(seed)
    return np.sort(rng.choice(np.nonzero(model['lbs_weights'][:, j] != 0)[0], n, replace=False)).astype(np.int64)


def vertices_wrists(model) -> np.ndarray:
    """all vertices skinned by joint 20 or 21 (the deepest kinematic chain)"""
    W = model['lbs_weights']
    return np.nonzero((W[:, 20] != 0) | (W[:, 21] != 0))[0].astype(np.int64)


def regressor(verts, layout: str, seed: int, negatives: bool = True) -> np.ndarray:
    """(17, 6890) float32.  'blocks': row i reads verts[i::17] (verts[i % n] when that is empty), values in [0.1, 0.6], not normalised.
    'dense': every row reads every vertex, a Dirichlet draw times a row scale in [0.5, 2].  negatives: three negative entries per row
    on vertices outside `verts` (ReLU removes them)."""
    verts = np.asarray(verts, dtype=np.int64)
    rng = np.random.RandomState(seed)
    J = np.zeros((NH, V), np.float32)
    n = len(verts)
    for i in range(NH):
        if layout == 'dense':
            J[i, verts] = (rng.dirichlet(np.ones(n)) * rng.uniform(0.5, 2.0)).astype(np.float32)
        elif layout == 'blocks':
            own = verts[i::NH] if len(verts[i::NH]) else verts[[i % n]]
            J[i, own] = rng.uniform(0.1, 0.6, len(own)).astype(np.float32)
        else:
            raise ValueError(layout)
    if negatives:
        free = np.setdiff1d(np.arange(V), verts)
        for i in range(NH):
            J[i, rng.choice(free, 3, replace=False)] = -rng.uniform(0.01, 0.2, 3).astype(np.float32)
    return J


def with_influences(model, verts, counts, seed: int = 3):
    """a copy of the body in which vertex verts[k] keeps its counts[k] largest skinning weights, renormalised (counts 1 .. 4); for
    count 6 it keeps its four and gets two more joints at weight 0.05 before renormalising.  Every other vertex is untouched."""
    rng = np.random.RandomState(seed)
    W = model['lbs_weights'].astype(np.float32).copy()
    for v, k in zip(verts, counts):
        order = np.argsort(-W[v], kind='stable')
        w = np.zeros(NJ, np.float32)
        if k <= 4:
            w[order[:k]] = W[v, order[:k]]
        elif k == 6:
            w[order[:4]] = W[v, order[:4]]
            spare = np.nonzero(W[v] == 0)[0]
            w[rng.choice(spare, 2, replace=False)] = 0.05
        else:
            raise ValueError(k)
        W[v] = w / w.sum()
    out = dict(model)
    out['lbs_weights'] = W
    return out


def shrinking_regressor(verts, seed: int) -> np.ndarray:
    """'blocks' values in [0.3, 0.6], plus 8 weak entries in [0.002, 0.03] per row on other vertices of `verts`: J steps of 1e-2 drive
    weak entries below zero while every vertex stays in some row's support"""
    verts = np.asarray(verts, dtype=np.int64)
    rng = np.random.RandomState(seed)
    J = np.zeros((NH, V), np.float32)
    for i in range(NH):
        own = verts[i::NH]
        J[i, own] = rng.uniform(0.3, 0.6, len(own)).astype(np.float32)
        weak = rng.choice(np.setdiff1d(verts, own), 8, replace=False)
        J[i, weak] = rng.uniform(0.002, 0.03, 8).astype(np.float32)
    return J


def column_mask(drop) -> np.ndarray:
    """a (17, 6890) mask of ones that zeroes the columns `drop` in every row"""
    m = np.ones((NH, V), np.float32)
    m[:, np.asarray(drop, dtype=np.int64)] = 0.0
    return m


def effective(J, mask=None) -> np.ndarray:
    """the entries that reach the joints: ReLU(J * mask) (scripts/utils.py:87-92, before the row normalisation)"""
    return np.maximum(J if mask is None else J * mask, 0.0)


def structure(model, J, mask=None) -> dict:
    """what the kernels' tables look like for this regressor on this body"""
    P = effective(J, mask) > 0
    sup = np.nonzero(P.any(0))[0]
    Wn = model['lbs_weights'][sup] != 0
    return dict(nsv=len(sup), entries=int(P.sum()), row_counts=[int(c) for c in P.sum(1)], max_reads=int(P.sum(0).max()),
                influences={int(k): int(c) for k, c in enumerate(np.bincount(Wn.sum(1))) if c}, per_joint=[int(c) for c in Wn.sum(0)],
                support=sup)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# id -> (vertices, n, layout, body, mask, hinted, B); vertices: 'spread' / 'joint7' / 'wrists'; body: 'surface' / 'influences'.
# The seed of the vertex set and of the regressor is n (one_joint: 1, wrists: 2, influences: 9, masked: 72).
B_DEFAULT = 33          # two workgroups, the second with one real pose; BP = 128
SPEC = {
    'n2_blocks': ('spread', 2, 'blocks', 'surface', False, False, B_DEFAULT),
    'n2_dense': ('spread', 2, 'dense', 'surface', False, False, B_DEFAULT),
    'n17_diag': ('spread', 17, 'blocks', 'surface', False, False, B_DEFAULT),
    'n32': ('spread', 32, 'blocks', 'surface', False, False, B_DEFAULT),
    'n33': ('spread', 33, 'blocks', 'surface', False, False, B_DEFAULT),
    'n63': ('spread', 63, 'blocks', 'surface', False, False, B_DEFAULT),
    'n64_blocks': ('spread', 64, 'blocks', 'surface', False, False, B_DEFAULT),
    'n33_dense': ('spread', 33, 'dense', 'surface', False, False, B_DEFAULT),
    'n64_dense': ('spread', 64, 'dense', 'surface', False, False, B_DEFAULT),
    'n65': ('spread', 65, 'blocks', 'surface', False, False, B_DEFAULT),
    'one_joint': ('joint7', 64, 'dense', 'surface', False, False, B_DEFAULT),
    'wrists': ('wrists', 25, 'blocks', 'surface', False, False, B_DEFAULT),
    'influences': ('spread', 64, 'dense', 'influences', False, False, B_DEFAULT),
    'masked': ('spread', 72, 'dense', 'surface', True, False, B_DEFAULT),
    'n64_dense_hinted': ('spread', 64, 'dense', 'surface', False, True, B_DEFAULT),
    'n33_hinted': ('spread', 33, 'blocks', 'surface', False, True, B_DEFAULT),
    'n64_dense_B1': ('spread', 64, 'dense', 'surface', False, False, 1),
}
INFLUENCE_COUNTS = (1, 2, 3, 4, 6)        # cycling over the 64 support vertices of `influences`
INFLUENCE_SEED = 9
ONE_JOINT = 7
MASKED_DROP = 8
BATCH_SEED = 5

# What each case must look like (tests/test_support_cases.py): support vertices, positive entries, fewest / most entries of a row, most
# rows that read one vertex, support vertices by number of skinning influences.
EXPECT = {
    'n2_blocks': dict(nsv=2, entries=17, row_min=1, row_max=1, max_reads=9, influences={4: 2}),
    'n2_dense': dict(nsv=2, entries=34, row_min=2, row_max=2, max_reads=17, influences={4: 2}),
    'n17_diag': dict(nsv=17, entries=17, row_min=1, row_max=1, max_reads=1, influences={4: 17}),
    'n32': dict(nsv=32, entries=32, row_min=1, row_max=2, max_reads=1, influences={4: 32}),
    'n33': dict(nsv=33, entries=33, row_min=1, row_max=2, max_reads=1, influences={4: 33}),
    'n63': dict(nsv=63, entries=63, row_min=3, row_max=4, max_reads=1, influences={4: 63}),
    'n64_blocks': dict(nsv=64, entries=64, row_min=3, row_max=4, max_reads=1, influences={4: 64}),
    'n33_dense': dict(nsv=33, entries=561, row_min=33, row_max=33, max_reads=17, influences={4: 33}),
    'n64_dense': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={4: 64}),
    'n65': dict(nsv=65, entries=65, row_min=3, row_max=4, max_reads=1, influences={4: 65}),
    'one_joint': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={4: 64}),
    'wrists': dict(nsv=25, entries=25, row_min=1, row_max=2, max_reads=1, influences={4: 25}),
    'influences': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={1: 13, 2: 13, 3: 13, 4: 13, 6: 12}),
    'masked': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={4: 64}),
    'n64_dense_hinted': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={4: 64}),
    'n33_hinted': dict(nsv=33, entries=33, row_min=1, row_max=2, max_reads=1, influences={4: 33}),
    'n64_dense_B1': dict(nsv=64, entries=1088, row_min=64, row_max=64, max_reads=17, influences={4: 64}),
}


def build(model, case: str) -> dict:
    """the case's body, regressor, mask (or None), vertex hint (or None) and batch size"""
    kind, n, layout, body, masked, hinted, B = SPEC[case]
    seed = {'joint7': 1, 'wrists': 2}.get(kind, INFLUENCE_SEED if body == 'influences' else n)
    if kind == 'spread':
        verts = vertices_spread(n, seed)
    elif kind == 'joint7':
        verts = vertices_of_joint(model, n, ONE_JOINT, seed)
    else:
        verts = vertices_wrists(model)
    J = regressor(verts, layout, seed)
    mask = column_mask(verts[3::9][:MASKED_DROP]) if masked else None
    if body == 'influences':
        model = with_influences(model, verts, [INFLUENCE_COUNTS[k % len(INFLUENCE_COUNTS)] for k in range(len(verts))])
    support = np.nonzero((effective(J, mask) > 0).any(0))[0]
    return dict(model=model, body=body, J=J, mask=mask, verts=verts, support=support, hint=support if hinted else None, B=B)


# ---- the shrinking support ----------------------------------------------------------------------------------------------------------
SHRINK_SEED = 4
SHRINK_ITERS = 6
SHRINK_J_LR = 1e-2


def shrinking_case() -> np.ndarray:
    return shrinking_regressor(vertices_spread(SUP_NSV, SHRINK_SEED), SHRINK_SEED)


def shrinking_oracle(model, J0: np.ndarray, B: int, sm) -> dict:
    """the oracle loop of tests/test_gpu_trajectory.py::config2_oracle_j_steps without the discriminator and with a J step after EVERY
    iteration: torch Adam for the poses kept across the J steps, oracle.adam_step for the raw regressor.  `sm`: the package's
    smpl_model module.  Returns the inputs, the refined poses, the final J and, per J step, the positive entries after it and the
    smallest |J| among the entries that were positive before it (how far the closest entry is from changing sides)."""
    import torch
    import oracle
    T = torch.from_numpy
    batch = sm.synthetic_batch(model, J0, B, seed=BATCH_SEED)
    x6d, betas = T(batch['pose6d']), T(batch['betas'])
    gt_c = oracle.move_pelvis(T(batch['gt_j3d']))
    smpl = oracle.OracleSMPL(model)
    J = T(J0).clone()
    mask = oracle.find_j_reg_mask(J)
    orient = x6d[:, :1].clone().requires_grad_(True)
    pose = x6d[:, 1:].clone().requires_grad_(True)
    b = betas.clone().requires_grad_(True)
    opt = torch.optim.Adam([pose, orient, b], lr=1e-2)
    Jm, Jv = torch.zeros_like(J), torch.zeros_like(J)
    positive, margin = [], []
    for it in range(SHRINK_ITERS):
        loss, _, _ = oracle.inner_losses(smpl, J, mask, orient, pose, b, gt_c)
        opt.zero_grad()
        loss.backward()
        opt.step()
        _, dJ, _ = oracle.j_regressor_loss_and_grad(smpl, J, orient.detach(), pose.detach(), b.detach(), gt_c, mask=mask)
        before = J > 0
        oracle.adam_step(J, dJ, Jm, Jv, it + 1, SHRINK_J_LR)          # in place
        positive.append((J > 0).numpy().copy())
        margin.append(float(J[before].abs().min()))
    return dict(x6d=x6d, betas=betas, gt_c=gt_c, x=torch.cat([orient.detach(), pose.detach()], 1), b=b.detach(), J=J, positive=positive,
                margin=margin)
