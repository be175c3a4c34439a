"""Host restatement of the regressor fit (`--fit_regressor`, include/jrr.h jrr_jfit_*) and the cases its tests share.

`Restatement` is one Adam step of the J_regressor on fixed meshes, written in torch autograd line by line after the reference
(scripts/utils.py:87-98 find_joints without the SMPL call, :106-114 move_pelvis, scripts/optimize.py:300-312): relu, division by the
row sum, matmul, move_pelvis, MSELoss, torch.optim.Adam on the DENSE (17,V) parameter.  It runs in float32 and in float64.

Bounds: there is no second implementation, so a comparison is held to `bound(a32, a64) = 3 * max|a32 - a64| + 1e-7`, the distance of the
restatement's float32 evaluation from its float64 evaluation on the test's own inputs (the convention of accel_cases.bound).
"""
import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
NJ, V, CAP = 17, 6890, 128
# entries per row of the synthetic regressor: one row at the cap of 128, 260 entries in all
COUNTS = (5, 128, 2, 3, 4, 5, 6, 2, 3, 4, 5, 6, 7, 3, 4, 11, 62)
N_COLS = 400                  # the vertex columns the synthetic table lives on
N_ROWS, BATCH = 150, 64       # minibatches of 64, 64 and 22
LR = 1e-2
TRAJECTORY_SEED = 2           # searched on the CPU (test_regressor_fit.py checks the conditions it was searched for)


def bound(a32, a64) -> float:
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    return 3.0 * float(np.max(np.abs(a32 - a64))) + 1e-7 if a64.size else 1e-7


def dist(got, want) -> float:
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.max(np.abs(got - want))) if want.size else 0.0


def normalise(J: torch.Tensor, mask=None) -> torch.Tensor:
    x = torch.nn.ReLU()(J if mask is None else J * mask)
    return x / torch.sum(x, dim=1).unsqueeze(1).expand(x.shape)


def move_pelvis(j3ds: torch.Tensor) -> torch.Tensor:
    pelvis = j3ds[:, [0], :].clone()
    out = j3ds.clone()
    out -= pelvis
    return out


class Restatement:
    """J (17,V) raw, mask (17,V) or None, as numpy float32; the state lives in `dtype`"""

    def __init__(self, J, mask=None, lr=LR, dtype=F64):
        self.dtype = dtype
        self.J = torch.tensor(np.asarray(J, dtype=np.float32), dtype=dtype, requires_grad=True)
        self.mask = None if mask is None else torch.tensor(np.asarray(mask, dtype=np.float32), dtype=dtype)
        self.opt = torch.optim.Adam([self.J], lr=lr)

    def _t(self, a):
        return torch.tensor(np.asarray(a, dtype=np.float32), dtype=self.dtype)

    def normalised(self) -> np.ndarray:
        with torch.no_grad():
            return normalise(self.J, self.mask).numpy().copy()

    def raw(self) -> np.ndarray:
        return self.J.detach().numpy().copy()

    def joints(self, verts) -> np.ndarray:
        with torch.no_grad():
            return torch.matmul(normalise(self.J, self.mask)[None], self._t(verts)).numpy()

    def loss_and_grad(self, verts, gt_mm):
        """(loss, dense gradient (17,V)) without a step"""
        self.opt.zero_grad()
        pred = torch.matmul(normalise(self.J, self.mask)[None].expand(len(verts), -1, -1), self._t(verts))
        loss = torch.nn.MSELoss()(move_pelvis(pred), self._t(gt_mm) / 1000)
        loss.backward()
        return float(loss.item()), self.J.grad.detach().numpy().copy()

    def step(self, verts, gt_mm):
        """one Adam step; returns (the loss before the update, the gradient)"""
        loss, grad = self.loss_and_grad(verts, gt_mm)
        self.opt.step()
        return loss, grad

    def moments(self):
        st = self.opt.state[self.J]
        return st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()


def schedule(n_rows, batch):
    return [(a, min(batch, n_rows - a)) for a in range(0, n_rows, batch)]


def run(J, mask, verts, gt_mm, batch, n_steps, dtype, lr=LR, first=0, watch=None):
    """n_steps steps over the minibatches first, first + 1, ... of the table, wrapping around after the last one (epochs in table
    order).  Returns (Restatement, losses, last gradient).  watch(step, restatement) is called after every step."""
    r = Restatement(J, mask, lr, dtype)
    steps = schedule(len(verts), batch)
    losses, grad = [], None
    for k in range(n_steps):
        a, n = steps[(first + k) % len(steps)]
        loss, grad = r.step(verts[a:a + n], gt_mm[a:a + n])
        losses.append(loss)
        if watch is not None:
            watch(k, r)
    return r, np.array(losses), grad


def to_lists(dense, vtx):
    """(17,128): the dense array's values on the rows' lists (vtx: per row the vertices, ascending), zeros behind a row's count"""
    out = np.zeros((NJ, CAP), dtype=np.asarray(dense).dtype)
    for i, v in enumerate(vtx):
        out[i, :len(v)] = np.asarray(dense)[i, v]
    return out


def regressor_case(seed, counts=COUNTS, n_cols=N_COLS, lo=0.02, hi=0.3):
    """(J (17,6890) float32, mask (17,6890) float32 of zeros and ones, cols (n_cols,), vtx: per row its listed vertices).  Row i has
    counts[i] positive entries of J * mask on the chosen columns; row 1 shares three vertices with row 0; the mask removes one further
    positive entry of rows 0 and 16, and J carries a few negative entries, which are never listed."""
    rng = np.random.RandomState(seed)
    cols = np.sort(rng.choice(V, n_cols, replace=False))
    J = np.zeros((NJ, V), dtype=np.float32)
    mask = np.ones((NJ, V), dtype=np.float32)
    vtx = []
    for i, n in enumerate(counts):
        if i == 1:
            shared = rng.choice(vtx[0], 3, replace=False)
            rest = rng.choice(np.setdiff1d(cols, shared), n - 3, replace=False)
            v = np.sort(np.concatenate([shared, rest]))
        else:
            v = np.sort(rng.choice(cols, n, replace=False))
        J[i, v] = rng.uniform(lo, hi, size=n).astype(np.float32)
        free = np.setdiff1d(cols, v)
        J[i, rng.choice(free, 2, replace=False)] = -rng.uniform(lo, hi, size=2).astype(np.float32)
        if i in (0, 16):
            extra = rng.choice(np.setdiff1d(free, np.flatnonzero(J[i])), 1)
            J[i, extra] = 0.1
            mask[i, extra] = 0.0
        vtx.append(v)
    return J, mask, cols, vtx


def table_case(seed, J, mask, cols, n_rows=N_ROWS, noise_mm=10.0):
    """(verts (n_rows,6890,3) float32: random points of body size at the chosen columns, zero elsewhere; gt_mm (n_rows,17,3) float32:
    pelvis-centred joints of ANOTHER regressor on the same support, in mm, with noise)"""
    rng = np.random.RandomState(seed + 1000)
    verts = np.zeros((n_rows, V, 3), dtype=np.float32)
    verts[:, cols] = (rng.normal(0, 1, size=(n_rows, len(cols), 3)) * np.array([0.15, 0.5, 0.1])).astype(np.float32)
    on = (J * mask) > 0
    other = np.where(on, rng.uniform(0.02, 0.3, size=J.shape), 0.0)
    other = other / other.sum(1, keepdims=True)
    joints = np.einsum('jv,bvc->bjc', other, verts.astype(np.float64))
    gt = (joints - joints[:, :1]) * 1000.0 + rng.normal(0, noise_mm, size=joints.shape)
    gt = gt - gt[:, :1]
    return verts, gt.astype(np.float32)


_CACHE = {}


def trajectory_case(seed=TRAJECTORY_SEED):
    """the shared case of the GPU tests (built once): regressor, mask, table, and the restatement's 30-step runs in both precisions with
    a snapshot after every epoch of three minibatches: the raw entries and the normalised weights on the lists, the joints of the whole table"""
    if seed in _CACHE:
        return _CACHE[seed]
    J, mask, cols, vtx = regressor_case(seed)
    verts, gt = table_case(seed, J, mask, cols)
    out = {'J': J, 'mask': mask, 'cols': cols, 'vtx': vtx, 'verts': verts, 'gt': gt}
    for name, dtype in (('f32', F32), ('f64', F64)):
        snaps, closest = [], [np.inf]

        def watch(k, r, snaps=snaps, closest=closest):
            raw = to_lists(r.raw(), vtx)
            listed = to_lists(np.ones((NJ, V)), vtx) > 0
            closest[0] = min(closest[0], float(np.abs(raw[listed]).min()))
            if (k + 1) % 3 == 0:
                snaps.append({'raw': raw, 'jn': to_lists(r.normalised(), vtx), 'joints': r.joints(verts)})
        r, losses, grad = run(J, mask, verts, gt, BATCH, 30, dtype, watch=watch)
        out[name] = {'snaps': snaps, 'losses': losses, 'closest': closest[0], 'final': r}
    _CACHE[seed] = out
    return out
