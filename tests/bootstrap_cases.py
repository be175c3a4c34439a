"""Host restatement and seeded inputs of the paired bootstrap (`--eval_ci`; tests/test_bootstrap.py, tests/test_gpu_bootstrap.py).

Written from include/jrr.h (jrr_paired_units, jrr_bootstrap_sums, JRR_BOOT_*), which is the specification, and from the Philox paper
(Salmon, Moraes, Dror, Shaw, SC11): Philox4x32-10 in uint64 numpy arithmetic, the draw rule, the pose -> unit accumulation in Python
integers, the order of units and segments, and the float64 derivation.  Everything behind the fp32 errors is an integer, so the GPU
path is compared with this file by exact equality."""
import numpy as np

F = np.float32
NJ = 17
UNIT_ROW, WINS_ROW, WINS_TRAILER = 5, 8, 3
M32 = np.uint64(0xffffffff)
PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


# ---- Philox4x32-10 and the draw rule -------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """counter (...,4) and key (2,) of 32-bit words -> (...,4) uint64 arrays holding the 32-bit output words"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & M32 for i in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xffffffff), np.uint64(int(key[1]) & 0xffffffff)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]              # < 2^64: both factors are below 2^32
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack(c, axis=-1)


def draws(seed: int, reps, s: int, count: int) -> np.ndarray:
    """(len(reps), count) int64: draw i of replicate r of segment s, in [0, count): ((w * count) >> 32) with w the word i & 3 of
    Philox at counter (i >> 2, r, s, 0) under key (seed & 0xffffffff, seed >> 32)"""
    reps = np.asarray(reps, dtype=np.uint64).reshape(-1)
    if count == 0:
        return np.zeros((reps.shape[0], 0), dtype=np.int64)
    seed = int(seed) & 0xffffffffffffffff
    n_blocks = (count + 3) // 4
    ctr = np.zeros((reps.shape[0], n_blocks, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(n_blocks, dtype=np.uint64)[None, :]
    ctr[..., 1] = reps[:, None]
    ctr[..., 2] = np.uint64(s)
    w = philox4x32_10(ctr, (seed & 0xffffffff, seed >> 32)).reshape(reps.shape[0], n_blocks * 4)[:, :count]
    return ((w * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def bootstrap_sums(units: np.ndarray, segments, seed: int, rep_begin: int, rep_count: int) -> np.ndarray:
    """(n_seg, rep_count, 5) int64 as jrr_bootstrap_sums defines it (the caller keeps the sums inside int64: numpy adds exactly there)"""
    units, segments = np.asarray(units, dtype=np.int64), np.asarray(segments, dtype=np.int64).reshape(-1, 2)
    out = np.zeros((segments.shape[0], rep_count, UNIT_ROW), dtype=np.int64)
    reps = np.arange(rep_begin, rep_begin + rep_count)
    for s, (begin, count) in enumerate(segments):
        idx = draws(seed, reps, s, int(count))
        out[s] = units[int(begin) + idx].sum(1) if count else 0
    return out


# ---- pose -> unit ------------------------------------------------------------------------------------------------------------------
def fixed24(e) -> np.ndarray:
    """rn(e * 2^24) of fp32 values as Python-exact int64: the product is exact in fp32 (a power of two), numpy rounds ties to even"""
    return np.rint(np.asarray(e, dtype=F) * F(16777216.0)).astype(np.float64).astype(np.int64)


def paired_units(eb, eb_pa, ea, ea_pa, group, unit, n_groups: int, n_units: int):
    """(units (n_units,5) int64, wins (n_groups * 8 + 3,) int64) of jrr_paired_units, accumulated in Python integers"""
    units = [[0] * UNIT_ROW for _ in range(n_units)]
    wins = [0] * (n_groups * WINS_ROW + WINS_TRAILER)
    arrays = [np.asarray(a, dtype=F) for a in (eb, eb_pa, ea, ea_pa)]
    for b in range(arrays[0].shape[0]):
        g, u = int(group[b]), int(unit[b])
        if g < 0:
            wins[n_groups * WINS_ROW + 0] += 1
        elif g >= n_groups:
            wins[n_groups * WINS_ROW + 1] += 1
        elif u < 0 or u >= n_units:
            wins[n_groups * WINS_ROW + 2] += 1
        elif not all(bool((a[b] < F(1.0e3)).all()) for a in arrays):
            wins[g * WINS_ROW + 1] += 1
        else:
            S = [sum(int(x) for x in fixed24(a[b])) for a in arrays]
            for c in range(4):
                units[u][c] += S[c]
            units[u][4] += 1
            wins[g * WINS_ROW + 0] += 1
            wins[g * WINS_ROW + (2 if S[2] < S[0] else 3 if S[2] > S[0] else 4)] += 1
            wins[g * WINS_ROW + (5 if S[3] < S[1] else 6 if S[3] > S[1] else 7)] += 1
    return np.array(units, dtype=np.int64).reshape(n_units, UNIT_ROW), np.array(wins, dtype=np.int64)


def plan(units, group_of_unit, n_groups: int):
    """(kept unit ids ordered by (group, unit id), segments (1 + n_groups, 2)): units without a counted pose are dropped; segment 0 is
    every kept unit, segment 1 + g the kept units of group g"""
    kept = sorted((int(group_of_unit[u]), u) for u in range(len(units)) if units[u][4] > 0)
    segments, at = [[0, len(kept)]], 0
    for g in range(n_groups):
        n = sum(1 for gg, _ in kept if gg == g)
        segments.append([at, n])
        at += n
    return np.array([u for _, u in kept], dtype=np.int64), np.array(segments, dtype=np.int64)


# ---- the derivation ----------------------------------------------------------------------------------------------------------------
def mean_mm(total, count):
    return total / float(1 << 24) / (NJ * count) * 1000.0


def interval(point, reps, level):
    lo, hi = np.percentile(reps, [100.0 * (1.0 - level) / 2.0, 100.0 * (1.0 + level) / 2.0])
    return {'mean_mm': float(point), 'lo_mm': float(lo), 'hi_mm': float(hi), 'se_mm': float(np.std(reps))}


def stats(point, reps, n_units, wrow, level):
    n = int(point[4])
    out = {'n_units': int(n_units), 'n_poses': n, 'n_bad': int(wrow[1]), 'raw_sums': [int(x) for x in point],
           'wins': {'mpjpe': {'better': int(wrow[2]), 'worse': int(wrow[3]), 'tie': int(wrow[4])},
                    'pampjpe': {'better': int(wrow[5]), 'worse': int(wrow[6]), 'tie': int(wrow[7])}}}
    for key, cb, ca in (('mpjpe', 0, 2), ('pampjpe', 1, 3)):
        if n == 0:
            out[key] = None
            continue
        counts = reps[:, 4].astype(np.float64)
        pb, pa = mean_mm(np.float64(point[cb]), np.float64(n)), mean_mm(np.float64(point[ca]), np.float64(n))
        rb, ra = mean_mm(reps[:, cb].astype(np.float64), counts), mean_mm(reps[:, ca].astype(np.float64), counts)
        diff = interval(pa - pb, ra - rb, level)
        diff['p_not_better'] = float(np.mean(ra - rb >= 0.0))
        out[key] = {'before': interval(pb, rb, level), 'after': interval(pa, ra, level), 'difference': diff}
    return out


def document(eb, eb_pa, ea, ea_pa, group, unit, group_of_unit, names, n_units: int, reps: int, seed: int, level: float, unit_kind: str) -> dict:
    """what ci_report.PairedBootstrap.finish returns for these per-joint errors: the `data` member of ci.json"""
    G = len(names)
    units, wins = paired_units(eb, eb_pa, ea, ea_pa, group, unit, G, n_units)
    kept, segments = plan(units, group_of_unit, G)
    table = units[kept]
    sums = bootstrap_sums(table, segments, seed, 0, reps) if len(kept) else np.zeros((G + 1, reps, UNIT_ROW), dtype=np.int64)
    wrows = wins[:G * WINS_ROW].reshape(G, WINS_ROW)
    point = lambda s: table[segments[s, 0]:segments[s, 0] + segments[s, 1]].sum(0) if segments[s, 1] else np.zeros(UNIT_ROW, dtype=np.int64)
    return {'groups': {name: stats(point(1 + i), sums[1 + i], segments[1 + i, 1], wrows[i], level) for i, name in enumerate(names)},
            'all': stats(point(0), sums[0], segments[0, 1], wrows.sum(0), level), 'ignored': int(wins[G * WINS_ROW]), 'reps': int(reps),
            'seed': int(seed), 'level': float(level), 'unit': unit_kind}


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------
SEGMENT_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 257, 1000)      # the Philox block edge, the wave edge (64 blocks = 256 draws), more than one pass
KERNEL_SEED = (0x9e3779b9 << 32) | 0x12345678                 # a non-zero high word
KERNEL_REPS, KERNEL_REP_BEGIN = 37, 11


def kernel_case():
    """(units (1462,5) int64 with the four sums above 2^40 -- a 32-bit accumulation or reduction loses them --, segments (10,2))"""
    rs = np.random.RandomState(2024)
    n = sum(SEGMENT_COUNTS)
    units = np.empty((n, UNIT_ROW), dtype=np.int64)
    units[:, :4] = rs.randint(1 << 40, 1 << 41, size=(n, 4), dtype=np.int64) + rs.randint(0, 1 << 20, size=(n, 4), dtype=np.int64)
    units[:, 4] = rs.randint(1, 6, size=n)
    begin = np.concatenate([[0], np.cumsum(SEGMENT_COUNTS)[:-1]])
    return units, np.stack([begin, np.array(SEGMENT_COUNTS)], axis=1).astype(np.int64)


POSE_B, POSE_UNITS, POSE_GROUPS = 130, 9, 3                   # three workgroups of 64 poses, the last with 2
POSE_IGNORED, POSE_BAD_GROUP, POSE_BAD_UNIT, POSE_NAN, POSE_TIES = 3, 77, 129, 100, (5, 64, 110)


def pose_case():
    """(eb, eb_pa, ea, ea_pa (130,17) float32 metres, group (130,), unit (130,) int32): unit u belongs to group u % 3; poses 20 .. 89
    form the 70-pose unit 4, which spans the first two workgroups; one pose each with group -1, group 3 and unit 9; one with a NaN in
    the after-aligned array only; three ties by identical before / after rows"""
    rs = np.random.RandomState(7)
    eb, eb_pa = (rs.rand(POSE_B, NJ) * 0.2).astype(F), (rs.rand(POSE_B, NJ) * 0.1).astype(F)
    ea, ea_pa = (eb + rs.randn(POSE_B, NJ).astype(F) * F(0.01)).astype(F), (eb_pa + rs.randn(POSE_B, NJ).astype(F) * F(0.005)).astype(F)
    ea, ea_pa = np.abs(ea), np.abs(ea_pa)
    others = [u for u in range(POSE_UNITS) if u != 4]
    unit = np.array([others[b % 8] for b in range(POSE_B)], dtype=np.int32)
    unit[20:90] = 4
    group = (unit % POSE_GROUPS).astype(np.int32)
    group[POSE_IGNORED], group[POSE_BAD_GROUP], unit[POSE_BAD_UNIT] = -1, POSE_GROUPS, POSE_UNITS
    ea_pa[POSE_NAN, 11] = np.nan
    for b in POSE_TIES:
        ea[b], ea_pa[b] = eb[b], eb_pa[b]
    return eb, eb_pa, ea, ea_pa, group, unit


def independent_units(n: int, seed: int):
    """(units (n,5) int64, x (n,) float64): n frame units of one pose each with independent paired errors -- before ~ 60 mm, the
    difference ~ N(-1 mm, 4 mm) per pose --, and the per-unit difference of the means in mm the analytic standard error is taken of"""
    rs = np.random.RandomState(seed)
    before = np.abs(0.06 + 0.02 * rs.randn(n, NJ)).astype(F)
    after = np.abs(before + (-0.001 + 0.004 * rs.randn(n, 1)) + 0.002 * rs.randn(n, NJ)).astype(F)
    units = np.zeros((n, UNIT_ROW), dtype=np.int64)
    units[:, 0], units[:, 1] = fixed24(before).sum(1), fixed24(before * F(0.5)).sum(1)
    units[:, 2], units[:, 3] = fixed24(after).sum(1), fixed24(after * F(0.5)).sum(1)
    units[:, 4] = 1
    x = mean_mm((units[:, 2] - units[:, 0]).astype(np.float64), 1.0)
    return units, x


# ---- stand-ins for a CPU run of ci_report.PairedBootstrap (tests/test_bootstrap.py: one process against two gloo ranks) ------------
def clean_pose_case():
    """pose_case without the two poses finish() refuses (group 3, unit 9): (the six arrays, group of every row as the host knows it)"""
    case = pose_case()
    keep = np.ones(POSE_B, dtype=bool)
    keep[[POSE_BAD_GROUP, POSE_BAD_UNIT]] = False
    case = [a[keep] for a in case]
    return case, np.where(case[4] < 0, case[5] % POSE_GROUPS, case[4]).astype(np.int32)


def fill(boot, case, lo: int, hi: int) -> None:
    """what PairedBootstrap.add leaves in the tables of `boot` for poses [lo, hi) of the case"""
    import torch
    units, wins = paired_units(*[a[lo:hi] for a in case], POSE_GROUPS, POSE_UNITS)
    boot.units += torch.from_numpy(units)
    boot.wins += torch.from_numpy(wins)


def host_bootstrap_sums(units, segments, seed, rep_begin, rep_count, max_word=None, out=None):
    """engine.bootstrap_sums on CPU tensors"""
    import torch
    return torch.from_numpy(bootstrap_sums(units.numpy(), segments, seed, rep_begin, rep_count))
