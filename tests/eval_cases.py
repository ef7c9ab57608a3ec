"""Inputs and references for the tests of the tracking kernels' evaluations alone
(include/eval/hc_eval_testing.h, hc_trifocal_eval_variant_batched): built on the
CPU, deterministic, shared by test_eval_cases_host.py and
test_gpu_eval_variants.py as lu_cases.py is by the LU's tests.

Two references:

* the oracle (bit-exact bar): p = param_homotopy(t, start, target), eval_hx,
  and eval_ht (kind 0: the negated dH/dt, the stage's right-hand side) or
  eval_h (kind 1);
* plain complex128 numpy from the raw index tables, in the manner of
  residual.py, at the fp32 p the oracle staged, each value with S = sum_j
  |term_j| (dH/dt: the magnitudes of both products of a term).

Point families (Points): path_points, scaled_points, threshold_points,
nonfinite_points; orders of points and kinds over the path slots of a workgroup:
arrangement; index tables: tables, rejected_table.
"""
from dataclasses import dataclass

import numpy as np

NV, NPP = 30, 34
IDLE = 2                      # HC_EVAL_KIND_IDLE: the slot is left without a point
U32 = 2.0 ** -24              # unit roundoff of fp32
BOUND_UNITS = 32.0            # |value - fp64| <= BOUND_UNITS * U32 * S (first order: <= 27 u, see test_eval_cases_host)
F32_TINY, F32_HUGE = 2.0 ** -126, float(np.finfo(np.float32).max)
SWAP = (0, 9)                 # a row order outside the specialised LU's structure
BANDS = ((61, 62), (64, 66), (70, 72))   # threshold_points: log2 of the largest dH/dx component


# ------------------------------------------------------------------ index tables
def row_permuted(problem, perm):
    """The index tables with the equations (rows) reordered: row r of the new
    system is row perm[r] of the reference's (a valid, equivalent problem).
    Returns (dHdx, dHdt, unified)."""
    dx = problem.dHdx_index.reshape(-1, 30)[:, perm].reshape(-1)
    dt = problem.dHdt_index.reshape(-1, 30)[:, perm].reshape(-1)
    return (np.ascontiguousarray(dx, np.int32), np.ascontiguousarray(dt, np.int32),
            np.ascontiguousarray(np.concatenate([dx, dt]), np.int32))


def owner_helper_perm():
    """Rows r <-> r + 16 for r = 2..13: the twelve rows of 13 or 16 dH/dt terms
    (18..29, the owners) sit in lanes 2..13 and their 10-term partners (the
    helpers) in lanes 18..29."""
    perm = np.arange(30)
    for r in range(2, 14):
        perm[r], perm[r + 16] = r + 16, r
    return perm


def tables(problem):
    """{name: (dHdx, dHdt, unified)}: the problem's own table, the row swap of
    test_gpu_abs_tables.py, and the exchange of owners and helpers."""
    swap = np.arange(30)
    swap[SWAP[0]], swap[SWAP[1]] = SWAP[1], SWAP[0]
    own = (np.ascontiguousarray(problem.dHdx_index, np.int32), np.ascontiguousarray(problem.dHdt_index, np.int32),
           np.ascontiguousarray(problem.unified_index, np.int32))
    return {"own": own, "swap_0_9": row_permuted(problem, swap), "owners_helpers": row_permuted(problem, owner_helper_perm())}


def rejected_table(problem):
    """The owner / helper exchange with one more 16-term row moved onto the
    partner lane of a 16-term row (lanes 2 and 18 hold rows 18 and 19): neither
    can help the other, and the table builder rejects the table."""
    perm = owner_helper_perm()
    perm[18], perm[3] = perm[3], perm[18]
    return row_permuted(problem, perm)[2]


def ht_terms_per_row(dt):
    return (np.asarray(dt).reshape(16, 6, 30)[:, 0, :] != 0).sum(axis=0)


def rows_reading(dx, dt, k):
    """(dH/dx entries (30, 30) bool [row][column], right-hand side rows (30,) bool)
    with a non-padding term that reads x[k]."""
    X = np.asarray(dx).reshape(30, 8, 5, 30)      # [c][j][part][r]
    reads = (X[:, :, 0, :] != 0) & ((X[:, :, 3, :] == k) | (X[:, :, 4, :] == k))
    T = np.asarray(dt).reshape(16, 6, 30)
    rr = (T[:, 0, :] != 0) & ((T[:, 3, :] == k) | (T[:, 4, :] == k) | (T[:, 5, :] == k))
    return reads.any(axis=1).T, rr.any(axis=0)


# ------------------------------------------------------------------ points
@dataclass
class Points:
    x: np.ndarray        # (n, 31, 2) float32, x[30] = 1
    target: np.ndarray   # (n, 34, 2) float32
    diff: np.ndarray     # (n, 34, 2) float32
    t: np.ndarray        # (n,) float32
    bad_x: np.ndarray    # (n,) the unknown made non-finite, -1: none

    def __len__(self):
        return self.x.shape[0]

    def take(self, idx):
        idx = np.asarray(idx)
        return Points(self.x[idx].copy(), self.target[idx].copy(), self.diff[idx].copy(), self.t[idx].copy(),
                      self.bad_x[idx].copy())

    def freeze(self):
        for a in (self.x, self.target, self.diff, self.t, self.bad_x):
            a.setflags(write=False)
        return self


def concat(parts):
    return Points(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("x", "target", "diff", "t", "bad_x")))


T_EDGES = (0.0, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0))), 2.0 ** -24, 0.5, 0.95)


def path_points(problem, samples100, n, seed):
    """Points as lu_cases.jacobians_from_path builds them (a start solution plus
    noise of 1e-4..1e-1, a random sample), keeping t and the sample; the first
    t are T_EDGES, the rest uniform draws."""
    tgt, dif, _ = samples100
    rng = np.random.default_rng(seed)
    xs, ts, tg, df = [], [], [], []
    for i in range(n):
        k = int(rng.integers(0, 312))
        s = int(rng.integers(0, tgt.shape[0]))
        x = problem.start_sols[k].copy()
        x[:30] += (rng.standard_normal((30, 2)) * 10 ** rng.uniform(-4, -1)).astype(np.float32)
        u = float(np.float32(rng.uniform(0, 1)))
        xs.append(x)
        ts.append(T_EDGES[i] if i < len(T_EDGES) else u)
        tg.append(tgt[s])
        df.append(dif[s])
    return Points(np.stack(xs).astype(np.float32), np.stack(tg).astype(np.float32), np.stack(df).astype(np.float32),
                  np.array(ts, np.float32), np.full(n, -1, np.int64))


X_SCALES = (-66, -40, -20, 20, 28)
P_SCALES = (12, 40)


def scaled_points(problem, samples100, per_scale=8, seed=21):
    """Path points with x[:30] times 2^e, e in X_SCALES, and with the target
    parameters times 2^12 and 2^40 (diff = target - start in fp32, as
    checks.scaled_samples makes it).  At 2^-66 the dH/dx entries are denormal
    and H's cubic terms underflow."""
    parts = []
    for j, e in enumerate(X_SCALES):
        p = path_points(problem, samples100, per_scale, seed + j)
        p.x[:, :30] *= np.float32(2.0 ** e)
        parts.append(p)
    for j, e in enumerate(P_SCALES):
        p = path_points(problem, samples100, per_scale, seed + 16 + j)
        p.target = (p.target * np.float32(2.0 ** e)).astype(np.float32)
        p.diff = (p.target - problem.start_params[None]).astype(np.float32)
        parts.append(p)
    return concat(parts)


def huge_partner_points(problem, samples100, n=4, seed=41):
    """Path points with the target parameters times 2^70 (checks.scaled_samples' far
    sample): partners whose values overflow."""
    p = path_points(problem, samples100, n, seed)
    p.target = (p.target * np.float32(2.0 ** 70)).astype(np.float32)
    p.diff = (p.target - problem.start_params[None]).astype(np.float32)
    return p


def _max_component(oracle, problem, dx, x, target, t):
    p = oracle.param_homotopy(float(t), problem.start_params, target)
    A = oracle.eval_hx(dx, x, p)
    return A


def false_rows(A):
    """Rows of a dH/dx (30, 30, 2) whose verdict must be false: a component
    that is not finite or at least 2^64 in magnitude."""
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(A) | (np.abs(A) >= np.float32(2.0 ** 64))
    return bad.any(axis=(1, 2))


def false_entries(A):
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(A) | (np.abs(A) >= np.float32(2.0 ** 64))
    return bad.any(axis=2)


def threshold_points(problem, samples100, oracle, per_band=16, seed=31):
    """For the finiteness verdict: path points whose x[:30] is scaled by the
    power of two that puts the largest dH/dx component, as the oracle computes
    it on the problem's table, into a band of BANDS (entries of mixed degree in
    x: a point for which no power of two does is passed over, and so is one of
    an upper band with fewer than 8 rows over the threshold).  Returns
    (points, band index per point)."""
    cand = path_points(problem, samples100, 12 * per_band, seed)
    dx = np.ascontiguousarray(problem.dHdx_index, np.int32)
    out, band = [], []
    for bi, (lo, hi) in enumerate(BANDS):
        got = 0
        for i in range(len(cand)):
            if got == per_band:
                break
            for e in range(20, 50):
                x = cand.x[i].copy()
                x[:30] *= np.float32(2.0 ** e)
                A = _max_component(oracle, problem, dx, x, cand.target[i], cand.t[i])
                if not np.isfinite(A).all():
                    break
                m = float(np.abs(A).max())
                if m >= 2.0 ** hi:
                    break
                if m >= 2.0 ** lo:
                    if bi == 0 or false_rows(A).sum() >= 8:
                        p = cand.take([i])
                        p.x[0] = x
                        out.append(p)
                        band.append(bi)
                        got += 1
                    break
        assert got == per_band, f"band {lo}..{hi}: only {got} points"
    return concat(out), np.array(band)


def nonfinite_points(problem, samples100, seed=51):
    """Path points with one component of one x[k] set to NaN, +Inf or -Inf:
    every unknown k with each of the three values, the real and the imaginary
    part in turn."""
    vals = (np.nan, np.inf, -np.inf)
    p = path_points(problem, samples100, 30 * len(vals), seed)
    for i in range(len(p)):
        k, v = i % 30, vals[i // 30]
        p.x[i, k, (i // 30 + k) % 2] = np.float32(v)
        p.bad_x[i] = k
    return p


# ------------------------------------------------------------------ arrangements
SAME, OTHER, ALONE = 0, 1, 2
COMBOS = tuple((s, k, pm) for s in range(8) for k in (0, 1) for pm in (SAME, OTHER, ALONE))


def arrangement(m, offset=0, partner_of=None):
    """An order of m points over the path slots: point j is placed in the slot,
    with the kind and beside the partner of combination (j + offset) % 48 of
    COMBOS (slot 0..7) x (own kind) x (partner of the same kind, of the other
    kind, none).  Its partner is point partner_of(j) (default j + 1, cyclic),
    which is evaluated as well.  Returns (idx, kind): the point and the kind
    (IDLE: no point) of each position; position i is slot i % 8 of workgroup
    i / 8, and the length is a multiple of 8."""
    per_wave = [[], [], [], []]
    for j in range(m):
        s, k, pm = COMBOS[(j + offset) % len(COMBOS)]
        q = (j + 1) % m if partner_of is None else partner_of(j)
        own, par = (j, k), (q, k if pm == SAME else 1 - k if pm == OTHER else IDLE)
        per_wave[s // 2].append((own, par) if s % 2 == 0 else (par, own))
    L = max(len(w) for w in per_wave)
    idx, kind = [], []
    for g in range(L):
        for w in per_wave:
            for i, k in (w[g] if g < len(w) else ((0, IDLE), (0, IDLE))):
                idx.append(i)
                kind.append(k)
    return np.array(idx), np.array(kind, np.uint8)


def coverage(kind):
    """The (slot, own kind, partner) combinations an order of kinds holds: the
    partner of position i is position i ^ 1, none if idle or past the end."""
    kind = np.asarray(kind)
    seen = set()
    for i, k in enumerate(kind):
        if k == IDLE:
            continue
        q = kind[i ^ 1] if (i ^ 1) < len(kind) else IDLE
        seen.add((i % 8, int(k), ALONE if q == IDLE else SAME if q == k else OTHER))
    return seen


# ------------------------------------------------------------------ references
def oracle_values(oracle, problem, dx, dt, pts):
    """(p (n, 34, 2), Hx (n, 30, 30, 2), ht (n, 30, 2), h (n, 30, 2)) of the oracle."""
    n = len(pts)
    P = np.zeros((n, NPP, 2), np.float32)
    HX = np.zeros((n, NV, NV, 2), np.float32)
    HT = np.zeros((n, NV, 2), np.float32)
    H = np.zeros((n, NV, 2), np.float32)
    for i in range(n):
        P[i] = oracle.param_homotopy(float(pts.t[i]), problem.start_params, pts.target[i])
        HX[i] = oracle.eval_hx(dx, pts.x[i], P[i])
        HT[i] = oracle.eval_ht(dt, pts.x[i], P[i], pts.diff[i])
        H[i] = oracle.eval_h(dt, pts.x[i], P[i])
    return P, HX, HT, H


def _c128(a):
    a = np.asarray(a, np.float64)
    out = a[..., 0].astype(np.complex128)
    out.imag = a[..., 1]        # (not re + 1j * im: an infinite im would make re NaN)
    return out


def fp64_values(dx, dt, x, p, d):
    """Plain complex128 evaluation from the raw tables at n points: x (n, 31, 2),
    p and d (n, 34, 2) fp32 values.  Returns ((Hx, S) (n, 30, 30), (ht, S) and
    (h, S) (n, 30)); ht is the negated dH/dt."""
    xx, pp, dd = _c128(x).copy(), _c128(p).copy(), _c128(d)
    X = np.asarray(dx).reshape(30, 8, 5, 30)       # [c][j][part][r]
    co = X[:, :, 0, :].astype(np.float64)
    with np.errstate(all="ignore"):
        tx = co * pp[:, X[:, :, 1, :]] * pp[:, X[:, :, 2, :]] * xx[:, X[:, :, 3, :]] * xx[:, X[:, :, 4, :]]   # (n, c, j, r)
        hx = (tx.sum(axis=2).transpose(0, 2, 1), np.abs(tx).sum(axis=2).transpose(0, 2, 1))
        T = np.asarray(dt).reshape(16, 6, 30)      # [j][part][r]
        c = T[:, 0, :].astype(np.float64)
        a, b = T[:, 1, :], T[:, 2, :]
        xs = xx[:, T[:, 3, :]] * xx[:, T[:, 4, :]] * xx[:, T[:, 5, :]]
        th = c * pp[:, a] * pp[:, b] * xs
        h = (th.sum(axis=1), np.abs(th).sum(axis=1))
        t1, t2 = c * dd[:, a] * pp[:, b] * xs, c * dd[:, b] * pp[:, a] * xs
        ht = (-(t1 + t2).sum(axis=1), (np.abs(t1) + np.abs(t2)).sum(axis=1))
    return hx, ht, h


def bound_check(val, ref):
    """val: fp32 values (..., 2); ref: (fp64 value, S).  Returns (ok, excluded,
    units): ok where the value is within BOUND_UNITS * u * S of the fp64 one
    (exactly 0 where S == 0) or excluded; excluded where S or the result leaves
    the fp32 normal range (judged on the fp64 reference alone); units: the
    error in units of u * S (0 where excluded or S == 0)."""
    v, S = ref
    with np.errstate(all="ignore"):
        excluded = (S > 0) & (~np.isfinite(S) | (S < F32_TINY) | (S > F32_HUGE) | ((np.abs(v) < F32_TINY) & (v != 0)))
        got = _c128(val)
        err = np.abs(got - v)
        units = np.where((S > 0) & ~excluded, err / (U32 * np.where(S > 0, S, 1.0)), 0.0)
        ok = np.where(S == 0, got == 0, excluded | (units <= BOUND_UNITS))
    return ok, excluded, units
