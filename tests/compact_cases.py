"""Systems for the GPU test of the fused solve on its compact row
(test_gpu_lu_compact.py), built on lu_cases.py's builders and accounted for by
the oracle's trace (oracle.cgesv_gpu_trace), never by a re-simulation.

In every system each low entry (columns 0..17) of the compiled-in pattern is
non-zero with a magnitude |re| + |im| of its own, so a value that reaches a
wrong slot of the compact row is a wrong value somewhere.

* forced: for each chain of each fused level, one system per candidate row in
  which that row is the chain's pivot row (90 systems: 30 + 24 + 24 + 12 rows).
  Rows 18..20 against 24..26, and 21..23 against 27..29, share slot 0 with
  different columns and merge into one chain at level 1: both sides are there;
* redo: a pivot below 2^-90 inside level 0 (step 5) and one at the sequential
  step 25, each beside a plain partner in its wave, which is re-solved with it.
"""
import numpy as np

import lu_cases

NV = lu_cases.NV
_cache = {}


def _own_magnitudes(rng, mask):
    """Random values on the pattern; the low entries replaced by values whose
    |re| + |im| are distinct (2^-3 .. 2^3, exact in fp32) in one of eight directions."""
    A = lu_cases._random_on_pattern(rng, mask, 1)[0]
    low = [(r, c) for r in range(NV) for c in lu_cases.FUSED if mask[r, c]]
    mags = (2.0 ** -3 * (1.0 + np.arange(len(low)) / len(low)) * 2.0 ** rng.integers(0, 6, len(low))).astype(np.float32)
    assert len(set(mags.tolist())) == len(low)
    for (r, c), m, d in zip(low, rng.permutation(mags), rng.integers(0, 8, len(low))):
        h = np.float32(m / 2)
        A[r, c] = [(m, 0), (-m, 0), (0, m), (0, -m), (h, h), (h, -h), (-h, h), (-h, -h)][d]
    return A.astype(np.float32)


def batch(oracle):
    """dict(A, b, names, ref, trace, forced, redo): forced[(step, row)] = the
    system in which `row` is the pivot row of fused step `step`; redo: the
    systems that must hand over to the dense solve, with their first rare step."""
    if "batch" in _cache:
        return _cache["batch"]
    pat, cand, mask = lu_cases.structure()
    rng = np.random.default_rng(2031)
    want = [(s, r) for s in lu_cases.FUSED for r in cand[s]]
    assert len(want) == 90
    got = {}
    for draw in range(20000):
        if len(got) == len(want):
            break
        A = _own_magnitudes(rng, mask)
        b = rng.standard_normal((NV, 2)).astype(np.float32)
        x, t = oracle.cgesv_gpu_trace(A, b)
        if lu_cases.rare_steps(t) or not lu_cases.entries_sparse(A) or not np.isfinite(x).all():
            continue
        # the rarest pair this draw gives that is still missing (one pair per system)
        new = [(s, int(t[s]["row"])) for s in lu_cases.FUSED if (s, int(t[s]["row"])) not in got]
        if new:
            assert all(r in cand[s] for s, r in new)
            got[max(new, key=lambda sr: (len(cand[sr[0]]), sr[0]))] = (A, b, x, t)
    assert len(got) == len(want), f"no draw made these the pivot row: {sorted(set(want) - set(got))}"
    As, bs, names, refs, traces, forced = [], [], [], [], [], {}
    for (s, r) in want:
        A, b, x, t = got[s, r]
        forced[s, r] = len(As)
        As.append(A); bs.append(b); refs.append(x); traces.append(t); names.append(f"row {r} pivots at step {s}")

    def plain():
        for draw in range(100):
            A = _own_magnitudes(rng, mask)
            b = rng.standard_normal((NV, 2)).astype(np.float32)
            x, t = oracle.cgesv_gpu_trace(A, b)
            if not lu_cases.rare_steps(t) and np.isfinite(x).all():
                return A, b
        raise AssertionError("no plain draw")

    redo = {}
    for step in (5, 25):
        for draw in range(100):
            A, b = plain()
            A[:, step] *= np.float32(2.0 ** -100)
            x, t = oracle.cgesv_gpu_trace(A, b)
            rare = lu_cases.rare_steps(t)
            if rare and rare[0] == (step, "range") and lu_cases.entries_sparse(A):
                break
        else:
            raise AssertionError(f"no draw gave a tiny pivot at step {step}")
        assert len(As) % 2 == 0
        redo[len(As)] = step
        As.append(A); bs.append(b); refs.append(x); traces.append(t); names.append(f"tiny pivot {step}")
        A, b = plain()
        x, t = oracle.cgesv_gpu_trace(A, b)
        As.append(A); bs.append(b); refs.append(x); traces.append(t); names.append(f"plain beside tiny pivot {step}")
    A, b = np.stack(As), np.stack(bs)
    assert len(A) <= 128 and len(A) % 2 == 0 and not (A[:, ~mask] != 0).any()
    _cache["batch"] = dict(A=A, b=b, names=names, ref=np.stack(refs), trace=traces, forced=forced, redo=redo)
    return _cache["batch"]
