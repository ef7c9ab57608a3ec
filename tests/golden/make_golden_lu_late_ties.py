"""Generates tests/golden/lu_late_ties.npz with the C oracle on the CPU.

Systems on the tracker LU's compiled-in pattern whose exact pivot ties cannot be
built by isolating two rows (tests/lu_cases.py late_cases): they are found by
drawing from lu_cases.units_on_pattern (entries in {+-1, +-i}, the entries of
each column 0..17 times distinct powers of two) and reading the oracle's trace
(oracle.cgesv_gpu_trace).  Every kept system has no rare condition at the fused
steps 0..17, every pivot in the fast reciprocal range and no NaN, so every
variant of the sparse solve keeps it.  The file holds at most 32 of them:

  * ties at step 26, whose structural rows hold columns 24..26 only (two rows
    reduced to column 26 alone make the system singular);
  * a tie of three or more rows at each of the steps 18..23;
  * ties produced by fill-in: the winning row lacks the column structurally;
  * ties at steps 24, 25 and 27 as they come (none at step 28 in 400 000 draws).

  A (n, 30, 30, 2) float32, b (n, 30, 2) float32
  tie_steps (n, 30) int32: the oracle's count of equal maxima per step (1: no tie)

The test reads the file and never re-draws: numpy does not promise a stable
Generator stream.  The script asserts what tests/test_lu_cases_host.py relies on.

Run:  python tests/golden/make_golden_lu_late_ties.py      (under a minute)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import lu_cases as LC  # noqa: E402
from oracle import oracle as O  # noqa: E402

MAX_SYSTEMS = 32
STEP26_WANTED = 3


def main():
    _, _, mask = LC.structure()
    rng = np.random.default_rng(26)
    needs = {("tie", 26, k) for k in range(STEP26_WANTED)} | {("wide", s) for s in range(18, 24)} | \
            {("fill-in", s) for s in range(18, 24)} | {("tie", s, 0) for s in (24, 25, 27)}
    must = {("tie", 26, 0), ("fill-in",)} | {("wide", s) for s in range(18, 24)}
    kept, got, draws, clean = [], set(), 0, 0
    while (needs - got or len(kept) % 2) and draws < 100000 and len(kept) < MAX_SYSTEMS:
        draws += 1
        A = LC.units_on_pattern(rng, mask)
        b = rng.standard_normal((LC.NV, 2)).astype(np.float32)
        x, t = O.cgesv_gpu_trace(A, b)
        rare = LC.rare_steps(t)
        if any(kind != "tie" or step < 18 for step, kind in rare) or not np.isfinite(x).all():
            continue
        clean += 1
        has = set()
        for step, _ in rare:
            n26 = sum(1 for g in got if g[:2] == ("tie", 26))
            if step == 26 and n26 < STEP26_WANTED:
                has.add(("tie", 26, n26))
            if step in (24, 25, 27):
                has.add(("tie", step, 0))
            if step < 24 and t[step]["equal"] >= 3:
                has.add(("wide", step))
            if step < 24 and not mask[int(t[step]["row"]), step]:
                has.add(("fill-in", step))
        if has - got or (len(kept) % 2 and not needs - got and rare):   # (the last: an even count)
            got |= has
            if any(g[0] == "fill-in" for g in has):
                got.add(("fill-in",))
            kept.append((A, b, np.array(t["equal"], np.int32), sorted(has)))
            print(f"draw {draws}: system {len(kept) - 1}: {sorted(has)}")
    print(f"{draws} draws, {clean} clean, {len(kept)} kept; not found: {sorted(needs - got)}")
    assert must <= got, sorted(must - got)
    assert len(kept) <= MAX_SYSTEMS and len(kept) % 2 == 0
    np.savez_compressed(LC.GOLDEN, A=np.stack([k[0] for k in kept]), b=np.stack([k[1] for k in kept]),
                        tie_steps=np.stack([k[2] for k in kept]))
    print("wrote", LC.GOLDEN, os.path.getsize(LC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
