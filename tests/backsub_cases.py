"""Systems for the tests of the level-wise back substitution of the throughput
tracker's LU (hc_lu_levels.hpp lu_back_level): tests/test_backsub_levels_host.py
says on the oracle alone what each of them does, tests/test_gpu_lu_backsub.py
solves them on the device.

* right-hand sides that isolate the propagation: on one tracker Jacobian and
  one random matrix on the pattern (both from lu_cases.levels_batch), the 30
  unit vectors e_r, a zero vector and a vector of -0 entries;
* back-substitution overflows: x becomes inf first (in the substitution's
  order, from position 29 down) at a chosen position P, with every pivot of the
  forward elimination in the fast reciprocal range.  Built with powers of two
  only: column P of a random matrix on the pattern times 2^-64 -- whichever row
  becomes the pivot row of step P, its pivot is 2^-64 times what it was, every
  other pivot, every multiplier and every pivot choice is unchanged, since the
  scaling is exact -- and b times 2^90, so that x_J stays near 2^90 above P and
  x_P is near 2^154.  Each stands at an even index beside a plain system, its
  partner in the wave.
"""
import numpy as np

import lu_cases
from lu_cases import NV

OVERFLOW_AT = (2, 3, 7, 14, 17, 18, 29)   # a fused position of each level 0, 1, 2, 3, 3; two sequential ones
COL_SCALE, RHS_SCALE = np.float32(2.0 ** -64), np.float32(2.0 ** 90)

_cache = {}


def systems(problem, oracle, samples100):
    """dict(A, b, names, ref, trace, overflow): the overflow pairs first (2k the
    overflowing system at OVERFLOW_AT[k], 2k + 1 its plain partner), then the 32
    right-hand sides on the Jacobian, then the 32 on the random matrix; the
    oracle's solutions and traces, computed once."""
    if "s" in _cache:
        return _cache["s"]
    _, _, mask = lu_cases.structure()
    lA, lb, what = lu_cases.levels_batch(problem, oracle, samples100)
    rng = np.random.default_rng(2121)
    As, bs, names = [], [], []

    def add(A, b, name):
        As.append(np.asarray(A, np.float32).copy()); bs.append(np.asarray(b, np.float32).copy()); names.append(name)

    for P in OVERFLOW_AT:
        A = rng.standard_normal((NV, NV, 2)).astype(np.float32) * mask[:, :, None]
        b = rng.standard_normal((NV, 2)).astype(np.float32)
        A[:, P] *= COL_SCALE
        add(A, b * RHS_SCALE, f"overflow {P}")
        add(rng.standard_normal((NV, NV, 2)).astype(np.float32) * mask[:, :, None],
            rng.standard_normal((NV, 2)).astype(np.float32), f"plain beside overflow {P}")
    for kind in ("jacobian", "random"):
        A = lA[what.index(kind)]
        for r in range(NV):
            e = np.zeros((NV, 2), np.float32)
            e[r, 0] = 1.0
            add(A, e, f"{kind} e_{r}")
        add(A, np.zeros((NV, 2), np.float32), f"{kind} zero rhs")
        add(A, np.full((NV, 2), -0.0, np.float32), f"{kind} -0 rhs")
    A, b = np.stack(As), np.stack(bs)
    sols = [oracle.cgesv_gpu_trace(A[i], b[i]) for i in range(len(A))]
    _cache["s"] = dict(A=A, b=b, names=names, ref=np.stack([s[0] for s in sols]), trace=[s[1] for s in sols],
                       overflow={2 * k: P for k, P in enumerate(OVERFLOW_AT)})
    return _cache["s"]
