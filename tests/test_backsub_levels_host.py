"""CPU tests of the level-wise back substitution of the throughput tracker's LU
(hc_lu_levels.hpp lu_back_level; the static_asserts lu_back_chains_nested and
lu_back_order_kept of hc_lu_struct.hpp).

The structural claim, restated from the library's row patterns alone: the row
pivoted at a fused step I can hold a non-zero in a column J, I < J <= 17, only
where every candidate row of I is a candidate row of J and J lies on a higher
level; and along the fused steps a row is a candidate of, the column rises with
the level.  So each lane updates its right-hand side once per level, with the
x of its own chain's column, in the reference's descending order.

And, on the oracle alone, that the systems of tests/test_gpu_lu_backsub.py
(tests/backsub_cases.py) do what they are built for."""
import numpy as np
import pytest

import backsub_cases
import lu_cases
from lu_cases import FUSED, NV


@pytest.fixture(scope="module")
def lib():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def bound(lib):
    """(cand, s) per step, derived from hc_lu_struct_pattern: the rows that may
    hold column i at step i and the columns above i their union may hold."""
    cur = [int(lib.hc_lu_struct_pattern(r)) for r in range(NV)]
    cand, s = [], []
    for i in range(NV):
        rows = [r for r in range(NV) if (cur[r] >> i) & 1]
        above = (0xFFFFFFFF << (i + 1)) & ((1 << NV) - 1)
        u = 0
        for r in rows:
            u |= cur[r]
        for r in rows:
            cur[r] |= u & above
        cand.append(sum(1 << r for r in rows))
        s.append(u & above)
    return cand, s


def test_a_fused_pivot_row_holds_fused_columns_of_its_ancestors_only(lib, bound):
    cand, s = bound
    seen = 0
    for i in FUSED:
        assert int(lib.hc_lu_candidates(i)) == cand[i], i
        for j in range(i + 1, 18):
            if (s[i] >> j) & 1:
                seen += 1
                assert cand[i] & ~cand[j] == 0, (i, j)
                assert int(lib.hc_lu_step_level(i)) < int(lib.hc_lu_step_level(j)), (i, j)
    # 0-3-6 and 1-4-7: 3 pairs each; 8 | 9-12-13-14 and 10 | 11-15-16-17: 7 each (rows
    # 18..20 reach column 14, and rows 24..26 column 13, only through step 12's bound)
    assert seen == 20


def test_a_rows_ancestors_rise_in_column_with_the_level(lib):
    chains = set()
    for r in range(NV):
        steps = [i for i in FUSED if (int(lib.hc_lu_candidates(i)) >> r) & 1]
        levels = [int(lib.hc_lu_step_level(i)) for i in steps]
        assert len(set(levels)) == len(levels), f"row {r}: two members on one level"
        by_level = [i for _, i in sorted(zip(levels, steps))]
        assert by_level == sorted(by_level), f"row {r}: {by_level}"
        chains.add(tuple(by_level))
    # the families of DESIGN.md §3.3
    assert chains == {(2,), (5,), (0, 3, 6), (1, 4, 7), (8, 12, 13, 14), (9, 12, 13, 14), (10, 15, 16, 17),
                      (11, 15, 16, 17)}


@pytest.fixture(scope="module")
def cases(problem, oracle, samples100):
    return backsub_cases.systems(problem, oracle, samples100)


def _sparse_throughout(A, trace):
    return all(lu_cases.fast_bits(trace[i]["key_bits"]) for i in range(NV)) and not lu_cases.raises_redo(A, trace, True)


def test_overflow_cases_overflow_in_the_back_substitution_only(cases):
    _, _, mask = lu_cases.structure()
    assert sorted(cases["overflow"].values()) == [2, 3, 7, 14, 17, 18, 29]
    for i, P in cases["overflow"].items():
        A, t, x, name = cases["A"][i], cases["trace"][i], cases["ref"][i], cases["names"][i]
        assert i % 2 == 0 and not (A[~mask] != 0).any(), name
        # every forward pivot in the fast range, nothing that raises `redo` in the elimination
        assert _sparse_throughout(A, t), name
        # x is finite above P, not finite at P, and the reference spreads that over every position below
        fin = np.isfinite(x).all(axis=1)
        assert fin[P + 1:].all() and not fin[P] and not fin[:P].any(), (name, fin)
        # the wave partner: plain, sparse, finite
        assert _sparse_throughout(cases["A"][i + 1], cases["trace"][i + 1]), cases["names"][i + 1]
        assert np.isfinite(cases["ref"][i + 1]).all(), cases["names"][i + 1]


def test_isolating_right_hand_sides_run_the_sparse_path(cases):
    n0 = 2 * len(cases["overflow"])
    assert len(cases["A"]) == n0 + 64
    for i in range(n0, n0 + 64):
        assert _sparse_throughout(cases["A"][i], cases["trace"][i]), cases["names"][i]
        assert np.isfinite(cases["ref"][i]).all(), cases["names"][i]
    for k, kind in enumerate(("jacobian", "random")):
        base = n0 + 32 * k
        for r in range(NV):
            assert cases["names"][base + r] == f"{kind} e_{r}"
            assert (cases["b"][base + r] != 0).sum() == 1 and cases["b"][base + r][r, 0] == 1.0
            assert (cases["ref"][base + r] != 0).any()
        assert (cases["ref"][base + 30] == 0).all() and (cases["ref"][base + 31] == 0).all()
        assert np.signbit(cases["b"][base + 31]).all() and not np.signbit(cases["b"][base + 30]).any()
