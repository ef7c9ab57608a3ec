"""GPU tests of the bookkeeping of the throughput tracker's fused LU levels
(hc_lu_levels.hpp: the per-row records, the labels' relabel through the half's
buffer, the owners of the back substitution): the solve alone, through
hc_cgesv_30x30_variant_batched with HC_LU_VARIANT_THROUGHPUT, value for value
against oracle.cgesv_gpu_trace's solutions.

* the existing batches unchanged: tests/lu_cases.py (122 systems: every exit of
  every pivot step) and tests/backsub_cases.py (78 systems: right-hand sides
  that isolate each row's propagation, overflows in the back substitution);
* tests/label_cases.py: systems whose row labels of steps 0..17 decide an exact
  tie at step 18, 19, 21 or 22 -- the overlap inside a level, rows relabelled
  once and twice, a label handed on by a late pivot row -- each beside a plain
  partner in its wave.  tests/test_label_cases_host.py says on the CPU what each
  does and that a wrong label gives another pivot row.

Bar: identical values (conftest.same: NaN == NaN, +0 == -0)."""
import numpy as np
import pytest

import backsub_cases
import label_cases
import lu_cases
from conftest import same

pytestmark = pytest.mark.gpu


def _solve(A, b):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_variant_batched
    return cgesv_variant_batched("throughput", A, b)


def _assert_identical(x, ref, names, what):
    wrong = [f"{i} ({names[i]}): positions {np.flatnonzero(~same(x[i], ref[i]).all(axis=1)).tolist()}"
             for i in range(len(ref)) if not same(x[i], ref[i]).all()]
    assert not wrong, f"{what}: {len(wrong)} of {len(ref)} systems differ from the oracle: " + "; ".join(wrong[:8])


def test_lu_cases_batch(problem, oracle, samples100):
    full = lu_cases.full_batch(problem, oracle, samples100)
    assert len(full["A"]) == 122
    _assert_identical(_solve(full["A"], full["b"]), full["ref"], full["names"], "lu_cases")


def test_backsub_cases_batch(problem, oracle, samples100):
    cases = backsub_cases.systems(problem, oracle, samples100)
    assert len(cases["A"]) == 78
    _assert_identical(_solve(cases["A"], cases["b"]), cases["ref"], cases["names"], "backsub_cases")


def test_label_cases_batch(oracle):
    """One launch, every system beside its partner; then each pair alone in a
    launch of one wave."""
    cases = label_cases.systems(oracle)
    assert 2 <= len(cases["A"]) <= 128
    _assert_identical(_solve(cases["A"], cases["b"]), cases["ref"], cases["names"], "label_cases")
    for first in range(0, len(cases["A"]), 2):
        x = _solve(cases["A"][first:first + 2], cases["b"][first:first + 2])
        _assert_identical(x, cases["ref"][first:first + 2], cases["names"][first:first + 2], f"label_cases pair at {first}")
