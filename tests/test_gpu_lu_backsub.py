"""GPU tests of the level-wise back substitution of the throughput tracker's LU
(hc_lu_levels.hpp lu_back_level): the solve alone, through both of its test
entries (hc_cgesv_30x30_struct_batched and hc_cgesv_30x30_variant_batched with
HC_LU_VARIANT_THROUGHPUT), against the oracle's LU, system by system, on the
systems of tests/backsub_cases.py -- right-hand sides that isolate each row's
propagation through its chain, and solutions that overflow in the back
substitution, which the solve hands to the dense one together with the plain
system in the other half of the wave -- and the throughput kernel against the
oracle's tracker.  tests/test_backsub_levels_host.py says on the CPU what each
system does.

Bar: identical values (conftest.same: NaN == NaN, +0 == -0)."""
import numpy as np
import pytest

import backsub_cases
from checks import SMALL_NEVER, assert_matches_oracle, launch_mode
from conftest import same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(problem, oracle, samples100):
    return backsub_cases.systems(problem, oracle, samples100)


def _solve(entry, A, b):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_struct_batched, cgesv_variant_batched
    return cgesv_struct_batched(A, b) if entry == "struct" else cgesv_variant_batched("throughput", A, b)


def _check(cases, entry, first, n):
    x = _solve(entry, cases["A"][first:first + n], cases["b"][first:first + n])
    for i in range(n):
        ok = same(x[i], cases["ref"][first + i])
        assert ok.all(), (f"system {first + i} ({cases['names'][first + i]}) of a batch of {n} at {first}: "
                          f"positions {np.flatnonzero(~ok.all(axis=1)).tolist()}")


@pytest.mark.parametrize("entry", ["struct", "variant"])
def test_one_wave_both_halves(cases, entry):
    """n = 2: every system beside its neighbour, the overflowing ones beside
    their plain partners (the wave-uniform `redo` re-solves both densely)."""
    for first in range(0, len(cases["A"]), 2):
        _check(cases, entry, first, 2)


@pytest.mark.parametrize("entry", ["struct", "variant"])
def test_a_lone_half(cases, entry):
    """n = 3: the third system alone in its wave, beside the zeros the component
    kernel fills the idle half with (that wave reports `redo`, as in
    test_gpu_lu_levels.py)."""
    for first in range(0, len(cases["A"]) - 2, 2):
        _check(cases, entry, first, 3)


@pytest.mark.parametrize("entry", ["struct", "variant"])
def test_mixed_batch(cases, entry):
    """64 systems in one launch: the overflow pairs, the Jacobian's right-hand
    sides and the first of the random matrix's."""
    assert len(cases["A"]) > 64 and max(cases["overflow"]) < 64
    _check(cases, entry, 0, 64)


@pytest.mark.parametrize("N", [2, 3])
def test_throughput_kernel_matches_oracle(problem, oracle, samples100, tracker, N):
    """The throughput kernel (never the latency-mode one) at 2 and 3 samples:
    tracks, flags and statistics against the oracle's tracker."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER):
        r = tracker.track(tgt[:N], dif[:N]).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index))
