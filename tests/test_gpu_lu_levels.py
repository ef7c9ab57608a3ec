"""GPU tests of the tracker LU's fused levels (hc_lu_levels.hpp lu_level): the
throughput tracker's solve alone (hc_cgesv_30x30_struct_batched) against the
oracle's LU, system by system, on inputs that reach every exit of a fused
level, and the throughput kernel against the oracle's tracker.

Bar: identical values (conftest.same: NaN == NaN, +0 == -0)."""
import numpy as np
import pytest

import lu_cases
from checks import SMALL_NEVER, assert_matches_oracle, launch_mode
from conftest import same
from lu_cases import FUSED, NV

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def structure():
    return lu_cases.structure()


@pytest.fixture(scope="module")
def batch(problem, oracle, samples100, structure):
    """The mixed batch (every case, fallback and common path in the same
    waves; lu_cases.levels_batch) and the oracle's solutions, computed once."""
    As, bs, what = lu_cases.levels_batch(problem, oracle, samples100)
    ref = np.stack([oracle.cgesv_gpu(As[i], bs[i]) for i in range(64)])
    return As, bs, ref, what


@pytest.mark.parametrize("n", [2, 3, 64])
def test_struct_solve_matches_oracle(batch, n):
    """n = 2: one wave, both halves; n = 3: a lone half; n = 64: the mixed batch.
    The component kernel fills the idle half of a lone half's wave with zeros,
    which no fused level accepts (every key is 0), so that wave reports `redo`
    and the lone system is solved densely: n = 3 checks the hand-over of a
    whole wave, and a lone half on the fused path is covered only by the
    tracker tests below, whose idle slots hold a parked path's system."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_struct_batched
    As, bs, ref, what = batch
    for first in ((0,) if n == 64 else range(0, 64 - n + 1, 7)):
        x = cgesv_struct_batched(As[first:first + n], bs[first:first + n])
        for i in range(n):
            assert same(x[i], ref[first + i]).all(), f"system {first + i} ({what[first + i]}) of a batch of {n}"


def test_struct_solve_covers_the_cases(batch, structure):
    _, _, _, what = batch
    kinds = {w.split()[0] for w in what}
    assert {"jacobian", "random", "tie", "zero", "tiny", "NaN", "inf", "entry"} <= kinds
    # per fused step: a tie inside a triple and, for a 6-row chain, one between its triples
    _, cand, _ = structure
    for step in FUSED:
        pairs = [tuple(int(v) for v in w.split()[2:]) for w in what if w.startswith(f"tie {step} ") and len(w.split()) == 4]
        assert any(a // 3 == b // 3 for a, b in pairs), f"no tie inside a triple at step {step}"
        if len(cand[step]) == 6:
            assert any(a // 3 != b // 3 for a, b in pairs), f"no tie between the triples at step {step}"


def test_entry_outside_the_structure_is_refused(batch, structure):
    import torch
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    _, _, mask = structure
    As, bs, _, _ = batch
    A = As[:4].copy()
    r, c = np.argwhere(~mask)[17]
    A[2, r, c, 1] = 1e-30
    dev = torch.device("cuda:0")
    At, bt = torch.from_numpy(A).to(dev), torch.from_numpy(bs[:4].copy()).to(dev)
    xt = torch.full((4, NV, 2), 7.0, dtype=torch.float32, device=dev)
    st = _abi.lib().hc_cgesv_30x30_struct_batched(4, _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
                                                  _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert st == 1, "HC_ERROR_INVALID_VALUE"
    assert (xt.cpu().numpy() == 7.0).all(), "x untouched"


@pytest.mark.parametrize("N", [2, 3])
def test_throughput_kernel_matches_oracle(problem, oracle, samples100, tracker, N):
    """The throughput kernel (never the latency-mode one) at 2 and 3 samples:
    tracks, flags and statistics against the oracle's tracker."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER):
        r = tracker.track(tgt[:N], dif[:N]).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index))
