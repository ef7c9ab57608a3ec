"""The throughput tracking kernel's slot-absolute address tables (hc_eval.hpp
AbsTables, built by k_prep_tables beside the packed tables) and its
finiteness check on the dH/dx entries (hc_lu.hpp ENTCHK).

The tables are indexed by the path slot of the workgroup (8 variants) and the
lane, live in the workspace under the packed tables' hash and are read by
k_track<false, 5, true, false, *> only; every other kernel keeps the packed
tables.  So the tests here run every slot variant, rebuild the tables under
one workspace, mix the two kinds of kernel on one workspace and drive the
entry-level check into the dense re-solve.  The bar is tests/checks.py's.
"""
import dataclasses

import numpy as np
import pytest

from checks import (KERNEL_BY_SIZE, SMALL_NEVER, assert_matches_golden, assert_matches_oracle, golden, launch_mode,
                    scaled_samples)
from eval_cases import row_permuted as _row_permuted

pytestmark = pytest.mark.gpu

N = 2
SWAP = (0, 9)   # a row order outside the specialised LU's structure (the structure-agnostic twin tracks it)


@pytest.fixture(scope="module")
def permuted_index(problem):
    perm = np.arange(30)
    perm[SWAP[0]], perm[SWAP[1]] = SWAP[1], SWAP[0]
    _, _, U = _row_permuted(problem, perm)
    U.setflags(write=False)
    return U


@pytest.fixture(scope="module")
def ref_plain(problem, oracle, samples100):
    tgt, dif, _ = samples100
    return oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N], problem.unified_index)


@pytest.fixture(scope="module")
def ref_permuted(problem, oracle, samples100, permuted_index):
    tgt, dif, _ = samples100
    return oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N], permuted_index)


def _own_tracker(problem, ransac0):
    """A tracker with a workspace of its own (the session's is shared)."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    tr = DeviceTracker(dataclasses.replace(problem), torch.device("cuda:0"))
    tr.set_ransac_data(ransac0)
    return tr


def test_every_slot_variant_serves_a_path(samples100, tracker):
    """40 samples = 12 480 paths on 10 240 path slots: each of the 8 slot
    variants of every workgroup dequeues at least one path.  Against rows
    0..12 479 of the committed golden run."""
    tgt, dif, _ = samples100
    n = 40
    r = tracker.track(tgt[:n], dif[:n]).host()
    assert_matches_golden(r, golden("gpuhc_N100_seed0"), rows=slice(0, 312 * n))


def test_one_workspace_changing_tables(problem, ransac0, samples100, permuted_index, ref_plain, ref_permuted):
    """A rebuild of the packed tables rebuilds the address tables: the
    row-permuted table, the problem's own, and the permuted one again through
    one workspace, the throughput kernel forced, each against the oracle on
    the same table."""
    import torch
    tgt, dif, _ = samples100
    tr = _own_tracker(problem, ransac0)
    own = tr.unified
    perm = torch.from_numpy(np.array(permuted_index)).to(tr.device)
    ws = None   # (the first sliced launch of a size grows the tracker's workspace)
    for U, ref in ((perm, ref_permuted), (own, ref_plain), (perm, ref_permuted)):
        tr.unified = U
        with launch_mode(tr.L, small=SMALL_NEVER):
            r = tr.track(tgt[:N], dif[:N]).host()
        ws = tr.workspace.data_ptr() if ws is None else ws
        assert tr.workspace.data_ptr() == ws, "the launches must share one workspace"
        assert_matches_oracle(r, ref)


def test_one_workspace_small_kernel_first(problem, ransac0, samples100, ref_plain):
    """k_track_small (packed tables) builds the workspace's tables, the
    throughput kernel then finds its address tables there."""
    tgt, dif, _ = samples100
    tr = _own_tracker(problem, ransac0)
    ws = None
    for mode in (KERNEL_BY_SIZE, SMALL_NEVER):
        with launch_mode(tr.L, small=mode):
            r = tr.track(tgt[:N], dif[:N]).host()
        ws = tr.workspace.data_ptr() if ws is None else ws
        assert tr.workspace.data_ptr() == ws, "the launches must share one workspace"
        assert_matches_oracle(r, ref_plain)


def test_entry_check_reaches_the_dense_resolve(problem, oracle, samples100, tracker):
    """The finiteness check on the stored dH/dx entries sends a system with an
    entry past 2^64 to the dense re-solve: config 2's sample 0 beside its target
    parameters scaled by 2^40 and 2^70 (waves pair a scaled sample's path with a
    healthy one), the throughput kernel forced, against the oracle."""
    tgt, _, _ = samples100
    T, D = scaled_samples(problem, tgt[0], order=(0, 40, 70))
    with launch_mode(tracker.L, small=SMALL_NEVER):
        r = tracker.track(T, D).host()
    ref = _, conv, inf, _ = oracle.gpuhc_track(problem.start_sols, problem.start_params, T, D, problem.unified_index)
    assert_matches_oracle(r, ref)
    assert inf[312:].sum() > 600 and conv[:312].sum() > 0   # the scaled samples diverge, sample 0 converges
