"""GPU tests of the fused solve's compact row (hc_lu_struct.hpp LuRowForm): the
solve alone on it, and the gather that fills it in the tracker.

* the solve: tests/compact_cases.py, 94 systems in one launch through
  hc_cgesv_30x30_variant_batched with HC_LU_VARIANT_THROUGHPUT, whose hook loads
  the 16 positions from dense A as the tracker's gather would; value for value
  against oracle.cgesv_gpu_trace's solutions (conftest.same: NaN == NaN, +0 == -0);
* the gather: hc_trifocal_compact_rows_batched at 16 points (two workgroups:
  every path slot), on the problem's table and on the row swap (0, 9), byte for
  byte against the oracle's dH/dx at the mapped column, +0 where a row has no
  column at a level."""
import numpy as np
import pytest

import compact_cases
import eval_cases as EC
from checks import _none_differ
from conftest import same

pytestmark = pytest.mark.gpu


def test_forced_pivot_rows_and_redo_against_the_oracle(oracle):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_variant_batched
    B = compact_cases.batch(oracle)
    assert 2 <= len(B["A"]) <= 128 and len(B["redo"]) == 2
    x = cgesv_variant_batched("throughput", B["A"], B["b"])
    differ = ~same(x, B["ref"]).all(axis=(1, 2))
    for i in np.flatnonzero(differ)[:8]:
        print(f"{i} ({B['names'][i]}): positions {np.flatnonzero(~same(x[i], B['ref'][i]).all(axis=1)).tolist()}")
    _none_differ("solutions of the compact-row solve", differ, np.arange(len(x)))


@pytest.mark.parametrize("table", ["own", "swap_0_9"])
def test_the_gather_fills_the_compact_row(problem, oracle, samples100, table):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import compact_rows_batched
    dx, dt, U = EC.tables(problem)[table]
    pts = EC.path_points(problem, samples100, 16, seed=61)
    kind = (np.arange(16) % 3 == 0).astype(np.uint8)
    rows, rhs = compact_rows_batched(U, pts.x, pts.target, pts.diff, problem.start_params, pts.t, kind)
    _, HX, HT, H = EC.oracle_values(oracle, problem, dx, dt, pts)
    L = _abi.lib()
    col = np.array([[int(L.hc_lu_compact_column(r, p)) for p in range(_abi.LU_COMPACT_WIDTH)] for r in range(30)])
    assert rows.shape == (16, 30, _abi.LU_COMPACT_WIDTH, 2)
    want = np.zeros_like(rows)          # +0 where the row has no column
    for r in range(30):
        for p in range(_abi.LU_COMPACT_WIDTH):
            if col[r, p] >= 0:
                want[:, r, p] = HX[:, r, col[r, p]]
    differ = (rows.view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2, 3))
    _none_differ(f"compact rows, table {table}", differ, np.arange(16))
    want_rhs = np.where((kind == 0)[:, None, None], HT, H)
    _none_differ("right-hand sides", (rhs.view(np.uint32) != want_rhs.view(np.uint32)).any(axis=(1, 2)), np.arange(16))
