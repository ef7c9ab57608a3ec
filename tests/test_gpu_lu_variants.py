"""GPU tests of every instantiation of the tracker's sparse solve alone
(hc_cgesv_30x30_variant_batched, include/lu/hc_lu_testing.h: lu_solve<false,
LAT, STRUCT, ENTCHK, FUSE> with the template arguments hc_lu.hpp's lu_mode gives
the kernels that run it) against the oracle's LU, system by system, on inputs built to leave the
common path at every pivot step (tests/lu_cases.py; what they cover is
accounted on the CPU, tests/test_lu_cases_host.py).  No tracker launch.

Bar: identical values (conftest.same: NaN == NaN, +0 == -0)."""
import numpy as np
import pytest

import lu_cases
from conftest import same
from lu_cases import NV

pytestmark = pytest.mark.gpu

VARIANTS = ("throughput", "throughput_twin", "abort", "abort_twin", "small", "small_twin", "archived",
            "archived_twin")
STRUCT = VARIANTS[0::2]    # the problem's structure: row patterns from LU_STRUCT_PAT
TWINS = VARIANTS[1::2]     # structure-agnostic: a row's pattern is its non-zero entries
# the rows of A and b in another order: what a table with its equations permuted
# feeds the structure-agnostic solve
PERM = np.random.RandomState(7).permutation(NV)


@pytest.fixture(scope="module")
def full(problem, oracle, samples100):
    return lu_cases.full_batch(problem, oracle, samples100)


@pytest.fixture(scope="module")
def permuted(full, oracle):
    A = np.ascontiguousarray(full["A"][:, PERM])
    b = np.ascontiguousarray(full["b"][:, PERM])
    return A, b, np.stack([oracle.cgesv_gpu(A[i], b[i]) for i in range(len(A))])


@pytest.fixture(scope="module")
def dense(problem, oracle, samples100):
    return lu_cases.dense_batch(problem, oracle, samples100)


def _solve(variant, A, b):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_variant_batched
    return cgesv_variant_batched(variant, A, b)


def _assert_identical(x, ref, names, what):
    wrong = [f"{i} ({names[i]})" for i in range(len(ref)) if not same(x[i], ref[i]).all()]
    assert not wrong, f"{what}: {len(wrong)} of {len(ref)} systems differ from the oracle: " + ", ".join(wrong[:12])


def test_variant_names_are_the_binding_s():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    assert VARIANTS == _abi.LU_VARIANTS


@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_matches_oracle(full, variant):
    """The whole batch in one launch: the 64 systems of the fused steps, the
    late-step cases and the fixture, a few waves; every x identical to the
    oracle's."""
    x = _solve(variant, full["A"], full["b"])
    _assert_identical(x, full["ref"], full["names"], variant)


@pytest.mark.parametrize("variant", TWINS)
def test_twin_matches_oracle_on_permuted_rows(full, permuted, variant):
    A, b, ref = permuted
    _assert_identical(_solve(variant, A, b), ref, full["names"], f"{variant}, rows permuted")


@pytest.mark.parametrize("variant", TWINS)
def test_twin_matches_oracle_off_the_pattern(dense, variant):
    """8 dense random systems, the ties of test_cgesv_edge_cases and the scales
    of test_cgesv_extreme_scales (tests/test_gpu_parity.py: the same builders)."""
    A, b, ref = dense
    names = ["dense random"] * 8 + [f"edge case {i}" for i in range(64)] + \
            [f"extreme scale {i}" for i in range(len(A) - 72)]
    _assert_identical(_solve(variant, A, b), ref, names, f"{variant}, off the pattern")


@pytest.mark.parametrize("variant", STRUCT)
def test_entry_outside_the_structure_is_refused(full, variant):
    import torch
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    _, _, mask = lu_cases.structure()
    A = full["A"][:4].copy()
    r, c = np.argwhere(~mask)[17]
    A[2, r, c, 1] = 1e-30
    dev = torch.device("cuda:0")
    At, bt = torch.from_numpy(A).to(dev), torch.from_numpy(full["b"][:4].copy()).to(dev)
    xt = torch.full((4, NV, 2), 7.0, dtype=torch.float32, device=dev)
    st = _abi.lib().hc_cgesv_30x30_variant_batched(VARIANTS.index(variant), 4, _abi.ptr(At), _abi.ptr(bt),
                                                   _abi.ptr(xt), _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert st == 1, "HC_ERROR_INVALID_VALUE"
    assert (xt.cpu().numpy() == 7.0).all(), "x untouched"


@pytest.mark.parametrize("variant", TWINS)
def test_twin_accepts_an_entry_outside_the_structure(full, oracle, variant):
    _, _, mask = lu_cases.structure()
    A, b = full["A"][:4].copy(), full["b"][:4]
    r, c = np.argwhere(~mask)[17]
    A[2, r, c, 1] = 1e-30
    x = _solve(variant, A, b)
    for i in range(4):
        assert same(x[i], oracle.cgesv_gpu(A[i], b[i])).all(), f"{variant}: system {i}"


@pytest.mark.parametrize("variant", [-1, 8, 1000])
def test_unknown_variant_is_refused(full, variant):
    import torch
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_variant_batched
    dev = torch.device("cuda:0")
    At, bt = torch.from_numpy(full["A"][:2].copy()).to(dev), torch.from_numpy(full["b"][:2].copy()).to(dev)
    xt = torch.full((2, NV, 2), 7.0, dtype=torch.float32, device=dev)
    st = _abi.lib().hc_cgesv_30x30_variant_batched(variant, 2, _abi.ptr(At), _abi.ptr(bt), _abi.ptr(xt),
                                                   _abi.ptr(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert st == 1, "HC_ERROR_INVALID_VALUE"
    assert (xt.cpu().numpy() == 7.0).all(), "x untouched"
    with pytest.raises(_abi.HCError):
        cgesv_variant_batched(variant, full["A"][:2], full["b"][:2])
