"""The P2C mode on the GPU against its CPU restatement (tests/p2c_ref).  The bar
is the project's (tests/checks.py): identical values, NaN == NaN, +0 == -0."""
import numpy as np
import pytest

import p2c_common as pc
from checks import assert_matches_golden, assert_matches_oracle, golden
from conftest import same
from p2c_common import p2c_ref

pytestmark = pytest.mark.gpu


def _tracker(problem, **kw):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    return DeviceTracker(problem, "cuda:0", **kw)


# ---- 8. the evaluation entry --------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 129])
def test_p2c_eval_entry_matches_the_restatement(problem, tracker, n):
    """n = 1, 3: an unpaired half-wave; 129: more than one workgroup (8 points
    each) and an unpaired last half.  Points: perturbed start solutions, the
    blocks of two samples alternately, t = 0 and t = 1 among them."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    rng = np.random.default_rng(2)
    hx, ht = pc.fixture_tables()
    chx, cht = pc.blocks(2)
    X = pc.perturbed_start_sols(rng)[:n]
    x = np.stack([X.real, X.imag], -1).astype(np.float32)
    t = rng.uniform(0.0, 1.0, n).astype(np.float32)
    t[0] = 0.0
    t[-1] = 1.0 if n > 1 else 0.0
    if n > 2:
        t[1] = 1.0
    smp = np.arange(n) % 2
    got = p2c.eval_batched(hx, ht, x, chx[smp], cht[smp], t)
    ref = p2c_ref.eval_batched(hx, ht, x, chx[smp], cht[smp], t)
    for name, g, r in zip(("dH/dx", "dH/dt", "H"), got, ref):
        bad = np.nonzero(~same(g, r).reshape(n, -1).all(1))[0]
        assert len(bad) == 0, f"{name}: points {bad[:5].tolist()} of {n} differ"


def test_p2c_eval_entry_at_t_one_alone(problem, tracker):
    """(n = 1 above evaluates at t = 0.)"""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    hx, ht = pc.fixture_tables()
    chx, cht = pc.blocks(2)
    x = problem.start_sols[5:6] * np.float32(1.01)
    x[:, 30] = (1.0, 0.0)
    t = np.ones(1, np.float32)
    got = p2c.eval_batched(hx, ht, x, chx[1:2], cht[1:2], t)
    ref = p2c_ref.eval_batched(hx, ht, x, chx[1:2], cht[1:2], t)
    for g, r in zip(got, ref):
        assert same(g, r).all()


# ---- 9. the tracker --------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2])
def test_track_p2c_matches_the_restatement(problem, tracker, n):
    """The reference's fixture tables.  N = 2: the per-sample strides of the
    coefficient blocks (114 and 76 complex values)."""
    tgt, dif = pc.samples(n)
    r = tracker.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host()
    assert_matches_oracle(r, pc.ref_track(n))
    assert r["stats"]["inliers21"].max() == 0 and r["stats"]["inliers31"].max() == 0


@pytest.mark.parametrize("kw", [dict(max_steps=5), dict(max_corrections=1)], ids=["max_steps5", "max_corrections1"])
def test_track_p2c_limits_match_the_restatement(problem, kw):
    tgt, dif = pc.samples(1)
    t = _tracker(problem, **kw)
    r = t.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host()
    ref = pc.ref_track(1, "fixture", kw.get("max_steps", 80), kw.get("max_corrections", 3))
    assert_matches_oracle(r, ref)
    if "max_steps" in kw:
        assert r["stats"]["steps"].max() == 6 and r["converge"].sum() == 0


def test_track_p2c_default_tables_from_ph(problem, tracker):
    """tables=None: p2c.tables_from_ph (PH term order, sorted pair numbering)."""
    tgt, dif = pc.samples(1)
    r = tracker.track_p2c(tgt, dif).host()
    assert_matches_oracle(r, pc.ref_track(1, "ph"))


def test_track_p2c_row_permuted_table_takes_the_structure_agnostic_twin(problem):
    """Rows 0 and 9 of both tables swapped: an equivalent system whose dH/dx
    structure lies outside the specialised LU's, so k_track_p2c<false> tracks it."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    hx, ht = pc.fixture_tables()
    perm = np.arange(30)
    perm[0], perm[9] = 9, 0
    hx_p = np.ascontiguousarray(hx.reshape(30, -1)[perm]).reshape(-1)
    ht_p = np.ascontiguousarray(ht.reshape(30, -1)[perm]).reshape(-1)
    coef = hx_p.reshape(30, 30, 8, 4)[..., 0]
    L = _abi.lib()
    pat = [sum(1 << c for c in range(30) if (coef[r, c] != 0).any()) for r in range(30)]
    assert [r for r in range(30) if pat[r] & ~int(L.hc_lu_struct_pattern(r))], "the swap stays within the LU's structure"
    tgt, dif = pc.samples(1)
    t = _tracker(problem)
    r = t.track_p2c(tgt, dif, tables=(hx_p, ht_p), coeff_map=pc.fixture_map()).host()
    chx, cht = pc.blocks(1)
    assert_matches_oracle(r, p2c_ref.track(problem.start_sols, hx_p, ht_p, chx, cht))


# ---- 10. one workspace, both table formats ------------------------------------------

def test_workspace_rebuilds_its_tables_when_the_format_changes(problem, oracle):
    """track -> track_p2c -> track on one workspace: each equal to its own reference."""
    tgt, dif = pc.samples(1)
    t = _tracker(problem)
    ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt, dif, problem.unified_index)
    assert_matches_oracle(t.track(tgt, dif).host(), ref)
    ws = t.workspace.data_ptr()
    assert_matches_oracle(t.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host(),
                          pc.ref_track(1))
    assert_matches_oracle(t.track(tgt, dif).host(), ref)
    assert_matches_oracle(t.track_p2c(tgt, dif).host(), pc.ref_track(1, "ph"))       # the other P2C tables
    assert_matches_oracle(t.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host(),
                          pc.ref_track(1))
    assert t.workspace.data_ptr() == ws


# ---- 11. config 2 ----------------------------------------------------------------------

def test_track_p2c_n100_matches_the_golden_run(problem, tracker):
    tgt, dif = pc.samples(100)
    r = tracker.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host()
    g = golden("gpuhc_p2c_N100_seed0")
    assert_matches_golden(r, g)
    from trifocal_pose_estimation_using_improved_gpuhc_amd import count_solutions
    assert list(count_solutions(r["tracks"], r["converge"], r["infinity"])) == g["counts"].tolist()


# ---- 12. the reference-named launcher --------------------------------------------------------

def test_shim_p2c_launcher_equals_track_p2c(problem, tracker):
    """kernel_GPUHC_trifocal_2op1p_30x30_P2C of the shim with the archived
    argument list (per-track pointer arrays, bool flags) at N = 2 against
    track_p2c: the same flags and tracks (the launchers report no counts)."""
    import ctypes as C
    import os

    import torch

    from checks import ROOT, assert_same_run
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    shim = os.path.join(ROOT, "integration", "build", "libhc_shim_test.so")
    assert os.path.exists(shim), "integration shim not built (__graft_entry__.build())"
    _abi.lib()
    L = C.CDLL(shim)
    L.shim_queue_create.restype = C.c_void_p
    L.shim_queue_create.argtypes = [C.c_void_p]
    L.shim_queue_destroy.argtypes = [C.c_void_p]
    L.hc_trifocal_shim_status.argtypes = [C.c_void_p]
    L.shim_p2c.restype = C.c_double
    N, dev, st, p = 2, tracker.device, tracker.settings, _abi.ptr
    tgt, dif = pc.samples(N)
    ref = tracker.track_p2c(tgt, dif, tables=pc.fixture_tables(), coeff_map=pc.fixture_map()).host()
    hx, ht = tracker.p2c_tables(pc.fixture_tables())
    chx, cht = (torch.from_numpy(np.array(b)).to(dev) for b in pc.blocks(N))
    ss = tracker.start_sols
    tracks = ss.unsqueeze(0).expand(N, -1, -1, -1).reshape(N * 312, 31, 2).contiguous()
    ssa = torch.tensor([ss.data_ptr() + k * 31 * 8 for k in range(312)], dtype=torch.int64, device=dev)
    tra = torch.tensor([tracks.data_ptr() + b * 31 * 8 for b in range(312 * N)], dtype=torch.int64, device=dev)
    conv = torch.zeros(312 * N, dtype=torch.bool, device=dev)
    inf = torch.zeros(312 * N, dtype=torch.bool, device=dev)
    q = L.shim_queue_create(p(torch.cuda.current_stream(dev)))
    try:
        rv = L.shim_p2c(C.c_void_p(q), C.c_int(N), C.c_int(st.max_steps), C.c_int(st.max_corrections),
                        C.c_int(st.delta_t_inc_steps), p(ssa), p(tra), p(hx), p(ht), p(chx), p(cht), p(conv), p(inf))
        torch.cuda.synchronize(dev)
        assert rv == 0.0 and int(L.hc_trifocal_shim_status(C.c_void_p(q))) == 0
    finally:
        L.shim_queue_destroy(C.c_void_p(q))
    got = dict(tracks=tracks.cpu().numpy(), converge=conv.cpu().numpy().astype(np.uint8),
               infinity=inf.cpu().numpy().astype(np.uint8))
    assert_same_run(got, ref["tracks"], ref["converge"], ref["infinity"], None, None)
    assert got["converge"].sum() > 0


# ---- argument checks of the Python driver ---------------------------------------------------

def test_launch_p2c_rejects_misshapen_buffers(problem, tracker):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    chx, cht = (torch.from_numpy(np.array(b)).to(tracker.device) for b in pc.blocks(1))
    tables = tracker.p2c_tables(pc.fixture_tables())
    r = tracker.allocate(1)
    with pytest.raises(_abi.HCError):
        tracker.launch_p2c((tables[0][:-1], tables[1]), chx, cht, r)
    with pytest.raises(_abi.HCError):
        tracker.launch_p2c(tables, chx[:, :37], cht, r)
    with pytest.raises(_abi.HCError):
        tracker.launch_p2c(tables, chx, cht, r, num_samples=2)
