"""GPU parity tests: the HIP kernels (through the C-ABI) against the C oracle.

Bar: identical values -- the kernel and the oracle implement the same
op-level spec, so every float must match exactly, treating +0 == -0 and
NaN == NaN; converged / infinity flags and step / correction counts identical.
"""
import numpy as np
import pytest

from checks import (KERNEL_BY_SIZE, SMALL_ALWAYS, SMALL_NEVER, assert_bit_identical, assert_matches_golden,
                    assert_matches_oracle, assert_untouched, found_ids, golden, golden_passing, launch_mode,
                    ring_counters, run_cli, scaled_samples, tracked)
from conftest import same
from eval_cases import row_permuted as _row_permuted
from lu_cases import edge_case_systems, extreme_scale_systems
from lu_cases import jacobians_from_path as _jacobians_from_path

pytestmark = pytest.mark.gpu


def test_eval_matches_oracle(problem, oracle, samples100):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_batched
    tgt, dif, _ = samples100
    X, P, D = _jacobians_from_path(problem, oracle, tgt, dif, n=256)
    HX, HT, H = eval_batched(problem.unified_index, X, P, D)
    for i in range(X.shape[0]):
        A = oracle.eval_hx(problem.dHdx_index, X[i], P[i])
        assert same(HX[i], A).all(), f"dH/dx mismatch at point {i}"
        assert same(HT[i], oracle.eval_ht(problem.dHdt_index, X[i], P[i], D[i])).all(), f"dH/dt mismatch {i}"
        assert same(H[i], oracle.eval_h(problem.dHdt_index, X[i], P[i])).all(), f"H mismatch {i}"


def test_eval_golden_kat(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_batched
    g = golden("kat_eval")
    HX, HT, H = eval_batched(problem.unified_index, g["x"][None], g["p"][None], g["d"][None])
    assert same(HX[0], g["Hx"]).all() and same(HT[0], g["Ht"]).all() and same(H[0], g["H"]).all()


def test_cgesv_matches_oracle_on_jacobians(problem, oracle, samples100):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_batched
    tgt, dif, _ = samples100
    X, P, D = _jacobians_from_path(problem, oracle, tgt, dif, n=256, seed=3)
    As = np.stack([oracle.eval_hx(problem.dHdx_index, X[i], P[i]) for i in range(X.shape[0])])
    bs = np.stack([oracle.eval_ht(problem.dHdt_index, X[i], P[i], D[i]) for i in range(X.shape[0])])
    xg = cgesv_batched(As, bs)
    for i in range(As.shape[0]):
        xr = oracle.cgesv_gpu(As[i], bs[i])
        assert same(xg[i], xr).all(), f"LU mismatch on system {i}"


def test_cgesv_edge_cases(oracle):
    """Random dense, exact ties in the pivot column, a zero column (zero pivot)
    and a NaN entry: the kernel follows dev-cgesv-batched-small.cuh semantics."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_batched
    A, b = edge_case_systems()
    n = A.shape[0]
    xg = cgesv_batched(A, b)
    for i in range(n):
        xr = oracle.cgesv_gpu(A[i], b[i])
        assert same(xg[i], xr).all(), f"edge-case LU mismatch on system {i}"
    # well-conditioned systems also solve the linear system
    Ac = A[8:, ..., 0] + 1j * A[8:, ..., 1]
    bc = b[8:, ..., 0] + 1j * b[8:, ..., 1]
    xc = xg[8:, ..., 0] + 1j * xg[8:, ..., 1]
    res = np.abs(np.einsum("nij,nj->ni", Ac, xc) - bc).max(axis=1) / np.abs(bc).max(axis=1)
    assert np.median(res) < 1e-4


def test_cgesv_extreme_scales(problem, oracle, samples100):
    """Every exit of the v9 LU's fast pivot step (hc_lu.hpp): pivots below 2^-90
    and at/above 2^120, entries at/above 2^88 (the whole solve runs dense), an
    infinity, NaN at the pivot position, denormals, and structurally sparse
    tracker Jacobians at those scales -- bit-exact against the oracle."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_batched
    As, bs = extreme_scale_systems(problem, oracle, samples100)
    xg = cgesv_batched(As, bs)
    for i in range(As.shape[0]):
        xr = oracle.cgesv_gpu(As[i], bs[i])
        assert same(xg[i], xr).all(), f"extreme-scale LU mismatch on system {i}"


@pytest.mark.parametrize("mode", [KERNEL_BY_SIZE, SMALL_NEVER], ids=["latency_kernel", "throughput_kernel"])
def test_tracker_matches_oracle_small(problem, oracle, samples100, tracker, mode):
    """Full GPU-HC tracking of 2 samples (624 paths) vs the oracle, value for value."""
    tgt, dif, _ = samples100
    N = 2
    with launch_mode(tracker.L, mode):
        r = tracker.track(tgt[:N], dif[:N]).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index))
    # x[30] is never written by the kernel (reference :282 writes tx < 30 only)
    assert (r["tracks"][:, 30, 0] == 1.0).all()


@pytest.mark.parametrize("mode", [KERNEL_BY_SIZE, SMALL_NEVER], ids=["latency_kernel", "throughput_kernel"])
def test_tracker_dense_resolve_matches_oracle(problem, oracle, samples100, tracker, mode):
    """The tracker's dense re-solve (hc_lu.hpp lu_solve<true>, taken when a
    Jacobian entry reaches 2^64 or a pivot leaves the fast-reciprocal range):
    config 2 never takes it (profiles/r3e_lu_work.json), so this run forces it.
    Sample 0 is config 2's, samples 1 and 2 have their target parameters scaled
    by 2^40 and 2^70: their Jacobians pass 2^64 within the first steps (2^70:
    at t = 0.01 already, max |entry| 7.5e36) and most paths run to infinity.
    Because the dequeue is track-major, waves pair a normal path with a scaled
    one, so a normal half is re-solved densely beside a scaled half (the redo is
    wave-uniform) and must come out identical.  Bit-exact against the oracle."""
    tgt, dif, _ = samples100
    T, D = scaled_samples(problem, tgt[0], (0, 40, 70))
    assert np.array_equal(T[0], tgt[0]) and np.array_equal(D[0], dif[0])
    with launch_mode(tracker.L, mode):
        r = tracker.track(T, D).host()
    ref = _, conv, inf, _ = oracle.gpuhc_track(problem.start_sols, problem.start_params, T, D, problem.unified_index)
    assert_matches_oracle(r, ref)
    assert inf[312:].sum() > 600 and conv[:312].sum() > 0   # the scaled samples diverge, sample 0 converges


def test_tracker_dense_resolve_abort_mode(problem, oracle, samples100, tracker):
    """The dense re-solve in the abort kernel (its latency-mode LU with the
    always-live column groups in pairs, then lu_solve<true>): the
    2^40- and 2^70-scaled samples first, so that all 936 paths are dequeued
    before any hypothesis can pass, then config 2's sample 0.  Every tracked
    path equals the oracle's abort-off run bit for bit."""
    tgt, dif, _ = samples100
    T, D = scaled_samples(problem, tgt[0], (40, 70, 0))
    r = tracker.track(T, D, abort=True).host()
    tracker.workspace_status()
    ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, T, D, problem.unified_index)
    trk = tracked(r)
    assert trk[:624].all(), "the scaled samples' paths must all be tracked"
    assert_matches_oracle(r, ref, where=trk)
    assert_untouched(r, problem.start_sols, ~trk, allow_empty=True)
    found_ids(r)
    assert ref[2][:624].sum() > 600


@pytest.mark.parametrize("mode", [KERNEL_BY_SIZE, SMALL_ALWAYS], ids=["throughput_kernel", "latency_kernel"])
def test_tracker_matches_golden_N100(problem, samples100, tracker, mode):
    """Config 2 (100 samples, abort off): every flag / count / track hash equals the committed golden run."""
    g = golden("gpuhc_N100_seed0")
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, mode):
        r = tracker.track(tgt, dif).host()
    assert_matches_golden(r, g)
    from trifocal_pose_estimation_using_improved_gpuhc_amd import count_solutions
    assert tuple(g["counts"]) == count_solutions(r["tracks"], r["converge"], r["infinity"])
    # per-path real flags: the input of the prefix pin against the reference's
    # GPU_Sols_Statistics.txt (272 / 5; test_oracle_kat.py)
    real = ((np.abs(r["tracks"][:, :30, 1]).astype(np.float64) <= 1e-4).all(axis=1) & (r["converge"] != 0))
    assert np.array_equal(real.astype(np.uint8), g["real"])
    cc, cr = np.cumsum(r["converge"].astype(np.int64)), np.cumsum(real.astype(np.int64))
    assert (cc[2971:3006] == 272).all() and (cr[2971:3006] == 5).all()


def test_time_slicing_is_bit_exact(problem, samples100, tracker):
    """Time slicing (paths suspended at step boundaries and resumed by any slot,
    hc_trifocal_workspace_size_for) changes when a path runs, never what it
    computes: the config-2 run with and without it agree bit for bit (sign of
    zero and NaN payloads included), and the sliced run did suspend paths."""
    tgt, dif, _ = samples100
    a = tracker.track(tgt, dif, time_slicing=False).host()
    b = tracker.track(tgt, dif, time_slicing=True).host()
    head, tail, avail = ring_counters(tracker)
    assert tail > 1000, f"only {tail} suspensions"
    assert head == tail and avail == 0, "every suspended path was resumed"
    assert_bit_identical(a, b)


def test_time_slicing_concurrent_streams(problem, samples100, tracker):
    """Four sliced launches in flight at once on four streams (own buffers and
    workspaces, the bench's pipelined leg): the suspend / resume hand-over of
    each launch stays inside its own workspace, and every launch equals the
    serial run bit for bit."""
    import torch
    tgt, dif, _ = samples100
    ref = tracker.track(tgt, dif).host()
    dev = tracker.device
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    bufs = [tracker.allocate(tgt.shape[0]) for _ in range(4)]
    wss = [tracker.new_workspace(tgt.shape[0]) for _ in range(4)]
    torch.cuda.synchronize(dev)
    for k in range(4):
        with torch.cuda.stream(streams[k]):
            tracker.reset_tracks(bufs[k])
        tracker.launch(t, d, bufs[k], stream=streams[k], workspace=wss[k])
    torch.cuda.synchronize(dev)
    for k in range(4):
        tracker.workspace_status(wss[k])
        assert_bit_identical(bufs[k].host(), ref)


def test_small_and_large_launches_share_a_workspace(problem, samples100, tracker):
    """One workspace, launches of 100, 8, 100 and 2 samples: the launcher
    alternates between the throughput kernel (k_track) and the latency-mode
    one (k_track_small), which keep the same control block, tables and ring;
    then four 8-sample launches in flight at once on four streams (own
    buffers and workspaces).  Every launch equals the serial run bit for bit."""
    import torch
    tgt, dif, _ = samples100
    ref = tracker.track(tgt, dif, time_slicing=False).host()
    dev = tracker.device
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    ws = tracker.new_workspace(100)
    for n in (100, 8, 100, 2):
        r = tracker.allocate(n)
        tracker.reset_tracks(r)
        tracker.launch(t, d, r, workspace=ws, num_samples=n)
        torch.cuda.synchronize(dev)
        tracker.workspace_status(ws)
        assert_bit_identical(r.host(), ref, rows=slice(0, n * 312))
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    bufs = [tracker.allocate(8) for _ in range(4)]
    wss = [tracker.new_workspace(8) for _ in range(4)]
    torch.cuda.synchronize(dev)
    for k in range(4):
        with torch.cuda.stream(streams[k]):
            tracker.reset_tracks(bufs[k])
        tracker.launch(t, d, bufs[k], stream=streams[k], workspace=wss[k], num_samples=8)
    torch.cuda.synchronize(dev)
    for k in range(4):
        tracker.workspace_status(wss[k])
        assert_bit_identical(bufs[k].host(), ref, rows=slice(0, 8 * 312))


def test_time_slicing_falls_back_when_the_ring_does_not_fit(problem, samples100, tracker):
    """A workspace sized for a smaller GPUHC_Max_Steps than the launch uses
    (hc_trifocal_workspace_size_for_steps) cannot hold one ring entry per
    possible suspension: the launch runs unsliced (ring counters untouched)
    and still equals the serial run bit for bit."""
    import torch
    tgt, dif, _ = samples100
    ref = tracker.track(tgt, dif).host()
    dev = tracker.device
    small = int(tracker.L.hc_trifocal_workspace_size_for_steps(tgt.shape[0], 10))
    assert small < int(tracker.L.hc_trifocal_workspace_size_for_steps(tgt.shape[0], tracker.settings.max_steps))
    ws = torch.zeros(small, dtype=torch.uint8, device=dev)
    r = tracker.allocate(tgt.shape[0])
    tracker.reset_tracks(r)
    tracker.launch(torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev), r, workspace=ws)
    torch.cuda.synchronize(dev)
    assert ring_counters(tracker, ws)[1] == 0, "a launch whose ring does not fit must not slice"
    assert_bit_identical(r.host(), ref)


def test_time_slicing_workspace_reused_across_launch_sizes(problem, samples100, tracker):
    """One workspace, sliced launches of 100, then 50, then 100 samples: the
    ring sits at a fixed offset, so the 50-sample launch meets only entries
    tagged by an older epoch; its suspend blocks follow its ring and overwrite
    cleared entries, which it records as the dirty range, and the second
    100-sample launch re-zeroes them.  (50 samples: 15 600 paths,
    more than the 10 240 path slots of a full grid, so that launch suspends
    paths too.)  Every launch equals the serial run bit for bit."""
    import torch
    tgt, dif, _ = samples100
    ref = tracker.track(tgt, dif, time_slicing=False).host()
    dev = tracker.device
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    ws = tracker.new_workspace(100)
    off = int(tracker.L.hc_trifocal_workspace_size())
    for n in (100, 50, 100):
        r = tracker.allocate(n)
        tracker.reset_tracks(r)
        tracker.launch(t, d, r, workspace=ws, num_samples=n)
        torch.cuda.synchronize(dev)
        tracker.workspace_status(ws)
        head, tail, _ = ring_counters(tracker, ws)
        assert tail > 0 and head == tail, "sliced, and every suspended path resumed"
        rq = np.frombuffer(ws[off:off + 1024].cpu().numpy().tobytes(), np.uint32)
        # RQ_CLEARED: the largest ring so far (one entry per possible suspension + 4096 spare);
        # after the 50-sample launch its suspend blocks lie inside it: the dirty range [195, 196)
        cap = lambda k: k * 312 * ((tracker.settings.max_steps + 1) // 3 + 1) + 4096  # noqa: E731
        assert rq[194] == cap(100)
        if n == 50:
            assert cap(50) <= rq[195] < rq[196] <= cap(100)
        else:
            assert rq[195] == rq[196] == 0
        assert_bit_identical(r.host(), ref, rows=slice(0, n * 312))


def test_time_slicing_abandoned_tickets_are_pushed_again(problem, samples100, tracker):
    """A consumer that waits too long for a ring entry abandons the ticket and
    its pusher pushes the path again: no path is lost to a paused wave
    (VERDICT r3 #5).  hc_trifocal_set_ring_test delays every 16th ticket's
    entry by 2 ms and lets consumers abandon after 250 us; the launch abandons
    tickets (control block word 12) and still equals the unsliced run bit for
    bit, with no device error.  (50 samples: more paths than path slots, so
    paths are suspended.)"""
    import torch
    tgt, dif, _ = samples100
    n = 50
    ref = tracker.track(tgt[:n], dif[:n], time_slicing=False).host()
    dev = tracker.device
    ws = tracker.new_workspace(n)
    r = tracker.allocate(n)
    tracker.reset_tracks(r)
    tracker.L.hc_trifocal_set_ring_test(200000)
    try:
        tracker.launch(torch.from_numpy(tgt[:n]).to(dev), torch.from_numpy(dif[:n]).to(dev), r, workspace=ws)
        torch.cuda.synchronize(dev)
    finally:
        tracker.L.hc_trifocal_set_ring_test(0)
    cb = np.frombuffer(ws[:64].cpu().numpy().tobytes(), np.uint32)
    tracker.workspace_status(ws)
    assert cb[12] > 0, "no ticket was abandoned: the test did not reach the re-push"
    assert_bit_identical(r.host(), ref)


def test_tracker_abort_mode(problem, samples100, tracker):
    """Config 3 semantics (abort on): the found hypothesis is one of the passing
    hypotheses of the abort-off run; tracked paths equal the abort-off results;
    skipped paths keep the start solution with conv = 0."""
    g = golden("gpuhc_N100_seed0")
    passing = golden_passing(g)
    assert passing, "the golden run must contain a passing hypothesis"
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif, abort=True).host()
    assert r["found"]
    found = set(found_ids(r).tolist())
    assert found and found <= passing
    st = r["stats"]
    trk = tracked(r)
    assert_matches_golden(r, g, where=trk)
    assert_untouched(r, problem.start_sols, ~trk, allow_empty=True)
    # inlier counts of scored paths equal the oracle's scoring
    sc = {int(b): s for b, s in zip(g["scored_ids"], g["scored"])}
    for b in np.nonzero(trk & (r["converge"] == 1))[0]:
        ok, i21, i31 = sc[int(b)]
        if st["inliers21"][b] or st["inliers31"][b] or ok:
            assert (st["inliers21"][b], st["inliers31"][b]) == (i21, i31)
    assert tracker.first_found_seconds() > 0


@pytest.mark.gpu
def test_tracker_abort_chunked(problem, samples100, tracker):
    """The multi-GPU early-stop protocol on one rank: 100 samples in chunks of
    10 launches, one workspace each.  Found ids (made global) are passing
    hypotheses, tracked paths equal the abort-off golden run, and once a chunk
    has found a pose every later chunk skips all of its paths."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import sharding
    g = golden("gpuhc_N100_seed0")
    passing = golden_passing(g)
    tgt, dif, _ = samples100
    dev = tracker.device
    t = torch.from_numpy(tgt).to(dev)
    d = torch.from_numpy(dif).to(dev)
    r = tracker.allocate(100, stats=True, abort=True)
    tracker.reset_tracks(r)
    wss = []
    parts = tracker.launch_abort_chunked(t, d, r, chunk_samples=10, workspaces=wss)
    torch.cuda.synchronize(dev)
    h = r.host()
    assert len(parts) == 10 and h["found"]
    found = set()
    for off, n in parts:   # a chunk launch writes ids within the chunk
        loc = h["batch_index"][off * 312:(off + n) * 312]
        found_ids(dict(batch_index=loc))
        found |= set(int(b) for b in sharding.global_batch_ids(loc, off, 0))
    assert found and found <= passing
    trk = tracked(h)
    assert_matches_golden(h, g, where=trk)
    assert_untouched(h, problem.start_sols, ~trk)
    first_chunk = min(b // 312 for b in found) // 10
    assert not trk[(first_chunk + 1) * 3120:].any()
    stamps = [tracker.read_timestamps(w)[:2] for w in wss]
    hz = tracker.read_timestamps(wss[0])[2]
    assert sharding.first_found_seconds(stamps, hz) > 0


@pytest.mark.gpu
def test_cli_config2_matches_golden(tmp_path):
    """bin/magmaHC-main (C++ GPU_HC_Solver over the C-ABI) on config 2: the
    solution statistics it writes equal the golden run's counts."""
    _, read = run_cli(tmp_path)
    stats = read("GPU_Sols_Statistics.txt").split()
    assert [int(v) for v in stats[:3]] == [int(v) for v in golden("gpuhc_N100_seed0")["counts"]]
    assert float(read("GPU_Timings.txt").split()[0]) > 0
    # device pose recovery: the maximal-support pose matches GT_Poses*_000
    pr = read("GPU_Pose_Results.txt").split()
    gp = golden("pose_N100_seed0")
    assert int(pr[0]) == 1 and [int(pr[5]), int(pr[6])] == gp["path"].tolist() and int(pr[7]) == int(gp["num_candidates"])
    assert max(float(v) for v in pr[1:5]) < 1e-3
    # abort mode (config 3 semantics through the CLI)
    run_cli(tmp_path, "-n", "1000", "--abort")


@pytest.mark.gpu
def test_cli_four_rounds(tmp_path):
    """`magmaHC-main -t 4` (TEST_RANSAC_TIMES = 4; cmd/magmaHC-main.cpp:38-48):
    round ti reads Triplet_Edgels_<ti> and GT_Poses*_<ti> and draws its samples
    with srand(ti) (GPU_HC_Solver.cpp:252-306).  Every round writes its timing,
    solution statistics and pose line; every round's counts equal the oracle's
    (tests/golden/cli_rounds_counts.npz)."""
    stdout, read = run_cli(tmp_path, "-t", "4")
    ms = [float(v) for v in read("GPU_Timings.txt").split()]
    assert len(ms) == 4 and min(ms) > 0
    stats = [ln.split() for ln in read("GPU_Sols_Statistics.txt").splitlines()]
    assert len(stats) == 4 and all(int(r[0]) > 0 for r in stats)
    assert [int(v) for v in stats[0]] == [int(v) for v in golden("gpuhc_N100_seed0")["counts"]]
    # every round's counts equal the oracle's run of that round's dataset and draw
    rounds = golden("cli_rounds_counts")["counts"]
    assert [[int(v) for v in r[:3]] for r in stats] == rounds.tolist()
    assert len(read("GPU_Pose_Results.txt").splitlines()) == 4
    assert "Running 4 rounds" in stdout


def test_ph_codeopt_matches_oracle_small(problem, oracle, samples100, tracker):
    """The archived ..._PH_CodeOpt semantics (hc_trifocal_2op1p_30x30_track_ph_codeopt:
    no depth-sign truncation) on 2 samples vs the oracle, value for value."""
    tgt, dif, _ = samples100
    N = 2
    r = tracker.track(tgt[:N], dif[:N], truncate=False).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index, oracle.settings(truncate=False)))


def test_ph_codeopt_matches_golden_N100(problem, samples100, tracker):
    """Config 2 without path truncation: every flag / count / track hash equals the
    oracle's committed run (tests/golden/gpuhc_phcodeopt_N100_seed0.npz)."""
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif, truncate=False).host()
    assert_matches_golden(r, golden("gpuhc_phcodeopt_N100_seed0"))


def test_ph_matches_oracle_small(problem, oracle, samples100, tracker):
    """The archived ..._PH semantics (explicit RK helpers, no truncation;
    hc_trifocal_2op1p_30x30_track_ph) on 2 samples vs the oracle, value for value."""
    tgt, dif, _ = samples100
    N = 2
    r = tracker.track(tgt[:N], dif[:N], truncate=False, explicit_rk=True).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N],
                                                problem.unified_index,
                                                oracle.settings(truncate=False, explicit_rk=True)))


def test_ph_matches_golden_N100(problem, samples100, tracker):
    """Config 2 through the archived ..._PH semantics: every flag / count / track
    hash equals the oracle's committed run (tests/golden/gpuhc_ph_N100_seed0.npz)."""
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif, truncate=False, explicit_rk=True).host()
    assert_matches_golden(r, golden("gpuhc_ph_N100_seed0"))


def test_eval_row_permuted_tables_match_oracle(problem, oracle, samples100):
    """The table builder's lane assignments (dH/dx entries bin-packed over the
    32 lanes, the dH/dt | H owner / helper pairs lane ^ 16) for equation orders
    other than the reference's: reversed (the long dH/dt rows land in lanes
    0..11, their helpers in 16..27) and a random order that still pairs every
    long row with a short one."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_batched
    tgt, dif, _ = samples100
    X, P, D = _jacobians_from_path(problem, oracle, tgt, dif, n=48, seed=5)
    nt = (problem.dHdt_index.reshape(-1, 30)[::6] != 0).sum(axis=0)   # terms per row (coefficient rows)
    rng = np.random.default_rng(11)
    perms = [np.arange(29, -1, -1)]
    while len(perms) < 2:
        p = rng.permutation(30)
        n = nt[p]
        if all(not (n[r] > 13 and (r ^ 16 >= 30 or n[r ^ 16] > 10)) for r in range(30)):
            perms.append(p)
    for perm in perms:
        dx, dt, U = _row_permuted(problem, perm)
        HX, HT, H = eval_batched(U, X, P, D)
        for i in range(X.shape[0]):
            assert same(HX[i], oracle.eval_hx(dx, X[i], P[i])).all(), f"dH/dx mismatch at point {i}, perm {perm}"
            assert same(HT[i], oracle.eval_ht(dt, X[i], P[i], D[i])).all(), f"dH/dt mismatch {i}, perm {perm}"
            assert same(H[i], oracle.eval_h(dt, X[i], P[i])).all(), f"H mismatch {i}, perm {perm}"


def test_eval_rejects_tables_without_helpers(problem):
    """Two long dH/dt rows paired as lane ^ 16 partners (neither can help the
    other): the table builder rejects the table (HC_ERROR_TABLE) and the
    kernels leave their outputs untouched."""
    import torch
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    perm = np.arange(30)
    perm[2], perm[19] = 19, 2          # lanes 2 and 18: rows 19 and 18, 16 terms each
    _, _, U = _row_permuted(problem, perm)
    L = _abi.lib()
    dev = torch.device("cuda:0")
    n = 4
    Ut = torch.from_numpy(U).to(dev)
    X = torch.zeros((n, 31, 2), dtype=torch.float32, device=dev)
    P = torch.zeros((n, 34, 2), dtype=torch.float32, device=dev)
    HX = torch.full((n, 30, 30, 2), 7.0, dtype=torch.float32, device=dev)
    HT = torch.full((n, 30, 2), 7.0, dtype=torch.float32, device=dev)
    H = torch.full((n, 30, 2), 7.0, dtype=torch.float32, device=dev)
    wsb = int(L.hc_trifocal_workspace_size())
    ws = torch.zeros(wsb, dtype=torch.uint8, device=dev)
    p = _abi.ptr
    _abi.call("hc_trifocal_eval_batched", n, p(Ut), p(X), p(P), p(P), p(HX), p(HT), p(H), p(ws), wsb,
              p(torch.cuda.current_stream(dev)))
    torch.cuda.synchronize(dev)
    assert int(L.hc_trifocal_workspace_status(p(ws))) == 5   # HC_ERROR_TABLE
    assert (HX == 7.0).all() and (HT == 7.0).all() and (H == 7.0).all()


def _outside_lu_structure(dx):
    """Rows whose dH/dx structure has an entry outside the specialised LU's
    (hc_lu_struct.hpp LU_STRUCT_PAT, include/hc_trifocal_testing.h)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    coef = dx.reshape(30, 8, 5, 30)[:, :, 0, :]            # [column, term, row]
    pat = [sum(1 << c for c in range(30) if (coef[c, :, r] != 0).any()) for r in range(30)]
    return [r for r in range(30) if pat[r] & ~int(L.hc_lu_struct_pattern(r))]


@pytest.mark.parametrize("mode", [KERNEL_BY_SIZE, SMALL_NEVER], ids=["latency_kernel", "throughput_kernel"])
def test_tracker_row_permuted_structure_matches_oracle(problem, oracle, samples100, ransac0, mode):
    """Any table the reference kernel takes is tracked.  A
    row-permuted system (valid and equivalent) has a dH/dx structure outside
    the one the specialised LU compiles in; k_prep_tables routes it to the
    structure-agnostic instantiation enqueued beside the specialised one.
    Tracking (abort off, the archived PH_CodeOpt semantics, and abort mode)
    of 2 samples equals the oracle on the same permuted tables value for
    value, and the problem's own table still runs the specialised kernel."""
    import dataclasses

    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    tgt, dif, _ = samples100
    N = 2
    for swap in ((0, 9), (5, 14)):
        perm = np.arange(30)
        perm[swap[0]], perm[swap[1]] = swap[1], swap[0]
        dx, dt, U = _row_permuted(problem, perm)
        assert _outside_lu_structure(dx), f"permutation {swap} stays within the specialised LU's structure"
        tr = DeviceTracker(dataclasses.replace(problem, dHdx_index=dx, dHdt_index=dt), torch.device("cuda:0"))
        tr.set_ransac_data(ransac0)
        for truncate in (True, False):
            with launch_mode(tr.L, mode):
                r = tr.track(tgt[:N], dif[:N], truncate=truncate).host()
            tr.workspace_status()
            ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:N], dif[:N], U,
                                     oracle.settings(truncate=truncate))
            assert_matches_oracle(r, ref)
            if truncate:
                ref_abort_off = ref
        # abort mode: every path it tracked equals the abort-off oracle run
        a = tr.track(tgt[:N], dif[:N], abort=True).host()
        tr.workspace_status()
        assert_matches_oracle(a, ref_abort_off, where=tracked(a))
    assert not _outside_lu_structure(problem.dHdx_index)


def test_ring_check_reports_an_undrained_ring(tracker):
    """The end check of a sliced launch (k_ring_check): a ring left
    with head != tail, or with an unclaimed entry (avail != 0), is a suspended
    path that was never resumed: HC_ERROR_DEVICE with ring_fail = (~0, avail,
    tail, head); a drained ring stays silent."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd._abi import ptr
    L = tracker.L
    wsb = int(L.hc_trifocal_workspace_size_for(1))
    hs = ptr(torch.cuda.current_stream(tracker.device))
    for head, tail, avail, bad in ((7, 7, 0, False), (9, 7, 0, True), (7, 7, 1, True)):
        ws = torch.zeros(wsb, dtype=torch.uint8, device=tracker.device)
        assert int(L.hc_trifocal_ring_check_test(ptr(ws), wsb, head, tail, avail, hs)) == 0
        torch.cuda.synchronize(tracker.device)
        st = int(L.hc_trifocal_workspace_status(ptr(ws)))
        cb = np.frombuffer(ws[:64].cpu().numpy().tobytes(), np.uint32)
        if bad:
            assert st == 4 and list(cb[8:12]) == [0xFFFFFFFF, avail, tail, head], (st, cb[8:12])
        else:
            assert st == 0 and (cb[8:12] == 0).all()
    small = int(L.hc_trifocal_workspace_size())
    assert int(L.hc_trifocal_ring_check_test(ptr(ws), small, 1, 0, 0, hs)) == 2
