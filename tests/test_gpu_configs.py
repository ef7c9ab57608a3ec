"""GPU tests of the BASELINE.json configs beyond config 2, through the C-ABI:

  config 5  sigma = 1 px noisy synthcurves (path pruning is always on): the HIP
            tracker against the oracle value for value (2 samples live, 100
            samples against the committed golden run), and the device pose
            support on those tracks against the golden selection;
  config 3  1000 samples with early abort, in both abort semantics
            (hcAbortArgs::inflight_stop = 0, the reference's; = 1): every found
            hypothesis passes the oracle's scoring on its own track, tracked
            paths equal the oracle's tracks of the same batch ids, skipped
            paths are untouched;
  gate 2     reference-independent: every converged real
            solution of config 2 satisfies the target system in FP64;
  largest   config 4's whole workload (8000 samples) in one tracking launch
            on one GPU: the golden prefix, oracle paths across the launch.
"""
import numpy as np
import pytest

from checks import (assert_matches_golden, assert_matches_oracle, assert_same_run, assert_untouched, found_ids, golden,
                    noisy_data, ring_counters, tracked)
from conftest import same
from residual import RESIDUAL_TOL, max_relative_residual, real_converged

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def noisy1px(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params
    nd = noisy_data()
    tgt, dif, picked = prepare_target_params(problem, nd, seed=0, num_samples=100)
    return nd, tgt, dif, picked


def test_noisy_samples_match_golden(noisy1px):
    """The native noise generator + Prepare_Target_Params reproduce the fixture's inputs."""
    g = golden("gpuhc_noisy1px_N100")
    _, tgt, dif, picked = noisy1px
    assert np.array_equal(picked, g["picked"])
    assert np.array_equal(tgt, g["target"]) and np.array_equal(dif, g["diff"])


def test_noisy_tracker_matches_oracle_small(problem, oracle, tracker, noisy1px):
    """Config 5 inputs, 2 samples (624 paths), value for value against the oracle."""
    _, tgt, dif, _ = noisy1px
    r = tracker.track(tgt[:2], dif[:2]).host()
    assert_matches_oracle(r, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:2], dif[:2],
                                                problem.unified_index))


def test_noisy_tracker_and_pose_match_golden_N100(tracker, noisy1px):
    """Config 5, 100 samples: every flag / count / track hash equals the oracle's
    golden run; the device pose support over the HIP tracks selects the golden
    paths with the golden inlier counts, and its GT verdict is the golden one."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import count_solutions, pose
    g = golden("gpuhc_noisy1px_N100")
    nd, tgt, dif, _ = noisy1px
    res = tracker.track(tgt, dif)
    r = res.host()
    assert_matches_golden(r, g)
    assert tuple(g["counts"]) == count_solutions(r["tracks"], r["converge"], r["infinity"])
    import torch
    E = torch.from_numpy(np.array(nd.locations)).to(tracker.device)
    inl, sel = pose.pose_support(res.tracks, res.converge, E, tracker.K)
    assert sel["num_candidates"] == int(g["num_candidates"])
    assert [sel["path21"], sel["path31"]] == g["path"].tolist()
    assert [sel["inliers21"], sel["inliers31"]] == g["inliers"].tolist()
    assert (inl[inl[:, 0] >= 0] == g["cand_inliers"]).all()
    out, ok = pose.residuals(nd, sel)
    assert ok == bool(g["success"]) and np.allclose(out, g["residuals"], rtol=0, atol=1e-6)


def test_residual_gate_config2(problem, samples100, tracker):
    """Gate 2: every converged real solution of config 2 (100 samples) has an FP64
    relative residual |H_r(x, p_target)| / sum_j |term_rj| <= 1e-4 on every equation."""
    tgt, dif, _ = samples100
    r = tracker.track(tgt, dif).host()
    ids = real_converged(r["tracks"], r["converge"])
    assert len(ids) > 0
    worst = max_relative_residual(problem.dHdt_index, r["tracks"], ids, tgt)
    assert worst <= RESIDUAL_TOL, worst


def test_largest_launch_config4_workload_on_one_gpu(problem, oracle, tracker, ransac0):
    """The largest launch: config 4's whole workload, 8000 samples (2 496 000
    paths), in one tracking launch on one GPU with time slicing (its ring and
    suspend blocks: 1.2 GB).  Samples are independent and their srand(0) draws
    are one sequence, so the first 100 samples equal the N = 100 golden run;
    700 paths drawn across the launch equal the oracle's tracks of the same
    batch ids; every suspended path was resumed."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params
    N = 8000
    tgt, dif, _ = prepare_target_params(problem, ransac0, seed=0, num_samples=N)
    r = tracker.track(tgt, dif)
    head, tail, avail = ring_counters(tracker)
    assert tail > 100000 and head == tail and avail == 0, "sliced, and every suspended path resumed"
    st = r.stats.cpu().numpy().view(np.int32).reshape(-1, 4)
    assert (st[:, 0] >= 1).all() and (st[:, 0] <= tracker.settings.max_steps + 1).all()

    def rows(sel):   # the host dict of some rows (all 2 496 000 tracks are 619 MB)
        at = torch.from_numpy(np.arange(N * 312)[sel]).to(r.tracks.device)
        return dict(tracks=r.tracks[at].cpu().numpy(), converge=r.converge[at].cpu().numpy(),
                    infinity=r.infinity[at].cpu().numpy(), stats=dict(steps=st[sel, 0], corrections=st[sel, 1]))

    assert_matches_golden(rows(slice(0, 100 * 312)), golden("gpuhc_N100_seed0"))
    ids = np.sort(np.random.default_rng(7).choice(N * 312, 700, replace=False))
    o_tr, o_conv, o_inf, o_st = oracle.gpuhc_track_subset(ids, problem.start_sols, problem.start_params, tgt, dif,
                                                          problem.unified_index)
    assert_same_run(rows(ids), o_tr[ids], o_conv[ids], o_inf[ids], o_st["steps"][ids], o_st["corrections"][ids])


@pytest.mark.parametrize("inflight_stop", [0, 1])
def test_abort_config3_N1000(problem, oracle, tracker, ransac0, inflight_stop):
    """Config 3 (1000 samples, abort on).  Found hypotheses pass the oracle's
    scoring on their own (HIP == oracle) tracks; every tracked path (round 4:
    all of them, ~14 k with the reference's semantics, ~6 k with inflight_stop;
    round 3 checked the found paths and a sample of 400) equals the oracle's
    track of the same batch id; skipped
    (and, with inflight_stop, stopped) paths keep the start solution with conv 0
    and zero stats.  Reference semantics (inflight_stop 0): a path that started
    tracking writes its full result."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params
    N = 1000
    tgt, dif, _ = prepare_target_params(problem, ransac0, seed=0, num_samples=N)
    r = tracker.track(tgt, dif, abort=True, inflight_stop=bool(inflight_stop)).host()
    assert r["found"]
    found = found_ids(r)
    st = r["stats"]
    trk = tracked(r)
    assert len(found) > 0 and trk[found].all() and (r["converge"][found] == 1).all()
    check = np.nonzero(trk)[0]
    assert_matches_oracle(r, oracle.gpuhc_track_subset(check, problem.start_sols, problem.start_params, tgt, dif,
                                                       problem.unified_index), where=check)
    for b in found:
        ok, i21, i31 = oracle.score_hypothesis(r["tracks"][b], ransac0.locations, ransac0.K)
        assert ok == 1 and (st["inliers21"][b], st["inliers31"][b]) == (i21, i31)
    assert_untouched(r, problem.start_sols, ~trk)
    if inflight_stop == 0:
        # nothing is cut short: every tracked path either converged, diverged,
        # was pruned or ran out of steps -- exactly what the oracle reports for it
        assert len(check) > len(found)


HELDOUT = ("010", "050", "099")


@pytest.mark.parametrize("ds", HELDOUT)
def test_heldout_dataset_matches_golden_N100(problem, oracle, tracker, ds):
    """Config 2 on synthcurves datasets no tuning of this build ever saw
    (the LU's always-live groups, the track order and the time
    to the first pose were measured on datasets 000-002 only): the reference's
    srand(0) samples drawn from Triplet_Edgels_<ds>, 100 samples.  Two samples
    value for value against the oracle live; all 100 against the committed
    golden run (flags, counts, track hashes); the device pose support over the
    HIP tracks selects the golden paths, and its verdict against GT_Poses21/31
    of the same dataset is the golden one."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import (count_solutions, load_ransac_data, pose,
                                                                   prepare_target_params)
    g = golden(f"gpuhc_ds{ds}_N100_seed0")
    data = load_ransac_data(int(ds))
    tgt, dif, picked = prepare_target_params(problem, data, seed=0, num_samples=100)
    assert np.array_equal(picked, g["picked"]) and np.array_equal(tgt, g["target"]) and np.array_equal(dif, g["diff"])
    if ds == "050":
        r2 = tracker.track(tgt[:2], dif[:2]).host()
        assert_matches_oracle(r2, oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:2], dif[:2],
                                                     problem.unified_index))
    res = tracker.track(tgt, dif)
    r = res.host()
    assert_matches_golden(r, g)
    assert same(r["tracks"][:624, :30], g["tracks_s01"][:, :30]).all()
    assert tuple(g["counts"]) == count_solutions(r["tracks"], r["converge"], r["infinity"])
    E = torch.from_numpy(np.ascontiguousarray(data.locations)).to(tracker.device)
    K = torch.from_numpy(np.ascontiguousarray(data.K)).to(tracker.device)
    inl, sel = pose.pose_support(res.tracks, res.converge, E, K)
    assert sel["num_candidates"] == int(g["num_candidates"])
    assert [sel["path21"], sel["path31"]] == g["path"].tolist()
    assert [sel["inliers21"], sel["inliers31"]] == g["inliers"].tolist()
    out, ok = pose.residuals(data, sel)
    assert ok == bool(g["success"]) and np.allclose(out, g["residuals"], rtol=0, atol=1e-6)
