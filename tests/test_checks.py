"""The parity bar itself (tests/checks.py), on the CPU: every checker accepts a
run against itself and rejects each single difference it exists to catch.

One oracle run of one sample (dataset 000, srand(0), sample 0: 312 paths, 32
converge, 20 go to infinity, path 104 alone passes score_hypothesis with 5117 of
5117 inliers in both views) stands in for a TrackResult.host() dict.
"""
import copy

import numpy as np
import pytest

import checks
from checks import (GroupCase, assert_bit_identical, assert_matches_golden, assert_matches_oracle, assert_same_run,
                    assert_untouched, check_group_result, found_ids, gate_score, golden, launch_mode, oracle_score,
                    passes_gate)
from joint_reference import joint_reference

N = 312
FOUND = 104


@pytest.fixture(scope="module")
def run(problem, oracle, ransac0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import prepare_target_params
    tgt, dif, _ = prepare_target_params(problem, ransac0, seed=0, num_samples=1)
    ref = tr, conv, inf, st = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt, dif,
                                                 problem.unified_index)
    assert (int(conv.sum()), int(inf.sum())) == (32, 20) and conv[FOUND] == 1 and (st["steps"] > 0).all()
    for v in ref:
        v.setflags(write=False)
    return dict(target=tgt, ref=ref, host=dict(tracks=tr, converge=conv, infinity=inf, stats=st))


def host(run, **changes):
    """A writable copy of the run as a host dict; changes: key -> (index, value),
    "steps" ... "inliers31" addressing the stats."""
    r = copy.deepcopy(run["host"])
    for k, (at, v) in changes.items():
        (r["stats"][k] if k in checks.STAT_KEYS else r[k])[at] = v
    return r


def rejects(check, *args, **kw):
    with pytest.raises(AssertionError):
        check(*args, **kw)


def test_same_run_accepts_the_run_itself(run):
    assert_matches_oracle(host(run), run["ref"])
    assert checks.tracked(run["host"]).all()


def test_same_run_accepts_a_zero_of_the_other_sign_and_nan_on_both_sides(run):
    tr = run["ref"][0].copy()
    tr[5, 2, 1], tr[7, 4, 0] = 0.0, np.nan
    ref = (tr,) + run["ref"][1:]
    assert_matches_oracle(host(run, tracks=((5, 2, 1), 0.0)), ref, where=[5])
    r = host(run, tracks=((5, 2, 1), -0.0))
    r["tracks"][7, 4, 0] = np.nan
    assert np.signbit(r["tracks"][5, 2, 1]) and not np.signbit(tr[5, 2, 1])
    assert_matches_oracle(r, ref)


@pytest.mark.parametrize("key,at,new", [
    ("converge", 40, lambda old: 1 - old), ("infinity", 40, lambda old: 1 - old), ("steps", 40, lambda old: old + 1),
    ("corrections", 40, lambda old: old + 1), ("tracks", (FOUND, 3, 0), lambda old: np.nextafter(old, np.float32(9))),
    ("tracks", (FOUND, 3, 0), lambda old: np.float32(np.nan))],
    ids=["converge", "infinity", "steps", "corrections", "one_ulp", "nan_on_one_side"])
def test_same_run_rejects_one_difference(run, key, at, new):
    old = (run["host"]["stats"] if key in checks.STAT_KEYS else run["host"])[key][at]
    assert np.isfinite(old) and abs(old) < 9 or key != "tracks"
    rejects(assert_matches_oracle, host(run, **{key: (at, new(old))}), run["ref"])


def test_matches_golden_and_its_rows(run):
    """The run is the first sample of the committed config-2 golden run."""
    g = golden("gpuhc_N100_seed0")
    assert_matches_golden(host(run), g, rows=slice(0, N))
    rejects(assert_matches_golden, host(run), g, rows=slice(N, 2 * N))
    rejects(assert_matches_golden, host(run, steps=(40, 1)), g, rows=slice(0, N))
    bad = {k: g[k][:N].copy() for k in ("conv", "inf", "steps", "corrections", "hash")}
    assert_matches_golden(host(run), bad)
    bad["hash"][40] ^= np.uint64(1)
    rejects(assert_matches_golden, host(run), bad)
    assert_matches_golden(host(run), bad, where=np.arange(N) != 40)


def test_bit_identical_is_stricter_than_same_run(run):
    a = host(run, tracks=((5, 2, 1), 0.0))
    b = host(run, tracks=((5, 2, 1), -0.0))
    assert_bit_identical(a, copy.deepcopy(a))
    assert_same_run(b, a["tracks"], a["converge"], a["infinity"], a["stats"]["steps"], a["stats"]["corrections"])
    rejects(assert_bit_identical, b, a)
    rejects(assert_bit_identical, host(run, tracks=((5, 30, 0), 2.0)), host(run))     # x[30] too
    rejects(assert_bit_identical, host(run, corrections=(40, 999)), host(run))
    two = {k: np.concatenate([v, v]) for k, v in a.items()}
    assert_bit_identical(a, two, rows=slice(N, 2 * N))


def test_where_restricts_the_comparison_and_must_select_something(run):
    r = host(run, converge=(200, 1 - run["host"]["converge"][200]))
    outside = np.ones(N, bool)
    outside[200] = False
    assert_matches_oracle(r, run["ref"], where=outside)
    assert_matches_oracle(r, run["ref"], where=np.array([199, 201]))
    rejects(assert_matches_oracle, r, run["ref"], where=~outside)
    rejects(assert_matches_oracle, r, run["ref"], where=np.array([200, 201]))
    rejects(assert_matches_oracle, host(run), run["ref"], where=np.zeros(N, bool))
    rejects(assert_matches_oracle, host(run), run["ref"], where=np.array([], np.int64))
    assert_matches_oracle(host(run), run["ref"], where=np.zeros(N, bool), allow_empty=True)
    rejects(assert_matches_oracle, host(run), run["ref"], where=np.ones(N + 1, bool))


def untouched(problem, gated=True):
    r = dict(tracks=problem.start_sols.copy(), converge=np.zeros(N, np.uint8), infinity=np.zeros(N, np.uint8),
             stats=np.zeros(N, checks_stats_dtype()))
    if gated:
        r["joint_inliers"] = np.full(N, -1, np.int32)
    return r


def checks_stats_dtype():
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import PATH_STATS_DTYPE
    return PATH_STATS_DTYPE


def test_untouched(problem):
    everything = np.ones(N, bool)
    assert_untouched(untouched(problem), problem.start_sols, everything)
    assert_untouched(untouched(problem, gated=False), problem.start_sols, everything)
    rejects(assert_untouched, untouched(problem), problem.start_sols, ~everything)
    for key, at, v in (("converge", 3, 1), ("infinity", 3, 1), ("inliers21", 3, 7), ("steps", 3, 1),
                       ("tracks", (3, 30, 0), 2.0), ("tracks", (3, 0, 1), 0.5), ("joint_inliers", 3, 0)):
        r = untouched(problem)
        (r["stats"][key] if key in checks.STAT_KEYS else r[key])[at] = v
        rejects(assert_untouched, r, problem.start_sols, everything)
        assert_untouched(r, problem.start_sols, np.arange(N) != 3)     # the other paths are still fine


def test_found_ids(run):
    bi = np.full(N, -1, np.int32)
    assert len(found_ids(dict(batch_index=bi))) == 0
    bi[FOUND] = FOUND
    assert found_ids(dict(batch_index=bi)).tolist() == [FOUND]
    bi[FOUND] = FOUND - 1
    rejects(found_ids, dict(batch_index=bi))


# ---- the group-result checker on one triplet with one sample ----------------

def group_result(run, **changes):
    """What a grouped abort launch that found path 104 would return: every
    path tracked as the plain run tracks it."""
    r = host(run, **changes)
    r["found"] = np.array([1], np.uint8)
    r["found_ticks"] = np.array([123456789], np.uint64)
    r["batch_index"] = np.full(N, -1, np.int32)
    r["batch_index"][FOUND] = FOUND
    return r


def skip_path(r, problem, p):
    """Path p as a launch leaves one it never dequeued."""
    r["tracks"][p] = problem.start_sols[p]
    r["converge"][p] = r["infinity"][p] = 0
    r["stats"][p] = 0
    if "joint_inliers" in r:
        r["joint_inliers"][p] = -1


@pytest.fixture(scope="module")
def abort_case(problem, oracle, ransac0, run):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    batch = TripletBatch(problem, [ransac0], seeds=0, samples_per_triplet=1)
    assert np.array_equal(batch.target, run["target"])
    ok, i21, i31 = oracle.score_hypothesis(run["host"]["tracks"][FOUND], ransac0.locations, ransac0.K)
    assert (ok, i21, i31) == (1, 5117, 5117)
    return GroupCase(batch, copy.deepcopy(run["host"])), dict(inliers21=(FOUND, i21), inliers31=(FOUND, i31))


def test_group_checker_with_the_oracle_score(problem, oracle, run, abort_case):
    case, counts = abort_case
    score = oracle_score(oracle)

    def check(r, expect_ids={FOUND}):
        return check_group_result(r, case, problem.start_sols, score, [1], expect_ids, all_tracked=(0,))

    assert check(group_result(run, **counts)).all()
    r = group_result(run, **counts)
    r["found"][0] = 0
    rejects(check, r)
    other = int(np.nonzero(run["host"]["converge"])[0][0])
    assert other != FOUND
    r = group_result(run, **counts)
    r["batch_index"][other] = other                    # a second id, which does not pass the oracle's scoring
    rejects(check, r)
    rejects(check, r, expect_ids=None)
    rejects(check, group_result(run, inliers21=(FOUND, 5116), inliers31=counts["inliers31"]))
    r = group_result(run, **counts)
    r["batch_index"][FOUND] = FOUND - 1
    rejects(check, r)
    r = group_result(run, **counts)
    r["found_ticks"][0] = 0
    rejects(check, r)
    rejects(check, group_result(run, steps=(40, 1), **counts))         # a tracked path unlike the plain run's
    # a path the launch skipped: fine with all_tracked=(), but only as the start solution
    r = group_result(run, **counts)
    skip_path(r, problem, 5)
    rejects(check, r)
    trk = check_group_result(r, case, problem.start_sols, score, [1], {FOUND})
    assert not trk[5] and trk.sum() == N - 1
    r["tracks"][5, 30, 0] = 2.0
    rejects(check_group_result, r, case, problem.start_sols, score, [1], {FOUND})
    rejects(check_group_result, group_result(run, **counts), case, problem.start_sols, score, [1], {FOUND},
            none_tracked=(0,))


def test_group_checker_with_the_gate_score(problem, oracle, ransac0, run):
    """The gated launch: reference counts from the oracle's joint scoring over
    the first 200 edgels, of which path 104 has all and no other path 180."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    E, gate = 200, 0.9
    batch = TripletBatch(problem, [ransac0], seeds=0, samples_per_triplet=1, edgel_counts=[E])
    conv_ids = np.nonzero(run["host"]["converge"])[0]
    counts = np.full((N, 3), -1, np.int32)
    counts[conv_ids] = joint_reference(oracle, run["host"]["tracks"][conv_ids], ransac0.locations[:E],
                                       ransac0.K)["counts"]
    assert counts[FOUND].tolist() == [E, E, E]
    assert np.nonzero(passes_gate(counts[:, 0], np.full(N, E), gate) & (counts[:, 0] >= 0))[0].tolist() == [FOUND]
    case = GroupCase(batch, copy.deepcopy(run["host"]), counts.copy())

    def result():
        r = group_result(run)
        r["joint_inliers"] = counts[:, 0].copy()
        r["stats"]["inliers21"], r["stats"]["inliers31"] = np.maximum(counts[:, 1], 0), np.maximum(counts[:, 2], 0)
        return r

    def check(r, found=[1], expect_ids={FOUND}, g=gate, **kw):
        return check_group_result(r, case, problem.start_sols, gate_score(g), found, expect_ids, **kw)

    assert check(result(), all_tracked=(0,)).all()
    assert check(result(), expect_ids=None).all()
    rejects(check, result(), g=2.0)                    # found a path that does not meet the gate
    r = result()
    r["joint_inliers"][FOUND] -= 1
    rejects(check, r)
    r = result()
    r["stats"]["inliers31"][int(conv_ids[0])] += 1
    rejects(check, r)
    r = result()
    r["batch_index"][FOUND], r["found"][0], r["found_ticks"][0] = -1, 0, 0    # met the gate and was not reported
    rejects(check, r, found=[0], expect_ids=set())
    r = result()
    skip_path(r, problem, 5)
    assert not check(r)[5]
    r["joint_inliers"][5] = 0
    rejects(check, r)


# ---- kernel choice ---------------------------------------------------------------

class Knobs:
    def __init__(self):
        self.calls = []

    def hc_trifocal_set_small_launch(self, v):
        self.calls.append(("small", v))

    def hc_trifocal_set_retry_reuse(self, v):
        self.calls.append(("reuse", v))


def test_launch_mode_restores_both_knobs():
    L = Knobs()
    with launch_mode(L, checks.SMALL_NEVER, reuse=False):
        assert L.calls == [("small", -1), ("reuse", 0)]
    assert L.calls[2:] == [("small", checks.KERNEL_BY_SIZE), ("reuse", 1)]
    L = Knobs()
    with pytest.raises(KeyError):
        with launch_mode(L, checks.SMALL_ALWAYS):
            raise KeyError("inside the block")
    assert L.calls == [("small", 1), ("reuse", 1), ("small", 0), ("reuse", 1)]


def test_scaled_samples(problem, run):
    tgt0 = run["target"][0]
    T, D = checks.scaled_samples(problem, tgt0, (40, 0, 70))
    assert T.dtype == D.dtype == np.float32 and T.shape == D.shape == (3, 34, 2)
    assert np.array_equal(T[1].view(np.uint32), tgt0.view(np.uint32))
    assert np.array_equal(T[0], tgt0 * np.float32(2.0 ** 40)) and np.array_equal(T[2], tgt0 * np.float32(2.0 ** 70))
    assert np.array_equal(D, T - problem.start_params[None])
