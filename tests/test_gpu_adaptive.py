"""GPU tests of the gated launch's adaptive sample limit
(include/adaptive/hc_trifocal_adaptive.h): a scored path lowers its triplet's
limit to the caller's table entry of its joint inlier count, and a sample whose
index within its triplet has reached the limit is not tracked.

Expected values come from code that is pinned to the oracle elsewhere in the
suite, as in test_gpu_gated.py: the plain track() of the same samples for every
tracked path and pose.pose_support_joint_grouped on those plain tracks for every
count.  Which paths a launch skips depends on when the limit came down, so one
checker states what must hold at any timing (check_adaptive) and the cases add
what their inputs make certain.

Facts of the inputs (test_gpu_gated.py): on clean data path 104 of dataset 000
(sample 0) has E of E joint inliers for any prefix of the edgels and no other
candidate of its first 128 samples reaches half; no candidate of dataset 099's
128 samples reaches half its edgels; the noisy fixture's best candidate is path
23612 (sample 75) with 1133 of 5117, the next 697.
"""
import numpy as np
import pytest

import graph_common as G
from checks import GroupCase, check_group_result, gate_score, noisy_data

pytestmark = pytest.mark.gpu

OFF = 2.0            # a ratio > 1 never passes: "limit only"
NEVER = 10 ** 6      # a table entry that lowers no limit of these tests


def Case(problem, tracker, ds, samples, **kw):
    return GroupCase.on_device(problem, tracker, ds, samples, joint=True, **kw)


def Stop(tables):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import AdaptiveStop
    return AdaptiveStop(tables=tables)


def sequential_limit(case, t, table, limit0):
    """The limit a sample-by-sample run of the rule reaches on the plain counts."""
    lim = int(limit0)
    for k, s in enumerate(case.batch.index[t]):
        if k >= lim:
            break
        cj = case.counts[s * 312:(s + 1) * 312, 0]
        cj = cj[cj >= 0]
        if len(cj):
            lim = min(lim, int(table[cj].min()))
    return lim


def check_adaptive(r, case, problem, tables, limit0, found, ratio=OFF, all_tracked=()):
    """What holds for an adaptive result r (host dict) at any timing.  tables:
    the triplets' need tables; limit0: the limits on entry; found: the expected
    flags.  checks.check_group_result gives (i) and the reporting half of (ii):
    every tracked path is the plain launch's with the pose support's counts, every
    other one is untouched (conv = 0, inf = 0, zero stats, joint_inliers -1, the
    start solution), the flags, batch_index and ticks follow the ratio gate.  A
    set flag skips paths as well, so (ii), (iii) and (v) are asserted for the
    triplets whose flag stayed 0.  Returns `tracked`."""
    b = case.batch
    expect_ids = None if any(found) else set()
    trk = check_group_result(r, case, problem.start_sols, gate_score(ratio), list(found), expect_ids,
                             all_tracked=all_tracked)
    limit = r["limit"]
    assert limit.dtype == np.int32 and limit.shape == (b.num_groups,)
    ordinal = np.repeat(b.sample_ordinal, 312)
    ji = r["joint_inliers"]
    for t in range(b.num_groups):
        paths = b.path_index(t)
        # (iv) the final limit: the minimum of the initial one and the entries of the counts written
        written = ji[paths][ji[paths] >= 0]
        expect = min([int(limit0[t])] + [int(v) for v in tables[t][written]])
        assert limit[t] == expect, f"group {t}: limit {limit[t]}, the written counts give {expect}"
        if found[t]:
            continue
        # (ii) a skipped path's sample is at or past the final limit, (iii) every sample before it was tracked
        skipped = paths[~trk[paths]]
        assert (ordinal[skipped] >= limit[t]).all(), f"group {t}: a path below the limit {limit[t]} was skipped"
        assert trk[paths[ordinal[paths] < limit[t]]].all()
        # (v) the device tracks a superset of the sequential run's samples
        assert limit[t] <= sequential_limit(case, t, tables[t], limit0[t])
    return trk


@pytest.fixture(scope="module")
def pair128(problem, tracker):   # cases 3 and 6
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data
    return Case(problem, tracker, [load_ransac_data(0), load_ransac_data(99)], 128, interleave=True)


@pytest.fixture(scope="module")
def half_tables(pair128):
    """need[c] = 4 from half the edgels on, no limit below."""
    return [np.where(2 * np.arange(E + 1) >= E, 4, NEVER).astype(np.int32) for E in pair128.batch.edgel_counts]


@pytest.fixture(scope="module")
def prefix_case(problem, tracker, ransac0):   # cases 4 and 7
    return Case(problem, tracker, [ransac0, ransac0], 8, edgel_counts=[33, 65])


def prefix_tables():
    tabs = [np.full(34, NEVER, np.int32), np.full(66, NEVER, np.int32)]
    tabs[0][33], tabs[1][65] = 2, 5
    return tabs


def test_nothing_lowers(problem, tracker, ransac0):
    """Case 1: tables that never lower, ratio off: everything is tracked, the
    counts are the pose support's and the limit is the budget."""
    c = Case(problem, tracker, [ransac0], 8)
    tabs = [np.full(5118, NEVER, np.int32)]
    r = tracker.track_grouped(c.dev, adaptive=Stop(tabs)).host()
    trk = check_adaptive(r, c, problem, tabs, [8], [0], all_tracked=(0,))
    assert trk.all() and trk.shape == (2496,)
    assert np.array_equal(r["joint_inliers"], c.counts[:, 0]) and (c.counts[:, 0] >= 0).any()
    assert r["limit"].tolist() == [8] and (r["batch_index"] == -1).all()


def test_preset_limit_carries_over(problem, tracker):
    """Case 2: limit = [3, 8] on entry, tables that never lower: exactly group
    0's samples 0..2 and all of group 1 are tracked."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data
    c = Case(problem, tracker, [load_ransac_data(0), load_ransac_data(99)], 8, interleave=True)
    assert c.batch.sample_group.tolist() == [s % 2 for s in range(16)]
    assert c.batch.sample_ordinal.tolist() == [s // 2 for s in range(16)]
    tabs = [np.full(E + 1, NEVER, np.int32) for E in c.batch.edgel_counts]
    r = tracker.track_grouped(c.dev, adaptive=Stop(tabs), limit=[3, 8]).host()
    trk = check_adaptive(r, c, problem, tabs, [3, 8], [0, 0], all_tracked=(1,))
    expect = np.repeat((c.batch.sample_group == 1) | (c.batch.sample_ordinal < 3), 312)
    assert np.array_equal(trk, expect) and trk.sum() == (3 + 8) * 312
    assert r["limit"].tolist() == [3, 8]


@pytest.mark.parametrize("inflight_stop", [0, 1])
def test_lowering_is_per_group(problem, tracker, pair128, half_tables, inflight_stop):
    """Case 3: path 104 (5117 of 5117) lowers group 0's limit to 4; group 1
    keeps its budget and is tracked in full; no flag is raised."""
    c = pair128
    assert c.counts[104].tolist() == [5117, 5117, 5117]
    r = tracker.track_grouped(c.dev, inflight_stop=bool(inflight_stop), adaptive=Stop(half_tables)).host()
    trk = check_adaptive(r, c, problem, half_tables, [128, 128], [0, 0], all_tracked=(1,))
    assert r["limit"].tolist() == [4, 128]
    assert r["found"].tolist() == [0, 0] and (r["batch_index"] == -1).all()
    assert trk[c.batch.path_index(1)].sum() == 39936
    assert (~trk[c.batch.path_index(0)]).any(), "no path of the lowered group was skipped"


def test_per_group_table_offsets(problem, tracker, prefix_case):
    """Case 4: two triplets over dataset 000 scored on its first 33 and 65
    edgels; path 104 of each counts E of E, and only need[E] lowers: 2 and 5.
    An offset off by one entry, or the other group's table, gives another limit."""
    c = prefix_case
    assert c.batch.edgel_counts.tolist() == [33, 65]
    assert c.counts[104].tolist() == [33] * 3 and c.counts[8 * 312 + 104].tolist() == [65] * 3
    tabs = prefix_tables()
    r = tracker.track_grouped(c.dev, inflight_stop=True, adaptive=Stop(tabs)).host()
    check_adaptive(r, c, problem, tabs, [8, 8], [0, 0])
    assert r["limit"].tolist() == [2, 5]


def test_real_table_on_the_noisy_fixture(problem, tracker):
    """Case 5: 100 samples at confidence 0.5, capped at the budget: the winner
    (path 23612, sample 75, 1133 of 5117) is the only candidate whose entry is
    below 100, so the final limit is that entry, and since nothing lowers the
    limit before it is scored, all of samples 0..75 are tracked."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import AdaptiveStop, need_table
    c = Case(problem, tracker, [noisy_data()], 100)
    stop = AdaptiveStop(confidence=0.5)
    table = need_table(5117, 0.5, 1, 100)
    assert np.array_equal(stop.host_tables(c.batch.edgel_counts, [100])[0], table)
    cj = c.counts[:, 0]
    assert cj[23612] == 1133 and np.sort(cj)[-2] == 697
    assert table[1133] < 76 and table[697] == 100 and (table[cj[cj >= 0]] < 100).sum() == 1
    r = tracker.track_grouped(c.dev, adaptive=stop).host()
    trk = check_adaptive(r, c, problem, [table], [100], [0])
    assert r["limit"].tolist() == [int(table[1133])]
    assert trk[:76 * 312].all() and r["joint_inliers"][23612] == 1133


def test_ratio_and_limit_together(problem, tracker, pair128, half_tables):
    """Case 6: case 3's data with ratio 0.5: path 104 raises its triplet's flag
    as in the gated launch and still lowers the limit to 4."""
    c = pair128
    r = tracker.track_grouped(c.dev, gate=0.5, adaptive=Stop(half_tables)).host()
    check_adaptive(r, c, problem, half_tables, [128, 128], [1, 0], ratio=0.5, all_tracked=(1,))
    assert r["found"].tolist() == [1, 0] and r["batch_index"][104] == 104
    assert r["limit"].tolist() == [4, 128]


def test_graph_capture_and_replay(problem, tracker, prefix_case):
    """Case 7: the adaptive mode recorded with tests/graph_common.py; the
    limits are restored by a copy node inside the graph (from [6, 8], so that
    group 0's samples 6 and 7 are skipped at any timing), every other in/out
    buffer by reset_tracks, and both replays satisfy the checker."""
    import torch
    c = prefix_case
    tabs = prefix_tables()
    stop = Stop(tabs)
    dev = c.dev
    stop.prepare(dev)                      # the tables' device copies, outside the capture
    r = tracker.allocate_grouped(dev, adaptive=True)
    limit0 = torch.tensor([6, 8], dtype=torch.int32, device=tracker.device)
    ws = tracker.new_workspace()

    def enqueue():
        tracker.reset_tracks(r)
        r.limit.copy_(limit0)
        tracker.launch_grouped(dev, r, workspace=ws, inflight_stop=True, adaptive=stop)

    cap, _ = G.capture(enqueue)
    try:
        for _ in range(2):
            G.poison(r.tracks, r.converge, r.infinity, r.stats, r.found, r.batch_index, r.found_ticks,
                     r.joint_inliers, r.limit)
            cap.replay()
            torch.cuda.synchronize()
            tracker.workspace_status(ws)
            h = r.host()
            trk = check_adaptive(h, c, problem, tabs, [6, 8], [0, 0])
            assert h["limit"].tolist() == [2, 5]
            assert not trk[6 * 312:8 * 312].any() and trk[:2 * 312].all()
    finally:
        G.release(cap)
