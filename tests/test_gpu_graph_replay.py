"""Graph capture and replay of every entry point that takes a stream.

include/hc_trifocal.h: the entry points "never allocate, copy to/from the host
or synchronise (hipGraph-capturable)".  Every case here records a launch under
torch.cuda.graph (tests/graph_common.py: one stream, the default "global" error
mode, which fails on any such host call) and replays it at least three times:
on data set A, on data set B written into the same device buffers, and on A
again.  Between replays only device buffer contents change, so whatever a launch
decides on the host is frozen into the graph, and whatever it must redo per
launch -- the control-block reset, the index-table hash check, the ring reset
and epoch, the found flags and timestamps, the cleared selection keys -- has to
be done by the recorded device work.  Pure outputs are poisoned before every
replay; in/out buffers are reset by nodes of the graph.

The comparisons are the suite's exact ones: the oracle, the committed golden
runs, the checkers of tests/checks.py, and byte equality with the eager call.

CAPTURED lists the entry points recorded here; tests/test_graph_coverage_host.py
holds it (with a short list of blocking test hooks) against the headers.
"""
import contextlib
import copy

import numpy as np
import pytest

import graph_common as G
import p2c_common as pc
import refine_reference as RR
from checks import (NOISE_SEED, SMALL_NEVER, GroupCase, assert_matches_golden, assert_matches_oracle,
                    assert_untouched, check_group_result, found_ids, gate_score, golden, golden_passing,
                    launch_mode, noisy_data, oracle_score, ring_counters, ring_epoch, tracked)
from p2c_common import p2c_ref

pytestmark = pytest.mark.gpu

# Every prototype under include/ with an hcStream parameter that a case below records
CAPTURED = (
    "hc_trifocal_2op1p_30x30_track",
    "hc_trifocal_2op1p_30x30_track_abort",
    "hc_trifocal_2op1p_30x30_track_abort_grouped",
    "hc_trifocal_2op1p_30x30_track_abort_gated",
    "hc_trifocal_2op1p_30x30_track_ph_codeopt",
    "hc_trifocal_2op1p_30x30_track_ph",
    "hc_trifocal_2op1p_30x30_track_p2c",
    "hc_shared_flag_reset",
    "hc_cgesv_30x30_batched",
    "hc_trifocal_eval_batched",
    "hc_trifocal_p2c_eval_batched",
    "hc_trifocal_pose_support",
    "hc_trifocal_pose_support_grouped",
    "hc_trifocal_pose_support_joint",
    "hc_trifocal_pose_support_joint_grouped",
    "hc_trifocal_pose_inlier_mask",
    "hc_trifocal_pose_refine",
    "hc_trifocal_pose_refine_grouped",
    "hc_trifocal_pose_topk_joint",
    "hc_trifocal_pose_topk_joint_grouped",
    "hc_trifocal_pose_refine_topk",
    "hc_trifocal_pose_refine_topk_grouped",
)
RECORDED_BY = {}   # entry point -> the tests that record it (filled by @records at import)
REPLAYS = ("A", "B", "A")


def records(*names):
    """Marks a test with the entry points its graph records."""
    def mark(fn):
        for n in names:
            assert n in CAPTURED, n
            RECORDED_BY.setdefault(n, []).append(fn.__name__)
        return fn
    return mark


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _sync():
    import torch
    torch.cuda.synchronize()


@contextlib.contextmanager
def recorded(enqueue, mode=None):
    """capture(enqueue), with the kernel-choice hook set around the recording
    only, and the graph destroyed after a synchronisation."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    with (launch_mode(_abi.lib(), mode) if mode is not None else contextlib.nullcontext()):
        cap, out = G.capture(enqueue)
    try:
        yield cap, out
    finally:
        G.release(cap)


# ---- tracking --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ab2(samples100):
    """A: samples 0-1 of samples100, B: samples 2-3 (target, diff)."""
    tgt, dif, _ = samples100
    return {"A": (tgt[0:2], dif[0:2]), "B": (tgt[2:4], dif[2:4])}


@pytest.fixture(scope="module")
def oracle_ab(problem, oracle, ab2):
    """The oracle's run of A and of B at given settings, computed once each."""
    cache = {}

    def ref(which, **kw):
        key = (which, tuple(sorted(kw.items())))
        if key not in cache:
            t, d = ab2[which]
            cache[key] = oracle.gpuhc_track(problem.start_sols, problem.start_params, t, d, problem.unified_index,
                                            oracle.settings(**kw))
            for v in cache[key]:
                v.setflags(write=False)
        return cache[key]
    return ref


def _replay_tracking(tracker, sets, ws, check, mode=None, abort=False, **launch_kw):
    """Records reset_tracks + one launch on workspace ws over buffers that hold
    sets["A"], then replays on A, B, A: check(which, replay number, host result)."""
    first = sets["A"]
    dev = tracker.device
    tgt, dif = _dev(first[0], dev), _dev(first[1], dev)
    r = tracker.allocate(first[0].shape[0], abort=abort)

    def enqueue():
        tracker.reset_tracks(r)
        tracker.launch(tgt, dif, r, abort=abort, workspace=ws, **launch_kw)

    with recorded(enqueue, mode) as (cap, _):
        for i, which in enumerate(REPLAYS):
            G.load(tgt, sets[which][0])
            G.load(dif, sets[which][1])
            # the in/out buffers too: their reset is part of the graph
            G.poison(r.tracks, r.converge, r.infinity, r.stats, r.found, r.batch_index)
            cap.replay()
            _sync()
            tracker.workspace_status(ws)
            check(which, i + 1, r.host())


@records("hc_trifocal_2op1p_30x30_track")
def test_tracking_latency_kernel(tracker, ab2, oracle_ab):
    """N = 2 (624 paths): the launcher picks the latency kernel by size."""
    def check(which, i, r):
        assert_matches_oracle(r, oracle_ab(which))
        assert (r["tracks"][:, 30, 0] == 1.0).all()
    _replay_tracking(tracker, ab2, tracker.new_workspace(2), check)


@records("hc_trifocal_2op1p_30x30_track")
def test_tracking_throughput_kernel_unsliced(tracker, ab2, oracle_ab):
    """N = 2 on the throughput kernel (the hook is read when the launch is
    recorded and is back at its default during the replays), in a workspace of
    the minimum size: no time slicing."""
    ws = tracker.new_workspace()
    assert ws.numel() == int(tracker.L.hc_trifocal_workspace_size())

    def check(which, i, r):
        assert_matches_oracle(r, oracle_ab(which))
    _replay_tracking(tracker, ab2, ws, check, mode=SMALL_NEVER)


@pytest.fixture(scope="module")
def heldout010(problem):
    """Held-out dataset 010 as test_heldout_dataset_matches_golden_N100 prepares it."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data, prepare_target_params
    g = golden("gpuhc_ds010_N100_seed0")
    tgt, dif, picked = prepare_target_params(problem, load_ransac_data(10), seed=0, num_samples=100)
    assert np.array_equal(picked, g["picked"]) and np.array_equal(tgt, g["target"]) and np.array_equal(dif, g["diff"])
    return tgt, dif, g


@records("hc_trifocal_2op1p_30x30_track")
def test_tracking_throughput_kernel_time_sliced(tracker, samples100, heldout010):
    """N = 100 with time slicing: the ring is reset and drained and its epoch
    bumped by the recorded k_prep_tables at every replay."""
    tgt, dif, _ = samples100
    sets = {"A": (tgt, dif), "B": heldout010[:2]}
    gold = {"A": golden("gpuhc_N100_seed0"), "B": heldout010[2]}
    ws = tracker.new_workspace(100)
    assert ring_epoch(tracker, ws) == 0

    def check(which, i, r):
        assert_matches_golden(r, gold[which])
        head, tail, avail = ring_counters(tracker, ws)
        assert tail > 0 and head == tail and avail == 0, (head, tail, avail)
        assert ring_epoch(tracker, ws) == 1 + i      # 1: the warm-up run; recording a launch runs nothing
    _replay_tracking(tracker, sets, ws, check)


def _samples_reversed(n):
    """Path ids of a launch whose n samples are in reverse order."""
    b = np.arange(312 * n)
    return (n - 1 - b // 312) * 312 + b % 312


@pytest.mark.parametrize("inflight_stop", [0, 1])
@records("hc_trifocal_2op1p_30x30_track_abort")
def test_abort_mode(problem, tracker, samples100, inflight_stop):
    """Abort mode at N = 100, checked as test_tracker_abort_mode checks it; B is
    A's samples in reverse order, so its abort-off run is the golden run with
    its rows permuted.  The device clock shows that each replay reset the
    control block: its start is later than the previous replay's, and its find
    is later than its own start (a leftover t_found would be earlier)."""
    tgt, dif, _ = samples100
    g = golden("gpuhc_N100_seed0")
    src = _samples_reversed(100)
    gold = {"A": {k: g[k] for k in ("conv", "inf", "steps", "corrections", "hash")}}
    gold["B"] = {k: v[src] for k, v in gold["A"].items()}
    passing = {"A": golden_passing(g)}
    passing["B"] = set(int(src[b]) for b in passing["A"])      # the permutation is its own inverse
    assert passing["A"]
    sets = {"A": (tgt, dif), "B": (tgt[::-1].copy(), dif[::-1].copy())}
    ws = tracker.new_workspace()
    starts = []

    def check(which, i, r):
        assert r["found"]
        found = set(found_ids(r).tolist())
        assert found and found <= passing[which]
        assert (gold[which]["conv"][sorted(found)] == 1).all()
        trk = tracked(r)
        assert_matches_golden(r, gold[which], where=trk)
        assert_untouched(r, problem.start_sols, ~trk, allow_empty=True)
        start, found_ticks, hz = tracker.read_timestamps(ws)
        assert hz > 0 and start > 0
        if starts:
            assert start > starts[-1], (start, starts)
        assert found_ticks > start, (found_ticks, start)
        starts.append(start)
    _replay_tracking(tracker, sets, ws, check, abort=True, inflight_stop=bool(inflight_stop))
    assert len(starts) == 3


# ---- grouped and gated abort ---------------------------------------------------------------------

def _reversed_within_groups(case):
    """case with every triplet's samples in reverse order (the batch is
    triplet-major, so sample_group stays as it is): the GroupCase of data set B
    and the path ids it takes from A."""
    b = case.batch
    src = np.arange(b.num_samples)
    for idx in b.index:
        src[idx] = idx[::-1]
    assert np.array_equal(b.sample_group[src], b.sample_group)
    rb = copy.copy(b)
    rb.target, rb.diff, rb.picked = (np.ascontiguousarray(v[src]) for v in (b.target, b.diff, b.picked))
    paths = (src[:, None] * 312 + np.arange(312)[None, :]).reshape(-1)
    plain = {k: v[paths].copy() for k, v in case.plain.items()}
    counts = None if case.counts is None else case.counts[paths].copy()
    return GroupCase(rb, plain, counts), paths


def _grouped_enqueue(tracker, case_dev, r, reset_found, workspace, **kw):
    def enqueue():
        if reset_found:
            tracker.reset_tracks(r)
        else:   # reset_tracks without the flags: they carry over from replay to replay
            n = r.tracks.shape[0] // 312
            r.tracks.view(n, 312, 31, 2).copy_(tracker.start_sols.unsqueeze(0).expand(n, -1, -1, -1))
            r.batch_index.fill_(-1)
            r.found_ticks.zero_()
        tracker.launch_grouped(case_dev, r, workspace=workspace, **kw)
    return enqueue


@pytest.fixture(scope="module")
def small_case(problem, tracker):
    """The small_case of test_gpu_grouped.py: 4 triplets x 8 samples; 000 finds
    at path 104, 050 (first 1000 edgels) at sample 18 track 52, 099 and 001 never."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data
    ds = [load_ransac_data(i) for i in (0, 99, 50, 1)]
    return GroupCase.on_device(problem, tracker, ds, 8, edgel_counts=[None, None, 1000, None])


@records("hc_trifocal_2op1p_30x30_track_abort_grouped")
def test_grouped_abort(problem, oracle, tracker, small_case):
    """The flags, ticks and batch index are reset by the graph: every replay is a fresh run."""
    case_b, paths = _reversed_within_groups(small_case)
    cases = {"A": small_case, "B": case_b}
    ids_a = {104, 18 * 312 + 52}
    ids = {"A": ids_a, "B": {int(np.nonzero(paths == b)[0][0]) for b in ids_a}}
    assert ids["B"] == {7 * 312 + 104, 21 * 312 + 52}
    dev = small_case.dev
    r = tracker.allocate_grouped(dev)
    ws = tracker.new_workspace()
    try:
        with recorded(_grouped_enqueue(tracker, dev, r, True, ws)) as (cap, _):
            for which in REPLAYS:
                G.load(dev.target, cases[which].batch.target)
                G.load(dev.diff, cases[which].batch.diff)
                G.poison(r.tracks, r.converge, r.infinity, r.stats, r.found, r.batch_index, r.found_ticks)
                cap.replay()
                _sync()
                tracker.workspace_status(ws)
                h = r.host()
                check_group_result(h, cases[which], problem.start_sols, oracle_score(oracle), [1, 0, 1, 0],
                                   ids[which], all_tracked=(1, 3))
                start = tracker.read_timestamps(ws)[0]
                assert start > 0 and (h["found_ticks"][[0, 2]] >= start).all()
    finally:   # the fixture's device copy is shared
        G.load(dev.target, small_case.batch.target)
        G.load(dev.diff, small_case.batch.diff)


@records("hc_trifocal_2op1p_30x30_track_abort_grouped")
def test_grouped_abort_flags_carry_over_between_replays(problem, oracle, tracker, small_case):
    """A graph without the reset of `found`: the replay after a finding one
    skips every path of the triplets found before (tracks untouched, converge
    0), as test_abort_grouped_carry_over pins eagerly -- the flags are read on
    the device at replay."""
    dev = small_case.dev
    r = tracker.allocate_grouped(dev)
    ws = tracker.new_workspace()
    score = oracle_score(oracle)
    with recorded(_grouped_enqueue(tracker, dev, r, False, ws)) as (cap, _):
        for fresh in (True, False, True):
            if fresh:
                r.found.zero_()                      # from outside the graph
            G.poison(r.tracks, r.converge, r.infinity, r.stats, r.batch_index, r.found_ticks)
            cap.replay()
            _sync()
            tracker.workspace_status(ws)
            h = r.host()
            if fresh:
                check_group_result(h, small_case, problem.start_sols, score, [1, 0, 1, 0], {104, 18 * 312 + 52},
                                   all_tracked=(1, 3))
            else:
                trk = check_group_result(h, small_case, problem.start_sols, score, [1, 0, 1, 0], set(),
                                         all_tracked=(1, 3), none_tracked=(0, 2), tick_groups=[])
                assert trk.sum() == 2 * 2496


@records("hc_trifocal_2op1p_30x30_track_abort_gated")
def test_gated_abort(problem, tracker, ransac0):
    """The gated launch on the 8-sample clean case scored on 33 edgels, gate 1.0:
    path 104 counts 33 of 33 and stops its triplet."""
    case_a = GroupCase.on_device(problem, tracker, [ransac0], 8, edgel_counts=[33], joint=True)
    case_b, paths = _reversed_within_groups(case_a)
    cases = {"A": case_a, "B": case_b}
    hit = {"A": 104, "B": 7 * 312 + 104}
    assert paths[hit["B"]] == 104 and case_a.counts[104].tolist() == [33, 33, 33]
    dev = case_a.dev
    r = tracker.allocate_grouped(dev, gate=True)
    ws = tracker.new_workspace()
    with recorded(_grouped_enqueue(tracker, dev, r, True, ws, gate=1.0)) as (cap, _):
        for which in REPLAYS:
            G.load(dev.target, cases[which].batch.target)
            G.load(dev.diff, cases[which].batch.diff)
            G.poison(r.tracks, r.converge, r.infinity, r.stats, r.found, r.batch_index, r.found_ticks,
                     r.joint_inliers)
            cap.replay()
            _sync()
            tracker.workspace_status(ws)
            h = r.host()
            check_group_result(h, cases[which], problem.start_sols, gate_score(1.0), [1], None)
            assert h["batch_index"][hit[which]] == hit[which] and h["joint_inliers"][hit[which]] == 33


# ---- archived kernels ------------------------------------------------------------------------------

@pytest.mark.parametrize("entry,kw", [("hc_trifocal_2op1p_30x30_track_ph_codeopt", dict(truncate=False)),
                                      ("hc_trifocal_2op1p_30x30_track_ph", dict(truncate=False, explicit_rk=True))],
                         ids=["ph_codeopt", "ph"])
@records("hc_trifocal_2op1p_30x30_track_ph_codeopt", "hc_trifocal_2op1p_30x30_track_ph")
def test_archived_ph_kernels(tracker, ab2, oracle_ab, entry, kw):
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import _TRACK_ENTRY
    assert _TRACK_ENTRY[False, kw["truncate"], kw.get("explicit_rk", False)] == entry

    def check(which, i, r):
        assert_matches_oracle(r, oracle_ab(which, **kw))
    _replay_tracking(tracker, ab2, tracker.new_workspace(), check, **kw)


@records("hc_trifocal_2op1p_30x30_track_p2c")
def test_archived_p2c_kernel(problem, tracker):
    """launch_p2c at N = 2 against the restatement: A is samples 0-1, B samples 2-3."""
    hx, ht = pc.fixture_tables()
    chx, cht = pc.blocks(4)
    sets = {"A": (chx[0:2], cht[0:2]), "B": (chx[2:4], cht[2:4])}
    assert np.array_equal(chx[0:2], pc.blocks(2)[0]) and np.array_equal(cht[0:2], pc.blocks(2)[1])
    refs = {"A": pc.ref_track(2), "B": p2c_ref.track(problem.start_sols, hx, ht, chx[2:4], cht[2:4])}
    dev = tracker.device
    tables = tracker.p2c_tables((hx, ht))
    bx, bt = _dev(sets["A"][0], dev), _dev(sets["A"][1], dev)
    r = tracker.allocate(2)
    ws = tracker.new_workspace()

    def enqueue():
        tracker.reset_tracks(r)
        tracker.launch_p2c(tables, bx, bt, r, workspace=ws)

    with recorded(enqueue) as (cap, _):
        for which in REPLAYS:
            G.load(bx, sets[which][0])
            G.load(bt, sets[which][1])
            G.poison(r.tracks, r.converge, r.infinity, r.stats)
            cap.replay()
            _sync()
            tracker.workspace_status(ws)
            assert_matches_oracle(r.host(), refs[which])


# ---- the documented chain in one graph ---------------------------------------------------------------

@records("hc_trifocal_2op1p_30x30_track", "hc_trifocal_pose_support_joint", "hc_trifocal_pose_topk_joint",
         "hc_trifocal_pose_refine_topk")
def test_chain_track_joint_topk_refine(problem, tracker):
    """INTEGRATION.md's chain as one graph: reset_tracks, the tracking launch
    (N = 100, sigma = 1 px noisy data), joint pose support, top-8, refine and
    select.  A is the noise seed of the committed goldens, B the seed of trial
    12 with its samples, srand(12) (both scenes have 5117 edgels, so the recorded
    edgel count fits both).
    Every replay equals the eager run of the same calls on the same data byte
    for byte; A also matches the goldens, B shows what test_trial12_is_repaired
    asserts of that scene."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose, prepare_target_params
    dev = tracker.device
    k = 8
    data = {"A": noisy_data(NOISE_SEED), "B": noisy_data(NOISE_SEED + 12)}
    sets = {}
    for which, d in data.items():
        tgt, dif, _ = prepare_target_params(problem, d, seed=0 if which == "A" else 12, num_samples=100)
        assert d.locations.shape == (5117, 6)
        sets[which] = (tgt, dif, np.array(d.locations))
    assert np.array_equal(data["A"].K, data["B"].K)
    tgt, dif, edgels = (_dev(v, dev) for v in sets["A"])
    K = _dev(data["A"].K, dev)
    r = tracker.allocate(100)
    ws = tracker.new_workspace(100)
    inl = torch.empty((31200, 3), dtype=torch.int32, device=dev)
    sel = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    cand = torch.empty(k * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    refined = torch.empty(k * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)

    def enqueue():
        tracker.reset_tracks(r)
        tracker.launch(tgt, dif, r, workspace=ws)
        pose.launch_pose_support_joint(r.tracks, r.converge, edgels, K, inl, sel)
        pose.launch_topk_joint(r.tracks, inl, k, candidates=cand)
        return pose.launch_refine_topk(cand, edgels, K, refined=refined)     # best, best_rank, refined, reports

    def put(which):
        for dst, src in zip((tgt, dif, edgels), sets[which]):
            G.load(dst, src)

    def snapshot(out):
        best, rank, ref, reports = out
        assert ref.data_ptr() == refined.data_ptr()
        return dict(tracks=G.raw(r.tracks), converge=G.raw(r.converge), infinity=G.raw(r.infinity),
                    stats=G.raw(r.stats), counts=G.raw(inl), joint=G.raw(sel), candidates=G.raw(cand),
                    refined=G.raw(ref), reports=G.raw(reports), best=G.raw(best), best_rank=G.raw(rank))

    eager = {}
    for which in ("B", "A"):
        put(which)
        out = enqueue()
        _sync()
        eager[which] = snapshot(out)
    with recorded(enqueue) as (cap, out):
        for which in REPLAYS:
            put(which)
            G.poison(r.tracks, r.converge, r.infinity, r.stats, inl, sel, cand, out)
            cap.replay()
            _sync()
            tracker.workspace_status(ws)
            got = snapshot(out)
            for key, exp in eager[which].items():
                assert got[key] == exp, f"replay on {which}: {key} differs from the eager run"
            h = r.host()
            joint = pose.joint_selection_dict(pose.joint_selection_struct(sel))
            best, rank, ref, reports = out
            rank = int(rank.cpu().numpy()[0])
            dicts = pose._selection_dicts(ref, k)
            best_d = pose.joint_selection_dict(pose.joint_selection_struct(best))
            assert G.raw(best) == G.raw(ref)[rank * pose.JOINT_SEL_BYTES:(rank + 1) * pose.JOINT_SEL_BYTES]
            if which == "A":
                assert_matches_golden(h, golden("gpuhc_noisy1px_N100"))
                g = golden("pose_joint_noisy1px_N100")
                assert np.array_equal(inl.cpu().numpy()[g["cand_ids"]], g["counts"])
                assert (joint["num_candidates"], joint["path"], joint["key"]) == (31, int(g["path"]), int(g["key"]))
                assert [joint["inliers"], joint["inliers21"], joint["inliers31"]] == g["inliers"].tolist()
                assert dicts[0]["path"] == int(g["path"])
            else:
                g = golden("pose_topk_noisy1px_trial12_N100")
                assert np.array_equal(inl.cpu().numpy()[g["cand_ids"]], g["counts"])
                assert (joint["path"], joint["inliers"], joint["num_candidates"]) == (29311, 644, 35)
                assert [d["path"] for d in dicts[:4]] == [29311, 15336, 3607, 20328]
                assert not pose.residuals(data["B"], dicts[0])[1]      # the joint winner stays in its wrong basin
                res, ok = pose.residuals(data["B"], dicts[2])          # the third-ranked candidate is repaired
                assert ok and res[0] < 0.1 and res[1] < 0.1
                assert abs(dicts[2]["inliers"] - int(g["ref_counts"][2, 0])) <= int(g["borderline"][2])
                # with k = 8 the right-basin candidates at ranks 2, 4 and 6 are closer than their
                # borderline edgels (test_trial12_against_the_reference): one of them wins
                res, ok = pose.residuals(data["B"], best_d)
                assert rank in (2, 4, 6) and ok and res[0] < 0.1 and res[1] < 0.1


# ---- the remaining stream entry points: two data sets in place, byte equality with the eager call ------

@pytest.fixture(scope="module")
def pose_inputs(tracker):
    """The 36 candidate tracks of pose_N100_seed0 at scattered ids of 624 paths
    (the inputs of test_gpu_pose_joint.py) and 200 noisy edgels; A lets the
    even-numbered candidates converge, B the odd-numbered ones."""
    dev = tracker.device
    cand = np.ascontiguousarray(golden("pose_N100_seed0")["cand_tracks"])
    ids = np.sort(np.random.default_rng(11).choice(624, len(cand), replace=False))
    tr = np.zeros((624, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    tr[ids] = cand
    conv = {"A": np.zeros(624, np.uint8), "B": np.zeros(624, np.uint8)}
    conv["A"][ids[0::2]] = 1
    conv["B"][ids[1::2]] = 1
    noisy0 = noisy_data()
    return dict(tracks=_dev(tr, dev), conv=conv, edgels=_dev(np.array(noisy0.locations[:200]), dev),
                K=_dev(noisy0.K, dev), noisy0=noisy0)


@pytest.fixture(scope="module")
def two_triplets(problem, tracker, pose_inputs):
    """A 2-triplet batch of one sample each (624 paths): 63 and 200 noisy edgels of two noise seeds."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    batch = TripletBatch(problem, [pose_inputs["noisy0"], noisy_data(20250216)], seeds=0, samples_per_triplet=1,
                         edgel_counts=[63, 200])
    assert batch.sample_group.tolist() == [0, 1]
    return batch.to(tracker.device)


def _replay_against_eager(enqueue, put, outputs, eager):
    """Records enqueue() and replays on A, B, A: after put(which), the bytes of
    outputs() equal eager(which), computed by the eager call on fresh buffers
    before anything is recorded."""
    exp = {}
    for which in ("A", "B"):
        put(which)
        exp[which] = eager(which)
    assert exp["A"] != exp["B"], "the two data sets give the same bytes: a replay that did nothing could pass"
    put("A")
    with recorded(enqueue) as (cap, out):
        for which in REPLAYS:
            put(which)
            G.poison(outputs(out))
            cap.replay()
            _sync()
            got = [G.raw(t) for t in outputs(out)]
            assert got == exp[which], f"replay on {which} differs from the eager call"


@pytest.mark.parametrize("quirks", [False, True], ids=["plain", "quirks"])
@records("hc_trifocal_pose_support")
def test_pose_support(pose_inputs, quirks):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    d = pose_inputs
    dev = d["tracks"].device
    conv = _dev(d["conv"]["A"], dev)
    inl = torch.empty((624, 2), dtype=torch.int32, device=dev)
    sel = torch.empty(pose.SEL_BYTES, dtype=torch.uint8, device=dev)

    def eager(which):
        i, _, s = pose._run(pose._PER_VIEW, d["tracks"], conv, (d["edgels"], d["K"]),
                            _abi.HC_POSE_REFERENCE_QUIRKS if quirks else 0)
        return [i.tobytes(), G.raw(s)]
    _replay_against_eager(lambda: pose.launch_pose_support(d["tracks"], conv, d["edgels"], d["K"], inl, sel, quirks),
                          lambda which: G.load(conv, d["conv"][which]), lambda out: (inl, sel), eager)


@records("hc_trifocal_pose_support_grouped")
def test_pose_support_grouped(pose_inputs, two_triplets):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = pose_inputs
    dev = d["tracks"].device
    conv = _dev(d["conv"]["A"], dev)
    inl = torch.empty((624, 2), dtype=torch.int32, device=dev)
    sels = torch.empty(2 * pose.SEL_BYTES, dtype=torch.uint8, device=dev)

    def eager(which):
        i, _, s = pose._run(pose._PER_VIEW, d["tracks"], conv, two_triplets)
        return [i.tobytes(), G.raw(s)]
    _replay_against_eager(lambda: pose.launch_pose_support_grouped(d["tracks"], conv, two_triplets, inl, sels),
                          lambda which: G.load(conv, d["conv"][which]), lambda out: (inl, sels), eager)


@records("hc_trifocal_pose_support_joint_grouped", "hc_trifocal_pose_topk_joint_grouped",
         "hc_trifocal_pose_refine_topk_grouped")
def test_grouped_joint_topk_refine(pose_inputs, two_triplets):
    """The grouped chain on the 2-triplet batch in one graph: joint support,
    top-4 per triplet, refine and select per triplet."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    d = pose_inputs
    dev = d["tracks"].device
    k = 4
    conv = _dev(d["conv"]["A"], dev)

    def buffers():
        return (torch.empty((624, 3), dtype=torch.int32, device=dev),
                torch.empty(2 * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev),
                torch.empty(2 * k * pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev))

    def chain(inl, sels, cand):
        pose.launch_pose_support_joint_grouped(d["tracks"], conv, two_triplets, inl, sels)
        pose.launch_topk_joint_grouped(d["tracks"], inl, two_triplets, k, candidates=cand)
        return (inl, sels, cand) + tuple(pose.launch_refine_topk_grouped(cand, two_triplets, k))

    def eager(which):
        out = chain(*buffers())
        _sync()
        return [G.raw(t) for t in out]
    mine = buffers()
    _replay_against_eager(lambda: chain(*mine), lambda which: G.load(conv, d["conv"][which]), lambda out: out, eager)


def _selection(pose32, loc, K, path, num_candidates, scale31):
    """A joint selection of the given pose with the counts it has on the scene
    (as tests/test_gpu_refine.py builds its inputs)."""
    m21, m31 = RR.score(loc, K, tuple(pose32[k] for k in RR.POSE_KEYS))
    cJ = int((m21 & m31).sum())
    d = dict(num_candidates=num_candidates, path=path, inliers=cJ, inliers21=int(m21.sum()),
             inliers31=int(m31.sum()), key=(cJ << 32) | path, scale31=np.float32(scale31))
    d.update({k: np.asarray(pose32[k], np.float32) for k in RR.POSE_KEYS})
    return d


@pytest.fixture(scope="module")
def clean33(tracker, ransac0):
    """The clean scene of test_gpu_refine.py at E = 33: the GT pose of dataset
    000 turned by 3e-4 rad (A) and by 2e-4 rad (B), as joint selections."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    E = 33
    loc = np.ascontiguousarray(ransac0.locations[:E])
    sels = {}
    for which, angle, path in (("A", 3e-4, 23612), ("B", 2e-4, 777)):
        s = _selection(RR.perturbed(RR.gt_pose(ransac0), angle), loc, ransac0.K, path, 31, 1.75)
        assert s["inliers"] == E
        sels[which] = np.frombuffer(bytes(pose.joint_selection_from_dict(s)), np.uint8).copy()
    return dict(E=E, edgels=_dev(loc, dev), K=_dev(ransac0.K, dev), sels=sels, data=ransac0)


@records("hc_trifocal_pose_refine")
def test_refine_joint_in_place(clean33):
    """launch_refine_joint with out aliasing selection: the selection buffer is
    in/out, reloaded from outside the graph before every replay."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c = clean33
    dev = c["edgels"].device
    sel = _dev(c["sels"]["A"], dev)

    def enqueue():
        out, report = pose.launch_refine_joint(sel, c["edgels"], c["K"], out=sel)
        assert out.data_ptr() == sel.data_ptr()
        return out, report

    def eager(which):
        out, report = pose.launch_refine_joint(_dev(c["sels"][which], dev), c["edgels"], c["K"])
        _sync()
        return [G.raw(out), G.raw(report)]
    exp = {w: eager(w) for w in ("A", "B")}
    assert exp["A"] != exp["B"]
    with recorded(enqueue) as (cap, out):
        for which in REPLAYS:
            G.load(sel, c["sels"][which])
            G.poison(out[1])
            cap.replay()
            _sync()
            assert [G.raw(t) for t in out] == exp[which], which


@records("hc_trifocal_pose_refine_grouped")
def test_refine_joint_grouped(problem, clean33):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    c = clean33
    dev = c["edgels"].device
    db = TripletBatch(problem, [c["data"], c["data"]], seeds=0, samples_per_triplet=1, edgel_counts=[33, 33]).to(dev)
    pairs = {"A": np.concatenate([c["sels"]["A"], c["sels"]["B"]]),
             "B": np.concatenate([c["sels"]["B"], c["sels"]["A"]])}
    sels = _dev(pairs["A"], dev)

    def eager(which):
        out = pose.launch_refine_joint_grouped(sels.clone(), db)
        _sync()
        return [G.raw(t) for t in out]
    _replay_against_eager(lambda: pose.launch_refine_joint_grouped(sels, db), lambda which: G.load(sels, pairs[which]),
                          lambda out: out, eager)
    assert torch.equal(sels.cpu(), torch.from_numpy(pairs["A"]))      # the input is left as it was


@records("hc_trifocal_pose_inlier_mask")
def test_inlier_mask(clean33, pose_inputs):
    """Through _abi.call: the Python wrapper synchronises by design.  The
    selections are the clean scene's, the edgels the first 33 noisy ones, so
    that the two masks differ."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    c = clean33
    dev = c["edgels"].device
    E = 33
    sets = {"A": (c["sels"]["A"], pose_inputs["noisy0"].locations[:E]),
            "B": (c["sels"]["B"], pose_inputs["noisy0"].locations[E:2 * E])}
    sel, edgels = _dev(sets["A"][0], dev), _dev(np.array(sets["A"][1]), dev)
    words = torch.empty(1, dtype=torch.int64, device=dev)

    def enqueue():
        _abi.call("hc_trifocal_pose_inlier_mask", _abi.ptr(sel), E, _abi.ptr(edgels), _abi.ptr(c["K"]),
                  _abi.ptr(words), _abi.ptr(torch.cuda.current_stream(dev)))

    def put(which):
        G.load(sel, sets[which][0])
        G.load(edgels, np.array(sets[which][1]))

    def eager(which):
        w = pose.inlier_mask(sel, edgels, c["K"], packed=True)
        assert 0 < bin(int(w[0])).count("1") < E
        return [w.tobytes()]
    _replay_against_eager(enqueue, put, lambda out: (words,), eager)


@records("hc_shared_flag_reset")
def test_shared_flag_reset():
    """The reset is a memset node: a word set from outside the graph is zero
    after every replay, and its neighbours are left alone."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    dev = torch.device("cuda:0")
    flag = torch.zeros(3, dtype=torch.int32, device=dev)

    def enqueue():
        _abi.call("hc_shared_flag_reset", _abi.ptr(flag[1:]), _abi.ptr(torch.cuda.current_stream(dev)))

    with recorded(enqueue) as (cap, _):
        for v in (1, 0x5A5A5A5A, 7):
            flag.fill_(v)
            cap.replay()
            _sync()
            assert flag.cpu().tolist() == [v, 0, v]


@pytest.fixture(scope="module")
def points(problem, samples100):
    """Two sets of three points (x, p, d): start solutions moved by 1 %, at the
    parameters of samples 0-2 (A) and 3-5 (B)."""
    tgt, dif, _ = samples100
    out = {}
    for which, s, f in (("A", slice(0, 3), 1.01), ("B", slice(3, 6), 0.99)):
        x = (problem.start_sols[s] * np.float32(f)).astype(np.float32)
        x[:, 30] = (1.0, 0.0)
        out[which] = (x, np.ascontiguousarray(tgt[s]), np.ascontiguousarray(dif[s]))
    return out


def _stream_ptr(dev):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    return _abi.ptr(torch.cuda.current_stream(dev))


@records("hc_trifocal_eval_batched")
def test_eval_batched(problem, tracker, points):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import eval_batched
    dev, n, p = tracker.device, 3, _abi.ptr
    X, P, D = (_dev(v, dev) for v in points["A"])
    outs = (torch.empty((n, 30, 30, 2), dtype=torch.float32, device=dev),
            torch.empty((n, 30, 2), dtype=torch.float32, device=dev),
            torch.empty((n, 30, 2), dtype=torch.float32, device=dev))
    ws = tracker.new_workspace()

    def enqueue():
        _abi.call("hc_trifocal_eval_batched", n, p(tracker.unified), p(X), p(P), p(D), *(p(t) for t in outs), p(ws),
                  ws.numel(), _stream_ptr(dev))

    def put(which):
        for dst, src in zip((X, P, D), points[which]):
            G.load(dst, src)
    _replay_against_eager(enqueue, put, lambda out: outs,
                          lambda which: [a.tobytes() for a in eval_batched(problem.unified_index, *points[which])])
    tracker.workspace_status(ws)


@records("hc_trifocal_p2c_eval_batched")
def test_p2c_eval_batched(tracker, points):
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, p2c
    dev, n, p = tracker.device, 3, _abi.ptr
    hx, ht = pc.fixture_tables()
    chx, cht = pc.blocks(4)
    sets = {"A": (points["A"][0], chx[[0, 1, 0]], cht[[0, 1, 0]], np.array([0.0, 1.0, 0.25], np.float32)),
            "B": (points["B"][0], chx[[2, 3, 3]], cht[[2, 3, 3]], np.array([1.0, 0.5, 0.0], np.float32))}
    tables = tracker.p2c_tables((hx, ht))
    bufs = tuple(_dev(v, dev) for v in sets["A"])
    outs = (torch.empty((n, 30, 30, 2), dtype=torch.float32, device=dev),
            torch.empty((n, 30, 2), dtype=torch.float32, device=dev),
            torch.empty((n, 30, 2), dtype=torch.float32, device=dev))
    ws = tracker.new_workspace()

    def enqueue():
        _abi.call("hc_trifocal_p2c_eval_batched", n, p(tables[0]), p(tables[1]), *(p(t) for t in bufs),
                  *(p(t) for t in outs), p(ws), ws.numel(), _stream_ptr(dev))

    def put(which):
        for dst, src in zip(bufs, sets[which]):
            G.load(dst, src)
    _replay_against_eager(enqueue, put, lambda out: outs,
                          lambda which: [a.tobytes() for a in p2c.eval_batched(hx, ht, *sets[which])])
    tracker.workspace_status(ws)


@records("hc_cgesv_30x30_batched")
def test_cgesv_batched(problem, oracle, tracker, points):
    """Three Jacobian systems dH/dx . x = dH/dt of the oracle's evaluations at the points."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import cgesv_batched
    dev, n, p = tracker.device, 3, _abi.ptr
    sets = {}
    for which, (x, pr, d) in points.items():
        sets[which] = (np.stack([oracle.eval_hx(problem.dHdx_index, x[i], pr[i]) for i in range(n)]),
                       np.stack([oracle.eval_ht(problem.dHdt_index, x[i], pr[i], d[i]) for i in range(n)]))
    A, b = (_dev(v.astype(np.float32), dev) for v in sets["A"])
    x = torch.empty_like(b)

    def put(which):
        G.load(A, sets[which][0].astype(np.float32))
        G.load(b, sets[which][1].astype(np.float32))
    _replay_against_eager(lambda: _abi.call("hc_cgesv_30x30_batched", n, p(A), p(b), p(x), _stream_ptr(dev)), put,
                          lambda out: (x,), lambda which: [cgesv_batched(*sets[which]).tobytes()])
