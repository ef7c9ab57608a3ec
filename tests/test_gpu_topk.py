"""GPU tests of the top-k calls (include/topk/hc_pose_topk.h).

Ranking: hc_trifocal_pose_topk_joint and its grouped form, exact against numpy
(tests/topk_reference.py) on synthetic count arrays over buffers whose every
path holds one of the 36 committed candidate tracks of pose_N100_seed0.npz
(path b holds track b % 36), and against the joint call itself on real counts.

Refine-and-select: hc_trifocal_pose_refine_topk and its grouped form against
hc_trifocal_pose_refine, byte for byte, on the candidates of two config-5 runs:
trial 0 (pose_joint_noisy1px_N100.npz) and trial 12
(pose_topk_noisy1px_trial12_N100.npz), the run whose joint winner cannot be
refined out of its wrong basin and whose third-ranked candidate can.  No test
tracks: the tracks arrays are assembled from the committed candidate tracks.
"""
import numpy as np
import pytest

import refine_reference as RR
import topk_reference as TR
from checks import NOISE_SEED, golden, noisy_data

pytestmark = pytest.mark.gpu

POSE_KEYS = RR.POSE_KEYS
NTRK = 312
# Largest pose distance of a refined top-k candidate of trial 12 (ranks 0..7) to
# the stored numpy reference, measured on an MI355X (test_trial12_against_the_reference
# prints it): 0 -- the 24 floats of all eight are the reference's, with the same
# counts and joint histories.  The bound is the rule of tests/test_gpu_refine.py:
# ten times the measured value, not below ten float32 steps at 1 (the reference
# sums through the host's BLAS), never above 1e-4.
MEASURED_D = 0.0
POSE_BOUND = max(10 * MEASURED_D, 10 * 2.0 ** -24)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _rows(t, count):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    return t.cpu().numpy().view(np.uint8).reshape(count, pose.JOINT_SEL_BYTES)


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _assert_none(d, nc):
    assert (d["num_candidates"], d["path"], d["inliers"], d["inliers21"], d["inliers31"], d["key"]) == \
        (nc, -1, -1, -1, -1, 0)
    assert not any(d[k].any() for k in POSE_KEYS) and d["scale31"] == 0


# ---- ranking ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def base(tracker):
    """36 candidate tracks, and per track the pose bits and scale31 the joint
    call gives over that track alone."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    cand = np.ascontiguousarray(golden("pose_N100_seed0")["cand_tracks"])
    assert cand.shape == (36, 31, 2)
    noisy0 = noisy_data()
    edgels = _dev(np.array(noisy0.locations[:200]), dev)
    K = _dev(noisy0.K, dev)
    tr = np.tile(cand, (9, 1, 1))[:NTRK]
    T = _dev(tr, dev)
    alone = []
    for j in range(36):
        conv = np.zeros(NTRK, np.uint8)
        conv[j] = 1
        _, s = pose.pose_support_joint(T, _dev(conv, dev), edgels, K)
        assert s["path"] == j and s["num_candidates"] == 1
        alone.append(s)
    cand.setflags(write=False)
    return dict(dev=dev, cand=cand, alone=alone, edgels=edgels, K=K, tracks={})


def _tracks(base, n):
    """(n, 31, 2) on the device: path b holds candidate track b % 36."""
    if n not in base["tracks"]:
        base["tracks"][n] = _dev(base["cand"][np.arange(n) % 36], base["dev"])
    return base["tracks"][n]


def _check_ranking(base, dicts, raw, inl, k, ids=None, track_of=None):
    """dicts / raw (k, 136): a call's output over counts inl (n, 3) whose row i
    is batch id ids[i] (default i) and holds track track_of[i] (default id % 36)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    n = len(inl)
    ids = np.arange(n) if ids is None else np.asarray(ids)
    rows = np.nonzero(inl[:, 0] >= 0)[0]
    order = rows[TR.rank(inl[rows], ids[rows])]
    nc = len(rows)
    assert len(dicts) == k
    for r, d in enumerate(dicts):
        assert bytes(pose.joint_selection_from_dict(d)) == raw[r].tobytes(), r      # the padding is 0
        if r >= nc:
            _assert_none(d, nc)
            continue
        i = int(order[r])
        b = int(ids[i])
        assert (d["num_candidates"], d["path"]) == (nc, b), r
        assert [d["inliers"], d["inliers21"], d["inliers31"]] == inl[i].tolist(), r
        assert d["key"] == (int(inl[i, 0]) << 32) | b, r
        one = base["alone"][(b % 36) if track_of is None else int(track_of[i])]
        for key in POSE_KEYS + ("scale31",):
            assert d[key].tobytes() == one[key].tobytes(), (r, key)
    ky = [d["key"] for d in dicts[:min(k, nc)]]
    assert ky == sorted(ky, reverse=True) and len(set(ky)) == len(ky)


def _patterns(n, k, rng):
    """name -> (n, 3) counts, -1 for non-candidates."""
    out = {}

    def make(ids, joint):
        a = np.full((n, 3), -1, np.int32)
        ids = np.asarray(ids, np.int64)
        a[ids, 0] = joint
        a[ids, 1] = np.asarray(joint) + 1
        a[ids, 2] = np.asarray(joint) + 2
        return a
    for m in sorted({0, 1, k - 1, k, k + 1}):
        ids = np.sort(rng.choice(n, m, replace=False))
        out[f"{m} scattered"] = make(ids, rng.integers(0, 50, m))       # repeated counts: ids break the ties
    start = int(rng.integers(0, n // 64 - 1)) * 64
    wave = np.arange(start, start + 64)                                   # one whole wave, more than k in one wave
    out["wave equal"] = make(wave, np.full(64, 7))
    out["wave increasing"] = make(wave, np.arange(64) + 3)                # every insertion displaces the whole chain
    out["wave decreasing"] = make(wave, 100 - np.arange(64))
    out["wave across"] = make(wave + 32, rng.integers(0, 4, 64))
    s = int(rng.integers(0, n // NTRK)) * NTRK
    sample = np.arange(s, s + NTRK)                                       # all 312 paths of a sample
    out["sample equal"] = make(sample, np.zeros(NTRK, np.int64))          # count 0: at s = 0 the key of path 0 is 0
    out["sample increasing"] = make(sample, np.arange(NTRK))
    out["sample decreasing"] = make(sample, 5000 - np.arange(NTRK))
    out["first and last"] = make([0, n - 1], [0, 0])
    return out


@pytest.mark.parametrize("k", [1, 2, 8, 32])
@pytest.mark.parametrize("n", [312, 624, 31200])
def test_ranking_against_numpy(base, n, k):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    T = _tracks(base, n)
    rng = np.random.default_rng(1000 * k + n)
    for name, inl in _patterns(n, k, rng).items():
        I = _dev(inl, base["dev"])
        dicts, raw = pose.topk_joint(T, I, k, return_device_selection=True)
        again = pose.launch_topk_joint(T, I, k)
        assert _bytes(raw) == _bytes(again), name                         # two calls, identical bytes
        try:
            _check_ranking(base, dicts, _rows(raw, k), inl, k)
        except AssertionError as e:
            raise AssertionError(f"pattern {name!r}: {e}") from e


def test_first_sample_all_candidates_with_count_zero(base):
    """Sample 0 whole, every count 0: keys 311 .. 0, and the key 0 of path 0 is
    a candidate like the others (rank 311 of 312 is beyond k = 32; with 3
    candidates it is the last rank)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    T = _tracks(base, 312)
    inl = np.full((312, 3), -1, np.int32)
    inl[[0, 5, 9]] = 0
    dicts, raw = pose.topk_joint(T, _dev(inl, base["dev"]), 4, return_device_selection=True)
    _check_ranking(base, dicts, _rows(raw, 4), inl, 4)
    assert [d["path"] for d in dicts] == [9, 5, 0, -1] and dicts[2]["key"] == 0 and dicts[2]["inliers"] == 0


def test_no_paths(base):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    T = _tracks(base, 312)
    I = _dev(np.zeros((0, 3), np.int32), base["dev"])
    for k in (1, 8):
        dicts = pose.topk_joint(T[:0], I, k)
        assert len(dicts) == k
        for d in dicts:
            _assert_none(d, 0)


def test_python_refuses_short_buffers(base, ransac0, problem):
    """Buffers that do not cover the call are refused before the library is called."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    dev = base["dev"]
    T = _tracks(base, 624)
    I = torch.full((624, 3), -1, dtype=torch.int32, device=dev)
    short = torch.empty(4 * pose.JOINT_SEL_BYTES - 1, dtype=torch.uint8, device=dev)
    for args, kw in (((T, I[:623], 4), {}), ((T, I, 4), dict(candidates=short)), ((T.cpu(), I, 4), {}),
                     ((T, I.t(), 4), {})):
        with pytest.raises(_abi.HCError):
            pose.launch_topk_joint(*args, **kw)
    db = TripletBatch(problem, [ransac0], seeds=0, samples_per_triplet=1).to(dev)
    with pytest.raises(_abi.HCError):
        pose.launch_topk_joint_grouped(T, I, db, 4)                          # 2 samples of tracks, a batch of 1
    cand = pose.launch_topk_joint(T, I, 4)
    with pytest.raises(_abi.HCError):
        pose.launch_refine_topk(cand[:-1], base["edgels"], base["K"])       # not a whole number of selections
    with pytest.raises(_abi.HCError):
        pose.launch_refine_topk(cand, base["edgels"], base["K"], refined=short)
    with pytest.raises(_abi.HCError):
        pose.launch_refine_topk_grouped(cand, db, 8)                         # 4 candidates for 1 x 8


def test_rank_0_is_the_joint_selection_and_every_rank_its_own_pose(base):
    """Real counts: 36 candidates at scattered ids of 624 paths, scored on 200
    noisy edgels.  candidates[0] is the joint call's selection in all 136
    bytes; every rank carries the counts of its path and the pose bits of the
    joint call over that track alone; ranks beyond the 36 are none."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = base["dev"]
    rng = np.random.default_rng(11)
    ids = np.sort(rng.choice(624, 36, replace=False))
    tr = np.zeros((624, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    perm = rng.permutation(36)
    tr[ids] = base["cand"][perm]
    conv = np.zeros(624, np.uint8)
    conv[ids] = 1
    T = _dev(tr, dev)
    inl_dev = torch.empty((624, 3), dtype=torch.int32, device=dev)
    sel_dev = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    pose.launch_pose_support_joint(T, _dev(conv, dev), base["edgels"], base["K"], inl_dev, sel_dev)
    inl = inl_dev.cpu().numpy()
    assert (inl[ids, 0] >= 0).all() and (np.delete(inl, ids, axis=0) == -1).all()
    track_of = np.zeros(624, np.int64)
    track_of[ids] = perm
    for k in (1, 8, 32):
        dicts, raw = pose.topk_joint(T, inl_dev, k, return_device_selection=True)
        rows = _rows(raw, k)
        assert rows[0].tobytes() == _bytes(sel_dev), k
        _check_ranking(base, dicts, rows, inl, k, track_of=track_of)
    dicts = pose.topk_joint(T, inl_dev, 32)
    assert all(d["path"] >= 0 for d in dicts) and dicts[0]["num_candidates"] == 36
    # 36 candidates, k = 32 < 36 < 2 k: merging the two halves' lists gives the one call's list
    parts = [pose.topk_joint(T[a:b].contiguous(), inl_dev[a:b].contiguous(), 32) for a, b in ((0, 312), (312, 624))]
    merged = pose.merge_topk(parts, [0, 312], 32)
    for m, d in zip(merged, dicts):
        assert bytes(pose.joint_selection_from_dict(m)) == bytes(pose.joint_selection_from_dict(d))


@pytest.mark.parametrize("T", [2, 3])
def test_grouped_ranking_equals_single_calls(problem, base, ransac0, T):
    """Interleaved samples of T triplets: every triplet's list is the single
    call over its own samples, with the call's batch ids."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    import torch
    dev = base["dev"]
    per = [2, 3, 1][:T]
    batch = TripletBatch(problem, [ransac0] * T, seeds=0, samples_per_triplet=per, interleave=True,
                         edgel_counts=[63, 200, 100][:T])
    assert batch.sample_group.tolist() == ([0, 1, 0, 1, 1] if T == 2 else [0, 1, 2, 0, 1, 1])
    db = batch.to(dev)
    n = batch.num_samples * NTRK
    tracks = _tracks(base, n)
    rng = np.random.default_rng(40 + T)
    inl = np.full((n, 3), -1, np.int32)
    spots = np.sort(rng.choice(n, 90, replace=False))
    inl[spots] = rng.integers(0, 6, (90, 1)) + np.arange(3)[None, :]
    if T == 3:
        inl[batch.path_index(2)] = -1                                      # a triplet without a candidate
    I = _dev(inl, dev)
    for k in (1, 8, 32):
        lists = pose.topk_joint_grouped(tracks, I, db, k)
        raw = _rows(pose.launch_topk_joint_grouped(tracks, I, db, k), T * k)
        assert len(lists) == T
        for t in range(T):
            rows = batch.path_index(t)
            _check_ranking(base, lists[t], raw[t * k:(t + 1) * k], inl[rows], k, ids=rows, track_of=rows % 36)
            idx = torch.from_numpy(rows).to(dev)
            single = pose.topk_joint(tracks[idx].contiguous(), I[idx].contiguous(), k)
            for s, g in zip(single, lists[t]):
                assert g["path"] == (int(rows[s["path"]]) if s["path"] >= 0 else -1)
                for key in ("num_candidates", "inliers", "inliers21", "inliers31"):
                    assert s[key] == g[key], (t, key)
                for key in POSE_KEYS + ("scale31",):
                    assert s[key].tobytes() == g[key].tobytes(), (t, key)
        if T == 3:
            assert all(d["path"] == -1 for d in lists[2])
    # the host copy of the batch is accepted like the device copy
    assert [d["path"] for d in pose.topk_joint_grouped(tracks, I, batch, 2)[0]] == [d["path"] for d in lists[0][:2]]


# ---- refine and select ----------------------------------------------------------------------------

def _trial(tracker, name, seed):
    """A config-5 run's candidates at their batch ids of a 31 200-path launch,
    scored on the 5117 noisy edgels by the joint call, and its 8 best."""
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    dev = tracker.device
    g = golden(name)
    data = noisy_data(seed)
    ids = g["cand_ids"]
    tr = np.zeros((31200, 31, 2), np.float32)
    tr[:, 30, 0] = 1.0
    tr[ids] = g["cand_tracks"]
    conv = np.zeros(31200, np.uint8)
    conv[ids] = 1
    edgels = _dev(np.array(data.locations), dev)
    K = _dev(data.K, dev)
    T, Cv = _dev(tr, dev), _dev(conv, dev)
    inl = torch.empty((31200, 3), dtype=torch.int32, device=dev)
    sel = torch.empty(pose.JOINT_SEL_BYTES, dtype=torch.uint8, device=dev)
    pose.launch_pose_support_joint(T, Cv, edgels, K, inl, sel)
    cand = pose.launch_topk_joint(T, inl, 8)
    torch.cuda.synchronize(dev)
    assert np.array_equal(inl.cpu().numpy()[ids], g["counts"])
    assert _rows(cand, 8)[0].tobytes() == _bytes(sel)
    return dict(g=g, data=data, edgels=edgels, K=K, tracks=T, conv=Cv, inl=inl, cand=cand,
                joint=pose.joint_selection_dict(pose.joint_selection_struct(sel)))


@pytest.fixture(scope="module")
def trial12(tracker):
    return _trial(tracker, "pose_topk_noisy1px_trial12_N100", NOISE_SEED + 12)


@pytest.fixture(scope="module")
def trial0(tracker):
    return _trial(tracker, "pose_joint_noisy1px_N100", NOISE_SEED)


def _head(cand, k):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    return cand[:k * pose.JOINT_SEL_BYTES]


def _check_consistency(c, k):
    """The properties every refine-and-select result has; returns the dicts."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    S, R = pose.JOINT_SEL_BYTES, pose.REPORT_BYTES
    cand = _head(c["cand"], k)
    keep = _bytes(cand)
    best, rank, refined, reports = pose.launch_refine_topk(cand, c["edgels"], c["K"])
    assert _bytes(cand) == keep
    rank = int(rank.cpu().numpy()[0])
    ref = _rows(refined, k)
    rep = reports.cpu().numpy().reshape(k, R)
    singles = []
    for r in range(k):
        one, one_rep = pose.launch_refine_joint(cand[r * S:(r + 1) * S], c["edgels"], c["K"])
        assert ref[r].tobytes() == _bytes(one), (k, r)
        assert rep[r].tobytes() == _bytes(one_rep), (k, r)
        singles.append(pose.joint_selection_dict(pose.joint_selection_struct(one)))
    # best is the max-key entry of the device's own refined
    keys = [(s["inliers"] << 32) | s["path"] if s["path"] >= 0 else -1 for s in singles]
    assert rank == int(np.argmax(keys)) and keys[rank] >= 0
    assert _bytes(best) == ref[rank].tobytes()
    assert singles[rank]["inliers"] >= singles[0]["inliers"]               # at least the refined joint winner's
    assert singles[0]["path"] == c["joint"]["path"]
    # refined == candidates, and a second call
    alias = cand.clone()
    b2, r2, f2, p2 = pose.launch_refine_topk(alias, c["edgels"], c["K"], refined=alias)
    assert f2.data_ptr() == alias.data_ptr()
    assert (_bytes(b2), _bytes(r2), _bytes(f2), _bytes(p2)) == (_bytes(best), np.int32(rank).tobytes(),
                                                                _bytes(refined), _bytes(reports))
    # the synchronous form
    bd, br, rd, pd = pose.refine_topk(cand, c["edgels"], c["K"])
    assert br == rank and bd["path"] == singles[rank]["path"] and bd["inliers"] == singles[rank]["inliers"]
    assert [d["inliers"] for d in rd] == [s["inliers"] for s in singles]
    assert [p["joint_history"][0] for p in pd] == [int(x) for x in _candidate_counts(c, k)]
    return singles, rank


def _candidate_counts(c, k):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    return [pose.joint_selection_dict(pose.joint_selection_struct(r))["inliers"] for r in _rows(_head(c["cand"], k), k)]


@pytest.mark.parametrize("k", [1, 4, 8])
def test_refine_topk_is_k_single_refinements_and_their_maximum(trial0, trial12, k):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    for c in (trial0, trial12):
        singles, rank = _check_consistency(c, k)
        if k == 1:
            # the refined joint winner, in every byte
            one, _ = pose.launch_refine_joint(c["cand"][:pose.JOINT_SEL_BYTES], c["edgels"], c["K"])
            best = pose.launch_refine_topk(_head(c["cand"], 1), c["edgels"], c["K"])[0]
            assert rank == 0 and _bytes(best) == _bytes(one)


def test_all_none_candidates(base, trial0):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, pose
    c = trial0
    T = _tracks(base, 312)
    cand = pose.launch_topk_joint(T[:0], _dev(np.zeros((0, 3), np.int32), base["dev"]), 4)
    best, rank, refined, reports = pose.refine_topk(cand, c["edgels"], c["K"])
    _assert_none(best, 0)
    assert rank == -1 and all(r["status"] == _abi.HC_REFINE_NONE for r in reports)
    for d in refined:
        _assert_none(d, 0)
    # fewer candidates than k: the none ranks never win
    inl = np.full((312, 3), -1, np.int32)
    inl[7] = 3
    cand = pose.launch_topk_joint(T, _dev(inl, base["dev"]), 4)
    best, rank, refined, reports = pose.refine_topk(cand, c["edgels"], c["K"])
    assert rank == 0 and best["path"] == 7 and [d["path"] for d in refined] == [7, -1, -1, -1]
    assert [r["none"] for r in reports] == [False, True, True, True]


def test_grouped_refine_topk_equals_single_calls(problem, trial0, trial12):
    """Two triplets of different edgel counts in one launch: each group's
    refined, reports, best and best_rank are the single call's on its scene."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
    import torch
    k = 4
    S, R = pose.JOINT_SEL_BYTES, pose.REPORT_BYTES
    counts = [5117, 2049]
    batch = TripletBatch(problem, [trial12["data"], trial0["data"]], seeds=0, samples_per_triplet=1,
                         edgel_counts=counts)
    dev = trial0["edgels"].device
    db = batch.to(dev)
    cand = torch.cat([_head(trial12["cand"], k), _head(trial0["cand"], k)]).contiguous()
    best, rank, refined, reports = pose.launch_refine_topk_grouped(cand, db, k)
    torch.cuda.synchronize(dev)
    for t, c in enumerate((trial12, trial0)):
        b1, r1, f1, p1 = pose.launch_refine_topk(cand[t * k * S:(t + 1) * k * S], c["edgels"][:counts[t]], c["K"])
        assert _bytes(refined[t * k * S:(t + 1) * k * S]) == _bytes(f1), t
        assert _bytes(reports[t * k * R:(t + 1) * k * R]) == _bytes(p1), t
        assert _bytes(best[t * S:(t + 1) * S]) == _bytes(b1) and _bytes(rank[t:t + 1]) == _bytes(r1), t
    out = pose.refine_topk_grouped(cand, batch, k, device=dev)              # the host batch, uploaded
    assert [o["best_rank"] for o in out] == rank.cpu().numpy().tolist()
    assert out[0]["best"]["path"] == 3607


def test_trial12_is_repaired(trial12):
    """The test the feature exists for.  The joint winner (path 29311, 644 joint
    inliers) refined alone stays in its wrong basin; refine_topk with k = 4
    returns the third-ranked candidate, path 3607, which passes the GT check."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c, g = trial12, trial12["g"]
    assert (c["joint"]["path"], c["joint"]["inliers"], c["joint"]["num_candidates"]) == (29311, 644, 35)
    alone, rep = pose.refine_joint(c["cand"][:pose.JOINT_SEL_BYTES], c["edgels"], c["K"])
    res, ok = pose.residuals(c["data"], alone)
    assert not ok and alone["path"] == 29311
    best, rank, refined, reports = pose.refine_topk(_head(c["cand"], 4), c["edgels"], c["K"])
    res, ok = pose.residuals(c["data"], best)
    print(f"trial 12, k = 4: best rank {rank}, path {best['path']}, refined counts "
          f"{[d['inliers'] for d in refined]} | reference {g['ref_counts'][:4, 0].tolist()}, residuals {res.tolist()}")
    assert [d["path"] for d in refined] == [29311, 15336, 3607, 20328]
    assert rank == 2 and best["path"] == 3607
    assert ok and res[0] < 0.1 and res[1] < 0.1
    assert abs(best["inliers"] - int(g["ref_counts"][2, 0])) <= int(g["borderline"][2])
    # the whole chain on one stream gives the same selection
    best2, info = pose.select_refined(c["tracks"], c["conv"], c["edgels"], c["K"], k=4)
    assert bytes(pose.joint_selection_from_dict(best2)) == bytes(pose.joint_selection_from_dict(best))
    assert info["best_rank"] == 2 and info["joint"]["path"] == 29311
    assert info["refined_inliers"] == [d["inliers"] for d in refined]
    assert [p["status"] for p in info["reports"]] == [p["status"] for p in reports]


def test_trial12_against_the_reference(trial12):
    """Ranks 0..7 refined on the device against the stored numpy reference: the
    pose within POSE_BOUND, the count within the stored borderline count."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
    c, g = trial12, trial12["g"]
    assert POSE_BOUND <= 1e-4
    best, rank, refined, reports = pose.refine_topk(c["cand"], c["edgels"], c["K"])
    worst = 0.0
    for r, (d, rep) in enumerate(zip(refined, reports)):
        ref = {k: v for k, v in zip(POSE_KEYS, np.split(g["ref_pose"][r], [9, 12, 21]))}
        dist = RR.pose_distance(d, ref)
        worst = max(worst, dist)
        print(f"trial 12 rank {r} path {d['path']}: d = {dist:.3e}, counts {d['inliers']} | {g['ref_counts'][r, 0]} "
              f"(B = {g['borderline'][r]}), best iteration {rep['best_iteration']} | {g['ref_best_iteration'][r]}, "
              f"history {rep['joint_history'][:11].tolist()} | {g['ref_history'][r][:11].tolist()}")
    print(f"trial 12: largest pose distance {worst:.3e} (MEASURED_D = {MEASURED_D}, bound {POSE_BOUND:.3e})")
    for r, d in enumerate(refined):
        ref = {k: v for k, v in zip(POSE_KEYS, np.split(g["ref_pose"][r], [9, 12, 21]))}
        assert d["path"] == int(g["cand_ids"][g["ranking"][r]])
        assert RR.pose_distance(d, ref) <= POSE_BOUND, r
        assert abs(d["inliers"] - int(g["ref_counts"][r, 0])) <= int(g["borderline"][r]), r
    # with 8 the reference's best two (3626 at rank 4, 3620 at rank 6) are closer than their
    # borderline edgels: only that a right-basin candidate wins is pinned
    assert rank in (2, 4, 6) and pose.residuals(c["data"], best)[1]
