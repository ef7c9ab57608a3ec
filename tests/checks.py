"""The parity bar of the GPU tests, stated once (tests/test_checks.py tests it
on the CPU).

Bar: the HIP tracker and the oracle implement the same op-level
spec, so converged / infinity flags, step / correction counts and every float
of x[0..29] are identical, treating +0 == -0 and NaN == NaN (conftest.same).
x[30] is never written by the kernels: it is compared only where a path must
not have been touched at all.

A result `r` is a TrackResult.host() dict, or any mapping with the same keys.
One without "stats" (the reference's launchers, driven through the shim, report
none) is compared on what it carries, and its caller passes None for the counts.
Every checker asserts the union of what the hand-written copies it replaced
asserted; a selection (`where`) that selects nothing fails unless the caller
says that it may be empty.
"""
import contextlib
import functools
import os
import shutil
import subprocess

import numpy as np

from conftest import same

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CLI = os.path.join(ROOT, "trifocal_pose_estimation_using_improved_gpuhc_amd", "bin", "magmaHC-main")
NOISE_SEED = 20250215   # synthcurves.DEFAULT_SEED: the bench's first config-5 trial
STAT_KEYS = ("steps", "corrections", "inliers21", "inliers31")


# ---- golden runs ----------------------------------------------------------

def track_hash(tracks):
    """Per-path 64-bit polynomial hash of x[0..29] with +0/-0 and NaN canonicalised."""
    a = np.ascontiguousarray(tracks[:, :30, :], np.float32).copy()
    a[a == 0] = 0.0
    a[np.isnan(a)] = np.float32(np.nan)
    w = a.reshape(a.shape[0], -1).view(np.uint32).astype(np.uint64)
    h = np.zeros(a.shape[0], np.uint64)
    P = np.uint64(1099511628211)
    with np.errstate(over="ignore"):
        for k in range(w.shape[1]):
            h = (h * P) ^ w[:, k]
    return h


def golden(name):
    """tests/golden/<name>.npz"""
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def golden_passing(g):
    """Batch ids of a golden run's hypotheses that pass the oracle's scoring."""
    return set(int(b) for b, s in zip(g["scored_ids"], g["scored"]) if s[0] == 1)


# ---- one run against another ----------------------------------------------

def tracked(r):
    """Paths an abort-mode launch tracked (every path of the committed inputs takes >= 13 steps
    at the default limits, and at least 1 at any: test_limits_host.py)."""
    return r["stats"]["steps"] > 0


def _selection(where, n, allow_empty):
    if where is None:
        ids = np.arange(n)
    else:
        where = np.asarray(where)
        if where.dtype == bool:
            assert where.shape == (n,), f"a mask of shape {where.shape} over {n} paths"
            ids = np.nonzero(where)[0]
        else:
            ids = where.astype(np.int64)
    assert allow_empty or len(ids) > 0, "nothing selected: the check would pass vacuously"
    return ids


def _none_differ(what, differ, ids):
    bad = ids[differ]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ids)} paths differ, first {bad[:5].tolist()}"


def _count_fields(r, conv, inf, steps, corrections):
    out = [("converge", r["converge"], conv), ("infinity", r["infinity"], inf)]
    if "stats" in r:
        out += [("steps", r["stats"]["steps"], steps), ("corrections", r["stats"]["corrections"], corrections)]
    else:
        assert steps is None and corrections is None, "a result without stats has no counts to compare"
    return out


def assert_same_run(r, tracks, conv, inf, steps, corrections, where=None, allow_empty=False):
    """r against another run of the same paths: flags and counts equal, x[0..29]
    the same values.  where (a mask or batch ids) restricts the comparison."""
    ids = _selection(where, len(r["converge"]), allow_empty)
    for what, got, exp in _count_fields(r, conv, inf, steps, corrections):
        got, exp = np.asarray(got), np.asarray(exp)
        assert got.shape == exp.shape, f"{what}: {got.shape} against {exp.shape}"
        _none_differ(what, got[ids] != exp[ids], ids)
    assert r["tracks"].shape == tracks.shape
    _none_differ("tracks", ~same(r["tracks"][ids, :30], tracks[ids, :30]).all(axis=(1, 2)), ids)


def assert_matches_oracle(r, ref, where=None, allow_empty=False):
    """ref: what oracle.gpuhc_track / gpuhc_track_subset returns."""
    tr, conv, inf, st = ref
    assert_same_run(r, tr, conv, inf, st["steps"], st["corrections"], where, allow_empty)


def assert_matches_golden(r, g, where=None, rows=None, allow_empty=False):
    """r against a committed golden run (flags, counts, track hashes); rows: the
    slice of the golden run that r covers (default: all of it)."""
    rows = slice(None) if rows is None else rows
    ids = _selection(where, len(r["converge"]), allow_empty)
    fields = _count_fields(r, g["conv"][rows], g["inf"][rows], g["steps"][rows], g["corrections"][rows])
    for what, got, exp in fields + [("track hashes", track_hash(r["tracks"]), g["hash"][rows])]:
        got = np.asarray(got)
        assert got.shape == exp.shape, f"{what}: {got.shape} against {exp.shape}"
        _none_differ(what, got[ids] != exp[ids], ids)


def assert_bit_identical(a, b, rows=None):
    """Two runs of the same build (time slicing, streams, shared workspaces
    change when a path runs, never what it computes): flags and counts equal and
    all 31 track entries the same bits, sign of zero and NaN payloads included.
    rows: the slice of b that a covers."""
    rows = slice(None) if rows is None else rows
    ids = np.arange(len(a["converge"]))
    for what, got, exp in _count_fields(a, b["converge"][rows], b["infinity"][rows], b["stats"]["steps"][rows],
                                        b["stats"]["corrections"][rows]):
        assert got.shape == exp.shape, f"{what}: {got.shape} against {exp.shape}"
        _none_differ(what, got != exp, ids)
    x, y = a["tracks"].view(np.uint32), b["tracks"][rows].view(np.uint32)
    assert x.shape == y.shape
    _none_differ("track bits", (x != y).any(axis=(1, 2)), ids)


# ---- abort-mode results -----------------------------------------------------

def assert_untouched(r, start_sols, where, allow_empty=False):
    """Paths an abort-mode launch did not track: flags and all four stats zero,
    all 31 track entries the start solution, no joint count."""
    ids = _selection(where, len(r["converge"]), allow_empty)
    _none_differ("converge of an untracked path", r["converge"][ids] != 0, ids)
    _none_differ("infinity of an untracked path", r["infinity"][ids] != 0, ids)
    if "stats" in r:
        for k in STAT_KEYS:
            _none_differ(f"{k} of an untracked path", r["stats"][k][ids] != 0, ids)
    start = start_sols[ids % start_sols.shape[0]]
    _none_differ("an untracked path's start solution",
                 (r["tracks"][ids].view(np.uint32) != start.view(np.uint32)).any(axis=(1, 2)), ids)
    if "joint_inliers" in r:
        _none_differ("joint_inliers of an untracked path", r["joint_inliers"][ids] != -1, ids)


def found_ids(r):
    """The batch ids an abort-mode launch reported; each entry holds its own id."""
    ids = np.nonzero(r["batch_index"] >= 0)[0]
    _none_differ("batch_index", r["batch_index"][ids] != ids, ids)
    return ids


class GroupCase:
    """A TripletBatch, the plain (abort-off) run of all its samples as a host
    dict and, for the gated launch, the grouped joint pose support of those
    plain tracks (n x 3 counts).  on_device() makes one with the device copies."""

    def __init__(self, batch, plain, counts=None, dev=None, plain_dev=None):
        self.batch, self.plain, self.counts, self.dev, self.plain_dev = batch, plain, counts, dev, plain_dev
        for v in list(plain.values()) + ([] if counts is None else [counts]):
            v.setflags(write=False)
        self.group_of_path = np.repeat(batch.sample_group, 312)
        self.E_of_path = np.repeat(batch.edgel_counts[batch.sample_group], 312)

    @classmethod
    def on_device(cls, problem, tracker, ds, samples, interleave=False, edgel_counts=None, plain=None, joint=False):
        from trifocal_pose_estimation_using_improved_gpuhc_amd import pose
        from trifocal_pose_estimation_using_improved_gpuhc_amd.multi import TripletBatch
        batch = TripletBatch(problem, ds, seeds=0, samples_per_triplet=samples, interleave=interleave,
                             edgel_counts=edgel_counts)
        dev = batch.to(tracker.device)
        plain_dev = plain if plain is not None else tracker.track(batch.target, batch.diff)
        counts = pose.pose_support_joint_grouped(plain_dev.tracks, plain_dev.converge, dev)[0] if joint else None
        return cls(batch, plain_dev.host(), counts, dev, plain_dev)


def oracle_score(oracle):
    """score of check_group_result for the grouped abort launch: every found
    path passes the oracle's score_hypothesis on its own triplet, with the
    inlier counts the launch reports."""
    def score(r, case, ids, trk):
        st = r["stats"]
        for p in ids:
            t = int(case.group_of_path[p])
            ok, i21, i31 = oracle.score_hypothesis(r["tracks"][p], case.batch.locations[t], case.batch.Ks[t])
            assert ok == 1 and (st["inliers21"][p], st["inliers31"][p]) == (i21, i31), p
    return score


def passes_gate(counts, E, gate):
    """The gate in double, as the kernel states it (the ratio is a float32)."""
    return counts.astype(np.float64) >= float(np.float32(gate)) * E.astype(np.float64)


def gate_score(gate):
    """score of check_group_result for the gated launch, with case.counts in
    the oracle's place: the found paths are exactly the tracked paths whose
    joint count meets the gate, and every tracked path carries its counts."""
    def score(r, case, ids, trk):
        ref, st, ji = case.counts, r["stats"], r["joint_inliers"]
        assert ji.shape == trk.shape and ji.dtype == np.int32
        scored = trk & (ref[:, 0] >= 0)
        expect = np.nonzero(scored & passes_gate(ref[:, 0], case.E_of_path, gate))[0]
        assert ids.tolist() == expect.tolist()
        assert np.array_equal(ji[trk], ref[trk, 0])            # -1 where not scored
        assert np.array_equal(st["inliers21"][trk], np.maximum(ref[trk, 1], 0))
        assert np.array_equal(st["inliers31"][trk], np.maximum(ref[trk, 2], 0))
    return score


def check_group_result(r, case, start_sols, score, found, expect_ids, all_tracked=(), none_tracked=(),
                       tick_groups=None):
    """The checks of a grouped abort-mode result r (host dict) of case's batch.
    score(r, case, ids, tracked): oracle_score or gate_score, the one part in
    which the two launches differ.  found: the expected flags; expect_ids: the
    expected set of batch_index entries (None: a non-empty set within the
    finding groups); all_tracked / none_tracked: groups whose paths must all /
    must none be tracked; tick_groups: the groups that found in this launch
    (default: those flagged).  Returns `tracked`."""
    b, plain = case.batch, case.plain
    assert r["found"].tolist() == found
    ids = found_ids(r)
    if expect_ids is not None:
        assert set(ids.tolist()) == set(expect_ids)
    else:
        assert len(ids) > 0
    trk = tracked(r)
    tick_groups = [t for t, f in enumerate(found) if f] if tick_groups is None else tick_groups
    assert set(case.group_of_path[ids].tolist()) == set(tick_groups)
    assert trk[ids].all() and (r["converge"][ids] == 1).all()
    score(r, case, ids, trk)
    # every tracked path is the plain launch's path of the same batch id, every other one untouched
    assert_same_run(r, plain["tracks"], plain["converge"], plain["infinity"], plain["stats"]["steps"],
                    plain["stats"]["corrections"], where=trk)
    assert_untouched(r, start_sols, ~trk, allow_empty=True)
    for t in all_tracked:
        assert trk[b.path_index(t)].all(), f"group {t}: {(~trk[b.path_index(t)]).sum()} paths not tracked"
    for t in none_tracked:
        assert not trk[b.path_index(t)].any(), f"group {t}: {trk[b.path_index(t)].sum()} paths tracked"
    ticks = r["found_ticks"]
    assert [t for t in range(b.num_groups) if ticks[t] != 0] == sorted(tick_groups)
    return trk


# ---- kernel choice ------------------------------------------------------------

# Tracking launches run the latency-mode kernel (k_track_small) when they fill
# at most half of the path slots (N <= 16 samples), the throughput kernel
# (k_track) otherwise (hc_trifocal_set_small_launch: 0 by size, 1 always small,
# -1 never).
KERNEL_BY_SIZE, SMALL_ALWAYS, SMALL_NEVER = 0, 1, -1


@contextlib.contextmanager
def launch_mode(L, small=KERNEL_BY_SIZE, reuse=True):
    """Kernel choice and the retry-reuse switch for the launches inside; the defaults after."""
    try:
        L.hc_trifocal_set_small_launch(small)
        L.hc_trifocal_set_retry_reuse(1 if reuse else 0)
        yield
    finally:
        L.hc_trifocal_set_small_launch(KERNEL_BY_SIZE)
        L.hc_trifocal_set_retry_reuse(1)


# ---- small builders and readers ---------------------------------------------------

def scaled_samples(problem, tgt0, order=(0, 40, 70)):
    """The inputs that reach the tracker's dense re-solve: one sample per entry
    e of order, tgt0's target parameters times 2^e (0: tgt0 itself).  The
    Jacobians of a scaled sample pass 2^64 within the first steps and most of
    its paths run to infinity.  Returns (target, diff)."""
    T = np.stack([(tgt0 * np.float32(2.0 ** e)).astype(np.float32) for e in order])
    D = (T - problem.start_params[None]).astype(np.float32)   # prepare_target_params' diff
    return T, D


@functools.lru_cache(maxsize=None)
def noisy_data(seed=NOISE_SEED):
    """Dataset 000 with sigma = 1 px noise on its edgels (read-only)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data, synthcurves
    d = synthcurves.noisy(load_ransac_data(0), 1.0, seed)
    d.locations.setflags(write=False)
    return d


def ring_counters(tracker, workspace=None):
    """(head, tail, avail) of the suspend ring after a launch: the counters
    behind the base workspace (KArgs::rq words 0, 64, 128).  tail counts the
    suspensions; a drained ring has head == tail and avail == 0."""
    ws = tracker.workspace if workspace is None else workspace
    off = int(tracker.L.hc_trifocal_workspace_size())
    rq = np.frombuffer(ws[off:off + 768].cpu().numpy().tobytes(), np.uint32)
    return int(rq[0]), int(rq[64]), int(rq[128])


def ring_epoch(tracker, workspace=None):
    """The ring epoch (KArgs::rq word 192), which k_prep_tables bumps on a
    sliced launch only: 0 in a new workspace, one more after every launch that
    ran with time slicing, unchanged by one that fell back to an unsliced run.
    The workspace must have been made for slicing (new_workspace(n > 0))."""
    ws = tracker.workspace if workspace is None else workspace
    off = int(tracker.L.hc_trifocal_workspace_size()) + 4 * 192
    assert ws.numel() >= off + 4, "a workspace without the time-slicing area"
    return int(np.frombuffer(ws[off:off + 4].cpu().numpy().tobytes(), np.uint32)[0])


def last_suspensions(tracker, num_samples, workspace):
    """The step-control words of every path's suspend block after a sliced
    launch of num_samples samples on workspace (made by new_workspace(num_samples)
    and used by that launch only): what the path's last suspension packed
    (hc_layout.hpp: word 31 = stepidx | nsteps << 16, ncorr | succ << 16 |
    end_zone << 30 | check << 31; a running path's kept slope overwrites words
    0..29 only).  A path that was never suspended has an all-zero word.  The
    blocks are the last 256 B per path of the time-slicing area."""
    paths = 312 * num_samples
    total = int(tracker.L.hc_trifocal_workspace_size_for_steps(num_samples, tracker.settings.max_steps))
    assert workspace.numel() == total, "the workspace was not made for this launch size"
    blocks = np.frombuffer(workspace[total - 256 * paths:].cpu().numpy().tobytes(), np.uint32).reshape(paths, 64)
    w2, w3 = blocks[:, 62].astype(np.int64), blocks[:, 63].astype(np.int64)
    return dict(suspended=(w2 | w3) != 0, stepidx=w2 & 0xFFFF, nsteps=w2 >> 16, ncorr=w3 & 0xFFFF,
                succ=(w3 >> 16) & 0x3FFF, end_zone=(w3 >> 30) & 1, check=(w3 >> 31) & 1)


def run_cli(tmp_path, *args, timeout=300):
    """bin/magmaHC-main on a copy of data/ under tmp_path (made on the first
    call).  Returns (stdout, read) with read(name) the text of
    Output_Write_Files/<name>."""
    assert os.path.exists(CLI), "CLI not built"
    data = os.path.join(tmp_path, "data")
    if not os.path.exists(data):
        shutil.copytree(os.path.join(ROOT, "data"), data)
    out = subprocess.run([CLI, "-p", "trifocal_2op1p_30x30", "-d", str(tmp_path), *args], capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout + out.stderr

    def read(name):
        with open(os.path.join(tmp_path, "Output_Write_Files", name)) as fh:
            return fh.read()
    return out.stdout, read
