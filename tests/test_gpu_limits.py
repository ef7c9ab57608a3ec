"""The tracking kernels at step, correction and step-growth limits other than
the defaults 80 / 3 / 4, against the oracle at the same limits.

The bar is the project's (tests/checks.py): flags, step and correction counts
and every float of x[0..29] identical, +0 == -0 and NaN == NaN.  At the defaults
every counter the kernels carry, park in SlotState or pack into a suspend block
stays below 256 and `succ` below 4; the settings of limits_common.py take them
past that, and to both sides of every comparison with a limit in
hc_track_body.inc and hc_layout.hpp: the corrector's stage count and its
max_corr <= 0 exit, succ >= inc_steps at 0 and 1, the least-attained-service
priority m * 4 / (max_steps + 1), the ring's (max_steps + 1) / SLICE_Q + 1
entries per path, slice_fits' fall-back to an unsliced launch, and a retry with
a kept slope that meets the step limit.  What each setting reaches is asserted
on the oracle's run before a kernel is compared with it
(tests/test_limits_host.py says what the limits mean on the oracle).

Not covered: the max_steps < 16000 clause of slice_fits.  An oracle run at
16000 steps takes minutes.
"""
import os
import shutil

import numpy as np
import pytest

from checks import (KERNEL_BY_SIZE, ROOT, SMALL_NEVER, assert_bit_identical, assert_matches_oracle, assert_untouched,
                    found_ids, last_suspensions, launch_mode, ring_counters, ring_epoch, run_cli, tracked)
from limits_common import (ARCHIVED, CORR_FACTS, CORR_MAX, CORR_SLICED, CORR_UNSLICED, DEFAULT, INC_FACTS, INC_SLICED,
                           INC_UNSLICED, SETTING_IDS, SETTINGS, assert_facts, oracle_run, same_runs)

pytestmark = pytest.mark.gpu

_trackers = {}


def _tracker(problem, ransac0, setting):
    """A DeviceTracker at setting, one per setting for the module."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    if setting not in _trackers:
        t = DeviceTracker(problem, "cuda:0", max_steps=setting[0], max_corrections=setting[1],
                          delta_t_inc_steps=setting[2])
        t.set_ransac_data(ransac0)
        assert (t.settings.max_steps, t.settings.max_corrections, t.settings.delta_t_inc_steps) == setting
        _trackers[setting] = t
    return _trackers[setting]


# ---- 1. both kernels against the oracle, per setting ------------------------------

@pytest.mark.parametrize("mode", [KERNEL_BY_SIZE, SMALL_NEVER], ids=["latency_kernel", "throughput_kernel"])
@pytest.mark.parametrize("setting", list(SETTINGS), ids=SETTING_IDS)
def test_tracker_matches_oracle_at_setting(problem, oracle, samples100, ransac0, setting, mode):
    """2 samples (624 paths), abort off: fewer paths than path slots, so every
    path runs from its first step to its last on one slot."""
    tgt, dif, _ = samples100
    ref = oracle_run(oracle, problem, samples100, setting)
    assert_facts(ref, setting, SETTINGS[setting])
    t = _tracker(problem, ransac0, setting)
    with launch_mode(t.L, mode):
        r = t.track(tgt[:2], dif[:2]).host()
    assert_matches_oracle(r, ref)
    assert (r["tracks"][:, 30, 0] == 1.0).all()


def test_step_growth_after_zero_and_after_one_success_agree(problem, oracle, samples100, ransac0):
    """inc_steps 0 and 1: the oracle's two runs are one run, and so are the kernels'."""
    tgt, dif, _ = samples100
    a, b = (oracle_run(oracle, problem, samples100, s) for s in ((80, 3, 0), (80, 3, 1)))
    assert same_runs(a, b)
    ra, rb = (_tracker(problem, ransac0, s).track(tgt[:2], dif[:2]).host() for s in ((80, 3, 0), (80, 3, 1)))
    assert_bit_identical(ra, rb)


@pytest.mark.parametrize("setting,kw,facts", ARCHIVED, ids=["ph_codeopt-40-3-4", "ph-80-1-4"])
def test_archived_semantics_match_oracle_at_setting(problem, oracle, samples100, ransac0, setting, kw, facts):
    """The archived ..._PH_CodeOpt (no truncation) and ..._PH (explicit RK helpers) kernels."""
    tgt, dif, _ = samples100
    ref = oracle_run(oracle, problem, samples100, setting, **kw)
    assert_facts(ref, setting, facts)
    r = _tracker(problem, ransac0, setting).track(tgt[:2], dif[:2], **kw).host()
    assert_matches_oracle(r, ref)


def test_abort_mode_at_setting(problem, oracle, samples100, ransac0):
    """Abort mode at (200, 5, 2): every path it tracked equals the oracle's
    abort-off run at the same limits, every other one is untouched."""
    setting = (200, 5, 2)
    tgt, dif, _ = samples100
    ref = oracle_run(oracle, problem, samples100, setting)
    assert ref[3]["steps"].max() == 201 and ref[3]["corrections"].max() > 255
    t = _tracker(problem, ransac0, setting)
    r = t.track(tgt[:2], dif[:2], abort=True).host()
    t.workspace_status()
    trk = tracked(r)
    assert trk.sum() >= 312
    assert_matches_oracle(r, ref, where=trk)
    assert_untouched(r, problem.start_sols, ~trk, allow_empty=True)
    ids = found_ids(r)
    assert bool(r["found"]) == (len(ids) > 0)
    assert trk[ids].all() and (r["converge"][ids] == 1).all()


# ---- 2. both sides of slice_fits ----------------------------------------------------------

def _launch_on(t, tgt, dif, ws, mode=SMALL_NEVER):
    """One tracking launch of t on the workspace ws (default: by the throughput kernel); the host result."""
    import torch
    T, D = torch.from_numpy(tgt).to(t.device), torch.from_numpy(dif).to(t.device)
    r = t.allocate(tgt.shape[0])
    t.reset_tracks(r)
    with launch_mode(t.L, mode):
        t.launch(T, D, r, workspace=ws)
        torch.cuda.synchronize(t.device)
    t.workspace_status(ws)
    return r.host()


def _run_and_epoch(problem, oracle, samples100, ransac0, setting, sliced):
    """setting's launch of 1 sample on a new workspace large enough for slicing:
    the ring epoch goes 0 -> 1 if the launch was sliced and stays 0 if not, and
    the run equals its own oracle run either way."""
    tgt, dif, _ = samples100
    t = _tracker(problem, ransac0, setting)
    ws = t.new_workspace(1)
    assert ring_epoch(t, ws) == 0
    r = _launch_on(t, tgt[:1], dif[:1], ws)
    assert ring_epoch(t, ws) == (1 if sliced else 0), f"{setting}: sliced launch expected: {sliced}"
    if sliced:
        head, tail, avail = ring_counters(t, ws)
        assert head == tail and avail == 0
    ref = oracle_run(oracle, problem, samples100, setting, n=1)
    assert_matches_oracle(r, ref)
    return r, ref


def test_correction_count_at_the_slicing_threshold(problem, oracle, samples100, ransac0):
    """max_corrections * (max_steps + 2) < 65536 (the suspend block's 16 bits
    for ncorr): 799 * 82 is below and the launch is sliced, 800 * 82 is not and
    the launch falls back.  The one place where ncorr leaves 8 bits by far."""
    _, a = _run_and_epoch(problem, oracle, samples100, ransac0, CORR_SLICED, True)
    _, b = _run_and_epoch(problem, oracle, samples100, ransac0, CORR_UNSLICED, False)
    for s, ref in ((CORR_SLICED, a), (CORR_UNSLICED, b)):
        assert_facts(ref, s, dict(CORR_FACTS, corr_max=CORR_MAX[s]))
        assert ref[3]["steps"].max() <= 34
    assert not same_runs(a, b)


def test_step_growth_limit_at_the_slicing_threshold(problem, oracle, samples100, ransac0):
    """inc_steps < 16384 (the suspend block's 14 bits for succ): 16383 is
    sliced, 16384 is not; no path gets that far, so the two runs are one run."""
    ra, a = _run_and_epoch(problem, oracle, samples100, ransac0, INC_SLICED, True)
    rb, b = _run_and_epoch(problem, oracle, samples100, ransac0, INC_UNSLICED, False)
    assert_facts(a, INC_SLICED, INC_FACTS)
    assert same_runs(a, b)
    assert_bit_identical(ra, rb)


# ---- 3. suspend and resume with wide counters ---------------------------------------------

# (setting, samples) -> facts of the oracle's run of the 400 paths drawn from that launch.
# (400, 3, 1000) is the one setting where succ grows past a handful: it counts a path's run
# of accepted steps and only a rejection resets it.  No path reaches 1000, so the results
# do not expose its value: the comparisons with the oracle cover its field only indirectly,
# by the fields beside it (ncorr below, the two flags above) coming back intact.  What the
# blocks held of it is read back and checked for width and against nsteps, not for its value.
WIDE = {((300, 6, 2), 40): dict(steps_above_255=91, corr_above_255=99, conv=49, inf=48),
        ((400, 3, 1000), 40): dict(steps_above_255=165, corr_above_255=166, conv=0, inf=2),
        ((400, 3, 1000), 100): dict(steps_above_255=157, corr_above_255=157, conv=1, inf=3, steps_min=66),
        # the sliced side of the correction threshold: a rejected step alone makes 799 corrections
        ((80, 799, 4), 100): dict(steps_above_255=0, corr_above_255=271, conv=96, inf=151, steps_min=10, steps_max=81,
                                  corr_max=35245)}
# the counters that the case's suspend blocks must have held past 8 bits (the docstring below says why)
WIDE_IN_BLOCKS = {((400, 3, 1000), 100): ("nsteps", "ncorr", "succ"), ((80, 799, 4), 100): ("ncorr",)}


@pytest.mark.parametrize("setting,n", list(WIDE),
                         ids=["300-6-2-N40", "400-3-1000-N40", "400-3-1000-N100", "80-799-4-N100"])
def test_suspend_and_resume_with_wide_counters(problem, oracle, samples100, ransac0, setting, n):
    """More paths than the 10 240 path slots (40 samples: 12 480, 100 samples:
    31 200): paths are suspended and resumed, their counters packed into the
    suspend block (word 31: stepidx | nsteps << 16, ncorr | succ << 16 | flags
    << 30).  The sliced run equals the unsliced one bit for bit, its ring is
    drained, and 400 paths drawn across it, a quarter of them with more than
    255 steps and corrections, equal the oracle.

    How wide the packed counters get is read back from the blocks
    (checks.last_suspensions), not assumed.  A path is suspended only while
    others wait for a slot.  With 40 samples the 2 240 paths in excess of the
    slots have found one as soon as that many paths have ended, which is within
    the first few dozen steps of the rest: the blocks of these launches hold
    small counts only (printed below).  With 100 samples at (400, 3, 1000) no
    path ends before its 66th step and fewer than the 20 960 paths in excess
    end within 255 steps (the oracle's facts below: 157 of 400 go on, the
    excess is 67 % of the launch), so the rotation lasts past step 255 and the
    blocks must hold counts past 8 bits; that case asserts it, for succ too:
    with inc_steps = 1000 the step never grows back after a rejection, so a
    path that is still running after 255 steps got there by long runs of
    accepted small steps.  So does (80,
    799, 4) with 100 samples: two thirds of the launch must end before the
    rotation does, two thirds of the paths make more than 255 corrections (one
    rejected step makes 799), and the largest count is 35 245: the one case
    where ncorr fills its 16 bits.  (With 40 samples its blocks stayed below
    180 corrections: the rejections come after the first 18 steps.)"""
    tgt, dif, _ = samples100
    t = _tracker(problem, ransac0, setting)
    ws = t.new_workspace(n)
    a = _launch_on(t, tgt[:n], dif[:n], ws, KERNEL_BY_SIZE)
    head, tail, avail = ring_counters(t, ws)
    assert tail > 0, "no path was suspended"
    assert head == tail and avail == 0, "every suspended path was resumed"
    b = t.track(tgt[:n], dif[:n], time_slicing=False).host()
    t.workspace_status()
    assert_bit_identical(a, b)
    ids = np.sort(np.random.default_rng(7).choice(312 * n, 400, replace=False))
    ref = oracle.gpuhc_track_subset(ids, problem.start_sols, problem.start_params, tgt[:n], dif[:n],
                                    problem.unified_index,
                                    oracle.settings(max_steps=setting[0], max_corrections=setting[1],
                                                    inc_steps=setting[2]))
    assert_facts(ref, setting, WIDE[setting, n], where=ids)
    st = ref[3][ids]
    assert (st["corrections"] > 255).sum() >= 20
    assert (st["steps"] > 255).sum() >= 20 or setting[0] < 255
    assert_matches_oracle(a, ref, where=ids)
    # what the suspend blocks held at each path's last suspension
    blk = last_suspensions(t, n, ws)
    sus = blk["suspended"]
    wide = {k: int((blk[k][sus] > 255).sum()) for k in ("nsteps", "ncorr", "succ")}
    print(f"{setting} N={n}: {tail} suspensions of {int(sus.sum())} paths; last blocks: max nsteps "
          f"{blk['nsteps'].max()}, ncorr {blk['ncorr'].max()}, succ {blk['succ'].max()}; above 255: {wide}")
    assert sus.any() and sus.sum() <= tail
    # a block is written at a step boundary: as many steps begun as ended, none past the limit,
    # and no count beyond what the path ended with
    assert np.array_equal(blk["stepidx"][sus], blk["nsteps"][sus])
    assert (blk["nsteps"][sus] >= 3).all() and (blk["nsteps"][sus] <= a["stats"]["steps"][sus]).all()
    assert (blk["ncorr"][sus] <= a["stats"]["corrections"][sus]).all()
    assert (blk["ncorr"][sus] <= setting[1] * blk["nsteps"][sus]).all()
    assert (blk["succ"][sus] <= blk["nsteps"][sus]).all() and (blk["succ"][sus] < max(setting[2], 1)).all()
    for k in WIDE_IN_BLOCKS.get((setting, n), ()):
        assert wide[k] >= 20, f"{k} went through no suspend block with more than 8 bits"


# ---- 4. the solver class and the CLI ------------------------------------------------------------

def test_cli_reads_the_limits_from_the_settings_file(tmp_path, problem, oracle, samples100):
    """GPU_HC_Solver takes the three limits from gpuhc_settings.yaml: with 40 /
    2 / 2 written there, `magmaHC-main -n 2` reports the solution counts of the
    oracle's run at (40, 2, 2), which are not those at the defaults."""
    data = os.path.join(tmp_path, "data")
    shutil.copytree(os.path.join(ROOT, "data"), data)
    path = os.path.join(data, "problems", "trifocal_2op1p_30x30", "gpuhc_settings.yaml")
    with open(path) as fh:
        text = fh.read()
    for key, old, new in (("GPUHC_Max_Steps", 80, 40), ("GPUHC_Max_Correction_Steps", 3, 2),
                          ("GPUHC_Num_Of_Steps_to_Increase_Delta_t", 4, 2)):
        assert text.count(f"{key}: {old}\n") == 1
        text = text.replace(f"{key}: {old}\n", f"{key}: {new}\n")
    with open(path, "w") as fh:
        fh.write(text)
    _, read = run_cli(tmp_path, "-n", "2")
    stats = [int(v) for v in read("GPU_Sols_Statistics.txt").split()[:3]]
    expect, default = (oracle.count_solutions(*oracle_run(oracle, problem, samples100, s)[:3])
                       for s in ((40, 2, 2), DEFAULT))
    assert expect != default
    assert stats == list(expect)
