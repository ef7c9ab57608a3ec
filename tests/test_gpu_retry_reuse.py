"""Retry reuse (csrc/hc_track_body.inc): in a sliced tracking launch the retry of
a rejected step takes its first RK4 slope from the path's suspend block instead
of solving the same system again.  It changes which stages run, never what a
path computes: every run below equals the oracle, the committed golden run or
the run with the switch off value for value (+0 == -0, NaN == NaN), flags and
step / correction counts included.

On dataset 000, srand(0), 2 samples, 604 of the 624 paths reject at least one
step and 6 226 rejected steps are retried (6 311 on the held-out dataset 050).
100 samples is the smallest committed shape with more paths than path slots, so
suspensions fall between a rejection and its retry.
"""
import pytest

from checks import (KERNEL_BY_SIZE, SMALL_NEVER, assert_matches_golden, assert_matches_oracle, assert_same_run, golden,
                    launch_mode, scaled_samples)

pytestmark = pytest.mark.gpu


def assert_equal_runs(r, h):
    assert_same_run(r, h["tracks"], h["converge"], h["infinity"], h["stats"]["steps"], h["stats"]["corrections"])


@pytest.fixture(scope="module")
def oracle_ds000(problem, oracle, samples100):
    tgt, dif, _ = samples100
    return oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:2], dif[:2], problem.unified_index)


@pytest.fixture(scope="module")
def throughput_on(samples100, tracker):
    """Run 1b: 2 samples on the throughput kernel, reuse on."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER, True):
        return tracker.track(tgt[:2], dif[:2]).host()


@pytest.fixture(scope="module")
def scaled(problem, oracle, samples100):
    """The input of test_gpu_parity's dense re-solve test: sample 0 and its target
    parameters x 2^40 and x 2^70, whose systems go to the dense re-solve."""
    tgt, dif, _ = samples100
    T, D = scaled_samples(problem, tgt[0], (0, 40, 70))
    ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, T, D, problem.unified_index)
    assert ref[2][312:].sum() > 600 and ref[1][:312].sum() > 0   # the scaled samples diverge, sample 0 converges
    return T, D, ref


def test_small_launch_kernel_matches_oracle(samples100, tracker, oracle_ds000):
    """1a: k_track_small (the default at this size), reuse on."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, KERNEL_BY_SIZE, True):
        r = tracker.track(tgt[:2], dif[:2]).host()
    assert_matches_oracle(r, oracle_ds000)


def test_throughput_kernel_matches_oracle(throughput_on, oracle_ds000):
    """1b: the headline kernel, reuse on."""
    assert_matches_oracle(throughput_on, oracle_ds000)


def test_switch_off_equals_on(samples100, tracker, throughput_on):
    """2a: the throughput kernel with the switch off equals run 1b."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER, False):
        r = tracker.track(tgt[:2], dif[:2]).host()
    assert_equal_runs(r, throughput_on)


def test_unsliced_launch_equals_sliced(samples100, tracker, throughput_on):
    """2b: a base-size workspace has no suspend blocks: slicing, and with it the
    reuse, is off whatever the switch says, and the run equals run 1b."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, SMALL_NEVER, True):
        r = tracker.track(tgt[:2], dif[:2], time_slicing=False).host()
    assert_equal_runs(r, throughput_on)


def test_held_out_dataset_matches_oracle(problem, oracle, tracker):
    """3: dataset 050, which nothing was tuned on."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import load_ransac_data, prepare_target_params
    tgt, dif, _ = prepare_target_params(problem, load_ransac_data(50), seed=0, num_samples=2)
    ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt, dif, problem.unified_index)
    with launch_mode(tracker.L, KERNEL_BY_SIZE, True):
        r = tracker.track(tgt, dif).host()
    assert_matches_oracle(r, ref)


@pytest.mark.parametrize("reuse", [True, False], ids=["on", "off"])
def test_config2_matches_golden(samples100, tracker, reuse):
    """4a, 4b: config 2 (100 samples, more paths than slots) against the committed golden run."""
    tgt, dif, _ = samples100
    with launch_mode(tracker.L, KERNEL_BY_SIZE, reuse):
        r = tracker.track(tgt, dif).host()
    assert_matches_golden(r, golden("gpuhc_N100_seed0"))


@pytest.mark.parametrize("reuse", [True, False], ids=["on", "off"])
def test_dense_resolve_matches_oracle(tracker, scaled, reuse):
    """5a, 5b: a kept slope that came from the dense re-solve."""
    T, D, ref = scaled
    with launch_mode(tracker.L, KERNEL_BY_SIZE, reuse):
        r = tracker.track(T, D).host()
    assert_matches_oracle(r, ref)
