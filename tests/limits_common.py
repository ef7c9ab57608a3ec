"""What tests/test_limits_host.py and tests/test_gpu_limits.py share: the
settings (GPUHC_Max_Steps, GPUHC_Max_Correction_Steps,
GPUHC_Num_Of_Steps_to_Increase_Delta_t) away from the defaults 80 / 3 / 4, what
the oracle's run of dataset 000's first samples (srand(0)) gives at each, and
those runs, computed once per setting and left unchanged.

At the defaults no path takes more than 81 steps, about 230 corrections or 3
consecutive successes; every setting below changes the outcome, and its facts
are asserted on the oracle's result (assert_facts) wherever a GPU run is
compared with it, so that no comparison passes on a run that did not reach
what the setting is for.
"""
import numpy as np

DEFAULT = (80, 3, 4)

# (max_steps, max_corrections, inc_steps) -> facts of the oracle's run of the
# first 2 samples (624 paths), abort off.  Keys of a fact dict: run_facts().
SETTINGS = {
    (0, 3, 4): dict(steps_min=1, steps_max=1, conv=0),                       # one step, then the limit
    (2, 3, 4): dict(steps_min=3, steps_max=3),                               # below SLICE_Q: ring of 1 entry per path
    (3, 3, 4): dict(steps_min=4, steps_max=4),                               # at SLICE_Q: 2 entries per path
    (40, 3, 4): dict(at_limit=284, conv=6, inf=16),                          # the limit met mid-path, also by a retry
    (200, 3, 4): dict(conv=69, inf=58, at_limit=137, corr_max=570),          # counters above 128
    (80, 0, 4): dict(steps_min=81, steps_max=81, corr_max=0, conv=0),        # no corrector: every step rejected
    (80, 1, 4): dict(conv=2, inf=4),                                         # the corrector ends on its first pass
    (80, 10, 4): dict(conv=78, inf=68, corr_max=663),                        # corrector stages past 3
    (80, 3, 0): dict(conv=61, inf=65),                                       # the step doubles after every success
    (80, 3, 1): dict(conv=61, inf=65),
    (80, 3, 8): dict(conv=45),                                               # slower growth
    (80, 3, 100): dict(steps_min=81, steps_max=81, conv=0),                  # the step never grows, succ above 3
    (300, 6, 2): dict(conv=60, inf=68, corr_max=1769),                       # all three, counters above 255
}
SETTING_IDS = ["-".join(str(v) for v in s) for s in SETTINGS]

# the archived semantics: (setting, oracle.settings keywords) -> facts, 2 samples
ARCHIVED = [((40, 3, 4), dict(truncate=False), dict(conv=44, inf=52)),
            ((80, 1, 4), dict(truncate=False, explicit_rk=True), dict(conv=19, inf=4))]

# both sides of slice_fits, 1 sample (312 paths): max_corrections * (max_steps + 2) below / at 65536 ...
CORR_SLICED, CORR_UNSLICED = (80, 799, 4), (80, 800, 4)
CORR_FACTS = dict(conv=78, inf=66, corr_above_255=169)     # of both; no path beyond 34 steps
CORR_MAX = {CORR_SLICED: 7927, CORR_UNSLICED: 7932}
# ... and inc_steps below / at 16384
INC_SLICED, INC_UNSLICED = (250, 3, 16383), (250, 3, 16384)
INC_FACTS = dict(conv=0, at_limit=117, corr_above_255=69)

_runs = {}


def oracle_run(oracle, problem, samples100, setting, n=2, **kw):
    """oracle.gpuhc_track of samples100's first n samples at setting (kw: the
    other oracle.settings keywords); one run per argument set, read-only."""
    key = (tuple(setting), n, tuple(sorted(kw.items())))
    if key not in _runs:
        tgt, dif, _ = samples100
        s = oracle.settings(max_steps=setting[0], max_corrections=setting[1], inc_steps=setting[2], **kw)
        ref = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt[:n], dif[:n], problem.unified_index, s)
        for a in ref:
            a.setflags(write=False)
        _runs[key] = ref
    return _runs[key]


def run_facts(ref, max_steps, where=None):
    """The counts the tables above state, of an oracle result (or of its paths `where`)."""
    _, conv, inf, st = ref
    sel = slice(None) if where is None else where
    steps, corr = st["steps"][sel], st["corrections"][sel]
    return dict(conv=int(conv[sel].sum()), inf=int(inf[sel].sum()), steps_min=int(steps.min()),
                steps_max=int(steps.max()), at_limit=int((steps == max_steps + 1).sum()), corr_max=int(corr.max()),
                steps_above_255=int((steps > 255).sum()), corr_above_255=int((corr > 255).sum()))


def assert_facts(ref, setting, expected, where=None):
    got = run_facts(ref, setting[0], where)
    assert {k: got[k] for k in expected} == expected, f"the oracle's run at {setting}: {got}"


def same_runs(a, b):
    """Two oracle results, bit for bit in flags, counts and all 31 track entries."""
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and
            np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]))
