"""What the label systems (tests/label_cases.py) do, accounted on the oracle
alone (CPU): tests/test_gpu_lu_bookkeeping.py solves them on the device.

A system counts for a family only if neither it nor its wave partner (index ^ 1)
raises `redo` in the fused solve, as in tests/test_lu_cases_host.py."""
import numpy as np
import pytest

import label_cases
import lu_cases
from label_cases import FAMILIES, TIE_STEPS


@pytest.fixture(scope="module")
def cases(oracle):
    return label_cases.systems(oracle)


def _counted(cases):
    n = len(cases["A"])
    redo = [lu_cases.raises_redo(cases["A"][i], cases["trace"][i], fused=True) for i in range(n)]
    return [i for i in range(0, n, 2) if not redo[i] and not redo[i + 1]]


def test_the_batch_is_paired_and_on_the_pattern(cases):
    _, _, mask = lu_cases.structure()
    n = len(cases["A"])
    assert n % 2 == 0 and 2 <= n <= 128
    assert cases["A"].dtype == np.float32 and cases["b"].dtype == np.float32
    for i in range(n):
        assert not (cases["A"][i][~mask] != 0).any(), cases["names"][i]
        if i % 2:   # the plain partner: nothing rare anywhere
            assert cases["tie"][i] is None and not lu_cases.rare_steps(cases["trace"][i]), cases["names"][i]


def test_every_system_is_the_tie_it_says(cases):
    """The tie of the two built rows on 8 at the stated step is the system's
    first rare condition, every rare condition is a tie at a late step, every
    pivot is in the fast range, and neither tied row was pivoted before."""
    for i in range(0, len(cases["A"]), 2):
        t, step, rows, name = cases["trace"][i], cases["tie"][i], cases["rows"][i], cases["names"][i]
        rare = lu_cases.rare_steps(t)
        assert step in TIE_STEPS and rare[0] == (step, "tie") and all(k == "tie" and s >= 18 for s, k in rare), name
        assert t[step]["equal"] == 2 and t[step]["key_bits"] == np.float32(8.0).view(np.int32), name
        assert int(t[step]["row"]) in rows, name
        assert not set(rows) & {int(t[s]["row"]) for s in range(step)}, name


def test_the_labels_decide_every_tie(cases):
    """The oracle's winner is the tied row at the lower replayed position, and
    the other row wins when the relabels of steps 0..17 are left out."""
    for i in range(0, len(cases["A"]), 2):
        d = label_cases.describe(cases["A"][i], cases["trace"][i], cases["tie"][i], cases["rows"][i])
        assert d["tracked"] == d["winner"], cases["names"][i]
        assert d["untracked"] != d["winner"], cases["names"][i]
        assert d == cases["info"][i]


def test_the_overlap_systems_need_the_second_pass(cases):
    """Overlap at level L: the holder of a member's position pivots another
    member of the level, and labels relabelled in one pass per level give the
    other winner."""
    for i in range(0, len(cases["A"]), 2):
        for fam in cases["info"][i]["families"]:
            if not fam.startswith("overlap"):
                continue
            lv = int(fam.split()[1])
            (fr, fc), _, waits = label_cases.OVERLAP[lv]
            t = cases["trace"][i]
            assert int(t[fc]["row"]) == fr and waits in cases["rows"][i], cases["names"][i]
            assert any(b == fc for _, b in label_cases.overlaps(t)[lv]), cases["names"][i]
            assert cases["info"][i]["single"] != cases["info"][i]["winner"], cases["names"][i]


def test_relabel_counts_are_what_the_families_say(cases):
    for i in range(0, len(cases["A"]), 2):
        fams, ch = cases["info"][i]["families"], cases["info"][i]["changes"]
        if "once" in fams:
            assert any(r < 18 and n == 1 for r, n in ch.items()), cases["names"][i]
        if "twice" in fams:
            assert any(r < 18 and n == 2 for r, n in ch.items()), cases["names"][i]


def test_every_family_has_a_counted_system(cases):
    counted = _counted(cases)
    for fam in FAMILIES:
        assert any(fam in cases["info"][i]["families"] for i in counted), f"no counted system for: {fam}"
    # an overlap at each of the levels 0, 1 and 2
    assert {fam for i in counted for fam in cases["info"][i]["families"]} >= {"overlap 0", "overlap 1", "overlap 2"}


def test_replays_agree_with_holder_of_position(cases):
    """label_cases.replay against lu_cases.holder_of_position, the replay the
    earlier LU tests use."""
    for i in range(0, len(cases["A"]), 2):
        t, step = cases["trace"][i], cases["tie"][i]
        rowid, _ = label_cases.replay(t, step)
        assert rowid.index(step) == lu_cases.holder_of_position(t, step)
        assert sorted(rowid) == list(range(lu_cases.NV))
