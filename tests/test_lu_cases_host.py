"""What the constructed LU systems (tests/lu_cases.py) cover, per instantiation of
the tracker's sparse solve, accounted from the oracle's trace
(oracle.cgesv_gpu_trace) on the CPU: tests/test_gpu_lu_variants.py runs the
batch, this file says which exit of which pivot step each system takes.

A system counts for (step, exit) in a variant only if neither it nor its wave
partner (the other half of the wave: index ^ 1) raises `redo` there, since
`redo` is wave-uniform and sends both halves to the dense solve."""
import numpy as np
import pytest

import lu_cases
from conftest import same
from lu_cases import NV

LATE = range(18, 29)   # step 29 has one eligible row and so no tie


@pytest.fixture(scope="module")
def full(problem, oracle, samples100):
    return lu_cases.full_batch(problem, oracle, samples100)


def test_traced_oracle_equals_the_untraced_one(full, oracle):
    """One body: the trace pointer changes nothing in x, on the whole batch."""
    for i in range(len(full["A"])):
        x = oracle.cgesv_gpu(full["A"][i], full["b"][i])
        assert (x.view(np.uint32) == full["ref"][i].view(np.uint32)).all(), full["names"][i]


def test_trace_records_the_search(oracle):
    """The trace on a system whose pivots are known: a permuted diagonal with a
    tie of three at step 1, a zero column 3, a NaN away from position 7 at step
    7, and then a NaN at position 9."""
    A = np.zeros((NV, NV, 2), np.float32)
    perm = np.roll(np.arange(NV), 1)           # row perm[c] holds column c: row 29 first, then 0, 1, ...
    for c in range(NV):
        A[perm[c], c, 0] = 2.0 + c
    A[10, 1] = (0.0, -3.0); A[20, 1] = (1.0, 2.0)          # keys 3, 3 against row 0's 3
    A[:, 3] = 0.0
    b = np.ones((NV, 2), np.float32)
    A1 = A.copy()
    A1[15, 7, 1] = np.nan                                  # row 15 holds position 15, not 7
    x, t = oracle.cgesv_gpu_trace(A1, b)
    assert same(x, oracle.cgesv_gpu(A1, b)).all()
    assert int(t[0]["row"]) == 29 and t[0]["equal"] == 1 and t[0]["key_bits"] == np.float32(2.0).view(np.int32)
    # step 1: rows 0 (position 29 after step 0), 10 and 20 tie on 3; the lowest position is row 10's
    assert t[1]["equal"] == 3 and int(t[1]["row"]) == 10 and t[1]["key_bits"] == np.float32(3.0).view(np.int32)
    assert lu_cases.holder_of_position(t, 1) == 1 and lu_cases.holder_of_position(t, 2) == 2
    assert lu_cases.holder_of_position(t, 29) == 0
    assert t[3]["key_bits"] == 0 and t[3]["equal"] == NV - 3 and t[3]["nans"] == 0
    assert t[7]["nans"] == 1 and t[7]["nan_at_step"] == 0
    kinds = dict(lu_cases.rare_steps(t))
    assert kinds[1] == "tie" and kinds[3] == "range" and kinds[7] == "nan" and 0 not in kinds and 2 not in kinds
    # NaN at the step's own position wins the step
    q = lu_cases.holder_of_position(oracle.cgesv_gpu_trace(A, b)[1], 9)
    A2 = A.copy()
    A2[q, 9, 0] = np.nan
    t2 = oracle.cgesv_gpu_trace(A2, b)[1]
    assert t2[9]["nan_at_step"] == 1 and int(t2[9]["row"]) == q and t2[9]["nans"] == 1


def test_every_system_lies_on_the_pattern(full):
    _, _, mask = lu_cases.structure()
    gA, gb = lu_cases.golden_late_ties()
    assert 2 <= len(gA) <= 32 and len(gA) % 2 == 0 and gA.dtype == np.float32 and gb.dtype == np.float32
    for k, A in enumerate(gA):
        assert not (A[~mask] != 0).any(), f"fixture {k}"
    for A, name in zip(full["A"], full["names"]):
        assert not (A[~mask] != 0).any(), name
    assert len(full["A"]) % 2 == 0 and len(full["A"]) <= 160


def test_the_fixture_holds_what_isolation_cannot_build(oracle):
    """golden/lu_late_ties.npz: a tie at step 26, a tie of three or more rows at
    each of the steps 18..23 and a tie won by a row that lacks the column
    structurally (fill-in); every system clean at steps 0..17, every pivot in
    the fast range."""
    _, _, mask = lu_cases.structure()
    gA, gb = lu_cases.golden_late_ties()
    tied, wide, fill_in = set(), set(), 0
    for k in range(len(gA)):
        t = oracle.cgesv_gpu_trace(gA[k], gb[k])[1]
        rare = lu_cases.rare_steps(t)
        assert rare and all(kind == "tie" and step >= 18 for step, kind in rare), f"fixture {k}: {rare}"
        assert not lu_cases.raises_redo(gA[k], t, fused=True), f"fixture {k}"
        for step, _ in rare:
            tied.add(step)
            if t[step]["equal"] >= 3:
                wide.add(step)
            fill_in += not mask[int(t[step]["row"]), step]
    assert 26 in tied
    assert set(range(18, 24)) <= wide
    assert fill_in >= 1


def _coverage(full, fused):
    """(ties, orders): the steps with a kept-sparse tie, and per step the winner
    orders of the kept-sparse ties built by isolation."""
    n = len(full["A"])
    redo = [lu_cases.raises_redo(full["A"][i], full["trace"][i], fused) for i in range(n)]
    ties, orders = set(), {}
    for i in range(n):
        if redo[i] or redo[i ^ 1]:
            continue
        for step, kind in lu_cases.rare_steps(full["trace"][i]):
            ties.add(step)
        e = full["expect"][i]
        if e is not None and e[0] == "tie":
            orders.setdefault(e[1], set()).add(e[2])
    return ties, orders, redo


@pytest.mark.parametrize("fused", [False, True], ids=["sequential", "fused"])
def test_kept_sparse_ties_cover_the_steps(full, fused):
    """The seven sequential variants: a kept-sparse tie at every step 0..28 (the
    ties of the fused-step batch serve 0..17).  The fused variant hands every
    tie at steps 0..17 to the dense solve, so it needs the steps 18..28, from
    systems that are clean at 0..17.  Both: steps 18..28 in both winner orders,
    except step 26, where one tie suffices."""
    ties, orders, _ = _coverage(full, fused)
    for step in (LATE if fused else range(29)):
        assert step in ties, f"no kept-sparse tie at step {step}"
    for step in LATE:
        if step != 26:
            assert orders.get(step) == {"low", "high"}, f"step {step}: winner orders {orders.get(step)}"


def test_late_ties_are_what_they_say(full):
    """An isolation tie: exactly the two built rows tie on 8 at the stated step,
    which is the system's first rare condition; the winner is the stated one;
    every pivot in the fast range."""
    seen = 0
    for i, e in enumerate(full["expect"]):
        if e is None or e[0] != "tie":
            continue
        seen += 1
        t, name = full["trace"][i], full["names"][i]
        step, (ra, rb) = e[1], (int(v) for v in name.split()[3:5])
        rare = lu_cases.rare_steps(t)
        assert rare[0] == (step, "tie") and all(kind == "tie" for _, kind in rare), name
        assert t[step]["equal"] == 2 and t[step]["key_bits"] == np.float32(8.0).view(np.int32), name
        assert int(t[step]["row"]) == (ra if e[2] == "low" else rb) and ra < rb, name
        assert i % 2 == 0 or full["expect"][i ^ 1][0] == "tie", "paired with another kept-sparse tie"
    assert seen == 2 * len(lu_cases.LATE_TIES)


def test_every_listed_redo_exit_is_present(full):
    """Each `redo` exit at a late step, once, at the stated step as the system's
    first rare condition, at an even index beside a plain random partner that
    raises no `redo` of its own (so a normal half is re-solved densely)."""
    want = {("zero", 20), ("zero", 25), ("zero", 29), ("tiny", 19), ("tiny", 27), ("tiny", 29),
            ("nan at position", 22), ("nan elsewhere", 22), ("inf", 28), ("huge entry", 21)}
    got = set()
    for i, e in enumerate(full["expect"]):
        if e is None or e[0] != "redo":
            continue
        _, step, kind = e
        A, t, name = full["A"][i], full["trace"][i], full["names"][i]
        rare = lu_cases.rare_steps(t)
        assert all(s >= step for s, _ in rare), name
        if kind == "zero":
            assert rare[0] == (step, "range") and t[step]["key_bits"] == 0, name
        elif kind == "tiny":
            assert rare[0] == (step, "range") and 0 < t[step]["key_bits"] < 0x12800000, name
        else:
            assert lu_cases.entries_redo(A), name
            bad = ~np.isfinite(A) | (np.abs(np.nan_to_num(A, nan=0.0, posinf=0.0, neginf=0.0)) >= 2.0 ** 64)
            assert bad[:, step].any() and not bad[:, np.arange(NV) != step].any(), name
            if kind == "nan at position":
                assert t[step]["nan_at_step"] == 1, name
            if kind == "nan elsewhere":
                assert t[step]["nans"] >= 1 and t[step]["nan_at_step"] == 0, name
            if kind == "inf":
                assert np.isinf(A[:, step]).any(), name
            if kind == "huge entry":
                assert np.isfinite(A).all() and np.abs(A[:, step]).max() == 2.0 ** 70, name
        for fused in (False, True):
            assert lu_cases.raises_redo(A, t, fused), name
            assert i % 2 == 0 and not lu_cases.raises_redo(full["A"][i + 1], full["trace"][i + 1], fused), name
        got.add((kind, step))
    assert got == want
    # the largest pivot a sparse solve can reach at step 24 (lu_cases.late_cases says why not 2^120)
    (i,) = [i for i, e in enumerate(full["expect"]) if e is not None and e[0] == "sparse"]
    assert full["trace"][i][24]["key_bits"] >= np.float32(2.0 ** 57).view(np.int32)
    assert not lu_cases.raises_redo(full["A"][i], full["trace"][i], True)
    assert not lu_cases.raises_redo(full["A"][i + 1], full["trace"][i + 1], True)
