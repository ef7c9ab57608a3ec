"""Systems that make the row labels of the fused pivot steps 0..17 matter, for the
tests of the throughput tracker's LU alone (hc_lu_levels.hpp: the labels'
relabel of a level through the half's buffer): tests/test_label_cases_host.py
says on the oracle alone what each of them does, tests/test_gpu_lu_bookkeeping.py
solves them on the device.

A label is the position a row holds (dev-cgesv-batched-small.cuh:70-82: the
pivot row takes position I, the row that held I the pivot row's old position).
Before step 18 nothing reads the labels but the relabels themselves; from step
18 on the first-position rule of an exact tie reads them, and the pivot rows
hand theirs on.  Every system here ends in an exact two-way tie at step 18, 19,
21 or 22 (the steps whose ties the sparse solve resolves inline), built by
isolation as in lu_cases.late_cases: two rows that hold the column
structurally, their entries in the earlier pivot columns zeroed, (8, 0) against
(3, 5).  Neither is pivoted before the tie, so which of them holds the lower
position is decided by the relabels alone.  The winner is read from the
oracle's trace; the labels are replayed from the trace's pivot rows, once as the
reference keeps them and once under a mistake:
  * untracked: the relabels of steps 0..17 left out (labels at their initial
    values when step 18 begins);
  * single pass: a level's relabels applied at once, every row that holds a
    member's position taking that member's pivot row's label, without the rule
    for a holder that is itself the pivot row of another member of the level.

Families (a system is named by the first it serves, and may serve several):
  * overlap L (L = 0, 1, 2): at level L the holder of a member's position is the
    pivot row of another member of the level, the row that waits for that position
    is one of the tied rows, and the single-pass labels give the other winner.
    Level 0: row 5 pivots step 0 while it holds position 5; level 1: row 4 pivots
    step 3; level 2: row 13 pivots step 6 (forced by a large entry);
  * once, twice: a tied row r < 18 has been relabelled exactly once, twice
    before step 18;
  * handed on: a tied row received its position at a step I >= 18 from the
    pivot row of that step, whose own label had been changed in steps 0..17.
In every one the untracked labels give the other winner.  Each system stands at
an even index beside a plain random partner.
"""
import numpy as np

import lu_cases
from lu_cases import NV

TIE_STEPS = (18, 19, 21, 22)
FAMILIES = ("overlap 0", "overlap 1", "overlap 2", "once", "twice", "handed on")
FORCE = 64.0
# overlap at level L: (row, column) of the forced pivot, the columns of that row
# zeroed so that the entry reaches its step unchanged, and the row that waits
OVERLAP = {0: ((5, 0), (), 0), 1: ((4, 3), (0,), 3), 2: ((13, 6), (0, 3), 6)}

_cache = {}


def levels():
    """The fusable steps by level, from the library's exports."""
    if "levels" not in _cache:
        from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
        L = _abi.lib()
        out = {}
        for i in range(NV):
            if bin(int(L.hc_lu_candidates(i))).count("1") <= 6:
                out.setdefault(int(L.hc_lu_step_level(i)), []).append(i)
        _cache["levels"] = [out[lv] for lv in sorted(out)]
        assert sorted(s for m in _cache["levels"] for s in m) == list(lu_cases.FUSED)
    return _cache["levels"]


# ------------------------------------------------------------------ label replays
def replay(trace, upto, first=0):
    """(rowid, events): rowid[r], the position row r holds when step `upto`
    begins, replayed from the trace's pivot rows with the relabels of the steps
    before `first` left out; events[r]: the (step, label it lost, label it took)
    of every time row r was relabelled as the holder of a step's position."""
    rowid = list(range(NV))
    events = [[] for _ in range(NV)]
    for i in range(first, upto):
        pl, ql = int(trace[i]["row"]), rowid.index(i)
        mid = rowid[pl]
        rowid[pl] = i
        if ql != pl:
            events[ql].append((i, i, mid))
            rowid[ql] = mid
    return rowid, events


def replay_single_pass(trace, upto):
    """rowid when step `upto` (>= 18) begins, with each level's relabels applied
    at once and in one pass: the pivot rows take their members, and a row not
    pivoted that holds a member's position takes that member's pivot row's label
    as it was when the level began -- also where that label is another member's
    position, which the reference passes on once more."""
    rowid = list(range(NV))
    pivoted = set()
    for members in levels():
        piv = {int(trace[i]["row"]): i for i in members}
        old = {i: rowid[int(trace[i]["row"])] for i in members}
        new = list(rowid)
        for r in range(NV):
            if r in piv:
                new[r] = piv[r]
            elif r not in pivoted and rowid[r] in old:
                new[r] = old[rowid[r]]
        rowid = new
        pivoted |= set(piv)
    for i in range(18, upto):
        pl = int(trace[i]["row"])
        holders = [r for r in range(NV) if rowid[r] == i and r not in pivoted and r != pl]
        mid = rowid[pl]
        rowid[pl] = i
        pivoted.add(pl)
        if holders:
            rowid[holders[0]] = mid
    return rowid


def overlaps(trace):
    """The levels at which the holder of a member's position, when the level
    begins, is the pivot row of another member of the level: {level: [(member
    whose position is held, member the holder pivots)]}."""
    out = {}
    rowid = list(range(NV))
    for lv, members in enumerate(levels()):
        piv = {int(trace[i]["row"]): i for i in members}
        for i in members:
            h = rowid.index(i)
            if h in piv and piv[h] != i:
                out.setdefault(lv, []).append((i, piv[h]))
        # the level's relabels one after the other (any order gives the same)
        for i in members:
            pl, ql = int(trace[i]["row"]), rowid.index(i)
            mid = rowid[pl]
            rowid[pl] = i
            if ql != pl:
                rowid[ql] = mid
    return out


def winner(rowid, rows):
    """The first-position rule among the tied rows."""
    return min(rows, key=lambda r: rowid[r])


def describe(A, trace, step, rows):
    """What the labels do in a system whose first rare condition is the tie of
    `rows` at `step`: dict(winner, untracked, single, changes, families)."""
    tracked, events = replay(trace, step)
    untracked, _ = replay(trace, step, first=18)
    single = replay_single_pass(trace, step)
    w = int(trace[step]["row"])
    fam = set()
    ov = overlaps(trace)
    for lv, ((fr, fc), _, waits) in OVERLAP.items():
        held = levels()[lv]
        if waits in rows and int(trace[fc]["row"]) == fr and any(b == fc for _, b in ov.get(lv, [])) and \
                winner(single, rows) != w and fr in held:
            fam.add(f"overlap {lv}")
    early = {r: [e for e in events[r] if e[0] < 18] for r in rows}
    for r in rows:
        if r < 18 and len(early[r]) == 1:
            fam.add("once")
        if r < 18 and len(early[r]) == 2:
            fam.add("twice")
        late = [e for e in events[r] if e[0] >= 18]
        if late:
            # the label row r holds at the tie came from the pivot row of step late[-1][0]
            i = late[-1][0]
            p = int(trace[i]["row"])
            before, ev_p = replay(trace, i)
            if any(e[0] < 18 for e in ev_p[p]) and before[p] == late[-1][2] and tracked[r] == late[-1][2]:
                fam.add("handed on")
    return dict(winner=w, tracked=winner(tracked, rows), untracked=winner(untracked, rows), single=winner(single, rows),
                changes={r: len(early[r]) for r in rows}, families=fam)


# ------------------------------------------------------------------ the systems
def _tie_system(rng, oracle, step, rows, force=None):
    """A random system on the pattern with the isolated tie of `rows` at `step`
    (and the forced pivot of an overlap), its right-hand side and trace; None
    when the tie is not the system's only kind of rare condition, or not what
    was built."""
    pat, cand, mask = lu_cases.structure()
    A = lu_cases._random_on_pattern(rng, mask, 1)[0]
    b = rng.standard_normal((NV, 2)).astype(np.float32)
    if force is not None:
        (fr, fc), zero, _ = force
        for c in zero:
            A[fr, c] = 0.0
        A[fr, fc] = (FORCE, 0.0)
    ra, rb = rows
    lu_cases._isolate(A, pat, cand, rows, step)
    A[ra, step] = (8.0, 0.0)
    A[rb, step] = (3.0, 5.0)
    t = oracle.cgesv_gpu_trace(A, b)[1]
    rare = lu_cases.rare_steps(t)
    if not rare or rare[0] != (step, "tie") or any(k != "tie" for _, k in rare):
        return None
    if t[step]["equal"] != 2 or t[step]["key_bits"] != 0x41000000 or int(t[step]["row"]) not in rows:
        return None
    if lu_cases.raises_redo(A, t, fused=True):
        return None
    return A, b, t


def systems(oracle):
    """dict(A, b, names, ref, trace, tie, rows, info): at every even index a
    system that serves a family (names[i] says which), tie[i] its step, rows[i]
    the tied rows, info[i] what describe() says; at every odd index its plain
    partner (tie[i] = None).  At most 128 systems."""
    if "s" in _cache:
        return _cache["s"]
    pat, cand, mask = lu_cases.structure()
    rng = np.random.default_rng(2030)
    out = []

    def plain():
        for _ in range(50):
            A = lu_cases._random_on_pattern(rng, mask, 1)[0]
            b = rng.standard_normal((NV, 2)).astype(np.float32)
            t = oracle.cgesv_gpu_trace(A, b)[1]
            if not lu_cases.rare_steps(t):
                return A, b
        raise AssertionError("no plain partner drawn")

    def search(name, want, steps, pairs_of, force=None, draws=4000):
        for _ in range(draws):
            step = int(rng.choice(steps))
            rows = pairs_of(step)
            got = _tie_system(rng, oracle, step, rows, force)
            if got is None:
                continue
            A, b, t = got
            d = describe(A, t, step, rows)
            if want in d["families"] and d["untracked"] != d["winner"] and d["tracked"] == d["winner"]:
                out.append(dict(A=A, b=b, name=f"{name}: tie {step} rows {rows[0]} {rows[1]}", tie=step, rows=rows, info=d))
                pa, pb = plain()
                out.append(dict(A=pa, b=pb, name=f"plain beside {name}", tie=None, rows=None, info=None))
                return
        raise AssertionError(f"no draw gave: {name}")

    def structural_pair(step):
        rows = [r for r in cand[step] if (pat[r] >> step) & 1]
        return tuple(sorted(int(r) for r in rng.choice(rows, 2, replace=False)))

    # the overlap of each level: the waiting row ties at step 18 with another row that holds column 18
    for lv, force in OVERLAP.items():
        waits = force[2]
        others = [r for r in cand[18] if (pat[r] >> 18) & 1 and r != waits]
        for k in range(2):
            search(f"overlap {lv}", f"overlap {lv}", (18,),
                   lambda step, waits=waits, others=others: tuple(sorted((waits, int(rng.choice(others))))), force)
    for fam in ("once", "twice", "handed on"):
        for k in range(2):
            search(fam, fam, TIE_STEPS if fam != "handed on" else (19, 21, 22), structural_pair)
    A, b = np.stack([c["A"] for c in out]).astype(np.float32), np.stack([c["b"] for c in out]).astype(np.float32)
    assert len(A) % 2 == 0 and len(A) <= 128
    for M in A:
        assert not (M[~mask] != 0).any()
    sols = [oracle.cgesv_gpu_trace(A[i], b[i]) for i in range(len(A))]
    _cache["s"] = dict(A=A, b=b, names=[c["name"] for c in out], ref=np.stack([s[0] for s in sols]),
                       trace=[s[1] for s in sols], tie=[c["tie"] for c in out], rows=[c["rows"] for c in out],
                       info=[c["info"] for c in out])
    return _cache["s"]
