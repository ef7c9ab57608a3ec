"""CPU tests of the fused solve's compact row (hc_lu_struct.hpp LuRowForm,
include/lu/hc_lu_compact_testing.h).

The fill-in bound and the levels are derived again in Python from the row
patterns the library exports, as tests/test_lu_levels.py does; from them: a row
can hold at most one of the columns 0..17 per level, which columns those are,
and that the library's position map puts every entry a row can ever hold on
exactly one of its 16 positions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NV, SLOTS, WIDTH, FIRST_HIGH = 30, 4, 16, 18

# rows -> the low column it can hold at level 0, 1, 2, 3 (None: no column at that level)
TABLE = {
    (0, 1, 2): (2, None, None, None),
    (9, 10, 11): (5, None, None, None),
    (3, 4, 5, 12, 13, 14): (0, 3, 6, None),
    (6, 7, 8, 15, 16, 17): (1, 4, 7, None),
    (18, 19, 20): (8, 12, 13, 14),
    (24, 25, 26): (9, 12, 13, 14),
    (21, 22, 23): (10, 15, 16, 17),
    (27, 28, 29): (11, 15, 16, 17),
}


@pytest.fixture(scope="module")
def lib():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def derived(lib):
    """(pat, final, level): the exported row patterns, each row's bound after the
    last step (everything the row can hold during a solve, whatever the pivot
    order), and each step's level."""
    pat = [int(lib.hc_lu_struct_pattern(r)) for r in range(NV)]
    cur = list(pat)
    cand, level = [], []
    for i in range(NV):
        rows = [r for r in range(NV) if (cur[r] >> i) & 1]
        above = (0xFFFFFFFF << (i + 1)) & ((1 << NV) - 1)
        u = 0
        for r in rows:
            u |= cur[r]
        for r in rows:
            cur[r] |= u & above
        cand.append(set(rows))
    for j in range(NV):
        level.append(max([level[i] + 1 for i in range(j) if cand[i] & cand[j]], default=0))
    return pat, cur, level


def _low(bound):
    return [c for c in range(FIRST_HIGH) if (bound >> c) & 1]


def test_a_row_holds_at_most_one_low_column_per_level(derived):
    _, final, level = derived
    assert sorted(r for rows in TABLE for r in rows) == list(range(NV))
    for rows, want in TABLE.items():
        for r in rows:
            by_level = {}
            for c in _low(final[r]):
                assert level[c] < SLOTS, (r, c)
                assert level[c] not in by_level, f"row {r}: columns {by_level[level[c]]} and {c} at level {level[c]}"
                by_level[level[c]] = c
            assert tuple(by_level.get(lv) for lv in range(SLOTS)) == want, r


def test_the_position_map(lib, derived):
    _, final, _ = derived
    for rows, want in TABLE.items():
        for r in rows:
            got = [int(lib.hc_lu_compact_column(r, p)) for p in range(WIDTH)]
            assert got[:SLOTS] == [-1 if c is None else c for c in want], r
            assert got[SLOTS:] == list(range(FIRST_HIGH, NV)), r
            # column 18 on an even position: the pairs of columns 18..29 stay pairs
            assert got.index(FIRST_HIGH) % 2 == 0
            # everything the row can hold has exactly one position
            for c in range(NV):
                if (final[r] >> c) & 1:
                    assert got.count(c) == 1, (r, c)
            assert all(c == -1 or (final[r] >> c) & 1 or c >= FIRST_HIGH for c in got), r


def test_every_pattern_entry_lands_on_exactly_one_position(lib, derived):
    pat, _, _ = derived
    for r in range(NV):
        got = [int(lib.hc_lu_compact_column(r, p)) for p in range(WIDTH)]
        for c in range(NV):
            if (pat[r] >> c) & 1:
                assert got.count(c) == 1, (r, c)


def test_out_of_range_is_refused(lib):
    for r, p in ((-1, 0), (NV, 0), (31, 0), (0, -1), (0, WIDTH)):
        assert int(lib.hc_lu_compact_column(r, p)) == -2


def test_compact_header_matches_the_table_and_the_library(lib):
    """include/lu/hc_lu_compact_testing.h against _abi.LU_COMPACT_SIGNATURES and the
    library's exports; no prototype takes a stream (the hook blocks on the null
    stream), and the argument checks need no device."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    raw = open(os.path.join(ROOT, "include", "lu", "hc_lu_compact_testing.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = {name: (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
              for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M)}
    assert set(protos) == {s.name for s in _abi.LU_COMPACT_SIGNATURES} and len(protos) == 2
    assert len(_abi.LU_COMPACT_SIGNATURES) == 2
    assert "hcStream" not in src and "locks" in raw
    assert int(re.search(r"#define\s+HC_LU_COMPACT_WIDTH\s+(\d+)", src).group(1)) == _abi.LU_COMPACT_WIDTH == WIDTH
    scalars = {"int": C.c_int, "size_t": C.c_size_t}
    for s in _abi.LU_COMPACT_SIGNATURES:
        ret, params = protos[s.name]
        assert s.restype is C.c_int and ret in ("int", "hcStatus")
        assert len(params) == len(s.argtypes), s.name
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p:
                assert t is C.c_void_p, (s.name, k)
            else:
                assert t is scalars[p.split()[0]], (s.name, k, p)
        fn = getattr(lib, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert {s.name for s in _abi.LU_COMPACT_SIGNATURES} <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    f = lib.hc_trifocal_compact_rows_batched
    buf = (C.c_char * 64)()
    a = C.cast(buf, C.c_void_p)
    ok_ptrs = (a,) * 10
    assert f(-1, *ok_ptrs, a, 1 << 30) == 1
    assert f(0, *ok_ptrs, a, 0) == 2                      # no room for the workspace
    assert f(0, *ok_ptrs, None, 1 << 30) == 2
    assert f(0, *((None,) * 10), a, 1 << 30) == 0         # n == 0 succeeds
    for k in range(10):
        ptrs = list(ok_ptrs)
        ptrs[k] = None
        assert f(4, *ptrs, a, 0) == 1, k


def test_the_gpu_batch_is_what_it_says(oracle):
    """compact_cases.batch by the oracle's trace: every candidate row of every
    fused step is the pivot row in its system, on the sparse path; the two redo
    systems leave it where they say, beside a partner that would not."""
    import compact_cases
    import lu_cases
    B = compact_cases.batch(oracle)
    pat, cand, mask = lu_cases.structure()
    assert len(B["A"]) == 94 and len(B["forced"]) == 90
    assert sorted(B["forced"]) == sorted((s, r) for s in range(FIRST_HIGH) for r in cand[s])
    for (s, r), i in B["forced"].items():
        assert int(B["trace"][i][s]["row"]) == r
        assert not lu_cases.raises_redo(B["A"][i], B["trace"][i], fused=True), B["names"][i]
    # the chains that merge at level 1 are entered from both of their level-0 triples
    for s, lo, hi in ((12, (18, 19, 20), (24, 25, 26)), (15, (21, 22, 23), (27, 28, 29))):
        assert all((s, r) in B["forced"] for r in lo + hi)
    for i, step in B["redo"].items():
        assert i % 2 == 0 and lu_cases.rare_steps(B["trace"][i])[0] == (step, "range")
        assert lu_cases.raises_redo(B["A"][i], B["trace"][i], fused=True)
        assert not lu_cases.raises_redo(B["A"][i + 1], B["trace"][i + 1], fused=True)
    assert sorted(B["redo"].values()) == [5, 25]
    # every low entry of the pattern is non-zero, with a magnitude of its own
    for A in B["A"]:
        low = np.array([abs(A[r, c, 0]) + abs(A[r, c, 1]) for r in range(NV) for c in range(FIRST_HIGH) if mask[r, c]])
        assert (low > 0).all() and len(set(low.tolist())) == len(low)
