"""CPU tests of the fused LU levels' row records (hc_lu_struct.hpp LU_ROWTAB,
include/lu/hc_lu_rowtable_testing.h).

The throughput tracker's solve reads, per level, one packed record per row from
LDS: the row's member (the pivot step whose candidates hold it), that step's
fill-in bound, its chain's pivot-row window, the row whose triple maximum it
takes across a 6-row chain, and its place in its lane triple.  The library
derives them at compile time from LU_LEVELS / LU_BOUND; these tests derive the
forest again in Python from the row patterns alone, as tests/test_lu_levels.py
does, and hold every field of every row and level against it."""
import ctypes as C
import os
import re
import subprocess

import pytest

import test_lu_levels as TL
from conftest import ROOT

NV = 30
ROWS, LEVELS = 32, 4
# the half's scratch (hc_lu_struct.hpp): row r's store window starts at entry 2r and
# holds 32 entries; the chains' pivot-row windows lie behind the last of them
CHAIN_WIN0 = 2 * 31 + 32
MEMBER, BOUND, WINDOW, PARTNER, PLACE, CHAIN = range(6)


@pytest.fixture(scope="module")
def lib():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def forest(lib):
    """Per level, {step: rows} of the fusable steps, and the bound per step:
    from hc_lu_struct_pattern only."""
    cur = [int(lib.hc_lu_struct_pattern(r)) for r in range(NV)]
    cand, bound, level = [], [], []
    for i in range(NV):
        rows = [r for r in range(NV) if (cur[r] >> i) & 1]
        above = (0xFFFFFFFF << (i + 1)) & ((1 << NV) - 1)
        u = 0
        for r in rows:
            u |= cur[r]
        for r in rows:
            cur[r] |= u & above
        cand.append(tuple(rows))
        bound.append(u & above)
    for j in range(NV):
        level.append(max([level[i] + 1 for i in range(j) if set(cand[i]) & set(cand[j])], default=0))
    levels = [{} for _ in range(LEVELS)]
    for i in range(NV):
        if 0 < len(cand[i]) <= 6:
            levels[level[i]][i] = cand[i]
    assert levels == TL.LEVELS, "the forest of tests/test_lu_levels.py"
    return levels, bound


def _field(lib, lv, r, f):
    return int(lib.hc_lu_row_field(lv, r, f))


def test_every_row_of_every_level(lib, forest):
    levels, bound = forest
    for lv, members in enumerate(levels):
        steps = sorted(members)
        seen_windows = set()
        for r in range(NV):
            mine = [s for s in steps if r in members[s]]
            assert len(mine) <= 1
            assert _field(lib, lv, r, PLACE) == r % 3, (lv, r)
            if not mine:
                assert _field(lib, lv, r, MEMBER) == -1 and _field(lib, lv, r, CHAIN) == -1, (lv, r)
                assert _field(lib, lv, r, BOUND) == 0 and _field(lib, lv, r, PARTNER) == r, (lv, r)
                assert _field(lib, lv, r, WINDOW) == 2 * r, (lv, r)
                continue
            step, k = mine[0], steps.index(mine[0])
            rows = members[step]
            assert _field(lib, lv, r, MEMBER) == step, (lv, r)
            assert _field(lib, lv, r, CHAIN) == k, (lv, r)
            assert _field(lib, lv, r, BOUND) == bound[step], (lv, r)
            assert bound[step] >> (step + 1) << (step + 1) == bound[step], "the bound lies above the pivot column"
            # chain k's window: 16 B (one column pair) after chain k - 1's, behind every row's own
            assert _field(lib, lv, r, WINDOW) == CHAIN_WIN0 + 2 * k, (lv, r)
            seen_windows.add(_field(lib, lv, r, WINDOW))
            # the same place in the chain's other triple
            if len(rows) == 3:
                partner = r
            else:
                lo, hi = rows[:3], rows[3:]
                assert lo == (lo[0], lo[0] + 1, lo[0] + 2) and hi == (hi[0], hi[0] + 1, hi[0] + 2) and lo[0] % 3 == 0 == hi[0] % 3
                partner = hi[lo.index(r)] if r in lo else lo[hi.index(r)]
            assert _field(lib, lv, r, PARTNER) == partner, (lv, r)
            assert partner % 3 == r % 3 and partner in rows
        assert len(seen_windows) == len(steps)
        assert max(2 * r + 32 for r in range(NV)) <= CHAIN_WIN0 <= min(seen_windows)


def test_the_pad_rows_are_neutral(lib):
    for lv in range(LEVELS):
        for r in (30, 31):
            assert _field(lib, lv, r, MEMBER) == -1 and _field(lib, lv, r, CHAIN) == -1
            assert _field(lib, lv, r, BOUND) == 0
            assert _field(lib, lv, r, WINDOW) == 2 * r      # its own window
            assert _field(lib, lv, r, PARTNER) == r         # itself
            assert _field(lib, lv, r, PLACE) == r % 3


def test_every_member_is_some_rows_member_exactly_once(lib, forest):
    """Steps 0..17 each appear at one level, in the rows of their candidates only."""
    levels, _ = forest
    where = {}
    for lv in range(LEVELS):
        for r in range(ROWS):
            m = _field(lib, lv, r, MEMBER)
            if m >= 0:
                where.setdefault(m, set()).add((lv, r))
    assert sorted(where) == list(range(18))
    for step, at in where.items():
        (lv,) = {l for l, _ in at}
        assert sorted(r for _, r in at) == list(levels[lv][step])


def test_out_of_range_is_refused(lib):
    for lv, r, f in ((-1, 0, 0), (LEVELS, 0, 0), (0, -1, 0), (0, ROWS, 0), (0, 0, -1), (0, 0, 6)):
        assert _field(lib, lv, r, f) == -2


def test_rowtable_header_matches_the_table_and_the_library(lib):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lu", "hc_lu_rowtable_testing.h")).read(), flags=re.S)
    protos = re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M)
    assert [(" ".join(ret.split()), name, [" ".join(p.split()) for p in params.split(",")]) for ret, name, params in protos] == \
        [("int", "hc_lu_row_field", ["int level", "int row", "int field"])]
    (s,) = _abi.LU_ROWTABLE_SIGNATURES
    assert s.name == "hc_lu_row_field" and s.restype is C.c_int and tuple(s.argtypes) == (C.c_int,) * 3
    fn = getattr(lib, s.name)
    assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r"\bHC_LU_ROW_(\w+)\s*=\s*(\d+)", src))
    assert enum.pop("field_count") == len(_abi.LU_ROW_FIELDS) == 6
    assert enum == {name: k for k, name in enumerate(_abi.LU_ROW_FIELDS)}
    assert "hcStream" not in src
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert "hc_lu_row_field" in {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
