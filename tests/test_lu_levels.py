"""CPU tests of the tracker LU's independent pivot steps (hc_lu_struct.hpp, LU_LEVELS).

A pivot step reads and writes only its candidate rows, so two steps with
disjoint candidate sets commute exactly.  The library derives, at compile
time, each step's level in that dependency forest; these tests derive the
candidates, the fill-in bound and the levels again in Python from the
library's row patterns alone and hold the exports against them."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

NV = 30

# the fusable steps (candidates of one or two row triples) by
# level, and the rows each works on
LEVELS = [
    {0: (3, 4, 5, 12, 13, 14), 1: (6, 7, 8, 15, 16, 17), 2: (0, 1, 2), 5: (9, 10, 11), 8: (18, 19, 20),
     9: (24, 25, 26), 10: (21, 22, 23), 11: (27, 28, 29)},
    {3: (3, 4, 5, 12, 13, 14), 4: (6, 7, 8, 15, 16, 17), 12: (18, 19, 20, 24, 25, 26), 15: (21, 22, 23, 27, 28, 29)},
    {6: (3, 4, 5, 12, 13, 14), 7: (6, 7, 8, 15, 16, 17), 13: (18, 19, 20, 24, 25, 26), 16: (21, 22, 23, 27, 28, 29)},
    {14: (18, 19, 20, 24, 25, 26), 17: (21, 22, 23, 27, 28, 29)},
]


@pytest.fixture(scope="module")
def lib():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    return _abi.lib()


@pytest.fixture(scope="module")
def derived(lib):
    """(cand, bound, level) per step, from hc_lu_struct_pattern only."""
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
        cand.append(sum(1 << r for r in rows))
        bound.append(u & above)
    for j in range(NV):
        level.append(max([level[i] + 1 for i in range(j) if cand[i] & cand[j]], default=0))
    return cand, bound, level


def test_levels_match_an_independent_derivation(lib, derived):
    cand, bound, level = derived
    for i in range(NV):
        assert int(lib.hc_lu_candidates(i)) == cand[i], i
        assert int(lib.hc_lu_step_level(i)) == level[i], i
    # the bound is what the dead column groups are derived from (groups of 2 after
    # a leading single column when step + 1 is odd)
    for i in range(NV - 1):
        j, k = i + 1, 0
        while j < NV:
            ln = 1 if (k == 0 and (i + 1) & 1) else min(2, NV - j)
            assert (int(lib.hc_lu_group_class(i, k)) == 1) == ((bound[i] & (((1 << ln) - 1) << j)) == 0), (i, k)
            j, k = j + ln, k + 1
    assert int(lib.hc_lu_step_level(-1)) == -1 and int(lib.hc_lu_step_level(NV)) == -1


def test_members_of_a_level_are_pairwise_disjoint(lib):
    by_level = {}
    for i in range(NV):
        by_level.setdefault(int(lib.hc_lu_step_level(i)), []).append(i)
    for lv, steps in by_level.items():
        seen = 0
        for i in steps:
            c = int(lib.hc_lu_candidates(i))
            assert c != 0 and (c & seen) == 0, (lv, i)
            seen |= c


def test_levels_are_the_documented_forest(lib):
    """Steps 0..17 are a forest of depth 4; step 18 shares no row with steps 14
    and 17 and so is on level 3 with them, but it reduces over 15 rows, and from
    18 on every step depends on the one before."""
    for lv, members in enumerate(LEVELS):
        for step, rows in members.items():
            assert int(lib.hc_lu_step_level(step)) == lv, step
            assert int(lib.hc_lu_candidates(step)) == sum(1 << r for r in rows), step
    assert sorted(s for m in LEVELS for s in m) == list(range(18))
    assert [int(lib.hc_lu_step_level(i)) for i in range(18, NV)] == list(range(3, 15))
    for i in range(18, NV):
        assert bin(int(lib.hc_lu_candidates(i))).count("1") in (15, 18, 30), i
    # the fusable steps are exactly those whose candidates are one or two triples
    assert [i for i in range(NV) if bin(int(lib.hc_lu_candidates(i))).count("1") <= 6] == list(range(18))


def test_lu_signature_table_matches_the_header_and_the_library(lib):
    """include/lu/hc_lu_testing.h against _abi.LU_SIGNATURES and the library's exports."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lu", "hc_lu_testing.h")).read(), flags=re.S)
    protos = {name: (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
              for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M)}
    assert set(protos) == set(_abi.LU_DECLARED_SYMBOLS) and len(protos) == 3
    assert len(_abi.LU_SIGNATURES) == 3, "a name is listed twice"
    # hcLuVariant against _abi.LU_VARIANTS: the same names with the same numbers
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r"\bHC_LU_VARIANT_(\w+)\s*=\s*(\d+)", src))
    assert enum.pop("count") == len(_abi.LU_VARIANTS) == 8
    assert enum == {name: k for k, name in enumerate(_abi.LU_VARIANTS)}
    returns = {"int": C.c_int, "hcStatus": C.c_int}
    for s in _abi.LU_SIGNATURES:
        ret, params = protos[s.name]
        assert s.restype is returns[ret], s.name
        assert len(params) == len(s.argtypes), s.name
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p or p.startswith("hcStream "):
                assert t is C.c_void_p, (s.name, k)
            else:
                assert p.startswith("int ") and t is C.c_int, (s.name, k, p)
        fn = getattr(lib, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert set(_abi.LU_DECLARED_SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert lib.hc_cgesv_30x30_struct_batched(-1, None, None, None, None) == 1
    assert lib.hc_cgesv_30x30_struct_batched(4, None, None, None, None) == 1
    assert lib.hc_cgesv_30x30_struct_batched(0, None, None, None, None) == 0
    for v in range(8):
        assert lib.hc_cgesv_30x30_variant_batched(v, -1, None, None, None, None) == 1
        assert lib.hc_cgesv_30x30_variant_batched(v, 4, None, None, None, None) == 1
        assert lib.hc_cgesv_30x30_variant_batched(v, 0, None, None, None, None) == 0
    for v in (-1, 8, 1 << 20):     # an unknown variant is refused, whatever the rest
        assert lib.hc_cgesv_30x30_variant_batched(v, 0, None, None, None, None) == 1
