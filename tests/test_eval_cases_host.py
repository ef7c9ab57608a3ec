"""CPU tests of the inputs and references of tests/eval_cases.py, which the GPU
tests of the tracking kernels' evaluations (test_gpu_eval_variants.py) rest on,
and of the hook's header, binding and argument checks.

The fp64 bound.  A value is a sum of up to 16 terms; a term is at most one real
scaling (error u = 2^-24) and four complex products (each at most sqrt(5) u, no
FMA assumed), about 10 u, and the accumulations add up to 16 u: at most 27 u of
S = sum_j |term_j| to first order.  The bound is 32 u S.  The oracle's own worst
case is printed; it stays near 4 to 6 u.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import eval_cases as EC
from conftest import ROOT


@pytest.fixture(scope="module")
def own(problem):
    return EC.tables(problem)["own"]


@pytest.fixture(scope="module")
def finite_points(problem, samples100):
    return EC.concat([EC.path_points(problem, samples100, 192, 7), EC.scaled_points(problem, samples100)]).freeze()


def test_oracle_stays_within_the_fp64_bound(problem, oracle, own, finite_points):
    dx, dt, _ = own
    P, HX, HT, H = EC.oracle_values(oracle, problem, dx, dt, finite_points)
    ref_hx, ref_ht, ref_h = EC.fp64_values(dx, dt, finite_points.x, P, finite_points.diff)
    values = excluded = 0
    for name, val, ref in (("dH/dx", HX, ref_hx), ("dH/dt", HT, ref_ht), ("H", H, ref_h)):
        ok, exc, units = EC.bound_check(val, ref)
        print(f"{name}: worst {units.max():.2f} u, {int(exc.sum())} of {int((ref[1] > 0).sum())} values excluded")
        assert ok.all(), (name, np.argwhere(~ok)[:8], units.max())
        assert units.max() > 0.5, f"{name}: the comparison sees no rounding at all"
        values += int((ref[1] > 0).sum())
        excluded += int(exc.sum())
    share = excluded / values
    print(f"excluded share: {100 * share:.2f} % of {values} values")
    assert share <= 0.05


def test_fp64_reference_tells_a_wrong_term_apart(problem, oracle, own, finite_points):
    """The bound is tight enough to see one term of one entry dropped or one
    operand index off by one: the reference on a table with such an error is
    outside the bound of the oracle on the right table."""
    dx, dt, _ = own
    pts = finite_points.take(np.arange(24))
    P, HX, HT, H = EC.oracle_values(oracle, problem, dx, dt, pts)
    bad_dx = dx.copy().reshape(30, 8, 5, 30)
    c, j, r = np.argwhere(bad_dx[:, :, 0, :] != 0)[37]
    bad_dx[c, j, 3, r] = (bad_dx[c, j, 3, r] + 1) % 30
    bad_dt = dt.copy().reshape(16, 6, 30)
    bad_dt[9, 0, 4] = 0            # row 4's last term dropped
    ref_hx, ref_ht, ref_h = EC.fp64_values(bad_dx.reshape(-1), bad_dt.reshape(-1), pts.x, P, pts.diff)
    assert not EC.bound_check(HX, ref_hx)[0][:, r, c].all()
    assert not EC.bound_check(HT, ref_ht)[0][:, 4].all() and not EC.bound_check(H, ref_h)[0][:, 4].all()


def test_nonfinite_values_enter_only_through_real_terms(problem, oracle, samples100):
    """With x[k] not finite, the oracle's non-finite values are exactly those
    with a non-padding term that reads x[k] (the padding terms read p[33] and
    x[30] only), on every table: the GPU tests' healthy-row expectations."""
    pts = EC.nonfinite_points(problem, samples100)
    assert set(pts.bad_x) == set(range(30)) and len(pts) == 90
    assert np.isnan(pts.x).any() and np.isposinf(pts.x).any() and np.isneginf(pts.x).any()
    assert (np.isfinite(pts.x).reshape(len(pts), -1).sum(axis=1) == 61).all()
    for name, (dx, dt, _) in EC.tables(problem).items():
        _, HX, HT, H = EC.oracle_values(oracle, problem, dx, dt, pts)
        for i in range(len(pts)):
            ent, rows = EC.rows_reading(dx, dt, int(pts.bad_x[i]))
            assert (~np.isfinite(HX[i]).all(axis=-1) == ent).all(), (name, i)
            assert (~np.isfinite(HT[i]).all(axis=-1) == rows).all(), (name, i)
            assert (~np.isfinite(H[i]).all(axis=-1) == rows).all(), (name, i)


def test_threshold_bands_hold_what_they_should(problem, oracle, samples100, own):
    dx, dt, _ = own
    pts, band = EC.threshold_points(problem, samples100, oracle)
    assert [int((band == b).sum()) for b in range(3)] == [16, 16, 16]
    P, HX, _, _ = EC.oracle_values(oracle, problem, dx, dt, pts)
    (v, _), _, _ = EC.fp64_values(dx, dt, pts.x, P, pts.diff)
    for i in range(len(pts)):
        lo, hi = EC.BANDS[band[i]]
        assert 2.0 ** lo <= np.abs(HX[i]).max() < 2.0 ** hi
        if band[i] == 0:
            # every row's (and, the entries being packed over the lanes, any six entries')
            # sum of squares stays below 2^127 in fp64: the verdict must be true
            sq = np.sort((v[i].real ** 2 + v[i].imag ** 2).reshape(-1))
            assert sq[-6:].sum() < 2.0 ** 127
            assert ((v[i].real ** 2 + v[i].imag ** 2).sum(axis=1) < 2.0 ** 127).all()
            assert not EC.false_rows(HX[i]).any()
        else:
            assert EC.false_rows(HX[i]).sum() >= 8


def test_arrangements_cover_every_slot_kind_and_partner():
    idx, kind = EC.arrangement(48)
    assert EC.coverage(kind) == set(EC.COMBOS) and len(EC.COMBOS) == 48
    assert len(idx) % 8 == 0 and set(idx[kind != EC.IDLE]) == set(range(48))
    # a family that is no multiple of 48 still covers them, at any offset
    for m, off in ((90, 0), (56, 17), (248, 5)):
        idx, kind = EC.arrangement(m, off)
        assert EC.coverage(kind) == set(EC.COMBOS)
        own = [(i, k) for i, k in zip(idx, kind) if k != EC.IDLE]
        assert set(i for i, _ in own) == set(range(m))
    # fewer points than combinations do not
    assert EC.coverage(EC.arrangement(20)[1]) != set(EC.COMBOS)


def test_tables_put_owners_and_helpers_where_they_say(problem):
    t = EC.tables(problem)
    n = EC.ht_terms_per_row(t["own"][1])
    assert (n[:18] == 10).all() and list(n[18:]) == [16, 16, 13] * 4
    n = EC.ht_terms_per_row(t["owners_helpers"][1])
    assert (n[2:14] > 10).all() and (n[18:30] == 10).all() and (n[:2] == 10).all() and (n[14:18] == 10).all()
    dt_rej = EC.rejected_table(problem)[36000:]
    n = EC.ht_terms_per_row(dt_rej)
    assert n[2] == 16 and n[18] == 16       # lane ^ 16 partners, neither can help
    assert sorted(EC.ht_terms_per_row(t["swap_0_9"][1])) == sorted(EC.ht_terms_per_row(t["own"][1]))


def test_eval_signature_table_matches_the_header_and_the_library():
    """include/eval/hc_eval_testing.h against _abi.EVAL_SIGNATURES and the
    library's exports, and the argument checks that need no device."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    lib = _abi.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "eval", "hc_eval_testing.h")).read(), flags=re.S)
    protos = {name: (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
              for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M)}
    assert set(protos) == set(_abi.EVAL_DECLARED_SYMBOLS) and len(protos) == 1
    assert len(_abi.EVAL_SIGNATURES) == 1
    enum = dict((n.lower(), int(v)) for n, v in re.findall(r"\bHC_EVAL_VARIANT_(\w+)\s*=\s*(\d+)", src))
    assert enum.pop("count") == len(_abi.EVAL_VARIANTS) == 2
    assert enum == {name: k for k, name in enumerate(_abi.EVAL_VARIANTS)}
    assert int(re.search(r"#define\s+HC_EVAL_REDO\s+(\d+)u", src).group(1)) == _abi.HC_EVAL_REDO
    assert int(re.search(r"#define\s+HC_EVAL_KIND_IDLE\s+(\d+)", src).group(1)) == EC.IDLE
    scalars = {"int": C.c_int, "unsigned": C.c_uint, "size_t": C.c_size_t}
    for s in _abi.EVAL_SIGNATURES:
        ret, params = protos[s.name]
        assert ret == "hcStatus" and s.restype is C.c_int
        assert len(params) == len(s.argtypes), s.name
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p or p.startswith("hcStream "):
                assert t is C.c_void_p, (s.name, k)
            else:
                assert t is scalars[p.split()[0]], (s.name, k, p)
        fn = getattr(lib, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert set(_abi.EVAL_DECLARED_SYMBOLS) <= {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    # the argument checks: before any device work
    f = lib.hc_trifocal_eval_variant_batched
    buf = (C.c_char * 64)()
    a = C.cast(buf, C.c_void_p)
    ok_ptrs = (a,) * 10
    assert f(0, 0, 0, *ok_ptrs, a, 0, None) == 2               # no room for the workspace
    assert f(0, 0, 0, *ok_ptrs, None, 1 << 30, None) == 2
    for v in (-1, 2, 1 << 20):
        assert f(v, 0, 0, *ok_ptrs, a, 1 << 30, None) == 1     # an unknown variant, whatever the rest
    for fl in (2, 3, 1 << 31):
        assert f(0, fl, 0, *ok_ptrs, a, 1 << 30, None) == 1    # unknown flag bits
    for v in (0, 1):
        for fl in (0, 1):
            assert f(v, fl, -1, *ok_ptrs, a, 1 << 30, None) == 1
            assert f(v, fl, 0, *((None,) * 10), a, 1 << 30, None) == 0      # n == 0 succeeds
            for k in range(10):
                ptrs = list(ok_ptrs)
                ptrs[k] = None
                want = 2 if (k == 9 and v == 0) else 1         # PACKED does not write ent_ok: it may be null
                assert f(v, fl, 4, *ptrs, a, 0, None) == want, (v, fl, k)
