"""The P2C mode on the CPU: the coefficient map, the FP64 equivalence of the two
formulations, the host generator, the restatement (tests/p2c_ref) and the ABI
of include/p2c/hc_trifocal_p2c.h."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import checks
import p2c_common as pc
from conftest import ROOT
from p2c_common import EPS, p2c_ref

P2C_HEADER = os.path.join(ROOT, "include", "p2c", "hc_trifocal_p2c.h")

# the map the issue lists, to check the derivation against (the library holds none of it)
EXPECTED_MAP = ([(0, 30), (0, 31)] + [(a, 33) for a in range(9, 19)] + [(1, 30), (1, 31)] +
                [(a, 33) for a in range(19, 29)] + [(2, 33)] + [(a, 33) for a in range(29, 33)] +
                [(a, 33) for a in range(3, 7)] + [(6, 32), (7, 33), (7, 32), (8, 33), (33, 33)])


# ---- 1. the map -------------------------------------------------------------

def test_map_derived_from_the_fixtures_is_unique(problem):
    m = pc.fixture_map()
    assert m.shape == (38, 2) and m.dtype == np.int32
    assert tuple(m[37]) == (33, 33)
    assert len({tuple(p) for p in m.tolist()}) == 38, "one pair per coefficient"
    assert [tuple(p) for p in m.tolist()] == EXPECTED_MAP


def test_term_order_differs_between_the_formulations(problem):
    """138 of the 558 dH/dx terms and 22 of the 360 dH/dt terms sit at the PH tables' positions."""
    hx, ht = pc.fixture_tables()
    m = pc.fixture_map()
    hx = hx.reshape(30, 30, 8, 4)
    ht = ht.reshape(30, 16, 5)
    ph_x = np.asarray(problem.dHdx_index).reshape(30, 8, 5, 30).transpose(3, 0, 1, 2)
    ph_t = np.asarray(problem.dHdt_index).reshape(16, 6, 30).transpose(2, 0, 1)
    def same_place(p2c_t, ph):
        real = p2c_t[..., 0] != 0
        pair = np.sort(ph[..., 1:3], axis=-1)
        eq = (p2c_t[..., 0] == ph[..., 0]) & (m[p2c_t[..., 1]] == pair).all(-1) & \
             (np.sort(p2c_t[..., 2:], -1) == np.sort(ph[..., 3:], -1)).all(-1)
        return int(real.sum()), int((real & eq).sum())
    assert same_place(hx, ph_x) == (558, 138)
    assert same_place(ht, ph_t) == (360, 22)


def test_tables_from_ph_round_trip(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    hx, ht, m = pc.ph_tables()
    assert hx.shape == (28800,) and ht.shape == (2400,) and hx.dtype == ht.dtype == np.int32
    assert tuple(m[37]) == (33, 33) and m.tolist() == sorted(m.tolist())
    assert np.array_equal(p2c.derive_coeff_map(problem, hx, ht), m)
    # the same pairs as the fixtures' map, numbered differently
    assert {tuple(p) for p in m.tolist()} == set(EXPECTED_MAP)
    # terms keep the PH order
    ph_x = np.asarray(problem.dHdx_index).reshape(30, 8, 5, 30).transpose(3, 0, 1, 2)
    assert np.array_equal(hx.reshape(30, 30, 8, 4)[..., 0], ph_x[..., 0])
    assert np.array_equal(hx.reshape(30, 30, 8, 4)[..., 2:], ph_x[..., 3:])


def test_derive_coeff_map_rejects_tables_that_do_not_pair_up(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi, p2c
    hx, ht = (t.copy() for t in pc.fixture_tables())
    k = int(np.nonzero(hx.reshape(-1, 4)[:, 0] != 0)[0][0])
    hx.reshape(-1, 4)[k, 0] += 1          # another coefficient value: no PH term to pair with
    with pytest.raises(_abi.HCError):
        p2c.derive_coeff_map(problem, hx, ht)
    hx, ht = (t.copy() for t in pc.fixture_tables())
    ht.reshape(-1, 5)[ht.reshape(-1, 5)[:, 1] == 36, 1] = 34    # k = 36 no longer occurs, 34 stands for two pairs
    with pytest.raises(_abi.HCError):
        p2c.derive_coeff_map(problem, hx, ht)


# ---- 2. FP64 equivalence of the formulations ----------------------------------

def test_fp64_p2c_tables_equal_ph_tables_at_p_of_t(problem):
    """dH/dx, H, dH/dt of the P2C tables with coef(t) against the PH tables at
    p(t): all 312 start solutions perturbed by 1 %, 5 random t, a random target.
    Bound 1e-12 on max |difference| / max |value| per array (measured 1.4e-15;
    the margin covers sums of <= 16 products of 5 factors)."""
    rng = np.random.default_rng(0)
    hx, ht = pc.fixture_tables()
    s = pc.cplx(problem.start_params)
    tgt = s * (1.0 + 0.5 * (rng.standard_normal(34) + 1j * rng.standard_normal(34)))
    tgt[33] = 1.0
    d = tgt - s
    C0, C1, C2 = pc.coeffs64(pc.fixture_map(), s, d)
    X = pc.perturbed_start_sols(rng)
    worst = [0.0, 0.0, 0.0]
    for t in rng.uniform(0.0, 1.0, 5):
        p = s + t * d
        cHx, cHt = C0 + C1 * t + C2 * t * t, C1 + 2.0 * C2 * t
        for x in X:
            A, Ht, H, _, _ = pc.p2c_eval64(hx, ht, x, cHx, cHt)
            for i, (got, ref) in enumerate(zip((A, Ht, H), pc.ph_eval64(problem, x, p, d))):
                worst[i] = max(worst[i], float(np.abs(got - ref).max() / np.abs(ref).max()))
    print("fp64 P2C against PH (dH/dx, dH/dt, H):", worst)
    assert max(worst) <= 1e-12


# ---- 3. the generator ----------------------------------------------------------

def test_generator_equals_the_restatement_and_fp64(problem):
    """hc_p2c_coefficients == the restatement's generator bit for bit, and both
    within 8 * 2^-24 * (sum of the magnitudes of the products forming the
    coefficient) of FP64 (two roundings per product component and one per sum)."""
    from trifocal_pose_estimation_using_improved_gpuhc_amd import p2c
    m = pc.fixture_map()
    dif = pc.samples(100)[1]
    chx, cht = p2c.coefficients(m, problem.start_params, dif)
    rhx, rht = pc.blocks(100)
    assert chx.shape == (100, 38, 3, 2) and cht.shape == (100, 38, 2, 2)
    assert np.array_equal(chx.view(np.uint32), rhx.view(np.uint32))
    assert np.array_equal(cht.view(np.uint32), rht.view(np.uint32))
    s = pc.cplx(problem.start_params)
    a, b = m[:, 0], m[:, 1]
    for n in range(100):
        d = pc.cplx(dif[n])
        C0, C1, C2 = pc.coeffs64(m, s, d)
        M0 = np.abs(s[a]) * np.abs(s[b])
        M1 = np.abs(s[a]) * np.abs(d[b]) + np.abs(d[a]) * np.abs(s[b])
        M2 = np.abs(d[a]) * np.abs(d[b])
        got = pc.cplx(chx[n])
        for o, (ref, mag) in enumerate(((C0, M0), (C1, M1), (C2, M2))):
            assert (np.abs(got[:, o] - ref) <= 8 * EPS * mag).all(), (n, o)
        got = pc.cplx(cht[n])
        assert (np.abs(got[:, 0] - C1) <= 8 * EPS * M1).all(), n
        assert (np.abs(got[:, 1] - 2 * C2) <= 8 * EPS * 2 * M2).all(), n


def test_generator_rejects_bad_arguments(problem):
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    m = pc.fixture_map().copy()
    sp = np.ascontiguousarray(problem.start_params)
    dp = np.ascontiguousarray(pc.samples(2)[1][:1])
    hx, ht = np.zeros((1, 38, 3, 2), np.float32), np.zeros((1, 38, 2, 2), np.float32)
    L, p = _abi.lib(), _abi.ptr
    assert L.hc_p2c_coefficients(1, None, p(sp), p(dp), p(hx), p(ht)) == 1
    assert L.hc_p2c_coefficients(-1, p(m), p(sp), p(dp), p(hx), p(ht)) == 1
    assert L.hc_p2c_coefficients(1, p(m), p(sp), p(dp), None, p(ht)) == 1
    m[5, 1] = 34
    assert L.hc_p2c_coefficients(1, p(m), p(sp), p(dp), p(hx), p(ht)) == 1


# ---- 4. the restatement's evaluations --------------------------------------------

def test_restatement_eval_against_fp64(problem):
    """FP32 restatement against FP64 at the same FP32 coefficient blocks and
    points: per output |error| <= 64 * 2^-24 * sum |terms|, a term's coefficient
    counted as |C0| + |C1| t + |C2| t^2 (what its interpolation rounds against)."""
    rng = np.random.default_rng(1)
    hx, ht = pc.fixture_tables()
    chx, cht = pc.blocks(2)
    X = pc.perturbed_start_sols(rng).astype(np.complex64)
    n = X.shape[0]
    t = rng.uniform(0.0, 1.0, n).astype(np.float32)
    t[0], t[1] = 0.0, 1.0
    smp = np.arange(n) % 2
    xf = np.stack([X.real, X.imag], -1).astype(np.float32)
    HX, HT, H = p2c_ref.eval_batched(hx, ht, xf, chx[smp], cht[smp], t)
    for i in range(n):
        cx, ct, tt = pc.cplx(chx[smp[i]]), pc.cplx(cht[smp[i]]), float(t[i])
        cHx = cx[:, 0] + cx[:, 1] * tt + cx[:, 2] * tt * tt
        cHt = ct[:, 0] + ct[:, 1] * tt
        mHx = np.abs(cx[:, 0]) + np.abs(cx[:, 1]) * tt + np.abs(cx[:, 2]) * tt * tt
        mHt = np.abs(ct[:, 0]) + np.abs(ct[:, 1]) * tt
        A, Ht, Hh, Am, Hm = pc.p2c_eval64(hx, ht, pc.cplx(xf[i]), cHx, cHt, mHx)
        _, _, _, _, Htm = pc.p2c_eval64(hx, ht, pc.cplx(xf[i]), cHx, cHt, mHt)
        assert (np.abs(pc.cplx(HX[i]) - A) <= 64 * EPS * Am).all(), i
        assert (np.abs(pc.cplx(H[i]) - Hh) <= 64 * EPS * Hm).all(), i
        assert (np.abs(pc.cplx(HT[i]) - Ht) <= 64 * EPS * Htm).all(), i


def test_clamp_constant_is_the_ph_kernels():
    """1 - 0.05 == 0.95 in C double: the P2C clamp fabs(1 - 0.05 - t0) is the PH kernels' fabs(0.95 - t0)."""
    assert p2c_ref.one_minus_005() == 0.95 and 1 - 0.05 == 0.95


# ---- 5. the restatement's tracker ------------------------------------------------

def test_restatement_tracker_residual_against_ph_codeopt(problem, oracle, ransac0):
    """Measured: P2C 2.893e-07 on its own system (1 real path of 240 converged),
    PH_CodeOpt 1.095e-07 on its own (6 real of 222); P2C against p_target
    2.402e-05 (recorded, not gated: coef(1) reaches the small target values by
    cancelling start-sized terms).  Pose support over these 624 tracks: 1
    candidate, whose pose does not pass the residual check (informative).

    2 samples, seed 0, dataset 000.  The FP64 relative residual (tests/residual.py:
    |H_r| / sum |terms|) of every converged real path on the system P2C solves,
    coefficients C0 + C1 + C2 in FP64 from the FP32 blocks, against the same
    statistic of the oracle's PH_CodeOpt run on its own system: P2C <= 10 x PH
    (the factor allows for the different step sequences and the cancellation in
    coef(1))."""
    from residual import max_relative_residual, real_converged
    hx, ht = pc.fixture_tables()
    tgt, dif = pc.samples(2)
    chx, _ = pc.blocks(2)
    tr, conv, inf, st = pc.ref_track(2)
    ids = real_converged(tr, conv)
    assert len(ids) > 0
    h = ht.reshape(30, 16, 5)
    worst = 0.0
    for b in ids:
        c1 = pc.cplx(chx[b // 312]).sum(1)               # coef(1) = C0 + C1 + C2
        x = pc.cplx(tr[b]); x[30] = 1.0
        terms = h[..., 0] * c1[h[..., 1]] * x[h[..., 2]] * x[h[..., 3]] * x[h[..., 4]]
        scale = np.abs(terms).sum(-1)
        worst = max(worst, float((np.abs(terms.sum(-1)) / np.where(scale > 0, scale, 1.0)).max()))
    vs_target = max_relative_residual(problem.dHdt_index, tr, ids, tgt)
    ph = oracle.gpuhc_track(problem.start_sols, problem.start_params, tgt, dif, problem.unified_index,
                            oracle.settings(truncate=False))
    ph_ids = real_converged(ph[0], ph[1])
    ph_worst = max_relative_residual(problem.dHdt_index, ph[0], ph_ids, tgt)
    inl, sel = oracle.pose_support(tr, conv, ransac0.locations, ransac0.K)
    res, ok = oracle.pose_residuals(ransac0.pose21, ransac0.pose31, sel) if sel["num_candidates"] else (None, False)
    print(f"P2C: {int(conv.sum())} converged, {len(ids)} real, {int(inf.sum())} inf, "
          f"mean steps {st['steps'].mean():.2f}; residual on its own system {worst:.3e}, on p_target {vs_target:.3e}; "
          f"PH_CodeOpt: {int(ph[1].sum())} converged, {len(ph_ids)} real, residual {ph_worst:.3e}; "
          f"pose support: {sel['num_candidates']} candidates, selected pose passes: {ok} {res}")
    assert worst <= 10 * ph_worst


# ---- 6. the golden run ---------------------------------------------------------------

def test_restatement_reproduces_the_golden_runs_first_samples():
    g = checks.golden("gpuhc_p2c_N100_seed0")
    tr, conv, inf, st = pc.ref_track(2)
    r = dict(tracks=tr, converge=conv, infinity=inf, stats=st)
    checks.assert_matches_golden(r, g, rows=slice(0, 624))


# ---- the ABI of the P2C header ---------------------------------------------------------

def _prototypes():
    src = open(P2C_HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for ret, name, params in re.findall(r"^([A-Za-z_][\w\s\*]*?)\b(hc_\w+)\s*\(([^()]*)\)", src, flags=re.M):
        out[name] = (" ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")])
    return out


def test_p2c_signature_table_matches_the_header_and_the_library():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    protos = _prototypes()
    assert set(protos) == set(_abi.P2C_DECLARED_SYMBOLS) and len(protos) == 3
    scalars = {"int": C.c_int}
    for s in _abi.P2C_SIGNATURES:
        ret, params = protos[s.name]
        assert ret == "hcStatus" and s.restype is C.c_int
        assert len(params) == len(s.argtypes), s.name
        for k, (p, t) in enumerate(zip(params, s.argtypes)):
            if "*" in p or p.startswith("hcStream "):
                assert t is C.c_void_p or issubclass(t, C._Pointer), (s.name, k)
            else:
                assert t is scalars.get(" ".join(w for w in p.split()[:-1] if w != "const"),
                                        C.c_size_t if p.startswith("size_t ") else None), (s.name, k, p)
    exported = subprocess.run(["nm", "-D", "--defined-only", _abi.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    assert set(_abi.P2C_DECLARED_SYMBOLS) <= exported
    L = _abi.lib()
    for s in _abi.P2C_SIGNATURES:
        fn = getattr(L, s.name)
        assert fn.restype is s.restype and tuple(fn.argtypes) == tuple(s.argtypes)
    assert L.hc_trifocal_abi_version() == 2    # no struct of hc_trifocal.h changed


def test_p2c_struct_mirror_matches_the_header_by_the_c_compiler(tmp_path):
    import shutil
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    cc = next(c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c))
    fields = [f[0] for f in _abi.hcP2cArgs._fields_]
    args = "".join(f", offsetof(hcP2cArgs, {f})" for f in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "p2c/hc_trifocal_p2c.h"\n'
                   f'int main(void) {{ printf("{"%zu " * 5}\\n", sizeof(hcP2cArgs){args}); return 0; }}\n')
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_abi.hcP2cArgs)] + [getattr(_abi.hcP2cArgs, f).offset for f in fields] == [32, 0, 8, 16, 24]


# ---- 13. argument validation (nothing is launched: no device is needed) ------------------

def test_missing_p2c_pointers_are_rejected_before_any_device_work():
    from trifocal_pose_estimation_using_improved_gpuhc_amd import _abi
    L = _abi.lib()
    a = _abi.hcTrackArgs()
    a.sub_ransac_iters = 1
    a.settings = _abi.hcTrackSettings(80, 3, 4)
    for f in ("start_sols", "tracks", "converge", "infinity"):
        setattr(a, f, 0x1000)                    # never dereferenced
    ws, wsb = C.c_void_p(0x1000), L.hc_trifocal_workspace_size()
    full = dict(hx_index=0x1000, ht_index=0x1000, coeffs_hx=0x1000, coeffs_ht=0x1000)
    assert L.hc_trifocal_2op1p_30x30_track_p2c(C.byref(a), None, ws, wsb, None) == 1
    for missing in full:
        p = _abi.hcP2cArgs(**{k: (None if k == missing else v) for k, v in full.items()})
        assert L.hc_trifocal_2op1p_30x30_track_p2c(C.byref(a), C.byref(p), ws, wsb, None) == 1, missing
    p = _abi.hcP2cArgs(**full)
    assert L.hc_trifocal_2op1p_30x30_track_p2c(None, C.byref(p), ws, wsb, None) == 1
    assert L.hc_trifocal_2op1p_30x30_track_p2c(C.byref(a), C.byref(p), None, wsb, None) == 2      # HC_ERROR_WORKSPACE
    assert L.hc_trifocal_2op1p_30x30_track_p2c(C.byref(a), C.byref(p), ws, wsb - 1, None) == 2
    a.converge = None
    assert L.hc_trifocal_2op1p_30x30_track_p2c(C.byref(a), C.byref(p), ws, wsb, None) == 1
    one = np.zeros(8, np.int32)
    q = _abi.ptr(one)
    assert L.hc_trifocal_p2c_eval_batched(1, None, q, q, q, q, q, q, q, q, ws, wsb, None) == 1
    assert L.hc_trifocal_p2c_eval_batched(1, q, q, q, q, q, None, q, q, q, ws, wsb, None) == 1
    assert L.hc_trifocal_p2c_eval_batched(-1, q, q, q, q, q, q, q, q, q, ws, wsb, None) == 1
    assert L.hc_trifocal_p2c_eval_batched(1, q, q, q, q, q, q, q, q, q, None, wsb, None) == 2
